"""Write tests/golden/pretrain_batch_small.npz from the REAL reference data pipeline (needs the reference tree and networkx).

    python tools/make_golden_pretrain_batch.py --reference <root of the reference tree>

The reference's R2RTextPathData / SapDataset / MlmDataset / sap_collate / mlm_collate (pretrain_src/pretrain_src/data) run on a synthetic
corpus: 2 scans x 9 viewpoints on a jittered 3 x 3 grid (edge weights without ties -- asserted --, several candidates sharing one view
index, one viewpoint with a single neighbour), feature rows 24 / 8 wide with image_feat_size 16.  `jsonlines` and `h5py` are stubbed
with a few lines (the in-memory feature store is filled directly); everything else is the reference's own code.  The file holds data
only: the synthetic inputs (arrays and JSON strings), the recorded batches, and the uniforms that drove random_word.
"""
import argparse
import json
import math
import os
import random
import sys
import tempfile
import types
from types import SimpleNamespace

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
IMAGE_FEAT, DEPTH_FEAT, LD_IMG, LD_DEP, MAX_TXT = 16, 8, 24, 8, 16


def make_scan(name, seed):
    rng = np.random.default_rng(seed)
    pts = [(3.0 * (i % 3) + rng.uniform(-0.6, 0.6), 3.0 * (i // 3) + rng.uniform(-0.6, 0.6), rng.uniform(-0.4, 0.4)) for i in range(9)]
    edges = {(0, 1), (1, 2), (3, 4), (4, 5), (6, 7), (0, 3), (3, 6), (1, 4), (4, 7), (2, 5), (0, 4), (1, 3), (1, 5), (2, 4), (3, 7),
             (4, 6), (5, 8)}                                      # viewpoint 8 has the single neighbour 5
    ids = [f"{name}v{i}" for i in range(9)]
    conn = []
    for i in range(9):
        pose = [0.0] * 16
        pose[3], pose[7], pose[11] = pts[i]
        conn.append({"image_id": ids[i], "pose": pose, "included": True,
                     "unobstructed": [(min(i, j), max(i, j)) in edges for j in range(9)]})
    w = sorted(math.dist(pts[a], pts[b]) for a, b in edges)
    assert all(y - x > 1e-6 for x, y in zip(w, w[1:])), "edge weights tie"
    cands = {}
    for i in range(9):
        nav = {}
        for j in range(9):
            if (min(i, j), max(i, j)) not in edges:
                continue
            dx, dy, dz = (pts[j][k] - pts[i][k] for k in range(3))
            d = math.dist(pts[i], pts[j])
            heading = math.atan2(dx, dy) % (2 * math.pi)
            hbin = int(heading // (math.pi / 2)) * 3             # coarse on purpose: neighbours of one quadrant share a view index
            nav[ids[j]] = [12 + hbin, d, heading - hbin * math.radians(30), math.asin(dz / d)]
        cands[f"{name}_{ids[i]}"] = nav
    return ids, conn, cands, edges


def long_walk(ids, cands, scan, edges, seed):
    """24 viewpoints with revisits such that both truncation mutations show: path[19] is a neighbour of path[21] and of path[23], and
    looks at them under another view index than path[20] resp. path[22] does"""
    adj = {i: [j for j in range(9) if (min(i, j), max(i, j)) in edges] for i in range(9)}
    rng = np.random.default_rng(seed)
    view = lambda a, b: cands[f"{scan}_{ids[a]}"][ids[b]][0]
    for _ in range(100000):
        p = [int(rng.integers(9))]
        while len(p) < 24:
            p.append(int(rng.choice(adj[p[-1]])))
        if (p[21] in adj[p[19]] and p[23] in adj[p[19]] and view(p[19], p[21]) != view(p[20], p[21])
                and view(p[19], p[23]) != view(p[22], p[23]) and p[22] != p[20]):
            return [ids[i] for i in p]
    raise RuntimeError("no such walk")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reference", required=True)
    ap.add_argument("--out", default=os.path.join(ROOT, "tests", "golden", "pretrain_batch_small.npz"))
    a = ap.parse_args()

    # ---- the synthetic corpus ----
    scans, conn, cands, idsof, edgesof = ["scanA", "scanB"], {}, {}, {}, {}
    for k, s in enumerate(scans):
        idsof[s], conn[s], c, edgesof[s] = make_scan(s, 11 + k)
        cands.update(c)
    shared = [k for k, nav in cands.items() if len({v[0] for v in nav.values()}) < len(nav)]
    assert len(shared) >= 3 and any(len(nav) == 1 for nav in cands.values())
    keys = [f"{s}_{v}" for s in scans for v in idsof[s]]
    n = len(keys)
    # small integers: exact in fp32, every (row, view, column) distinct, and the file compresses
    img = (np.arange(n * 36 * LD_IMG, dtype=np.float32).reshape(n, 36, LD_IMG) % 4099) - 2048
    dep = (np.arange(n * 36 * LD_DEP, dtype=np.float32).reshape(n, 36, LD_DEP) % 1021) * 0.5 - 200
    rng = np.random.default_rng(5)
    A, B = idsof["scanA"], idsof["scanB"]
    enc = lambda m: [101] + [int(x) for x in rng.integers(1996, 29611, m)] + [102]
    annos = [
        {"instr_id": "a0", "scan": "scanA", "heading": 0.7, "path": [A[0], A[1], A[4], A[7]], "instr_encoding": enc(7)},
        {"instr_id": "b1", "scan": "scanB", "heading": 2.1, "path": [B[6], B[3], B[4], B[5], B[8]], "instr_encoding": enc(10)},
        {"instr_id": "a2", "scan": "scanA", "heading": 4.0, "path": [A[8]], "instr_encoding": enc(3)},
        {"instr_id": "b3", "scan": "scanB", "heading": 0.0, "path": long_walk(B, cands, "scanB", edgesof["scanB"], 3),
         "instr_encoding": enc(20)},                               # longer than max_txt_len
        {"instr_id": "a4", "scan": "scanA", "heading": 5.5, "path": [A[2], A[4], A[3], A[1], A[5], A[8]], "instr_encoding": enc(5)},
    ]
    # (item, end index or None = 'pos' without end_vp, how the reference is called)
    samples = [(0, 1, "end_vp"), (0, 3, "end_vp"), (2, None, "pos"), (3, None, "pos"), (3, 21, "randint"), (1, 2, "end_vp"),
               (4, 5, "end_vp"), (4, 0, "end_vp")]

    # ---- the reference, with two stubs ----
    jl = types.ModuleType("jsonlines")

    class _Reader:
        def __init__(self, path):
            self.f = open(path)

        def __enter__(self):
            return (json.loads(x) for x in self.f if x.strip())

        def __exit__(self, *e):
            self.f.close()

    jl.open = lambda path, mode="r": _Reader(path)
    sys.modules["jsonlines"] = jl
    sys.modules["h5py"] = types.ModuleType("h5py")
    sys.path.insert(0, os.path.join(a.reference, "pretrain_src", "pretrain_src"))
    from data import dataset as rd, tasks as rt          # noqa: E402

    rec = {}
    with tempfile.TemporaryDirectory() as td:
        with open(os.path.join(td, "scans.txt"), "w") as f:
            f.write("\n".join(scans) + "\n")
        for s in scans:
            json.dump(conn[s], open(os.path.join(td, f"{s}_connectivity.json"), "w"))
        json.dump(cands, open(os.path.join(td, "cands.json"), "w"))
        with open(os.path.join(td, "anno.jsonl"), "w") as f:
            for x in annos:
                f.write(json.dumps(x) + "\n")
        dbs = {}
        for flag in (False, True):
            db = rd.R2RTextPathData([os.path.join(td, "anno.jsonl")], None, None, os.path.join(td, "cands.json"), td,
                                    image_feat_size=IMAGE_FEAT, depth_feat_size=DEPTH_FEAT, max_txt_len=MAX_TXT, in_memory=True,
                                    act_visited_node=flag)
            for i, k in enumerate(keys):
                db._feature_store[k], db._feature_store_depth[k] = img[i], dep[i]
            dbs[flag] = db
    db = dbs[False]
    for s in scans:                                      # load_nav_graphs' own distances and hop counts, in its node order
        nodes = list(db.graphs[s].nodes.keys())
        rec[f"nav_{s}_nodes"] = json.dumps(nodes)
        rec[f"nav_{s}_dist"] = np.array([[db.shortest_distances[s][x][y] for y in nodes] for x in nodes], dtype=np.float64)
        rec[f"nav_{s}_hops"] = np.array([[len(db.shortest_paths[s][x][y]) - 1 for y in nodes] for x in nodes], dtype=np.int32)
        rec[f"nav_{s}_pos"] = np.stack([db.graphs[s].nodes[x]["position"] for x in nodes])

    class Forced:
        """SapDataset's nav_db: dataset index k -> samples[k], through the REAL get_input"""

        def __init__(self, real):
            self.real, self.data = real, samples

        def get_input(self, k, end_vp_type, return_act_label=False):
            i, e, how = samples[k]
            if how == "end_vp":
                return self.real.get_input(i, end_vp_type, return_act_label=return_act_label, end_vp=annos[i]["path"][e])
            if how == "pos":
                return self.real.get_input(i, "pos", return_act_label=return_act_label)
            old = np.random.randint
            np.random.randint = lambda m: e
            try:
                return self.real.get_input(i, "neg_in_gt_path", return_act_label=return_act_label)
            finally:
                np.random.randint = old

    tok = SimpleNamespace(cls_token_id=101, sep_token_id=102, mask_token_id=103, pad_token_id=0)
    TENSORS = ["txt_ids", "txt_lens", "traj_vp_view_lens", "traj_view_img_fts", "traj_view_dep_fts", "traj_loc_fts", "traj_nav_types",
               "gmap_lens", "gmap_step_ids", "gmap_visited_masks", "gmap_pos_fts", "gmap_pair_dists"]
    LISTS = ["traj_step_lens", "traj_cand_vpids", "traj_vpids", "gmap_vpids"]

    def put(prefix, batch, extra=()):
        for k in TENSORS + list(extra):
            rec[f"{prefix}_{k}"] = batch[k].numpy()
        rec[f"{prefix}_lists"] = json.dumps({k: batch[k] for k in LISTS})

    sap = {flag: rt.SapDataset(Forced(dbs[flag]), tok) for flag in (False, True)}
    full = {flag: rt.sap_collate([sap[flag][k] for k in range(len(samples))]) for flag in (False, True)}
    put("sap_all", full[False], ("local_act_labels", "global_act_labels"))
    for k in TENSORS:                                    # act_visited_node changes the visited masks and nothing else
        same = bool((full[True][k] == full[False][k]).all())
        assert same == (k != "gmap_visited_masks"), k
    rec["sap_all_gmap_visited_masks_act"] = full[True]["gmap_visited_masks"].numpy()
    put("sap_two", rt.sap_collate([sap[False][k] for k in (0, 5)]), ("local_act_labels", "global_act_labels"))
    labels = full[False]["global_act_labels"].tolist()
    assert labels[1] == 0 and labels[2] == 0 and max(int(x) for x in full[False]["traj_vp_view_lens"]) > 36, labels
    assert len(full[False]["traj_vpids"][3]) == 21 and len(full[False]["traj_vpids"][4]) == 21

    # ---- MLM: random_word driven by recorded uniforms ----
    mlm_items = [0, 1, 2, 3, 4]
    urng = np.random.default_rng(9)
    mlm = rt.MlmDataset(db, tok)
    outs = []
    for i in mlm_items:
        m = len(annos[i]["instr_encoding"][:MAX_TXT])
        u, u2 = urng.random(m), urng.random(m)
        if i == 2:
            u = 0.2 + 0.8 * u                           # nothing drawn: "at least mask 1"
        if i == 1:
            u[:4] = [0.01, 0.125, 0.14, 0.149]           # mask, random word, keep, keep
        calls = {"n": 0}

        def rnd():
            calls["n"] += 1
            return float(u[calls["n"] - 1])

        old = random.random, random.choice
        random.random, random.choice = rnd, (lambda seq: seq[int(u2[calls["n"] - 1] * len(seq))])
        try:
            outs.append(mlm[i])
        finally:
            random.random, random.choice = old
        rec[f"mlm_u_{i}"], rec[f"mlm_u2_{i}"] = u, u2
    put("mlm_all", rt.mlm_collate(outs), ("txt_labels",))

    rec.update({"scans": json.dumps(scans), "connectivity": json.dumps(conn), "scanvp_cands": json.dumps(cands),
                "annotations": json.dumps(annos), "samples": json.dumps([[i, e] for i, e, _ in samples]),
                "mlm_items": json.dumps(mlm_items), "store_keys": json.dumps(keys), "store_img": img, "store_dep": dep,
                "sizes": np.array([IMAGE_FEAT, DEPTH_FEAT, MAX_TXT], dtype=np.int64),
                "numpy_version": np.array(np.__version__)})
    np.savez_compressed(a.out, **rec)
    print(a.out, os.path.getsize(a.out), "bytes")


if __name__ == "__main__":
    main()
