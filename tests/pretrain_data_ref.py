"""numpy restatement of the pre-training data path (etpnav_amd/pretrain_data.py, csrc/traj_batch.hip), its fixture, its comparator and
the mutations that comparator must reject.

    traj_views(...) / pair_dists(...)      the two kernels, output for output (status words included; `fill` = what a guarded buffer holds)
    get_input(corpus, idx, end_idx, ...)   R2RTextPathData.get_input (pretrain_src/pretrain_src/data/dataset.py:408-526) in the reference's own
                                           per-sample shape: dict / loop based, independent of the host layer's compact records
    collate(outs) / to_batch(...)          sap_collate / mlm_collate (tasks.py:98-138, 322-364) -> this repository's batch dict
    expected(prefix)                       the recording of the REAL classes (tests/golden/pretrain_batch_small.npz,
                                           tools/make_golden_pretrain_batch.py) in the same layout
    differing(got, want)                   the comparator: keys whose shape, dtype or BYTES differ, lists that are not equal

tests/test_pretrain_data_ref_cpu.py pins this file and the host layer to the recording; tests/test_pretrain_data_gpu.py holds the kernels to
traj_views / pair_dists and the native loaders to expected().
"""
import atexit
import functools
import json
import math
import os
import shutil
import tempfile

import numpy as np

from etpnav_amd import pretrain_data as pdata
from etpnav_amd.features import FeatureStore, write_flat_pack

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "pretrain_batch_small.npz")
MUTATIONS = ["free_reversed", "shared_freed_twice", "cands_after_free", "slice_dropped", "base_view_0", "div30_f32", "nonzero_diag",
             "cur_angle_after_trunc", "label_truncated_idx"]
ERR_COUNT, ERR_VIEW, ERR_ROW, ERR_VIEWS = 1, 2, 4, 8
ERR_LEN, ERR_SCAN, ERR_INDEX = 1, 2, 4


# ---- the kernels -------------------------------------------------------------------------------------------------------------------
def traj_views(img, dep, pano_row, count, view, cand_loc, tab, V, Fimg, Fdep, fill=None):
    """etp_traj_views.  fill: None = fresh zeros, else {name: array} of what the output buffers hold before the call (flagged steps keep it)"""
    R, Kmax = view.shape
    N, P = img.shape[:2]
    out = {"rgb_fts": np.zeros((R, V, Fimg), np.float32), "loc_fts": np.zeros((R, V, 4), np.float32), "nav_types": np.zeros((R, V), np.int64),
           "view_lens": np.zeros(R, np.int64), "status": np.zeros(R, np.int32)}
    if dep is not None:
        out["dep_fts"] = np.zeros((R, V, Fdep), np.float32)
    if fill is not None:
        out = {k: np.array(fill[k], copy=True) for k in out}
    for r in range(R):
        k, err, used = int(count[r]), 0, []
        if k < 0 or k > Kmax:
            err |= ERR_COUNT
        if pano_row[r] < 0 or pano_row[r] >= N:
            err |= ERR_ROW
        if not err & ERR_COUNT:
            used = [int(x) for x in view[r, :k]]
            if any(x < 0 or x >= P for x in used):
                err |= ERR_VIEW
            length = k + P - len({x for x in used if 0 <= x < P})
            if length > V:
                err |= ERR_VIEWS
        out["status"][r] = err
        if err:
            continue
        order = used + [i for i in range(P) if i not in set(used)]
        out["view_lens"][r] = length
        out["rgb_fts"][r] = 0
        out["rgb_fts"][r, :length] = img[pano_row[r], order, :Fimg]
        if dep is not None:
            out["dep_fts"][r] = 0
            out["dep_fts"][r, :length] = dep[pano_row[r], order, :Fdep]
        out["loc_fts"][r] = 0
        out["loc_fts"][r, :k] = cand_loc[r, :k]
        out["loc_fts"][r, k:length] = tab[order[k:]]
        out["nav_types"][r] = 0
        out["nav_types"][r, :k] = 1
    return out


def pair_dists(dist_tab, scan_off, scan_n, gmap_idx, gmap_len, fill=None):
    """etp_traj_pair_dists: directional lookup, one double division rounded once, written to both triangles"""
    B, G = gmap_idx.shape
    out = {"gmap_pair_dists": np.zeros((B, G, G), np.float32), "gmap_masks": np.zeros((B, G), np.uint8), "status": np.zeros(B, np.int32)}
    if fill is not None:
        out = {k: np.array(fill[k], copy=True) for k in out}
    for b in range(B):
        n, off, ln = int(scan_n[b]), int(scan_off[b]), int(gmap_len[b])
        err = ERR_LEN if ln < 1 or ln > G else 0
        if n < 1 or off < 0 or off > dist_tab.size or n * n > dist_tab.size - off:
            err |= ERR_SCAN
        if not err and any(x < 0 or x >= n for x in gmap_idx[b, 1:ln]):
            err = ERR_INDEX
        out["status"][b] = err
        if err:
            continue
        d = dist_tab[off:off + n * n].reshape(n, n)
        out["gmap_pair_dists"][b] = 0
        out["gmap_masks"][b] = np.arange(G) < ln
        for i in range(1, ln):
            for j in range(i + 1, ln):
                out["gmap_pair_dists"][b, i, j] = out["gmap_pair_dists"][b, j, i] = np.float32(d[gmap_idx[b, i], gmap_idx[b, j]] / 30.0)
    return out


# ---- the fixture -------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def fixture():
    z = np.load(GOLDEN)
    return {k: z[k] for k in z.files}


def js(name):
    return json.loads(str(fixture()[name]))


@functools.lru_cache(maxsize=None)
def corpus():
    """the synthetic inputs of the recording as the host layer takes them: NavGraphs, a FeatureStore over a flat pack, the lists"""
    f = fixture()
    graphs = pdata.NavGraphs.from_connectivity(js("connectivity"))
    td = tempfile.mkdtemp(prefix="pretrain_batch_")
    atexit.register(shutil.rmtree, td, ignore_errors=True)       # the flat packs are memory-mapped for the life of the process
    keys = js("store_keys")
    write_flat_pack(os.path.join(td, "img.etpf"), zip(keys, f["store_img"]))
    write_flat_pack(os.path.join(td, "dep.etpf"), zip(keys, f["store_dep"]))
    store = FeatureStore(os.path.join(td, "img.etpf"), os.path.join(td, "dep.etpf"))
    return {"graphs": graphs, "store": store, "cands": js("scanvp_cands"), "annos": js("annotations"), "keys": keys,
            "img": f["store_img"], "dep": f["store_dep"], "sizes": [int(x) for x in f["sizes"]]}


def make_index(act_visited_node=False, store=None, graphs=None):
    c = corpus()
    Fi, Fd, T = c["sizes"]
    return pdata.R2RTextPathIndex([c["annos"]], store or c["store"], c["cands"], graphs or c["graphs"], image_feat_size=Fi,
                                  depth_feat_size=Fd, max_txt_len=T, act_visited_node=act_visited_node)


def expected(prefix, visited_act=False):
    """the recorded collate output as this repository's batch dict (numpy)"""
    f = fixture()
    g = lambda k: f[f"{prefix}_{k}"]
    L, G = g("txt_ids").shape[1], g("gmap_step_ids").shape[1]
    lists = js(f"{prefix}_lists")
    out = {"rgb_fts": g("traj_view_img_fts"), "dep_fts": g("traj_view_dep_fts"), "loc_fts": g("traj_loc_fts"), "nav_types": g("traj_nav_types"),
           "view_lens": g("traj_vp_view_lens"), "txt_ids": g("txt_ids"), "txt_masks": np.arange(L)[None] < g("txt_lens")[:, None],
           "gmap_step_ids": g("gmap_step_ids"), "gmap_pos_fts": g("gmap_pos_fts"), "gmap_masks": np.arange(G)[None] < g("gmap_lens")[:, None],
           "gmap_visited_masks": f[f"{prefix}_gmap_visited_masks_act"] if visited_act else g("gmap_visited_masks"),
           "gmap_pair_dists": g("gmap_pair_dists"),
           "traj": {"traj_step_lens": lists["traj_step_lens"], "traj_vpids": lists["traj_vpids"], "traj_cand_vpids": lists["traj_cand_vpids"],
                    "gmap_vpids": lists["gmap_vpids"],
                    "traj_vp_lens": np.split(g("traj_vp_view_lens"), np.cumsum(lists["traj_step_lens"])[:-1])}}
    out["traj"]["traj_vp_lens"] = [[int(x) for x in v] for v in out["traj"]["traj_vp_lens"]]
    if f"{prefix}_global_act_labels" in f:
        out["labels"] = g("global_act_labels")
    if f"{prefix}_txt_labels" in f:
        out["txt_labels"] = g("txt_labels")
    return out


def differing(got, want, keys=None):
    """keys of `want` (or `keys`) that `got` does not reproduce bit for bit (tensors: shape, dtype and bytes; 'traj': list equality)"""
    bad = []
    for k in (keys or want):
        if k == "traj":
            bad += [f"traj.{n}" for n, v in want[k].items() if k not in got or got[k].get(n) != v]
            continue
        a, b = got.get(k), want[k]
        a = None if a is None else np.asarray(a.cpu() if hasattr(a, "cpu") else a)
        if a is None or a.shape != b.shape or a.dtype != b.dtype or a.tobytes() != np.ascontiguousarray(b).tobytes():
            bad.append(k)
    return bad


# ---- get_input / collate, the reference's shape ------------------------------------------------------------------------------------
def get_input(idx, end_idx, act_visited_node=False, mutate=None, c=None):
    c = corpus() if c is None else c
    Fi, Fd, T = c["sizes"]
    g, cands, item = c["graphs"], c["cands"], c["annos"][idx]
    scan, full = item["scan"], item["path"]
    end_idx = len(full) - 1 if end_idx is None else end_idx
    end_vp = full[end_idx]
    sg = g.scans[scan]
    row = {k: i for i, k in enumerate(c["keys"])}
    base = pdata.view_rel_angles(0 if mutate == "base_view_0" else 12)

    def cur_angle(path):
        if len(path) < 2:
            return item["heading"], 0
        v = cands[f"{scan}_{path[-2]}"][path[-1]][0]
        return (v % 12) * math.radians(30), (v // 12 - 1) * math.radians(30)

    path = full[:end_idx + 1]
    heading, elevation = cur_angle(path)
    if len(path) > pdata.TRAIN_MAX_STEP:
        path = path[:pdata.TRAIN_MAX_STEP] + [end_vp]
    if mutate == "cur_angle_after_trunc":
        heading, elevation = cur_angle(path)
    out = {"txt": item["instr_encoding"][:T], "img": [], "dep": [], "loc": [], "nav": [], "cand_vpids": [], "vpids": path}
    for vp in path:
        nav = cands[f"{scan}_{vp}"]
        vimg, vdep = c["img"][row[f"{scan}_{vp}"]], c["dep"][row[f"{scan}_{vp}"]]
        used, order, angles = [], [], []
        for k, v in nav.items():
            used.append(v[0])
            order.append(v[0])
            angles.append([np.float32(base[v[0]][0]) + np.float32(v[2]), np.float32(base[v[0]][1]) + np.float32(v[3])])
        free = [i for i in range(36) if i not in set(used)]
        if mutate == "free_reversed":
            free = free[::-1]
        if mutate == "shared_freed_twice":
            free = free[:36 - len(used)]
        ncand = len(used)
        order, angles = order + free, angles + [base[i] for i in free]
        nav_types = [1] * ncand + [0] * len(free)
        if mutate == "cands_after_free":
            order, angles, nav_types = order[ncand:] + order[:ncand], angles[ncand:] + angles[:ncand], nav_types[ncand:] + nav_types[:ncand]
        ang = np.stack([np.asarray(x, dtype=np.float32) for x in angles], 0)
        out["img"].append(vimg[order] if mutate == "slice_dropped" else vimg[order][:, :Fi])
        out["dep"].append(vdep[order][:, :Fd])
        out["loc"].append(pdata.angle_fts(ang[:, 0], ang[:, 1]))
        out["nav"].append(nav_types)
        out["cand_vpids"].append(list(nav.keys()))
    visited, unvisited = {}, {}
    for t, vp in enumerate(path):
        visited[vp] = t + 1
        if vp in unvisited:
            del unvisited[vp]
        for nxt in cands[f"{scan}_{vp}"].keys():
            if nxt not in visited:
                unvisited[nxt] = 0
    vpids = [None] + list(visited.keys()) + list(unvisited.keys())
    out["gmap_vpids"] = vpids
    out["gmap_step_ids"] = [0] + list(visited.values()) + list(unvisited.values())
    out["gmap_visited_masks"] = ([0] + [1 if vp == path[-1] else 0 for vp in vpids[1:]]) if act_visited_node else \
        ([0] + [1] * len(visited) + [0] * len(unvisited))
    ix, cur = sg["index"], sg["index"][path[-1]]
    a = sg["pos"][cur]
    ang, dis = [], []
    for vp in vpids:
        if vp is None:
            ang.append([0, 0])
            dis.append([0, 0, 0])
            continue
        b = sg["pos"][ix[vp]]
        dx, dy, dz = b[0] - a[0], b[1] - a[1], b[2] - a[2]
        xy = max(np.sqrt(dx ** 2 + dy ** 2), 1e-8)
        xyz = max(np.sqrt(dx ** 2 + dy ** 2 + dz ** 2), 1e-8)
        h = np.arcsin(dx / xy)
        if b[1] < a[1]:
            h = np.pi - h
        h -= heading
        e = np.arcsin(dz / xyz)
        e -= elevation
        ang.append([h, e])
        dis.append([xyz / 30, sg["dist"][cur, ix[vp]] / 30, int(sg["hops"][cur, ix[vp]]) / 10])
    ang, dis = np.array(ang).astype(np.float32), np.array(dis).astype(np.float32)
    out["gmap_pos_fts"] = np.concatenate([pdata.angle_fts(ang[:, 0], ang[:, 1]), dis], 1)
    n = len(vpids)
    pd_ = np.zeros((n, n), dtype=np.float32)
    for i in range(1, n):
        for j in range(i + (0 if mutate == "nonzero_diag" else 1), n):
            d = sg["dist"][ix[vpids[i]], ix[vpids[j]]]
            d = d + 1.0 if i == j else d
            pd_[i, j] = pd_[j, i] = (np.float32(d) / np.float32(30)) if mutate == "div30_f32" else d / 30
    out["gmap_pair_dists"] = pd_
    if end_vp == full[-1]:
        out["label"] = 0
    else:
        nxt = full[(min(end_idx, pdata.TRAIN_MAX_STEP) if mutate == "label_truncated_idx" else end_idx) + 1]
        out["label"] = vpids.index(nxt) if nxt in vpids else -100
    return out


def collate(outs, txt=None, txt_labels=None):
    """sap_collate / mlm_collate -> the batch dict; txt / txt_labels: per-sample masked ids and labels (MLM)"""
    B = len(outs)
    txt = [np.asarray(o["txt"], dtype=np.int64) for o in outs] if txt is None else txt
    steps = [x for o in outs for x in o["img"]]
    R, V = len(steps), max(len(x) for x in steps)
    L, G = max(len(t) for t in txt), max(len(o["gmap_vpids"]) for o in outs)
    b = {"rgb_fts": np.zeros((R, V, steps[0].shape[1]), np.float32), "dep_fts": np.zeros((R, V, outs[0]["dep"][0].shape[1]), np.float32),
         "loc_fts": np.zeros((R, V, 4), np.float32), "nav_types": np.zeros((R, V), np.int64), "view_lens": np.zeros(R, np.int64),
         "txt_ids": np.zeros((B, L), np.int64), "txt_masks": np.zeros((B, L), np.bool_), "gmap_step_ids": np.zeros((B, G), np.int64),
         "gmap_pos_fts": np.zeros((B, G, 7), np.float32), "gmap_masks": np.zeros((B, G), np.bool_),
         "gmap_visited_masks": np.zeros((B, G), np.bool_), "gmap_pair_dists": np.zeros((B, G, G), np.float32),
         "labels": np.array([o["label"] for o in outs], dtype=np.int64)}
    r = 0
    for o in outs:
        for t in range(len(o["img"])):
            n = len(o["img"][t])
            if o["img"][t].shape[1] != b["rgb_fts"].shape[2]:
                raise ValueError("feature width differs")
            b["rgb_fts"][r, :n], b["dep_fts"][r, :n], b["loc_fts"][r, :n] = o["img"][t], o["dep"][t], o["loc"][t]
            b["nav_types"][r, :n] = o["nav"][t]
            b["view_lens"][r] = n
            r += 1
    for i, o in enumerate(outs):
        g = len(o["gmap_vpids"])
        b["txt_ids"][i, :len(txt[i])] = txt[i]
        b["txt_masks"][i, :len(txt[i])] = True
        b["gmap_step_ids"][i, :g], b["gmap_pos_fts"][i, :g], b["gmap_masks"][i, :g] = o["gmap_step_ids"], o["gmap_pos_fts"], True
        b["gmap_visited_masks"][i, :g] = o["gmap_visited_masks"]
        b["gmap_pair_dists"][i, :g, :g] = o["gmap_pair_dists"]
    if txt_labels is not None:
        b["txt_labels"] = np.full((B, L), -1, np.int64)
        for i, t in enumerate(txt_labels):
            b["txt_labels"][i, :len(t)] = t
    b["traj"] = {"traj_step_lens": [len(o["img"]) for o in outs], "traj_vp_lens": [[len(x) for x in o["img"]] for o in outs],
                 "traj_vpids": [o["vpids"] for o in outs], "traj_cand_vpids": [o["cand_vpids"] for o in outs],
                 "gmap_vpids": [o["gmap_vpids"] for o in outs]}
    return b


def sap_batch(samples, act_visited_node=False, mutate=None, c=None):
    """c: another corpus than the fixture's ({graphs, cands, annos, keys, img, dep, sizes}; tools/pretrain_data_bench.py)"""
    return collate([get_input(i, e, act_visited_node, mutate, c) for i, e in samples])


def mlm_batch(items, uniforms):
    outs = [get_input(i, None) for i in items]
    masked = [pdata.mask_tokens(o["txt"], u, u2=u2) for o, (u, u2) in zip(outs, uniforms)]
    return collate(outs, [m[0] for m in masked], [m[1] for m in masked])


def mlm_uniforms():
    f = fixture()
    return [(f[f"mlm_u_{i}"], f[f"mlm_u2_{i}"]) for i in js("mlm_items")]


# ---- the host layer without a GPU: records -> staging arrays -> the kernels' restatement -------------------------------------------
def host_layer_batch(index, recs, txt, labels, txt_labels=None):
    """what _Batches.assemble computes, with traj_views / pair_dists standing in for the two launches"""
    c = corpus()
    R = sum(len(r["rows"]) for r in recs)
    Kmax = max(1, max(len(v) for r in recs for v, _ in r["tables"]))
    V = max(n for r in recs for n in r["view_lens"])
    G = max(len(r["gmap_vpids"]) for r in recs)
    count, view, loc = np.zeros(R, np.int32), np.zeros((R, Kmax), np.int32), np.zeros((R, Kmax, 4), np.float32)
    rows = np.concatenate([r["rows"] for r in recs])
    k = 0
    for r in recs:
        for v, l in r["tables"]:
            count[k], view[k, :len(v)], loc[k, :len(v)] = len(v), v, l
            k += 1
    out = traj_views(c["img"], c["dep"], rows, count, view, loc, index.view_loc_tab, V, index.image_feat_size, index.depth_feat_size)
    gi = np.zeros((len(recs), G), np.int32)
    for b, r in enumerate(recs):
        gi[b, :len(r["gmap_idx"])] = r["gmap_idx"]
    flat = np.concatenate([g["dist"].reshape(-1) for g in index.graphs.scans.values()])
    pd_ = pair_dists(flat, np.array([index.graphs.offset[r["scan"]] for r in recs]), np.array([len(index.graphs.scans[r["scan"]]["vps"]) for r in recs]),
                     gi, np.array([len(r["gmap_vpids"]) for r in recs]))
    assert not out.pop("status").any() and not pd_.pop("status").any()
    outs = [{"txt": t, "img": [None] * len(r["rows"]), "gmap_vpids": r["gmap_vpids"]} for r, t in zip(recs, txt)]
    B, L = len(recs), max(len(t) for t in txt)
    b = dict(out)
    b.update({"gmap_pair_dists": pd_["gmap_pair_dists"], "gmap_masks": pd_["gmap_masks"].astype(np.bool_),
              "txt_ids": np.zeros((B, L), np.int64), "txt_masks": np.zeros((B, L), np.bool_), "gmap_step_ids": np.zeros((B, G), np.int64),
              "gmap_pos_fts": np.zeros((B, G, 7), np.float32), "gmap_visited_masks": np.zeros((B, G), np.bool_),
              "labels": np.asarray(labels, dtype=np.int64)})
    for i, r in enumerate(recs):
        g = len(r["gmap_vpids"])
        b["txt_ids"][i, :len(txt[i])], b["txt_masks"][i, :len(txt[i])] = txt[i], True
        b["gmap_step_ids"][i, :g], b["gmap_pos_fts"][i, :g], b["gmap_visited_masks"][i, :g] = r["gmap_step_ids"], r["gmap_pos_fts"], r["gmap_visited_masks"]
    if txt_labels is not None:
        b["txt_labels"] = np.full((B, L), -1, np.int64)
        for i, t in enumerate(txt_labels):
            b["txt_labels"][i, :len(t)] = t
    b["traj"] = {"traj_step_lens": [len(r["rows"]) for r in recs], "traj_vp_lens": [list(r["view_lens"]) for r in recs],
                 "traj_vpids": [r["traj_vpids"] for r in recs], "traj_cand_vpids": [r["traj_cand_vpids"] for r in recs],
                 "gmap_vpids": [r["gmap_vpids"] for r in recs]}
    del outs
    return b
