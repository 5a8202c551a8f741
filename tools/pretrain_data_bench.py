"""One pre-training SAP batch build at B = 32 on the GPU, by two routes, with the SAP step time of the same run beside them:
  native   etpnav_amd.pretrain_data.SapBatches.batch: records -> one pinned staging buffer -> one copy -> etp_traj_views +
           etp_traj_pair_dists; ends in a device synchronise
  host     the numpy restatement of the reference's get_input + sap_collate (tests/pretrain_data_ref.py) plus .to(device) of every
           tensor; ends in a device synchronise

    python tools/pretrain_data_bench.py [--out profiles/pretrain_data_bench.json] [--rounds 7] [--iters 20] [--kernel-stats DIR]
    rocprofv3 --kernel-trace --stats --output-format csv -d DIR -- python tools/pretrain_data_bench.py --native-only 50

The corpus is synthetic, of R2R proportions: 6 scans of 120 viewpoints (each tied to its 4 nearest neighbours), rows 768 + 128 wide,
paths of 4-7 steps, 256 annotations; every batch draws its 32 samples and end points anew, so both routes see a mix of cached and new
records, as an epoch does.  Same box, one process: the legs are warmed up and alternate within a round; a leg is timed with a host
clock over `iters` batches.  Reported per leg: the median over rounds of the per-batch mean, the lowest and the highest round.
--kernel-stats DIR (the output of the rocprofv3 run above, a run of its own) adds traj_views_kernel's mean time and the bytes it moves,
computed from the shapes of the batches of that run where its printed JSON line was saved as DIR/native_only.json, else of this run's."""
import argparse
import csv
import glob
import json
import math
import os
import statistics
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402
import torch  # noqa: E402

from etpnav_amd import pretrain_data as pdata  # noqa: E402
from etpnav_amd.features import FeatureStore, write_flat_pack  # noqa: E402

DEV = "cuda"
B, FI, FD = 32, 768, 128


def make_corpus(seed=0, scans=6, n=120, items=256):
    rng = np.random.default_rng(seed)
    conn, cands, annos, keys = {}, {}, [], []
    for s in range(scans):
        name = f"scan{s}"
        pts = np.concatenate([rng.uniform(0, 30, (n, 2)), rng.uniform(-1, 1, (n, 1))], 1)
        d = np.linalg.norm(pts[:, None] - pts[None], axis=2)
        adj = np.zeros((n, n), bool)
        for i in range(n):
            adj[i, np.argsort(d[i])[1:5]] = True
        adj |= adj.T
        ids = [f"{name}v{i}" for i in range(n)]
        data = []
        for i in range(n):
            pose = [0.0] * 16
            pose[3], pose[7], pose[11] = (float(x) for x in pts[i])
            data.append({"image_id": ids[i], "pose": pose, "included": True, "unobstructed": [bool(x) for x in adj[i]]})
        conn[name] = data
        for i in range(n):
            nav = {}
            for j in np.nonzero(adj[i])[0]:
                dx, dy, dz = pts[j] - pts[i]
                heading = math.atan2(dx, dy) % (2 * math.pi)
                hbin = int(round(heading / math.radians(30))) % 12
                nav[ids[j]] = [12 + hbin, float(d[i, j]), heading - hbin * math.radians(30), math.asin(dz / d[i, j])]
            cands[f"{name}_{ids[i]}"] = nav
            keys.append(f"{name}_{ids[i]}")
        for k in range(items // scans + 1):
            path = [int(rng.integers(n))]
            for _ in range(int(rng.integers(4, 8)) - 1):
                nxt = [j for j in np.nonzero(adj[path[-1]])[0] if j not in path]
                if not nxt:
                    break
                path.append(int(rng.choice(nxt)))
            annos.append({"instr_id": f"{name}_{k}", "scan": name, "heading": float(rng.uniform(0, 6.28)), "path": [ids[i] for i in path],
                          "instr_encoding": [101] + [int(x) for x in rng.integers(1996, 29611, int(rng.integers(20, 80)))] + [102]})
    img = rng.standard_normal((len(keys), 36, FI)).astype(np.float32)
    dep = rng.standard_normal((len(keys), 36, FD)).astype(np.float32)
    return {"connectivity": conn, "cands": cands, "annos": annos[:items], "keys": keys, "img": img, "dep": dep, "sizes": [FI, FD, 100]}


def draw(c, rng):
    out = []
    for i in rng.integers(0, len(c["annos"]), B):
        n = len(c["annos"][i]["path"])
        out.append((int(i), None) if rng.random() < 0.2 or n < 2 else (int(i), int(rng.integers(n - 1))))
    return out


def timed(fn, iters):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(iters):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / iters * 1e6


def views_bytes(batch):
    """what etp_traj_views moves for this batch: the live rows read once, every output element written once"""
    R, V, _ = batch["rgb_fts"].shape
    live = int(batch["view_lens"].sum())
    return live * (FI + FD + 4) * 4 + R * V * ((FI + FD + 4) * 4 + 8) + R * 12


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "pretrain_data_bench.json"))
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--native-only", type=int, default=0, help="build that many native batches and stop (the rocprofv3 run)")
    ap.add_argument("--kernel-stats", default=None)
    ap.add_argument("--no-step", action="store_true")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("tools/pretrain_data_bench.py measures on the GPU; there is none here")
    from tests import pretrain_data_ref as ref
    c = make_corpus()
    with tempfile.TemporaryDirectory() as td:
        write_flat_pack(os.path.join(td, "img.etpf"), zip(c["keys"], c["img"]))
        write_flat_pack(os.path.join(td, "dep.etpf"), zip(c["keys"], c["dep"]))
        store = FeatureStore(os.path.join(td, "img.etpf"), os.path.join(td, "dep.etpf")).to_device(DEV)
    c["graphs"] = pdata.NavGraphs.from_connectivity(c["connectivity"]).to_device(DEV)
    index = pdata.R2RTextPathIndex([c["annos"]], store, c["cands"], c["graphs"], FI, FD, 100)
    sap = pdata.SapBatches(index, B, np.random.default_rng(1), DEV)
    rng = np.random.default_rng(2)

    def native():
        out = sap.batch(draw(c, rng))
        torch.cuda.synchronize()
        return out

    def host():
        b = ref.sap_batch(draw(c, rng), c=c)
        out = {k: (torch.from_numpy(v).to(DEV) if k != "traj" else v) for k, v in b.items()}
        torch.cuda.synchronize()
        return out

    if a.native_only:
        moved = [views_bytes(native()) for _ in range(a.native_only)]
        sap.check()
        print(json.dumps({"native_batches": a.native_only, "traj_views_bytes_mean": statistics.mean(moved)}))
        return
    samples = draw(c, rng)
    got, want = sap.batch(samples), ref.sap_batch(samples, c=c)
    sap.check()
    assert ref.differing(got, want) == [], ref.differing(got, want)       # the two routes build the same batch, bit for bit
    legs = {"native": native, "host": host}
    for fn in legs.values():
        for _ in range(3):
            fn()
    per_round = {k: [] for k in legs}
    for _ in range(a.rounds):
        for k, fn in legs.items():
            per_round[k].append(timed(fn, a.iters))
    result = {"device": torch.cuda.get_device_name(0), "rounds": a.rounds, "iters": a.iters, "B": B,
              "unit": "us per SAP batch, host clock, from sample choices to the batch dict on the device, synchronised",
              "corpus": {"scans": 6, "viewpoints_per_scan": 120, "row_width": [FI, FD], "path_steps": "4-7", "annotations": len(c["annos"])},
              "batch_shape": {k: list(v.shape) for k, v in got.items() if k != "traj"}, "routes_bit_identical": True}
    for k, v in per_round.items():
        result[k] = {"median_us": round(statistics.median(v), 1), "min_us": round(min(v), 1), "max_us": round(max(v), 1)}
    result["speedup"] = round(result["host"]["median_us"] / result["native"]["median_us"], 2)
    result["host_copy_bytes"] = int(sum(v.numel() * v.element_size() for k, v in got.items() if k != "traj"))
    result["traj_views_bytes"] = views_bytes(got)
    if not a.no_step:
        from oracle import planner_oracle as po
        from etpnav_amd.planner import GlocalTextPathNavCMT
        from etpnav_amd.step import PlannerStep
        cfg = po.PlannerConfig.r2r(image_feat_size=FI, depth_feat_size=FD)
        model = GlocalTextPathNavCMT(cfg.to_dict(), dtype=torch.bfloat16, device=DEV)
        st = PlannerStep(model, got, dropout=None, zero_grads=True, grad_overwrite=False)
        for _ in range(3):
            st.run_eager()
        v = [timed(st.run_eager, a.iters) for _ in range(a.rounds)]
        result["sap_step"] = {"median_us": round(statistics.median(v), 1), "min_us": round(min(v), 1), "max_us": round(max(v), 1),
                              "dtype": "bf16", "note": "PlannerStep.run_eager on the batch above, randomly initialised full-size planner"}
        st.close()
    if a.kernel_stats:
        rows = []
        for path in glob.glob(os.path.join(a.kernel_stats, "**", "*kernel_stats.csv"), recursive=True):
            with open(path) as f:
                rows += [r for r in csv.DictReader(f) if "traj_views_kernel" in r.get("Name", "")]
        if not rows:
            raise SystemExit(f"no traj_views_kernel row under {a.kernel_stats}")
        ns = float(rows[0]["AverageNs"])
        result["traj_views_kernel"] = {"mean_us": round(ns / 1e3, 2), "calls": int(rows[0]["Calls"]),
                                       "source": "rocprofv3 --kernel-trace --stats, a run of its own (--native-only)"}
        summary = glob.glob(os.path.join(a.kernel_stats, "**", "native_only.json"), recursive=True)
        moved = json.load(open(summary[0]))["traj_views_bytes_mean"] if summary else result["traj_views_bytes"]
        result["traj_views_kernel"]["bytes_mean"] = moved
        result["traj_views_kernel"]["GB_per_s"] = round(moved / ns, 1)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")
    print(json.dumps(result))


if __name__ == "__main__":
    main()
