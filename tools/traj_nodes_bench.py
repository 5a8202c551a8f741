"""One pre-training SAP step at B = 32 fed by the native loaders, by the two routes of the node aggregation, in one process:
  csr      PlannerStep(traj_nodes=False): load_batch runs graph_inputs.pack_traj_csr on the batch's string lists (Python), makes six
           torch.tensor conversions and six host-to-device copies; the step calls etp_gather_sum twice
  tables   PlannerStep (default for a loader's TrajBatch): load_batch takes the batch's descriptor tensors by reference; the step calls
           etp_traj_nodes_fwd / etp_traj_nodes_bwd (csrc/traj_batch.hip)

    python tools/traj_nodes_bench.py [--out profiles/traj_nodes_bench.json] [--rounds 7] [--iters 20] [--kernel-stats DIR]
    rocprofv3 --kernel-trace --stats --output-format csv -d DIR -- python tools/traj_nodes_bench.py --profile 30

The corpus is tools/pretrain_data_bench.py's (synthetic, of R2R proportions); one draw of 32 samples is built into a small pool of
batches of one shape, so that the step can load_batch them in turn.  Both legs run on ONE step object whose route is switched between
rounds (`step.traj_nodes`), hence on the same streams.  (With one step object per route, the object created second ran its
iterations in 13.9 ms against 5.8 ms for the first -- about the serial sum of its kernels' times; on one object both routes' device
side takes 5.7-5.9 ms.  Supposed cause, not examined: how the second object's side streams map to hardware queues.)  Per iteration: load_batch + run_eager + device synchronise, host
clock.  The two legs are warmed up and alternate in rounds of `iters` iterations; reported per leg are the median over rounds of the
per-iteration mean, the lowest and the highest round, and the same for the host time spent inside load_batch alone (it enqueues copies
and does not synchronise) and for the rest (issue + device step + synchronise).  `tables_lower_in_every_pair` says whether the tables'
round was the faster one in every pair of neighbouring rounds: the condition for the route to be the default.
--profile N runs N iterations of each leg and stops (the rocprofv3 run, a run of its own); --kernel-stats DIR adds the kernels' own
times from that run's CSV."""
import argparse
import csv
import glob
import importlib.util
import json
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
KERNELS = ("traj_nodes_fwd_kernel", "traj_nodes_bwd_kernel", "gather_sum_kernel")


def _corpus_tool():
    spec = importlib.util.spec_from_file_location("pretrain_data_bench", os.path.join(ROOT, "tools", "pretrain_data_bench.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def leg(step, pool, iters, tables):
    """-> (us per iteration, us per iteration inside load_batch, us per iteration for the rest)"""
    step.traj_nodes = tables                                      # read by load_batch and by both node-assembly calls
    torch.cuda.synchronize()
    t_load = 0.0
    t0 = time.perf_counter()
    for i in range(iters):
        a = time.perf_counter()
        step.load_batch(pool[i % len(pool)])
        t_load += time.perf_counter() - a
        step.run_eager()
        torch.cuda.synchronize()
    total = time.perf_counter() - t0
    return total / iters * 1e6, t_load / iters * 1e6, (total - t_load) / iters * 1e6


def summary(v):
    return {"median_us": round(statistics.median(v), 1), "min_us": round(min(v), 1), "max_us": round(max(v), 1)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "traj_nodes_bench.json"))
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--profile", type=int, default=0, help="run that many iterations of each leg and stop (the rocprofv3 run)")
    ap.add_argument("--kernel-stats", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("tools/traj_nodes_bench.py measures on the GPU; there is none here")
    from oracle import planner_oracle as po
    from etpnav_amd.planner import GlocalTextPathNavCMT
    from etpnav_amd.step import PlannerStep
    tool = _corpus_tool()
    B, FI, FD = tool.B, tool.FI, tool.FD
    c = tool.make_corpus()
    with tempfile.TemporaryDirectory() as td:
        write_flat_pack(os.path.join(td, "img.etpf"), zip(c["keys"], c["img"]))
        write_flat_pack(os.path.join(td, "dep.etpf"), zip(c["keys"], c["dep"]))
        store = FeatureStore(os.path.join(td, "img.etpf"), os.path.join(td, "dep.etpf")).to_device(DEV)
    graphs = pdata.NavGraphs.from_connectivity(c["connectivity"]).to_device(DEV)
    index = pdata.R2RTextPathIndex([c["annos"]], store, c["cands"], graphs, FI, FD, 100)
    sap = pdata.SapBatches(index, B, np.random.default_rng(1), DEV)
    samples = tool.draw(c, np.random.default_rng(2))
    pool = [sap.batch(samples) for _ in range(4)]
    sap.check()
    cfg = po.PlannerConfig.r2r(image_feat_size=FI, depth_feat_size=FD)
    model = GlocalTextPathNavCMT(cfg.to_dict(), dtype=torch.bfloat16, device=DEV)
    step = PlannerStep(model, pool[0], dropout=None)
    assert step.traj_nodes
    legs = {"csr": False, "tables": True}
    seen = {}
    for _ in range(3):
        for k, on in legs.items():
            leg(step, pool, 2, on)
            seen[k] = (step.gimg.clone(), step.logits.clone())
    step.check_traj()
    same = all(bool((x.view(torch.int32) == y.view(torch.int32)).all()) for x, y in zip(seen["csr"], seen["tables"]))
    assert same, "the two routes disagree on gmap_img_fts / logits"
    if a.profile:
        for on in legs.values():
            leg(step, pool, a.profile, on)
        print(json.dumps({"profile_iterations_per_leg": a.profile}))
        return
    rounds = {k: [] for k in legs}
    for _ in range(a.rounds):
        for k, on in legs.items():
            rounds[k].append(leg(step, pool, a.iters, on))
    tr = pool[0]["traj"]
    R, V = pool[0]["rgb_fts"].shape[:2]
    result = {"device": torch.cuda.get_device_name(0), "rounds": a.rounds, "iters": a.iters, "B": B, "dtype": "bf16",
              "unit": "us per iteration (load_batch + run_eager + synchronise), host clock; legs alternate in rounds on one step object",
              "shape": {"R": int(R), "V": int(V), "G": int(pool[0]["gmap_step_ids"].shape[1]), "L": int(pool[0]["txt_ids"].shape[1]),
                        "Kmax": int(pool[0].traj_dev["Kmax"]), "steps_per_sample": [len(p) for p in tr["traj_vpids"]]},
              "routes_bit_identical": same}
    for k, v in rounds.items():
        result[k] = {"iteration": summary([x[0] for x in v]), "load_batch_host": summary([x[1] for x in v]),
                     "issue_step_sync": summary([x[2] for x in v])}
    pairs = [(o[0], n[0]) for o, n in zip(rounds["csr"], rounds["tables"])]
    result["pairs_us"] = [[round(o, 1), round(n, 1)] for o, n in pairs]
    result["tables_lower_in_every_pair"] = all(n < o for o, n in pairs)
    result["saved_us_median"] = round(result["csr"]["iteration"]["median_us"] - result["tables"]["iteration"]["median_us"], 1)
    if a.kernel_stats:
        found = {}
        for path in glob.glob(os.path.join(a.kernel_stats, "**", "*kernel_stats.csv"), recursive=True):
            with open(path) as f:
                for r in csv.DictReader(f):
                    for k in KERNELS:
                        if k in r.get("Name", ""):
                            e = found.setdefault(k, {"calls": 0, "total_ns": 0.0})
                            e["calls"] += int(r["Calls"])
                            e["total_ns"] += float(r["AverageNs"]) * int(r["Calls"])
        if not found:
            raise SystemExit(f"no kernel row of {KERNELS} under {a.kernel_stats}")
        result["kernels"] = {k: {"calls": e["calls"], "mean_us": round(e["total_ns"] / e["calls"] / 1e3, 2)} for k, e in found.items()}
        result["kernels"]["source"] = "rocprofv3 --kernel-trace --stats, a run of its own (--profile); forward and backward launches of " \
                                      "gather_sum_kernel are averaged together"
    step.close()
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")
    print(json.dumps(result))


if __name__ == "__main__":
    main()
