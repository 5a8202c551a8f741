"""What the per-batch rebuild of the pre-training step objects costs: PretrainDriver(reuse_steps=False) -- today's per-shape cache of
PlannerSteps and a new MlmStep per MLM batch, with its synchronise -- against reuse_steps=True -- one capacity step object per task
(etpnav_amd/step.py _Staging), MLM selection by etp_mlm_select from the loader's device labels, no synchronise per batch.

    python tools/pretrain_reuse_bench.py                         -> profiles/pretrain_reuse_bench.json
    rocprofv3 --kernel-trace --stats --output-format csv -d DIR -- python tools/pretrain_reuse_bench.py --profile 40
    python tools/pretrain_reuse_bench.py --kernel-stats DIR      (adds mlm_select_kernel's own time from that run)

The synthetic corpus of R2R proportions of tools/pretrain_data_bench.py, the native loaders (SapBatches / MlmBatches, B = 32), the full
pre-training model in bf16 with the config's dropout, SAP : MLM 1 : 1 (run_pt/r2r_pretrain_habitat.json).  Both legs draw the same
batches (loaders and task plan seeded alike) and train the same model; they alternate in rounds of --iters optimizer steps inside one
process, each round closed by one synchronise.  Reported per leg: the median, lowest and highest round in ms per optimizer step, the
step objects constructed and the capacity steps' regrows.  The flag-off leg is the yardstick; no target is set.
--sync-each synchronises after every optimizer step in both legs, --ahead N lets the host run at most N steps ahead (an event per
step): how the result depends on the host's lead (profiles/pretrain_reuse_bench_{sync_each,ahead1,ahead3}.json)."""
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

from etpnav_amd import pretrain, pretrain_data as pdata, step as step_mod  # noqa: E402
from etpnav_amd.features import FeatureStore, write_flat_pack  # noqa: E402

DEV = "cuda"


def _corpus_tool():
    spec = importlib.util.spec_from_file_location("pretrain_data_bench", os.path.join(ROOT, "tools", "pretrain_data_bench.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


class Counter:
    """counts the step objects constructed, by wrapping the two constructors"""

    def __init__(self):
        self.n = {"sap": 0, "mlm": 0}
        outer = self

        class Sap(step_mod.PlannerStep):
            def __init__(self, *a, **kw):
                outer.n["sap"] += 1
                super().__init__(*a, **kw)

        class Mlm(pretrain.MlmStep):
            def __init__(self, *a, **kw):
                outer.n["mlm"] += 1
                super().__init__(*a, **kw)

        step_mod.PlannerStep, pretrain.MlmStep = Sap, Mlm

    def take(self):
        out, self.n = dict(self.n), {"sap": 0, "mlm": 0}
        return out


def summary(v):
    return {"median_ms": round(statistics.median(v), 3), "min_ms": round(min(v), 3), "max_ms": round(max(v), 3)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "pretrain_reuse_bench.json"))
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--profile", type=int, default=0, help="run that many optimizer steps of the reuse leg and stop (the rocprofv3 run)")
    ap.add_argument("--kernel-stats", default=None)
    ap.add_argument("--sync-each", action="store_true", help="synchronise after every optimizer step in both legs: the host cannot run ahead")
    ap.add_argument("--ahead", type=int, default=None, help="let the host run at most that many optimizer steps ahead of the device "
                                                            "(an event per step, a wait on the one issued that many steps ago)")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("tools/pretrain_reuse_bench.py measures on the GPU; there is none here")
    from oracle import planner_oracle as po
    from etpnav_amd.planner import GlocalTextPathNavCMT
    tool = _corpus_tool()
    B, FI, FD = tool.B, tool.FI, tool.FD
    c = tool.make_corpus()
    with tempfile.TemporaryDirectory() as td:
        write_flat_pack(os.path.join(td, "img.etpf"), zip(c["keys"], c["img"]))
        write_flat_pack(os.path.join(td, "dep.etpf"), zip(c["keys"], c["dep"]))
        store = FeatureStore(os.path.join(td, "img.etpf"), os.path.join(td, "dep.etpf")).to_device(DEV)
    graphs = pdata.NavGraphs.from_connectivity(c["connectivity"]).to_device(DEV)
    index = pdata.R2RTextPathIndex([c["annos"]], store, c["cands"], graphs, FI, FD, 100)
    cfg = po.PlannerConfig.r2r(image_feat_size=FI, depth_feat_size=FD, use_lang2visn_attn=True)
    model = GlocalTextPathNavCMT(cfg.to_dict(), dtype=torch.bfloat16, device=DEV)
    counter = Counter()
    legs, its = {}, {}
    for name, reuse in (("rebuild", False), ("reuse", True)):
        loaders = {"sap": (pdata.SapBatches(index, B, np.random.default_rng(1), DEV), 1, None),
                   "mlm": (pdata.MlmBatches(index, B, np.random.default_rng(2), DEV), 1, None)}
        legs[name] = pretrain.PretrainDriver(model, loaders, dropout="config", seed=3, generator=torch.Generator().manual_seed(4),
                                             reuse_steps=reuse, batch_size=B)
        its[name] = iter(legs[name].meta)

    def run(name, n):
        drv, it = legs[name], its[name]
        torch.cuda.synchronize()
        ring = []
        t0 = time.perf_counter()
        for _ in range(n):
            task, batch = next(it)
            drv.train_step(task, batch)
            if a.sync_each:
                torch.cuda.synchronize()
            elif a.ahead is not None:
                ring.append(torch.cuda.Event())
                ring[-1].record()
                if len(ring) > a.ahead:
                    ring.pop(0).synchronize()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) / n * 1e3

    if a.profile:
        run("reuse", a.profile)
        legs["reuse"].check_steps()
        print(json.dumps({"profile_optimizer_steps": a.profile}))
        return
    for name in legs:                                     # warm-up: kernels loaded, caches and capacities settled
        run(name, a.iters)
    counter.take()
    warm_regrows = sum(st.regrows for st in legs["reuse"]._reused.values())
    rounds, built = {k: [] for k in legs}, {k: {"sap": 0, "mlm": 0} for k in legs}
    for _ in range(a.rounds):
        for name in legs:
            rounds[name].append(run(name, a.iters))
            for k, v in counter.take().items():
                built[name][k] += v
    legs["reuse"].check_steps()
    result = {"device": torch.cuda.get_device_name(0), "rounds": a.rounds, "iters": a.iters, "B": B, "dtype": "bf16", "dropout": "config", "sync_each": bool(a.sync_each), "ahead": a.ahead,
              "task_mix": "sap : mlm = 1 : 1",
              "unit": "ms per optimizer step (loader + train_step), host clock, one synchronise per round of `iters` steps; the legs "
                      "alternate in rounds inside one process and train the same model",
              "rebuild": {"step": summary(rounds["rebuild"]), "constructed_in_timed_rounds": built["rebuild"]},
              "reuse": {"step": summary(rounds["reuse"]), "constructed_in_timed_rounds": built["reuse"],
                        "regrows_in_warmup": warm_regrows,
                        "regrows_in_timed_rounds": sum(st.regrows for st in legs["reuse"]._reused.values()) - warm_regrows,
                        "capacity": {f"{t}{'' if tr else '_eval'}": dict(st._cap) for (t, tr), st in legs["reuse"]._reused.items()}}}
    pairs = list(zip(rounds["rebuild"], rounds["reuse"]))
    result["pairs_ms"] = [[round(o, 3), round(n, 3)] for o, n in pairs]
    result["reuse_lower_in_every_pair"] = all(n < o for o, n in pairs)
    result["reuse_higher_in_every_pair"] = all(n > o for o, n in pairs)
    result["saved_ms_median"] = round(result["rebuild"]["step"]["median_ms"] - result["reuse"]["step"]["median_ms"], 3)
    if a.kernel_stats:
        calls, total = 0, 0.0
        for path in glob.glob(os.path.join(a.kernel_stats, "**", "*kernel_stats.csv"), recursive=True):
            with open(path) as f:
                for r in csv.DictReader(f):
                    if "mlm_select_kernel" in r.get("Name", ""):
                        calls += int(r["Calls"])
                        total += float(r["AverageNs"]) * int(r["Calls"])
        if not calls:
            raise SystemExit(f"no mlm_select_kernel row under {a.kernel_stats}")
        result["mlm_select_kernel"] = {"calls": calls, "mean_us": round(total / calls / 1e3, 2),
                                       "source": "rocprofv3 --kernel-trace --stats, a run of its own (--profile)"}
    for drv in legs.values():
        drv.close()
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")
    print(json.dumps(result))


if __name__ == "__main__":
    main()
