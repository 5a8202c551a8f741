"""Host time of a same-shape load_batch on a fixed step (the default PretrainDriver's SAP path takes one per micro-step).

Two steps, no run_eager in between (only the load is timed): a PlannerStep at tools/h2d_bench.py's shape (workload c2, bf16, pinned host
batches) and an MlmStep at the largest batch of tests/test_step_reuse_gpu.py (the pre-training config of oracle/make_golden_pretrain.py).
Per run `--loads` loads between two time.perf_counter() reads with one device synchronise at the end; `--runs` runs, median and lowest /
highest in microseconds per load.  The file runs unchanged on an older tree: point --label at what is being measured.

    python tools/step_load_bench.py --label parent > load_parent.json
"""
import argparse
import json
import os
import statistics
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from bench import WORKLOADS  # noqa: E402
from etpnav_amd.planner import GlocalTextPathNavCMT, default_config  # noqa: E402
from etpnav_amd.pretrain import MlmStep  # noqa: E402
from etpnav_amd.step import PlannerStep  # noqa: E402
from etpnav_amd.synthetic import make_batch, make_sap_batch  # noqa: E402

MLM_SHAPE = dict(B=5, L=28, T=4, V=12, n_cand=5)     # tests/test_step_reuse_gpu.py SEQ[4]


def timed(step, batches, loads, runs):
    out = []
    for _ in range(runs + 1):                            # the first run warms up and is dropped
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for i in range(loads):
            step.load_batch(batches[i % len(batches)])
        torch.cuda.synchronize()
        out.append((time.perf_counter() - t0) / loads * 1e6)
    out = out[1:]
    return {"us_per_load_median": round(statistics.median(out), 2), "us_per_load_runs": [round(x, 2) for x in out]}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--label", default="this tree")
    ap.add_argument("--loads", type=int, default=300)
    ap.add_argument("--runs", type=int, default=3)
    a = ap.parse_args()
    res = {"label": a.label, "loads": a.loads, "runs": a.runs}

    w = WORKLOADS["c2"]
    cfg = default_config(w["task"], image_feat_size=w["image_feat_size"])
    model = GlocalTextPathNavCMT(cfg, dtype=torch.bfloat16, device="cuda")
    model.init_weights(seed=0)
    mk = lambda seed: make_batch(cfg.vocab_size, cfg.image_feat_size, cfg.depth_feat_size, w["B"], w["L"], w["V"], w["G"], seed=seed)
    host = [{k: v.pin_memory() for k, v in mk(1234 + i).items()} for i in range(4)]
    step = PlannerStep(model, mk(1), overlap=True, dropout="config", drop_seed=0)
    res["planner_step_c2"] = timed(step, host, a.loads, a.runs)
    step.close()

    from oracle.make_golden_pretrain import make_case
    pcfg, P, _ = make_case()
    pmodel = GlocalTextPathNavCMT(pcfg.to_dict(), dtype=torch.bfloat16, device="cuda")
    pmodel.load_state_dict(dict(P), strict=True)
    batches = []
    for seed in (15, 16):                                # two batches of one shape with the same masked positions: Nm is equal
        b = make_sap_batch(pcfg.vocab_size, pcfg.image_feat_size, pcfg.depth_feat_size, seed=seed, **MLM_SHAPE)
        lab = torch.full_like(b["txt_ids"], -1)
        lab[:, 1::4] = b["txt_ids"][:, 1::4]
        b["txt_labels"] = lab
        batches.append(b)
    step = MlmStep(pmodel, batches[0], dropout="config")
    res["mlm_step_reuse_largest"] = timed(step, batches, a.loads, a.runs)
    step.close()
    print(json.dumps(res))


if __name__ == "__main__":
    main()
