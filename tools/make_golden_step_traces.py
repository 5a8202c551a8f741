"""The call trace of every recorded training step -> tests/golden/step_traces.json (needs the MI355X).

    python tools/make_golden_step_traces.py            # rewrite the fixture from the checked-out step code

For every schedule case of tests/test_sched_gpu.py (its CASES table, both graphs of split_text_bwd), the MLM step and two forward-only
recordings, the fixture holds what the recorder tells about the graph without a pointer in it: the etp_graph_trace rows (kind, stream,
event, node), the node names in creation order and n_kernels / n_edges / n_streams.  tests/test_step_trace_gpu.py records the same
steps from the current step code and requires equality, so a change to the layer that ISSUES a step (step.py, pretrain.py) is held to
"the same calls in the same order on the same streams".  Cases, models, batches and the recording helpers are those of
tests/test_sched_gpu.py; nothing of them is restated here.

Format: {"names": [...], "graphs": {key: [graph, ...]}} with graph = {"rows": flat 4 x int per call, "nodes": index into names per
node, "n_kernels", "n_edges", "n_streams"}; compact JSON, one line.  Every key is recorded twice from fresh step objects and nothing
is written unless the two agree.
"""
from __future__ import annotations

import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
GOLDEN = os.path.join(ROOT, "tests", "golden", "step_traces.json")

MLM, FWD_PLANNER, FWD_MLM = "mlm_pretrain", "forward_only_default_bf16", "forward_only_mlm"


def keys():
    from tests.test_sched_gpu import CASES
    return list(CASES) + [MLM, FWD_PLANNER, FWD_MLM]


def _graph(rec):
    """one Recorded -> plain data (names still strings)"""
    return {"rows": [int(x) for row in rec.trace for x in row], "nodes": [rec.name(i) for i in range(rec.n)],
            "n_kernels": rec.n_kernels, "n_edges": rec.n_edges, "n_streams": rec.n_streams}


def _mlm_graphs(stream, backward):
    import torch
    from oracle.make_golden_pretrain import make_case
    from tests import test_sched_gpu as ts
    from etpnav_amd.pretrain import MlmStep
    L = ts._lib.lib()
    cfg, P, batch = make_case()
    model = ts.GlocalTextPathNavCMT(cfg.to_dict(), dtype=torch.bfloat16, device="cuda")
    model.load_state_dict(P, strict=True)
    model.eval()
    step = MlmStep(model, batch, dropout=(0.1, 0.1, 0.1, 0.0), drop_seed=9, overlap=True)
    recs = []
    try:
        step.step_no = -1
        step.run_eager()
        torch.cuda.synchronize()
        recs.append(ts.record(L, lambda st: step.run_eager(backward=backward), stream))    # MlmStep issues on torch's current stream
        return [_graph(r) for r in recs]
    finally:
        torch.cuda.synchronize()
        for r in recs:
            r.destroy()
        step.close()


def record_key(key, stream):
    """-> the graphs of one key as plain data, recorded once after one warm-up step (step_no = -1, run_eager, record)"""
    import torch
    from tests import test_sched_gpu as ts
    if key in (MLM, FWD_MLM):
        return _mlm_graphs(stream, backward=(key == MLM))
    backward = key != FWD_PLANNER
    dtype, overlap, env, cfg_kw, (B, Lt), how = ts.CASES["default_bf16" if key == FWD_PLANNER else key]
    L = ts._lib.lib()
    cfg, model = ts.model_for(dtype, **cfg_kw)
    batch = ts.po.make_batch(cfg, B=B, L=Lt, V=19, G=10, seed=99, ragged=True)
    saved = {k: os.environ.get(k) for k in env}
    os.environ.update(env)                       # the switches are read once, in PlannerStep.__init__
    try:
        if how == "micro":
            step = ts.MicroBatchedStep(model, batch, n_micro=2, dropout=ts.RATES, drop_seed=ts.SEED)
            parts = step.parts
        else:
            step = ts.PlannerStep(model, batch, overlap=overlap, dropout=ts.RATES, drop_seed=ts.SEED)
            parts = [step]
    finally:
        for k, v in saved.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v
    recs = []
    try:
        for p in parts:
            p.step_no = -1
        step.run_eager()
        torch.cuda.synchronize()
        if how == "split":
            recs.append(ts.record(L, lambda st: step.enqueue_main(st, True), stream))
            recs.append(ts.record(L, step.enqueue_txt_bwd, stream))
        elif how == "dp":
            from etpnav_amd import dp
            groups = dp.planner_buckets_layered(model, text_groups=2)[2]
            recs.append(ts.record(L, lambda st: step.run_data_parallel(groups, lambda i, side: None, stream=st, overlapped=True), stream))
        elif backward:
            recs.append(ts.record(L, lambda st: step.run_eager(stream=st), stream))
        else:
            recs.append(ts.record(L, lambda st: step.run_eager(stream=st, backward=False), stream))
        return [_graph(r) for r in recs]
    finally:
        torch.cuda.synchronize()
        for r in recs:
            r.destroy()
        step.close()


def new_stream():
    import ctypes
    from etpnav_amd import _lib
    s = ctypes.c_void_p()
    _lib.check(_lib.lib().etp_stream_create(ctypes.byref(s)), "stream_create")
    return s.value


def encode(graphs_by_key) -> str:
    """the file's text: one name table, integers otherwise"""
    names = sorted({n for gs in graphs_by_key.values() for g in gs for n in g["nodes"]})
    at = {n: i for i, n in enumerate(names)}
    out = {"names": names, "graphs": {k: [{**g, "nodes": [at[n] for n in g["nodes"]]} for g in gs] for k, gs in graphs_by_key.items()}}
    return json.dumps(out, separators=(",", ":")) + "\n"


def load():
    """the fixture with the node names put back -> {key: [graph, ...]}"""
    with open(GOLDEN) as f:
        d = json.load(f)
    names = d["names"]
    return {k: [{**g, "nodes": [names[i] for i in g["nodes"]]} for g in gs] for k, gs in d["graphs"].items()}


if __name__ == "__main__":
    import torch
    from etpnav_amd import _lib
    stream = new_stream()
    first = {k: record_key(k, stream) for k in keys()}
    second = {k: record_key(k, stream) for k in keys()}
    torch.cuda.synchronize()
    _lib.lib().etp_stream_destroy(stream)
    differ = [k for k in first if first[k] != second[k]]
    if differ:
        sys.exit(f"two recordings of the same step differ for {differ}: nothing written")
    text = encode(first)
    with open(GOLDEN, "w") as f:
        f.write(text)
    print(GOLDEN, len(text), "bytes;", sum(len(g) for g in first.values()), "graphs,",
          sum(len(x["nodes"]) for g in first.values() for x in g), "nodes")
