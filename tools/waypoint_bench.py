"""One waypoint call -- candidates(forward(depth embeddings)) and the copy of the candidate table to the host -- at B = 8, 16, 32 on
the GPU: the native head (etpnav_amd/waypoint.py, bf16 and fp32 engines) against the same arithmetic in eager fp32 torch
(tests/waypoint_ref.head_ref on the device, then the heat-map tail the way the reference walks it: softmax, wrap, a five-round nms
loop of small launches, one .nonzero() and host copy per episode).

    python tools/waypoint_bench.py [--out profiles/waypoint_bench.json] [--rounds 5] [--iters 30]

Every leg is warmed up; the legs alternate within a round, `rounds` times; a call is timed with a host clock and ends in a device
synchronise (the table copy, or .cpu() of the last episode).  Reported per leg: the median over rounds of the per-call mean, and the
lowest and highest round.  Launches per native call and their kernel times come from the library's per-launch event timing, in a run of their own.
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402

from etpnav_amd import _lib  # noqa: E402
from etpnav_amd import waypoint as wp  # noqa: E402
from tests import waypoint_ref as wr  # noqa: E402

DEV = "cuda"


def eager_tail(logits):
    """the reference's walk over the heat map in eager torch (Policy_ViewSelection_ETP.py:220-239,304-305; utils.py:37-64)"""
    B = logits.shape[0]
    p = torch.softmax(logits.reshape(B, -1), 1).reshape(B, 120, 12)
    pred = torch.cat((p[:, -1:], p, p[:, :1]), 1)
    out = torch.zeros_like(pred)
    supp = pred.clone()
    rows = torch.arange(B, device=logits.device)
    xs = torch.arange(12, device=logits.device, dtype=torch.float32)[None, None]
    ys = torch.arange(122, device=logits.device, dtype=torch.float32)[None, :, None]
    for _ in range(5):
        _, ix = torch.max(supp.reshape(B, -1), 1)
        out.reshape(B, -1)[rows, ix] = pred.reshape(B, -1)[rows, ix]
        y_mu = (ix / 12).float()[:, None, None]
        x_mu = (ix % 12).float()[:, None, None]
        xd = torch.min(torch.abs(xs - x_mu), torch.abs(xs - x_mu + 12))
        g = torch.logical_and(xd <= 7.0, torch.abs(ys - y_mu) <= 5.0).float()
        supp = supp * (1 - g)
    out = out[:, 1:-1]
    res = []
    for j in range(B):
        nz = out[j].nonzero()
        res.append((nz[:, 0].cpu().tolist(), nz[:, 1].cpu().tolist()))
    return res


def kernel_trace(fn):
    """-> (number of library launches of one call, [(kernel, us)] in issue order) from the library's per-launch event timing (a run
    of its own: the events slow the host down)"""
    import ctypes
    L = _lib.lib()
    L.etp_ktime_reset()
    L.etp_ktime_enable(1)
    fn()
    torch.cuda.synchronize()
    L.etp_ktime_enable(0)
    buf = ctypes.create_string_buffer(1 << 16)
    L.etp_ktime_report(buf, 1 << 16)
    L.etp_ktime_reset()
    rows = [ln.split("\t") for ln in buf.value.decode().splitlines() if ln]
    return len(rows), [(r[4].split("(")[0][-60:], float(r[0])) for r in rows]


def timed(fn, iters):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(iters):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / iters * 1e6


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "waypoint_bench.json"))
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--iters", type=int, default=30)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("tools/waypoint_bench.py measures on the GPU; there is none here")
    W = wr.make_weights(wr.GOLDEN_SEED)
    Wd = {k: v.to(DEV) for k, v in W.items()}
    models = {}
    for name, dt in (("native_bf16", torch.bfloat16), ("native_fp32", torch.float32)):
        m = wp.BinaryDistPredictorTRM(device=DEV, dtype=dt)
        m.load_state_dict(W, strict=True)
        models[name] = m.eval()
    result = {"device": torch.cuda.get_device_name(0), "rounds": a.rounds, "iters": a.iters, "unit": "us per call", "B": {}}
    for B in (8, 16, 32):
        g = torch.Generator().manual_seed(B)
        depth = torch.randn(12 * B, 2048, generator=g).abs().to(DEV)
        legs = {name: (lambda m=m: m.candidates(m(None, depth), False).table.cpu()) for name, m in models.items()}
        legs["eager_fp32"] = lambda: eager_tail(wr.head_ref(Wd, depth, dtype=torch.float32).float())
        with torch.no_grad():
            for fn in legs.values():                       # warm-up: code objects, workspaces, the bf16 shadow
                for _ in range(5):
                    fn()
            launches, kernel_us = {}, {}
            for name in ("native_bf16", "native_fp32"):
                launches[name], kernel_us[name] = kernel_trace(legs[name])
            # the native candidates equal the eager walk's on these inputs (fp32 engine)
            tab = legs["native_fp32"]().numpy()
            want = legs["eager_fp32"]()
            same = all(tab[1, j, :int(tab[0, j, 0])].tolist() == want[j][0] and tab[2, j, :int(tab[0, j, 0])].tolist() == want[j][1]
                       for j in range(B))
            per_round = {name: [] for name in legs}
            for _ in range(a.rounds):
                for name, fn in legs.items():
                    per_round[name].append(timed(fn, a.iters))
        row = {name: {"median_us": round(statistics.median(v), 1), "min_us": round(min(v), 1), "max_us": round(max(v), 1)}
               for name, v in per_round.items()}
        row["launches_per_call"] = launches
        row["kernel_us_in_issue_order"] = kernel_us
        row["candidates_equal_eager_fp32"] = bool(same)
        result["B"][str(B)] = row
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")
    print(json.dumps(result))


if __name__ == "__main__":
    main()
