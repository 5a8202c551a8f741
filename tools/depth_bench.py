"""Times the native DD-PPO ResNet-50 depth encoder (etpnav_amd.depth.DepthEncoder.encode_views) on an MI355X and writes
profiles/depth_bench.json.

    python tools/depth_bench.py [--out profiles/depth_bench.json] [--rounds 9] [--calls 20] [--batches 8,16,32] [--dtypes bf16,fp32] [--no-eager]

Per (operand dtype, B): encode_views on 12 B depth views of 256 x 256 beside the torch restatement of the network
(tests/depth_ref.py::ResNetEncoder, i.e. torch's own convolution, GroupNorm and pooling kernels) in eager fp16 on the same device for the
bf16 row and in fp32 for the fp32 row, fed the clockwise batch directly (it is not charged for the reorder).  The two are timed in
alternating rounds after 3 warm-up calls each: every round puts `calls` back-to-back calls of one, then of the other, into one HIP-event
window each (40 ... 170 ms per window at the default 20 calls); the file keeps the median, the least and the greatest per-call time over
the rounds, and the same three figures of the per-round ratio.  Then ONE call under the library's per-launch event timing
(etp_ktime_*): the launches are grouped by kernel class (GEMM, gn_stats, gn_apply, conv_rows, stem, max-pool), giving the time share of
every class.  FLOPs and bytes are computed from the shapes below, not measured.  Weights and images are the counter-based values of tests/depth_ref.py: timing does not depend on
them.  No target is set in advance; the file records what was measured."""
import argparse
import ctypes
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

from etpnav_amd import _lib  # noqa: E402
from etpnav_amd import depth as dp  # noqa: E402
from tests import depth_ref as dr  # noqa: E402

S, BP, BLOCKS = dr.FULL
CLASSES = (("gemm", "gemm"), ("mm32", "gemm"), ("gn_stats", "gn_stats"), ("gn_apply", "gn_apply"), ("conv_rows", "conv_rows"),
           ("depth_stem", "stem"), ("maxpool", "maxpool"))


def window(fn, calls):
    """ms per call of `calls` back-to-back calls inside one HIP-event window"""
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(calls):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / calls


def alternated(fns, rounds, calls, warmup=3):
    """{name: [ms per call, one figure per round]}: every round times each function once, in turn, so that whatever else the machine does
    during the measurement meets all of them alike"""
    for fn in fns.values():
        for _ in range(warmup):
            fn()
    torch.cuda.synchronize()
    ms = {k: [] for k in fns}
    for _ in range(rounds):
        for k, fn in fns.items():
            ms[k].append(window(fn, calls))
    return ms


def spread(v):
    return statistics.median(v), min(v), max(v)


def shape_counts():
    """per view: (product FLOPs, im2col elements written, pre-norm fp32 elements) from the network's shapes"""
    flops = rows = pre = 0
    H, cin = S // 8, BP
    pre += (S // 4) ** 2 * BP
    flops += 2 * 49 * (S // 4) ** 2 * BP
    for l in range(4):
        p = BP << l
        for i in range(BLOCKS[l]):
            s = 2 if (l > 0 and i == 0) else 1
            Ho = H // s
            flops += 2 * (H * H * cin * p + Ho * Ho * 9 * p * p + Ho * Ho * p * 4 * p)
            rows += Ho * Ho * 9 * p
            pre += H * H * p + Ho * Ho * p + Ho * Ho * 4 * p
            if i == 0:
                flops += 2 * Ho * Ho * cin * 4 * p
                pre += Ho * Ho * 4 * p
                rows += Ho * Ho * cin if s == 2 else 0
            H, cin = Ho, 4 * p
    flops += 2 * H * H * 9 * cin * 128
    rows += H * H * 9 * cin
    pre += H * H * 128
    return flops, rows, pre


def per_launch(enc, obs):
    """one call under etp_ktime: [(us, kernel name)] in launch order"""
    L = _lib.lib()
    enc.encode_views(obs)
    torch.cuda.synchronize()
    L.etp_ktime_reset()
    L.etp_ktime_enable(1)
    enc.encode_views(obs)
    torch.cuda.synchronize()
    L.etp_ktime_enable(0)
    cap = 1 << 20
    buf = ctypes.create_string_buffer(cap)
    L.etp_ktime_report(buf, cap)
    L.etp_ktime_reset()
    rows = []
    for line in buf.value.decode().splitlines():
        f = line.split("\t")
        if len(f) >= 5:
            rows.append((float(f[0]), f[4]))
    return rows


def class_of(kernel):
    for part, name in CLASSES:
        if part in kernel:
            return name
    return "other"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "depth_bench.json"))
    ap.add_argument("--rounds", type=int, default=9, help="rounds; each times every candidate once, in turn")
    ap.add_argument("--calls", type=int, default=20, help="calls inside one HIP-event window")
    ap.add_argument("--batches", default="8,16,32")
    ap.add_argument("--no-eager", action="store_true", help="skip the eager-torch comparison")
    ap.add_argument("--dtypes", default="bf16,fp32", help="operand dtypes to run (a profiler run wants one)")
    a = ap.parse_args()
    assert torch.cuda.is_available(), "this measurement needs the GPU; there is no CPU fallback"
    W = dr.make_weights(S, BP, BLOCKS, 1)
    flops, rows, pre = shape_counts()
    result = {"device": torch.cuda.get_device_name(0), "image_size": S, "base_planes": BP, "blocks": list(BLOCKS),
              "gflop_per_view": flops / 1e9, "im2col_elements_per_view": rows, "pre_norm_fp32_elements_per_view": pre,
              "launches_per_call": 19 + 10 * sum(BLOCKS), "rows": []}
    for dt_name, dt, ref_dt in (("bf16", torch.bfloat16, torch.float16), ("fp32", torch.float32, torch.float32)):
        if dt_name not in a.dtypes.split(","):
            continue
        enc = dp.DepthEncoder(device="cuda", dtype=dt)
        enc.load_state_dict(W, strict=True)
        ref = None if a.no_eager else dr.module_with(W, S, BP, BLOCKS, ref_dt).to("cuda")
        for B in [int(b) for b in a.batches.split(",")]:
            N = 12 * B
            images = dr.make_depth(0, 12, S).repeat(B, 1, 1, 1).to("cuda")
            obs = {("depth" if v == 0 else f"depth_{v * 30.0}"): images[(12 - v) % 12::12].contiguous() for v in range(12)}
            fns = {"native": lambda: enc.encode_views(obs)}
            if ref is not None:
                x = images.to(ref_dt)
                fns["eager"] = lambda: ref({"depth": x})
            with torch.no_grad():
                ms = alternated(fns, a.rounds, a.calls)
            med, lo, hi = spread(ms["native"])
            es = 2 if dt == torch.bfloat16 else 4
            row = {"dtype": dt_name, "B": B, "views": N, "rounds": a.rounds, "calls_per_window": a.calls,
                   "native_ms": med, "native_ms_min": lo, "native_ms_max": hi,
                   "native_tflops": flops * N / med / 1e9, "scratch_gb": int(enc.L.etp_depth_ws_bytes(enc.handle, N)) / 1e9,
                   "im2col_gb_written_and_read": 2 * rows * N * es / 1e9,
                   "group_norm_gb": pre * N * (3 * 4 + es) / 1e9}       # two statistics passes and the apply read fp32; one store
            if ref is not None:
                emed, elo, ehi = spread(ms["eager"])
                rmed, rlo, rhi = spread([e / n for e, n in zip(ms["eager"], ms["native"])])      # per round: neighbours in time
                row.update({"eager_torch_dtype": str(ref_dt).replace("torch.", ""), "eager_torch_ms": emed, "eager_torch_ms_min": elo,
                            "eager_torch_ms_max": ehi, "speedup_vs_eager": rmed, "speedup_vs_eager_min": rlo,
                            "speedup_vs_eager_max": rhi})
            launches = per_launch(enc, obs)
            row["launches_timed"] = len(launches)
            total = sum(us for us, _ in launches)
            share = {}
            for us, name in launches:
                share[class_of(name)] = share.get(class_of(name), 0.0) + us
            row["sum_of_launch_us"] = total
            row["class_us"] = share
            row["class_share"] = {k: v / total for k, v in share.items()} if total else {}
            if "other" in share:
                row["other_kernels"] = sorted({n for _, n in launches if class_of(n) == "other"})
            result["rows"].append(row)
            os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
            with open(a.out, "w") as f:                       # after every row: a later row that fails keeps the earlier ones
                json.dump(result, f, indent=1, sort_keys=True)
            print(json.dumps({k: row.get(k) for k in ("dtype", "B", "native_ms", "native_ms_min", "native_ms_max", "eager_torch_ms", "speedup_vs_eager",
                                                      "speedup_vs_eager_min", "speedup_vs_eager_max", "launches_timed",
                                                      "class_share")}), flush=True)
            del images, obs
        del enc, ref
        torch.cuda.empty_cache()
    print(a.out)


if __name__ == "__main__":
    main()
