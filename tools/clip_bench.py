"""Times the native CLIP ViT-B/32 view encoder (etpnav_amd.clip.CLIPEncoder.encode_views) on an MI355X and writes
profiles/clip_bench.json.

    python tools/clip_bench.py [--out profiles/clip_bench.json] [--iters 10] [--batches 8,16,32]

Per (operand dtype, B): one encode_views call on 12 B views of 224 x 224 (median of `iters` HIP-event timings after 3 warm-up calls),
beside the same arithmetic as an eager-torch restatement on the same device (tests/clip_ref.forward in half precision for the bf16
row, fp32 for the fp32 row; weights already converted, so only the forward is timed).  Then ONE call under the library's per-launch
event timing (etp_ktime_*): the launches are attributed to their class by position in the engine's fixed issue order (1 + 1 + 1 +
8 x layers + 2), giving the time share of every class and, for the five GEMM classes, the achieved TFLOP/s next to what
tools/gemm_bench.run gives for that shape alone.  Weights and images are the counter-based values of tests/clip_ref.py: timing does not
depend on them.  No target is set in advance; the file records what was measured."""
import argparse
import importlib.util
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

from etpnav_amd import _lib  # noqa: E402
from etpnav_amd import clip as cl  # noqa: E402
from tests import clip_ref as cr  # noqa: E402

S, LAYERS, T, P = 224, 12, 50, 49
LAYER_CLASSES = ("ln_1", "gemm qkv", "attention", "gemm out_proj", "ln_2", "gemm c_fc", "quick_gelu", "gemm c_proj")
# class -> (rows per image, N, K, tools/gemm_bench kind that is closest: fp32 C + residual, or operand-dtype C + bias)
GEMMS = {"gemm conv1": (P, 768, 3072, "fwd_s"), "gemm qkv": (T, 2304, 768, "fwd"), "gemm out_proj": (T, 768, 768, "fwd_s"),
         "gemm c_fc": (T, 3072, 768, "fwd"), "gemm c_proj": (T, 768, 3072, "fwd_s"), "gemm proj": (1, 512, 768, None)}


def timed(fn, iters, warmup=3):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(iters):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        torch.cuda.synchronize()
        ms.append(e0.elapsed_time(e1))
    return statistics.median(ms), min(ms), max(ms)


def launch_classes():
    names = ["patch_rows", "gemm conv1", "tokens"]
    for _ in range(LAYERS):
        names += list(LAYER_CLASSES)
    return names + ["cls_ln", "gemm proj"]


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
    import ctypes
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "clip_bench.json"))
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--batches", default="8,16,32")
    a = ap.parse_args()
    spec = importlib.util.spec_from_file_location("gemm_bench", os.path.join(ROOT, "tools", "gemm_bench.py"))
    gb = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(gb)
    W = cr.make_weights(S, LAYERS, cr.CASE_SEED)
    flops_per_view = 2.0 * (P * 768 * 3072 + LAYERS * T * (2304 * 768 + 768 * 768 + 2 * 3072 * 768) + 768 * 512) + LAYERS * 4.0 * 12 * T * T * 64
    result = {"device": torch.cuda.get_device_name(0), "image_size": S, "layers": LAYERS, "gflop_per_view": flops_per_view / 1e9,
              "launches_per_call": 3 + 8 * LAYERS + 2, "rows": []}
    for dt_name, dt, ref_dt in (("bf16", torch.bfloat16, torch.float16), ("fp32", torch.float32, torch.float32)):
        enc = cl.CLIPEncoder(device="cuda", dtype=dt, image_size=S, layers=LAYERS)
        enc.load_state_dict(W, strict=True)
        Wd = {k: v.to("cuda", ref_dt) for k, v in W.items()}
        for B in [int(b) for b in a.batches.split(",")]:
            N = 12 * B
            images = cr.make_images(N, S, 5).to("cuda")
            obs = {("rgb" if v == 0 else f"rgb_{v * 30.0}"): images[(12 - v) % 12::12].contiguous() for v in range(12)}
            med, lo, hi = timed(lambda: enc.encode_views(obs), a.iters)
            with torch.no_grad():
                emed, elo, ehi = timed(lambda: cr.forward(Wd, images, LAYERS, dtype=ref_dt)[0], a.iters)
            row = {"dtype": dt_name, "B": B, "views": N, "native_ms": med, "native_ms_min": lo, "native_ms_max": hi,
                   "native_tflops": flops_per_view * N / med / 1e9, "eager_torch_dtype": str(ref_dt).replace("torch.", ""),
                   "eager_torch_ms": emed, "eager_torch_ms_min": elo, "eager_torch_ms_max": ehi, "speedup_vs_eager": emed / med}
            launches = per_launch(enc, obs)
            names = launch_classes()
            row["launches_timed"] = len(launches)
            if len(launches) == len(names):
                total = sum(us for us, _ in launches)
                share = {}
                for (us, _), cls_name in zip(launches, names):
                    share[cls_name] = share.get(cls_name, 0.0) + us
                row["sum_of_launch_us"] = total
                row["class_us"] = share
                row["class_share"] = {k: v / total for k, v in share.items()}
                non_gemm = {k: v for k, v in share.items() if not k.startswith("gemm")}
                row["largest_non_gemm_class"] = max(non_gemm, key=non_gemm.get)
                row["gemm"] = {}
                for cls_name, (rows_per, n, k, kind) in GEMMS.items():
                    M = N * rows_per
                    count = LAYERS if cls_name in LAYER_CLASSES else 1
                    us = share[cls_name] / count
                    g = {"M": M, "N": n, "K": k, "us_in_call": us, "tflops_in_call": 2.0 * M * n * k / us / 1e6}
                    if kind is not None:
                        alone_us, alone_tf = gb.run(kind, M, n, k, dtype=_lib.ETP_BF16 if dt == torch.bfloat16 else _lib.ETP_F32)
                        g.update({"gemm_bench_kind": kind, "us_alone": alone_us, "tflops_alone": alone_tf})
                    row["gemm"][cls_name] = g
            else:
                row["kernels"] = sorted({n for _, n in launches})
            result["rows"].append(row)
            print(json.dumps({k: row[k] for k in ("dtype", "B", "native_ms", "eager_torch_ms", "speedup_vs_eager", "launches_timed")}
                             | {"largest_non_gemm_class": row.get("largest_non_gemm_class")}), flush=True)
            del images, obs
        del enc, Wd
        torch.cuda.empty_cache()
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(result, f, indent=1, sort_keys=True)
    print(a.out)


if __name__ == "__main__":
    main()
