"""Write tests/golden/depth_small.npz: what the depth-encoder tests compare against (CPU only, a minute).

    python tools/make_golden_depth.py

For each engine case of tests/depth_ref.py (the three small networks at 13 images, the full network at 12 images, one network at image
size 192 at 3 images), with the counter-based weights and depth images of that file:

    case_<i>          (image_size, base_planes, blocks..., number of images)
    seeds_<i>         (weight seed, image case index): make_weights(..., seed) and make_depth(case index, n, image_size) rebuild the inputs
    y64_<i>           the torch module's output in float64 [n, Cc, fs, fs]
    gap_fp32_<i>      max |module in fp32 - y64| / max |y64|: the module's own fp32 gap (one valid fp32 summation order)
    gap_bf16_<i>      || module under torch.autocast("cpu", bfloat16) - y64 || / || y64 ||: its own bf16 gap

The module is tests/depth_ref.py::ResNetEncoder, a restatement of habitat-lab's source; habitat's own classes were not available.
"""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from tests import depth_ref as dr  # noqa: E402

WEIGHT_SEED = 1


def main():
    torch.manual_seed(0)
    out = {}
    cases = list(zip(dr.ALL_CASES, dr.ALL_CASE_N))
    for i, ((S, bp, blocks), n) in enumerate(cases):
        W = dr.make_weights(S, bp, blocks, WEIGHT_SEED)
        depth = dr.make_depth(i, n, S)
        with torch.no_grad():
            y64 = dr.module_with(W, S, bp, blocks, torch.float64)({"depth": depth.double()})
            m32 = dr.module_with(W, S, bp, blocks, torch.float32)
            y32 = m32({"depth": depth}).double()
            with torch.autocast("cpu", dtype=torch.bfloat16):
                ybf = m32({"depth": depth}).double()
        out[f"case_{i}"] = np.array([S, bp, *blocks, n], dtype=np.int64)
        out[f"seeds_{i}"] = np.array([WEIGHT_SEED, i], dtype=np.int64)
        out[f"y64_{i}"] = y64.numpy()
        out[f"gap_fp32_{i}"] = np.float64(((y32 - y64).abs().max() / y64.abs().max()).item())
        out[f"gap_bf16_{i}"] = np.float64(((ybf - y64).norm() / y64.norm()).item())
        print(f"case {i} {(S, bp, blocks)} n {n}: out {tuple(y64.shape)}, fp32 gap / |y|inf {out[f'gap_fp32_{i}']:.3e}, "
              f"bf16 autocast gap (relative L2) {out[f'gap_bf16_{i}']:.3e}, zeros {(y64 == 0).double().mean().item():.2f}")
    path = os.path.join(ROOT, "tests", "golden", "depth_small.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
