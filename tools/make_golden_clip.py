"""Writes tests/golden/clip_small.npz: what tests/test_clip_ref_cpu.py and tests/test_clip_gpu.py pin the CLIP view encoder to.

    python tools/make_golden_clip.py

For every case of tests/clip_ref.GOLDEN_CASES (image size, layers, images; weights and images from the counter-based hash of
tests/clip_ref.py, seed CASE_SEED) the file holds, all computed by transformers.CLIPVisionModelWithProjection on the CPU:

    <case>/emb          [n, 512] float64      image_embeds of the float64 run
    <case>/probe_rows   [r] int64             rows of the [n T, 768] residual stream that are kept (all of them for the small case; the
                                              class-token rows, the first and last patch rows and a stride in between for (224, 12): the
                                              whole stream would be 1.8 MB)
    <case>/probes       [3, r, 768] float64   the residual stream after ln_pre, after layer 0 and after the last layer at those rows
    <case>/bf16_gap     float64               relative L2 of image_embeds of the SAME model in fp32 under torch.autocast("cpu", bfloat16)
                                              against its float64 run (the yardstick of the engine's bf16 mode)

No weights and no images are stored.  Needs transformers; nothing else outside the repository.
"""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from tests import clip_ref as cr  # noqa: E402


def probe_rows(n, T):
    if n * T <= 64:
        return np.arange(n * T, dtype=np.int64)
    rows = set()
    for i in range(n):
        rows.update(i * T + t for t in (0, 1, T - 1))
        rows.update(range(i * T + 2, (i + 1) * T - 1, 9))
    return np.array(sorted(rows), dtype=np.int64)


def main():
    torch.manual_seed(0)
    store = {}
    for name, (S, layers, n) in cr.GOLDEN_CASES.items():
        W = cr.make_weights(S, layers, cr.CASE_SEED)
        images = cr.make_images(n, S, cr.CASE_SEED)
        emb, probes = cr.hf_forward(W, images, layers)
        low, _ = cr.hf_forward(W, images, layers, dtype=torch.float32, autocast=True)
        rows = probe_rows(n, (S // cr.PATCH) ** 2 + 1)
        store[f"{name}/emb"] = emb.numpy()
        store[f"{name}/probe_rows"] = rows
        store[f"{name}/probes"] = probes[:, torch.from_numpy(rows)].numpy()
        store[f"{name}/bf16_gap"] = np.float64(cr.rel_l2(low, emb))
        print(f"{name}: |emb|max {float(emb.abs().max()):.4f}  rows kept {len(rows)}  bf16 autocast gap {store[f'{name}/bf16_gap']:.3e}")
    dst = os.path.join(ROOT, "tests", "golden", "clip_small.npz")
    np.savez(dst, **store)
    print(dst, os.path.getsize(dst), "bytes")


if __name__ == "__main__":
    main()
