"""Pins tests/clip_ref.py, the float64 restatement of OpenAI CLIP's visual tower that tests/test_clip_gpu.py measures the HIP encoder
against: to transformers.CLIPVisionModelWithProjection in float64 (1e-10 relative, embeddings and the three residual probes, in_proj
split into q / k / v), to the committed fixture tests/golden/clip_small.npz (tools/make_golden_clip.py), and against nine planted
mistakes, each of which must move the embeddings by far more than the pin allows.  Also checks the counter-based value generator and
the QuickGELU bound's own arithmetic.  No kernel is launched here."""
import os

import numpy as np
import pytest
import torch

from tests import clip_ref as cr

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "clip_small.npz")
PIN = 1e-10
F64 = torch.float64
_CACHE = {}


def case(name):
    """weights, images and the float64 restatement of one fixture case, computed once per session and never modified"""
    if name not in _CACHE:
        S, layers, n = cr.GOLDEN_CASES[name]
        W = cr.make_weights(S, layers, cr.CASE_SEED)
        images = cr.make_images(n, S, cr.CASE_SEED)
        _CACHE[name] = (W, images, layers) + cr.forward(W, images, layers)
    return _CACHE[name]


def test_splitmix64_known_values():
    # the first outputs of splitmix64 seeded with 0 (reference implementation by Vigna): state advances by the golden-ratio constant
    z = np.array([0, 0x9E3779B97F4A7C15], dtype=np.uint64)
    got = [int(v) for v in cr._splitmix64(z)]
    assert got == [0xE220A8397B1DCDAF, 0x6E789E6AA1B965F4]
    a, b = cr.hash_uniform("a", 1, (1000,)), cr.hash_uniform("b", 1, (1000,))
    assert float(a.min()) >= -1 and float(a.max()) < 1 and abs(float(a.mean())) < 0.1 and not torch.equal(a, b)
    assert torch.equal(a, cr.hash_uniform("a", 1, (1000,))) and not torch.equal(a, cr.hash_uniform("a", 2, (1000,)))


def test_weight_statistics():
    W = cr.make_weights(64, 1, 1)
    assert [k for k, _ in cr.param_shapes(64, 1)] == list(W.keys())
    assert float(W["conv1.weight"].abs().max()) <= 3072 ** -0.5 and float(W["proj"].abs().max()) <= 768 ** -0.5
    assert float((W["ln_pre.weight"] - 1).abs().max()) <= 0.1 + 1e-6 and float(W["class_embedding"].abs().max()) <= 0.02
    assert float(W["transformer.resblocks.0.ln_2.weight"].min()) >= 0.9 - 1e-6
    assert float(W["transformer.resblocks.0.attn.in_proj_weight"].abs().max()) <= 768 ** -0.5


@pytest.mark.parametrize("name", list(cr.GOLDEN_CASES))
def test_restatement_equals_transformers(name):
    pytest.importorskip("transformers")
    W, images, layers, y, probes = case(name)
    hy, hp = cr.hf_forward(W, images, layers)
    assert cr.rel_l2(y, hy) <= PIN, cr.rel_l2(y, hy)
    for i in range(3):
        assert cr.rel_l2(probes[i], hp[i]) <= PIN, (i, cr.rel_l2(probes[i], hp[i]))


@pytest.mark.parametrize("name", list(cr.GOLDEN_CASES))
def test_restatement_equals_fixture(name):
    W, images, layers, y, probes = case(name)
    g = np.load(GOLDEN)
    assert cr.rel_l2(y, torch.from_numpy(g[f"{name}/emb"])) <= PIN
    rows = torch.from_numpy(g[f"{name}/probe_rows"])
    want = torch.from_numpy(g[f"{name}/probes"])
    for i in range(3):
        assert cr.rel_l2(probes[i][rows], want[i]) <= PIN, i
    S, _, n = cr.GOLDEN_CASES[name]
    T = (S // 32) ** 2 + 1
    assert set(range(0, n * T, T)) <= set(rows.tolist())                  # every class-token row is kept
    gap = float(g[f"{name}/bf16_gap"])
    assert 1e-4 < gap < 5e-2, gap                                         # a bf16 forward: neither exact nor broken


@pytest.mark.parametrize("mut", cr.MUTATIONS)
def test_planted_mistakes_are_rejected(mut):
    W, images, layers, y, _ = case("s64_l2_n3")
    ym, _ = cr.forward(W, images, layers, mut=mut)
    assert cr.rel_l2(ym, y) > 1e-3, (mut, cr.rel_l2(ym, y))               # seven orders of magnitude beyond the pin


def test_patch_rows_restatement_is_the_convolution():
    W, images, _, _, _ = case("s64_l2_n3")
    conv = torch.nn.functional.conv2d(cr.normalise(images).to(F64), W["conv1.weight"].to(F64), stride=32)   # [N, 768, G, G]
    want = conv.flatten(2).transpose(1, 2).reshape(-1, 768)
    got = cr.patch_rows(images).to(F64) @ W["conv1.weight"].to(F64).reshape(768, -1).T
    assert cr.rel_l2(got, want) <= 1e-12


def test_clockwise_slots_is_the_reference_permutation():
    views = [torch.full((3, 2), float(a)) + torch.arange(3).view(3, 1) * 100 for a in range(12)]
    out = cr.clockwise_slots(views)
    for a in range(12):
        for b in range(3):
            assert float(out[(12 - a) % 12 + 12 * b, 0]) == a + 100 * b


def test_quick_gelu_bound_arithmetic():
    v = cr.qgelu_values(4096)
    ref = cr.qgelu_reference(v)
    assert torch.isnan(ref[5]) and ref[4] == float("inf") and ref[0] == 0
    assert torch.equal(torch.isnan(ref), torch.isnan(v * torch.sigmoid(1.702 * v)))           # torch's fp32 agrees on where NaN is
    fin = torch.isfinite(ref)
    b = cr.qgelu_bound(v, ref, False)
    # an fp32 emulation of the kernel's chain with exact exp / reciprocal stays inside the bound; a tanh-GELU does not
    t = torch.tensor(1.702, dtype=torch.float32) * v
    emu = v * (1 / (1 + torch.exp2(t * torch.tensor(-1.4426950408889634, dtype=torch.float32))))
    assert bool(((emu.to(F64) - ref).abs()[fin] <= b[fin]).all())
    wrong = torch.nn.functional.gelu(v, approximate="tanh")
    assert bool(((wrong.to(F64) - ref).abs()[fin] > b[fin]).any())
    assert float(ref[fin].min()) == pytest.approx(float(ref[6]), abs=1e-6)                    # the planted minimum is the minimum
