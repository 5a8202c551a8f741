"""CPU checks of the depth encoder's yardsticks (tests/depth_ref.py): the float64 NHWC restatement is the torch module (habitat's
architecture, restated) and the committed fixture; the key contract (162 tensors, 7 069 408 parameters, (128, 4, 4)); the DD-PPO key
filter; nine planted mistakes each move the output by at least 100 x the fp32 bound the GPU test uses; and fp32 emulations of the
statistics' and the stem's schedules stay inside the derived bounds on every case the GPU test runs."""
import os

import numpy as np
import pytest
import torch

from tests import depth_ref as dr
from tests import reduce_ref as rr

F64 = torch.float64
FIXTURE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "depth_small.npz")


@pytest.fixture(scope="module")
def fx():
    return np.load(FIXTURE)


@pytest.mark.parametrize("ci", range(len(dr.ENGINE_CASES)))
def test_restatement_is_the_module_and_the_fixture(fx, ci):
    S, bp, blocks = dr.ENGINE_CASES[ci]
    assert tuple(fx[f"case_{ci}"]) == (S, bp, *blocks, dr.ENGINE_N_MAX)
    W = dr.make_weights(S, bp, blocks, int(fx[f"seeds_{ci}"][0]))
    depth = dr.make_depth(int(fx[f"seeds_{ci}"][1]), 3, S)
    with torch.no_grad():
        ym = dr.module_with(W, S, bp, blocks, F64)({"depth": depth.double()})
    y = dr.forward64(W, depth, bp, blocks)
    assert y.shape == ym.shape == (3, *dr.ResNetEncoder(S, bp, blocks).output_shape)
    assert float((y - ym).abs().max()) <= 1e-10 * float(ym.abs().max())
    assert float((y - torch.from_numpy(fx[f"y64_{ci}"][:3])).abs().max()) <= 1e-10 * float(ym.abs().max())
    assert 0 < float(fx[f"gap_fp32_{ci}"]) < 1e-4 and 0 < float(fx[f"gap_bf16_{ci}"]) < 0.2


def test_image_size_192_restatement_is_the_module_and_the_fixture(fx):
    """3 x 3 maps and Cc = 228"""
    S, bp, blocks = dr.CASE_192
    assert tuple(fx["case_4"]) == (S, bp, *blocks, dr.CASE_192_N) and dr.ALL_CASES[4] == dr.CASE_192
    W = dr.make_weights(S, bp, blocks, int(fx["seeds_4"][0]))
    depth = dr.make_depth(int(fx["seeds_4"][1]), dr.CASE_192_N, S)
    with torch.no_grad():
        ym = dr.module_with(W, S, bp, blocks, F64)({"depth": depth.double()})
    y = dr.forward64(W, depth, bp, blocks)
    assert y.shape == ym.shape == (3, 228, 3, 3)
    assert float((y - ym).abs().max()) <= 1e-10 * float(ym.abs().max())
    assert float((y - torch.from_numpy(fx["y64_4"])).abs().max()) <= 1e-10 * float(ym.abs().max())


def test_full_size_restatement_is_the_fixture(fx):
    S, bp, blocks = dr.FULL
    assert tuple(fx["case_3"]) == (S, bp, *blocks, dr.NUM_IMGS)
    W = dr.make_weights(S, bp, blocks, int(fx["seeds_3"][0]))
    y = dr.forward64(W, dr.make_depth(int(fx["seeds_3"][1]), 1, S), bp, blocks)
    want = torch.from_numpy(fx["y64_3"][:1])
    assert y.shape == (1, 128, 4, 4) and float((y - want).abs().max()) <= 1e-10 * float(want.abs().max())


def test_key_contract():
    shapes = dr.param_shapes(*dr.FULL)
    assert len(shapes) == dr.N_TENSORS == 162 and sum(int(np.prod(s)) for _, s in shapes) == dr.N_PARAMS == 7069408
    names = [k for k, _ in shapes]
    assert names[:6] == ["backbone.conv1.0.weight", "backbone.conv1.1.weight", "backbone.conv1.1.bias", "backbone.layer1.0.convs.0.weight",
                         "backbone.layer1.0.convs.1.weight", "backbone.layer1.0.convs.1.bias"]
    assert "backbone.layer1.0.downsample.1.bias" in names and "backbone.layer1.1.downsample.0.weight" not in names
    assert names[-3:] == ["compression.0.weight", "compression.1.weight", "compression.1.bias"]
    d = dict(shapes)
    assert d["backbone.conv1.0.weight"] == (32, 1, 7, 7) and d["backbone.layer4.0.convs.3.weight"] == (256, 256, 3, 3)
    assert d["backbone.layer1.0.downsample.0.weight"] == (128, 32, 1, 1) and d["compression.0.weight"] == (128, 1024, 3, 3)
    with torch.device("meta"):
        assert dr.ResNetEncoder(*dr.FULL).output_shape == (128, 4, 4)


def test_ddppo_key_filter_on_a_synthetic_checkpoint(tmp_path):
    from etpnav_amd import depth as dp
    S, bp, blocks = dr.ENGINE_CASES[1]
    W = dr.make_weights(S, bp, blocks, 5)
    ckpt = dr.ddppo_checkpoint(W)
    m = dp.DepthEncoder(device="cpu", dtype=torch.float32, image_size=S, base_planes=bp, blocks=blocks)
    m.load_ddppo_state_dict(ckpt["state_dict"])
    for k, v in m.state_dict().items():
        assert torch.equal(v, W[k]), k
    # the reference's own filter (resnet_encoders.py:40-47), restated, keeps the same keys
    kept = {}
    for k, v in ckpt["state_dict"].items():
        parts = k.split(".")[2:]
        if parts[0] != "visual_encoder":
            continue
        kept[".".join(parts[1:])] = v
    assert list(kept) == list(m.state_dict())
    short = dict(ckpt["state_dict"])
    del short["actor_critic.net.visual_encoder.compression.1.bias"]
    with pytest.raises(RuntimeError):
        m.load_ddppo_state_dict(short)
    with pytest.raises(KeyError):
        m.load_ddppo_state_dict({"actor_critic.critic.fc.bias": torch.zeros(1)})
    # from_checkpoint reads the file layout of a DD-PPO checkpoint; only the full-size network has one
    Wf = dr.make_weights(*dr.FULL, seed=2)
    path = str(tmp_path / "ddppo.pth")
    torch.save(dr.ddppo_checkpoint(Wf), path)
    full = dp.DepthEncoder.from_checkpoint(path, device="cpu", dtype=torch.float32)
    assert full.output_shape == (128, 4, 4) and torch.equal(full.state_dict()["compression.1.bias"], Wf["compression.1.bias"])


@pytest.mark.parametrize("mut", dr.MUTATIONS)
def test_planted_mutations_are_rejected(fx, mut):
    """each mistake moves the output by >= 100 x the GPU test's fp32 bound (4 x the fixture's fp32 gap, relative to max |y|).  The third
    case has a 2x2 output map, which the layout mistake needs.  Without the average pool the network halves its input one time too few,
    so that mistake is measured on every second pixel of the image: the same shapes, the pool replaced by a subsampling."""
    ci = 2
    S, bp, blocks = dr.ENGINE_CASES[ci]
    W = dr.make_weights(S, bp, blocks, int(fx[f"seeds_{ci}"][0]))
    need = 100 * 4 * float(fx[f"gap_fp32_{ci}"])
    if mut == "views_counter_clockwise":
        views = [dr.make_depth(ci, 1, S, first=a) for a in range(dr.NUM_IMGS)]
        y = dr.forward64(W, dr.clockwise(views), bp, blocks)
        ym = dr.forward64(W, dr.clockwise(views, mut), bp, blocks)
    else:
        depth = dr.make_depth(ci, 3, S)
        y = dr.forward64(W, depth, bp, blocks)
        ym = dr.forward64(W, depth[:, ::2, ::2] if mut == "no_avg_pool" else depth, bp, blocks, mut=mut)
    assert ym.shape == y.shape
    moved = float((ym - y).abs().max() / y.abs().max())
    assert moved >= need, (mut, moved, need)


def _stats_input(HW, C, G, N, seed, offset=0.0):
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(N, HW, C, generator=g) * (0.5 + torch.rand(N, 1, C, generator=g)) + torch.randn(N, 1, C, generator=g) + offset
    return x.to(torch.float32)


@pytest.mark.parametrize("HW", dr.GN_HW)
@pytest.mark.parametrize("C", dr.GN_C)
def test_stats_schedule_emulation_stays_inside_its_bounds(HW, C):
    """every case of the GPU test (depth_ref.gn_cases), at its own N"""
    for (hw, c, G, N) in dr.gn_cases():
        if (hw, c) != (HW, C):
            continue
        x = _stats_input(HW, C, G, N, 11 + C + G + N)
        got = dr.emulate_stats(x, G).to(F64)
        mean, rstd, dm, dr_ = dr.stats_bounds(x.to(F64), G)
        rr.within(("emulate_stats", f"{HW}x{C}/{G}"), got[..., 0], mean, dm)
        rr.within(("emulate_stats", f"{HW}x{C}/{G}"), got[..., 1], rstd, dr_)


def test_one_pass_variance_fails_where_two_passes_hold():
    """|mean| = 1e3 std: E[x^2] - E[x]^2 loses the variance to cancellation (relative error ~ u mean^2 / var = 6 %), the kernel's
    two-pass schedule does not."""
    HW, C, G = 1024, 32, 16
    g = torch.Generator().manual_seed(3)
    x = (1000.0 + torch.randn(2, HW, C, generator=g)).to(torch.float32)
    mean, rstd, dm, dr_ = dr.stats_bounds(x.to(F64), G)
    two = dr.emulate_stats(x, G).to(F64)
    one = dr.emulate_stats(x, G, one_pass=True).to(F64)
    assert bool(((two[..., 1] - rstd).abs() <= dr_).all()) and bool(((two[..., 0] - mean).abs() <= dm).all())
    bad = (one[..., 1] - rstd).abs() > dr_
    assert bool(bad.any()) and float(((one[..., 1] - rstd).abs() / rstd).max()) > 1e-3
    const = torch.full((1, 49, 32), 0.1, dtype=torch.float32)
    s = dr.emulate_stats(const, 16)
    assert bool((s[..., 0] == const[0, 0, 0]).all()) and bool((s[..., 1] == np.float32(1.0) / np.sqrt(np.float32(1e-5))).all())


@pytest.mark.parametrize("S", dr.STEM_S)
@pytest.mark.parametrize("bp", dr.STEM_BP)
def test_stem_schedule_emulation_stays_inside_its_bound(S, bp):
    W = dr.make_weights(S, bp, (1, 1, 1, 1), 4)
    w = W["backbone.conv1.0.weight"] * 20.0          # O(1) taps
    depth = dr.make_depth(9, 3, S)
    got = dr.emulate_stem(depth, w)
    ref = dr.conv(dr.pool2(depth.to(F64)), w.to(F64), 2)
    assert got.shape == ref.shape == (3, S // 4, S // 4, bp)
    rr.within(("emulate_stem", f"{S}/{bp}"), got, ref, dr.stem_bound(depth.to(F64), w.to(F64)))
