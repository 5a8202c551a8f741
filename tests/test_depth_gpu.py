"""The native DD-PPO ResNet depth encoder on an MI355X: the kernels of etpnav_amd/csrc/depth.hip at operator level and the engine of
csrc/depth_engine.hip through etpnav_amd.depth.DepthEncoder, against tests/depth_ref.py (float64; pinned to the torch module and to the
fixture by tests/test_depth_ref_cpu.py).

  stem         every element inside gam(52) sum |w| |pooled| (the tap order's bound, no multiplier), borders included, both input forms,
               guards, NaN pre-fill, second run bit-identical
  rows, pool   bit for bit, both dtypes, NaN pre-fill between guards
  GroupNorm    statistics inside depth_ref.stats_bounds, apply inside gam(4) (|x - m| r |g| + |b|) per branch with the kernel's own
               statistics; |mean| = 1e3 std; a constant group gives beta exactly; every residual form x ReLU x layout; bf16 output =
               round-to-nearest-even of the fp32 output, bit for bit
  engine fp32  max |y - y64| <= 4 x the fixture's fp32 gap x max |y64| (the gap is one draw of a valid fp32 order, the engine's tile
               order another; the CPU test keeps planted mistakes >= 100 x above this), the three probes under the same rule
  engine bf16  relative L2 against float64 <= 2 x the module's bf16-autocast gap recorded in the fixture
  all engine   second run bit-identical, scratch of exactly etp_depth_ws_bytes between sentinels, stale / refreshed packed weights,
               waypoint_mode with encode_views == forward on the reference's hand-built depth_batch

ETP_DEPTH_BOUNDS_OUT=<path> writes the worst observed ratios there (profiles/depth_op_bounds.txt is such a file, from an MI355X)."""
import atexit
import os
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from etpnav_amd import depth as dp
from tests import depth_ref as dr
from tests import reduce_ref as rr
from tests.reduce_ref import Guarded

pytestmark = pytest.mark.gpu
DEV = "cuda"
F64 = torch.float64
U = rr.U
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "depth_small.npz")
DT = {"f32": torch.float32, "bf16": torch.bfloat16}
WORST = {}


def record(key, ratio):
    WORST[key] = max(WORST.get(key, 0.0), float(ratio))


@atexit.register
def _write_worst():
    dst = os.environ.get("ETP_DEPTH_BOUNDS_OUT")
    if dst and WORST:
        with open(dst, "w") as f:
            f.write("DD-PPO ResNet depth encoder: worst observed error / bound per check (tests/test_depth_gpu.py)\n")
            for k in sorted(WORST):
                f.write(f"  {k:<64}{WORST[k]:10.4f}\n")


def sync():
    torch.cuda.synchronize()


def within(key, got, ref, bound):
    record(key, rr.within((key, ""), got.cpu(), ref, bound))


# ---- stem ------------------------------------------------------------------------------------------------------------------------------
def stem_weight(bp):
    return (dr.make_weights(64, bp, (1, 1, 1, 1), 4)["backbone.conv1.0.weight"] * 20.0).contiguous()        # O(1) taps


def run_stem(views_dev, batch, w):
    """views_dev: a tensor or 12 of them on the device; batch: the clockwise [N, S, S, 1] they stand for (CPU)"""
    N, S, bp = batch.shape[0], batch.shape[1], w.shape[0]
    ref = dr.conv(dr.pool2(batch.to(F64)), w.to(F64), 2)
    out = Guarded((N, S // 4, S // 4, bp))
    wd = w.to(DEV)
    dp.stem(views_dev, wd, out.t)
    sync()
    out.check("stem")
    within(f"stem S{S} bp{bp}", out.t, ref, dr.stem_bound(batch.to(F64), w.to(F64)))
    first = out.t.clone()
    out.t.fill_(float("nan"))
    dp.stem(views_dev, wd, out.t)
    sync()
    rr.same_bits("stem second run", out.t, first)


@pytest.mark.parametrize("S", dr.STEM_S)
@pytest.mark.parametrize("bp", dr.STEM_BP)
@pytest.mark.parametrize("N", dr.STEM_N)
def test_stem_single_tensor(S, bp, N):
    batch = dr.make_depth(20, N, S)
    run_stem(batch.to(DEV), batch, stem_weight(bp))


@pytest.mark.parametrize("S", dr.STEM_S)
@pytest.mark.parametrize("bp", dr.STEM_BP)
@pytest.mark.parametrize("B", dr.STEM_B)
def test_stem_twelve_views_clockwise(S, bp, B):
    views = [dr.make_depth(21, B, S, first=100 * a) for a in range(12)]
    run_stem([v.to(DEV) for v in views], dr.clockwise(views), stem_weight(bp))


# ---- conv_rows, max-pool ---------------------------------------------------------------------------------------------------------------
def signed_input(N, H, C, seed, dtype):
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(N, H, H, C, generator=g) - 0.5).to(dtype)            # mostly negative windows: padding must never win


@pytest.mark.parametrize("H", dr.ROWS_HW)
@pytest.mark.parametrize("k,stride", dr.ROWS_KS)
@pytest.mark.parametrize("N", dr.ROWS_N)
def test_conv_rows_bit_for_bit(H, k, stride, N):
    for C in dr.ROWS_C:
        for name, dtype in DT.items():
            x = signed_input(N, H, C, H * 7 + C + k, dtype)
            want, Ho, Wo = dr.rows(x, k, stride)
            out = Guarded((N * Ho * Wo, k * k * C), dtype=dtype)
            dp.conv_rows(x.to(DEV), out.t, k, stride)
            sync()
            out.check("conv_rows")
            rr.same_bits(f"conv_rows {name} H{H} C{C} k{k} s{stride}", out.t.cpu(), want.contiguous())


@pytest.mark.parametrize("H", dr.ROWS_HW)
@pytest.mark.parametrize("N", dr.ROWS_N)
def test_maxpool_bit_for_bit(H, N):
    for C in dr.ROWS_C:
        for name, dtype in DT.items():
            x = signed_input(N, H, C, H * 11 + C, dtype)
            want = dr.maxpool(x.float()).to(dtype)
            out = Guarded(tuple(want.shape), dtype=dtype)
            dp.maxpool3x3s2(x.to(DEV), out.t)
            sync()
            out.check("maxpool")
            rr.same_bits(f"maxpool {name} H{H} C{C}", out.t.cpu(), want.contiguous())


# ---- GroupNorm -------------------------------------------------------------------------------------------------------------------------
def gn_input(N, HW, C, seed, offset=0.0):
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(N, HW, C, generator=g) * (0.5 + torch.rand(N, 1, C, generator=g)) + torch.randn(N, 1, C, generator=g) + offset
    return x.to(torch.float32)


def affine(C, seed):
    g = torch.Generator().manual_seed(seed)
    return (1.0 + 0.3 * torch.randn(C, generator=g)).float(), (0.2 * torch.randn(C, generator=g)).float()


def check_stats(tag, x, G):
    xd = x.to(DEV)
    got = dp.gn_stats(xd, G)
    sync()
    mean, rstd, dm, drs = dr.stats_bounds(x.to(F64), G)
    within(f"gn_stats mean {tag}", got[..., 0], mean, dm)
    within(f"gn_stats rstd {tag}", got[..., 1], rstd, drs)
    rr.same_bits("gn_stats second run", dp.gn_stats(xd, G), got)
    return xd, got


@pytest.mark.parametrize("HW", dr.GN_HW)
@pytest.mark.parametrize("C", dr.GN_C)
def test_group_norm_stats_and_apply(HW, C):
    """every group count x every N of depth_ref.gn_cases for this (HW, C): the full cross product, N = 13 left out where HW C >= 2^20"""
    for (hw, c, G, N) in dr.gn_cases():
        if (hw, c) != (HW, C):
            continue
        x = gn_input(N, HW, C, 31 + HW + C + G + N)
        xd, stats = check_stats("cases", x, G)
        gamma, beta = affine(C, C + G)
        y, bound = dr.apply_ref(x.to(F64), stats.cpu().to(F64), gamma.to(F64), beta.to(F64))
        out = Guarded((N, HW, C))
        dp.gn_apply(xd, stats, gamma.to(DEV), beta.to(DEV), out.t, relu=True)
        sync()
        out.check("gn_apply")
        within("gn_apply fp32 relu", out.t, torch.relu(y), bound)
        lo = Guarded((N, HW, C), dtype=torch.bfloat16)
        dp.gn_apply(xd, stats, gamma.to(DEV), beta.to(DEV), lo.t, relu=True)
        sync()
        lo.check("gn_apply bf16")
        rr.same_bits("gn_apply bf16 = RNE(fp32)", lo.t.cpu(), rr.bf16_rne(out.t.cpu()))


def test_group_norm_large_mean_and_constant_group():
    """|mean| = 1e3 std: the two-pass statistics hold their bound where E[x^2] - E[x]^2 (emulated on the CPU, same summation schedule)
    does not; a constant group comes out as exactly beta."""
    N, HW, C, G = 3, 1024, 32, 16
    g = torch.Generator().manual_seed(3)
    x = (1000.0 + torch.randn(N, HW, C, generator=g)).to(torch.float32)
    x[:, :, 6:8] = 0.1                                                     # group 3 is constant
    x[1, :, 20:22] = -1234.5678                                            # group 10 of image 1 too
    xd, stats = check_stats("mean = 1e3 std", x, G)
    mean, rstd, dm, drs = dr.stats_bounds(x[:1].to(F64), G)
    one = dr.emulate_stats(x[:1], G, one_pass=True).to(F64)
    assert bool(((one[..., 1] - rstd).abs() > drs).any()), "the one-pass variance was expected to miss the bound here"
    gamma, beta = affine(C, 5)
    out = torch.full((N, HW, C), float("nan"), device=DEV)
    dp.gn_apply(xd, stats, gamma.to(DEV), beta.to(DEV), out)
    got = out.cpu()
    rr.same_bits("constant group = beta", got[:, :, 6:8], beta[6:8].expand(N, HW, 2).contiguous())
    rr.same_bits("constant group = beta", got[1, :, 20:22], beta[20:22].expand(HW, 2).contiguous())
    assert float(stats[0, 3, 0]) == float(x[0, 0, 6]) and float(stats[0, 3, 1]) == float(np.float32(1.0) / np.sqrt(np.float32(1e-5)))


@pytest.mark.parametrize("res", ["none", "finished", "prenorm"])
@pytest.mark.parametrize("relu", [False, True])
@pytest.mark.parametrize("nchw", [False, True])
def test_group_norm_apply_residual_forms(res, relu, nchw):
    for (N, HW, C, G) in ((3, 49, 32, 16), (1, 16, 128, 8), (2, 4, 2048, 1)):
        x, x2 = gn_input(N, HW, C, 41), gn_input(N, HW, C, 42, offset=0.5)
        gamma, beta = affine(C, 43)
        gamma2, beta2 = affine(C, 44)
        xd, x2d = x.to(DEV), x2.to(DEV)
        st, st2 = dp.gn_stats(xd, G), dp.gn_stats(x2d, G)
        y, bound = dr.apply_ref(x.to(F64), st.cpu().to(F64), gamma.to(F64), beta.to(F64))
        fin = rr.bf16_rne(gn_input(N, HW, C, 45)).float()                                      # representable in both dtypes
        results = {}
        for name, dtype in DT.items():
            kw = {}
            want, wb = y, bound
            if res == "finished":
                kw = dict(res=fin.to(dtype).to(DEV))
                want, wb = y + fin.to(F64), bound * (1 + U) + U * (y + fin.to(F64)).abs()
            elif res == "prenorm":
                kw = dict(res=x2d, res_stats=st2, res_gamma=gamma2.to(DEV), res_beta=beta2.to(DEV))
                y2, b2 = dr.apply_ref(x2.to(F64), st2.cpu().to(F64), gamma2.to(F64), beta2.to(F64))
                want, wb = y + y2, (bound + b2) * (1 + U) + U * (y + y2).abs()
            if relu:
                want = torch.relu(want)
            if nchw:
                if name == "bf16" and res != "finished":
                    continue                                                                    # the NCHW output is fp32; dtype only types `res`
                out = Guarded((N, C, HW))
                dp.gn_apply(xd, st, gamma.to(DEV), beta.to(DEV), out.t, relu=relu, nchw=True, **kw)
                sync()
                out.check("gn_apply nchw")
                within(f"gn_apply {res} nchw", out.t, want.permute(0, 2, 1).contiguous(), wb.permute(0, 2, 1).contiguous())
                results[name] = out.t.cpu()
            else:
                out = Guarded((N, HW, C), dtype=dtype)
                dp.gn_apply(xd, st, gamma.to(DEV), beta.to(DEV), out.t, relu=relu, **kw)
                sync()
                out.check("gn_apply nhwc")
                if name == "f32":
                    within(f"gn_apply {res} nhwc", out.t, want, wb)
                results[name] = out.t.cpu()
        if len(results) == 2 and not nchw:
            rr.same_bits("bf16 = RNE(fp32)", results["bf16"], rr.bf16_rne(results["f32"]))
        if len(results) == 2 and nchw:
            rr.same_bits("nchw fp32 output whatever types the residual", results["bf16"], results["f32"])


# ---- engine ----------------------------------------------------------------------------------------------------------------------------
_REF = {}


def fixture():
    if "fx" not in _REF:
        _REF["fx"] = np.load(GOLDEN)
    return _REF["fx"]


def reference(ci, with_probes=True):
    """-> (W, depth [n], y64 [n] from the fixture, probes of the float64 restatement or None, fp32 gap, bf16 gap), computed once"""
    key = (ci, with_probes)
    if key not in _REF:
        fx = fixture()
        S, bp, blocks = dr.ALL_CASES[ci]
        n = int(fx[f"case_{ci}"][-1])
        W = dr.make_weights(S, bp, blocks, int(fx[f"seeds_{ci}"][0]))
        depth = dr.make_depth(int(fx[f"seeds_{ci}"][1]), n, S)
        probes = None
        if with_probes:
            probes = []
            y = dr.forward64(W, depth[:dr.FULL_N if ci == 3 else n], bp, blocks, probes=probes)
            assert float((y - torch.from_numpy(fx[f"y64_{ci}"][:y.shape[0]])).abs().max()) <= 1e-10 * float(y.abs().max())
        _REF[key] = (W, depth, torch.from_numpy(fx[f"y64_{ci}"]), probes, float(fx[f"gap_fp32_{ci}"]), float(fx[f"gap_bf16_{ci}"]))
    return _REF[key]


def encoder(ci, dtype, W):
    S, bp, blocks = dr.ALL_CASES[ci]
    enc = dp.DepthEncoder(device=DEV, dtype=dtype, image_size=S, base_planes=bp, blocks=blocks)
    enc.load_state_dict(W, strict=True)
    return enc


def sentinel_scratch(enc, N):
    """install scratch of exactly etp_depth_ws_bytes(N) for N images between two 256-byte sentinels"""
    nbytes = int(enc.L.etp_depth_ws_bytes(enc.handle, N))
    buf = torch.full((nbytes + 1024,), 0xA5, dtype=torch.uint8, device=DEV)
    off = (-buf.data_ptr()) % 256 + 256
    enc._ws[N] = buf[off:off + nbytes]

    def check():
        assert bool((buf[:off] == 0xA5).all()) and bool((buf[off + nbytes:] == 0xA5).all()), "scratch sentinels overwritten"
    return check


def split_views(images):
    """the inverse of the reference loop: 12 view tensors whose clockwise batch is `images` [12 B, ...]"""
    return {("depth" if a == 0 else f"depth_{a * 30.0}"): images[(12 - a) % 12::12].contiguous().to(DEV) for a in range(12)}


def run_engine(ci, N, dtype, views=False):
    W, depth, y64, probes, gap32, gapbf = reference(ci, with_probes=not views)
    depth, y = depth[:N], y64[:N]
    enc = encoder(ci, dtype, W)
    check = sentinel_scratch(enc, N)
    use_probes = probes is not None and N <= probes[0].shape[0]
    probe = enc.set_probe(True, N) if use_probes else None
    if views:
        obs = split_views(depth)
        assert torch.equal(dr.clockwise([obs[k].cpu() for k in obs]), depth)
        call = lambda: enc.encode_views(obs)
    else:
        dev = depth.to(DEV)
        call = lambda: enc({"depth": dev})
    got = call()
    sync()
    check()
    assert got.shape == y.shape and got.dtype == torch.float32 and bool(torch.isfinite(got).all())
    tag = f"case {ci} {'views' if views else 'batch'}"
    g = got.cpu().to(F64)
    if dtype == torch.float32:
        err = float((g - y).abs().max() / y.abs().max())
        print(f"engine fp32 {tag} N {N}: max err / max |y| {err:.3e}, 4 x fp32 gap {4 * gap32:.3e}")
        if use_probes:
            off = 0
            for name, p, n in zip(("max-pool", "layer1", "layer4"), probes, enc.probe_sizes(N)):
                want = p[:N].reshape(-1)
                e = float((probe[off:off + n].cpu().to(F64) - want).abs().max() / want.abs().max())
                print(f"  probe {name}: max err / max |probe| {e:.3e}")
                record(f"engine fp32 {tag} probe {name} / (4 x fp32 gap)", e / (4 * gap32))
                assert e <= 4 * gap32, (tag, N, name, e, 4 * gap32)
                off += n
        record(f"engine fp32 {tag} / (4 x fp32 gap)", err / (4 * gap32))
        assert err <= 4 * gap32, (tag, N, err, 4 * gap32)
    else:
        rel = float((g - y).norm() / y.norm())
        print(f"engine bf16 {tag} N {N}: rel L2 {rel:.3e}, 2 x autocast gap {2 * gapbf:.3e}")
        record(f"engine bf16 {tag} rel L2 / (2 x autocast gap)", rel / (2 * gapbf))
        assert rel <= 2 * gapbf, (tag, N, rel, 2 * gapbf)
    if use_probes:
        enc.set_probe(False)
    again = call()
    sync()
    check()
    rr.same_bits("engine second run", got, again)
    return enc


@pytest.mark.parametrize("ci", range(len(dr.ENGINE_CASES)))
@pytest.mark.parametrize("N", dr.ENGINE_NS)
def test_engine_fp32_small(ci, N):
    run_engine(ci, N, torch.float32)


def test_engine_fp32_image_size_192():
    """3 x 3 maps, 6 x 6 stem tiles, Cc = 228: the one product whose N is no multiple of 8"""
    run_engine(4, dr.CASE_192_N, torch.float32)


def test_engine_bf16_image_size_192():
    run_engine(4, dr.CASE_192_N, torch.bfloat16)


def test_engine_fp32_full_network():
    run_engine(3, dr.FULL_N, torch.float32)


def test_engine_fp32_full_network_through_encode_views():
    run_engine(3, dr.NUM_IMGS, torch.float32, views=True)


@pytest.mark.parametrize("ci", range(len(dr.ENGINE_CASES)))
@pytest.mark.parametrize("N", dr.ENGINE_NS)
def test_engine_bf16_within_twice_the_autocast_gap(ci, N):
    run_engine(ci, N, torch.bfloat16)


def test_engine_bf16_full_network():
    run_engine(3, dr.FULL_N, torch.bfloat16)


def test_engine_bf16_full_network_through_encode_views():
    run_engine(3, dr.NUM_IMGS, torch.bfloat16, views=True)


@pytest.mark.parametrize("dt", ["f32", "bf16"])
def test_weight_edit_needs_and_gets_a_refresh_of_the_packed_copy(dt):
    W, depth, _, _, _, _ = reference(1)
    enc = encoder(1, DT[dt], W)
    dev = depth[:3].to(DEV)
    p = dict(enc.named_parameters())["compression.0.weight"]
    y0 = enc({"depth": dev}).clone()
    p.data.neg_()                                 # behind the version counter's back: the packed copy is stale
    rr.same_bits("stale packed copy", enc({"depth": dev}), y0)
    enc.refresh_weights()
    assert not torch.equal(enc({"depth": dev}), y0)
    with torch.no_grad():
        p.neg_()                                  # a tracked edit is detected and refreshes by itself
    rr.same_bits("tracked edit", enc({"depth": dev}), y0)
    dict(enc.named_parameters())["compression.1.bias"].data.add_(1.0)      # GroupNorm parameters are read from the arena: at once
    assert not torch.equal(enc({"depth": dev}), y0)


class _ForwardOnly(torch.nn.Module):
    """an encoder with forward alone, as the reference's VlnResnetDepthEncoder is"""

    def __init__(self, enc):
        super().__init__()
        self._enc = [enc]

    def forward(self, observations):
        return self._enc[0](observations)


def test_waypoint_mode_uses_encode_views_and_gives_forwards_bits():
    from etpnav_amd import waypoint as wp
    from etpnav_amd.policy import ETP
    from tests import waypoint_ref as wr
    B = 2
    W, depth, _, _, _, _ = reference(3, with_probes=False)
    S = depth.shape[1]
    images = torch.cat([depth, depth.flip(1)])                      # 24 clockwise images: 2 episodes
    enc = encoder(3, torch.bfloat16, W)
    obs = {}
    for a in range(12):                          # the rollout's key order: rgb, depth, rgb_30.0, depth_30.0, ...
        suffix = "" if a == 0 else f"_{a * 30.0}"
        obs["rgb" + suffix] = torch.full((B, 4, 4, 3), a, dtype=torch.uint8, device=DEV)
        obs["depth" + suffix] = images[(12 - a) % 12::12].contiguous().to(DEV)
    net = ETP(model_config=SimpleNamespace(task_type="r2r"), dtype=torch.float32, device=DEV).eval()
    net.rgb_encoder = lambda o: torch.zeros(o["rgb"].shape[0], 512, device=DEV)
    pred = wp.BinaryDistPredictorTRM(device=DEV, dtype=torch.float32)
    pred.load_state_dict(wr.make_weights(2), strict=True)
    calls = []
    real = enc.encode_views
    enc.encode_views = lambda o: (calls.append(1), real(o))[1]
    net.depth_encoder = enc
    native = wp.waypoint_mode(net, pred, obs, False)
    assert calls == [1]
    net.depth_encoder = _ForwardOnly(enc)        # no encode_views: the unchanged path builds depth_batch by hand and calls forward
    assert not hasattr(net.depth_encoder, "encode_views")
    by_hand = wp.waypoint_mode(net, pred, obs, False)
    assert calls == [1]
    rr.same_bits("pano_depth", native["pano_depth"], by_hand["pano_depth"])
    direct = enc({"depth": images.to(DEV)}).reshape(B, 12, 128, 4, 4)
    ccw = net.space_pool_depth(torch.cat((direct[:, 0:1], torch.flip(direct[:, 1:], [1])), 1))
    rr.same_bits("pano_depth is forward on the clockwise batch, flipped back and pooled", native["pano_depth"], ccw)
    assert bool((native["pano_depth"] != 0).any())
    for a, b in zip(native["cand_depth"], by_hand["cand_depth"]):
        rr.same_bits("cand_depth", a, b)
    assert len(native["cand_angles"]) == B and native["cand_angles"] == by_hand["cand_angles"]
