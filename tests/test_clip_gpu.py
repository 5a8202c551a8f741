"""The native CLIP ViT-B/32 view encoder on an MI355X: the four kernels of etpnav_amd/csrc/clip.hip at operator level and the engine of
csrc/clip_engine.hip through etpnav_amd.clip.CLIPEncoder, against tests/clip_ref.py (float64; pinned to transformers and to the fixture by
tests/test_clip_ref_cpu.py).

  patch rows   fp32 bit for bit against torch's CPU fp32 (x.float() / 255 - mean) / std, bf16 = its round-to-nearest-even, every byte
               value in every channel, the clockwise slot permutation against the reference loop, guards, NaN pre-fill, second run
  tokens, cls  every element inside reduce_ref.ln_fwd_bounds on the kernels' row schedule (no multiplier); an all-equal row gives beta
  QuickGELU    every element inside clip_ref.qgelu_bound (the instruction forms' roundings); NaN exactly at -inf, +inf at +inf
  engine fp32  |y - y64| <= 2e-4 max|y64| (the project's fp32 whole-model bound), for the embeddings and the three residual probes
  engine bf16  per-image relative L2 against float64 <= 2 x the bf16-autocast gap of transformers' model recorded in the fixture
  all engine   second run bit-identical, scratch of exactly etp_clip_ws_bytes between sentinels, stale / refreshed bf16 shadow,
               waypoint_mode with encode_views == forward on the reference's hand-built rgb_batch

ETP_CLIP_BOUNDS_OUT=<path> writes the worst observed ratios there (profiles/clip_op_bounds.txt is such a file, from an MI355X)."""
import atexit
import os
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from etpnav_amd import _lib
from etpnav_amd import clip as cl
from tests import clip_ref as cr
from tests import reduce_ref as rr
from tests.reduce_ref import Guarded, gptr

pytestmark = pytest.mark.gpu
DEV = "cuda"
F64 = torch.float64
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "clip_small.npz")
DT = {"f32": torch.float32, "bf16": torch.bfloat16}
FP32_MODEL_BOUND = 2e-4
WORST = {}


def record(key, ratio):
    WORST[key] = max(WORST.get(key, 0.0), float(ratio))


@atexit.register
def _write_worst():
    dst = os.environ.get("ETP_CLIP_BOUNDS_OUT")
    if dst and WORST:
        with open(dst, "w") as f:
            f.write("CLIP view encoder: worst observed error / bound per check (tests/test_clip_gpu.py)\n")
            for k in sorted(WORST):
                f.write(f"  {k:<64}{WORST[k]:10.4f}\n")


def sync():
    torch.cuda.synchronize()


# ---- patch rows ----------------------------------------------------------------------------------------------------------------
def images_with_every_byte(n, S, seed):
    im = cr.make_images(n, S, seed)
    flat = im[0].view(-1, 3)
    for c in range(3):
        flat[c:c + 256, c] = torch.arange(256, dtype=torch.uint8)
    for c in range(3):
        assert len(set(im[..., c].flatten().tolist())) == 256
    return im


def run_patch_rows(views_dev, want):
    for name, dt in DT.items():
        exp = want if dt == torch.float32 else rr.bf16_rne(want)
        runs = []
        for _ in range(2):
            g = Guarded(tuple(want.shape), dtype=dt)
            assert bool(torch.isnan(g.t.float()).all())
            cl.patch_rows(views_dev, g.t)
            sync()
            g.check("patch_rows " + name)
            rr.same_bits("patch_rows " + name, g.t.cpu(), exp)
            runs.append(g.t.clone())
        rr.same_bits("patch_rows second run " + name, runs[0], runs[1])


@pytest.mark.parametrize("S", [32, 64, 224])
@pytest.mark.parametrize("N", [1, 3, 13])
def test_patch_rows_single_tensor(S, N):
    im = images_with_every_byte(N, S, 10 + N)
    dev = im.to(DEV)
    run_patch_rows(dev, cr.patch_rows(im))
    assert torch.equal(dev.cpu(), im)


@pytest.mark.parametrize("S", [32, 64, 224])
@pytest.mark.parametrize("B", [1, 3])
def test_patch_rows_twelve_views_clockwise(S, B):
    views = [cr.make_images(B, S, 20 + B, name=f"view{a}") for a in range(12)]
    views[0] = images_with_every_byte(B, S, 20 + B)
    want = cr.patch_rows(cr.clockwise_slots(views))
    # the permutation itself, on the painted slot of every view: view a of episode b lands in image (12 - a) % 12 + 12 b
    P = (S // 32) ** 2
    for a in (0, 1, 11):
        for b in range(B):
            assert torch.equal(want[((12 - a) % 12 + 12 * b) * P:((12 - a) % 12 + 12 * b + 1) * P], cr.patch_rows(views[a][b:b + 1]))
    run_patch_rows([v.to(DEV) for v in views], want)


# ---- tokens and class-token LayerNorm ---------------------------------------------------------------------------------------------
def ln_params(seed):
    g = (1 + 0.1 * cr.hash_uniform("g", seed, (768,))).float()
    b = (0.02 * cr.hash_uniform("b", seed, (768,))).float()
    return g, b


@pytest.mark.parametrize("S", [32, 64, 224])          # T = 2, 5, 50
@pytest.mark.parametrize("N", [1, 3, 13])
def test_tokens(S, N):
    T = (S // 32) ** 2 + 1
    prod = cr.hash_uniform("prod", N, (N * (T - 1), 768)).float()
    cls = (0.02 * cr.hash_uniform("cls", N, (768,))).float()
    pos = (0.02 * cr.hash_uniform("pos", N, (T, 768))).float()
    prod[0], pos[1] = 0.5, 0.0                        # row 1 of image 0 is all-equal: its LayerNorm is exactly beta
    g, b = ln_params(N)
    ref, bound = cr.tokens_reference(prod, cls, pos, g, b, N, T)
    d = [t.to(DEV) for t in (prod, cls, pos, g, b)]
    runs = []
    for _ in range(2):
        x = Guarded((N * T, 768))
        cl.tokens(*d, x.t, N, S)
        sync()
        x.check("tokens")
        record("clip_tokens", rr.within(("etp_clip_tokens", f"S{S}"), x.t.cpu(), ref, bound))
        rr.same_bits("tokens: all-equal row", x.t[1].cpu(), b)
        runs.append(x.t.clone())
    rr.same_bits("tokens second run", runs[0], runs[1])
    for t, t0 in zip(d, (prod, cls, pos, g, b)):
        assert torch.equal(t.cpu(), t0)


@pytest.mark.parametrize("S", [32, 64, 224])
@pytest.mark.parametrize("N", [1, 3, 13])
@pytest.mark.parametrize("dt", ["f32", "bf16"])
def test_cls_ln(S, N, dt):
    T = (S // 32) ** 2 + 1
    x = (3 * cr.hash_uniform("x", N, (N * T, 768))).float()
    x[0] = 0.5
    g, b = ln_params(N + 7)
    ref, bound = cr.cls_ln_reference(x, g, b, N, T, dt == "bf16")
    xd, gd, bd = x.to(DEV), g.to(DEV), b.to(DEV)
    runs = []
    for _ in range(2):
        out = Guarded((N, 768), dtype=DT[dt])
        cl.cls_ln(xd, gd, bd, out.t, N, S)
        sync()
        out.check("cls_ln")
        record("clip_cls_ln " + dt, rr.within(("etp_clip_cls_ln", dt), out.t.cpu(), ref, bound))
        rr.same_bits("cls_ln: all-equal row", out.t[0].cpu(), b if dt == "f32" else rr.bf16_rne(b))
        runs.append(out.t.clone())
    rr.same_bits("cls_ln second run", runs[0], runs[1])
    assert torch.equal(xd.cpu(), x)


# ---- QuickGELU ---------------------------------------------------------------------------------------------------------------------
GRID_CAP_ELEMS = 2048 * 256 * 8                       # one trip of the capped grid (clip.hip CLIP_GRID_CAP)


@pytest.mark.parametrize("n", [8, 3072, 3072 * 7, 2 * GRID_CAP_ELEMS + 1032])
@pytest.mark.parametrize("dt", ["f32", "bf16"])
def test_quick_gelu(n, dt):
    v = cr.qgelu_values(n).to(DT[dt])
    if n > 8:
        v[-1], v[n // 2] = -30.0, 30.0
    ref = cr.qgelu_reference(v)
    bound = cr.qgelu_bound(v, ref, dt == "bf16")
    runs = []
    for _ in range(2):
        g = Guarded((n,), dtype=DT[dt], init=v.to(DEV))
        cl.quick_gelu(g.t)
        sync()
        g.check("quick_gelu")
        got = g.t.cpu()
        assert torch.equal(torch.isnan(got.float()), v.float() == float("-inf")), "NaN exactly at -inf"
        assert bool((got.float()[v.float() == float("inf")] == float("inf")).all())
        fin = torch.isfinite(ref)
        record("quick_gelu " + dt, rr.within(("etp_quick_gelu", dt), got[fin], ref[fin], bound[fin]))
        runs.append(g.t.clone())
    same = runs[0].view(torch.int16 if dt == "bf16" else torch.int32) == runs[1].view(torch.int16 if dt == "bf16" else torch.int32)
    assert bool(same.all())


# ---- engine --------------------------------------------------------------------------------------------------------------------------
_REF = {}


def reference(S, layers, n, seed=cr.CASE_SEED):
    """weights, images, float64 embeddings and probes; computed once, shared, never modified"""
    key = (S, layers, n, seed)
    if key not in _REF:
        W = cr.make_weights(S, layers, seed)
        images = cr.make_images(n, S, seed)
        y, probes = cr.forward(W, images, layers)
        _REF[key] = (W, images, y, probes)
    return _REF[key]


def encoder(S, layers, dtype, W):
    enc = cl.CLIPEncoder(device=DEV, dtype=dtype, image_size=S, layers=layers)
    enc.load_state_dict(W, strict=True)
    return enc


def sentinel_scratch(enc, N):
    """install scratch of exactly etp_clip_ws_bytes(N) for N images between two 256-byte sentinels"""
    nbytes = int(enc.L.etp_clip_ws_bytes(enc.handle, N))
    buf = torch.full((nbytes + 1024,), 0xA5, dtype=torch.uint8, device=DEV)
    off = (-buf.data_ptr()) % 256 + 256
    enc._ws[N] = buf[off:off + nbytes]

    def check():
        assert bool((buf[:off] == 0xA5).all()) and bool((buf[off + nbytes:] == 0xA5).all()), "scratch sentinels overwritten"
    return check


def run_fp32(S, layers, N, views=None):
    W, images, y, probes = reference(S, layers, N)
    enc = encoder(S, layers, torch.float32, W)
    check = sentinel_scratch(enc, N)
    probe = enc.set_probe(True, N)
    if views is None:
        call = lambda: enc({"rgb": images.to(DEV)})
    else:
        call = lambda: enc.encode_views(views)
    got = call()
    sync()
    check()
    tag = f"S{S} L{layers}"
    err = float((got.cpu().to(F64) - y).abs().max()) / (FP32_MODEL_BOUND * float(y.abs().max()))
    record(f"engine fp32 {tag} embeddings", err)
    assert err <= 1.0, (tag, N, err)
    assert bool(torch.isfinite(got).all())
    for i, name in enumerate(("ln_pre", "layer 0", "last layer")):
        e = float((probe[i].cpu().to(F64) - probes[i]).abs().max()) / (FP32_MODEL_BOUND * float(probes[i].abs().max()))
        record(f"engine fp32 {tag} probe {name}", e)
        assert e <= 1.0, (tag, N, name, e)
    enc.set_probe(False)
    again = call()
    sync()
    check()
    rr.same_bits("engine fp32 second run", got, again)
    return enc, got


@pytest.mark.parametrize("S,layers", [(32, 1), (64, 2), (96, 2)])
@pytest.mark.parametrize("N", [1, 5, 13])
def test_engine_fp32_small(S, layers, N):
    run_fp32(S, layers, N)


def test_engine_fp32_full_size_one_layer():
    run_fp32(224, 1, 3)


def split_views(images):
    """the inverse of the reference loop: 12 view tensors whose clockwise batch is `images` [12 B, ...]"""
    return {("rgb" if a == 0 else f"rgb_{a * 30.0}"): images[(12 - a) % 12::12].contiguous().to(DEV) for a in range(12)}


def test_engine_fp32_vit_b32_through_encode_views():
    W, images, y, probes = reference(224, 12, 12)
    obs = split_views(images)
    assert torch.equal(cr.clockwise_slots([obs[k].cpu() for k in obs]), images)
    run_fp32(224, 12, 12, views=obs)


@pytest.mark.parametrize("name", list(cr.GOLDEN_CASES))
def test_engine_bf16_within_twice_the_autocast_gap(name):
    S, layers, n = cr.GOLDEN_CASES[name]
    g = np.load(GOLDEN)
    gap, y = float(g[f"{name}/bf16_gap"]), torch.from_numpy(g[f"{name}/emb"])
    W, images, y_ref, _ = reference(S, layers, n)
    assert cr.rel_l2(y_ref, y) <= 1e-10
    enc = encoder(S, layers, torch.bfloat16, W)
    check = sentinel_scratch(enc, n)
    got = enc({"rgb": images.to(DEV)})
    sync()
    check()
    for i in range(n):
        r = cr.rel_l2(got[i].cpu(), y[i]) / (2 * gap)
        print(f"{name} image {i}: rel L2 {cr.rel_l2(got[i].cpu(), y[i]):.3e}, 2 x gap {2 * gap:.3e}")
        record(f"engine bf16 {name} rel L2 / (2 x autocast gap)", r)
        assert r <= 1.0, (name, i, r)
    again = enc({"rgb": images.to(DEV)})
    sync()
    rr.same_bits("engine bf16 second run", got, again)


@pytest.mark.parametrize("N", [1, 5, 13])
def test_engine_bf16_small_batches(N):
    """the same bound at the batch sizes of the fp32 cases, against the fixture's gap of the (64, 2) case"""
    gap = float(np.load(GOLDEN)["s64_l2_n3/bf16_gap"])
    W, images, y, _ = reference(64, 2, N)
    enc = encoder(64, 2, torch.bfloat16, W)
    check = sentinel_scratch(enc, N)
    got = enc({"rgb": images.to(DEV)})
    sync()
    check()
    for i in range(N):
        r = cr.rel_l2(got[i].cpu(), y[i]) / (2 * gap)
        record("engine bf16 S64 L2 batches rel L2 / (2 x autocast gap)", r)
        assert r <= 1.0, (N, i, r)
    rr.same_bits("engine bf16 second run", got, enc({"rgb": images.to(DEV)}))


def test_weight_edit_needs_and_gets_a_shadow_refresh():
    W, images, _, _ = reference(64, 2, 3)
    enc = encoder(64, 2, torch.bfloat16, W)
    dev = images.to(DEV)
    y0 = enc({"rgb": dev}).clone()
    enc.proj.data.mul_(2.0)                      # behind the version counter's back: the bf16 shadow is stale
    y1 = enc({"rgb": dev}).clone()
    rr.same_bits("stale shadow", y0, y1)
    enc.refresh_weights()
    y2 = enc({"rgb": dev}).clone()
    rr.same_bits("refreshed shadow (a factor 2 is exact)", y2, 2 * y0)
    with torch.no_grad():
        enc.proj.mul_(0.5)                       # a tracked edit refreshes by itself
    rr.same_bits("tracked edit", enc({"rgb": dev}), y0)
    f = encoder(64, 2, torch.float32, W)         # fp32 mode has no shadow: an edit acts at once
    z0 = f({"rgb": dev}).clone()
    f.ln_post.bias.data.add_(1.0)
    assert not torch.equal(f({"rgb": dev}), z0)


class _ForwardOnly(torch.nn.Module):
    """an encoder with forward alone, as the reference's CLIPEncoder is"""

    def __init__(self, enc):
        super().__init__()
        self._enc = [enc]

    def forward(self, observations):
        return self._enc[0](observations)


def test_waypoint_mode_uses_encode_views_and_gives_forwards_bits():
    from etpnav_amd import waypoint as wp
    from etpnav_amd.policy import ETP
    from tests import waypoint_ref as wr
    B, S = 2, 64
    W, images, _, _ = reference(S, 2, 12 * B)
    enc = encoder(S, 2, torch.bfloat16, W)
    obs = {}
    for a in range(12):                          # the rollout's key order: rgb, depth, rgb_30.0, depth_30.0, ...
        suffix = "" if a == 0 else f"_{a * 30.0}"
        obs["rgb" + suffix] = images[(12 - a) % 12::12].contiguous().to(DEV)
        obs["depth" + suffix] = torch.full((B, 4, 4, 1), float(a), device=DEV)
    net = ETP(model_config=SimpleNamespace(task_type="r2r"), dtype=torch.float32, device=DEV).eval()
    net.depth_encoder = lambda o: torch.zeros(o["depth"].shape[0], 128, 4, 4, device=DEV)
    pred = wp.BinaryDistPredictorTRM(device=DEV, dtype=torch.float32)
    pred.load_state_dict(wr.make_weights(2), strict=True)
    calls = []
    real = enc.encode_views
    enc.encode_views = lambda o: (calls.append(1), real(o))[1]
    net.rgb_encoder = enc
    native = wp.waypoint_mode(net, pred, obs, False)
    assert calls == [1]
    net.rgb_encoder = _ForwardOnly(enc)          # no encode_views: the unchanged path builds rgb_batch by hand and calls forward
    assert not hasattr(net.rgb_encoder, "encode_views")
    by_hand = wp.waypoint_mode(net, pred, obs, False)
    assert calls == [1]
    rr.same_bits("pano_rgb", native["pano_rgb"], by_hand["pano_rgb"])
    direct = enc({"rgb": images.to(DEV)}).reshape(B, 12, 512)
    ccw = torch.cat((direct[:, 0:1], torch.flip(direct[:, 1:], [1])), 1)
    rr.same_bits("pano_rgb is forward on the clockwise batch, flipped back", native["pano_rgb"], ccw)
    for a, b in zip(native["cand_rgb"], by_hand["cand_rgb"]):
        rr.same_bits("cand_rgb", a, b)
