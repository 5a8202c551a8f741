"""The native waypoint head on the MI355X: etp_ring_attn_fwd and etp_waypoint_tail against fp64 with derived bounds
(tests/waypoint_ref.py), the engine and ETP.forward(mode='waypoint') against tests/golden/waypoint_small.npz (recorded from the real
reference classes by tools/make_golden_waypoint.py).

etp_ring_attn_fwd: B in {1, 2, 5, 33} (12 .. 396 rows), neighbor in {0, 1, 5}, bf16 and fp32, alpha 0.125, Q | K | V as column blocks
of one [rows, 2304] buffer and as separate buffers; ctx at leading dimension 768 + 64 inside guard rows (NaN in the output region, a
sentinel around it that must come back bit-identical); a second run is bit-identical; every element within waypoint_ref.ring_attn_ref's
bound (no multiplier).  One case plants, for every out-of-window (query, key) pair, a score 80 above the window's: the output equals,
bit for bit, the run with those key entries zeroed -- the kernel does not read them.  Four refusals leave the NaN fill intact.

etp_waypoint_tail: random logits N(0, 3) at B in {1, 3, 17} x max_pred in {1, 5, 8}; crafted maps (waypoint_ref.CRAFTED, max_pred 5
and 8; the last one an exact tie).  cand_*, cand_count, the zero pattern of nms_map and samp_* exact; heat and the non-zero nms values within
waypoint_ref.heat_bound (expf within one ulp, as the HIP math API documents, and an addition chain of 14).  The two input conditions
(pick margins >= 1e-4 in logit, uniforms at CDF midpoints of cells with regional probability >= 1e-3) are asserted on the fp64
reference for every case.

ETP_WAYPOINT_BOUNDS_OUT=<path> writes the worst ratios there (profiles/waypoint_op_bounds.txt is such a file).
"""
import functools
import os
from types import SimpleNamespace

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from etpnav_amd import _lib  # noqa: E402
from etpnav_amd import waypoint as wp  # noqa: E402
from tests import waypoint_ref as wr  # noqa: E402
from tests.attn_ref import merge_heads, same_bits  # noqa: E402

DEV = "cuda"
SENTINEL = -777.0
GUARD = 8
H = 768
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "waypoint_small.npz")


def L():
    return _lib.lib()


def stream():
    return torch.cuda.current_stream().cuda_stream


@pytest.fixture(scope="module", autouse=True)
def report_worst():
    yield
    lines = ["# tests/test_waypoint_gpu.py: worst |got - fp64| / bound per kernel and tensor (bounds: tests/waypoint_ref.py, no multiplier)"]
    lines += [f"{k:28s} {v[0]:.4f}   {v[1]}" for k, v in sorted(wr.WORST.items())]
    print("\n" + "\n".join(lines))
    out = os.environ.get("ETP_WAYPOINT_BOUNDS_OUT")
    if out:
        with open(out, "w") as f:
            f.write("\n".join(lines) + "\n")


# ---- etp_ring_attn_fwd ------------------------------------------------------------------------------------------------------------
class Guarded:
    """[rows, 768] output at leading dimension ld inside GUARD rows: NaN in the output region, SENTINEL around it"""

    def __init__(self, rows, ld, t):
        self.rows, self.ld = rows, ld
        self.buf = torch.full((rows + 2 * GUARD, ld), SENTINEL, device=DEV, dtype=t)
        self.buf[GUARD:GUARD + rows, :H] = float("nan")
        self.ptr = self.buf.data_ptr() + GUARD * ld * self.buf.element_size()

    def out(self):
        return self.buf[GUARD:GUARD + self.rows, :H]

    def check_guard(self, name):
        got = self.buf.clone()
        got[GUARD:GUARD + self.rows, :H] = SENTINEL
        same_bits(f"{name}: guard rows / extra columns", got, torch.full_like(got, SENTINEL))

    def untouched(self, name):
        assert bool(torch.isnan(self.out()).all()), f"{name}: the refused call wrote into ctx"
        self.check_guard(name)


def run_attn(q, k, v, B, n, t, packed, alpha=0.125, ld=H + 64):
    """q / k / v [B, heads, 12, 64] fp32 (stored values) -> (ctx tensor [B*12, 768] of dtype t, Guarded)"""
    qm, km, vm = (merge_heads(x).to(DEV).to(t) for x in (q, k, v))
    es = qm.element_size()
    if packed:
        buf = torch.cat([qm, km, vm], 1).contiguous()
        ops = (buf.data_ptr(), 3 * H, buf.data_ptr() + H * es, 3 * H, buf.data_ptr() + 2 * H * es, 3 * H)
    else:
        qm, km, vm = qm.contiguous(), km.contiguous(), vm.contiguous()
        ops = (qm.data_ptr(), H, km.data_ptr(), H, vm.data_ptr(), H)
    g = Guarded(B * 12, ld, t)
    dt = _lib.ETP_BF16 if t == torch.bfloat16 else _lib.ETP_F32
    _lib.check(L().etp_ring_attn_fwd(dt, *ops, g.ptr, ld, B, n, alpha, stream()), "etp_ring_attn_fwd")
    torch.cuda.synchronize()
    return g.out().clone(), g


@functools.lru_cache(maxsize=None)
def attn_reference(B, n, bf16):
    q, k, v = wr.attn_case(B, n, bf16)
    ctx, E = wr.ring_attn_ref(q, k, v, n, 0.125, bf16)
    return q, k, v, merge_heads(ctx), merge_heads(E)


@pytest.mark.parametrize("packed", [True, False], ids=["qkv3", "separate"])
@pytest.mark.parametrize("bf16", [True, False], ids=["bf16", "fp32"])
@pytest.mark.parametrize("n", wr.ATTN_N)
@pytest.mark.parametrize("B", wr.ATTN_B)
def test_ring_attn_against_fp64(B, n, bf16, packed):
    q, k, v, ctx, E = attn_reference(B, n, bf16)
    t = torch.bfloat16 if bf16 else torch.float32
    name = f"ring_attn B={B} n={n} {'bf16' if bf16 else 'fp32'} {'qkv3' if packed else 'separate'}"
    got, g = run_attn(q, k, v, B, n, t, packed)
    g.check_guard(name)
    wr.record(f"ring_attn/{'bf16' if bf16 else 'fp32'}/ctx", got.double().cpu().numpy(), ctx.numpy(), E.numpy(), name)
    again, g2 = run_attn(q, k, v, B, n, t, packed)
    same_bits(name + ": second run", again, got)


@pytest.mark.parametrize("bf16", [True, False], ids=["bf16", "fp32"])
def test_ring_attn_does_not_read_keys_outside_the_window(bf16):
    """q_i carries 8 on head dimension i, key j carries 80 on every dimension i whose query does not see j: alpha q_i . k_j gains 80
    exactly on the out-of-window pairs and nothing (an FMA with 0) on the others.  Plain standard normal operands otherwise (none of
    attn_case's scaled rows: the other 52 dimensions move a score by a few units, far less than the 80)."""
    B, n = 2, 1
    g = torch.Generator().manual_seed(505)
    q, k, v = (torch.randn(B, wr.HEADS, wr.TOK, 64, generator=g) for _ in range(3))
    if bf16:
        q, k, v = (x.bfloat16().float() for x in (q, k, v))
    q[..., :12] = 0.0
    k[..., :12] = 0.0
    k_plain = k.clone()
    mask = torch.from_numpy(wr.ring_mask(n))                      # [query i, key j]
    for i in range(12):
        q[:, :, i, i] = 8.0
        for j in range(12):
            if not mask[i, j]:
                k[:, :, j, i] = 80.0
    s = 0.125 * (q.double() @ k.double().transpose(-1, -2))
    inw = mask.bool()[None, None]
    assert float(s.masked_fill(inw, float("inf")).amin()) >= float(s.masked_fill(~inw, float("-inf")).amax()) + 50.0
    t = torch.bfloat16 if bf16 else torch.float32
    got, _ = run_attn(q, k, v, B, n, t, True)
    plain, _ = run_attn(q, k_plain, v, B, n, t, True)
    same_bits("out-of-window keys 80 above the window", got, plain)
    ctx, E = wr.ring_attn_ref(q, k_plain, v, n, 0.125, bf16)
    wr.record(f"ring_attn/{'bf16' if bf16 else 'fp32'}/ctx", got.double().cpu().numpy(), merge_heads(ctx).numpy(), merge_heads(E).numpy(),
              "ring_attn out-of-window")


@pytest.mark.parametrize("bf16", [True, False], ids=["bf16", "fp32"])
def test_ring_attn_refusals_launch_nothing(bf16):
    t = torch.bfloat16 if bf16 else torch.float32
    dt = _lib.ETP_BF16 if bf16 else _lib.ETP_F32
    B = 2
    buf = torch.randn(B * 12 + 1, 3 * H, device=DEV).to(t)
    es = buf.element_size()
    p = buf.data_ptr()
    ld = H + 64
    ok = (p, 3 * H, p + H * es, 3 * H, p + 2 * H * es, 3 * H)
    bad = {
        "neighbor 6": lambda g: L().etp_ring_attn_fwd(dt, *ok, g.ptr, ld, B, 6, 0.125, stream()),
        "neighbor -1": lambda g: L().etp_ring_attn_fwd(dt, *ok, g.ptr, ld, B, -1, 0.125, stream()),
        "B 0": lambda g: L().etp_ring_attn_fwd(dt, *ok, g.ptr, ld, 0, 1, 0.125, stream()),
        "B -3": lambda g: L().etp_ring_attn_fwd(dt, *ok, g.ptr, ld, -3, 1, 0.125, stream()),
        "misaligned K": lambda g: L().etp_ring_attn_fwd(dt, p, 3 * H, p + H * es + es, 3 * H, p + 2 * H * es, 3 * H, g.ptr, ld, B, 1,
                                                        0.125, stream()),
        "misaligned ctx": lambda g: L().etp_ring_attn_fwd(dt, *ok, g.ptr + es, ld, B, 1, 0.125, stream()),
        "ldq 2306": lambda g: L().etp_ring_attn_fwd(dt, p, 3 * H + 2, p + H * es, 3 * H, p + 2 * H * es, 3 * H, g.ptr, ld, B, 1, 0.125,
                                                    stream()),
        "ldc 766": lambda g: L().etp_ring_attn_fwd(dt, *ok, g.ptr, 766, B, 1, 0.125, stream()),
    }
    for name, call in bad.items():
        g = Guarded(B * 12, ld, t)
        assert call(g) != 0, name
        torch.cuda.synchronize()
        g.untouched(name)


# ---- etp_waypoint_tail ---------------------------------------------------------------------------------------------------------------
TAIL_CASES = ([(f"random B={B} max_pred={mp}", (lambda B=B, mp=mp: wr.tail_random(B, mp)), mp) for B, mp in wr.TAIL_RANDOM]
              + [(f"{kind} max_pred={mp}", (lambda kind=kind: wr.tail_crafted(kind)), mp) for kind in wr.CRAFTED for mp in (5, 8)])


def run_tail(logits, max_pred, uniforms):
    t = wp.waypoint_tail(torch.from_numpy(logits).to(DEV), max_pred, (7.0, 5.0),
                         None if uniforms is None else torch.from_numpy(uniforms).to(DEV))
    torch.cuda.synchronize()
    return t


@pytest.mark.parametrize("case", TAIL_CASES, ids=[c[0].replace(" ", "_") for c in TAIL_CASES])
def test_waypoint_tail_against_fp64(case):
    name, make, mp = case
    logits = make()
    uniforms = wr.make_uniforms(logits, mp, 1)
    ref = wr.check_conditions(logits, mp, uniforms, name=name)          # both input conditions, on the fp64 reference alone
    E = wr.heat_bound(logits)
    for u in (uniforms, None):
        got = run_tail(logits, mp, u)
        tab = got.table.cpu().numpy()
        assert tab[0, :, 0].tolist() == ref["count"].tolist(), (name, tab[0, :, 0].tolist(), ref["count"].tolist())
        for row, key in ((1, "angle"), (2, "dist"), (3, "img_cw"), (4, "img_ccw")):
            assert (tab[row] == ref[key]).all(), (name, key, tab[row].tolist(), ref[key].tolist())
        if u is not None:
            for row, key in ((5, "samp_angle"), (6, "samp_dist")):
                assert (tab[row] == ref[key]).all(), (name, key, tab[row].tolist(), ref[key].tolist())
        heat, nms = got.heat.double().cpu().numpy(), got.nms_map.double().cpu().numpy()
        assert ((nms != 0) == (ref["nms_map"] != 0)).all(), f"{name}: zero pattern of nms_map"
        wr.record("waypoint_tail/heat", heat, ref["heat"], E, name)
        wr.record("waypoint_tail/nms_map", nms, ref["nms_map"], E, name)
        again = run_tail(logits, mp, u)
        same_bits(name + ": heat, second run", again.heat, got.heat)
        same_bits(name + ": nms_map, second run", again.nms_map, got.nms_map)
        assert torch.equal(again.table, got.table), name


def test_waypoint_tail_refusals_launch_nothing():
    B, mp = 2, 5
    logits = torch.from_numpy(wr.tail_random(3, 5))[:B].contiguous().to(DEV)

    def outputs():
        f = [torch.full((B + 1, 120, 12), float("nan"), device=DEV) for _ in range(2)]
        i = [torch.full((B * 8 + 8,), -7, dtype=torch.int32, device=DEV) for _ in range(7)]
        return f, i

    def call(lg, Bn, mpn, f, i, uni=None, off=0):
        return L().etp_waypoint_tail(lg, Bn, mpn, 7.0, 5.0, uni, f[0].data_ptr() + off, f[1].data_ptr(), i[0].data_ptr(),
                                     i[1].data_ptr(), i[2].data_ptr(), i[3].data_ptr(), i[4].data_ptr(),
                                     i[5].data_ptr() if uni else None, i[6].data_ptr() if uni else None, stream())

    uni = torch.rand(B, 8, device=DEV)
    bad = {
        "max_pred 0": lambda f, i: call(logits.data_ptr(), B, 0, f, i),
        "max_pred 9": lambda f, i: call(logits.data_ptr(), B, 9, f, i),
        "B 0": lambda f, i: call(logits.data_ptr(), 0, mp, f, i),
        "B -1": lambda f, i: call(logits.data_ptr(), -1, mp, f, i),
        "misaligned logits": lambda f, i: call(logits.data_ptr() + 4, B, mp, f, i),
        "misaligned heat": lambda f, i: call(logits.data_ptr(), B, mp, f, i, off=4),
        "uniforms without samp": lambda f, i: L().etp_waypoint_tail(
            logits.data_ptr(), B, mp, 7.0, 5.0, uni.data_ptr(), f[0].data_ptr(), f[1].data_ptr(), i[0].data_ptr(), i[1].data_ptr(),
            i[2].data_ptr(), i[3].data_ptr(), i[4].data_ptr(), None, None, stream()),
    }
    for name, fn in bad.items():
        f, i = outputs()
        assert fn(f, i) != 0, name
        torch.cuda.synchronize()
        assert all(bool(torch.isnan(x).all()) for x in f) and all(bool((x == -7).all()) for x in i), f"{name}: the refused call wrote"


# ---- engine and host mirror against the fixture ------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def golden():
    g = dict(np.load(GOLDEN))
    W = wr.make_weights(int(g["seed"]), float(g["cls_scale"]))
    fp = wr.fingerprint(W)
    assert [k for k, _ in wr.param_shapes()] == [str(k) for k in g["keys"]]
    np.testing.assert_allclose(np.array([fp[k] for k, _ in wr.param_shapes()]), g["fingerprint"], rtol=1e-12, atol=0)
    g["W"] = W
    return g


@functools.lru_cache(maxsize=None)
def predictor(bf16):
    return wp.BinaryDistPredictorTRM(device=DEV, dtype=torch.bfloat16 if bf16 else torch.float32)


def loaded(golden, bf16):
    m = predictor(bf16)
    m.load_state_dict(golden["W"], strict=True)
    return m.eval()


def test_engine_fp32_logits_match_the_reference(golden):
    m = loaded(golden, False)
    depth = torch.from_numpy(golden["depth_cw"].astype(np.float32)).to(DEV)
    logits = m(None, depth.reshape(-1, 128, 4, 4))
    assert tuple(logits.shape) == (3, 120, 12)
    err = float((logits.cpu() - torch.from_numpy(golden["logits"])).abs().max())
    print(f"fp32 engine against the reference's fp32 logits: {err:.3e} (|logits| up to {float(np.abs(golden['logits']).max()):.2f})")
    assert err <= 2e-4
    same_bits("second run", m(None, depth), logits)
    # the tail on those logits: the recorded heat map and the reference nms
    t = m.candidates(logits, False)
    assert float((t.heat.cpu() - torch.from_numpy(golden["heat"])).abs().max()) <= 1e-5
    assert ((t.nms_map.cpu().numpy() != 0) == (golden["nms_map"] != 0)).all()


def test_engine_bf16_logits_within_twice_the_reference_autocast_gap(golden):
    m = loaded(golden, True)
    gap = float(golden["bf16_autocast_gap"])
    depth = torch.from_numpy(golden["depth_cw"].astype(np.float32)).to(DEV)
    logits = m(None, depth)
    err = float((logits.cpu() - torch.from_numpy(golden["logits"])).abs().max())
    print(f"bf16 engine against the reference's fp32 logits: {err:.4f}; the reference's own autocast gap {gap:.4f}")
    assert err <= 2 * gap
    # candidate lists on the episodes whose every pick leads by 4 x the gap (the generator asserts: all three)
    t = m.candidates(logits, False)
    tab = t.table.cpu().numpy()
    ref = wr.tail_ref(golden["logits"], 5)
    robust = [j for j in range(3) if float(golden["pick_margins"][j]) >= 4 * gap]
    assert robust == [0, 1, 2]
    for j in robust:
        assert int(tab[0, j, 0]) == int(ref["count"][j])
        assert tab[1, j].tolist() == ref["angle"][j].tolist() and tab[2, j].tolist() == ref["dist"][j].tolist(), j


def test_state_dict_is_strict_under_the_reference_keys(golden):
    m = predictor(False)
    assert list(m.state_dict().keys()) == [k for k, _ in wr.param_shapes()]
    assert all(not p.requires_grad for p in m.parameters())
    m.load_state_dict(golden["W"], strict=True)
    short = dict(golden["W"])
    del short["visual_merge.0.weight"]                       # unused by the forward, still part of the strict contract
    with pytest.raises(RuntimeError):
        m.load_state_dict(short, strict=True)
    extra = dict(golden["W"])
    extra["visual_fc_rgb.1.weight"] = torch.zeros(1)
    with pytest.raises(RuntimeError):
        m.load_state_dict(extra, strict=True)


class _Encoders:
    """stand-ins for the perception encoders: look the stored embedding up by the view id painted into the observation"""

    def __init__(self, golden):
        self.depth_table = torch.from_numpy(golden["depth_table"].astype(np.float32)).to(DEV)
        self.rgb_table = torch.from_numpy(golden["rgb_table"].astype(np.float32)).to(DEV)

    def depth(self, o):
        return self.depth_table[o["depth"][:, 0, 0, 0].long()].reshape(-1, 128, 4, 4)

    def rgb(self, o):
        return self.rgb_table[o["rgb"][:, 0, 0, 0].long()]


def observations(B):
    obs = {}
    for a in range(12):
        suffix = "" if a == 0 else f"_{a * 30.0}"
        ids = (torch.arange(B) * 12 + a).float().reshape(B, 1, 1, 1)
        obs["rgb" + suffix] = ids.expand(B, 2, 2, 3).clone().to(DEV)
        obs["depth" + suffix] = ids.expand(B, 2, 2, 1).clone().to(DEV)
    return obs


@pytest.fixture(scope="module")
def net():
    from etpnav_amd.policy import ETP
    return ETP(model_config=SimpleNamespace(task_type="r2r"), dtype=torch.float32, device=DEV).eval()


def check_outputs(out, golden, prefix):
    assert list(out.keys()) == ["cand_rgb", "cand_depth", "cand_angle_fts", "cand_img_idxes", "cand_angles", "cand_distances",
                                "pano_rgb", "pano_depth", "pano_angle_fts", "pano_img_idxes"]
    for j in range(3):
        for k in ("cand_rgb", "cand_depth", "cand_angle_fts"):
            assert isinstance(out[k], list) and isinstance(out[k][j], torch.Tensor)
            np.testing.assert_allclose(out[k][j].float().cpu().numpy(), golden[f"{prefix}{k}_{j}"], rtol=0, atol=1e-5, err_msg=f"{k}[{j}]")
        assert isinstance(out["cand_img_idxes"][j], np.ndarray)
        assert out["cand_img_idxes"][j].tolist() == golden[f"{prefix}cand_img_idxes_{j}"].tolist()
        assert isinstance(out["cand_angles"][j], list) and isinstance(out["cand_distances"][j], list)
        np.testing.assert_allclose(out["cand_angles"][j], golden[f"{prefix}cand_angles_{j}"], rtol=0, atol=1e-5)
        np.testing.assert_allclose(out["cand_distances"][j], golden[f"{prefix}cand_distances_{j}"], rtol=0, atol=1e-5)
    for k in ("pano_rgb", "pano_depth", "pano_angle_fts"):
        np.testing.assert_allclose(out[k].float().cpu().numpy(), golden[prefix + k], rtol=0, atol=1e-5, err_msg=k)
    assert isinstance(out["pano_img_idxes"], np.ndarray) and out["pano_img_idxes"].tolist() == golden[prefix + "pano_img_idxes"].tolist()


def test_waypoint_mode_matches_the_reference_branch_with_one_host_copy(golden, net, monkeypatch):
    pred = loaded(golden, False)
    with pytest.raises(NotImplementedError):                  # no encoders attached: as before
        net(mode="waypoint", waypoint_predictor=pred, observations=observations(3), in_train=False)
    enc = _Encoders(golden)
    net.depth_encoder, net.rgb_encoder = enc.depth, enc.rgb
    try:
        out = net(mode="waypoint", waypoint_predictor=pred, observations=observations(3), in_train=False)
        check_outputs(out, golden, "eval_")
        # in_train: the stored uniforms reproduce the recorded samples
        out_t = wp.waypoint_mode(net, pred, observations(3), True, uniforms=torch.from_numpy(golden["uniforms"]).to(DEV))
        check_outputs(out_t, golden, "train_")
        # exactly one device-to-host copy per call
        copies = []
        for fn in ("cpu", "tolist", "item", "numpy", "nonzero"):
            real = getattr(torch.Tensor, fn)

            def counted(self, *a, _real=real, _fn=fn, **k):
                if self.is_cuda:
                    copies.append(_fn)
                return _real(self, *a, **k)
            monkeypatch.setattr(torch.Tensor, fn, counted)
        obs = observations(3)
        torch.cuda.synchronize()
        net(mode="waypoint", waypoint_predictor=pred, observations=obs, in_train=False)
        assert copies == ["cpu"], copies
        del copies[:]
        net(mode="waypoint", waypoint_predictor=pred, observations=obs, in_train=True)
        assert copies == ["cpu"], copies
    finally:
        net.depth_encoder = net.rgb_encoder = None
