"""The dropout sites of the row kernels and of the cast, at operator level, through the `_drop` entry points (tests/drop_ref.py):

  etp_text_embed_fwd_drop / _bwd_drop   text_embed_fwd_kernel, text_embed_bwd_kernel      row_dropout, embed.hip   row * H + col
  etp_pano_embed_fwd_drop / _bwd_drop   pano_embed_fwd_kernel, pano_embed_bwd_kernel<PART 0/1/2>
  etp_sap_tail_fwd_drop / _bwd_drop     sap_tail_fwd_kernel, sap_tail_bwd_kernel (the mask twice)
  etp_ln_stream_bwd_drop, etp_ln_stream_bwd_stage1_drop   ln_bwd_s_kernel, atomic and slab mode    norm.hip   on dx_lp only
  etp_cast_f32_to_drop                  cast_drop_kernel                                   the flat index

Every case (the lists of drop_ref.py; tests/test_drop_bounds_cpu.py plants the mistakes on the same lists), p in {0.1, 0.4}, two sites:
  mask read-out, exact   y (text, panorama), dst (cast): the exact zeros are {i: multiplier(i) == 0} of the numpy restatement, every
                         element compared; the reference alone shows beforehand that no kept element can read as zero.  dx_lp of
                         ln_bwd_s is RNE(dx * multiplier) of the kernel's own dx, bit for bit, and the cast's dst likewise.  At M <= 8
                         one-hot rows of dy / dlogits read the BACKWARD's mask out of dbeta (text, panorama), dw2 and dbeta (SAP: its
                         two applications) -- the backward regenerates the forward's mask.
  values                 every output within the bound of the fp64 restatement with dropout (drop_ref's docstring)
  plain entry            `_drop` with NULL and with p = 0 returns the bits of the plain entry point; p = 1e-6 (threshold 0) drops
                         nothing and scales by 1 / (1 - p)
  harness                outputs NaN-filled inside guarded buffers, inputs unchanged afterwards, a second run bit for bit wherever no
                         atomics are involved
"""
import ctypes

import pytest
import torch

pytestmark = pytest.mark.gpu

from etpnav_amd import _lib  # noqa: E402
from etpnav_amd._lib import check, ptr  # noqa: E402
from tests import drop_ref as dr  # noqa: E402
from tests import move_ref as mv  # noqa: E402
from tests import reduce_ref as rf  # noqa: E402
from tests import row_ref as rr  # noqa: E402

DEV = "cuda"
F64, F32 = torch.float64, torch.float32
TDT = dr.TDT
EDT = {"fp32": _lib.ETP_F32, "bf16": _lib.ETP_BF16}
INVALID = -1
Guarded, gptr = rf.Guarded, rf.gptr


def L():
    return _lib.lib()


def stream():
    return torch.cuda.current_stream().cuda_stream


def csite(site):
    """Site -> (the ctypes struct, kept alive by the caller; its byref)"""
    s = _lib.DropSite(site.p, site.seed, site.mode, site.layer, site.slot)
    return s, ctypes.byref(s)


def ids(cases):
    return ["-".join(str(v) for v in c) for c in cases]


def snapshot(*tensors):
    return [None if t is None else t.clone() for t in tensors]


def unchanged(what, tensors, before):
    for i, (t, b) in enumerate(zip(tensors, before)):
        if t is not None:
            mv.exact(f"{what}: read-only input {i}", t, b)


@pytest.fixture(scope="module", autouse=True)
def leave_the_global_generators_alone():
    """every operand here comes from its own seeded generator; other files draw from torch's global ones without seeding them, so this
    file hands them back as it found them"""
    cpu, gpu = torch.get_rng_state(), torch.cuda.get_rng_state()
    yield
    assert torch.equal(torch.get_rng_state(), cpu) and torch.equal(torch.cuda.get_rng_state(), gpu), "a case drew from a global generator"


@pytest.fixture(scope="module", autouse=True)
def report_worst():
    yield
    rows = [f"  {str(k[0]):<44}{str(k[1]):<12}{v:8.3f}" for k, v in sorted(dr.WORST.items(), key=str)]
    print("\ndropout sites of the row kernels, worst err / bound per (entry point, tensor):\n" + "\n".join(rows))
    print("row_ref classes: " + ", ".join(f"{k} {v:.3g} ({n})" for k, (v, n) in rr.WORST.items()))


# ---- text embedding ------------------------------------------------------------------------------------------------------------
TEXT = dr.text_cases()
TEXT_GRADS = ("dword", "dpos", "dtype0", "dgamma", "dbeta")


def _text_fwd(c, e, t, with_lp, site_ref, plain=False):
    B, Lt, H = c["B"], c["L"], c["H"]
    M = B * Lt
    y, lp, stats = Guarded((M, H)), Guarded((M, H), t) if with_lp else None, Guarded((M, 2))
    args = (e, ptr(c["ids"]), ptr(c["word"]), ptr(c["pos"]), ptr(c["type0"]), ptr(c["gamma"]), ptr(c["beta"]), gptr(y), gptr(lp), gptr(stats),
            B, Lt, H, c["eps"], stream())
    check(L().etp_text_embed_fwd(*args) if plain else L().etp_text_embed_fwd_drop(*args, site_ref), "text_embed_fwd")
    torch.cuda.synchronize()
    for g, n in ((y, "y"), (lp, "y_lp"), (stats, "stats")):
        if g is not None:
            g.check("text_embed_fwd " + n)
    return y, lp, stats


def _text_bwd(c, e, dy, site_ref, init=None, plain=False):
    B, Lt, H = c["B"], c["L"], c["H"]
    got = {k: Guarded(tuple(c["init_" + k].shape), init=c["init_" + k] if init is None else init[k]) for k in TEXT_GRADS}
    args = (e, ptr(dy), ptr(c["ids"]), ptr(c["word"]), ptr(c["pos"]), ptr(c["type0"]), ptr(c["gamma"]), ptr(c["stats"]),
            *[gptr(got[k]) for k in TEXT_GRADS], B, Lt, H, stream())
    check(L().etp_text_embed_bwd(*args) if plain else L().etp_text_embed_bwd_drop(*args, site_ref), "text_embed_bwd")
    torch.cuda.synchronize()
    for k in TEXT_GRADS:
        got[k].check("text_embed_bwd " + k)
    return {k: v.t for k, v in got.items()}


@pytest.mark.parametrize("i", range(len(TEXT)), ids=ids(TEXT))
def test_text_embed_drop(i):
    dt, H, B, Lt, p, triple = TEXT[i]
    site = dr.Site(p, triple)
    c = dr.text_case(B, Lt, H, site, seed=100 + i, device=DEV)
    M, t, e = B * Lt, TDT[dt], EDT[dt]
    keep, sref = csite(site)
    inputs = [c[k] for k in ("ids", "word", "pos", "type0", "gamma", "beta", "dy", "stats")]
    before = snapshot(*inputs)
    runs = [_text_fwd(c, e, t, True, sref) for _ in range(2)]
    for a, b in zip(*runs):
        rf.same_bits("text_embed_fwd_drop (second run)", a.t, b.t)
    y, lp, stats = (g.t for g in runs[0])
    name = f"etp_text_embed_fwd_drop {dt}"
    dr.zero_set(name + " y", y, c["m"])
    dr.within((name, "y"), y, c["y"], c["by"])
    dr.within((name, "stats"), stats, c["st"], c["bst"])
    rf.same_bits(name + " y_lp (round-to-nearest-even copy of y)", lp, y.to(t))
    # the plain entry point: NULL and p = 0 are its bits; p = 1e-6 keeps everything and scales it
    plain = _text_fwd(c, e, t, True, None, plain=True)
    zero, zref = csite(dr.Site(0.0, triple))
    for what, ref in (("NULL", None), ("p = 0", zref)):
        for a, b in zip(_text_fwd(c, e, t, True, ref), plain):
            rf.same_bits(f"text_embed_fwd_drop with {what} against the plain entry point", a.t, b.t)
    tiny, tref = csite(dr.Site(dr.P_TINY, triple))
    yt = _text_fwd(c, e, t, False, tref)[0].t
    rf.same_bits("text_embed_fwd_drop p = 1e-6: y = y_plain / (1 - p)", yt, plain[0].t * float(dr.inv_keep(dr.P_TINY)))
    # backward
    d = dr.text_backward(c)
    got = _text_bwd(c, e, c["dy"], sref)
    rf.check_text_bwd(f"etp_text_embed_bwd_drop {dt}", d, got)
    for k in TEXT_GRADS:
        dr.record((f"etp_text_embed_bwd_drop {dt}", k), rf.WORST.get((f"etp_text_embed_bwd_drop {dt}", k), 0.0))
    gp = _text_bwd(c, e, c["dy"], None, plain=True)
    for what, ref in (("NULL", None), ("p = 0", zref)):
        g0 = _text_bwd(c, e, c["dy"], ref)
        for k in ("dpos",):                                   # one workgroup and one atomic per element: the one deterministic gradient
            rf.same_bits(f"text_embed_bwd_drop with {what} against the plain entry point, {k}", g0[k], gp[k])
        rf.check_text_bwd(f"etp_text_embed_bwd_drop {what}", dr.text_backward(c, torch.ones_like(c["m"])), g0)
    if M <= dr.PROBE_ROWS:
        zeros = {k: torch.zeros_like(c["init_" + k]) for k in TEXT_GRADS}
        for row in range(M):
            dy = torch.zeros(M, H, device=DEV)
            dy[row] = torch.where(c["dy"].reshape(M, H)[row] == 0, torch.ones(H, device=DEV), c["dy"].reshape(M, H)[row])
            g1 = _text_bwd(c, e, dy.reshape(B, Lt, H), sref, init=zeros)
            dr.zero_set(f"text_embed_bwd_drop dbeta, one-hot dy row {row}", g1["dbeta"], c["m"][row])
            assert torch.equal(g1["dbeta"], dy[row] * c["m"][row]), f"text_embed_bwd_drop dbeta != dy * multiplier, row {row}"   # (-0 == +0: 0 + -0)
    unchanged("text embedding", inputs, before)


# ---- panorama embedding --------------------------------------------------------------------------------------------------------
PANO = dr.pano_cases()


def _pano_fwd(c, e, site_ref, plain=False):
    M, H = c["M"], c["H"]
    PP = (ctypes.c_void_p * 12)(*[p.data_ptr() for p in c["params"]])
    y, stats = Guarded((M, H)), Guarded((M, 8))
    args = (e, ptr(c["a"]), ptr(c["d"]), ptr(c["loc"]), ptr(c["nav"]), PP, gptr(y), gptr(stats), M, H, stream())
    check(L().etp_pano_embed_fwd(*args) if plain else L().etp_pano_embed_fwd_drop(*args, site_ref), "pano_embed_fwd")
    torch.cuda.synchronize()
    y.check("pano_embed_fwd y")
    stats.check("pano_embed_fwd stats")
    return y.t, stats.t


def _pano_bwd(c, e, dy, stats, site_ref, init=None, plain=False):
    M, H, t = c["M"], c["H"], c["a"].dtype
    PP = (ctypes.c_void_p * 12)(*[p.data_ptr() for p in c["params"]])
    grads = [Guarded((g.numel(),), init=g) for g in (c["init"] if init is None else init)]
    GG = (ctypes.c_void_p * 12)(*[g.t.data_ptr() for g in grads])
    da, dd = Guarded((M, H), t), Guarded((M, H), t) if c["depth"] else None
    args = (e, ptr(dy), ptr(c["a"]), ptr(c["d"]), ptr(c["loc"]), ptr(c["nav"]), ptr(stats), PP, GG, gptr(da), gptr(dd), M, H, stream())
    check(L().etp_pano_embed_bwd(*args) if plain else L().etp_pano_embed_bwd_drop(*args, site_ref), "pano_embed_bwd")
    torch.cuda.synchronize()
    for g, n in [(da, "da"), (dd, "dd")] + [(g, "d" + k) for g, k in zip(grads, rr.PANO_NAMES)]:
        if g is not None:
            g.check("pano_embed_bwd " + n)
    return da.t, None if dd is None else dd.t, [g.t for g in grads]


@pytest.mark.parametrize("i", range(len(PANO)), ids=ids(PANO))
def test_pano_embed_drop(i):
    dt, H, M, depth, p, triple = PANO[i]
    site = dr.Site(p, triple)
    c = dr.pano_case(M, H, depth, TDT[dt], site, seed=200 + i, device=DEV)
    e = EDT[dt]
    keep, sref = csite(site)
    inputs = [c["a"], c["d"], c["loc"], c["nav"], c["dy"]] + c["params"]
    before = snapshot(*inputs)
    (y, stats), (y2, stats2) = _pano_fwd(c, e, sref), _pano_fwd(c, e, sref)
    rf.same_bits("pano_embed_fwd_drop y (second run)", y, y2)
    dr.zero_set(f"etp_pano_embed_fwd_drop {dt} y", y, c["m"])
    rr.check_pano_fwd(y, stats, c["y"], c["st"], depth)
    yp, sp = _pano_fwd(c, e, None, plain=True)
    zero, zref = csite(dr.Site(0.0, triple))
    for what, ref in (("NULL", None), ("p = 0", zref)):
        y0, s0 = _pano_fwd(c, e, ref)
        rf.same_bits(f"pano_embed_fwd_drop with {what} against the plain entry point", y0, yp)
        mv.exact(f"pano_embed_fwd_drop with {what} against the plain entry point, stats", s0, sp)
    tiny, tref = csite(dr.Site(dr.P_TINY, triple))
    rf.same_bits("pano_embed_fwd_drop p = 1e-6: y = y_plain / (1 - p)", _pano_fwd(c, e, tref)[0], yp * float(dr.inv_keep(dr.P_TINY)))
    # backward
    ref = dr.pano_backward(c)
    da, dd, grads = _pano_bwd(c, e, c["dy"], stats, sref)
    da2, dd2, _ = _pano_bwd(c, e, c["dy"], stats, sref)
    rf.same_bits("pano_embed_bwd_drop da (second run)", da, da2)
    rr.check_pano_bwd(da, dd, grads, c["init"], ref, depth)
    dap, ddp, _ = _pano_bwd(c, e, c["dy"], stats, None, plain=True)
    for what, r0 in (("NULL", None), ("p = 0", zref)):
        da0, dd0, g0 = _pano_bwd(c, e, c["dy"], stats, r0)
        rf.same_bits(f"pano_embed_bwd_drop with {what} against the plain entry point, da", da0, dap)
        if depth:
            rf.same_bits(f"pano_embed_bwd_drop with {what} against the plain entry point, dd", dd0, ddp)
        rr.check_pano_bwd(da0, dd0, g0, c["init"], dr.pano_backward(c, torch.ones_like(c["m"])), depth)
    if M <= dr.PROBE_ROWS:
        zeros = [torch.zeros_like(g) for g in c["init"]]
        j = rr.PANO_NAMES.index("b_out")
        for row in range(M):
            dy = torch.zeros(M, H, device=DEV)
            dy[row] = torch.where(c["dy"][row] == 0, torch.ones(H, device=DEV), c["dy"][row])
            g1 = _pano_bwd(c, e, dy, stats, sref, init=zeros)[2]
            dr.zero_set(f"pano_embed_bwd_drop db_out, one-hot dy row {row}", g1[j], c["m"][row])
            assert torch.equal(g1[j], dy[row] * c["m"][row]), f"pano_embed_bwd_drop db_out != dy * multiplier, row {row}"   # (-0 == +0: 0 + -0)
    unchanged("panorama embedding", inputs, before)


# ---- SAP tail ------------------------------------------------------------------------------------------------------------------
SAP = dr.sap_cases()
SAP_GRADS = ("dgamma", "dbeta", "dw2", "db2")


def _sap_fwd(c, e, site_ref, plain=False):
    M, H = c["M"], c["H"]
    logits, stats = Guarded((M,)), Guarded((M, 2))
    args = (e, ptr(c["r"]), ptr(c["gamma"]), ptr(c["beta"]), ptr(c["w2"]), ptr(c["b2"]), ptr(c["vis"]), ptr(c["val"]), gptr(logits),
            gptr(stats), M, H, stream())
    check(L().etp_sap_tail_fwd(*args) if plain else L().etp_sap_tail_fwd_drop(*args, site_ref), "sap_tail_fwd")
    torch.cuda.synchronize()
    logits.check("sap_tail_fwd logits")
    stats.check("sap_tail_fwd stats")
    return logits.t, stats.t


def _sap_bwd(c, e, dl, stats, site_ref, init=None, plain=False):
    M, H = c["M"], c["H"]
    init = c["init"] if init is None else init
    got = {k: Guarded(tuple(init[k].shape), init=init[k]) for k in SAP_GRADS}
    dz = Guarded((M, H), c["r"].dtype)
    args = (e, ptr(dl), ptr(c["r"]), ptr(c["gamma"]), ptr(c["beta"]), ptr(c["w2"]), ptr(stats), ptr(c["vis"]), ptr(c["val"]), gptr(dz),
            *[gptr(got[k]) for k in SAP_GRADS], M, H, stream())
    check(L().etp_sap_tail_bwd(*args) if plain else L().etp_sap_tail_bwd_drop(*args, site_ref), "sap_tail_bwd")
    torch.cuda.synchronize()
    dz.check("sap_tail_bwd dz")
    for k in SAP_GRADS:
        got[k].check("sap_tail_bwd " + k)
    return dz.t, {k: v.t for k, v in got.items()}


@pytest.mark.parametrize("i", range(len(SAP)), ids=ids(SAP))
def test_sap_tail_drop(i):
    dt, H, M, pattern, p, triple = SAP[i]
    site = dr.Site(p, triple)
    c = dr.sap_case(M, H, pattern, TDT[dt], site, seed=300 + i, device=DEV)
    e, masked = EDT[dt], c["masked"]
    keep, sref = csite(site)
    inputs = [c[k] for k in ("r", "gamma", "beta", "w2", "b2", "vis", "val")]
    before = snapshot(*inputs)
    (logits, stats), (lg2, _) = _sap_fwd(c, e, sref), _sap_fwd(c, e, sref)
    mv.exact("sap_tail_fwd_drop logits (second run)", logits, lg2)
    ref_lg, ref_st = dr.sap_forward(c)
    rr.check_sap_fwd(logits, stats, ref_lg, ref_st, masked)
    lgp, stp = _sap_fwd(c, e, None, plain=True)
    zero, zref = csite(dr.Site(0.0, triple))
    for what, r0 in (("NULL", None), ("p = 0", zref)):
        l0, s0 = _sap_fwd(c, e, r0)
        mv.exact(f"sap_tail_fwd_drop with {what} against the plain entry point, logits", l0, lgp)
        mv.exact(f"sap_tail_fwd_drop with {what} against the plain entry point, stats", s0, stp)
    tiny_site = dr.Site(dr.P_TINY, triple)
    tiny, tref = csite(tiny_site)
    ones_scaled = torch.full_like(c["m"], float(dr.inv_keep(dr.P_TINY)))
    rr.check_sap_fwd(_sap_fwd(c, e, tref)[0], stats, dr.sap_forward(c, ones_scaled)[0], ref_st, masked)
    # backward: whatever the loss left in masked rows must not leak
    dl = c["dl"].clone()
    dl[masked] = float("nan")
    ref = dr.sap_backward(c)
    dz, got = _sap_bwd(c, e, dl, stats, sref)
    dz2, _ = _sap_bwd(c, e, dl, stats, sref)
    rf.same_bits("sap_tail_bwd_drop dz (second run)", dz, dz2)
    rr.check_sap_bwd(dz, got, c["init"], ref, masked, c["r"])
    dzp, _ = _sap_bwd(c, e, dl, stats, None, plain=True)
    for what, r0 in (("NULL", None), ("p = 0", zref)):
        dz0, g0 = _sap_bwd(c, e, dl, stats, r0)
        rf.same_bits(f"sap_tail_bwd_drop with {what} against the plain entry point, dz", dz0, dzp)
        ones = torch.ones_like(c["m"])
        rr.check_sap_bwd(dz0, g0, c["init"], dr.sap_backward(c, ones, ones), masked, c["r"])
    if M <= dr.PROBE_ROWS:
        zeros = {k: torch.zeros_like(v) for k, v in c["init"].items()}
        for row in range(M):
            if bool(masked[row]):
                continue
            one = torch.zeros(M, device=DEV)
            one[row] = 1.5
            _, g1 = _sap_bwd(c, e, one, stats, sref, init=zeros)
            dr.zero_set(f"sap_tail_bwd_drop dw2 (dl * dropout(n)), one-hot dlogits row {row}", g1["dw2"], c["m"][row])
            dr.zero_set(f"sap_tail_bwd_drop dbeta (dl * w2 * mask), one-hot dlogits row {row}", g1["dbeta"], c["m"][row])
            r1 = dr.sap_backward(c, dl=one)
            rr.accumulated(f"sap dw2, one-hot row {row}", g1["dw2"], zeros["dw2"], r1["dw2"])
            rr.accumulated(f"sap dbeta, one-hot row {row}", g1["dbeta"], zeros["dbeta"], r1["dbeta"])
    unchanged("SAP tail", inputs, before)


# ---- ln_bwd_s ------------------------------------------------------------------------------------------------------------------
LN = dr.ln_cases()


def _ln(c, e, t, slabs, add, site_ref, plain=False, with_dx=True, lp_is_dx=False):
    M, H = c["M"], c["H"]
    dx, lp = Guarded((M, H)) if with_dx else None, Guarded((M, H), t)
    dg, db = Guarded((H,), init=c["init_g"]), Guarded((H,), init=c["init_b"])
    head = (e, ptr(c["dy"]), ptr(c["x"]), ptr(c["stats"]), ptr(c["gamma"]), ptr(add), gptr(dx), gptr(dx) if lp_is_dx else gptr(lp), gptr(dg),
            gptr(db))
    if slabs:
        nbytes = int(L().etp_ln_bwd_part_bytes(M, H))
        part = torch.full((nbytes // 4,), float("nan"), device=DEV)
        args = head + (ptr(part), M, H, stream())
        rc = L().etp_ln_stream_bwd_stage1(*args) if plain else L().etp_ln_stream_bwd_stage1_drop(*args, site_ref)
        if rc == 0:
            check(L().etp_ln_part_reduce(ptr(part), M, H, gptr(dg), gptr(db), stream()), "ln stage 2")
    else:
        args = head + (M, H, stream())
        rc = L().etp_ln_stream_bwd(*args) if plain else L().etp_ln_stream_bwd_drop(*args, site_ref)
    torch.cuda.synchronize()
    return rc, dx, lp, dg, db


@pytest.mark.parametrize("i", range(len(LN)), ids=ids(LN))
def test_ln_stream_bwd_drop(i):
    dt, H, M, slabs, with_add, p, triple = LN[i]
    site = dr.Site(p, triple)
    c = dr.ln_case(M, H, slabs, site, seed=400 + i, device=DEV)
    t, e = TDT[dt], EDT[dt]
    add = c["add"] if with_add else None
    keep, sref = csite(site)
    inputs = [c["dy"], c["x"], c["stats"], c["gamma"], add]
    before = snapshot(*inputs)
    name = "etp_ln_stream_bwd_stage1_drop+reduce" if slabs else "etp_ln_stream_bwd_drop"
    runs = []
    for _ in range(2):
        rc, dx, lp, dg, db = _ln(c, e, t, slabs, add, sref)
        check(rc, name)
        for g, n in ((dx, "dx"), (lp, "dx_lp"), (dg, "dgamma"), (db, "dbeta")):
            g.check(f"{name} {n}")
        runs.append((dx, lp))
    rf.same_bits(f"{name} dx (second run)", runs[0][0].t, runs[1][0].t)
    rf.same_bits(f"{name} dx_lp (second run)", runs[0][1].t, runs[1][1].t)
    dr.check_ln(f"{name} {dt}", c, dx.t, lp.t, dg.t, db.t, add)
    # plain entry point
    _, dxp, lpp, _, _ = _ln(c, e, t, slabs, add, None, plain=True)
    zero, zref = csite(dr.Site(0.0, triple))
    for what, r0 in (("NULL", None), ("p = 0", zref)):
        rc, dx0, lp0, dg0, db0 = _ln(c, e, t, slabs, add, r0)
        check(rc, name)
        rf.same_bits(f"{name} with {what} against the plain entry point, dx", dx0.t, dxp.t)
        rf.same_bits(f"{name} with {what} against the plain entry point, dx_lp", lp0.t, lpp.t)
        rf.check_ln_bwd(f"{name} {what}", c, dx0.t, lp0.t, dg0.t, db0.t, add)
    tiny, tref = csite(dr.Site(dr.P_TINY, triple))
    rc, dxt, lpt, _, _ = _ln(c, e, t, slabs, add, tref)
    check(rc, name)
    rf.same_bits(f"{name} p = 1e-6: dx", dxt.t, dxp.t)
    rf.same_bits(f"{name} p = 1e-6: dx_lp = RNE(dx / (1 - p))", lpt.t, (dxp.t * float(dr.inv_keep(dr.P_TINY))).to(t))
    # refused without a separate operand copy: nothing is written
    for kw in ({"with_dx": False}, {"lp_is_dx": True}) if dt == "fp32" else ({"with_dx": False},):
        rc, dxr, lpr, dgr, dbr = _ln(c, e, t, slabs, add, sref, **kw)
        if "with_dx" in kw:                                   # dx_lp alone IS a separate copy: accepted, and it carries the mask
            check(rc, name)
            ref = c["dx0"] if add is None else c["dx0"] + add.to(F64)
            bound = dr.scaled_bound(ref, rf.ln_dx_bound(c["t"], ref, add, H, False), c["m"])
            if t == torch.bfloat16:
                bound = bound + rr.ulp_bf16(ref * c["m"].to(F64))
            dr.within((f"{name} {dt}", "dx_lp alone"), lpr.t, ref * c["m"].to(F64), bound)
            continue
        assert rc == INVALID, rc
        for g, n in ((dxr, "dx"), (lpr, "dx_lp"), (dgr, "dgamma"), (dbr, "dbeta")):
            g.intact(f"refused {name}, {n}")
    rc = (L().etp_ln_stream_bwd_drop(e, ptr(c["dy"]), ptr(c["x"]), ptr(c["stats"]), ptr(c["gamma"]), ptr(add), gptr(dx), None, None, None, M, H,
                                     stream(), sref))
    assert rc == INVALID, rc
    unchanged("ln_bwd_s", inputs, before)


# ---- cast_drop -----------------------------------------------------------------------------------------------------------------
CAST = dr.cast_cases()


def _cast(e, t, src, n, site_ref, plain=False):
    dst = mv.guarded((n,), t)
    args = (e, ptr(src), gptr(dst), n, stream())
    check(L().etp_cast_f32_to(*args) if plain else L().etp_cast_f32_to_drop(*args, site_ref), "cast_f32_to")
    torch.cuda.synchronize()
    dst.check("cast_f32_to dst")
    return dst.t


@pytest.mark.parametrize("i", range(len(CAST)), ids=ids(CAST))
def test_cast_drop(i):
    dt, n, p, triple = CAST[i]
    site = dr.cast_site(p, triple, n)
    t, e = TDT[dt], EDT[dt]
    src = dr.cast_case(n, seed=500 + i, device=DEV)
    before = src.clone()
    m = site.flat(n, device=DEV)
    keep, sref = csite(site)
    dst, dst2 = _cast(e, t, src, n, sref), _cast(e, t, src, n, sref)
    mv.exact("cast_f32_to_drop (second run)", dst, dst2)
    dr.check_cast(f"etp_cast_f32_to_drop {dt} n={n}", dst, src, m)
    plain = _cast(e, t, src, n, None, plain=True)
    zero, zref = csite(dr.Site(0.0, triple))
    mv.exact("cast_f32_to_drop with NULL against the plain entry point", _cast(e, t, src, n, None), plain)
    mv.exact("cast_f32_to_drop with p = 0 against the plain entry point", _cast(e, t, src, n, zref), plain)
    tiny, tref = csite(dr.Site(dr.P_TINY, triple))
    mv.exact("cast_f32_to_drop p = 1e-6: dst = RNE(src / (1 - p))", _cast(e, t, src, n, tref), (src * float(dr.inv_keep(dr.P_TINY))).to(t))
    mv.exact("cast_f32_to_drop: src unchanged", src, before)


def test_bad_sites_are_refused():
    """p outside [0, 1), a slot of 16 and negative fields are refused before anything is launched"""
    n = 8
    src, dst = dr.cast_case(n, seed=9, device=DEV), mv.guarded((n,), F32)
    for bad in ((1.0, 1, 0, 0), (-0.1, 1, 0, 0), (0.1, 1, 0, 16), (0.1, -1, 0, 0), (0.1, 1, -1, 0), (0.1, 1, 0, -1)):
        s = _lib.DropSite(bad[0], dr.SEED, bad[1], bad[2], bad[3])
        assert L().etp_cast_f32_to_drop(_lib.ETP_F32, ptr(src), gptr(dst), n, stream(), ctypes.byref(s)) == INVALID, bad
    torch.cuda.synchronize()
    dst.intact("refused cast")
