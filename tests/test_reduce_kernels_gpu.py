"""Op-level tests of the row-reducing kernels against float64 references with ELEMENTWISE derived bounds (tests/reduce_ref.py), through
the C ABI:

  etp_ln_fwd / etp_ln_bwd                           ln_fwd_kernel<T>, ln_bwd_kernel<T>                 (norm.hip)
  etp_ln_stream_bwd                                 ln_bwd_s_kernel<T>, atomic mode (128 blocks)
  etp_ln_stream_bwd_stage1 + etp_ln_part_reduce     ln_bwd_s_kernel<T> slab mode + ln_part_reduce_kernel
  etp_text_embed_fwd / _bwd                         text_embed_fwd_kernel<T>, text_embed_bwd_kernel    (embed.hip)
  etp_sap_ce                                        sap_ce_kernel
  etp_gather_sum, etp_colsum                        gather_sum_kernel<T>, colsum_kernel<T>
  etp_cast_f32_to_bf16 / _bf16_to_f32, etp_scale_f32

The cases come from the lists of reduce_ref.py and nowhere else (tests/test_reduce_bounds_cpu.py emulates every one of them on the
CPU).  Every output is filled with NaN, every accumulated buffer with a random "previous gradient", and every output lives inside a
guarded buffer whose 64 guard elements on either side must survive bit for bit.  `stats` handed to a backward kernel are the fp64
statistics rounded to fp32, so that each kernel is judged alone.

A second run is compared bit for bit wherever no atomics are involved:
  LayerNorm            dx, dx_lp, y, stats (every mode); the slabs of stage 1; dgamma / dbeta only where one workgroup (atomic modes) or
                       one chunk of slabs (two-stage) adds onto them
  text embedding       the forward (y, y_lp, stats); every gradient of the backward goes through atomics
  cross-entropy        loss and dlogits (one workgroup, no atomics)
  gather_sum, casts    everything
  colsum               db where M <= 64 (one atomic per column)

The module prints reduce_ref.WORST after its last case (pytest -s); the figures of the MI355X run are in profiles/reduce_op_bounds.txt.
"""
import pytest
import torch

pytestmark = pytest.mark.gpu

from etpnav_amd import _lib  # noqa: E402
from etpnav_amd._lib import check, ptr  # noqa: E402
from tests import reduce_ref as rf  # noqa: E402

DEV = "cuda"
F64 = torch.float64
TDT = {"fp32": torch.float32, "bf16": torch.bfloat16}
EDT = {"fp32": _lib.ETP_F32, "bf16": _lib.ETP_BF16}
INVALID = -1


def L():
    return _lib.lib()


def stream():
    return torch.cuda.current_stream().cuda_stream


Guarded, gptr = rf.Guarded, rf.gptr


@pytest.fixture(scope="module", autouse=True)
def report_worst():
    yield
    print("\nreductions, worst err / bound per (entry point, tensor):\n" + rf.worst_table())


def ids(cases):
    return ["-".join(str(v) for v in c) for c in cases]


# ---- typed LayerNorm: etp_ln_fwd / etp_ln_bwd ------------------------------------------------------------------------------------
TYPED = rf.ln_typed_cases()
FWD_ONLY = [(dt, H, M, rf.LN_EPS[i % 2], False, False) for i, (dt, H) in enumerate((d, h) for d in ("fp32", "bf16") for h in rf.LN_H)
            for M in rf.LN_FWD_ONLY_M]


@pytest.mark.parametrize("case", TYPED + FWD_ONLY, ids=ids(TYPED + FWD_ONLY))
def test_ln_typed_fwd_bwd(case):
    dt, H, M, eps, with_add, with_params = case
    t, e = TDT[dt], EDT[dt]
    blocks = rf.ln_typed_blocks(M)
    c = rf.ln_case(M, H, eps, blocks, False, seed=M + H, dtype=t, device=DEV)
    torch.manual_seed(M + H)
    beta = 0.5 * torch.randn(H, device=DEV)
    with_stats = with_params or case in FWD_ONLY
    runs = []
    for _ in range(2):
        y, stats = Guarded((M, H), t), Guarded((M, 2)) if with_stats else None
        check(L().etp_ln_fwd(e, ptr(c["x"]), ptr(c["gamma"]), ptr(beta), gptr(y), gptr(stats), M, H, eps, stream()), "ln_fwd")
        torch.cuda.synchronize()
        y.check("ln_fwd y")
        runs.append((y, stats))
    rf.same_bits("ln_fwd y (second run)", runs[0][0].t, runs[1][0].t)
    ref_y, ref_st = rf.ln_fwd(c["x"], c["gamma"], beta, eps)
    by, bst = rf.ln_fwd_bounds(c["x"], c["gamma"], beta, eps, ref_y, ref_st, t == torch.bfloat16)
    rf.within(("etp_ln_fwd " + dt, "y"), y.t, ref_y, by)
    if with_stats:
        stats.check("ln_fwd stats")
        rf.same_bits("ln_fwd stats (second run)", runs[0][1].t, runs[1][1].t)
        rf.within(("etp_ln_fwd " + dt, "stats"), stats.t, ref_st, bst)
    if case in FWD_ONLY:
        return
    add = c["add"] if with_add else None
    runs = []
    for _ in range(2):
        dx = Guarded((M, H), t)
        dg = Guarded((H,), init=c["init_g"]) if with_params else None
        db = Guarded((H,), init=c["init_b"]) if with_params else None
        check(L().etp_ln_bwd(e, ptr(c["dy"]), ptr(c["x"]), ptr(c["stats"]), ptr(c["gamma"]), ptr(add), gptr(dx), gptr(dg), gptr(db), M, H,
                             stream()), "ln_bwd")
        torch.cuda.synchronize()
        for g, n in ((dx, "dx"), (dg, "dgamma"), (db, "dbeta")):
            if g is not None:
                g.check("ln_bwd " + n)
        runs.append((dx, dg, db))
    rf.same_bits("ln_bwd dx (second run)", runs[0][0].t, runs[1][0].t)
    if with_params and blocks == 1:
        rf.same_bits("ln_bwd dgamma (second run, one workgroup)", runs[0][1].t, runs[1][1].t)
    rf.check_ln_bwd("etp_ln_bwd " + dt, c, dx.t, None, dg.t if dg else None, db.t if db else None, add)


def test_ln_refusals():
    """a mixed NULL pair of dgamma / dbeta and misaligned pointers are refused before anything is launched"""
    M, H = 8, 256
    x, dy = torch.randn(M * H + 4, device=DEV), torch.randn(M * H + 4, device=DEV)
    gamma, beta, stats = torch.ones(H + 4, device=DEV), torch.zeros(H + 4, device=DEV), torch.zeros(M, 2, device=DEV)
    stats[:, 1] = 1.0
    out, dg, db, lp = Guarded((M * H + 4,)), Guarded((H,)), Guarded((H,)), Guarded((M * H + 4,), torch.bfloat16)
    s, f, b = stream(), _lib.ETP_F32, _lib.ETP_BF16
    o1, x1, g1 = out.t[1:], x[1:], gamma[1:]                                # 4 bytes off a 16-byte boundary
    lp1 = lp.t[1:]                                                          # 2 bytes off an 8-byte boundary
    calls = [
        L().etp_ln_bwd(f, ptr(dy), ptr(x), ptr(stats), ptr(gamma), None, gptr(out), gptr(dg), None, M, H, s),
        L().etp_ln_bwd(f, ptr(dy), ptr(x), ptr(stats), ptr(gamma), None, gptr(out), None, gptr(db), M, H, s),
        L().etp_ln_stream_bwd(f, ptr(dy), ptr(x), ptr(stats), ptr(gamma), None, gptr(out), None, gptr(dg), None, M, H, s),
        L().etp_ln_fwd(f, x1.data_ptr(), ptr(gamma), ptr(beta), gptr(out), None, M, H, 1e-5, s),
        L().etp_ln_fwd(f, ptr(x), ptr(gamma), ptr(beta), o1.data_ptr(), None, M, H, 1e-5, s),
        L().etp_ln_fwd(f, ptr(x), g1.data_ptr(), ptr(beta), gptr(out), None, M, H, 1e-5, s),
        L().etp_ln_fwd(b, ptr(lp.t), ptr(gamma), ptr(beta), lp1.data_ptr(), None, M, H, 1e-5, s),
        L().etp_ln_bwd(f, ptr(dy), x1.data_ptr(), ptr(stats), ptr(gamma), None, gptr(out), None, None, M, H, s),
        L().etp_ln_bwd(f, ptr(dy), ptr(x), ptr(stats), ptr(gamma), x1.data_ptr(), gptr(out), None, None, M, H, s),
        L().etp_ln_stream_fwd(b, ptr(x), ptr(gamma), ptr(beta), gptr(out), lp1.data_ptr(), None, M, H, 1e-5, s),
        L().etp_ln_stream_bwd(f, ptr(dy), ptr(x), ptr(stats), ptr(gamma), None, o1.data_ptr(), None, None, None, M, H, s),
        L().etp_ln_stream_bwd(b, ptr(dy), ptr(x), ptr(stats), ptr(gamma), None, gptr(out), lp1.data_ptr(), None, None, M, H, s),
        L().etp_ln_stream_bwd_stage1(f, x1.data_ptr(), ptr(x), ptr(stats), ptr(gamma), None, gptr(out), None, gptr(dg), gptr(db),
                                     gptr(out), M, H, s),
    ]
    torch.cuda.synchronize()
    assert calls == [INVALID] * len(calls), calls
    for g, n in ((out, "out"), (dg, "dgamma"), (db, "dbeta"), (lp, "lp")):
        g.intact("refused LayerNorm call, " + n)


# ---- LayerNorm on the fp32 stream: atomic path ---------------------------------------------------------------------------------
ATOMIC = rf.ln_atomic_cases()


def _stream_outputs(outs, M, H, t):
    dx = Guarded((M, H)) if outs in ("dx", "both") else None
    lp = Guarded((M, H), t) if outs in ("lp", "both") else None
    return dx, lp


@pytest.mark.parametrize("case", ATOMIC, ids=ids(ATOMIC))
def test_ln_stream_bwd_atomic(case):
    dt, H, M, eps, outs, with_add, with_params = case
    blocks = rf.ln_atomic_blocks(M)
    c = rf.ln_case(M, H, eps, blocks, False, seed=M + H + 1, device=DEV)
    add = c["add"] if with_add else None
    runs = []
    for _ in range(2):
        dx, lp = _stream_outputs(outs, M, H, TDT[dt])
        dg = Guarded((H,), init=c["init_g"]) if with_params else None
        db = Guarded((H,), init=c["init_b"]) if with_params else None
        check(L().etp_ln_stream_bwd(EDT[dt], ptr(c["dy"]), ptr(c["x"]), ptr(c["stats"]), ptr(c["gamma"]), ptr(add), gptr(dx), gptr(lp),
                                    gptr(dg), gptr(db), M, H, stream()), "ln_stream_bwd")
        torch.cuda.synchronize()
        for g, n in ((dx, "dx"), (lp, "dx_lp"), (dg, "dgamma"), (db, "dbeta")):
            if g is not None:
                g.check("ln_stream_bwd " + n)
        runs.append((dx, lp, dg, db))
    for i, n in enumerate(("dx", "dx_lp")):
        if runs[0][i] is not None:
            rf.same_bits(f"ln_stream_bwd {n} (second run)", runs[0][i].t, runs[1][i].t)
    if with_params and blocks == 1:
        rf.same_bits("ln_stream_bwd dgamma (second run, one workgroup)", runs[0][2].t, runs[1][2].t)
    rf.check_ln_bwd("etp_ln_stream_bwd", c, dx.t if dx else None, lp.t if lp else None, dg.t if dg else None, db.t if db else None, add)


# ---- LayerNorm on the fp32 stream: stage 1 + part reduce -----------------------------------------------------------------------
STAGE = rf.ln_stage_cases()


@pytest.mark.parametrize("case", STAGE, ids=ids(STAGE))
def test_ln_stream_bwd_two_stage(case, etp_opt):
    dt, H, M, eps, grid, outs, with_add = case
    if grid is not None:
        etp_opt("LNBWD_GRID", grid)
    blocks = rf.ln_stage_blocks(M, grid)
    nbytes = int(L().etp_ln_bwd_part_bytes(M, H))
    assert nbytes == rf.ln_part_bytes(M, H, grid) == 2 * H * 4 * blocks
    c = rf.ln_case(M, H, eps, blocks, True, seed=M + H + 2, device=DEV)
    add = c["add"] if with_add else None
    runs = []
    for _ in range(2):
        dx, lp = _stream_outputs(outs, M, H, TDT[dt])
        dg, db = Guarded((H,), init=c["init_g"]), Guarded((H,), init=c["init_b"])
        part = torch.full((nbytes // 2,), float("nan"), device=DEV)             # twice etp_ln_bwd_part_bytes: the second half is a sentinel
        half = part[nbytes // 4:].clone()
        check(L().etp_ln_stream_bwd_stage1(EDT[dt], ptr(c["dy"]), ptr(c["x"]), ptr(c["stats"]), ptr(c["gamma"]), ptr(add), gptr(dx), gptr(lp),
                                           gptr(dg), gptr(db), ptr(part), M, H, stream()), "ln stage 1")
        torch.cuda.synchronize()
        dg.intact("stage 1 dgamma")
        db.intact("stage 1 dbeta")
        slabs = part[:nbytes // 4].clone()
        assert bool(torch.isfinite(slabs).all()), "stage 1 left a slab element unwritten"
        check(L().etp_ln_part_reduce(ptr(part), M, H, gptr(dg), gptr(db), stream()), "ln stage 2")
        torch.cuda.synchronize()
        rf.same_bits("slab buffer beyond etp_ln_bwd_part_bytes", part[nbytes // 4:], half)
        rf.same_bits("slabs after stage 2 (read only)", part[:nbytes // 4], slabs)
        for g, n in ((dx, "dx"), (lp, "dx_lp"), (dg, "dgamma"), (db, "dbeta")):
            if g is not None:
                g.check("two-stage " + n)
        runs.append((dx, lp, dg, db, slabs))
    for i, n in enumerate(("dx", "dx_lp")):
        if runs[0][i] is not None:
            rf.same_bits(f"two-stage {n} (second run)", runs[0][i].t, runs[1][i].t)
    rf.same_bits("slabs (second run)", runs[0][4], runs[1][4])
    if blocks <= rf.LN_PART_CHUNK:
        rf.same_bits("two-stage dgamma (second run, one chunk)", runs[0][2].t, runs[1][2].t)
        rf.same_bits("two-stage dbeta (second run, one chunk)", runs[0][3].t, runs[1][3].t)
    rf.check_ln_bwd("etp_ln_stream_bwd_stage1+reduce", c, dx.t if dx else None, lp.t if lp else None, dg.t, db.t, add)


# ---- text embedding ------------------------------------------------------------------------------------------------------------
TEXT = rf.text_cases()


@pytest.mark.parametrize("i", range(len(TEXT)), ids=ids(TEXT))
def test_text_embed_fwd_bwd(i):
    """the forward is deterministic (second run bit for bit: y, y_lp, stats); the backward's five gradients all go through atomics"""
    dt, H, B, Lt, kind, eps, bwd = TEXT[i]
    c = rf.text_reference(rf.text_case(B, Lt, H, kind, eps, seed=i, device=DEV), bwd)
    M = B * Lt
    runs = []
    for _ in range(2):
        y, lp, stats = Guarded((M, H)), Guarded((M, H), TDT[dt]) if i % 3 else None, Guarded((M, 2))
        check(L().etp_text_embed_fwd(EDT[dt], ptr(c["ids"]), ptr(c["word"]), ptr(c["pos"]), ptr(c["type0"]), ptr(c["gamma"]), ptr(c["beta"]),
                                     gptr(y), gptr(lp), gptr(stats), B, Lt, H, eps, stream()), "text_embed_fwd")
        torch.cuda.synchronize()
        for g, n in ((y, "y"), (lp, "y_lp"), (stats, "stats")):
            if g is not None:
                g.check("text_embed_fwd " + n)
        runs.append((y, lp, stats))
    for a, b in zip(*runs):
        if a is not None:
            rf.same_bits("text_embed_fwd (second run)", a.t, b.t)
    rf.check_text_fwd("etp_text_embed_fwd", c, y.t, lp.t if lp else None, stats.t)
    if not bwd:
        return
    names = ("dword", "dpos", "dtype0", "dgamma", "dbeta")
    got = {k: Guarded(tuple(c["init_" + k].shape), init=c["init_" + k]) for k in names}
    check(L().etp_text_embed_bwd(EDT[dt], ptr(c["dy"]), ptr(c["ids"]), ptr(c["word"]), ptr(c["pos"]), ptr(c["type0"]), ptr(c["gamma"]),
                                 ptr(c["stats"]), *[gptr(got[k]) for k in names], B, Lt, H, stream()), "text_embed_bwd")
    torch.cuda.synchronize()
    for k in names:
        got[k].check("text_embed_bwd " + k)
    rf.check_text_bwd("etp_text_embed_bwd", c, {k: got[k].t for k in names})


# ---- cross-entropy -------------------------------------------------------------------------------------------------------------
CE = rf.ce_cases()


@pytest.mark.parametrize("i", range(len(CE)), ids=ids(CE))
def test_sap_ce(i):
    B, G, pat = CE[i]
    logits, labels, scale, ii = rf.ce_case(B, G, pat, seed=i, device=DEV)
    runs = []
    for with_dl in (True, True, False):
        loss = Guarded((1,))
        dl = Guarded((B, G)) if with_dl else None
        check(L().etp_sap_ce(ptr(logits), ptr(labels), gptr(loss), gptr(dl), B, G, scale, ii, stream()), "sap_ce")
        torch.cuda.synchronize()
        loss.check("sap_ce loss")
        if dl is not None:
            dl.check("sap_ce dlogits")
        rf.check_ce("etp_sap_ce", loss.t, dl.t if dl else None, logits, labels, scale, ii)
        runs.append((loss, dl))
    rf.same_bits("sap_ce loss (second run)", runs[0][0].t, runs[1][0].t)
    rf.same_bits("sap_ce loss (dlogits NULL)", runs[0][0].t, runs[2][0].t)
    rf.same_bits("sap_ce dlogits (second run)", runs[0][1].t, runs[1][1].t)


# ---- gather_sum ----------------------------------------------------------------------------------------------------------------
GATHER = [(dt, H, N, acc) for dt in ("fp32", "bf16") for H in rf.GATHER_H for N in rf.GATHER_N for acc in (0, 1)]


@pytest.mark.parametrize("case", GATHER, ids=ids(GATHER))
def test_gather_sum(case):
    dt, H, N, acc = case
    t = TDT[dt]
    src, p, idx, w, init = rf.gather_case(N, H, t, seed=N + H, device=DEV)
    rows = N + 3                                                       # rows >= N are untouched
    full = torch.cat([init, torch.randn(3, H, device=DEV).to(t)])
    runs = []
    for _ in range(2):
        out = Guarded((rows, H), t, init=full)
        check(L().etp_gather_sum(EDT[dt], ptr(src), ptr(p), ptr(idx), ptr(w), gptr(out), N, H, acc, stream()), "gather_sum")
        torch.cuda.synchronize()
        out.check("gather_sum out")
        runs.append(out)
    rf.same_bits("gather_sum (second run)", runs[0].t, runs[1].t)
    rf.same_bits("gather_sum rows >= N", out.t[N:], full[N:])
    ref, mag, lens = rf.gather_sum(src, p, idx, w, init if acc else None)
    rf.within(("etp_gather_sum " + dt, "out"), out.t[:N], ref, rf.gather_bound(ref, mag, lens, acc, t == torch.bfloat16))


# ---- colsum --------------------------------------------------------------------------------------------------------------------
COLSUM = [(dt, M, N, pad) for dt in ("fp32", "bf16") for M in rf.COLSUM_M for N in rf.COLSUM_N for pad in (0, 8)]


@pytest.mark.parametrize("case", COLSUM, ids=ids(COLSUM))
def test_colsum(case):
    dt, M, N, pad = case
    dy, init, bound, _ = rf.colsum_case(M, N, TDT[dt], seed=M * N, device=DEV)
    buf = torch.full((M, N + pad), float("nan"), device=DEV, dtype=TDT[dt])        # the pad columns hold NaN
    buf[:, :N] = dy
    runs = []
    for _ in range(2):
        db = Guarded((N,), init=init)
        check(L().etp_colsum(EDT[dt], ptr(buf), N + pad, gptr(db), M, N, stream()), "colsum")
        torch.cuda.synchronize()
        db.check("colsum db")
        runs.append(db)
    if M <= 64:
        rf.same_bits("colsum db (second run, one atomic per column)", runs[0].t, runs[1].t)
    rf.within(("etp_colsum " + dt, "db"), db.t, init.to(F64) + rf.colsum(dy), bound)


def test_colsum_refusals():
    dy, db = torch.randn(8, 16, device=DEV), Guarded((16,), init=torch.randn(16, device=DEV))
    s = stream()
    calls = [L().etp_colsum(_lib.ETP_F32, ptr(dy), 16, gptr(db), 8, 6, s), L().etp_colsum(_lib.ETP_F32, ptr(dy), 14, gptr(db), 8, 12, s),
             L().etp_colsum(_lib.ETP_F32, dy.view(-1)[1:].data_ptr(), 16, gptr(db), 7, 12, s),
             L().etp_colsum(_lib.ETP_BF16, dy.view(-1)[1:].data_ptr(), 16, gptr(db), 7, 12, s)]
    torch.cuda.synchronize()
    assert calls == [INVALID] * 4, calls
    db.intact("refused colsum")
    src, p, idx, w, init = rf.gather_case(3, 256, torch.float32, seed=1, device=DEV)
    flat = torch.cat([src.view(-1), src.view(-1)[:4]])
    out = Guarded((3 * 256 + 4,))
    calls = [L().etp_gather_sum(_lib.ETP_F32, flat[1:].data_ptr(), ptr(p), ptr(idx), ptr(w), gptr(out), 3, 256, 0, s),
             L().etp_gather_sum(_lib.ETP_F32, ptr(src), ptr(p), ptr(idx), ptr(w), out.t[1:].data_ptr(), 3, 256, 0, s)]
    torch.cuda.synchronize()
    assert calls == [INVALID] * 2, calls
    out.intact("refused gather_sum")


# ---- casts and scale -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", rf.CAST_N)
def test_cast_f32_to_bf16(n):
    torch.manual_seed(n)
    sp = rf.cast_specials(DEV)
    src = torch.randn(n, device=DEV) * 2.0 ** torch.randint(-20, 20, (n,), device=DEV).float()
    k = min(n, sp.numel())
    src[:k] = sp[:k] if n > 9 else sp[n:n + k]                          # the short sizes walk through the list of specials
    if n > 100:
        src[-sp.numel():] = sp                                          # and the scalar tail of the last thread sees them too
    runs = []
    for _ in range(2):
        dst = Guarded((n,), torch.bfloat16)
        check(L().etp_cast_f32_to_bf16(ptr(src), gptr(dst), n, stream()), "cast_f32_to_bf16")
        torch.cuda.synchronize()
        dst.check("cast_f32_to_bf16")
        runs.append(dst)
    rf.check_cast("etp_cast_f32_to_bf16", dst.t, src)
    finite = ~torch.isnan(src)
    rf.same_bits("cast (second run)", runs[0].t[finite], runs[1].t[finite])


@pytest.mark.parametrize("n", rf.SCALE_N)
def test_cast_back_and_scale(n):
    torch.manual_seed(n)
    src = (torch.randn(n, device=DEV) * 3).to(torch.bfloat16)
    for scale in rf.SCALES:
        scale = rf.f32(scale)
        dst = Guarded((n,))
        check(L().etp_cast_bf16_to_f32(ptr(src), gptr(dst), n, scale, stream()), "cast_bf16_to_f32")
        p = Guarded((n,), init=src.float())
        check(L().etp_scale_f32(gptr(p), n, scale, stream()), "scale_f32")
        torch.cuda.synchronize()
        dst.check("cast_bf16_to_f32")
        p.check("scale_f32")
        want = (src.to(F64) * scale).float()                                # the single-rounded fp32 product
        rf.same_bits("etp_cast_bf16_to_f32", dst.t, want)
        rf.same_bits("etp_scale_f32", p.t, want)
