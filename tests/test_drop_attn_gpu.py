"""Dropout on the attention probabilities at operator level, through etp_attn_fwd_drop / etp_attn_bwd_drop (and the two folded
entry points), on every kernel family -- each case ASSERTS its family (etp_attn_family under the switches it sets) -- against
tests/drop_ref.py's fp64 restatement (Pd = P * m, ctx = Pd V, dP = (dO V^T) * m, dV = Pd^T dO; P itself and the softmax backward
undropped) under attn_ref's derived bound evaluated on the dropped operands.

  family 2 register-resident   bf16, (Lq, Lk) in (5, 5), (21, 21), (64, 37), (16, 80), (128, 128): with Lk = 21 and 37 the runs of four
                               start at odd element indices on every odd query row (drop_mult_run's second branch)    attn_rows.hip
  family 1 LDS-tile            the same pairs in bf16 under ATTN_ROWS=0; fp32 at the pairs <= 64                       attn.hip
  family 3 streaming           bf16 (64, 129) and (130, 200)                                                           attn.hip flash_*
  family 0 batched-GEMM        fp32 (70, 70) and bf16 (130, 200) with the distance bias: drop_rows + the second probability
                               buffer `Pd` of the _drop entries; refused without it                         planner.hip, norm.hip
Every pair with both mask modes (key 0 / every fifth key / the last keys invalid) and the distance bias on and off (family 3 has
none), B x heads alternating 2 x 12 and 3 x 2, p alternating 0.1 and 0.4, two sites, ldS = round_up(Lk, 8) + 8.

Every case:
  mask read-out, exact   one-hot probes: ctx with V[key] = e_(key mod 64), one launch per 64-key block, reads the FORWARD's mask;
                         dV with dO[q] = e_(q mod 64), one backward per 64-query block, reads the mask the BACKWARD regenerates.
                         Exact zeros == {multiplier == 0} over every valid key (P > 0; masked-out keys are left out of this
                         comparison and of nothing else), after the reference alone has shown that no kept probability can read
                         as zero
  values                 ctx, dQ, dK, dV, d_sp_w, d_sp_b under the bound (d_sp_* onto a previous gradient)
  plain entry            _drop with NULL and with p = 0 leaves the bits of etp_attn_fwd / etp_attn_bwd; p = 1e-6 scales by 1 / (1 - p)
  harness                NaN-filled outputs inside sentinel rows and columns, a second run bit for bit
"""
import ctypes
import math

import pytest
import torch

pytestmark = pytest.mark.gpu

from etpnav_amd import _lib  # noqa: E402
from etpnav_amd._lib import AttnDesc, AttnBwdDesc, GemmDesc, check  # noqa: E402
from tests import attn_ref as ar  # noqa: E402
from tests import drop_ref as dr  # noqa: E402

DEV = "cuda"
SENTINEL = -777.0
GUARD = 8
INVALID = -1


def L():
    return _lib.lib()


def stream():
    return torch.cuda.current_stream().cuda_stream


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
    cells = sorted({k.rsplit("/", 1)[0] for k in ar.WORST if k.startswith("drop ")})
    print("\nattention dropout, worst |got - fp64| / E per (family, dtype, tensor):")
    for cell in cells:
        print(f"  {cell:36s} " + "  ".join(f"{n} {ar.WORST[f'{cell}/{n}'][0]:.3f}" for n in ar.NAMES if f"{cell}/{n}" in ar.WORST))


class Guarded:
    """[rows, H] output at leading dimension ld with GUARD rows before and after; NaN inside, SENTINEL around"""

    def __init__(self, rows, H, ld, t):
        self.rows, self.H = rows, H
        self.buf = torch.full((rows + 2 * GUARD, ld), SENTINEL, device=DEV, dtype=t)
        self.buf[GUARD:GUARD + rows, :H] = float("nan")
        self.ptr = self.buf.data_ptr() + GUARD * ld * self.buf.element_size()

    def out(self):
        return self.buf[GUARD:GUARD + self.rows, :self.H]

    def check(self, name):
        got = self.buf.clone()
        got[GUARD:GUARD + self.rows, :self.H] = SENTINEL
        ar.same_bits(f"{name}: guard rows / extra columns", got, torch.full_like(got, SENTINEL))


def csite(site):
    return None if site is None else _lib.DropSite(site.p, site.seed, site.mode, site.layer, site.slot)


def run(c, bf16, expect, site, v=None, dctx=None, plain=False, d_init=None, with_pd=True, backward=True):
    """forward (+ backward on what it left) on fresh buffers -> dict of [B, heads, L, 64] outputs.  v / dctx: probe operands."""
    t, dtype = (torch.bfloat16, _lib.ETP_BF16) if bf16 else (torch.float32, _lib.ETP_F32)
    B, nh, Lq, Lk = c["B"], c["nh"], c["Lq"], c["Lk"]
    H = nh * 64
    ldo = H + 64
    ldS = (Lk + 7) // 8 * 8 + 8
    qm, km_, vm = (ar.merge_heads(x).to(DEV).to(t).contiguous() for x in (c["q"], c["k"], c["v"] if v is None else v))
    P = torch.full((B, nh, Lq, ldS), float("nan"), device=DEV, dtype=t)
    dP = torch.full_like(P, float("nan"))
    Pd = torch.full_like(P, float("nan")) if (expect == 0 and with_pd) else None
    ctx, dq = Guarded(B * Lq, H, ldo, t), Guarded(B * Lq, H, ldo, t)
    dk, dv = Guarded(B * Lk, H, ldo, t), Guarded(B * Lk, H, ldo, t)
    km = c["km"].to(DEV).contiguous()
    dist = None if c["dist"] is None else c["dist"].to(DEV).contiguous()
    w, b0 = torch.tensor([c["sp_w"]], device=DEV), torch.tensor([c["sp_b"]], device=DEV)
    d = AttnDesc()
    d.dtype, d.B, d.heads, d.Lq, d.Lk, d.ldS = dtype, B, nh, Lq, Lk, ldS
    d.Q, d.ldq, d.K, d.ldk, d.V, d.ldv = qm.data_ptr(), H, km_.data_ptr(), H, vm.data_ptr(), H
    d.P, d.ctx, d.ldc = P.data_ptr(), ctx.ptr, ldo
    d.keymask, d.mask_mode, d.alpha = km.data_ptr(), c["mask_mode"], c["alpha"]
    if dist is not None:
        d.dist, d.sp_w, d.sp_b = dist.data_ptr(), w.data_ptr(), b0.data_ptr()
    fam = L().etp_attn_family(ctypes.byref(d))
    assert fam == expect, f"this case meant family {expect}, the dispatch takes family {fam}"
    s = csite(site)
    sref = None if s is None else ctypes.byref(s)
    pd = None if Pd is None else Pd.data_ptr()
    rc = L().etp_attn_fwd(ctypes.byref(d), stream()) if plain else L().etp_attn_fwd_drop(ctypes.byref(d), stream(), pd, sref)
    torch.cuda.synchronize()
    if rc != 0 or not backward:
        ctx.check("ctx")
        return {"rc": rc, "ctx": ar.split_heads(ctx.out(), B, nh), "ctx_buf": ctx}
    do = ar.merge_heads(c["dctx"] if dctx is None else dctx).to(DEV).to(t).contiguous()
    bd = AttnBwdDesc()
    bd.f = d
    bd.dctx, bd.ldd, bd.dP = do.data_ptr(), H, dP.data_ptr()
    bd.dQ, bd.lddq, bd.dK, bd.lddk, bd.dV, bd.lddv = dq.ptr, ldo, dk.ptr, ldo, dv.ptr, ldo
    dwb = None
    if dist is not None:
        dwb = torch.tensor(d_init if d_init is not None else [0.0, 0.0], device=DEV, dtype=torch.float32)
        bd.d_sp_w, bd.d_sp_b = dwb.data_ptr(), dwb.data_ptr() + 4
    rc = L().etp_attn_bwd(ctypes.byref(bd), stream()) if plain else L().etp_attn_bwd_drop(ctypes.byref(bd), stream(), pd, sref)
    torch.cuda.synchronize()
    check(rc, "attn_bwd")
    out = {"rc": 0}
    for n, g in (("ctx", ctx), ("dQ", dq), ("dK", dk), ("dV", dv)):
        g.check(n)
        out[n] = ar.split_heads(g.out(), B, nh)
    if dwb is not None:
        out["d_sp_w"], out["d_sp_b"] = dwb[0], dwb[1]
    return out


def one_case(cell, Lq, Lk, B, nh, bf16, expect, mask_mode, with_dist, site, seed, etp_opt, opts):
    for k in ("ATTN_ROWS", "ATTN_FUSED", "ATTN_FLASH", "ATTN_Q96"):
        etp_opt(k, opts.get(k))
    c = dr.attn_case(Lq, Lk, B, nh, bf16, mask_mode, with_dist, seed)
    name = f"{cell} {Lq}x{Lk} B{B}x{nh} mode {mask_mode}{' dist' if with_dist else ''} p {site.p}"
    gemm, tile = expect == 0, expect == 1
    m = dr.attn_index_mask(site, B, nh, Lq, Lk, device=DEV)
    val, E = dr.attn_ref(c, m, gemm=gemm, tile=tile, device=DEV)
    d_init = None
    if with_dist:
        d_init = [2.5 * float(E["d_sp_w"]), -2.25 * float(E["d_sp_b"])]
    got = run(c, bf16, expect, site, d_init=d_init)
    d32 = None if d_init is None else [float(torch.tensor(x, dtype=torch.float32)) for x in d_init]
    ar.check_all(got, val, E, name, cell, d32)
    again = run(c, bf16, expect, site, d_init=d_init)
    for n in ("ctx", "dQ", "dK", "dV"):
        ar.same_bits(f"{name}: {n} of a second run", again[n].contiguous(), got[n].contiguous())
    # the plain entry points
    plain = run(c, bf16, expect, None, plain=True)
    for what, s0 in (("NULL", None), ("p = 0", dr.Site(0.0, (site.mode, site.layer, site.slot)))):
        g0 = run(c, bf16, expect, s0)
        for n in ("ctx", "dQ", "dK", "dV"):
            ar.same_bits(f"{name}: {n} with {what} against the plain entry point", g0[n].contiguous(), plain[n].contiguous())
    tiny = run(c, bf16, expect, dr.Site(dr.P_TINY, (site.mode, site.layer, site.slot)))
    vt, Et = dr.attn_ref(c, torch.full_like(m, float(dr.inv_keep(dr.P_TINY))), gemm=gemm, tile=tile, device=DEV)
    ar.check_all(tiny, vt, Et, name + " p = 1e-6", cell + " p=1e-6")
    # mask read-out: the forward's mask through ctx, the backward's through dV
    for j in range((Lk + 63) // 64):
        pv = dr.probe_v(c, j)
        vj, Ej = dr.attn_ref(c, m, gemm=gemm, tile=tile, device=DEV, v=pv)
        gj = run(c, bf16, expect, site, v=pv, backward=False)
        assert gj["rc"] == 0
        dr.probe_ctx_check(f"{name}: ctx probe of key block {j}", c, j, gj["ctx"], m, vj, Ej)
    for i in range((Lq + 63) // 64):
        pdo = dr.probe_do(c, i)
        vi, Ei = dr.attn_ref(c, m, gemm=gemm, tile=tile, device=DEV, dctx=pdo)
        gi = run(c, bf16, expect, site, dctx=pdo)
        dr.probe_dv_check(f"{name}: dV probe of query block {i}", c, i, gi["dV"], m, vi, Ei)


def ids(g):
    return [f"{x[0]}x{x[1]}-B{x[2]}x{x[3]}-m{x[4]}-{'dist' if x[5] else 'nodist'}-p{x[6]}" for x in g]


SHORT_G, F32_G, LONG_G, GEMM_G = dr.ATTN_SHORT_G, dr.ATTN_F32_G, dr.ATTN_LONG_G, dr.ATTN_GEMM_G


def _case(x, cell, bf16, expect, etp_opt, opts):
    Lq, Lk, B, nh, mask_mode, with_dist, p, triple, seed = x
    one_case(cell, Lq, Lk, B, nh, bf16, expect, mask_mode, with_dist, dr.Site(p, triple), seed, etp_opt, opts)


@pytest.mark.parametrize("x", SHORT_G, ids=ids(SHORT_G))
def test_register_resident_bf16(x, etp_opt):
    _case(x, "drop register-resident bf16", True, 2, etp_opt, {})


@pytest.mark.parametrize("x", SHORT_G, ids=ids(SHORT_G))
def test_lds_tile_bf16(x, etp_opt):
    _case(x, "drop LDS-tile bf16", True, 1, etp_opt, {"ATTN_ROWS": 0})


@pytest.mark.parametrize("x", F32_G, ids=ids(F32_G))
def test_lds_tile_fp32(x, etp_opt):
    _case(x, "drop LDS-tile fp32", False, 1, etp_opt, {})


@pytest.mark.parametrize("x", LONG_G, ids=ids(LONG_G))
def test_streaming_bf16(x, etp_opt):
    _case(x, "drop streaming bf16", True, 3, etp_opt, {})


@pytest.mark.parametrize("x", GEMM_G, ids=ids(GEMM_G))
def test_batched_gemm_with_the_second_probability_buffer(x, etp_opt):
    """fp32 beyond 64 and bf16 with the distance bias beyond 128 go to the batched-GEMM path by themselves: no switch"""
    bf16 = x[0] == 130
    _case(x, "drop batched-GEMM " + ("bf16" if bf16 else "fp32"), bf16, 0, etp_opt, {})


def test_batched_gemm_refuses_dropout_without_the_second_buffer(etp_opt):
    c = dr.attn_case(70, 70, 2, 2, False, 0, False, 5)
    got = run(c, False, 0, dr.Site(0.1, dr.SITES[0]), with_pd=False)
    assert got["rc"] == INVALID and b"second probability buffer" in L().etp_last_error(), (got["rc"], L().etp_last_error())
    assert bool(torch.isnan(got["ctx"].float()).all()), "a refused call wrote ctx"
    assert run(c, False, 0, None, with_pd=False, backward=False)["rc"] == 0             # without a mask the buffer is not needed


# ---- the folded entry points, at shapes the planner takes them (12 heads, H = 768) ----------------------------------------------
def test_fused_qkv_forward_with_dropout():
    """etp_attn_fwd_qkv_drop: ctx is the dropped attention of the Q / K / V stash the kernel wrote; NULL gives etp_attn_fwd_qkv's bits"""
    gen = torch.Generator().manual_seed(7)
    t, nh, B, Lx = torch.bfloat16, 12, 3, 36
    H = nh * 64
    ldS = (Lx + 7) // 8 * 8 + 8
    site = dr.Site(0.4, dr.SITES[1])
    x = (torch.randn(B * Lx, H, generator=gen) * 0.5).to(DEV).to(t)
    W = (torch.randn(3 * H, H, generator=gen) / math.sqrt(H)).to(DEV).to(t)
    bias = (torch.randn(3 * H, generator=gen) * 0.1).to(DEV)
    km = torch.ones(B, Lx, dtype=torch.bool, device=DEV)
    km[1, 0::5] = False
    outs = []
    for s in (csite(site), None, "plain"):
        qkv = torch.full((B * Lx, 3 * H), float("nan"), device=DEV, dtype=t)
        P = torch.full((B, nh, Lx, ldS), float("nan"), device=DEV, dtype=t)
        ctx = Guarded(B * Lx, H, H + 64, t)
        d = AttnDesc()
        d.dtype, d.B, d.heads, d.Lq, d.Lk, d.ldS = _lib.ETP_BF16, B, nh, Lx, Lx, ldS
        d.Q, d.ldq, d.K, d.ldk, d.V, d.ldv = qkv.data_ptr(), 3 * H, qkv.data_ptr() + 2 * H, 3 * H, qkv.data_ptr() + 4 * H, 3 * H
        d.P, d.ctx, d.ldc = P.data_ptr(), ctx.ptr, H + 64
        d.keymask, d.mask_mode, d.alpha = km.data_ptr(), 0, 0.125
        assert L().etp_attn_family(ctypes.byref(d)) == 2
        args = (ctypes.byref(d), x.data_ptr(), H, W.data_ptr(), H, bias.data_ptr(), stream())
        check(L().etp_attn_fwd_qkv(*args) if s == "plain" else L().etp_attn_fwd_qkv_drop(*args, None if s is None else ctypes.byref(s)),
              "attn_fwd_qkv")
        torch.cuda.synchronize()
        ctx.check("ctx")
        outs.append((ar.split_heads(ctx.out(), B, nh), qkv))
    ar.same_bits("etp_attn_fwd_qkv_drop with NULL against the plain entry point", outs[1][0].contiguous(), outs[2][0].contiguous())
    ar.same_bits("the Q / K / V stash does not depend on the mask", outs[0][1], outs[2][1])
    q, k, v = (ar.split_heads(outs[0][1][:, i * H:(i + 1) * H], B, nh).float().cpu() for i in range(3))
    c = dict(q=q, k=k, v=v, dctx=torch.zeros_like(q), km=km.cpu(), dist=None, sp_w=0.0, sp_b=0.0, alpha=0.125, mask_mode=0, bf16=True,
             Lq=Lx, Lk=Lx, B=B, nh=nh)
    m = dr.attn_index_mask(site, B, nh, Lx, Lx, device=DEV)
    val, E = dr.attn_ref(c, m, device=DEV)
    ar.close(outs[0][0], val["ctx"], E["ctx"], "fused QKV with dropout", "drop register-resident bf16 fused QKV/ctx")
    vp, Ep = dr.attn_ref(c, torch.ones_like(m), device=DEV)
    assert float((val["ctx"] - vp["ctx"]).abs().max()) > 10 * float(E["ctx"].max()), "the mask does not show in this case"


def test_folded_out_projection_backward_with_dropout(etp_opt):
    """etp_attn_bwd_proj_drop against the launch pair (etp_gemm into dctx, etp_attn_bwd_drop) and against fp64 on the pair's dctx"""
    etp_opt("ATTN_PROJ", 1)
    B, nh, Lq, Lk, t = 2, 12, 16, 80, torch.bfloat16
    H = nh * 64
    site = dr.Site(0.1, dr.SITES[0])
    c = dr.attn_case(Lq, Lk, B, nh, True, 0, False, 11)
    gen = torch.Generator().manual_seed(3)
    dy = (torch.randn(B * Lq, H, generator=gen) * 0.5).to(DEV).to(t)
    Wo = (torch.randn(H, H, generator=gen) / math.sqrt(H)).to(DEV).to(t)
    dctx = torch.empty(B * Lq, H, device=DEV, dtype=t)
    g = GemmDesc()
    g.A, g.B, g.C, g.M, g.N, g.K, g.lda, g.ldb, g.ldc = dy.data_ptr(), Wo.data_ptr(), dctx.data_ptr(), B * Lq, H, H, H, H, H
    g.trans_a, g.trans_b, g.dtype, g.c_dtype, g.batch, g.batch_inner, g.ksplit, g.alpha = 0, 1, _lib.ETP_BF16, _lib.ETP_BF16, 1, 1, 1, 1.0
    check(L().etp_gemm(ctypes.byref(g), stream()), "out-projection dgrad")
    torch.cuda.synchronize()
    c["dctx"] = ar.split_heads(dctx.float().cpu(), B, nh)
    m = dr.attn_index_mask(site, B, nh, Lq, Lk, device=DEV)
    val, E = dr.attn_ref(c, m, device=DEV)
    pair = run(c, True, 2, site)
    ar.check_all(pair, val, E, "pair with dropout", "drop fold pair")
    # the folded launch: the forward of `run`, then etp_attn_bwd_proj_drop on dY
    ldS = (Lk + 7) // 8 * 8 + 8
    qm, km_, vm = (ar.merge_heads(c[n]).to(DEV).to(t).contiguous() for n in ("q", "k", "v"))
    P = torch.full((B, nh, Lq, ldS), float("nan"), device=DEV, dtype=t)
    ctx = torch.empty(B * Lq, H, device=DEV, dtype=t)
    km = c["km"].to(DEV).contiguous()
    d = AttnDesc()
    d.dtype, d.B, d.heads, d.Lq, d.Lk, d.ldS = _lib.ETP_BF16, B, nh, Lq, Lk, ldS
    d.Q, d.ldq, d.K, d.ldk, d.V, d.ldv = qm.data_ptr(), H, km_.data_ptr(), H, vm.data_ptr(), H
    d.P, d.ctx, d.ldc, d.keymask, d.mask_mode, d.alpha = P.data_ptr(), ctx.data_ptr(), H, km.data_ptr(), 0, c["alpha"]
    s = csite(site)
    check(L().etp_attn_fwd_drop(ctypes.byref(d), stream(), None, ctypes.byref(s)), "attn_fwd_drop")
    outs = []
    for sref in (ctypes.byref(s), ctypes.byref(s), None, "plain"):
        bd = AttnBwdDesc()
        bd.f = d
        dP = torch.empty(B, nh, Lq, ldS, device=DEV, dtype=t)
        dq, dk, dv = Guarded(B * Lq, H, H, t), Guarded(B * Lk, H, H, t), Guarded(B * Lk, H, H, t)
        bd.dctx, bd.ldd, bd.dP = dy.data_ptr(), H, dP.data_ptr()
        bd.dQ, bd.lddq, bd.dK, bd.lddk, bd.dV, bd.lddv = dq.ptr, H, dk.ptr, H, dv.ptr, H
        args = (ctypes.byref(bd), Wo.data_ptr(), H, stream())
        check(L().etp_attn_bwd_proj(*args) if sref == "plain" else L().etp_attn_bwd_proj_drop(*args, sref), "attn_bwd_proj")
        torch.cuda.synchronize()
        for n, gd in (("dQ", dq), ("dK", dk), ("dV", dv)):
            gd.check(n)
        outs.append({"dQ": ar.split_heads(dq.out(), B, nh), "dK": ar.split_heads(dk.out(), B, nh), "dV": ar.split_heads(dv.out(), B, nh)})
    for n in ("dQ", "dK", "dV"):
        ar.close(outs[0][n], val[n], E[n], f"folded with dropout {n}", f"drop fold fused/{n}")
        ar.same_bits(f"folded with dropout, {n} of a second run", outs[1][n].contiguous(), outs[0][n].contiguous())
    # (NULL after a DROPPED forward: lse is the same, so the plain backward's bits must come out)
    for n in ("dQ", "dK", "dV"):
        ar.same_bits(f"etp_attn_bwd_proj_drop with NULL against the plain entry point, {n}", outs[2][n].contiguous(), outs[3][n].contiguous())
    vp, _ = dr.attn_ref(c, torch.ones_like(m), device=DEV)
    assert float((val["dV"] - vp["dV"]).abs().max()) > 10 * float(E["dV"].max()), "the mask does not show in this case"
