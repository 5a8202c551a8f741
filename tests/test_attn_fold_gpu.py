"""The out-projection input gradient folded into the register-resident attention backward (etp_attn_bwd_proj; attn_rows.hip
rows_bwd_kernel<.., PROJ>: weight slabs by LDS-DMA into a ring that aliases the Q / K / V tiles) against the launch pair it replaces
(etp_gemm into dctx, then etp_attn_bwd) and against float64 (tests/attn_ref.py).

Shapes (B = 2, 12 heads, H = 768), by what the prologue does there (w = wavefronts of the workgroup; wavefronts 0..3 issue the DMA):
  (16, 80)  w = 5, one query tile: one wavefront computes, three only load, one only waits at the hand-overs
  (16, 16)  w = 4, one query tile, with the distance bias of the graph self-attention
  (24, 40)  w = 4, two query tiles, a ragged second tile
  (36, 36)  w = 4, three query tiles
  (80, 80)  w = 5 = query tiles: a computing wavefront that issues no DMA
  (64, 80)  four query tiles, a fifth wavefront without one
  (13, 77)  padding on both axes (dY rows past Lq are read clamped and zeroed where the tile is stored)

Reference and bound: attn_ref on the STORED operands, dctx being the bf16 tile the GEMM of the pair stored.  The fused kernel rounds its
own fp32 sums to bf16 at the same point, so it differs from the pair through the order of the fp32 sums only (an occasional bf16 ulp of
dctx); both are held to the bound the pair gets, elementwise, no multiplier.  The same inputs run twice give bit-identical dQ, dK, dV.
Worst |got - fp64| / bound seen on the MI355X: dV 0.72, dQ 0.26, dK 0.24, the same for the pair and the fused launch on every shape.

Attention dropout inside the fused kernel: etp_attn_bwd_proj_drop, tests/test_drop_attn_gpu.py.  Not reachable through
etp_attn_bwd_proj (it takes no kv_mod): the per-episode K/V indirection inside the fused kernel; the planner-level suites run it
through the fused backward (train-mode fixtures with B * heads <= CUs or Lq <= 64).
"""
import ctypes
import math

import pytest
import torch

pytestmark = pytest.mark.gpu

from etpnav_amd import _lib  # noqa: E402
from etpnav_amd._lib import AttnDesc, AttnBwdDesc, GemmDesc, check  # noqa: E402
from tests import attn_ref as ar  # noqa: E402

DEV = "cuda"
B, NH = 2, 12
H = NH * 64
T = torch.bfloat16
#         Lq, Lk, distance bias, mask_mode, first mask pattern of attn_ref.MASKS (batch entry b takes pattern rot + b)
CASES = [(16, 80, False, 0, 0), (16, 16, True, 0, 3), (24, 40, False, 1, 4), (36, 36, False, 0, 3), (80, 80, False, 1, 4),
         (64, 80, False, 0, 5), (13, 77, False, 1, 3)]
IDS = [f"{c[0]}x{c[1]}{'-dist' if c[2] else ''}-m{c[3]}" for c in CASES]
_CACHE = {}


def L():
    return _lib.lib()


def stream():
    return torch.cuda.current_stream().cuda_stream


def prepared(case):
    """operands, the forward's lse, the pair's dctx and the float64 reference of one case: computed once, shared, never modified"""
    if case in _CACHE:
        return _CACHE[case]
    Lq, Lk, with_dist, mask_mode, rot = case
    c = ar.make_case(Lq, Lk, B, NH, True, mask_mode, with_dist, 0.125, 0.3, seed=5, rot=rot)
    q = ar.merge_heads(c["q"]).to(DEV).to(T).contiguous()
    kv = torch.cat([ar.merge_heads(c["k"]), ar.merge_heads(c["v"])], 1).to(DEV).to(T).contiguous()
    km = c["km"].to(DEV).contiguous()
    dist = c["dist"].to(DEV).contiguous() if with_dist else None
    w = torch.tensor([c["sp_w"]], device=DEV); b0 = torch.tensor([c["sp_b"]], device=DEV)
    ldS = (Lk + 7) // 8 * 8
    P = torch.empty(B, NH, Lq, ldS, device=DEV, dtype=T)
    ctx = torch.empty(B * Lq, H, device=DEV, dtype=T)
    d = AttnDesc()
    d.dtype, d.B, d.heads, d.Lq, d.Lk, d.ldS = _lib.ETP_BF16, B, NH, Lq, Lk, ldS
    d.Q, d.ldq, d.K, d.ldk, d.V, d.ldv = q.data_ptr(), H, kv.data_ptr(), 2 * H, kv.data_ptr() + 2 * H, 2 * H
    d.P, d.ctx, d.ldc = P.data_ptr(), ctx.data_ptr(), H
    d.keymask, d.mask_mode, d.alpha = km.data_ptr(), mask_mode, c["alpha"]
    if with_dist:
        d.dist, d.sp_w, d.sp_b = dist.data_ptr(), w.data_ptr(), b0.data_ptr()
    assert L().etp_attn_family(ctypes.byref(d)) == 2, "these shapes belong to the register-resident kernels"
    check(L().etp_attn_fwd(ctypes.byref(d), stream()), "attn_fwd")
    gen = torch.Generator().manual_seed(17 * Lq + Lk)
    dy = (torch.randn(B * Lq, H, generator=gen) * 0.5).to(DEV).to(T)
    Wo = (torch.randn(H, H, generator=gen) / math.sqrt(H)).to(DEV).to(T)           # [out][in], as nn.Linear stores it
    dctx = torch.empty(B * Lq, H, device=DEV, dtype=T)
    g = GemmDesc()
    g.A, g.B, g.C, g.M, g.N, g.K, g.lda, g.ldb, g.ldc = dy.data_ptr(), Wo.data_ptr(), dctx.data_ptr(), B * Lq, H, H, H, H, H
    g.trans_a, g.trans_b, g.dtype, g.c_dtype, g.batch, g.batch_inner, g.ksplit, g.alpha = 0, 1, _lib.ETP_BF16, _lib.ETP_BF16, 1, 1, 1, 1.0
    check(L().etp_gemm(ctypes.byref(g), stream()), "out-projection dgrad")
    torch.cuda.synchronize()
    # the GEMM's own tile against float64: one bf16 rounding of a sum whose terms are exact products
    exact = dy.double() @ Wo.double()
    bound = ar.U_BF16 * exact.abs() + ar.FP32_REL * (dy.double().abs() @ Wo.double().abs())
    ar.close(dctx, exact, bound, f"dctx {Lq}x{Lk}")
    c64 = dict(c)
    c64["dctx"] = ar.split_heads(dctx.float().cpu(), B, NH)
    val, E = ar.ref_of(c64, device=DEV)
    keep = (q, kv, km, dist, w, b0, P, ctx, dy, Wo, dctx)
    _CACHE[case] = dict(c=c, d=d, dy=dy, Wo=Wo, dctx=dctx, val=val, E=E, keep=keep, with_dist=with_dist)
    return _CACHE[case]


def backward(p, fused):
    """-> dict dQ / dK / dV [B, heads, L, 64] (+ d_sp_w, d_sp_b) of one backward on fresh NaN-filled outputs"""
    Lq, Lk = p["d"].Lq, p["d"].Lk
    bd = AttnBwdDesc()
    bd.f = p["d"]
    dP = torch.empty(B, NH, Lq, p["d"].ldS, device=DEV, dtype=T)
    dq = torch.full((B * Lq, H), float("nan"), device=DEV, dtype=T)
    dkv = torch.full((B * Lk, 2 * H), float("nan"), device=DEV, dtype=T)
    dwb = torch.zeros(2, device=DEV)
    bd.dctx, bd.ldd, bd.dP = (p["dy"] if fused else p["dctx"]).data_ptr(), H, dP.data_ptr()
    bd.dQ, bd.lddq, bd.dK, bd.lddk, bd.dV, bd.lddv = dq.data_ptr(), H, dkv.data_ptr(), 2 * H, dkv.data_ptr() + 2 * H, 2 * H
    if p["with_dist"]:
        bd.d_sp_w, bd.d_sp_b = dwb.data_ptr(), dwb.data_ptr() + 4
    if fused:
        check(L().etp_attn_bwd_proj(ctypes.byref(bd), p["Wo"].data_ptr(), H, stream()), "attn_bwd_proj")
    else:
        check(L().etp_attn_bwd(ctypes.byref(bd), stream()), "attn_bwd")
    torch.cuda.synchronize()
    out = {"dQ": ar.split_heads(dq, B, NH), "dK": ar.split_heads(dkv[:, :H], B, NH), "dV": ar.split_heads(dkv[:, H:], B, NH)}
    if p["with_dist"]:
        out["d_sp_w"], out["d_sp_b"] = dwb[0], dwb[1]
    return out


def held(got, p, name):
    for n in ("dV", "dQ", "dK"):
        worst = ar.close(got[n], p["val"][n], p["E"][n], f"{name} {n}", f"fold {name.split()[0]}/{n}")
        print(f"{name} {n}: worst |got - fp64| / bound {worst:.3f}")
    if p["with_dist"]:
        for n in ("d_sp_w", "d_sp_b"):
            worst = ar.close(got[n].reshape(()), p["val"][n], p["E"][n], f"{name} {n}", f"fold {name.split()[0]}/{n}")
            print(f"{name} {n}: worst |got - fp64| / bound {worst:.3f}")


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_fused_backward_against_the_pair_and_float64(case, etp_opt):
    etp_opt("ATTN_PROJ", 1)
    p = prepared(case)
    name = f"{case[0]}x{case[1]}"
    pair, fused = backward(p, False), backward(p, True)
    held(pair, p, f"pair {name}")
    held(fused, p, f"fused {name}")
    # fused against the pair: both inside the same bound around the same reference, so at most two bounds apart
    for n in ("dQ", "dK", "dV"):
        ar.close(fused[n], pair[n].double(), 2.0 * p["E"][n], f"fused against pair {name} {n}", f"fold fused-pair/{n}")


@pytest.mark.parametrize("case", [CASES[0], CASES[4]], ids=[IDS[0], IDS[4]])
def test_fused_backward_is_bit_identical_between_two_runs(case, etp_opt):
    etp_opt("ATTN_PROJ", 1)
    p = prepared(case)
    one, two = backward(p, True), backward(p, True)
    for n in ("dQ", "dK", "dV"):
        ar.same_bits(f"{case[0]}x{case[1]} {n} of a second run", two[n].contiguous(), one[n].contiguous())
