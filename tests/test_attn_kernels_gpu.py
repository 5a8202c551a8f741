"""Op-level tests of every attention kernel family against float64 with a derived bound (tests/attn_ref.py), through the C ABI
(etp_attn_fwd, then etp_attn_bwd on what it left):

  family (etp_attn_family)   selected by                                              dtypes / shapes
  2 register-resident        default                                                  bf16, both axes <= 128        attn_rows.hip
  3 streaming                default                                                  bf16, an axis > 128, no dist  attn.hip flash_*
  1 LDS-tile                 ATTN_ROWS=0 (+ ATTN_Q96=0 once for 64 < Lq, Lk <= 96)    bf16 <= 128, fp32 <= 64       attn.hip attn_*_kernel
  0 batched-GEMM             ATTN_ROWS=0 + ATTN_FUSED=0 (+ ATTN_FLASH=0 on long       both                          planner.hip + gemm
                             axes); under seed 1 WITHOUT switches where the dispatch
                             sends the shape there itself (fp32 beyond 64, bf16 with
                             dist beyond 128)

Every case asserts the family it meant to run (etp_attn_family evaluates the dispatch's own predicates), so a predicate that quietly
says no cannot turn four families into one.  The tests are ordered register-resident, streaming, LDS-tile, batched-GEMM.

Shapes: attn_ref.SHORT (30 pairs: every 16-row tile count and the 64 / 96 / 128 tile edges on both axes), attn_ref.LONG (8 pairs
around the 128-key tiles), two seeds.  Per case, cycling with the case index instead of multiplying the list (attn_ref.case_grid):
  * (B, heads) from (1, 12), (3, 4), (23, 12) -- 276 workgroups of the one-per-(batch, head) kernels;
  * mask_mode 0 under one seed, 1 under the other; alpha 0.125 or 0.2; the distance bias on / off, sp_w 0.3 or -1.7;
  * per batch entry one mask pattern of: all valid, only key 0, only the last key, key 0 invalid + random others, whole trailing tiles
    invalid, the whole LEADING tile invalid (the streaming forward's fully excluded prefix), every key invalid (mask_mode 0 only);
    or no mask pointer at all.  Under mask_mode 1 every row keeps a valid key (a row without one is outside the contract);
  * standard normal operands; in batch entry 0 a key equal to 3 x query 0 in the last tile, in the last batch entry a query scaled by 8;
  * layouts: packed; Q | K | V as column blocks of one [rows, 3H] buffer (Lq == Lk); K | V as halves of [rows, 2H]; ctx / dQ / dK / dV
    tight or inside wider buffers (leading dimension H + 64) -- always with 8 guard rows before and after; guard rows and extra columns
    hold a sentinel that must be bit-identical afterwards; outputs start as NaN, P and dP too.

Checks: every tensor against attn_ref within its elementwise bound (no multiplier); d_sp_w / d_sp_b start at a previous gradient a few
bounds large and must end at initial + reference; with only key 0 (or only the last key) valid under mask_mode 0, ctx equals that key's
V row bit for bit; forward and backward run twice and ctx, dQ, dK, dV are bit-identical between the runs.  d_sp_w / d_sp_b are exempt
from that: every workgroup adds its partial sum with one fp32 atomicAdd (attn_rows.hip rows_bwd_kernel `atomicAdd(a.d_sp_w, sw)`,
attn.hip attn_bwd_kernel `atomicAdd(a.d_sp_w, red[0] + ...)`, norm.hip softmax_bwd_kernel), so their last bits follow the order in
which workgroups retire.

etp_attn_fwd_qkv (QKV projection folded into the register-resident forward): its ctx is held to attn_ref of the Q / K / V stash it wrote
back, with the same bound.  Attention dropout: tests/test_drop_attn_gpu.py (etp_attn_*_drop); the kv_mod indirection:
tests/test_attn_kv_steps_gpu.py.

Worst |got - ref| / E observed on the MI355X (328 cases, 7 s; profiles/attn_op_bounds.txt has the whole table, the module prints it
after its last case under pytest -s): ctx 0.85 and dV 0.79 (register-resident and LDS-tile bf16), dQ 0.40, dK 0.37 (LDS-tile bf16);
streaming ctx 0.81; batched-GEMM bf16 0.57 (dV, long); fp32 families 0.48 (ctx); d_sp_w / d_sp_b 0.001.
"""
import ctypes
import math
import time

import pytest
import torch

pytestmark = pytest.mark.gpu

from etpnav_amd import _lib  # noqa: E402
from etpnav_amd._lib import AttnDesc, AttnBwdDesc, check  # noqa: E402
from tests import attn_ref as ar  # noqa: E402

DEV = "cuda"
SENTINEL = -777.0
GUARD = 8
T0 = [None]
COUNT = [0]


def L():
    return _lib.lib()


def stream():
    return torch.cuda.current_stream().cuda_stream


@pytest.fixture(scope="module", autouse=True)
def report_worst():
    T0[0] = time.time()
    yield
    cells = sorted({k.rsplit("/", 1)[0] for k in ar.WORST if not k.startswith("cpu-")})
    print(f"\nattention kernels, worst |got - fp64| / E per (family, dtype, tensor); {COUNT[0]} cases, {time.time() - T0[0]:.1f} s")
    for cell in cells:
        row = "  ".join(f"{n} {ar.WORST[f'{cell}/{n}'][0]:.3f}" for n in ar.NAMES if f"{cell}/{n}" in ar.WORST)
        print(f"  {cell:32s} {row}")


class Guarded:
    """[rows, H] output at leading dimension ld inside a buffer with GUARD rows before and after: the output region starts as NaN,
    everything else holds SENTINEL and must come back bit-identical."""

    def __init__(self, rows, H, ld, t):
        self.rows, self.H, self.ld = rows, H, ld
        self.buf = torch.full((rows + 2 * GUARD, ld), SENTINEL, device=DEV, dtype=t)
        self.buf[GUARD:GUARD + rows, :H] = float("nan")
        self.ptr = self.buf.data_ptr() + GUARD * ld * self.buf.element_size()

    def out(self):
        return self.buf[GUARD:GUARD + self.rows, :self.H]

    def check(self, name):
        got = self.buf.clone()
        got[GUARD:GUARD + self.rows, :self.H] = SENTINEL
        ar.same_bits(f"{name}: guard rows / extra columns", got, torch.full_like(got, SENTINEL))


def operands(c, layout, t):
    """-> (Q, ldq, K, ldk, V, ldv, keep-alive) device pointers of the case's stored operands in `layout`"""
    B, nh = c["B"], c["nh"]
    H = nh * 64
    qm, km, vm = (ar.merge_heads(c[n]).to(DEV).to(t) for n in ("q", "k", "v"))
    es = qm.element_size()
    if layout == "qkv3":
        buf = torch.cat([qm, km, vm], 1).contiguous()
        return buf.data_ptr(), 3 * H, buf.data_ptr() + H * es, 3 * H, buf.data_ptr() + 2 * H * es, 3 * H, (buf,)
    if layout == "kv2":
        kv = torch.cat([km, vm], 1).contiguous()
        qm = qm.contiguous()
        return qm.data_ptr(), H, kv.data_ptr(), 2 * H, kv.data_ptr() + H * es, 2 * H, (qm, kv)
    qm, km, vm = qm.contiguous(), km.contiguous(), vm.contiguous()
    return qm.data_ptr(), H, km.data_ptr(), H, vm.data_ptr(), H, (qm, km, vm)


def run_once(c, layout, wide, t, dtype, expect, d_init):
    """one forward + backward on fresh buffers -> dict of outputs ([B, heads, L, 64] views in dtype t), after the layout checks"""
    B, nh, Lq, Lk = c["B"], c["nh"], c["Lq"], c["Lk"]
    H = nh * 64
    ldo = H + 64 if wide else H
    ldS = (Lk + 7) // 8 * 8
    Q, ldq, K, ldk, V, ldv, keep = operands(c, layout, t)
    P = torch.full((B, nh, Lq, ldS), float("nan"), device=DEV, dtype=t)
    dP = torch.full_like(P, float("nan"))
    ctx, dq = Guarded(B * Lq, H, ldo, t), Guarded(B * Lq, H, ldo, t)
    dk, dv = Guarded(B * Lk, H, ldo, t), Guarded(B * Lk, H, ldo, t)
    km = None if c["km"] is None else c["km"].to(DEV).contiguous()
    dist = None if c["dist"] is None else c["dist"].to(DEV).contiguous()
    w = torch.tensor([c["sp_w"]], device=DEV, dtype=torch.float32)
    b0 = torch.tensor([c["sp_b"]], device=DEV, dtype=torch.float32)
    d = AttnDesc()
    d.dtype, d.B, d.heads, d.Lq, d.Lk, d.ldS = dtype, B, nh, Lq, Lk, ldS
    d.Q, d.ldq, d.K, d.ldk, d.V, d.ldv = Q, ldq, K, ldk, V, ldv
    d.P, d.ctx, d.ldc = P.data_ptr(), ctx.ptr, ldo
    d.keymask, d.mask_mode = (None if km is None else km.data_ptr()), c["mask_mode"]
    if dist is not None:
        d.dist, d.sp_w, d.sp_b = dist.data_ptr(), w.data_ptr(), b0.data_ptr()
    d.alpha = c["alpha"]
    fam = L().etp_attn_family(ctypes.byref(d))
    assert fam == expect, f"this case meant family {expect}, the dispatch takes family {fam}"
    check(L().etp_attn_fwd(ctypes.byref(d), stream()), "attn_fwd")
    torch.cuda.synchronize()
    dctx = ar.merge_heads(c["dctx"]).to(DEV).to(t).contiguous()
    bd = AttnBwdDesc()
    bd.f = d
    bd.dctx, bd.ldd, bd.dP = dctx.data_ptr(), H, dP.data_ptr()
    bd.dQ, bd.lddq, bd.dK, bd.lddk, bd.dV, bd.lddv = dq.ptr, ldo, dk.ptr, ldo, dv.ptr, ldo
    dwb = None
    if dist is not None:
        dwb = torch.tensor(d_init, device=DEV, dtype=torch.float32)
        bd.d_sp_w, bd.d_sp_b = dwb.data_ptr(), dwb.data_ptr() + 4
    assert L().etp_attn_family(ctypes.byref(bd.f)) == expect
    check(L().etp_attn_bwd(ctypes.byref(bd), stream()), "attn_bwd")
    torch.cuda.synchronize()
    del keep
    out = {}
    for n, g in (("ctx", ctx), ("dQ", dq), ("dK", dk), ("dV", dv)):
        g.check(n)
        out[n] = ar.split_heads(g.out(), B, nh)
    if dwb is not None:
        out["d_sp_w"], out["d_sp_b"] = dwb[0], dwb[1]
    return out


def run_case(x, bf16, expect, cell, etp_opt, opts, layouts=("packed", "qkv3", "kv2")):
    Lq, Lk, B, nh, mask_mode, with_dist, alpha, sp_w, seed, rot, null_mask = x
    for name, value in opts.items():
        etp_opt(name, value)
    dtype, t = (_lib.ETP_BF16, torch.bfloat16) if bf16 else (_lib.ETP_F32, torch.float32)
    c = ar.make_case(Lq, Lk, B, nh, bf16, mask_mode, with_dist, alpha, sp_w, seed, rot, null_mask)
    layout = layouts[rot % len(layouts)]
    if layout == "qkv3" and Lq != Lk:
        layout = "kv2"
    wide = (rot // 3) % 2 == 1
    val, E = ar.ref_of(c, gemm=(expect == 0), device=DEV)
    # the previous gradient the d_sp_w / d_sp_b buffers hold: random, a few bounds large (a store in place of the add must show)
    gen = torch.Generator().manual_seed(rot)
    r = torch.rand(2, generator=gen) + 2.0
    d_init = [float(r[0]) * float(E["d_sp_w"]), -float(r[1]) * float(E["d_sp_b"])] if with_dist else None
    got = run_once(c, layout, wide, t, dtype, expect, d_init)
    COUNT[0] += 1
    name = f"{cell} {Lq}x{Lk} B{B}x{nh} mode {mask_mode} {layout}{' wide' if wide else ''}"
    d_init32 = None if d_init is None else [float(torch.tensor(v, dtype=torch.float32)) for v in d_init]
    ar.check_all(got, val, E, name, cell, d_init32)
    if c["kinds"] is not None and mask_mode == 0:            # P is exactly 1 and 0: ctx is that key's V row
        for b, kind in enumerate(c["kinds"]):
            if kind in ("first", "last"):
                vrow = c["v"][b, :, 0 if kind == "first" else Lk - 1].to(DEV).to(t)            # [heads, 64]
                ar.same_bits(f"{name}: ctx of batch entry {b} (only the {kind} key valid)", got["ctx"][b].contiguous(),
                             vrow[:, None, :].expand(nh, Lq, 64).contiguous())
    again = run_once(c, layout, wide, t, dtype, expect, d_init)
    for n in ("ctx", "dQ", "dK", "dV"):
        ar.same_bits(f"{name}: {n} of a second run", again[n].contiguous(), got[n].contiguous())


def ids(g):
    return [f"{x[0]}x{x[1]}-B{x[2]}x{x[3]}-m{x[4]}-{'dist' if x[5] else 'nodist'}-a{x[6]}-s{x[8]}{'-nullmask' if x[10] else ''}" for x in g]


SHORT_G = ar.case_grid(ar.SHORT)
LONG_G = ar.case_grid(ar.LONG, dist_ok=False)
LONG_GD = ar.case_grid(ar.LONG)
F32_TILE_G = ar.case_grid(ar.SHORT_F32_TILE)
Q96_G = ar.case_grid(ar.SHORT_Q96)
ROWS_OFF = {"ATTN_ROWS": 0}
GEMM_ONLY = {"ATTN_ROWS": 0, "ATTN_FUSED": 0}


# ---- 2: register-resident ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("x", SHORT_G, ids=ids(SHORT_G))
def test_register_resident_bf16(x, etp_opt):
    run_case(x, True, 2, "register-resident bf16", etp_opt, {})


# ---- 3: streaming ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("x", LONG_G, ids=ids(LONG_G))
def test_streaming_bf16(x, etp_opt):
    run_case(x, True, 3, "streaming bf16", etp_opt, {})


# ---- 1: LDS-tile -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("x", SHORT_G, ids=ids(SHORT_G))
def test_lds_tile_bf16(x, etp_opt):
    run_case(x, True, 1, "LDS-tile bf16", etp_opt, ROWS_OFF)


@pytest.mark.parametrize("x", Q96_G, ids=ids(Q96_G))
def test_lds_tile_bf16_without_the_96_query_tile(x, etp_opt):
    run_case(x, True, 1, "LDS-tile bf16", etp_opt, {"ATTN_ROWS": 0, "ATTN_Q96": 0})


@pytest.mark.parametrize("x", F32_TILE_G, ids=ids(F32_TILE_G))
def test_lds_tile_fp32(x, etp_opt):
    run_case(x, False, 1, "LDS-tile fp32", etp_opt, {})


# ---- 0: batched-GEMM ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("x", SHORT_G, ids=ids(SHORT_G))
def test_batched_gemm_bf16_short(x, etp_opt):
    run_case(x, True, 0, "batched-GEMM bf16 short", etp_opt, GEMM_ONLY)


@pytest.mark.parametrize("x", LONG_GD, ids=ids(LONG_GD))
def test_batched_gemm_bf16_long(x, etp_opt):
    """with the distance bias the dispatch sends a long bf16 axis here itself: no switch under seed 1"""
    auto = x[5] and x[8] == 1
    run_case(x, True, 0, "batched-GEMM bf16 long dist" if x[5] else "batched-GEMM bf16 long", etp_opt,
             {} if auto else {**GEMM_ONLY, "ATTN_FLASH": 0})


@pytest.mark.parametrize("x", SHORT_G + LONG_GD, ids=ids(SHORT_G + LONG_GD))
def test_batched_gemm_fp32(x, etp_opt):
    """fp32 beyond 64 on either axis goes here by itself: no switch under seed 1"""
    auto = max(x[0], x[1]) > 64 and x[8] == 1
    run_case(x, False, 0, "batched-GEMM fp32", etp_opt, {} if auto else {**GEMM_ONLY, "ATTN_FLASH": 0})


# ---- the fused QKV projection's forward -------------------------------------------------------------------------------------
@pytest.mark.parametrize("with_dist", [False, True], ids=["nodist", "dist"])
@pytest.mark.parametrize("Lx,B", [(80, 3), (36, 23), (128, 3), (17, 1), (1, 3), (113, 3)])
def test_fused_qkv_forward_against_its_own_stash(Lx, B, with_dist):
    """etp_attn_fwd_qkv writes the Q / K / V stash and goes on with the attention: ctx must be attn_ref of THAT stash (the stash itself
    is compared with the GEMM in test_ops_gpu.py::test_self_attention_fwd_with_fused_qkv_projection)."""
    torch.manual_seed(100 + Lx)
    t, nh = torch.bfloat16, 12
    H = nh * 64
    ldS = (Lx + 7) // 8 * 8
    x = torch.randn(B * Lx, H, device=DEV).to(t)
    W = (torch.randn(3 * H, H, device=DEV) / math.sqrt(H)).to(t)
    bias = torch.randn(3 * H, device=DEV) * 0.1
    gen = torch.Generator().manual_seed(Lx)
    kinds = [ar.MASKS[(Lx + b) % 5] for b in range(B)]                  # all / first / last / not0 / tail
    km = torch.stack([ar.key_mask(kd, Lx, 0, 16, gen) for kd in kinds]).to(DEV)
    dist = torch.rand(B, Lx, Lx, device=DEV) * 3.0 if with_dist else None
    sp_w, sp_b = float(torch.tensor(-1.7, dtype=torch.float32)), float(torch.tensor(0.1, dtype=torch.float32))
    w = torch.tensor([sp_w], device=DEV); b0 = torch.tensor([sp_b], device=DEV)
    qkv = torch.full((B * Lx, 3 * H), float("nan"), device=DEV, dtype=t)
    P = torch.full((B, nh, Lx, ldS), float("nan"), device=DEV, dtype=t)
    ctx = Guarded(B * Lx, H, H + 64, t)
    d = AttnDesc()
    d.dtype, d.B, d.heads, d.Lq, d.Lk, d.ldS = _lib.ETP_BF16, B, nh, Lx, Lx, ldS
    d.Q, d.ldq = qkv.data_ptr(), 3 * H
    d.K, d.ldk = qkv.data_ptr() + 2 * H, 3 * H
    d.V, d.ldv = qkv.data_ptr() + 4 * H, 3 * H
    d.P, d.ctx, d.ldc = P.data_ptr(), ctx.ptr, H + 64
    d.keymask, d.mask_mode = km.data_ptr(), 0
    if with_dist:
        d.dist, d.sp_w, d.sp_b = dist.data_ptr(), w.data_ptr(), b0.data_ptr()
    d.alpha = 0.125
    assert L().etp_attn_family(ctypes.byref(d)) == 2
    check(L().etp_attn_fwd_qkv(ctypes.byref(d), x.data_ptr(), H, W.data_ptr(), H, bias.data_ptr(), stream()), "attn_fwd_qkv")
    torch.cuda.synchronize()
    assert bool(torch.isfinite(qkv).all()), "the stash keeps part of its NaN fill"
    ctx.check("ctx")
    q, k, v = (ar.split_heads(qkv[:, i * H:(i + 1) * H], B, nh) for i in range(3))
    val, E = ar.attn_ref(q, k, v, km, 0, dist, sp_w, sp_b, 0.125, torch.zeros_like(q))
    COUNT[0] += 1
    ar.close(ar.split_heads(ctx.out(), B, nh), val["ctx"], E["ctx"], f"fused QKV {Lx} B{B}", "register-resident bf16 fused QKV/ctx")
