"""fp64 restatements, launch geometry and ELEMENTWISE derived bounds for the kernels that reduce over rows or update state
(tests/test_reduce_kernels_gpu.py, tests/test_optim_kernels_gpu.py):

  norm.hip   ln_bwd_kernel (etp_ln_bwd), ln_bwd_s_kernel in its atomic and slab modes (etp_ln_stream_bwd,
             etp_ln_stream_bwd_stage1), ln_part_reduce_kernel (etp_ln_part_reduce), the typed ln_fwd_kernel (etp_ln_fwd)
  embed.hip  text_embed_fwd_kernel, text_embed_bwd_kernel, sap_ce_kernel, gather_sum_kernel, colsum_kernel, cast_f32_bf16_kernel, cast_bf16_f32_kernel, scale_f32_kernel
  optim.hip  adamw_kernel, adamw_bump_kernel, sqnorm_kernel

tests/test_reduce_ref_cpu.py pins every restatement to the code it restates (fp64, 1e-12); tests/test_reduce_bounds_cpu.py shows
that fp32 emulations of the kernels' schedules stay inside the bounds and that the listed mutations are rejected.

Bounds.  u = 2^-24 (fp32 unit roundoff), gam(k) = k u / (1 - k u).  Every reduction is held, per output element, to

    gam(d + e) * sum_i |t_i|  (+ the input-rounding terms below)

where t_i are the fp64 terms of that element (the "previous gradient" an accumulating kernel adds onto is one of them), e the number
of roundings a single term carries before it enters the sum, and d the LONGEST CHAIN OF ADDITIONS a term can pass through under the
launch geometry.  d is computed, never fitted:

  LayerNorm backward, dgamma / dbeta (ln_depth).  A wavefront owns rows blk*4 + wave + k*4*blocks: R = ceil(M / (4 blocks)) adds
    into its register accumulator; 3 adds combine the four waves (((w0 + w1) + w2) + w3); then either
      atomic mode   `blocks` atomics per column onto the previous gradient (any order: every add counts), or
      slab mode     ln_part_reduce: chunks of LN_PART_CHUNK = 32 slabs, four accumulators (c // 4 + c % 4 adds for a chunk of c
                    slabs, the longer of a full chunk and the last one), 2 adds for (a0 + a1) + (a2 + a3), and one atomic per chunk.
    blocks: etp_ln_bwd min(ceil(M / 8), 128); etp_ln_stream_bwd min(ceil(M / 4), 128); stage 1 ln_stage_blocks (at most 1024 or
    the LNBWD_GRID switch, the same number of rows for every wave).  M = 8192, H = 768, default switch: 2 + 3 + 8 + 2 + 32 = 47.
    A term of dgamma is dy * xhat with xhat = (x - mean~) * rstd~ from the fp32 `stats` the kernel is handed (each within u of the
    fp64 value): |d xhat| <= 3u |xhat| + u |mean| rstd, one more rounding for the product: e = 4 and an extra
    u * sum_i |dy_i| |mean_i| rstd_i.  dbeta's terms are the inputs themselves: e = 0.
  LayerNorm backward, dx (ln_dx_bound).  The two row means run 4*NCH lane-sequential adds and the 6 levels of the wave butterfly
    (D = 4 NCH + 6); the bound propagates the errors of gy, xhat, s1, s2 through rstd * (gy - s1 - xhat * s2) (+ add) term by term.
  colsum.  <= 16 rows per wave of a 64-row block, 3 adds for the waves, ceil(M / 64) atomics per column: d = 16 + 3 + ceil(M / 64).
  gather_sum.  out (+)= sum_j w_j src[idx_j]: one chain over the segment, d = len (+ 1 accumulating), e = 1 (the product).
  cross-entropy (ce_bounds).  expf / logf within one ulp (2u relative), the row sum ceil(G / 64) + 6 deep, the loss
    ceil(B / 16) + 16 deep (16 waves, then a sequential sum of the 16 partials).
  sumsq (sumsq_bound).  Per thread ceil(n / 4 / (256 grid)) iterations of ((a + b) + c) + d then + s; 6 butterfly levels; 3 adds for
    the waves; then `grid` atomics.  All terms are >= 0, so the atomic chain is bounded by u times the sum of its running sums
    in the WORST order (largest partial first) instead of grid * u * total.
  AdamW (adamw_bounds).  Restarted from the kernel's own p, m, v at every step; per element, in |p_old|, |p_new| and |update|,
    with the fp32 bias corrections of the counted entry point as their own term (powf within one ulp: 2u beta^t / (1 - beta^t)).

Where the kernel stores bf16 the bound grows by one bf16 ulp of the fp64 value.  No multiplier is fitted to what a kernel returns,
and no element is left out of a comparison.  Comparators record their worst err / bound in WORST[(kernel, tensor)].

Sentinel rows (ln_case / colsum_case): the last row, the first row of a second grid-stride sweep and a row of the last slab are
built so that each of their terms exceeds 8x the bound of its column (assert_sentinels, on the fp64 terms alone): dropping one of
them cannot hide inside any column's bound.
"""
import math

import torch

from oracle import planner_oracle as po
from tests.row_ref import ulp_bf16

F64 = torch.float64
U = 2.0 ** -24
LN_BWD_MAX_BLOCKS = 1024      # kernels.h
LN_PART_CHUNK = 32            # norm.hip
LN_ATOMIC_BLOCKS = 128        # norm.hip: ln_bwd_t, ln_bwd_s without slabs
WORST = {}


def gam(k):
    return k * U / (1.0 - k * U)


def _record(key, ratio):
    if ratio > WORST.get(key, 0.0):
        WORST[key] = ratio


def within(key, got, ref, bound):
    """every element of `got` finite (where ref is) and |got - ref| <= bound, elementwise; records max err / bound."""
    got, ref, bound = got.detach().to(F64), ref.detach().to(F64), bound.detach().to(F64)
    assert got.shape == ref.shape == bound.shape, (key, tuple(got.shape), tuple(ref.shape), tuple(bound.shape))
    assert bool(torch.isfinite(ref).all()) and bool(torch.isfinite(bound).all()), f"{key}: reference / bound not finite"
    assert bool(torch.isfinite(got).all()), f"{key}: {int((~torch.isfinite(got)).sum())} non-finite elements"
    err = (got - ref).abs()
    ratio = torch.where(bound > 0, err / bound.clamp_min(1e-300), torch.where(err > 0, torch.full_like(err, float("inf")), torch.zeros_like(err)))
    worst = float(ratio.max()) if ratio.numel() else 0.0
    _record(key, worst)
    assert worst <= 1.0, f"{key}: {int((ratio > 1).sum())} of {ratio.numel()} elements beyond their bound, worst err / bound {worst:.3g}"
    return worst


def same_bits(key, got, want):
    assert got.dtype == want.dtype and got.shape == want.shape, (key, got.dtype, want.dtype, tuple(got.shape), tuple(want.shape))
    iv = {torch.float32: torch.int32, torch.bfloat16: torch.int16, torch.float64: torch.int64, torch.uint8: torch.uint8,
          torch.int32: torch.int32}[got.dtype]
    diff = got.contiguous().view(iv) != want.contiguous().view(iv)
    assert not bool(diff.any()), f"{key}: {int(diff.sum())} elements differ bitwise"


NOTES = {}         # figures recorded for the report only, never asserted and never part of WORST


def note(key, value):
    if value > NOTES.get(key, 0.0):
        NOTES[key] = value


def worst_table():
    rows = [f"  {k[0]:<48}{k[1]:<20}{v:8.3f}" for k, v in sorted(WORST.items())]
    return "\n".join([f"  {'entry point':<48}{'tensor':<20}err/bound"] + rows)


# ---- bf16 round-to-nearest-even ------------------------------------------------------------------------------------------------
def bf16_rne_bits(x):
    """fp32 tensor -> int16 bit patterns of its round-to-nearest-even bf16 (NaN -> a quiet NaN of the same sign)."""
    i = x.contiguous().view(torch.int32).to(torch.int64) & 0xFFFFFFFF
    rounded = (i + 0x7FFF + ((i >> 16) & 1)) >> 16
    nan = (i & 0x7FFFFFFF) > 0x7F800000
    out = torch.where(nan, (i >> 16) | 0x40, rounded) & 0xFFFF
    return torch.where(out >= 0x8000, out - 0x10000, out).to(torch.int16)


def bf16_rne(x):
    return bf16_rne_bits(x).view(torch.bfloat16)


def check_cast(key, got_bf16, src):
    """bit for bit, except that any NaN pattern is accepted for a NaN source"""
    want = bf16_rne_bits(src)
    got = got_bf16.contiguous().view(torch.int16)
    nan = torch.isnan(src)
    assert bool(torch.isnan(got_bf16[nan].float()).all()), f"{key}: a NaN did not stay NaN"
    diff = (got != want) & ~nan
    assert not bool(diff.any()), f"{key}: {int(diff.sum())} elements are not the round-to-nearest-even bf16"


def cast_specials(device="cpu"):
    """fp32 values whose bf16 rounding goes wrong first: signed zeros, infinities, NaN, denormals, ties to even in both directions,
    just above / below a tie, the largest finite value (rounds to inf)."""
    bits = [0x00000000, 0x80000000, 0x7F800000, 0xFF800000, 0x7FC00000, 0x7F800001, 0xFFC12345, 0x00000001, 0x80000001, 0x007FFFFF,
            0x00008000, 0x00018000, 0x3F808000, 0x3F818000, 0x3F808001, 0x3F807FFF, 0xBF808000, 0xBF818000, 0x7F7FFFFF, 0xFF7FFFFF,
            0x7F7F8000, 0x7F7F7FFF, 0x3F7FFFFF, 0x3F7F8000]
    t = torch.tensor([b - (1 << 32) if b >= (1 << 31) else b for b in bits], dtype=torch.int64).to(torch.int32)
    return t.view(torch.float32).to(device)


# ---- LayerNorm backward --------------------------------------------------------------------------------------------------------
def cdiv(a, b):
    return (a + b - 1) // b


def ln_typed_blocks(M):
    return min(cdiv(M, 8), LN_ATOMIC_BLOCKS)


def ln_atomic_blocks(M):
    return min(cdiv(M, 4), LN_ATOMIC_BLOCKS)


def ln_stage_blocks(M, cap=None):
    """norm.hip ln_bwd_blocks: the switch LNBWD_GRID is clamped to [1, 1024]; every wave gets the same number of rows."""
    groups = cdiv(M, 4)
    cap = min(LN_BWD_MAX_BLOCKS, max(1, LN_BWD_MAX_BLOCKS if cap is None else int(cap)))
    rounds = cdiv(groups, cap)
    return cdiv(groups, rounds)


def ln_part_bytes(M, H, cap=None):
    return 2 * H * 4 * ln_stage_blocks(M, cap)


def ln_depth(M, blocks, slabs):
    R = cdiv(M, 4 * blocks)
    if not slabs:
        return R + 3 + blocks
    chunks = cdiv(blocks, LN_PART_CHUNK)
    last = blocks - (chunks - 1) * LN_PART_CHUNK
    full = LN_PART_CHUNK // 4 if blocks >= LN_PART_CHUNK else 0
    return R + 3 + max(full, last // 4 + last % 4) + 2 + chunks


def ln_stats(x, eps):
    mu = x.mean(-1, keepdim=True)
    var = ((x - mu) * (x - mu)).mean(-1, keepdim=True)
    return torch.cat([mu, 1.0 / torch.sqrt(var + eps)], -1)


def ln_bwd(dy, x, gamma, eps, add=None):
    """-> dx (+ add), dgamma, dbeta of y = layer_norm(x) * gamma + beta, through autograd of the oracle's own layer_norm."""
    x_ = x.detach().to(F64).requires_grad_(True)
    g_ = gamma.detach().to(F64).requires_grad_(True)
    b_ = torch.zeros_like(g_).requires_grad_(True)
    po.layer_norm(x_, g_, b_, eps).backward(dy.detach().to(F64))
    dx = x_.grad if add is None else x_.grad + add.detach().to(F64)
    return dx, g_.grad, b_.grad


def ln_terms(dy, x, gamma, eps):
    dy, x, gamma = dy.to(F64), x.to(F64), gamma.to(F64)
    st = ln_stats(x, eps)
    mean, rstd = st[:, :1], st[:, 1:]
    return {"dy": dy, "xh": (x - mean) * rstd, "gy": dy * gamma, "mean": mean, "rstd": rstd}


def ln_param_bounds(t, init_g, init_b, d):
    """per-column bounds of dgamma, dbeta (module docstring)"""
    tg = (t["dy"] * t["xh"]).abs().sum(0) + init_g.to(F64).abs()
    bg = gam(d + 4) * tg + 1.0001 * U * (t["dy"].abs() * t["mean"].abs() * t["rstd"]).sum(0)
    bb = gam(d) * (t["dy"].abs().sum(0) + init_b.to(F64).abs())
    return bg, bb


def ln_dx_bound(t, dx_ref, add, H, bf16_out, e_x=None):
    """e_x: elementwise error the kernel's own x already carries (the text embedding forms x = (word + pos) + type in fp32)"""
    D = 4 * (H // 256) + 6
    gy, xh, rstd = t["gy"], t["xh"], t["rstd"]
    e_xh = 3 * U * xh.abs() + U * t["mean"].abs() * rstd + (0 if e_x is None else rstd * e_x)
    s1, s2 = gy.mean(-1, keepdim=True), (gy * xh).mean(-1, keepdim=True)
    e_s1 = gam(D + 3) * gy.abs().mean(-1, keepdim=True)
    e_s2 = gam(D + 5) * (gy * xh).abs().mean(-1, keepdim=True) + (gy.abs() * e_xh).mean(-1, keepdim=True)
    mag = gy.abs() + s1.abs() + (xh * s2).abs()
    inner = U * gy.abs() + e_s1 + xh.abs() * e_s2 + s2.abs() * e_xh + 3 * U * mag
    b = rstd * inner + 2 * U * rstd * mag
    if add is not None:
        b = b + U * (dx_ref.abs() + add.to(F64).abs())
    if bf16_out:
        b = b + ulp_bf16(dx_ref)
    return b


def sentinel_rows(M, blocks):
    """last row, first row of the second grid-stride sweep, first row of the last block (= last slab)"""
    rows = {M - 1}
    if 4 * blocks < M:
        rows.add(4 * blocks)
    if 4 * (blocks - 1) < M:
        rows.add(4 * (blocks - 1))
    return sorted(rows)


def assert_sentinels(what, terms, bound, rows):
    for r in rows:
        short = terms[r].abs() <= 8 * bound
        assert not bool(short.any()), f"{what}: row {r} has {int(short.sum())} terms within 8x their column's bound"


def ln_case(M, H, eps, blocks, slabs, seed, dtype=torch.float32, device="cpu", with_add=True):
    """One LayerNorm-backward case: rows scaled 2^-10 .. 2^3, an all-zero row, a row with |mean| / std ~ 1e3 and the sentinel rows,
    values rounded to `dtype` (the operand dtype of etp_ln_bwd; fp32 for the stream kernels).  -> dict of fp32 / `dtype` inputs, the
    fp64 reference, the per-element bounds for this geometry and the sentinel rows (asserted here, on the reference alone)."""
    g = torch.Generator().manual_seed(seed)
    scale = 2.0 ** torch.randint(-10, 4, (M, 1), generator=g).double()
    x = (torch.randn(M, H, generator=g, dtype=F64) * 1.5 + torch.randn(M, 1, generator=g, dtype=F64)) * scale
    dy = torch.randn(M, H, generator=g, dtype=F64) * 2.0 ** torch.randint(-10, 4, (M, 1), generator=g).double()
    sent = sentinel_rows(M, blocks)
    free = [r for r in range(M) if r not in sent]
    if len(free) >= 1:
        x[free[len(free) // 2]] = 0.0                                    # all-zero row: rstd = eps^-1/2
    if len(free) >= 2:
        r = free[len(free) // 3]
        x[r] = 1000.0 + torch.randn(H, generator=g, dtype=F64)           # |mean| / std ~ 1e3
    for r in sent:                                                        # |xhat| ~ 1, |dy| in [4, 8]: every term of the row is O(4)
        sign = torch.where(torch.rand(H, generator=g) < 0.5, -1.0, 1.0).double()
        x[r] = sign * (1.0 + 0.25 * torch.rand(H, generator=g, dtype=F64))
        dy[r] = torch.where(torch.rand(H, generator=g) < 0.5, -1.0, 1.0).double() * (4.0 + 4.0 * torch.rand(H, generator=g, dtype=F64))
    gamma = 1.0 + 0.3 * torch.randn(H, generator=g, dtype=F64)
    add = torch.randn(M, H, generator=g, dtype=F64) if with_add else None
    init_g, init_b = torch.randn(H, generator=g), torch.randn(H, generator=g)
    x, dy = x.to(dtype), dy.to(dtype)
    add = None if add is None else add.to(dtype)
    gamma = gamma.float()
    c = {"M": M, "H": H, "eps": eps, "x": x, "dy": dy, "gamma": gamma, "add": add, "init_g": init_g, "init_b": init_b, "sent": sent}
    c = {k: (v.to(device) if torch.is_tensor(v) else v) for k, v in c.items()}
    c["stats"] = ln_stats(c["x"].to(F64), eps).float()                    # what an exact forward would hand over, rounded to fp32
    for _ in range(3):
        # a long chain (one block sweeping thousands of rows) has a bound above an O(4) term: scale the sentinel rows' dy by the power
        # of two that lifts every term of theirs to 16x its column's bound (8x is asserted; their own share of the bound is d * u of them)
        t = ln_terms(c["dy"], c["x"], c["gamma"], eps)
        bg, bb = ln_param_bounds(t, c["init_g"], c["init_b"], ln_depth(M, blocks, slabs))
        need = max(float((16 * bg / (t["dy"] * t["xh"])[sent].abs()).max()), float((16 * bb / t["dy"][sent].abs()).max()))
        if need <= 1.0:
            break
        c["dy"][sent] = c["dy"][sent] * 2.0 ** math.ceil(math.log2(need))
    ln_case_reference(c, blocks, slabs)
    return c


def ln_case_reference(c, blocks, slabs):
    """(re)compute reference and bounds of a case for one launch geometry"""
    if "t" not in c:
        c["t"] = ln_terms(c["dy"], c["x"], c["gamma"], c["eps"])
        c["dx0"], c["dgamma"], c["dbeta"] = ln_bwd(c["dy"], c["x"], c["gamma"], c["eps"])
    d = ln_depth(c["M"], blocks, slabs)
    c["depth"] = d
    c["bg"], c["bb"] = ln_param_bounds(c["t"], c["init_g"], c["init_b"], d)
    c["sent"] = sentinel_rows(c["M"], blocks)
    assert_sentinels("dgamma", c["t"]["dy"] * c["t"]["xh"], c["bg"], c["sent"])
    assert_sentinels("dbeta", c["t"]["dy"], c["bb"], c["sent"])
    return c


def check_ln_bwd(name, c, dx, dx_lp, dgamma, dbeta, add):
    """dx / dx_lp / dgamma may be None (not passed).  dgamma / dbeta are what the buffers hold after the call (init + gradient)."""
    ref = c["dx0"] if add is None else c["dx0"] + add.to(F64)
    if dx is not None:
        within((name, "dx"), dx, ref, ln_dx_bound(c["t"], ref, add, c["H"], dx.dtype == torch.bfloat16))
    if dx_lp is not None:
        if dx is not None:
            same_bits(f"{name} dx_lp (round-to-nearest-even copy of dx)", dx_lp, dx.to(dx_lp.dtype))
        else:
            within((name, "dx_lp"), dx_lp, ref, ln_dx_bound(c["t"], ref, add, c["H"], dx_lp.dtype == torch.bfloat16))
    if dgamma is not None:
        within((name, "dgamma"), dgamma, c["init_g"].to(F64) + c["dgamma"], c["bg"])
        within((name, "dbeta"), dbeta, c["init_b"].to(F64) + c["dbeta"], c["bb"])


def _wave_sum32(v):
    """v [M, 64] fp32: the xor butterfly of wave_sum (every lane ends with the same value; lane 0 returned)"""
    idx = torch.arange(64, device=v.device)
    for o in (32, 16, 8, 4, 2, 1):
        v = v + v[:, idx ^ o]
    return v[:, :1]


def _row_sum32(a):
    """a [M, H] fp32 -> [M, 1]: lane-sequential over (chunk, element), then the butterfly"""
    M, H = a.shape
    a = a.reshape(M, H // 256, 64, 4)
    s = torch.zeros(M, 64, dtype=torch.float32, device=a.device)
    for ch in range(H // 256):
        for e in range(4):
            s = s + a[:, ch, :, e]
    return _wave_sum32(s)


def emulate_ln_bwd(c, blocks, slabs, add, out_dtype=torch.float32):
    """fp32 emulation of ln_bwd_kernel / ln_bwd_s_kernel (+ ln_part_reduce_kernel) in the kernel's operation order; the atomics of
    a column are applied in reverse block order onto the previous gradient (one of the orders the hardware may take)."""
    f = torch.float32
    M, H = c["M"], c["H"]
    x, dy, gamma, st = c["x"].to(f), c["dy"].to(f), c["gamma"].to(f), c["stats"]
    mean, rstd = st[:, :1], st[:, 1:]
    xh = (x - mean) * rstd
    gy = dy * gamma
    s1 = _row_sum32(gy) * f32(1.0 / H)
    s2 = _row_sum32(gy * xh) * f32(1.0 / H)
    dx = rstd * (gy - s1 - xh * s2)
    if add is not None:
        dx = dx + add.to(f)
    dx = dx.to(out_dtype)
    R = cdiv(M, 4 * blocks)
    pad = R * blocks * 4 - M

    def colsum(t):
        t = torch.cat([t, torch.zeros(pad, H, dtype=f)], 0).reshape(R, blocks, 4, H)
        acc = torch.zeros(blocks, 4, H, dtype=f)
        for k in range(R):
            acc = acc + t[k]
        return ((acc[:, 0] + acc[:, 1]) + acc[:, 2]) + acc[:, 3]              # [blocks, H]

    out = []
    for part, init in ((colsum(dy * xh), c["init_g"]), (colsum(dy), c["init_b"])):
        if slabs:
            vals = []
            for b0 in range(0, blocks, LN_PART_CHUNK):
                b1 = min(blocks, b0 + LN_PART_CHUNK)
                a = [torch.zeros(H, dtype=f) for _ in range(4)]
                b = b0
                while b + 4 <= b1:
                    for j in range(4):
                        a[j] = a[j] + part[b + j]
                    b += 4
                while b < b1:
                    a[0] = a[0] + part[b]
                    b += 1
                vals.append((a[0] + a[1]) + (a[2] + a[3]))
            part = torch.stack(vals)
        acc = init.to(f).clone()
        for b in reversed(range(part.shape[0])):
            acc = acc + part[b]
        out.append(acc)
    return dx, out[0], out[1]


def f32(v):
    return float(torch.tensor(v, dtype=torch.float32))


# the GPU matrix of the LayerNorm kernels (tests/test_reduce_kernels_gpu.py builds its cases from these lists and from nothing else;
# tests/test_reduce_bounds_cpu.py emulates every one of them)
LN_H = (256, 512, 768, 1024)
LN_EPS = (1e-12, 1e-5)
LN_TYPED_M = (1, 5, 77, 513, 1029)            # 513: one row past one sweep of 64 blocks; 1029: past the 128-block cap's 1024 rows
LN_FWD_ONLY_M = (16389,)                      # one row past the forward's 16384-row trip
LN_ATOMIC_M = (1, 3, 4, 5, 511, 513, 2053)    # 513: second sweep of the 128-block atomic path; 2053: fifth
LN_STAGE_M = (1, 4, 5, 124, 128, 132, 4096, 4097, 8192)   # 31 / 32 / 33 slabs; the 1024-block cap, one row past it (513 blocks), 2 sweeps
LN_GRIDS = (None, 1, 3, 2048)                 # the LNBWD_GRID switch (2048 is clamped to 1024)


def ln_typed_cases():
    """(dtype name, H, M, eps, add?, dgamma / dbeta?)"""
    out, i = [], 0
    for H in LN_H:
        for M in LN_TYPED_M:
            for dt in ("fp32", "bf16"):
                out.append((dt, H, M, LN_EPS[i % 2], i % 3 != 0, i % 4 != 1))
                i += 1
    return out


def ln_atomic_cases():
    """(dtype name of dx_lp, H, M, eps, outputs in {'dx', 'lp', 'both'}, add?, dgamma / dbeta?)"""
    out, i = [], 0
    for H in LN_H:
        for M in LN_ATOMIC_M:
            out.append((("fp32", "bf16")[i % 2], H, M, LN_EPS[(i // 2) % 2], ("both", "dx", "lp")[i % 3], i % 4 != 2, i % 5 != 3))
            i += 1
    return out


def ln_stage_cases():
    """(dtype name of dx_lp, H, M, eps, LNBWD_GRID or None, outputs, add?)"""
    out, i = [], 0
    for M in LN_STAGE_M:
        for H in LN_H:
            out.append((("bf16", "fp32")[i % 2], H, M, LN_EPS[(i // 2) % 2], None, ("both", "dx", "lp")[i % 3], i % 4 != 2))
            i += 1
        for j, grid in enumerate(LN_GRIDS[1:]):
            out.append((("bf16", "fp32")[i % 2], LN_H[(i + j) % 4], M, LN_EPS[(i // 2) % 2], grid, ("both", "dx", "lp")[i % 3], i % 4 != 2))
            i += 1
    return out


# ---- LayerNorm forward (typed) -------------------------------------------------------------------------------------------------
def ln_fwd(x, gamma, beta, eps):
    x = x.to(F64)
    return po.layer_norm(x, gamma.to(F64), beta.to(F64), eps), ln_stats(x, eps)


def ln_fwd_bounds(x, gamma, beta, eps, ref_y, ref_st, bf16_out, e_x=None):
    """y = xc * rstd * gamma + beta with xc = x - mean~; mean~ carries D + 1 roundings of mean|x|, the variance D + 3 of itself
    (plus 2 |xc| d mean), rstd half of the variance's relative error plus rsqrtf's one ulp."""
    x = x.to(F64)
    H = x.shape[-1]
    D = 4 * (H // 256) + 6
    mean, rstd = ref_st[:, :1], ref_st[:, 1:]
    e_in = torch.zeros_like(x) if e_x is None else e_x
    e_mean = gam(D + 2) * x.abs().mean(-1, keepdim=True) + e_in.mean(-1, keepdim=True)
    xc = x - mean
    var = (xc * xc).mean(-1, keepdim=True)
    e_xc = e_mean + e_in + U * xc.abs()
    e_var = gam(D + 4) * var + 2 * (xc.abs() * e_xc).mean(-1, keepdim=True) + (e_xc * e_xc).mean(-1, keepdim=True) + U * (var + eps)
    e_rstd = rstd * (0.5 * e_var / (var + eps) + 3 * U)
    g = gamma.to(F64).abs()
    by = e_xc * rstd * g + xc.abs() * e_rstd * g + 3 * U * (xc * rstd).abs() * g + U * ref_y.abs() + U * beta.to(F64).abs()
    if bf16_out:
        by = by + ulp_bf16(ref_y)
    return by, torch.cat([e_mean, e_rstd], -1)


# ---- text embedding ------------------------------------------------------------------------------------------------------------
TEXT_H = (256, 512, 768)
TEXT_SHAPES = ((1, 7), (3, 9), (5, 24), (32, 80), (2, 1030))     # B < 4 (idle waves) twice; B % 4 != 0; ordinary; L past the 1024-block grid
TEXT_FWD_ONLY = ((17, 965),)                                     # 16405 rows: past the forward's 16384-row trip
TEXT_IDS = ("random", "one", "padding", "last", "edges")
TEXT_VOCAB = 211


def text_blocks(L):
    return min(L, 1024)


def text_ids(kind, B, L, g):
    if kind == "one":                       # one id everywhere: the most same-address atomics a word row can see
        return torch.full((B, L), 5, dtype=torch.int64)
    if kind == "padding":
        return torch.zeros(B, L, dtype=torch.int64)
    ids = torch.randint(1, min(TEXT_VOCAB - 1, 40), (B, L), generator=g)          # repeats; rows 40.. are named by nothing
    if kind == "last":
        ids[:, L // 2] = TEXT_VOCAB - 1
    if kind == "edges":
        ids[:, 0] = 0
        ids[:, -1] = 0
    return ids


def text_fwd(ids, word, pos, type0, gamma, beta, eps):
    """LN(word[id] + pos[l] + type[0]) -> y [B, L, H], stats [B, L, 2], and the un-normalised sum"""
    L = ids.shape[1]
    e = torch.nn.functional.embedding(ids, word, padding_idx=0) + pos[:L][None] + type0[None, None]
    return po.layer_norm(e, gamma, beta, eps), ln_stats(e, eps), e


def text_bwd(dy, ids, word, pos, type0, gamma, beta, eps):
    """-> dict of the five parameter gradients + dword (row 0, the padding row, gets none) and dx, the gradient of the sum"""
    q = [t.detach().to(F64).requires_grad_(True) for t in (word, pos, type0, gamma, beta)]
    y, _, e = text_fwd(ids, *q, eps)
    e.retain_grad()
    y.backward(dy.to(F64))
    out = dict(zip(("dword", "dpos", "dtype0", "dgamma", "dbeta"), (t.grad for t in q)))
    out["dx"] = e.grad
    return out


def text_case(B, L, H, kind, eps, seed, device="cpu"):
    g = torch.Generator().manual_seed(seed)
    ids = text_ids(kind, B, L, g)
    c = {"B": B, "L": L, "H": H, "eps": eps, "ids": ids,
         "word": torch.randn(TEXT_VOCAB, H, generator=g), "pos": torch.randn(L + 3, H, generator=g) * 0.5,
         "type0": torch.randn(H, generator=g) * 0.5, "gamma": 1.0 + 0.3 * torch.randn(H, generator=g),
         "beta": 0.5 * torch.randn(H, generator=g), "dy": torch.randn(B, L, H, generator=g)}
    for k, shape in (("dword", (TEXT_VOCAB, H)), ("dpos", (L + 3, H)), ("dtype0", (H,)), ("dgamma", (H,)), ("dbeta", (H,))):
        c["init_" + k] = torch.randn(*shape, generator=g)
    # sentinel rows (b, l): the last row, a row of the last workgroup (position 1023) and, past the 1024-block grid, the first row of the
    # second sweep (position 1024).  The id pattern stays as it is: pos[l] is set so that word[id] + pos[l] + type0 = +-(1 .. 1.25) (|xhat| ~ 1 in every
    # column), and dy so that dy * gamma = +-(4 .. 8) with zero row means: every term of dgamma (dy xhat), dbeta (dy) and dtype0 (dx) is O(4).
    # text_reference scales their dy by a power of two where a long chain needs more, and asserts the 8x condition.
    c["gamma"] = torch.where(c["gamma"].abs() < 0.25, torch.full_like(c["gamma"], 0.25), c["gamma"])
    grid = text_blocks(L)
    # (distinct positions: pos[l] is shared by the batch.  Up to 1024 positions the last workgroup's rows ARE position L - 1; the first
    # workgroup's first row stands in as the second sentinel)
    sent = sorted({(B - 1, L - 1), (0, grid - 1 if L > 1024 else 0)} | ({(0, 1024)} if L > 1024 else set()))
    for (b, l) in sent:
        # columns in pairs (2k, 2k + 1): the same x, opposite dy * gamma -- mean(gy) = mean(gy xhat) = 0, so dx = rstd * gy in every column
        sign = torch.where(torch.rand(H // 2, generator=g) < 0.5, -1.0, 1.0)
        target = (sign * (1.0 + 0.25 * torch.rand(H // 2, generator=g))).repeat_interleave(2)
        c["pos"][l] = target - c["word"][ids[b, l]] - c["type0"]
        v = 4.0 + 4.0 * torch.rand(H // 2, generator=g)
        c["dy"][b, l] = torch.stack([v, -v], 1).reshape(H) / c["gamma"]
    c["sent"] = [b * L + l for (b, l) in sent]
    return {k: (v.to(device) if torch.is_tensor(v) else v) for k, v in c.items()}


def text_reference(c, backward=True):
    """fp64 reference and bounds of one case.  Chain depths of the backward (text_embed_bwd_kernel: one workgroup per position l, stride
    min(L, 1024); its four waves split the batch):
      dgamma, dbeta   ceil(L / grid) * ceil(B / 4) adds per wave, 3 for the waves, `grid` atomics
      dpos[l]         ceil(B / 4) + 3 + 1 (one atomic onto the previous gradient)
      dtype0          ceil(B / 4) + ceil(L / grid) + 3 + grid
      dword[id]       one atomic per occurrence of id, in any order: count(id)
    every term of dpos / dtype0 / dword is a dx element and brings that element's own bound (ln_dx_bound) with it."""
    B, L, H, eps = c["B"], c["L"], c["H"], c["eps"]
    w64, p64, t64 = c["word"].to(F64), c["pos"].to(F64), c["type0"].to(F64)
    y, st, e = text_fwd(c["ids"], w64, p64, t64, c["gamma"].to(F64), c["beta"].to(F64), eps)
    wp = w64[c["ids"]] + p64[:L][None]
    e_x = U * wp.abs() + U * e.abs()                                            # (word + pos) + type: two roundings
    M = B * L
    by, bst = ln_fwd_bounds(e.reshape(M, H), c["gamma"], c["beta"], eps, y.reshape(M, H), st.reshape(M, 2), False, e_x.reshape(M, H))
    c.update(y=y.reshape(M, H), st=st.reshape(M, 2), by=by, bst=bst, stats=st.reshape(M, 2).float())
    if not backward:
        return c
    for attempt in range(3):
        _text_backward_reference(c, e, e_x)
        t, b, sent = c["t"], c["bounds"], c["sent"]
        need = max(float((16 * b["dgamma"] / (t["dy"] * t["xh"])[sent].abs()).max()), float((16 * b["dbeta"] / t["dy"][sent].abs()).max()),
                   float((16 * b["dtype0"] / c["ref"]["dx"].reshape(M, H)[sent].abs()).max()))
        if need <= 1.0:
            break
        assert need <= 8.0, f"a sentinel term is {need:.3g}x short: the rows are not built as text_case says"
        c["dy"].reshape(M, H)[sent] *= 2.0 ** math.ceil(math.log2(need))
    assert_sentinels("text dgamma", t["dy"] * t["xh"], b["dgamma"], sent)
    assert_sentinels("text dbeta", t["dy"], b["dbeta"], sent)
    assert_sentinels("text dtype0", c["ref"]["dx"].reshape(M, H), b["dtype0"], sent)
    return c


def _text_backward_reference(c, e, e_x):
    B, L, H, eps = c["B"], c["L"], c["H"], c["eps"]
    M = B * L
    r = text_bwd(c["dy"], c["ids"], c["word"], c["pos"], c["type0"], c["gamma"], c["beta"], eps)
    t = ln_terms(c["dy"].reshape(M, H), e.reshape(M, H), c["gamma"], eps)
    grid = text_blocks(L)
    dx = r["dx"].reshape(M, H)
    bdx = ln_dx_bound(t, dx, None, H, False, e_x.reshape(M, H))
    e_xh_extra = (t["rstd"] * e_x.reshape(M, H))
    d_par = cdiv(L, grid) * cdiv(B, 4) + 3 + grid
    tg = (t["dy"] * t["xh"]).abs().sum(0) + c["init_dgamma"].to(F64).abs()
    bounds = {"dgamma": gam(d_par + 4) * tg + 1.0001 * (t["dy"].abs() * (U * t["mean"].abs() * t["rstd"] + e_xh_extra)).sum(0),
              "dbeta": gam(d_par) * (t["dy"].abs().sum(0) + c["init_dbeta"].to(F64).abs())}
    dx3, bdx3 = dx.reshape(B, L, H), bdx.reshape(B, L, H)
    bpos = torch.zeros_like(c["init_dpos"], dtype=F64)
    bpos[:L] = gam(cdiv(B, 4) + 4) * (dx3.abs().sum(0) + c["init_dpos"][:L].to(F64).abs()) + bdx3.sum(0)
    bounds["dpos"] = bpos
    bounds["dtype0"] = gam(cdiv(B, 4) + cdiv(L, grid) + 3 + grid) * (dx.abs().sum(0) + c["init_dtype0"].to(F64).abs()) + bdx.sum(0)
    flat = c["ids"].reshape(-1)
    count = torch.bincount(flat, minlength=TEXT_VOCAB).to(F64)
    mag = torch.zeros(TEXT_VOCAB, H, dtype=F64, device=dx.device).index_add_(0, flat, dx.abs())
    eb = torch.zeros(TEXT_VOCAB, H, dtype=F64, device=dx.device).index_add_(0, flat, bdx)
    bw = gam(count)[:, None] * (mag + c["init_dword"].to(F64).abs()) + eb
    bw[0] = 0.0
    bounds["dword"] = bw
    named = count > 0
    named[0] = False
    c.update(ref=r, bounds=bounds, named=named, t=t)


def check_text_fwd(name, c, y, y_lp, stats):
    within((name, "y"), y, c["y"], c["by"])
    within((name, "stats"), stats, c["st"], c["bst"])
    if y_lp is not None:
        same_bits(f"{name} y_lp (round-to-nearest-even copy of y)", y_lp, y.to(y_lp.dtype))


def check_text_bwd(name, c, got):
    """got: dict of the five buffers after the call (init + gradient).  Word rows no id names, and row 0, and dpos rows >= L: bit for bit."""
    L = c["L"]
    same_bits(f"{name} dword (rows no id names, padding row)", got["dword"][~c["named"]], c["init_dword"][~c["named"]])
    same_bits(f"{name} dpos (rows >= L)", got["dpos"][L:], c["init_dpos"][L:])
    for k in ("dword", "dpos", "dtype0", "dgamma", "dbeta"):
        within((name, k), got[k], c["init_" + k].to(F64) + c["ref"][k], c["bounds"][k])


def emulate_text(c, backward=True):
    """fp32 emulation of text_embed_fwd_kernel / text_embed_bwd_kernel in their operation order (atomics in reverse order)"""
    f = torch.float32
    B, L, H = c["B"], c["L"], c["H"]
    M = B * L
    ids = c["ids"]
    x = ((c["word"][ids] + c["pos"][:L][None]) + c["type0"]).reshape(M, H)
    mean = _row_sum32(x) * f32(1.0 / H)
    xc = x - mean
    rstd = torch.rsqrt(_row_sum32(xc * xc) * f32(1.0 / H) + torch.tensor(c["eps"], dtype=f))
    y = xc * rstd * c["gamma"] + c["beta"]
    stats = torch.cat([mean, rstd], 1)
    if not backward:
        return y, stats, None
    st = c["stats"]
    xh = (x - st[:, :1]) * st[:, 1:]
    dy = c["dy"].reshape(M, H)
    gy = dy * c["gamma"]
    c1 = _row_sum32(gy) * f32(1.0 / H)
    c2 = _row_sum32(gy * xh) * f32(1.0 / H)
    dx = (st[:, 1:] * (gy - c1 - xh * c2)).reshape(B, L, H)
    grid = text_blocks(L)
    got = {k: c["init_" + k].clone() for k in ("dword", "dpos", "dtype0", "dgamma", "dbeta")}
    zero = lambda: torch.zeros(4, H, dtype=f)
    comb = lambda a: ((a[0] + a[1]) + a[2]) + a[3]
    dyx = (dy * xh).reshape(B, L, H)
    dy3 = dy.reshape(B, L, H)
    for blk in reversed(range(grid)):
        ag, ab, at = zero(), zero(), zero()
        for l in range(blk, L, grid):
            ap = zero()
            for b in range(B):
                w = b % 4
                ag[w] = ag[w] + dyx[b, l]
                ab[w] = ab[w] + dy3[b, l]
                ap[w] = ap[w] + dx[b, l]
                if int(ids[b, l]) != 0:
                    got["dword"][int(ids[b, l])] += dx[b, l]
            got["dpos"][l] += comb(ap)
            at = at + ap
        got["dgamma"] += comb(ag)
        got["dbeta"] += comb(ab)
        got["dtype0"] += comb(at)
    return y, stats, got


def text_cases():
    """(dtype name of y_lp, H, B, L, id pattern, eps, backward?)"""
    out, i = [], 0
    for H in TEXT_H:
        for (B, L) in TEXT_SHAPES + TEXT_FWD_ONLY:
            out.append((("bf16", "fp32")[i % 2], H, B, L, TEXT_IDS[i % len(TEXT_IDS)], LN_EPS[(i // 2) % 2], (B, L) not in TEXT_FWD_ONLY))
            i += 1
    for i, kind in enumerate(TEXT_IDS):                  # every id pattern at the ordinary shape, whatever the cycle above gave it
        out.append((("fp32", "bf16")[i % 2], TEXT_H[i % 3], 32, 80, kind, LN_EPS[i % 2], True))
    return out


def emulate_ln_fwd(x, gamma, beta, eps, out_dtype):
    """fp32 emulation of ln_fwd_kernel: lane-sequential sums then the butterfly, two-pass variance, rsqrt"""
    f = torch.float32
    x = x.to(f)
    H = x.shape[1]
    mean = _row_sum32(x) * f32(1.0 / H)
    v = x - mean
    rstd = torch.rsqrt(_row_sum32(v * v) * f32(1.0 / H) + torch.tensor(eps, dtype=f))
    return (v * rstd * gamma.to(f) + beta.to(f)).to(out_dtype), torch.cat([mean, rstd], 1)


# ---- cross-entropy -------------------------------------------------------------------------------------------------------------
def ce(logits, labels, scale, ignore_index):
    """F.cross_entropy(reduction='sum', ignore_index) * scale, restated: -> loss, dlogits, and the per-row pieces the bound uses"""
    s = logits.to(F64)
    keep = labels != ignore_index
    mx = s.max(-1, keepdim=True).values
    sm = torch.exp(s - mx).sum(-1, keepdim=True)
    lse = mx + torch.log(sm)
    y = torch.where(keep, labels, torch.zeros_like(labels))
    nll = (lse - s.gather(1, y[:, None])).squeeze(1)
    nll = torch.where(keep, nll, torch.zeros_like(nll))
    loss = scale * nll.sum()
    p = torch.exp(s - lse)
    onehot = torch.zeros_like(s).scatter_(1, y[:, None], 1.0)
    dl = torch.where(keep[:, None], scale * (p - onehot), torch.zeros_like(s))
    return loss, dl, {"p": p, "onehot": onehot, "lse": lse, "mx": mx, "sum": sm, "nll": nll, "keep": keep, "s": s}


def ce_bounds(q, B, G, scale):
    s, lse, mx, sm = q["s"], q["lse"], q["mx"], q["sum"]
    fin = torch.isfinite(s)
    span = torch.where(fin, (s - mx).abs(), torch.zeros_like(s)).max(-1, keepdim=True).values
    e_sum = (2 * U + U * span) + gam(cdiv(G, 64) + 6)                       # relative error of the row sum
    e_lse = e_sum + 2 * U * torch.log(sm).abs() + U * lse.abs()             # absolute error of lse
    sl = torch.where(fin, (s - lse).abs(), torch.zeros_like(s))
    bdl = abs(scale) * (q["p"] * (e_lse + U * sl + 2 * U) + 2 * U * (q["p"] - q["onehot"]).abs())
    bdl = torch.where(q["keep"][:, None], bdl, torch.zeros_like(bdl))
    keep = q["keep"].to(F64)
    d = cdiv(B, 16) + 16
    bloss = abs(scale) * float((keep * e_lse.squeeze(1)).sum()) + gam(d + 2) * abs(scale) * float(q["nll"].abs().sum())
    return torch.tensor(bloss, dtype=F64, device=s.device), bdl


def check_ce(name, loss, dlogits, logits, labels, scale, ignore_index):
    B, G = logits.shape
    rl, rd, q = ce(logits, labels, scale, ignore_index)
    bl, bd = ce_bounds(q, B, G, scale)
    if not bool(q["keep"].any()):
        assert float(loss) == 0.0, f"{name}: loss {float(loss)} with every row ignored"
    within((name, "loss"), loss.reshape(()), rl, bl)
    if dlogits is not None:
        zero = (~q["keep"])[:, None] | torch.isneginf(logits)
        assert bool((dlogits[zero.expand_as(dlogits)] == 0).all()), f"{name}: dlogits non-zero on an ignored row or in a -inf column"
        within((name, "dlogits"), dlogits, rd, bd)


def emulate_ce(logits, labels, scale, ignore_index):
    f = torch.float32
    B, G = logits.shape
    s = logits.to(f)
    sc = torch.tensor(scale, dtype=f)
    Gp = cdiv(G, 64) * 64
    mx = s.max(-1, keepdim=True).values
    e = torch.cat([torch.exp(s - mx), torch.zeros(B, Gp - G, dtype=f)], 1).reshape(B, Gp // 64, 64)
    acc = torch.zeros(B, 64, dtype=f)
    for j in range(Gp // 64):
        acc = acc + e[:, j]
    lse = mx + torch.log(_wave_sum32(acc))
    keep = labels != ignore_index
    y = torch.where(keep, labels, torch.zeros_like(labels))
    onehot = torch.zeros_like(s).scatter_(1, y[:, None], 1.0)
    dl = torch.where(keep[:, None], sc * (torch.exp(s - lse) - onehot), torch.zeros_like(s))
    nll = torch.where(keep, sc * (lse.squeeze(1) - s.gather(1, y[:, None]).squeeze(1)), torch.zeros(B, dtype=f))
    red = torch.zeros(16, dtype=f)
    for r in range(B):
        red[r % 16] = red[r % 16] + nll[r]
    t = torch.zeros((), dtype=f)
    for w in range(16):
        t = t + red[w]
    return t, dl


def ce_case(B, G, pattern, seed, device="cpu"):
    """pattern = (shift, ignored in {'none', 'some', 'all'}, ignore_index, scale kind).  -inf columns that no label points at,
    labels at column 0 and G - 1."""
    shift, ign, ignore_index, sk = pattern
    g = torch.Generator().manual_seed(seed)
    logits = (torch.randn(B, G, generator=g) * 3 + shift).float()
    labels = torch.randint(0, G, (B,), generator=g)
    labels[0] = 0
    labels[-1] = G - 1
    if G > 2:
        col = torch.rand(B, G, generator=g) < 0.2
        col[torch.arange(B), labels] = False
        logits[col] = float("-inf")
    if ign == "all":
        labels[:] = ignore_index
    elif ign == "some" and B > 1:
        labels[torch.rand(B, generator=g) < 0.4] = ignore_index
        labels[B // 2] = ignore_index
    scale = f32(1.0 / B) if sk == "mean" else f32(0.37)
    return logits.to(device), labels.to(device), scale, ignore_index


CE_B = (1, 7, 16, 17, 33, 100)
CE_G = (1, 2, 63, 64, 65, 130, 1000)
CE_PATTERNS = [(sh, ign, ii, sk) for sh in (0.0, 80.0, -80.0) for ign in ("none", "some", "all") for ii in (-100, -1) for sk in ("mean", "fixed")]


def ce_cases():
    out = []
    for i, (B, G) in enumerate((b, g) for b in CE_B for g in CE_G):
        out.append((B, G, CE_PATTERNS[(i * 7) % len(CE_PATTERNS)]))
        out.append((B, G, CE_PATTERNS[(i * 7 + 19) % len(CE_PATTERNS)]))
    return out


# ---- column sum ----------------------------------------------------------------------------------------------------------------
COLSUM_M = (1, 63, 64, 65, 333)
COLSUM_N = (4, 252, 256, 260, 776)


def colsum(dy):
    return dy.to(F64).sum(0)


def colsum_depth(M):
    return min(16, cdiv(M, 4)) + 3 + cdiv(M, 64)


def colsum_case(M, N, dtype, seed, device="cpu"):
    g = torch.Generator().manual_seed(seed)
    dy = torch.randn(M, N, generator=g) * 2.0 ** torch.randint(-10, 4, (M, 1), generator=g).float()
    sent = sorted({M - 1, 64 * ((M - 1) // 64)})                  # last row; first row of the last 64-row block
    for r in sent:
        dy[r] = torch.where(torch.rand(N, generator=g) < 0.5, -1.0, 1.0) * (4.0 + 4.0 * torch.rand(N, generator=g))
    dy = dy.to(dtype)
    init = torch.randn(N, generator=g)
    bound = gam(colsum_depth(M)) * (dy.to(F64).abs().sum(0) + init.to(F64).abs())
    assert_sentinels("colsum", dy.to(F64), bound, sent)
    return dy.to(device), init.to(device), bound.to(device), sent


def emulate_colsum(dy, init):
    f = torch.float32
    M, N = dy.shape
    acc = init.to(f).clone()
    for r0 in reversed(range(0, M, 64)):
        w = [torch.zeros(N, dtype=f) for _ in range(4)]
        for r in range(r0, min(M, r0 + 64)):
            w[(r - r0) % 4] = w[(r - r0) % 4] + dy[r].to(f)
        acc = acc + (((w[0] + w[1]) + w[2]) + w[3])
    return acc


# ---- weighted CSR gather-sum ---------------------------------------------------------------------------------------------------
GATHER_N = (1, 3, 5, 16389)
GATHER_H = (256, 512, 768)


def gather_sum(src, ptr, idx, w, out_init=None):
    """out[n] (+)= sum_{j in [ptr[n], ptr[n+1])} w[j] src[idx[j]]  -> (out, sum of |terms|, segment lengths)"""
    N = ptr.numel() - 1
    lens = (ptr[1:] - ptr[:-1]).long()
    seg = torch.repeat_interleave(torch.arange(N, device=src.device), lens)
    E = int(ptr[-1])
    terms = w[:E].to(F64)[:, None] * src.to(F64)[idx[:E].long()]
    out = torch.zeros(N, src.shape[1], dtype=F64, device=src.device)
    mag = torch.zeros_like(out)
    out.index_add_(0, seg, terms)
    mag.index_add_(0, seg, terms.abs())
    if out_init is not None:
        out, mag = out + out_init.to(F64), mag + out_init.to(F64).abs()
    return out, mag, lens


def gather_bound(ref, mag, lens, accumulate, bf16_out):
    b = gam(lens.to(F64) + 1 + (1 if accumulate else 0))[:, None] * mag
    return b + ulp_bf16(ref) if bf16_out else b


def gather_case(N, H, dtype, seed, device="cpu", S=97):
    """segments of 0 .. 40 entries, empty at the first row, the last row and mid-way; repeated indices; negative and zero weights"""
    g = torch.Generator().manual_seed(seed)
    lens = torch.randint(0, 41 if N < 100 else 6, (N,), generator=g)
    lens[0] = 0
    lens[-1] = 0
    lens[N // 2] = 0
    if N >= 3:
        lens[1] = 40
    ptr = torch.zeros(N + 1, dtype=torch.int32)
    ptr[1:] = torch.cumsum(lens, 0)
    E = max(int(ptr[-1]), 1)
    idx = torch.randint(0, S, (E,), generator=g, dtype=torch.int32)
    idx[: E // 3] = idx[0]                                                  # repeats
    w = torch.randn(E, generator=g)
    w[::5] = 0.0
    src = torch.randn(S, H, generator=g).to(dtype)
    init = torch.randn(N, H, generator=g).to(dtype)
    return src.to(device), ptr.to(device), idx.to(device), w.to(device), init.to(device)


def emulate_gather(src, ptr, idx, w, init, accumulate, dtype):
    """fp32, the kernel's order: entry k of every segment is added in step k (one sequential chain per row), one rounding at the end"""
    f = torch.float32
    N = ptr.numel() - 1
    out = init.to(f).clone() if accumulate else torch.zeros(N, src.shape[1], dtype=f)
    start, lens = ptr[:-1].long(), (ptr[1:] - ptr[:-1]).long()
    for k in range(int(lens.max()) if N else 0):
        rows = (lens > k).nonzero().squeeze(1)
        j = start[rows] + k
        out[rows] = out[rows] + w[j][:, None] * src[idx[j].long()].to(f)
    return out.to(dtype)


# ---- sum of squares ------------------------------------------------------------------------------------------------------------
SQNORM_GRID_CAP = 256 * 8
ADAMW_GRID_CAP = 256 * 16
SQNORM_N = (4, 1028, 2097152 + 1028)


def frozen_elems(mask, n):
    """bool [n]: the elements of the 64-blocks whose mask byte is 2 or 3 (bit 1 of a byte > 3 still means 'decay', not 'frozen')"""
    if mask is None:
        return None
    fr = (mask == 2) | (mask == 3)
    return fr.repeat_interleave(64)[:n]


def sumsq(g, mask=None):
    """-> (sum of squares, count of non-finite values) over the blocks that are not frozen; non-finite values count and poison"""
    x = g.to(F64)
    fr = frozen_elems(mask, g.numel())
    if fr is not None:
        x = x[~fr]
    return (x * x).sum(), int((~torch.isfinite(x)).sum())


def sumsq_bound(g, mask, start):
    n = g.numel()
    n4 = n // 4
    grid = min(cdiv(n4, 256), SQNORM_GRID_CAP)
    iters = cdiv(n4, 256 * grid)
    x = g.to(F64)
    fr = frozen_elems(mask, n)
    if fr is not None:
        x = torch.where(fr, torch.zeros_like(x), x)
    sq = x * x
    total = float(sq.sum())
    q = torch.cat([sq.reshape(-1, 4).sum(1), torch.zeros(iters * grid * 256 - n4, dtype=F64, device=g.device)])
    parts = q.reshape(iters, grid, 256).sum((0, 2))                         # block partials
    chain = torch.cumsum(torch.cat([torch.tensor([abs(start)], dtype=F64, device=g.device), torch.sort(parts, descending=True).values]), 0)[1:]
    return gam(1 + 3 + iters + 6 + 3) * total + U * float(chain.sum())


def emulate_sumsq(g, mask, start):
    f = torch.float32
    n = g.numel()
    n4 = n // 4
    grid = min(cdiv(n4, 256), SQNORM_GRID_CAP)
    iters = cdiv(n4, 256 * grid)
    x = g.to(f)
    fr = frozen_elems(mask, n)
    if fr is not None:
        x = torch.where(fr, torch.zeros_like(x), x)
    sq = (x * x).reshape(-1, 4)
    q = ((sq[:, 0] + sq[:, 1]) + sq[:, 2]) + sq[:, 3]
    q = torch.cat([q, torch.zeros(iters * grid * 256 - n4, dtype=f)]).reshape(iters, grid, 4, 64)
    s = torch.zeros(grid, 4, 64, dtype=f)
    for k in range(iters):
        s = s + q[k]
    w = _wave_sum32(s.reshape(grid * 4, 64)).reshape(grid, 4)
    parts = ((w[:, 0] + w[:, 1]) + w[:, 2]) + w[:, 3]
    acc = torch.tensor(start, dtype=f)
    for b in torch.sort(parts, descending=True).values:
        acc = acc + b
    return acc


# ---- AdamW ---------------------------------------------------------------------------------------------------------------------
ADAMW_N = (64, 1028, 1 << 18, 4194304 + 1028)
MASK_BYTES = (0, 1, 2, 3, 255)
HYPER = ((0.9, 0.98, 1e-6), (0.9, 0.999, 1e-8))                  # (beta1, beta2, eps): pre-training; torch's defaults (fine-tuning)
COUNTED_N = (1028, 1 << 18)
COUNTED = ((0, 1, 1), (1, 0, 1), (0, 0, 1), (1, 1, 1), (0, 1, 0))  # (hf_style, index into HYPER, correct_bias)
CAST_N = (1, 7, 8, 9, 100003, 8388621)
SCALE_N = (1, 5, 1048579)
SCALES = (1.0, 1.0 / 3.0, -0.37)


def adamw_cases():
    """(n, hf_style, correct_bias, index into HYPER, grad_scale, max_norm, shadow in {'half', 'all', 'zero', 'null'}, mask?, zero_grads)"""
    out = []
    for i, (n, hf, cb, h) in enumerate((n, hf, cb, h) for n in ADAMW_N for hf in (0, 1) for cb in (0, 1) for h in (0, 1)):
        out.append((n, hf, cb, h, (1.0, 0.5, 1.0 / 65536)[i % 3], (0.0, 1.0, 5.0)[(i // 2) % 3], ("half", "all", "zero", "null")[(i // 3) % 4],
                    i % 5 != 4, i % 7 != 6))
    return out


def sqnorm_cases():
    return [(n, masked, bad) for n in SQNORM_N for masked in (False, True) for bad in (0, 1, 5)]


def mask_elems(mask, n):
    """-> (decay bool [n], frozen bool [n]) from one byte per 64 elements: 0 no decay, 1 decay, 2 / 3 frozen, > 3 decay"""
    if mask is None:
        return None, None
    mb = torch.where(mask > 3, torch.ones_like(mask), mask)
    return ((mb & 1) != 0).repeat_interleave(64)[:n], ((mb & 2) != 0).repeat_interleave(64)[:n]


def adamw(p, g, m, v, cfg, sumsq_val=None, mask=None, skip=False, steps_applied=None):
    """One step in fp64 from fp32 state.  cfg: dict of the etp_adamw_cfg fields, every float already the fp32 value the ABI carries.
    steps_applied: the device counter BEFORE this call (etp_adamw_step_counted) -- the step used is steps_applied + 1 when the update
    is applied, and the counter does not move on a skipped step; None: cfg['step'].
    -> dict p, m, v (new, fp64), upd (the Adam update that was subtracted), q (hf style: p after the update, before the decay),
    counter, and the pieces the bound needs."""
    n = p.numel()
    p0, g0, m0, v0 = (t.to(F64) for t in (p, g, m, v))
    decay, frozen = mask_elems(mask, n)
    counter = steps_applied
    if skip:
        return {"p": p0, "m": m0, "v": v0, "counter": counter, "skipped": True, "frozen": frozen}
    step = cfg["step"] if steps_applied is None else steps_applied + 1
    counter = None if steps_applied is None else steps_applied + 1
    b1, b2, lr, eps = cfg["beta1"], cfg["beta2"], cfg["lr"], cfg["eps"]
    gs = cfg["grad_scale"]
    if cfg["max_norm"] > 0.0 and sumsq_val is not None:
        gs = gs * min(1.0, cfg["max_norm"] / (math.sqrt(sumsq_val) * abs(cfg["grad_scale"]) + 1e-6))
    gr = g0 * gs
    m1 = b1 * m0 + (1.0 - b1) * gr
    v1 = b2 * v0 + (1.0 - b2) * gr * gr
    bc1 = 1.0 - b1 ** step if cfg["correct_bias"] else 1.0
    bc2 = 1.0 - b2 ** step if cfg["correct_bias"] else 1.0
    wd = cfg["weight_decay"] * (torch.ones_like(p0) if decay is None else decay.to(F64))
    if cfg["hf_style"]:
        denom = torch.sqrt(v1) + eps
        upd = (lr * math.sqrt(bc2) / bc1) * m1 / denom
        q = p0 - upd
        p1 = q - lr * wd * q
        coef = lr * math.sqrt(bc2) / bc1
    else:
        denom = torch.sqrt(v1) / math.sqrt(bc2) + eps
        q = p0 * (1.0 - lr * wd)
        upd = (lr / bc1) * m1 / denom
        p1 = q - upd
        coef = lr / bc1
    out = {"p": p1, "m": m1, "v": v1, "upd": upd, "q": q, "gr": gr, "denom": denom, "coef": coef, "counter": counter, "skipped": False,
           "frozen": frozen, "step": step}
    if frozen is not None:
        for k, old in (("p", p0), ("m", m0), ("v", v0)):
            out[k] = torch.where(frozen, old, out[k])
    return out


def adamw_bounds(p, m, v, r, cfg, counted):
    """elementwise bounds of p, m, v after one step (r = adamw(...) from the same fp32 p, m, v).
      gr      g * gs: one rounding, gs itself 5 (sqrtf, *|grad_scale|, + 1e-6, /, * grad_scale)                     -> 6u relative
      m'      b1*m + (1-b1)*gr: 2 roundings on the first product's path, 1-b1 / product / sum on the second          -> u (2|b1 m| + 9|(1-b1) gr|)
      v'      the same with gr*gr (twice gr's error plus the product)                                               -> u (2|b2 v| + 16|(1-b2) gr^2|)
      update  coef * m' / denom: m' contributes coef / denom * bound_m; denom = sqrt(v') (/ sqrt(bc2)) + eps is relatively within
              bound_v / (2 v') + 4u; coef (lr, bc1, sqrt(bc2): one product, one quotient), the quotient and the product 5u more; the
              bias corrections e_bc: u each when computed on the host in double and rounded, and on the device (counted entry point)
              powf within one ulp: 2u b^t / (1 - b^t) + 2u for the subtraction and the sqrtf
      p       decay: three roundings on p_old's path (lr*wd, 1 - ., product) resp. on q's (hf style); the final subtraction one on
              p_new:  4u (|p_old| + |q|) + u |p_new| + bound_update"""
    p0, m0, v0 = (t.to(F64) for t in (p, m, v))
    b1, b2 = cfg["beta1"], cfg["beta2"]
    gr = r["gr"]
    bm = U * (2 * (b1 * m0).abs() + 9 * ((1.0 - b1) * gr).abs())
    bv = U * (2 * (b2 * v0).abs() + 16 * ((1.0 - b2) * gr * gr).abs())
    e_bc = 0.0
    if cfg["correct_bias"]:
        if counted:
            t = r["step"]
            e_bc = (2 * b1 ** t / (1 - b1 ** t) + 2) * U + (b2 ** t / (1 - b2 ** t) + 2) * U
        else:
            e_bc = 2 * U
    rel_v = torch.where(r["v"] > 0, bv / r["v"].clamp_min(1e-300), torch.zeros_like(bv))
    bupd = r["coef"] / r["denom"] * bm + r["upd"].abs() * (0.5 * rel_v + 9 * U + e_bc)
    bp = 4 * U * (p0.abs() + r["q"].abs()) + U * r["p"].abs() + bupd
    if r["frozen"] is not None:
        z = torch.zeros_like(bp)
        bp, bm, bv = (torch.where(r["frozen"], z, b) for b in (bp, bm, bv))
    return bp, bm, bv


def cfg_f32(**kw):
    """the hyper-parameters as the fp32 values the ABI carries"""
    out = dict(kw)
    for k in ("lr", "beta1", "beta2", "eps", "weight_decay", "grad_scale", "max_norm"):
        out[k] = f32(out[k])
    return out


def emulate_adamw(p, g, m, v, cfg, sumsq_val, mask, counted_step=None):
    """adamw_kernel's exact operation order in fp32 (no fused multiply-adds).  counted_step: the device counter after the bump."""
    f = torch.float32
    T = lambda x: torch.tensor(x, dtype=f)
    n = p.numel()
    b1, b2, lr, eps, wdv = T(cfg["beta1"]), T(cfg["beta2"]), T(cfg["lr"]), T(cfg["eps"]), T(cfg["weight_decay"])
    one = T(1.0)
    if not cfg["correct_bias"]:
        bc1, bc2s = one, one
    elif counted_step is not None:
        t = T(float(counted_step))
        bc1, bc2s = one - torch.pow(b1, t), torch.sqrt(one - torch.pow(b2, t))
    else:
        bc1 = T(1.0 - float(b1.double()) ** cfg["step"])
        bc2s = T(math.sqrt(1.0 - float(b2.double()) ** cfg["step"]))
    gs = T(cfg["grad_scale"])
    if cfg["max_norm"] > 0 and sumsq_val is not None:
        norm = torch.sqrt(T(sumsq_val)) * gs.abs()
        gs = gs * torch.minimum(one, T(cfg["max_norm"]) / (norm + T(1e-6)))
    decay, frozen = mask_elems(mask, n)
    wd = wdv * (torch.ones(n, dtype=f) if decay is None else decay.to(f))
    gr = g * gs
    m1 = b1 * m + (one - b1) * gr
    v1 = b2 * v + (one - b2) * gr * gr
    if cfg["hf_style"]:
        upd = p - (lr * bc2s / bc1) * m1 / (torch.sqrt(v1) + eps)
        p1 = upd - lr * wd * upd
    else:
        dec = p * (one - lr * wd)
        p1 = dec - (lr / bc1) * m1 / (torch.sqrt(v1) / bc2s + eps)
    if frozen is not None:
        p1, m1, v1 = torch.where(frozen, p, p1), torch.where(frozen, m, m1), torch.where(frozen, v, v1)
    return p1, m1, v1


def adamw_mask(n, seed, device="cpu"):
    """ceil(n / 64) bytes drawn from MASK_BYTES, every value present when there are enough blocks"""
    g = torch.Generator().manual_seed(seed)
    nb = cdiv(n, 64)
    mask = torch.tensor(MASK_BYTES, dtype=torch.uint8)[torch.randint(0, len(MASK_BYTES), (nb,), generator=g)]
    if nb >= 10:
        mask[:5] = torch.tensor(MASK_BYTES, dtype=torch.uint8)
        mask[-1] = 0                                                         # the (partial) last block does not decay, the guard byte behind it
        mask[-2] = 1                                                         # means FROZEN: a read one byte too far changes the result
    return mask.to(device)


def check_adamw(name, got, old, r, cfg, counted, shadow=None, shadow_old=None, n_shadow=0):
    """got / old: (p, m, v) after / before the call; r: adamw(...) of `old`.  Frozen blocks and a skipped step: bit for bit."""
    if r["skipped"]:
        for k, a, b in zip("pmv", got, old):
            same_bits(f"{name} {k} (skipped step)", a, b)
        if shadow is not None:
            same_bits(f"{name} shadow (skipped step)", shadow, shadow_old)
        return
    bp, bm, bv = adamw_bounds(*old, r, cfg, counted)
    within((name, "p"), got[0], r["p"], bp)
    within((name, "m"), got[1], r["m"], bm)
    within((name, "v"), got[2], r["v"], bv)
    fr = r["frozen"]
    if fr is not None:
        for k, a, b in zip("pmv", got, old):
            same_bits(f"{name} {k} (frozen blocks)", a[fr], b[fr])
    if shadow is not None:
        want = bf16_rne(got[0][:n_shadow])
        live = torch.ones(n_shadow, dtype=torch.bool, device=shadow.device) if fr is None else ~fr[:n_shadow]
        same_bits(f"{name} shadow (round-to-nearest-even copy of the new p)", shadow[:n_shadow][live], want[live])
        same_bits(f"{name} shadow (frozen blocks)", shadow[:n_shadow][~live], shadow_old[:n_shadow][~live])
        same_bits(f"{name} shadow (beyond n_shadow)", shadow[n_shadow:], shadow_old[n_shadow:])


def check_grads_after(name, g_after, g_before, zero_grads):
    """zero_grads: every gradient exactly zero, frozen blocks included; otherwise bit-intact"""
    if zero_grads:
        assert not bool((g_after != 0).any()) and not bool(torch.isnan(g_after).any()), f"{name}: a gradient was left non-zero"
    else:
        same_bits(f"{name} gradients (zero_grads = 0)", g_after, g_before)


# ---- guarded output buffers (GPU files) ---------------------------------------------------------------------------------------
GUARD = 64


class Guarded:
    """a tensor inside a larger allocation: GUARD elements of a fixed bit pattern on either side, which a kernel must leave alone"""

    def __init__(self, shape, dtype=torch.float32, init=None, device="cuda"):
        n = 1
        for s in shape:
            n *= s
        self.buf = torch.full((n + 2 * GUARD,), -7.0e4 if dtype != torch.uint8 else 2, dtype=dtype, device=device)
        self.t = self.buf[GUARD:GUARD + n].view(*shape)
        self.t.copy_(init) if init is not None else self.t.fill_(float("nan"))
        self.ref = self.buf.clone()

    def check(self, name):
        same_bits(f"{name}: front guard", self.buf[:GUARD], self.ref[:GUARD])
        same_bits(f"{name}: back guard", self.buf[-GUARD:], self.ref[-GUARD:])

    def intact(self, name):
        same_bits(f"{name}: untouched", self.buf, self.ref)


def gptr(g):
    return None if g is None else g.t.data_ptr()
