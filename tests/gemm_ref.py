"""fp64 restatement of the GEMM operator (etp_gemm / etp_gemm_group, include/etpnav_hip.h) with a propagated, elementwise error
bound, the comparator and the case generator of its op-level tests (tests/test_gemm_kernels_gpu.py).

tests/test_gemm_ref_cpu.py pins the values to oracle/planner_oracle.py's `linear`, `gelu_erf` and their autograd;
tests/test_gemm_bounds_cpu.py shows that CPU emulations of the kernels' summation and rounding schedules stay inside the bound and
that the comparator can fail.

  gemm_ref(A, B, alpha=, bias=, R=, C0=, Z=, act=, out_mode=, ksplit=, bk=, bf16=, c_bf16=, colsum_old=) -> (values, bounds)
      A [.., M, K], B [.., N, K]: the STORED operand values in their logical orientation (bf16 or fp32 values, converted exactly);
      bias [N] fp32; R, C0 [.., M, N] in the output dtype; Z [.., M, N] the activation operand of the backward forms (operand dtype,
      IEEE half values for ACT_MUL_Z in bf16 mode); colsum_old [M].  values / bounds: dicts over "C", "Z" (where the epilogue writes
      it) and "a_colsum" (where colsum_old is given).

      acc = sum_k A[m,k] B[n,k]      v = alpha acc + bias      y = act(v) [* factor(Z)] + R      C = y | C0 + y

The bound is not a measured number and carries no multiplier: it is the first-order propagation of the rounding points the kernels
document, per element, with S = |A| |B|^T.  Each line names what it models:

  E_acc = (K + 2) 2^-24 |alpha| S           K fp32 additions in ANY order (MFMA chains, ring slabs, the two partial sums of the mm32
                                            k2 classes); with fp32 operands the products' own rounding as well.  Loose on purpose (a
                                            chained fp32 sum stays below 0.03 of it): it scales with the element's own S, so an element
                                            of a 2^-10 row is held as tightly, relative to itself, as one of a 2^3 row.
  E_v   = E_acc + 2^-24 (|alpha acc| + |v|) the scaling and the bias addition (summed over the splits under ksplit > 1: the bias
                                            goes to split 0 only).  E_v = 0 where S = 0: a zero operand row gives v = bias exactly,
                                            so those outputs are exactly epi(0) up to the epilogue's own roundings below.
  Z, ACT_GELU:          E_v + u_T |v|                               u_T = 2^-8 (bf16 store) or 0 (fp32)
  Z, ACT_GELU_SAVEGRAD: 0.8 E_v + u_Z |gelu'(v)| + FP32_REL         0.8 >= max |gelu''|; u_Z = 2^-11 (IEEE half store) or 0
  y, GELU (both forms): |gelu'(v)| E_v + FP32_REL                   FP32_REL: the project's fp32 class of the erf / exp / rcp forms
  y, RELU:              E_v                                         relu is 1-Lipschitz: an element with |v| <= E_v may come out 0 or v
  y, GELU_BWD:          |gelu'(Z)| E_v + FP32_REL |v|
  y, MUL_Z / RELU_BWD:  |factor| E_v                                factor = Z / (Z > 0); RELU_BWD operands are generated away from 0
     MUL_Z:             + 2^-24 |v factor|                          the fp32 product's own rounding (RELU_BWD selects, GELU_BWD's
                                                                    FP32_REL |v| covers it).  Not a guess: with a bias, an accumulator
                                                                    that is negligible beside it (a 2^-10 row) and a small residual
                                                                    the three roundings bias-add, product, residual-add each reach
                                                                    2^-24 |y| while the terms above sum to 2 x 2^-24 |y|
                                                                    (tests/test_gemm_bounds_cpu.py found it at 128 x 384 x 96).
  + R, + old C (out_mode 1): 2^-24 (|term| + |result|) per fp32 addition
  out_mode 2:           ksplit 2^-24 (sum_splits |partial| + |C0|)  the atomic additions, in any order
  C store:              u_C |y|                                     u_C = 2^-8 for a bf16 C (out_mode 1 rounds once, after the fp32 sum)
  a_colsum:             (K + 2) 2^-24 sum_k |A[m,k]| + 2^-24 |old|
"""
import math

import torch

from tests.attn_ref import FP32_REL, U_BF16, same_bits  # noqa: F401  (same_bits: re-exported for the GPU tests)

F64 = torch.float64
U_HALF = 2.0 ** -11
EPS32 = 2.0 ** -24
ACT_NONE, ACT_GELU, ACT_RELU, ACT_GELU_BWD, ACT_RELU_BWD, ACT_GELU_SAVEGRAD, ACT_MUL_Z = range(7)    # include/etpnav_hip.h
ACTS = (ACT_NONE, ACT_GELU, ACT_RELU, ACT_GELU_BWD, ACT_RELU_BWD, ACT_GELU_SAVEGRAD, ACT_MUL_Z)
ACT_WRITES_Z = (ACT_GELU, ACT_GELU_SAVEGRAD)
ACT_READS_Z = (ACT_GELU_BWD, ACT_RELU_BWD, ACT_MUL_Z)

# worst |got - ref| / E seen per key (the GPU tests use "<kernel instance name>/<tensor>")
WORST = {}


def f32(x):
    """the value a kernel sees for a Python float passed as a C float"""
    return float(torch.tensor(x, dtype=torch.float32))


def gelu(v):
    return v * 0.5 * (1.0 + torch.erf(v / math.sqrt(2.0)))


def gelu_grad(v):
    return 0.5 * (1.0 + torch.erf(v / math.sqrt(2.0))) + v * torch.exp(-0.5 * v * v) / math.sqrt(2.0 * math.pi)


def split_ranges(K, ksplit, bk):
    """[k_begin, k_end) of every split: gemm.hip's `per = round_up(ceil(K / ksplit), BK)`; trailing splits may be empty"""
    if ksplit <= 1:
        return [(0, K)]
    per = (-(-K // ksplit) + bk - 1) // bk * bk
    return [(min(K, s * per), min(K, (s + 1) * per)) for s in range(ksplit)]


def gemm_ref(A, B, alpha=1.0, bias=None, R=None, C0=None, Z=None, act=ACT_NONE, out_mode=0, ksplit=1, bk=64, bf16=True,
             c_bf16=None, colsum_old=None):
    A, B = A.detach().to(F64), B.detach().to(F64)
    K = A.shape[-1]
    c_bf16 = bf16 if c_bf16 is None else c_bf16
    # (the library refuses a residual on a split product; the restatement keeps it -- added once -- for the mutation tests)
    assert ksplit == 1 or (Z is None and act == ACT_NONE and out_mode == 2), "the contract of include/etpnav_hip.h"
    assert out_mode == 0 or C0 is not None
    Bt = B.transpose(-1, -2)
    S = A.abs() @ Bt.abs()
    b64 = torch.zeros((), dtype=F64, device=A.device) if bias is None else bias.detach().to(F64)
    parts = [alpha * (A[..., a:b] @ Bt[..., a:b, :]) for a, b in split_ranges(K, ksplit, bk)]      # alpha acc_s
    vs = [p + b64 if s == 0 else p for s, p in enumerate(parts)]
    v = sum(vs)
    E_v = (K + 2) * EPS32 * abs(alpha) * S + EPS32 * sum(p.abs() + x.abs() for p, x in zip(parts, vs))
    E_v = torch.where(S == 0, torch.zeros_like(E_v), E_v)
    val, E = {}, {}
    if act == ACT_NONE:
        y, E_y = v, E_v
    elif act in ACT_WRITES_Z:
        d = gelu_grad(v)
        y, E_y = gelu(v), d.abs() * E_v + FP32_REL
        if act == ACT_GELU:
            val["Z"], E["Z"] = v, E_v + (U_BF16 if bf16 else 0.0) * v.abs()
        else:
            val["Z"], E["Z"] = d, 0.8 * E_v + (U_HALF if bf16 else 0.0) * d.abs() + FP32_REL
    elif act == ACT_RELU:
        y, E_y = torch.relu(v), E_v
    else:
        z = Z.detach().to(F64)
        f = gelu_grad(z) if act == ACT_GELU_BWD else (z if act == ACT_MUL_Z else (z > 0).to(F64))
        y, E_y = v * f, f.abs() * E_v
        if act == ACT_GELU_BWD:
            E_y = E_y + FP32_REL * v.abs()
        elif act == ACT_MUL_Z:
            E_y = E_y + EPS32 * y.abs()
    if R is not None:
        r = R.detach().to(F64)
        y = y + r
        E_y = E_y + EPS32 * (r.abs() + y.abs())
    if out_mode == 1:
        c0 = C0.detach().to(F64)
        y = y + c0
        E_y = E_y + EPS32 * (c0.abs() + y.abs())
    elif out_mode == 2:
        c0 = C0.detach().to(F64)
        # (under ksplit == 1 `y` may carry an activation and a residual: one atomic addition of it)
        E_y = E_y + ksplit * EPS32 * ((sum(x.abs() for x in vs) if (ksplit > 1 and R is None) else y.abs()) + c0.abs())
        y = y + c0
    if c_bf16:
        E_y = E_y + U_BF16 * y.abs()
    val["C"], E["C"] = y, E_y
    if colsum_old is not None:
        old = colsum_old.detach().to(F64)
        val["a_colsum"] = old + A.sum(-1)
        E["a_colsum"] = (K + 2) * EPS32 * A.abs().sum(-1) + EPS32 * old.abs()
    return val, E


def close(got, ref, E, name, key=None):
    """every element of `got` finite and |got - ref| <= E elementwise (E = 0: equal); the worst ratio goes to WORST[key or name]."""
    got, ref = got.detach().to(F64), ref.detach().to(F64)
    E = torch.as_tensor(E, dtype=F64, device=ref.device).expand_as(ref)
    assert got.shape == ref.shape, (name, tuple(got.shape), tuple(ref.shape))
    bad = ~torch.isfinite(got)
    assert not bool(bad.any()), f"{name}: {int(bad.sum())} non-finite elements"
    diff = (got - ref).abs()
    ratio = torch.where(diff == 0, torch.zeros_like(diff), diff / E)        # E = 0 and a difference: inf
    worst = float(ratio.max()) if ratio.numel() else 0.0
    key = key or name
    if worst > WORST.get(key, (0.0, ""))[0]:
        WORST[key] = (worst, name)
    if worst > 1.0:
        i = int(ratio.reshape(-1).argmax())
        idx = tuple(int(x) for x in torch.unravel_index(torch.tensor(i), ratio.shape)) if ratio.dim() else ()
        raise AssertionError(f"{name}: |got - ref| = {worst:.3g} x the bound at {idx} (got {float(got.reshape(-1)[i]):.6g}, "
                             f"ref {float(ref.reshape(-1)[i]):.6g}, bound {float(E.reshape(-1)[i]):.3g}); "
                             f"{int((ratio > 1).sum())} of {ratio.numel()} elements beyond it")
    return worst


def check_all(got, val, E, name, key):
    """got: dict over the keys of `val` ("C", "Z", "a_colsum")"""
    for n in val:
        close(got[n], val[n], E[n], f"{name} {n}", f"{key}/{n}")


# ---- guards: an output sits inside a flat buffer of SENTINEL; everything the contract does not name must still hold it ----------
SENTINEL = -96.0                           # exact in bf16, half and fp32; no kernel result of these operands equals it by accident


class Guarded:
    """flat buffer of SENTINEL with one strided region carved out of it: `view` (sizes / strides in elements, `offset` from the
    buffer's start) is what a kernel may write.  intact() raises when any other element changed."""

    def __init__(self, total, offset, sizes, strides, dtype, device="cpu"):
        hi = offset + sum((n - 1) * s for n, s in zip(sizes, strides))
        assert 0 <= offset and hi < total, ("region outside its buffer", offset, hi, total)
        self.flat = torch.full((total,), SENTINEL, dtype=dtype, device=device)
        self.view = self.flat.as_strided(sizes, strides, offset)
        self.mask = torch.zeros(total, dtype=torch.bool, device=device)
        self.mask.as_strided(sizes, strides, offset).fill_(True)
        self.offset = offset

    def intact(self, name):
        bad = (self.flat != SENTINEL) & ~self.mask
        if bool(bad.any()):
            i = int(bad.nonzero()[0])
            raise AssertionError(f"{name}: {int(bad.sum())} elements outside the output were written, the first at flat index {i} "
                                 f"(output starts at {self.offset})")


def guarded_2d(M, N, ld, dtype, device="cpu", col0=8, rows=2):
    """an [M, N] output with leading dimension ld at column col0 of a [rows + M + rows, ld] buffer: guard rows above and below, guard
    columns 0 .. col0 - 1 and col0 + N .. ld - 1 in every row"""
    assert col0 + N <= ld
    return Guarded((M + 2 * rows) * ld, rows * ld + col0, (M, N), (ld, 1), dtype, device)


# ---- operands --------------------------------------------------------------------------------------------------------------
SCALE_EXPS = tuple(range(-10, 4))          # 2^-10 .. 2^3


def row_scales(n, gen):
    """one power-of-two scale per row: every exponent of SCALE_EXPS as often as the others, shuffled"""
    e = torch.tensor(SCALE_EXPS, dtype=torch.float64)[torch.arange(n) % len(SCALE_EXPS)]
    return (2.0 ** e[torch.randperm(n, generator=gen)]).float()


def make_operands(M, N, K, bf16, seed, batch=()):
    """CPU fp32 tensors holding the stored values: A [*batch, M, K] standard normal, B [*batch, N, K] with the project's asymmetric
    0.1 x + 0.01 (catches row / column swaps), rows of both scaled by independent powers of two 2^-10 .. 2^3, row M // 3 of A and
    row N // 2 of B exactly zero.  -> A, B, sa [M], sb [N] (the scales)."""
    gen = torch.Generator().manual_seed(100003 * seed + 1009 * M + 101 * N + K)
    sa, sb = row_scales(M, gen), row_scales(N, gen)
    A = torch.randn(*batch, M, K, generator=gen) * sa[:, None]
    B = (torch.randn(*batch, N, K, generator=gen) * 0.1 + 0.01) * sb[:, None]
    A[..., M // 3, :] = 0.0
    B[..., N // 2, :] = 0.0
    if bf16:
        A, B = A.bfloat16().float(), B.bfloat16().float()
    return A, B, sa, sb


def make_epilogue(M, N, act, bf16, c_bf16, seed, with_bias=True, with_r=True, with_c0=True, batch=()):
    """CPU fp32 tensors of the epilogue operands in their stored values: bias [N], R and C0 [*batch, M, N] (output dtype), Z the operand
    of the backward forms (operand dtype; IEEE half values for ACT_MUL_Z in bf16 mode; away from 0 for ACT_RELU_BWD) or None."""
    gen = torch.Generator().manual_seed(7919 * seed + 31 * M + N + 13 * act)
    rc = (lambda x: x.bfloat16().float()) if c_bf16 else (lambda x: x)
    out = dict(bias=torch.randn(N, generator=gen) if with_bias else None,
               R=rc(torch.randn(*batch, M, N, generator=gen)) if with_r else None,
               C0=rc(torch.randn(*batch, M, N, generator=gen)) if with_c0 else None, Z=None)
    if act in ACT_READS_Z:
        z = torch.randn(*batch, M, N, generator=gen)
        if act == ACT_RELU_BWD:
            z = torch.where(z.abs() < 0.05, z.sign() * 0.05 + (z == 0) * 0.05, z)
        if act == ACT_MUL_Z:
            z = z.half().float() if bf16 else z
        else:
            z = z.bfloat16().float() if bf16 else z
        out["Z"] = z
    return out


# ---- the shape matrix of tests/test_gemm_kernels_gpu.py (tests/test_gemm_bounds_cpu.py runs its emulations over the same list) ---
TILES = ((64, 64), (32, 64), (128, 64), (128, 128), (256, 128))
REG_K = (0, 8, 40, 64, 72, 160)            # register-staged kernels: no slab, part of one, one, one and a part, two and a half


def tile_shapes(BM, BN):
    """(M, N) per tile class: whole tiles with tiles_m > tiles_n and with tiles_m < tiles_n (2 and 3 workgroups: no multiple of 8),
    ragged in both directions, N = 20 and N = BN + 4 (N % 8 != 0)"""
    return dict(whole=(2 * BM, BN), wide=(BM, 3 * BN), ragged=(BM + 1, BN + 8), n20=(BM + 1, 20), nbn4=(BM, BN + 4))


def xcd_shapes(BM, BN, whole=False):
    """10 workgroups (the XCD map is the identity below 9): 5 x 2 and 2 x 5 tiles, the second ragged unless `whole` (mm32)"""
    return [(5 * BM, 2 * BN), (2 * BM, 5 * BN) if whole else (2 * BM - 3, 5 * BN - 8)]


def dma_slabs(stages):
    return sorted({2, max(2, stages - 1), stages, stages + 1, 5, 12})        # (5: a ring of two has four lengths as well)


# the kernel classes of the GPU matrix: (value of the forcing switch, BM, BN, ring depth[, k2])
DMA_CLASSES = (("64s3", 64, 64, 3), ("64s4", 64, 64, 4), ("32", 32, 64, 4), ("ws2", 128, 64, 2), ("ws3", 128, 64, 3), ("ws4", 128, 64, 4),
               ("128s2", 128, 128, 2), ("128s3", 128, 128, 3), ("256s2", 256, 128, 2), ("256s3", 256, 128, 3))
DMA_CLASSES_F32 = ("64s3", "64s4", "128s2", "128s3")
MM32_CLASSES = (("128", 128, 128, 2, False), ("64", 128, 64, 3, False), ("264", 128, 64, 3, True), ("262", 128, 64, 2, True))


def k_list(kind, bf16, S):
    """reduction lengths of one instance: kind 'reg' (register-staged), 'dma', 'mm32', 'mm32k2'"""
    bk = 64 if bf16 else 32
    if kind == "reg":
        return list(REG_K)
    if kind == "mm32k2":                         # whole pairs of slabs, at least two pairs: 2, 3, 4, 5 and 12 slabs per wave group
        return [256, 384, 512, 640, 1536]
    return [s * bk for s in dma_slabs(S)]


def xcd_k(kind, bf16):
    return 72 if kind == "reg" else (384 if kind.startswith("mm32") else 3 * (64 if bf16 else 32))


def instance_shapes(kind, bf16, BM, BN, S):
    """every (M, N, K) test_instance and the XCD test launch for one instance"""
    sh, ks = tile_shapes(BM, BN), k_list(kind, bf16, S)
    mm32 = kind.startswith("mm32")
    keys = ("whole", "wide") if mm32 else tuple(sh)
    out = {(*sh[k], K) for k in keys for K in ks}
    return out | {(M, N, xcd_k(kind, bf16)) for M, N in xcd_shapes(BM, BN, mm32)}


GROUP_K = (128, 512, 256, 512, 128, 1024, 256, 192)              # the group launcher's stable sort by K changes this order


def group_members(BM, BN, whole, n):
    """(M, N) of the n problems of a group in tile class BM x BN: whole tiles only (mm32_group), or ragged rows, ragged columns and
    N % 8 != 0 among them (gemm_group; every member keeps M >= BM and N >= BN, which the forced 128- and 256-row classes require)"""
    if whole:
        return [((1 + i % 2) * BM, (1 + (i // 2) % 2) * BN) for i in range(n)]
    base = [(BM + 6, BN + 8), (BM, BN + 4), (2 * BM + 2, BN), (BM, BN), (BM + 1, 2 * BN + 8), (BM, 148), (BM + 64, BN + 8), (BM + 6, BN)]
    if BM == 64:
        base[1] = (64, 20)
    return base[:n]


def shape_matrix():
    """every (M, N, K, bf16) the GPU matrix launches, once (run_case and the group / batched tests refuse a shape that is not here)"""
    out = set()
    for bf16 in (True, False):
        for BM in (64, 128):
            out |= {(*x, bf16) for x in instance_shapes("reg", bf16, BM, BM, 0)}
        for t, BM, BN, S in DMA_CLASSES:
            if bf16 or t in DMA_CLASSES_F32:
                out |= {(*x, bf16) for x in instance_shapes("dma", bf16, BM, BN, S)}
    for _, BM, BN, S, k2 in MM32_CLASSES:
        out |= {(*x, True) for x in instance_shapes("mm32k2" if k2 else "mm32", True, BM, BN, S)}
    for bf16 in (True, False):
        # default dispatch, pad columns, epilogue matrix, batched products, split-K
        out |= {(65, 72, K, bf16) for K in (32, 40, 64, 72, 96, 128, 130, 136, 192, 256, 1000)}
        out |= {(65, 20, 128, bf16), (65, 68, 128, bf16), (65, 68, 192, bf16), (128, 128, 72, bf16), (128, 128, 256, bf16)}
        out |= {(70, N, K, bf16) for N in (40, 20) for K in (64, 128, 200)}
    out |= {(32, 64, 320, True), (31, 72, 256, True), (64, 64, 256, True)}
    out |= {(M, N, K, True) for M, N in ((136, 72), (64, 20)) for K in (512, 1024)}
    for BM, BN in ((64, 64), (128, 128), (256, 128)):
        for whole in (False, True):
            if whole and BM == 64:
                continue
            for (M, N), K in zip(group_members(BM, BN, whole, 8), GROUP_K):
                out |= {(M, N, K, True), (M, N, 256, True)}
    for (M, N), K in zip(group_members(64, 64, False, 8), GROUP_K):
        out |= {(M, N, K // 2, False), (M, N, 128, False)}
    out |= {(128, 64, 3072, True), (256, 128, 3072, True), (256, 128, 3072, False), (256, 64, 3072, True)}
    return sorted(out)


# ---- the instance lists (tests/test_gemm_kernels_gpu.py launches them, tests/test_gemm_dispatch_cpu.py asks etp_gemm_instance for them) ----
STOR = ((0, 0), (0, 1), (1, 1))                       # (trans_a, trans_b): NT, NN, TN


def tname(bf16):
    return "bf16" if bf16 else "f32"


def sname(ta, tb):
    return ("T" if ta else "N") + ("N" if tb else "T")


def inst(kind, bf16, c_bf16, ta, tb, BM, BN, S, k2=False):
    return f"{kind}<{tname(bf16)},{tname(c_bf16)},{sname(ta, tb)},{BM}x{BN},s{S}{',k2' if k2 else ''}>"


def c_of(ta, tb, bf16):
    """output dtype an instance is listed with: weight gradients (TN) of bf16 operands leave fp32, everything else the operand dtype"""
    return bf16 and not (ta and tb)


REG = [dict(name=inst("gemm", bf, cb, ta, tb, bm, bm, 0), opts={"GEMM_TILE": f"{bm}r", "MM32": "0"}, BM=bm, BN=bm, S=0, ta=ta, tb=tb,
            bf16=bf, c_bf16=cb, kind="reg")
       for bm in (64, 128) for bf, cb in ((True, True), (True, False), (False, False)) for ta, tb in STOR]
DMA = [dict(name=inst("gemm_dma", True, c_of(ta, tb, True), ta, tb, bm, bn, s), opts={"GEMM_TILE": t, "MM32": "0"}, BM=bm, BN=bn, S=s,
            ta=ta, tb=tb, bf16=True, c_bf16=c_of(ta, tb, True), kind="dma")
       for t, bm, bn, s in DMA_CLASSES for ta, tb in STOR if not (t == "32" and ta)]
DMA += [dict(name=inst("gemm_dma", False, False, ta, tb, bm, bn, s), opts={"GEMM_TILE": t, "MM32": "0"}, BM=bm, BN=bn, S=s, ta=ta, tb=tb,
             bf16=False, c_bf16=False, kind="dma")
        for t, bm, bn, s in DMA_CLASSES if t in DMA_CLASSES_F32 for ta, tb in STOR]
MM32 = [dict(name=inst("mm32", True, cb, ta, tb, bm, bn, s, k2), opts={"MM32": c}, BM=bm, BN=bn, S=s, ta=ta, tb=tb, bf16=True, c_bf16=cb,
             kind="mm32k2" if k2 else "mm32")
        for c, bm, bn, s, k2 in MM32_CLASSES for cb in (True, False) for ta, tb in STOR if not (k2 and ta)]
GROUP_CLASSES = [("64s3", 64, 64, 3), ("64s4", 64, 64, 4), ("128s2", 128, 128, 2), ("128s3", 128, 128, 3), ("256s2", 256, 128, 2),
                 ("256s3", 256, 128, 3)]
GROUPS = [dict(name=inst("gemm_group", True, False, 1, 1, bm, bn, s), opts={"GROUP_TILE": t, "MM32": "0"}, BM=bm, BN=bn, ta=1, tb=1,
               bf16=True, c_bf16=False) for t, bm, bn, s in GROUP_CLASSES]
GROUPS += [dict(name=inst("gemm_group", False, False, 1, 1, 64, 64, 3), opts={"GROUP_TILE": "64s3"}, BM=64, BN=64, ta=1, tb=1, bf16=False,
                c_bf16=False),
           dict(name=inst("gemm_group", True, True, 0, 0, 64, 64, 3), opts={"GROUP_TILE": "64s3", "MM32": "0"}, BM=64, BN=64, ta=0, tb=0,
                bf16=True, c_bf16=True)]
MM32_GROUPS = [dict(name=inst("mm32_group", True, False, 1, 1, 128, 128, 2), opts={"MM32": "128", "MM32_GROUP": "128"}, BM=128, BN=128,
                    ta=1, tb=1, bf16=True, c_bf16=False, whole=True),
               dict(name=inst("mm32_group", True, False, 1, 1, 256, 128, 3), opts={"MM32": "128", "MM32_GROUP": "256"}, BM=256, BN=128,
                    ta=1, tb=1, bf16=True, c_bf16=False, whole=True)]
SINGLES = REG + DMA + MM32
GEMM_SWITCHES = ("GEMM_TILE", "MM32", "MM32_GROUP", "GROUP_TILE", "GEMM_XCD", "MM32_K2", "GEMM_WIDE", "GEMM_SMALL")


# ---- dispatch records (tests/golden/gemm_dispatch.json; tools/record_gemm_dispatch.py writes them, test_gemm_dispatch_cpu.py reads them) --
def rup(x, m):
    return (x + m - 1) // m * m


def dispatch_rec(M, N, K, ta=0, tb=0, bf16=True, c_bf16=None, batch=1, ksplit=1, act=ACT_NONE, out_mode=0, bias=False, R=False, Z=False,
                 colsum=False, lda=None, ldb=None, ldc=None, ldr=None, ldz=None):
    """one product as a plain dict of descriptor fields (leading dimensions default to the chunk-rounded extents)"""
    epc = 8 if bf16 else 4
    return dict(M=M, N=N, K=K, ta=ta, tb=tb, bf16=bool(bf16), c_bf16=bool(bf16 if c_bf16 is None else c_bf16), batch=batch, ksplit=ksplit,
                act=act, out_mode=out_mode, bias=bool(bias), R=bool(R), Z=bool(Z), colsum=bool(colsum),
                lda=lda or (rup(M, epc) if ta else rup(K, epc)), ldb=ldb or (rup(N, epc) if tb else rup(K, epc)), ldc=ldc or N,
                ldr=(ldr or ldc or N) if R else 0, ldz=(ldz or ldc or N) if Z else 0)


def dispatch_pack(r):
    """the record without its zero / False fields (the fixture's form); dispatch_unpack restores them"""
    return {k: v for k, v in r.items() if v not in (0, False)}


def dispatch_unpack(p):
    return dict(dispatch_rec(1, 1, 0), ta=0, tb=0, bf16=False, c_bf16=False, batch=0, ksplit=0, M=0, N=0, lda=0, ldb=0, ldc=0) | p


def dispatch_extents(r):
    """elements each buffer of a record spans: A, B, C, R, Z (bias: N, a_colsum: M)"""
    nb = max(r["batch"], 1)
    a = (r["K"] if r["ta"] else r["M"]) * r["lda"]
    b = (r["K"] if r["tb"] else r["N"]) * r["ldb"]
    return dict(A=max(a, 1), B=max(b, 1), C=nb * r["M"] * r["ldc"], R=r["M"] * r["ldr"], Z=r["M"] * r["ldz"])


def dispatch_desc(d, r, ptr):
    """fill the GemmDesc `d` from record `r`; ptr(name) -> the address of that buffer (16-byte aligned, or whatever the caller means to test)"""
    d.A, d.B, d.C = ptr("A"), ptr("B"), ptr("C")
    d.M, d.N, d.K, d.lda, d.ldb, d.ldc = r["M"], r["N"], r["K"], r["lda"], r["ldb"], r["ldc"]
    d.trans_a, d.trans_b, d.dtype, d.c_dtype = r["ta"], r["tb"], 1 if r["bf16"] else 0, 1 if r["c_bf16"] else 0
    d.batch, d.batch_inner, d.ksplit, d.alpha = r["batch"], 1, r["ksplit"], 1.0
    d.sCo = r["M"] * r["ldc"] if r["batch"] > 1 else 0           # batched records: every entry on the same operands, its own C
    d.bias = ptr("bias") if r["bias"] else None
    d.R, d.ldr = (ptr("R"), r["ldr"]) if r["R"] else (None, 0)
    d.Z, d.ldz = (ptr("Z"), r["ldz"]) if r["Z"] else (None, 0)
    d.act, d.out_mode = r["act"], r["out_mode"]
    d.a_colsum = ptr("colsum") if r["colsum"] else None
    return d
