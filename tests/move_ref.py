"""fp64 restatements, case lists, launch geometry and derived bounds for the MLM loss tail and the data-movement kernels
(tests/test_move_kernels_gpu.py runs them through the C ABI, tests/test_move_ref_cpu.py pins and emulates them without a GPU):

  embed.hip  vocab_ce_kernel<T> (etp_vocab_ce), gelu_bwd_kernel<T> (etp_gelu_bwd), sum_steps_kernel<T> (etp_sum_steps),
             repeat_block_kernel (etp_repeat_block), copy_f32_kernel (etp_copy_f32), zero_f32_kernel (etp_memset_async, value 0),
             cast_drop_kernel<T> without dropout (etp_cast_f32_to), seq_mask_kernel (etp_seq_mask)
  graph.hip  vp_gather_kernel (etp_vp_gather)

Both test files take every case from the lists of this module and from nowhere else.

Bounds.  u = 2^-24, gam(k) = k u / (1 - k u) (tests/reduce_ref.py).  Nothing below is fitted to what a kernel returns.

  vocab_ce (vce_reference): reduce_ref.ce_bounds with this kernel's chain.  expf / logf within one ulp (2u relative); the row sum is
    ceil(V / 256) sequential adds per thread, the 6 levels of the wave butterfly and 3 adds over the four waves' LDS slots:
        e_sum = 2u + u max|s - mx| + gam(ceil(V / 256) + 6 + 3)              relative error of sum_k exp(s_k - mx)
        e_lse = e_sum + 2u |log sum| + u |lse|                               absolute error of lse
        dl    : |scale| (p (e_lse + u |s - lse| + 2u) + 2u |p - onehot| + 2^-126)
    2^-126: a subnormal intermediate may be flushed to zero (the cases keep p itself normal: vce_case).  A bf16 dl adds one bf16
    rounding of the reference value, half a bf16 ulp (round-to-nearest-even; if the fp32 value sits just across a power of two from
    the reference it rounds onto that power of two, so the reference's own binade gives the larger half ulp).
    The loss is start + sum over the rows in ANY order (one atomic per row):
        gam(Nm + 1) (|start| + sum_r |scale nll_r|) + |scale| sum_r e_lse_r
    The padding columns of dl and every -inf column are EXACTLY zero (asserted apart from the bound).
  gelu_bwd (gelu_bound): FP32_REL |d| -- the project's fp32 class of the erf / exp forms (row_ref.FP32_REL) on |gelu'| <= 1.13 --
    plus the bf16 rounding of the reference for bf16.  z = +-inf: x phi(x) is inf * 0, NaN in the reference, in torch and in
    the kernel; those elements are required to BE NaN and are left out of the bound.
  sum_steps (sum_bound): the accumulator starts at +0, so the first add is exact and steps - 1 roundings remain:
    gam(steps - 1) sum_t |src_t|, plus the bf16 rounding; steps = 1 is a bit-for-bit copy.
  repeat_block, copy_f32, zero_f32, cast_drop(p = 0), seq_mask, vp_gather: exact (same_bits); EXACT[key] counts differing elements.

Launch geometry (schedule): each data-movement kernel's index schedule -- vector body, grid-stride trips under the launcher's grid
cap, scalar tail -- is restated from the launcher and replayed on the CPU; every element must be written exactly once.

Comparators record the worst err / bound in WORST[(entry point, tensor)] and the differing elements of the exact kernels in EXACT.
"""
import torch

from tests import reduce_ref as rf
from tests.gemm_ref import gelu, gelu_grad  # noqa: F401  (gelu: the mutation tests' wrong derivative)
from tests.reduce_ref import F64, U, Guarded, bf16_rne, bf16_rne_bits, cast_specials, cdiv, ce, f32, gam, gptr  # noqa: F401
from tests.row_ref import FP32_REL, ulp_bf16

F32, BF16 = torch.float32, torch.bfloat16
TDT = {"fp32": F32, "bf16": BF16}
TINY = 2.0 ** -126            # smallest normal fp32
WORST, EXACT = {}, {}


# ---- comparators ---------------------------------------------------------------------------------------------------------------
def within(key, got, ref, bound):
    """reduce_ref.within, the worst ratio also kept in this module's table (recorded before the assertion)"""
    try:
        return rf.within(key, got, ref, bound)
    finally:
        WORST[key] = max(WORST.get(key, 0.0), rf.WORST.get(key, 0.0))


def _bytes(t):
    return t.contiguous().view(-1).view(torch.uint8)


def exact(key, got, want):
    """bit for bit, any dtype; EXACT[key] += the number of differing elements"""
    assert got.dtype == want.dtype and got.shape == want.shape, (key, got.dtype, want.dtype, tuple(got.shape), tuple(want.shape))
    size = got.element_size()
    diff = (_bytes(got) != _bytes(want)).view(-1, size).any(1) if got.numel() else torch.zeros(0, dtype=torch.bool)
    n = int(diff.sum())
    EXACT[key] = EXACT.get(key, 0) + n
    assert n == 0, f"{key}: {n} of {got.numel()} elements differ bitwise (first at {int(diff.nonzero()[0])})"


def table():
    rows = [f"  {'entry point':<40}{'tensor':<20}err/bound"]
    rows += [f"  {k[0]:<40}{k[1]:<20}{v:8.3f}" for k, v in sorted(WORST.items())]
    rows += ["", f"  {'exact entry point':<60}differing elements"]
    rows += [f"  {k:<60}{v:8d}" for k, v in sorted(EXACT.items())]
    return "\n".join(rows)


def half_ulp_bf16(ref):
    return 0.5 * ulp_bf16(ref)


# ---- output buffers: payload NaN (0xFF bytes) inside reduce_ref.Guarded ---------------------------------------------------------
def payload(shape, dtype, device="cpu"):
    """what an output holds before the call: a quiet NaN with a payload (fp32 0x7FC12345, bf16 0x7FD5), 0xFF for bytes"""
    if dtype == F32:
        return torch.full(shape, 0x7FC12345, dtype=torch.int32, device=device).view(F32)
    if dtype == BF16:
        return torch.full(shape, 0x7FD5, dtype=torch.int16, device=device).view(BF16)
    assert dtype == torch.uint8, dtype
    return torch.full(shape, 0xFF, dtype=torch.uint8, device=device)


def guarded(shape, dtype=F32, init=None, device="cuda"):
    shape = tuple(shape)
    return Guarded(shape, dtype, init=payload(shape, dtype, device) if init is None else init, device=device)


def guarded_i64(shape, device="cuda"):
    """int64 output as 0xFF bytes (every element -1) inside a guarded byte buffer -> (Guarded, int64 view)"""
    n = 1
    for s in shape:
        n *= s
    g = guarded((n * 8,), torch.uint8, device=device)
    return g, g.t.view(torch.int64).view(*shape)


# ---- launch geometry -----------------------------------------------------------------------------------------------------------
#            vector width, + 1 block, grid cap, scalar tail      (embed.hip launchers)
GEOMETRY = {"copy_f32": (4, True, 2048, True), "zero_f32": (4, True, 4096, True), "cast_drop": (4, False, 4096, False),
            "sum_steps": (4, False, 4096, False), "repeat_block": (1, False, 4096, False), "gelu_bwd": (1, False, 2048, False)}


def schedule(kernel, n):
    """replay the kernel's index schedule over n elements (repeat_block: n 16-byte vectors)
    -> (writes per element [n] int32, blocks, trips of the vector body, tail length)"""
    vec, plus_one, cap, tail = GEOMETRY[kernel]
    nv = n // vec
    blocks = min(cdiv(nv, 256) + (1 if plus_one else 0), cap)
    count = torch.zeros(n, dtype=torch.int32)
    if n == 0:
        return count, 0, 0, 0
    threads = blocks * 256
    trips = cdiv(nv, threads)
    for k in range(trips):
        ids = k * threads + torch.arange(threads)
        ids = ids[ids < nv]
        for e in range(vec):
            count[ids * vec + e] += 1
    ntail = n - nv * vec if tail else 0
    if tail:
        i = nv * vec + torch.arange(threads)
        while bool((i < n).any()):
            count[i[i < n]] += 1
            i = i + threads
    return count, blocks, trips, ntail


# ---- vocab_ce ------------------------------------------------------------------------------------------------------------------
VCE_V = (1, 2, 63, 255, 256, 257, 1000, 30522)
VCE_NM, VCE_NM_BIG = (1, 3, 77, 300), (1, 5)
VCE_DOM = 60.0                # the dominating column: e^-60 / Nm stays a normal fp32
VCE_PAD = 3e38                # what the logits' padding columns hold: finite, so a read of the padding moves max and sum (fmaxf drops a NaN)
VCE_PATTERNS = [(sh, sk, st) for sh in (0.0, 80.0, -80.0, "dom") for sk in ("mean", "fixed") for st in (0.0, 3.25)]


def round_up(a, b):
    return cdiv(a, b) * b


def vce_cases():
    """(dtype name, V, ldv, Nm, (shift | 'dom', scale kind, loss start))"""
    out = []
    for V in VCE_V:
        for ldv in (round_up(V, 8), V + 16):
            for Nm in (VCE_NM_BIG if V == 30522 else VCE_NM):
                for dt in ("fp32", "bf16"):
                    i = len(out)
                    out.append((dt, V, ldv, Nm, VCE_PATTERNS[(7 * i + i // 16) % len(VCE_PATTERNS)]))
    return out


def vce_case(V, ldv, Nm, pattern, seed, device="cpu"):
    """logits [Nm, ldv] fp32 with VCE_PAD in columns >= V; labels at column 0 (first row), V - 1 (last row) and the row's argmax
    (middle row; a single row takes one of the three by seed); at least one -inf column per row when V > 2, never the label's."""
    shift, sk, start = pattern
    g = torch.Generator().manual_seed(seed)
    s = torch.randn(Nm, V, generator=g) * 3
    if shift == "dom":
        s[torch.arange(Nm), torch.randint(0, V, (Nm,), generator=g)] += VCE_DOM
    else:
        s = s + shift
    labels = torch.randint(0, V, (Nm,), generator=g)
    labels[0] = 0
    labels[-1] = V - 1
    if Nm == 1:
        labels[0] = (0, V - 1, 0)[seed % 3]
    rows = torch.arange(Nm)
    mid = Nm // 2 if Nm >= 3 else (0 if seed % 3 == 2 else None)
    if V > 2:
        col = torch.rand(Nm, V, generator=g) < 0.2
        col[rows, (labels + 1) % V] = True
        col[rows, labels] = False
        if mid is not None:
            am = int(torch.where(col[mid], torch.full_like(s[mid], float("-inf")), s[mid]).argmax())
            labels[mid] = am
            col[mid, (am + 1) % V] = True
        s[col] = float("-inf")
    elif mid is not None:
        labels[mid] = int(s[mid].argmax())
    buf = torch.full((Nm, ldv), VCE_PAD)
    buf[:, :V] = s
    scale = f32(1.0 / Nm) if sk == "mean" else f32(0.37)
    return {"V": V, "ldv": ldv, "Nm": Nm, "buf": buf.to(device), "labels": labels.to(device), "scale": scale, "start": float(start)}


def vce_reference(c, bf16):
    """-> c with the fp64 loss / dlogits ([Nm, ldv], zero padding) and their bounds"""
    V, ldv, Nm, scale, start = c["V"], c["ldv"], c["Nm"], c["scale"], c["start"]
    logits = c["buf"][:, :V]
    rl, rd, q = ce(logits, c["labels"], scale, -100)              # -100 names no row: labels are in [0, V)
    s, lse, mx, sm = q["s"], q["lse"], q["mx"], q["sum"]
    fin = torch.isfinite(s)
    span = torch.where(fin, (s - mx).abs(), torch.zeros_like(s)).max(-1, keepdim=True).values
    e_sum = (2 * U + U * span) + gam(cdiv(V, 256) + 6 + 3)
    e_lse = e_sum + 2 * U * torch.log(sm).abs() + U * lse.abs()
    sl = torch.where(fin, (s - lse).abs(), torch.zeros_like(s))
    bdl = abs(scale) * (q["p"] * (e_lse + U * sl + 2 * U) + 2 * U * (q["p"] - q["onehot"]).abs() + TINY)
    if bf16:
        bdl = bdl + half_ulp_bf16(rd)
    dl = torch.zeros(Nm, ldv, dtype=F64, device=s.device)
    bd = torch.zeros_like(dl)
    dl[:, :V], bd[:, :V] = rd, bdl
    terms = scale * q["nll"]
    c.update(loss=start + rl, dl=dl, bdl=bd, neginf=torch.isneginf(logits), q=q, terms=terms,
             bloss=gam(Nm + 1) * (abs(start) + terms.abs().sum()) + abs(scale) * e_lse.sum())
    return c


def check_vce(name, c, loss, dl):
    """loss: what *loss holds after the call (start + sum); dl [Nm, ldv] in the operand dtype"""
    V = c["V"]
    pad = dl[:, V:].float()
    assert bool((pad == 0).all()), f"{name}: {int((pad != 0).sum())} padding elements of dlogits are not zero"
    assert bool((dl[:, :V].float()[c["neginf"]] == 0).all()), f"{name}: dlogits non-zero in a -inf column"
    within((name, "dlogits"), dl, c["dl"], c["bdl"])
    within((name, "loss"), loss.reshape(()), c["loss"].reshape(()), c["bloss"].reshape(()))


def emulate_vce(c, dtype):
    """fp32 emulation of vocab_ce_kernel: 256 strided threads, the wave butterfly, ((r0 + r1) + r2) + r3 over the LDS slots; the
    rows' atomics are applied in reverse row order onto the start value"""
    V, ldv, Nm = c["V"], c["ldv"], c["Nm"]
    s = c["buf"][:, :V].to(F32)
    sc = torch.tensor(c["scale"], dtype=F32)
    mx = s.max(-1, keepdim=True).values
    J = cdiv(V, 256)
    e = torch.cat([torch.exp(s - mx), torch.zeros(Nm, J * 256 - V, dtype=F32)], 1).reshape(Nm, J, 256)
    acc = torch.zeros(Nm, 256, dtype=F32)
    for j in range(J):
        acc = acc + e[:, j]
    w = rf._wave_sum32(acc.reshape(Nm * 4, 64)).reshape(Nm, 4)
    lse = mx + torch.log((((w[:, 0] + w[:, 1]) + w[:, 2]) + w[:, 3])[:, None])
    y = c["labels"]
    onehot = torch.zeros_like(s).scatter_(1, y[:, None], 1.0)
    dl = torch.zeros(Nm, ldv, dtype=F32)
    dl[:, :V] = sc * (torch.exp(s - lse) - onehot)
    terms = sc * (lse.squeeze(1) - s.gather(1, y[:, None]).squeeze(1))
    loss = torch.tensor(c["start"], dtype=F32)
    for r in reversed(range(Nm)):
        loss = loss + terms[r]
    return loss, dl.to(dtype)


# ---- gelu_bwd ------------------------------------------------------------------------------------------------------------------
GELU_GRID = 2048
GELU_N = (1, 255, 256, 257, GELU_GRID * 256 + 1029)          # the last: 1029 elements in the second trip of the 2048-block grid
GELU_ZERO = -0.7517915246936                                    # gelu'(x) = 0
GELU_SPECIALS = (GELU_ZERO, 0.0, float("inf"), float("-inf"), 10.0, -10.0, -0.75, 0.75)


def gelu_cases():
    return [(dt, n) for n in GELU_N for dt in ("fp32", "bf16")]


def gelu_case(n, dtype, seed, device="cpu"):
    """z in [-10, 10] with GELU_SPECIALS at the front and again over the last elements (the second trip where there is one); a single
    element walks through the specials by seed.  -> d, z in `dtype`"""
    g = torch.Generator().manual_seed(seed)
    z = torch.rand(n, generator=g) * 20 - 10
    sp = torch.tensor(GELU_SPECIALS)
    if n < sp.numel():
        z[:] = sp[torch.arange(seed, seed + n) % sp.numel()]
    else:
        z[:sp.numel()] = sp
        z[-sp.numel():] = sp
    d = torch.randn(n, generator=g) * 2.0 ** torch.randint(-6, 7, (n,), generator=g).float()
    return d.to(dtype).to(device), z.to(dtype).to(device)


def gelu_bwd(d, z):
    return d.to(F64) * gelu_grad(z.to(F64))


def gelu_bound(d, ref, bf16):
    b = FP32_REL * d.to(F64).abs()
    return b + half_ulp_bf16(torch.nan_to_num(ref)) if bf16 else b


def check_gelu(name, got, d, z):
    """d, z: the operands as stored before the call"""
    ref = gelu_bwd(d, z)
    nan = torch.isinf(z.float()) & (d.float() == d.float())
    assert bool(torch.isnan(ref[nan]).all()) and bool(torch.isfinite(ref[~nan]).all())
    assert bool(torch.isnan(got.float()[nan]).all()), f"{name}: z = +-inf did not give NaN (inf * 0)"
    zero = torch.zeros_like(ref)
    bound = gelu_bound(d, ref, got.dtype == BF16)
    within((name, "d"), torch.where(nan, zero, got.to(F64)), torch.where(nan, zero, ref), torch.where(nan, zero, bound))


def emulate_gelu(d, z):
    x, dd = z.to(F32), d.to(F32)
    cdf = 0.5 * (1.0 + torch.erf(x * 0.70710678118654752))
    pdf = 0.39894228040143268 * torch.exp(-0.5 * x * x)
    return (dd * (cdf + x * pdf)).to(d.dtype)


# ---- sum_steps -----------------------------------------------------------------------------------------------------------------
SUM_BIG = 4 * (4096 * 256) + 1028                             # 257 float4s in the second trip of the 4096-block grid
SUM_N = (4, 1028, SUM_BIG)
SUM_STEPS = (1, 2, 5, 25)


def sum_cases():
    return [(dt, n, st) for n in SUM_N for st in SUM_STEPS for dt in ("fp32", "bf16") if not (st == 25 and n == SUM_BIG)]


def sum_case(n, steps, dtype, seed, device="cpu"):
    """src [steps, n] in `dtype`: per-element scales 2^-8 .. 2^4; with more than one step every third element's last term is minus the
    sum of the others, up to 2^-10 of it: the sum nearly cancels"""
    g = torch.Generator().manual_seed(seed)
    src = torch.randn(steps, n, generator=g) * 2.0 ** torch.randint(-8, 5, (n,), generator=g).float()
    src = src.to(dtype)
    if steps > 1:
        part = src[:-1, ::3].to(F64).sum(0)
        src[-1, ::3] = (-part * (1.0 + 2.0 ** -10)).to(dtype)
    return src.to(device)


def sum_steps(src):
    return src.to(F64).sum(0)


def sum_bound(src, ref, bf16):
    b = gam(src.shape[0] - 1) * src.to(F64).abs().sum(0)
    return b + half_ulp_bf16(ref) if bf16 else b


def check_sum(name, got, src):
    ref = sum_steps(src)
    if src.shape[0] == 1:
        exact(f"{name} (steps = 1: a copy)", got, src[0])
    within((name, "dst"), got, ref, sum_bound(src, ref, got.dtype == BF16))


def emulate_sum(src):
    a = torch.zeros(src.shape[1], dtype=F32)
    for t in range(src.shape[0]):
        a = a + src[t].to(F32)
    return a.to(src.dtype)


# ---- the exact kernels ---------------------------------------------------------------------------------------------------------
REPEAT_BYTES = (16, 48, 16 * 1027, 16 * (4096 * 256 + 5))     # the last: 5 vectors in the second trip
REPEAT_T = (1, 2, 5)
COPY_N = (1, 3, 4, 5, 1027, 4 * (2048 * 256) + 1027)          # tails of 1, 3, 0, 1, 3, 3; the last: a second trip of the 2048-block grid
ZERO_N = (0, 1, 3, 4, 5, 1027, 4 * (4096 * 256) + 1031)
CASTTO_N = (4, 8, 1028, 4 * (4096 * 256) + 1028)
SEQ_SHAPES = ((1, 1), (3, 12), (7, 37), (32, 36))


def random_bytes(n, seed, device="cpu"):
    return torch.randint(0, 256, (n,), generator=torch.Generator().manual_seed(seed), dtype=torch.uint8).to(device)


def random_f32(n, seed, device="cpu"):
    """random values with the cast's special values at both ends where they fit"""
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(n, generator=g) * 2.0 ** torch.randint(-20, 20, (n,), generator=g).float()
    sp = cast_specials()
    k = min(n, sp.numel())
    x[:k] = sp[:k] if n > 9 else sp[n:n + k]
    if n > 100:
        x[-sp.numel():] = sp
    return x.to(device)


def repeat_block(src, T):
    return src.repeat(T)


def check_cast_to(name, got, src):
    if got.dtype == F32:
        exact(name + " fp32", got, src)
        return
    nan = torch.isnan(src)
    assert bool(torch.isnan(got.float()[nan]).all()), f"{name}: a NaN did not stay NaN"
    exact(name + " bf16", torch.where(nan, torch.zeros_like(got), got), torch.where(nan, torch.zeros_like(got), bf16_rne(src)))


def seq_lens(B, V, seed):
    """int64 [B]: 0, 1, V - 1, V, V + 5 first, random in [0, V + 5] after them"""
    g = torch.Generator().manual_seed(seed)
    lens = torch.randint(0, V + 6, (B,), generator=g)
    edge = torch.tensor([0, 1, V - 1, V, V + 5])
    k = min(B, edge.numel())
    lens[:k] = edge[torch.arange(seed, seed + k) % edge.numel()] if B < edge.numel() else edge
    return lens


def seq_mask(lens, V):
    return (torch.arange(V, device=lens.device)[None, :] < lens[:, None]).to(torch.uint8)


# ---- vp_gather -----------------------------------------------------------------------------------------------------------------
VP_B, VP_P, VP_F = (1, 3), (12, 36), (7, 128, 300, 2048)
VP_K = {1: ((0,), (1,), ("P",)), 3: ((0, 1, "P"), ("P", 0, 1), (1, 1, 0), (0, 0, 0))}
VP_MASKS = ("none", "some", "all")


def vp_cases():
    """(B, P, F, K per episode, mask kind, V - largest length, shared panorama table?, nav_types / view_lens passed?)"""
    out = []
    for B in VP_B:
        for P in VP_P:
            for F in VP_F:
                for j in range(3):
                    i = len(out)
                    ks = tuple(P if k == "P" else k for k in VP_K[B][(i + i // 3) % len(VP_K[B])])
                    out.append((B, P, F, ks, VP_MASKS[j], (0, 3)[(i // 2) % 2], bool((i // 4 + j) % 2), i % 5 != 3))
    return out


def vp_case(case, seed, device="cpu"):
    B, P, F, ks, kind, vpad, shared, _ = case
    g = torch.Generator().manual_seed(seed)
    mask = torch.zeros(B, P, dtype=torch.uint8)
    for b in range(B):
        if kind == "all" or (kind == "some" and B > 1 and b == B - 1 and seed % 2):
            mask[b] = 1
        elif kind == "some":
            mask[b] = (torch.rand(P, generator=g) < 0.35).to(torch.uint8)
            mask[b, 0] = 1
            mask[b, P - 1] = b % 2
            mask[b, 1] = 0
    cand_ptr = torch.zeros(B + 1, dtype=torch.int32)
    cand_ptr[1:] = torch.cumsum(torch.tensor(ks), 0)
    total = int(cand_ptr[-1])
    cand = torch.randn(total, F, generator=g) if total else None
    pano = torch.randn(P, F, generator=g) if shared else torch.randn(B, P, F, generator=g)
    lens = [k + P - int(mask[b].sum()) for b, k in enumerate(ks)]
    V = max(1, max(lens)) + vpad
    mv = lambda t: None if t is None else t.to(device)
    return {"cand": mv(cand), "cand_ptr": mv(cand_ptr), "pano": mv(pano), "mask": mv(mask), "B": B, "P": P, "F": F, "V": V,
            "stride": 0 if shared else P * F, "lens": lens}


def vp_gather(cand, cand_ptr, pano, mask, V):
    """RLTrainer._vp_feature_variable's ordering, restated: per episode the candidate rows, then the panorama views whose mask byte is
    zero in index order, then zero rows up to V.  pano [B, P, F] or a shared [P, F].  -> out [B, V, F], nav_types [B, V], view_lens [B]"""
    B, P = mask.shape
    F = pano.shape[-1]
    out = torch.zeros(B, V, F, dtype=pano.dtype, device=pano.device)
    nav = torch.zeros(B, V, dtype=torch.int64, device=pano.device)
    lens = torch.zeros(B, dtype=torch.int64, device=pano.device)
    for b in range(B):
        lo, hi = int(cand_ptr[b]), int(cand_ptr[b + 1])
        free = (mask[b] == 0).nonzero().squeeze(1)
        table = pano if pano.dim() == 2 else pano[b]
        rows = table[free] if hi == lo else torch.cat([cand[lo:hi], table[free]], 0)
        n = rows.shape[0]
        assert n <= V, "the contract of include/etpnav_hip.h: V >= K + free views"
        out[b, :n] = rows
        nav[b, :hi - lo] = 1
        lens[b] = n
    return out, nav, lens


def vp_from_obs(obs, cand_key, pano_key):
    """the host side of graph_inputs.vp_feature_variable for one feature: -> cand, cand_ptr, pano, mask, V"""
    B, P = len(obs["cand_rgb"]), obs["pano_rgb"].shape[1]
    ks = [int(x.shape[0]) for x in obs["cand_rgb"]]
    cand_ptr = torch.zeros(B + 1, dtype=torch.int32)
    cand_ptr[1:] = torch.cumsum(torch.tensor(ks), 0)
    mask = torch.zeros(B, P, dtype=torch.uint8)
    for i in range(B):
        mask[i, torch.as_tensor(obs["cand_img_idxes"][i]).long()] = 1
    V = max(k + P - int(mask[i].sum()) for i, k in enumerate(ks))
    cand = torch.cat([torch.as_tensor(x, dtype=F32) for x in obs[cand_key]], 0)
    return cand, cand_ptr, torch.as_tensor(obs[pano_key], dtype=F32), mask, V


def check_vp(name, out, nav, lens, want):
    exact(name + " out_fts", out, want[0])
    if nav is not None:
        exact(name + " nav_types", nav, want[1])
        exact(name + " view_lens", lens, want[2])
