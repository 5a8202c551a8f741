"""The dropout sites of the kernels at operator level: a numpy restatement of the mask generator, fp64 restatements WITH dropout of
every operator that carries a site, their bounds, the case lists of the GPU files and the planted mistakes of the CPU file.

  tests/test_drop_ref_cpu.py      pins the generator bit for bit (oracle DropSpec.mult, the library's etp_dropout_multipliers) and
                                  the restatements to the oracle blocks that take `drop` (1e-12)
  tests/test_drop_bounds_cpu.py   every planted mistake is rejected on every case shape below; fp32 / bf16 emulations pass
  tests/test_drop_rows_gpu.py     text / panorama embedding, SAP tail, ln_bwd_s, cast_drop through the `_drop` entry points
  tests/test_drop_gemm_gpu.py     the GEMM epilogue's three masked compositions through etp_gemm_drop      (section "GEMM epilogue")
  tests/test_drop_attn_gpu.py     the four attention families through etp_attn_*_drop                      (section "attention")

The generator (csrc/common.h).  site seed = drop_hash(f(step seed), g(mode << 16 | layer << 4 | slot)); the multiplier of element i is
decided by ONE 32-bit word per PAIR of elements, w = drop_pair(site seed, i >> 1): element 2j reads the low 16 bits, 2j + 1 the high
16 bits; keep <=> bits >= round(p * 65536); a kept element is scaled by the fp32 value 1.0f / (1.0f - p).  Indices are 32-bit.

Index conventions (include/etpnav_hip.h beside etp_drop_site):
  row kernels   row * H + col     text / panorama embedding: y and dy; SAP tail: the normalised row n, forward and twice backward;
                                  ln_bwd_s: the operand copy dx_lp only
  cast_drop     the flat index
  GEMM          row * N + col of the M x N product, never ldc
  attention     ((b * heads + h) * Lq + q) * Lk + key on the probabilities, never ldS

Where the mask sits, and how a reference takes it.  Every one of these kernels forms `value * multiplier` as ONE fp32 multiply:
  forward (text, panorama: y = LN(...) * m)   reference y64 * m; bound = (existing bound of y) * m * (1 + u) + u |y64 * m|: the
                                              existing bound scaled like its value, plus the multiply's one rounding
  backward (text, panorama: dy * m first)     the reference's dy operand is RNE32(dy * m): the product exactly as IEEE fp32 forms it
                                              (both factors are fp32 inputs), so the multiply's rounding is in the operand and the
                                              existing bounds are used as they stand, on the dropped operand
  SAP tail                                    n = LN(r) * m inside (sap_fwd / sap_bwd below, written out by hand so that the
                                              backward's two applications can be told apart); row_ref's comparators
  ln_bwd_s                                    dx_lp = RNE(dx * m) of the kernel's OWN dx, bit for bit; dx, dgamma, dbeta: the
                                              undropped reference and bounds of reduce_ref
  cast_drop                                   dst = RNE(src * m), bit for bit
No bound carries a multiplier and none comes from a GPU run.

Mask read-out.  Where an output is elementwise in the mask (y, dst, dx_lp) its exact zeros must be {i: m(i) == 0}.  That needs
every undropped reference value to exceed its own bound (a kept element can then not read as zero): `readable` asserts it on the
reference alone, and the case builders walk a fixed list of seeds until it holds.  Where it is not (the backward sums over rows),
one-hot probes at M <= 8 make it so: one row of dy / dlogits at a time, zero previous gradients, and dbeta (text, panorama: sum of
dy * m), dw2 (SAP: dl * n * m) and dbeta (SAP: dl * w2 * m, the second application) show one row of the mask each.

Planted mistakes (MASK_MISTAKES, ATTN_MASKS, the `place` of gemm_ref, m_b of attn_ref).  Each is a wrong mask or a wrong placement; tests/test_drop_bounds_cpu.py builds what a kernel with
that mistake would return (the fp64 reference of the wrong formula, rounded to the output dtype) and requires the comparators to
reject it.  A mistake that names the same multiplier for every element of a shape IS the right code at that shape (row and column
swapped at M = 1; there is no leading dimension and no odd-start run in a row kernel): the CPU file asserts that identity instead,
and the mistake is rejected at every other shape.
"""
import numpy as np
import torch

from oracle import planner_oracle as po
from tests import move_ref as mv
from tests import reduce_ref as rf
from tests import row_ref as rr

F64, F32, BF16 = torch.float64, torch.float32, torch.bfloat16
U = rf.U
TDT = {"fp32": F32, "bf16": BF16}
RATES = (0.1, 0.4)
P_TINY = 1e-6                 # threshold round(p * 65536) = 0: nothing is dropped, everything is scaled by 1 / (1 - p)
SEED = 0x1234_5678_9ABC_DEF1
# (mode, layer, slot): the text embedding's own site and one with every field nonzero
SITES = ((po.MODE_TXT, 0, po.SITE_EMBED), (po.MODE_NAV, 3, po.SITE_HEAD))
WORST = {}


# ---- the generator -------------------------------------------------------------------------------------------------------------
def _u32(x):
    return np.asarray(x, dtype=np.uint64).astype(np.uint32) if not isinstance(x, np.ndarray) else (x.astype(np.uint64) & np.uint64(0xFFFFFFFF)).astype(np.uint32)


def _pair(seed, pair):
    """drop_pair: the word shared by elements 2 * pair and 2 * pair + 1"""
    with np.errstate(over="ignore"):
        x = _u32(pair) * np.uint32(0x9E3779B1) + np.uint32(seed)
        x ^= x >> np.uint32(16); x *= np.uint32(0x85EBCA6B); x ^= x >> np.uint32(13); x *= np.uint32(0xC2B2AE35); x ^= x >> np.uint32(16)
    return x


def _hash(seed, idx):
    """drop_hash: the site-seed mixer"""
    with np.errstate(over="ignore"):
        seed = np.uint32(seed)
        x = _pair(seed, idx)
        x += np.full_like(x, seed) * np.uint32(0x27D4EB2F); x ^= x >> np.uint32(15); x *= np.uint32(0x2C1B3C6D); x ^= x >> np.uint32(12)
    return x


def site_seed(seed, mode, layer, slot):
    """drop_site: the 32-bit seed of site (mode, layer, slot) under the 64-bit step seed"""
    s = int(seed) & 0xFFFFFFFFFFFFFFFF
    with np.errstate(over="ignore"):
        a = np.array([(s ^ (s >> 32)) & 0xFFFFFFFF], dtype=np.uint32) * np.uint32(0x9E3779B1) + np.uint32(0x7F4A7C15)
        b = np.array([(mode << 16) | (layer << 4) | slot], dtype=np.uint32) * np.uint32(0x632BE5AB) + np.uint32(17)
    return int(_hash(a[0], b)[0])


def threshold(p):
    return np.uint32(int(np.float32(p) * np.float32(65536.0) + np.float32(0.5)))


def inv_keep(p):
    return np.float32(1.0) / (np.float32(1.0) - np.float32(p))


def keep_at(p, sseed, idx, swap_halves=False):
    """bool array: element idx (any shape, taken modulo 2^32) of the site with seed `sseed` is kept"""
    idx = _u32(np.asarray(idx))
    w = _pair(sseed, idx >> np.uint32(1))
    odd = (idx & np.uint32(1)) != 0
    if swap_halves:
        odd = ~odd
    return np.where(odd, w >> np.uint32(16), w & np.uint32(0xFFFF)) >= threshold(p)


def mult_at(p, sseed, idx, swap_halves=False, scale=True):
    """fp32 multipliers (0 or 1.0f / (1.0f - p)) of the elements `idx`"""
    k = keep_at(p, sseed, idx, swap_halves)
    return np.where(k, inv_keep(p) if scale else np.float32(1.0), np.float32(0.0)).astype(np.float32)


def mult(p, seed, mode, layer, slot, n):
    """the library's etp_dropout_multipliers: elements 0 .. n - 1"""
    if p <= 0.0:
        return np.ones(n, dtype=np.float32)
    return mult_at(p, site_seed(seed, mode, layer, slot), np.arange(n, dtype=np.uint64))


def mult_runs(p, sseed, starts, N, odd_as_even=False):
    """drop_mult_run<N>: [..., N] multipliers of the runs starting at `starts`, branch by branch as common.h has them.
    odd_as_even: the planted mistake -- an odd start walks the even branch (pairs counted from the run's start)."""
    starts = _u32(np.asarray(starts))
    thr, inv = threshold(p), inv_keep(p)
    q0 = starts >> np.uint32(1)
    even = np.empty(starts.shape + (N,), dtype=bool)
    odd = np.empty(starts.shape + (N,), dtype=bool)
    for j in range(N // 2):
        w = _pair(sseed, q0 + np.uint32(j))
        even[..., 2 * j] = (w & np.uint32(0xFFFF)) >= thr
        even[..., 2 * j + 1] = (w >> np.uint32(16)) >= thr
    odd[..., 0] = (_pair(sseed, q0) >> np.uint32(16)) >= thr
    for j in range(1, N // 2 + 1):
        w = _pair(sseed, q0 + np.uint32(j))
        odd[..., 2 * j - 1] = (w & np.uint32(0xFFFF)) >= thr
        if 2 * j < N:
            odd[..., 2 * j] = (w >> np.uint32(16)) >= thr
    is_even = ((starts & np.uint32(1)) == 0)[..., None]
    k = even if odd_as_even else np.where(is_even, even, odd)
    return np.where(k, inv, np.float32(0.0)).astype(np.float32)


class Site:
    """one dropout site of a test: rate, step seed, (mode, layer, slot)"""

    def __init__(self, p, triple, seed=SEED):
        self.p, self.seed, (self.mode, self.layer, self.slot) = float(p), int(seed), triple

    @property
    def sseed(self):
        return site_seed(self.seed, self.mode, self.layer, self.slot)

    def spec(self, p_name="p_hidden"):
        """the oracle's DropSpec with this rate under `p_name` and every other rate 0"""
        d = po.DropSpec(0.0, 0.0, 0.0, 0.0, self.seed)
        setattr(d, p_name, self.p)
        return d

    def other_slot(self):
        return Site(self.p, (self.mode, self.layer, (self.slot + 1) % 16), self.seed)

    def other_site(self):
        return Site(self.p, SITES[1] if (self.mode, self.layer, self.slot) == SITES[0] else SITES[0], self.seed)

    def rows(self, M, H, mistake=None, device="cpu", ld=None):
        """fp32 [M, H] multipliers at index row * H + col -- or what a kernel with the planted mistake `mistake` would use
        (ld: the leading dimension of the mistake "ld", index row * ld + col)"""
        if self.p <= 0.0:
            return torch.ones(M, H, dtype=F32, device=device)
        r, c = np.arange(M, dtype=np.uint64)[:, None], np.arange(H, dtype=np.uint64)[None, :]
        idx, site, kw = r * np.uint64(H) + c, self, {}
        if mistake == "shift":
            idx = idx + np.uint64(1)
        elif mistake == "swap_rc":
            idx = c * np.uint64(M) + r
        elif mistake == "ld":
            idx = r * np.uint64(ld) + c
        elif mistake == "swap_halves":
            kw["swap_halves"] = True
        elif mistake == "other_slot":
            site = self.other_slot()
        elif mistake == "other_site":
            site = self.other_site()
        elif mistake == "no_inv_keep":
            kw["scale"] = False
        elif mistake == "none":
            return torch.ones(M, H, dtype=F32, device=device)
        else:
            assert mistake is None, mistake
        return torch.from_numpy(mult_at(self.p, site.sseed, idx, **kw)).to(device)

    def flat(self, n, mistake=None, device="cpu"):
        return self.rows(1, n, mistake, device).reshape(n)


# the wrong masks a row / cast kernel could use (Site.rows); placement mistakes are named by the builders below
MASK_MISTAKES = ("shift", "swap_rc", "swap_halves", "other_slot", "no_inv_keep")


def rne32(x64):
    """fp64 -> the fp32 value an IEEE multiply of two fp32 factors stores (the product of two fp32 values is exact in fp64)"""
    return x64.to(F32)


def record(key, ratio):
    WORST[key] = max(WORST.get(key, 0.0), float(ratio))


def within(key, got, ref, bound):
    try:
        return rf.within(key, got, ref, bound)
    finally:
        record(key, rf.WORST.get(key, 0.0))


def readable(what, ref, bound):
    """the read-out precondition, on the reference alone: every undropped value exceeds its own bound"""
    short = ref.detach().to(F64).abs() <= bound
    return not bool(short.any()), f"{what}: {int(short.sum())} undropped reference values do not exceed their bound"


def zero_set(what, got, m):
    """exact: got == 0 exactly where the multiplier is 0; every element is compared"""
    z, want = (got.detach().to(F64) == 0), (m.to(got.device) == 0)
    assert z.shape == want.shape, (what, tuple(z.shape), tuple(want.shape))
    bad = z != want
    assert not bool(bad.any()), (f"{what}: {int(bad.sum())} of {bad.numel()} elements are zero where the mask keeps them or nonzero "
                                 f"where it drops them (first at {int(bad.reshape(-1).nonzero()[0])})")


def scaled_bound(ref_plain, bound_plain, m):
    """bound of ref_plain * m formed by one fp32 multiply from a value within bound_plain of ref_plain"""
    m = m.to(F64)
    return bound_plain * m * (1.0 + U) + U * (ref_plain * m).abs()


# ---- case lists (the GPU file takes its cases from here; the CPU file walks the same lists) ------------------------------------------
TEXT_H = (256, 768)
TEXT_SHAPES = ((1, 7), (3, 9), (5, 24))
PANO_M = (1, 37, 385)
SAP_M = (1, 5, 77)
LN_M = (1, 5, 513)
CAST_N = (4, 1028, 4 * 4096 * 256 + 1028)
PROBE_ROWS = 8                # one-hot probes run where the case has at most this many rows
SEED_WALK = 16                # seeds tried for the read-out precondition


def _cycle(i):
    """(rate, site triple) of case i: both rates and both triples in either dtype"""
    return RATES[i % 2], SITES[(i // 2) % 2]


def text_cases():
    """(dtype name of y_lp, H, B, L, p, site triple)"""
    out = []
    for dt in ("fp32", "bf16"):
        for H in TEXT_H:
            for (B, L) in TEXT_SHAPES:
                out.append((dt, H, B, L) + _cycle(len(out) + (dt == "bf16")))
    return out


def pano_cases():
    """(operand dtype name, H, M, depth?, p, site triple)"""
    out = []
    for dt in ("fp32", "bf16"):
        for M in PANO_M:
            for depth in (True, False):
                out.append((dt, 256 if (M == 37 and not depth) else 768, M, depth) + _cycle(len(out) + (dt == "bf16")))
    return out


def sap_cases():
    """(operand dtype name, H, M, mask pattern, p, site triple)"""
    out = []
    for dt in ("fp32", "bf16"):
        for M, pat in zip(SAP_M, ("null", "none", "both")):
            out.append((dt, 256 if M == 5 else 768, M, pat) + _cycle(len(out) + (dt == "bf16")))
    return out


def ln_cases():
    """(dtype name of dx_lp, H, M, slab mode?, add?, p, site triple)"""
    out = []
    for dt in ("fp32", "bf16"):
        for M in LN_M:
            for slabs in (False, True):
                i = len(out)
                out.append((dt, (768, 256, 512, 1024)[i % 4], M, slabs, i % 3 != 1) + _cycle(i + (dt == "bf16")))
    return out


def cast_cases():
    """(dst dtype name, n, p, site triple)"""
    out = []
    for dt in ("fp32", "bf16"):
        for n in CAST_N:
            out.append((dt, n) + _cycle(len(out) + (dt == "bf16")))
    return out


# ---- text embedding ------------------------------------------------------------------------------------------------------------
def text_case(B, L, H, site, seed, device="cpu"):
    """reduce_ref.text_case (random ids, eps 1e-12) with the forward reference, walked over seeds until y is readable.
    -> the case dict: y / by are the DROPPED reference and bound, y_plain / by_plain the undropped ones, m the [M, H] multipliers"""
    why = ""
    for k in range(SEED_WALK):
        c = rf.text_reference(rf.text_case(B, L, H, "random", 1e-12, seed + 1000 * k, device=device), backward=False)
        ok, why = readable(f"text y (seed {seed + 1000 * k})", c["y"], c["by"])
        if ok:
            break
    assert ok, why
    M = B * L
    c["m"] = site.rows(M, H, device=device)
    c["y_plain"], c["by_plain"] = c["y"], c["by"]
    c["y"], c["by"] = c["y_plain"] * c["m"].to(F64), scaled_bound(c["y_plain"], c["by_plain"], c["m"])
    return c


def text_backward(c, m_bwd=None, dy=None, round_product=True):
    """reference and bounds of the backward with the mask m_bwd (default: the case's own) on dy -> a case dict for
    reduce_ref.check_text_bwd.  dy: another upstream gradient (the one-hot probes).  round_product False: dy * m in fp64 (the
    pin against the oracle)."""
    B, L, H, eps = c["B"], c["L"], c["H"], c["eps"]
    M = B * L
    m = c["m"] if m_bwd is None else m_bwd
    d = dict(c)
    dy = c["dy"] if dy is None else dy
    d["dy"] = (dy.reshape(M, H).to(F64) * m.to(F64)).reshape(B, L, H)
    if round_product:
        d["dy"] = rne32(d["dy"])
    w64, p64, t64 = c["word"].to(F64), c["pos"].to(F64), c["type0"].to(F64)
    e = w64[c["ids"]] + p64[:L][None] + t64[None, None]
    e_x = U * (w64[c["ids"]] + p64[:L][None]).abs() + U * e.abs()
    rf._text_backward_reference(d, e, e_x)
    return d


def text_got(d, dtype=F32):
    """what a kernel that computes exactly the reference of `d` returns: init + gradient, stored in fp32"""
    return {k: (d["init_" + k].to(F64) + d["ref"][k]).to(dtype) for k in ("dword", "dpos", "dtype0", "dgamma", "dbeta")}


# ---- panorama embedding --------------------------------------------------------------------------------------------------------
PANO_SIZES = lambda H: [H, H, H, H, 4 * H, H, H, H, 2 * H, H, H, H]      # noqa: E731  (row_ref.PANO_NAMES order)


def pano_y_bound(a, d, loc, nav, p):
    """elementwise bound of the UNDROPPED y of pano_embed_fwd_kernel, for the read-out precondition only (the values are held to
    row_ref's fp32 class): reduce_ref.ln_fwd_bounds through the kernel's chain -- the inner LayerNorms of a and d, the angle
    projection (bias + four products, at most 5 roundings per term) and its LayerNorm, the four adds of the branch sum, the outer
    LayerNorm with the branch sum's error as its input error"""
    H = a.shape[-1]
    ya = po.layer_norm(a, p["g_img"], p["b_img"], rr.EPS)
    e_sum = rf.ln_fwd_bounds(a, p["g_img"], p["b_img"], rr.EPS, ya, rr.ln_stats(a), False)[0]
    mag = ya.abs()
    x = ya
    if d is not None:
        yd = po.layer_norm(d, p["g_dep"], p["b_dep"], rr.EPS)
        e_sum = e_sum + rf.ln_fwd_bounds(d, p["g_dep"], p["b_dep"], rr.EPS, yd, rr.ln_stats(d), False)[0]
        mag, x = mag + yd.abs(), x + yd
    w = p["w_loc"].reshape(H, 4)
    lp = po.linear(loc, w, p["bias_loc"])
    e_lp = rf.gam(5) * (p["bias_loc"].abs()[None] + loc.abs() @ w.abs().t())
    yl = po.layer_norm(lp, p["g_loc"], p["b_loc"], rr.EPS)
    e_sum = e_sum + rf.ln_fwd_bounds(lp, p["g_loc"], p["b_loc"], rr.EPS, yl, rr.ln_stats(lp), False, e_lp)[0]
    nv = p["nav_emb"].reshape(2, H)[nav]
    mag = mag + yl.abs() + nv.abs() + p["type1"].abs()[None]
    x = x + yl + nv + p["type1"]
    e_sum = e_sum + rf.gam(4) * mag
    y = po.layer_norm(x, p["g_out"], p["b_out"], rr.EPS)
    return rf.ln_fwd_bounds(x, p["g_out"], p["b_out"], rr.EPS, y, rr.ln_stats(x), False, e_sum)[0]


def pano_case(M, H, depth, dtype, site, seed, device="cpu"):
    """inputs in the operand dtype (a / d rounded once; the reference upcasts those values), the undropped and the dropped forward
    reference.  b_out is then moved, column by column, into the widest gap between the values -xhat * g_out of that column's rows,
    so that no y comes near zero (385 x 768 random values always hold a few within 1e-6 of it): y is readable (pano_y_bound)."""
    why = ""
    for k in range(1):
        g = torch.Generator().manual_seed(seed + 1000 * k)
        a = (torch.randn(M, H, generator=g) * 2 + 0.3).to(dtype)
        d = (torch.randn(M, H, generator=g) * 0.5 - 1.0).to(dtype) if depth else None
        loc = torch.randn(M, 4, generator=g)
        nav = torch.randint(0, 2, (M,), generator=g)
        params = []
        for name, n in zip(rr.PANO_NAMES, PANO_SIZES(H)):
            if name.startswith("g_"):
                params.append(1.0 + 0.3 * torch.randn(n, generator=g))
            elif name.startswith("b_") or name == "bias_loc":
                params.append(0.5 * torch.randn(n, generator=g))
            else:
                params.append(torch.randn(n, generator=g))
        dy = torch.randn(M, H, generator=g)
        init = [torch.randn(n, generator=g) for n in PANO_SIZES(H)]
        p64 = {k: v.to(F64) for k, v in zip(rr.PANO_NAMES, params)}
        v = -(rr.pano_fwd(a.to(F64), None if d is None else d.to(F64), loc.to(F64), nav, p64)[0] - p64["b_out"])     # [M, H]
        v = torch.cat([v.min(0, keepdim=True).values - 1.0, v.sort(0).values, v.max(0, keepdim=True).values + 1.0], 0)
        lo = (v[1:] - v[:-1]).argmax(0, keepdim=True)
        params[11] = (0.5 * (v.gather(0, lo) + v.gather(0, lo + 1))).reshape(H).float()
        p64["b_out"] = params[11].to(F64)
        y, st = rr.pano_fwd(a.to(F64), None if d is None else d.to(F64), loc.to(F64), nav, p64)
        m = site.rows(M, H)
        ok, why = readable(f"pano y (seed {seed + 1000 * k})", y,
                           pano_y_bound(a.to(F64), None if d is None else d.to(F64), loc.to(F64), nav, p64))
        if ok:
            break
    assert ok, why
    c = {"M": M, "H": H, "depth": depth, "a": a, "d": d, "loc": loc, "nav": nav, "params": params, "dy": dy, "init": init, "m": m}
    c = {k: (v.to(device) if torch.is_tensor(v) else [t.to(device) for t in v] if isinstance(v, list) else v) for k, v in c.items()}
    c.update(p64={k: v.to(device) for k, v in p64.items()}, y_plain=y.to(device), st=st.to(device), y=(y * m.to(F64)).to(device))
    return c


def pano_backward(c, m_bwd=None, dy=None, round_product=True):
    m = c["m"] if m_bwd is None else m_bwd
    dy = (c["dy"] if dy is None else dy).to(F64) * m.to(F64)
    return rr.pano_bwd(rne32(dy) if round_product else dy, c["a"], c["d"], c["loc"], c["nav"], c["p64"])


def pano_got(c, ref):
    """what a kernel that computes exactly `ref` returns (da / dd in the operand dtype, init + gradient in fp32)"""
    t = c["a"].dtype
    grads = [(i.to(F64) + ref[k].reshape(-1)).to(F32) for k, i in zip(rr.PANO_NAMES, c["init"])]
    if not c["depth"]:
        for j in (2, 3):
            grads[j] = c["init"][j].clone()
    return ref["da"].to(t), None if ref["dd"] is None else ref["dd"].to(t), grads


# ---- SAP tail ------------------------------------------------------------------------------------------------------------------
def sap_fwd(r, gamma, beta, w2, b2, m, visited=None, valid=None):
    """row_ref.sap_fwd with the ClsPrediction dropout (vilmodel_cmt.py:657): logits = (LN(r) * m) . w2 + b2"""
    n = po.layer_norm(r, gamma, beta, rr.EPS) * m
    logit = po.linear(n, w2.reshape(1, -1), b2.reshape(1)).squeeze(-1)
    return logit.masked_fill(rr.sap_masked(r.shape[0], visited, valid, r.device), float("-inf")), rr.ln_stats(r)


def sap_bwd(dlogits, r, gamma, beta, w2, m_w, m_n, visited=None, valid=None):
    """the backward written out, so that the mask's two applications are separate arguments (the right code passes the same mask):
      dw2 = sum_rows dl * (LN(r) * m_w),  db2 = sum dl,  dn = dl * w2 * m_n,  (dr, dgamma, dbeta) = LayerNorm backward of dn,
      dz = dr * (r > 0); dlogits of masked rows count as 0"""
    r, gamma, beta, w2 = r.to(F64), gamma.to(F64), beta.to(F64), w2.to(F64)
    masked = rr.sap_masked(r.shape[0], visited, valid, r.device)
    dl = torch.where(masked, torch.zeros_like(dlogits, dtype=F64), dlogits.to(F64))
    n = po.layer_norm(r, gamma, beta, rr.EPS)
    dn = dl[:, None] * w2[None, :] * m_n.to(F64)
    dr, dgamma, dbeta = rf.ln_bwd(dn, r, gamma, rr.EPS)
    return {"dz": dr * (r > 0), "dgamma": dgamma, "dbeta": dbeta, "dw2": (dl[:, None] * n * m_w.to(F64)).sum(0), "db2": dl.sum().reshape(1)}


def sap_case(M, H, pattern, dtype, site, seed, device="cpu"):
    """r = relu(randn) in the operand dtype with an all-zero row (M >= 3); masks by `pattern` (test_row_kernels_gpu's); walked over
    seeds until LN(r) -- what dw2 shows of the mask -- and w2 are readable"""
    why = ""
    for k in range(SEED_WALK):
        g = torch.Generator().manual_seed(seed + 1000 * k)
        r = torch.relu(torch.randn(M, H, generator=g)).to(dtype)
        if M >= 3:
            r[1] = 0
        gamma, beta = 1.0 + 0.3 * torch.randn(H, generator=g), 0.5 * torch.randn(H, generator=g)
        w2, b2 = torch.randn(H, generator=g) * 0.05, torch.randn(1, generator=g)
        vis = (torch.rand(M, generator=g) < 0.3).to(torch.uint8)
        val = (torch.rand(M, generator=g) < 0.8).to(torch.uint8)
        if pattern == "none":
            vis, val = torch.zeros_like(vis), torch.ones_like(val)
        elif pattern == "both" and M >= 3:
            vis[0], val[0], vis[2], val[M - 1] = 0, 1, 1, 0                         # one kept, one visited, one padded row at least
        if pattern == "null":
            vis = val = None
        dl = torch.randn(M, generator=g)
        init = {"dgamma": torch.randn(H, generator=g), "dbeta": torch.randn(H, generator=g), "dw2": torch.randn(H, generator=g),
                "db2": torch.randn(1, generator=g)}
        n = po.layer_norm(r.to(F64), gamma.to(F64), beta.to(F64), rr.EPS)
        ok, why = readable(f"sap n (seed {seed + 1000 * k})", n,
                           rf.ln_fwd_bounds(r.to(F64), gamma, beta, rr.EPS, n, rr.ln_stats(r.to(F64)), False)[0])
        ok2, why2 = readable("sap w2", w2, torch.full_like(w2, 2.0 ** -100, dtype=F64))      # dl * w2: one exact-or-rounded product
        if ok and ok2:
            break
        why = why if not ok else why2
    assert ok and ok2, why
    c = {"M": M, "H": H, "r": r, "gamma": gamma, "beta": beta, "w2": w2, "b2": b2, "vis": vis, "val": val, "dl": dl, "init": init,
         "m": site.rows(M, H), "n": n}
    c = {k: (v.to(device) if torch.is_tensor(v) else {a: b.to(device) for a, b in v.items()} if isinstance(v, dict) else v)
         for k, v in c.items()}
    c["masked"] = rr.sap_masked(M, c["vis"], c["val"], device)
    return c


def sap_forward(c, m=None):
    p64 = [c[k].to(F64) for k in ("gamma", "beta", "w2", "b2")]
    return sap_fwd(c["r"].to(F64), *p64, (c["m"] if m is None else m).to(F64), visited=c["vis"], valid=c["val"])


def sap_backward(c, m_w=None, m_n=None, dl=None):
    return sap_bwd(c["dl"] if dl is None else dl, c["r"], c["gamma"], c["beta"], c["w2"], c["m"] if m_w is None else m_w,
                   c["m"] if m_n is None else m_n, visited=c["vis"], valid=c["val"])


def sap_got(c, ref, init=None):
    init = c["init"] if init is None else init
    return ref["dz"].to(c["r"].dtype), {k: (init[k].to(F64) + ref[k]).to(F32) for k in ("dgamma", "dbeta", "dw2", "db2")}


# ---- ln_bwd_s ------------------------------------------------------------------------------------------------------------------
def ln_blocks(M, slabs):
    return rf.ln_stage_blocks(M) if slabs else rf.ln_atomic_blocks(M)


def ln_case(M, H, slabs, site, seed, device="cpu"):
    """reduce_ref.ln_case (eps 1e-12; its rows span 2^-10 .. 2^3, an all-zero row, a row far from zero mean, the sentinel rows)"""
    c = rf.ln_case(M, H, 1e-12, ln_blocks(M, slabs), slabs, seed, device=device)
    c["m"] = site.rows(M, H, device=device)
    return c


def check_ln(name, c, dx, dx_lp, dgamma, dbeta, add):
    """dx, dgamma, dbeta: the UNDROPPED reference and bounds; dx_lp = RNE(dx * m) of the kernel's own dx, bit for bit"""
    rf.check_ln_bwd(name, c, dx, None, dgamma, dbeta, add)
    for k in ("dx", "dgamma", "dbeta"):
        record((name, k), rf.WORST.get((name, k), 0.0))
    rf.same_bits(f"{name} dx_lp (round-to-nearest-even of dx * multiplier)", dx_lp, (dx * c["m"].to(dx.device)).to(dx_lp.dtype))


# ---- cast_drop -----------------------------------------------------------------------------------------------------------------
def cast_case(n, seed, device="cpu"):
    """fp32 payload without zeros: magnitudes 2^-20 .. 2^20, both signs, ties of the bf16 rounding among them"""
    g = torch.Generator().manual_seed(seed)
    src = torch.randn(n, generator=g) * 2.0 ** torch.randint(-20, 21, (n,), generator=g).float()
    src = torch.where(src == 0, torch.ones_like(src), src)
    ties = torch.tensor([0x3F808000, 0x3F818000, 0x3F808001, 0x3F807FFF], dtype=torch.int32).view(F32)
    src[:4] = ties[:min(4, n)]
    return src.to(device)


def cast_site(p, triple, n):
    """the site of a cast case: the step seed is walked until every wrong mask of MASK_MISTAKES that can differ on n elements does
    (four elements under p = 0.1 are all kept under most seeds, and a shifted index then names the same four multipliers)"""
    for k in range(256):
        site = Site(p, triple, SEED + k)
        right = site.flat(n)
        if all(not torch.equal(site.flat(n, kind), right) for kind in MASK_MISTAKES if kind != "swap_rc"):
            return site
    raise AssertionError(f"no step seed tells the planted masks apart on {n} elements")


def check_cast(name, dst, src, m):
    mv.exact(name, dst, (src * m.to(src.device)).to(dst.dtype))
    zero_set(name + " (zeros)", dst, m)


# ---- GEMM epilogue -------------------------------------------------------------------------------------------------------------
# Order of the epilogue (csrc/gemm_shared.h, vector path and scalar path alike):
#     v = alpha * acc + bias  ->  activation (GELU_SAVEGRAD: Z = gelu'(v) stored here, C gets gelu(v); MUL_Z: v * Z)
#       ->  * multiplier(row * N + col)  ->  + R  ->  (+ old C under out_mode 1)  ->  store
# so   C = m * act(alpha A B^T + bias) + R,   Z of GELU_SAVEGRAD undropped,   MUL_Z: C = m * (Z * (alpha A B^T + bias)) -- the
# product with Z first, then the mask.
from tests import gemm_ref as gr  # noqa: E402

GEMM_COMPS = ("bias_res", "savegrad", "mul_z")
# (id, switches, kernel, BM, BN, S, k2, bf16 operands, the (M, N) list, the K list, output layout)
# mm32 takes whole tiles and whole 64-slabs only (two at least; the k2 classes two pairs): its reduction lengths are the two
# shortest it accepts instead of 64 and 160, and it has no ragged shape.  gemm_dma in bf16 needs whole 64-slabs as well.
GEMM_INSTANCES = (
    ("mm32-128", {"MM32": "128"}, "mm32", 128, 128, 2, False, True, ((256, 128),), (128, 192), "pad"),
    ("mm32-64", {"MM32": "64"}, "mm32", 128, 64, 3, False, True, ((256, 64),), (128, 192), "pad"),
    ("mm32-264", {"MM32": "264"}, "mm32", 128, 64, 3, True, True, ((256, 64),), (256, 384), "pad"),
    ("dma-bf16", {"GEMM_TILE": "64s3", "MM32": "0"}, "gemm_dma", 64, 64, 3, False, True, ((128, 64), (65, 72)), (128, 192), "pad"),
    ("dma-f32", {"GEMM_TILE": "64s3", "MM32": "0"}, "gemm_dma", 64, 64, 3, False, False, ((128, 64), (65, 72)), (64, 160), "pad"),
    ("reg-bf16", {"GEMM_TILE": "64r", "MM32": "0"}, "gemm", 64, 64, 0, False, True, ((128, 64), (65, 72)), (64, 160), "pad"),
    ("reg-f32", {"GEMM_TILE": "64r", "MM32": "0"}, "gemm", 64, 64, 0, False, False, ((65, 72),), (64, 160), "pad"),
    ("scalar-dma", {"GEMM_TILE": "64s3", "MM32": "0"}, "gemm_dma", 64, 64, 3, False, True, ((65, 69),), (128, 192), "pad"),
    ("scalar-reg", {"GEMM_TILE": "64r", "MM32": "0"}, "gemm", 64, 64, 0, False, False, ((65, 69),), (64, 160), "odd"),
)


def gemm_comp(comp, bf16):
    """-> (act, C in bf16?, storage (trans_a, trans_b)) of a composition: what the planner launches with a mask
    bias_res   linear_fwd_s: y = x + dropout(dense(h)), bias + mask + residual into the fp32 stream
    savegrad   the FFN's inner product: h = dropout(gelu(v)) in the operand dtype, Z = gelu'(v) kept for the backward, undropped
    mul_z      the FFN's dgrad: dv = dropout'(dh) * gelu'(v) = m * Z * (dy W2), operand dtype, NN storage"""
    return {"bias_res": (gr.ACT_NONE, False, (0, 0)), "savegrad": (gr.ACT_GELU_SAVEGRAD, bf16, (0, 0)),
            "mul_z": (gr.ACT_MUL_Z, bf16, (0, 1))}[comp]


def gemm_case(M, N, K, bf16, comp, seed, out_mode=0):
    """Stored operand values (CPU fp32 tensors).  A standard normal with one zero row, B 0.35 / sqrt(K) x + 0.01 with one zero row (acc stays
    within ~ +-2, so gelu never sinks below its bound on the negative side); the bias of column c puts every v of that column 0.5
    or more above zero (even c) or below zero (odd c), so that no undropped value comes near its bound; Z of MUL_Z: half values
    with |z| >= 0.05; R, C0 in the output dtype."""
    act, c_bf16, _ = gemm_comp(comp, bf16)
    g = torch.Generator().manual_seed(7 * seed + 131 * M + 17 * N + K)
    A = torch.randn(M, K, generator=g)
    B = torch.randn(N, K, generator=g) * (0.35 / K ** 0.5) + 0.01
    A[M // 3] = 0.0
    B[N // 2] = 0.0
    if bf16:
        A, B = A.bfloat16().float(), B.bfloat16().float()
    alpha = gr.f32(0.5 if comp == "mul_z" else 1.0)
    acc = alpha * (A.to(F64) @ B.to(F64).t())
    even = torch.arange(N) % 2 == 0
    bias = torch.where(even, 0.5 - acc.min(0).values, -0.5 - acc.max(0).values).float()
    rc = (lambda x: x.bfloat16().float()) if c_bf16 else (lambda x: x)
    c = dict(M=M, N=N, K=K, bf16=bf16, c_bf16=c_bf16, act=act, alpha=alpha, A=A, B=B, bias=bias, out_mode=out_mode, comp=comp,
             R=rc(torch.randn(M, N, generator=g)) if comp == "bias_res" else None,
             C0=rc(torch.randn(M, N, generator=g)) if out_mode else None, Z=None)
    if comp == "mul_z":
        z = torch.randn(M, N, generator=g)
        z = torch.where(z.abs() < 0.05, torch.where(z < 0, -0.05, 0.05), z)
        c["Z"] = z.half().float() if bf16 else z
    return c


def gemm_ref(c, m, place="after"):
    """gemm_ref.gemm_ref with the mask between the activation and the residual -> (values, bounds) over "C" (and "Z").
    Built ON gemm_ref: its value and bound of act(v) (no residual, no old C, no output rounding), then
        y = act * m                      bound E_act * m * (1 + u) + u |y|       (one fp32 multiply)
        + R, + old C, the C store        gemm_ref's own lines
    place: where a kernel with a planted mistake would put the mask -- "before_act" (on v), "on_z" (on the stored Z as well),
    "on_r" (on act + R)."""
    m = m.to(F64)
    dev = m.device
    t = lambda x: None if x is None else x.to(dev)      # noqa: E731
    kw = dict(alpha=c["alpha"], bias=t(c["bias"]), Z=t(c["Z"]), act=c["act"], bf16=c["bf16"], c_bf16=False)
    val, E = gr.gemm_ref(t(c["A"]), t(c["B"]), **kw)
    y, E_y = val["C"], E["C"]
    if place == "before_act":
        v = c["alpha"] * (t(c["A"]).to(F64) @ t(c["B"]).to(F64).t()) + t(c["bias"]).to(F64)
        y = gr.gelu(v * m) if c["act"] == gr.ACT_GELU_SAVEGRAD else (v * m * t(c["Z"]).to(F64) if c["act"] == gr.ACT_MUL_Z else v * m)
    elif place != "on_r":
        y, E_y = y * m, E_y * m * (1.0 + U) + U * (y * m).abs()
    if c["R"] is not None:
        r = t(c["R"]).to(F64)
        y = y + r
        E_y = E_y + gr.EPS32 * (r.abs() + y.abs())
    if place == "on_r":
        y = y * m
    if c["out_mode"] == 1:
        c0 = t(c["C0"]).to(F64)
        y = y + c0
        E_y = E_y + gr.EPS32 * (c0.abs() + y.abs())
    if c["c_bf16"]:
        E_y = E_y + gr.U_BF16 * y.abs()
    val["C"], E["C"] = y, E_y
    if "Z" in val and place == "on_z":
        val["Z"] = val["Z"] * m
    return val, E


def gemm_readable(c):
    """the read-out precondition of a GEMM case, on the reference alone: every UNDROPPED act(v) / (1 - p_max) exceeds twice the
    bound of its output (twice: the dropped elements of a residual form are compared with the fp32 sum R (+ old C), one more
    rounding away from the reference)"""
    val, E = gemm_ref(c, torch.ones(c["M"], c["N"]))
    y = val["C"] - (0 if c["R"] is None else c["R"].to(F64)) - (0 if c["C0"] is None else c["C0"].to(F64))
    return readable(f"gemm {c['comp']} {c['M']}x{c['N']}x{c['K']}", y, 2 * E["C"] * float(inv_keep(max(RATES))))


def gemm_zero_set(what, c, got_c, m):
    """exact: C equals the fp32 (bf16) value of R (+ old C) -- 0 without them -- exactly where the multiplier is 0"""
    base = torch.zeros_like(got_c, dtype=F32)
    if c["R"] is not None:
        base = base + c["R"].to(got_c.device)
    if c["C0"] is not None:
        base = base + c["C0"].to(got_c.device)
    zero_set(what, got_c.to(F64) - base.to(got_c.dtype).to(F64), m)


def check_gemm(name, key, c, got, m):
    val, E = gemm_ref(c, m)
    gemm_zero_set(f"{name} C", c, got["C"], m)
    for n in val:
        ratio = gr.close(got[n], val[n], E[n], f"{name} {n}", f"{key}/{n}")
        record((key, n), ratio)


# ---- attention -----------------------------------------------------------------------------------------------------------------
# Dropout sits on the probabilities, index ((b * heads + h) * Lq + q) * Lk + key (never ldS):
#     Pd = P * m     ctx = Pd V     dPd = dO V^T     dP = dPd * m     D = rowsum(P * dP)     dS = P (dP - D)     dV = Pd^T dO
# (D = rowsum(dO * ctx) still holds: P * dP = Pd * dPd.)  The stored P and the softmax backward see the UNDROPPED P.
from tests import attn_ref as ar  # noqa: E402

ATTN_PAIRS = ((5, 5), (21, 21), (64, 37), (16, 80), (128, 128))          # 21 and 37: odd Lk, the odd-start runs of family 2
ATTN_BATCHES = ((2, 12), (3, 2))
ATTN_LONG = ((64, 129), (130, 200))


def attn_index_mask(site, B, nh, Lq, Lk, mistake=None, ldS=None, device="cpu"):
    """fp32 [B, heads, Lq, Lk] multipliers at index ((b * heads + h) * Lq + q) * Lk + key -- or the planted mistake's:
    "ld" indexes with ldS, "swap_rc" with (.. * Lk + key) * Lq + q, "even_branch" walks every run of four keys that starts at an
    odd index as if it started at an even one (drop_mult_run's second branch replaced by the first)"""
    M = B * nh * Lq
    if mistake == "even_branch":
        nrun = (Lk + 3) // 4
        starts = np.arange(M, dtype=np.uint64)[:, None] * np.uint64(Lk) + np.uint64(4) * np.arange(nrun, dtype=np.uint64)[None, :]
        m = torch.from_numpy(mult_runs(site.p, site.sseed, starts, 4, odd_as_even=True).reshape(M, nrun * 4)[:, :Lk].copy()).to(device)
    elif mistake == "swap_rc":
        bh = np.arange(B * nh, dtype=np.uint64)[:, None, None]
        qi, ki = np.arange(Lq, dtype=np.uint64)[None, :, None], np.arange(Lk, dtype=np.uint64)[None, None, :]
        m = torch.from_numpy(mult_at(site.p, site.sseed, (bh * np.uint64(Lk) + ki) * np.uint64(Lq) + qi)).to(device)
    else:
        m = site.rows(M, Lk, mistake, device=device, ld=ldS)
    return m.reshape(B, nh, Lq, Lk)


ATTN_MASKS = ("ld", "even_branch") + MASK_MISTAKES


def attn_case(Lq, Lk, B, nh, bf16, mask_mode, with_dist, seed):
    """attn_ref.make_case's dict with operands that keep every valid key's probability readable: q, k ~ 0.5 N(0, 1) (scores within
    about +-1), sp_w 0.3 on dist in [0, 3); one invalid-key pattern (key 0 and every fifth key of odd batch entries, the last three
    keys of even ones; a valid key always remains)"""
    g = torch.Generator().manual_seed(1000 * seed + 7 * Lq + Lk + 131 * B)
    rnd = lambda *s: torch.randn(*s, generator=g)      # noqa: E731
    q, k, v, do = 0.5 * rnd(B, nh, Lq, 64), 0.5 * rnd(B, nh, Lk, 64), rnd(B, nh, Lk, 64), rnd(B, nh, Lq, 64)
    if bf16:
        q, k, v, do = (t.bfloat16().float() for t in (q, k, v, do))
    km = torch.ones(B, Lk, dtype=torch.bool)
    for b in range(B):
        if b % 2:
            km[b, 0::5] = False
        else:
            km[b, max(1, Lk - 3):] = False
    km[:, min(1, Lk - 1)] = True
    dist = torch.rand(B, Lq, Lk, generator=g) * 3.0 if with_dist else None
    return dict(q=q, k=k, v=v, dctx=do, km=km, dist=dist, sp_w=gr.f32(0.3), sp_b=gr.f32(0.1), alpha=gr.f32(0.125), mask_mode=mask_mode,
                bf16=bf16, Lq=Lq, Lk=Lk, B=B, nh=nh)


def attn_ref(c, m_f, m_b=None, gemm=False, device=None, v=None, dctx=None, tile=False):
    """attn_ref.attn_ref with the mask m_f [B, heads, Lq, Lk] on the forward's probabilities and m_b (default m_f) wherever the
    backward regenerates it -> (values, bounds) like attn_ref's.  v / dctx: other operands (the one-hot probes).
    The bounds are attn_ref's lines on the dropped operands (Pd for P in E_ctx and E_dV, dP = dPd * m in E_dS) plus
      2^-24 Pd |V|, 2^-24 Pd^T |dO|, 2^-24 |dP|   the multiply by the mask, one fp32 rounding
      gemm and bf16 (family 0): drop_rows stores the dropped copy of the bf16 P in bf16 again, and dP = dPd * m over the bf16 dPd
      in place: a second u on Pd |V|, Pd^T |dO| and |dP|
      tile and bf16 (family 1): attn_bwd_kernel reads the bf16 P tile the forward stored and writes P * m back into the tile in
      bf16 for dV = Pd^T dO: a second u on Pd^T |dO| (its forward rounds Pd once, from fp32; its dP stays in registers)"""
    t = lambda x: None if x is None else (x.to(device) if device else x)      # noqa: E731
    q, k, vv, do = (t(x).detach().to(F64) for x in (c["q"], c["k"], c["v"] if v is None else v, c["dctx"] if dctx is None else dctx))
    km, dist, alpha, bf16, mask_mode = t(c["km"]), t(c["dist"]), c["alpha"], c["bf16"], c["mask_mode"]
    m_f = t(m_f).to(F64)
    m_b = m_f if m_b is None else t(m_b).to(F64)
    B, nh, Lq, _ = q.shape
    u = ar.U_BF16 if bf16 else 0.0
    twice = 2.0 if (gemm and bf16) else 1.0
    twice_dv = 2.0 if ((gemm or tile) and bf16) else 1.0
    s0 = alpha * (q @ k.transpose(-1, -2))
    add = torch.zeros(B, 1, 1, k.shape[2], dtype=F64, device=q.device)
    if km is not None:
        add = torch.where(km, 0.0, float("-inf") if mask_mode else -10000.0).to(F64)[:, None, None, :]
    n_add = 1
    if dist is not None:
        dist = dist.detach().to(F64)
        add = add + (dist * float(c["sp_w"]) + float(c["sp_b"]))[:, None]
        n_add = 2
    P = torch.softmax(s0 + add, -1)
    Pf, Pb = P * m_f, P * m_b
    ctx = Pf @ vv
    dPd = do @ vv.transpose(-1, -2)
    dP = dPd * m_b
    D = (P * dP).sum(-1, keepdim=True)
    dS = P * (dP - D)
    val = {"ctx": ctx, "dQ": alpha * (dS @ k), "dK": alpha * (dS.transpose(-1, -2) @ q), "dV": Pb.transpose(-1, -2) @ do, "P": P}
    if dist is not None:
        val["d_sp_w"], val["d_sp_b"] = (dS.sum(1) * dist).sum(), dS.sum()
    Es = torch.zeros(B, nh, Lq, 1, dtype=F64, device=q.device)
    E_dP = gr.EPS32 * dP.abs()
    if gemm and bf16:
        Es = Es + u * s0.abs().amax(-1, keepdim=True)
        E_dP = E_dP + 2.0 * u * dP.abs()
    if km is not None and not mask_mode:
        Es = Es + n_add * 2.0 ** -11 * (~km.any(-1)).to(F64)[:, None, None, None]
    E_P = 2.0 * Es * P
    av, ado = vv.abs(), do.abs()
    E_ctx = u * (twice * (Pf @ av) + ctx.abs()) + (E_P * m_f) @ av + gr.EPS32 * (Pf @ av)
    E_dV = u * (twice_dv * (Pb.transpose(-1, -2) @ ado) + val["dV"].abs()) + (E_P * m_b).transpose(-1, -2) @ ado + gr.EPS32 * (Pb.transpose(-1, -2) @ ado)
    E_D = (ado * E_ctx).sum(-1, keepdim=True)
    E_dS = u * dS.abs() + P * E_D + E_P * (dP - D).abs() + P * (E_dP + (P * E_dP).sum(-1, keepdim=True))
    E = {"ctx": E_ctx, "dQ": alpha * (E_dS @ k.abs()) + u * val["dQ"].abs(), "dK": alpha * (E_dS.transpose(-1, -2) @ q.abs()) + u * val["dK"].abs(),
         "dV": E_dV}
    for n in ("ctx", "dQ", "dK", "dV"):
        E[n] = E[n] + ar.FP32_REL * max(1.0, float(val[n].abs().max()))
    if dist is not None:
        E["d_sp_w"] = (E_dS.sum(1) * dist.abs()).sum() + ar.FP32_REL * max(1.0, float((dS.abs().sum(1) * dist.abs()).sum()))
        E["d_sp_b"] = E_dS.sum() + ar.FP32_REL * max(1.0, float(dS.abs().sum()))
    return val, E


def probe_v(c, j):
    """V of the ctx probe of key block j: V[key] = e_(key - 64 j) inside the block, 0 outside -> ctx[q, d] = Pd[q, 64 j + d]"""
    v = torch.zeros_like(c["v"])
    for key in range(64 * j, min(c["Lk"], 64 * j + 64)):
        v[:, :, key, key - 64 * j] = 1.0
    return v


def probe_do(c, i):
    """dO of the dV probe of query block i: dO[q] = e_(q - 64 i) inside the block, 0 outside -> dV[key, d] = Pd[64 i + d, key]"""
    do = torch.zeros_like(c["dctx"])
    for qq in range(64 * i, min(c["Lq"], 64 * i + 64)):
        do[:, :, qq, qq - 64 * i] = 1.0
    return do


def probe_ctx_check(what, c, j, got_ctx, m, val, E):
    """ctx of probe j against the mask: exact zeros == {multiplier == 0} over the VALID keys of the block (P > 0), after showing on
    the reference alone that every valid key's undropped probability / (1 - p) ... exceeds the probe's own bound"""
    Lk = c["Lk"]
    n = min(Lk, 64 * j + 64) - 64 * j
    P = val["P"][..., 64 * j:64 * j + n]                                         # [B, heads, Lq, n]
    valid = P > 0
    keep = m.to(P.device)[..., 64 * j:64 * j + n] != 0
    short = valid & (P <= E["ctx"][..., :n])
    assert not bool(short.any()), f"{what}: {int(short.sum())} valid probabilities do not exceed the probe's bound"
    zero = got_ctx.to(F64)[..., :n] == 0
    bad = valid & (zero == keep)
    assert not bool(bad.any()), f"{what}: {int(bad.sum())} of {int(valid.sum())} valid probabilities read zero where kept or nonzero where dropped"
    assert bool((got_ctx.to(F64)[..., n:] == 0).all()), f"{what}: columns past the block are not zero"


def probe_dv_check(what, c, i, got_dv, m, val, E):
    """dV of probe i: dV[key, d] = Pd[64 i + d, key]"""
    Lq = c["Lq"]
    n = min(Lq, 64 * i + 64) - 64 * i
    P = val["P"][..., 64 * i:64 * i + n, :].transpose(-1, -2)                    # [B, heads, Lk, n]
    valid = P > 0
    keep = m.to(P.device)[..., 64 * i:64 * i + n, :].transpose(-1, -2) != 0
    short = valid & (P <= E["dV"][..., :n])
    assert not bool(short.any()), f"{what}: {int(short.sum())} valid probabilities do not exceed the probe's bound"
    zero = got_dv.to(F64)[..., :n] == 0
    bad = valid & (zero == keep)
    assert not bool(bad.any()), f"{what}: {int(bad.sum())} of {int(valid.sum())} valid probabilities read zero where kept or nonzero where dropped"


def attn_grid(pairs, dist_options=(True, False)):
    """(Lq, Lk, B, heads, mask_mode, with_dist, p, site triple, seed): mask modes x distance bias on every pair, the rest cycling"""
    out = []
    for (Lq, Lk) in pairs:
        for mask_mode in (0, 1):
            for with_dist in dist_options:
                i = len(out)
                B, nh = ATTN_BATCHES[i % 2]
                out.append((Lq, Lk, B, nh, mask_mode, with_dist, RATES[(i // 2) % 2], SITES[(i // 4 + i) % 2], i))
    return out


ATTN_SHORT_G = attn_grid(ATTN_PAIRS)                                          # families 2 and 1 (bf16)
ATTN_F32_G = attn_grid([p for p in ATTN_PAIRS if max(p) <= 64])              # family 1 (fp32)
ATTN_LONG_G = attn_grid(ATTN_LONG, dist_options=(False,))                    # family 3
ATTN_GEMM_G = [(70, 70, 2, 12, 0, True, 0.1, SITES[0], 1), (70, 70, 3, 2, 1, False, 0.4, SITES[1], 2),          # family 0: fp32
               (130, 200, 3, 2, 0, True, 0.4, SITES[0], 3), (130, 200, 2, 12, 1, True, 0.1, SITES[1], 4)]      #           bf16
