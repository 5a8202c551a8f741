"""Op-level tests of the fused row kernels against float64 references (tests/row_ref.py), through the C ABI:

  etp_pano_embed_fwd / _bwd   pano_embed_fwd_kernel, pano_embed_bwd_kernel<T, NCH, PART 0/1/2>   vilmodel_cmt.py:695-711
  etp_gmap_embed_fwd / _bwd   gmap_embed_fwd_kernel, gmap_embed_bwd_kernel                       :728-730
  etp_sap_tail_fwd / _bwd     sap_tail_fwd_kernel, sap_tail_bwd_kernel                           :651-661, 742-744
  etp_ln_stream_fwd           ln_fwd_s_kernel                                                    :150-154, 189-193

Every case takes the inputs in the operand dtype (bf16 mode: a / d / r are rounded to bf16 once and the reference upcasts those
values), so the only bf16 rounding left is the kernel's own output store.  Every output is filled with NaN first (a row the kernel
never writes fails), and every parameter-gradient buffer with a random "previous gradient" (the kernels accumulate: expected =
initial + reference).

Grid: fp32 and bf16 x H = 768 x M in {1, 3, 5, 257, 385, 1152, 7680}, H = 256 and 512 at M in {5, 385}; the forward kernels also at
M = 16389, one row past their 16384-row grid-stride trip (4096 blocks x 4 rows).  M = 385 is one row past the pano backward's trip
(96 blocks x 4), M = 257 one past the gmap / SAP backward's (64 x 4).  The per-kernel patterns (depth or not, nav types, step ids,
masks, output pointers, eps) cycle over that grid so that each appears in both dtypes.

Bounds (row_ref.py):
  fp32 results and parameter gradients   max|got - ref| <= 2e-5 * max(1, max|ref|) per tensor (test_text_embedding_fwd_bwd's
                                         convention); rstd 1e-5 relative.  They hold in bf16 mode too: the inputs are bf16 already.
  bf16 results without an fp32 twin      (da, dd, dz, a lone y_lp) within one bf16 ulp of the fp64 value + 2e-5 * max|ref|
  structural checks, exact               -inf logits of masked rows, dz == 0 on masked rows and where r == 0, untouched g_dep /
                                         b_dep without depth and untouched step-table rows, bf16 copies == round-to-nearest-even
                                         of the kernel's own fp32 result
Worst observed on the MI355X (96 cases, 4.8 s): fp32 class 1.1e-6 x max(1, max|ref|) (a lone fp32 y_lp of the LayerNorm), rstd
1.7e-7 relative (SAP stats), bf16 class 0.50 ulp beyond the 2e-5 slack (pano da: the rounding of the store itself).  The module
prints these figures after its last case (pytest -s).
"""
import ctypes
import itertools

import pytest
import torch

pytestmark = pytest.mark.gpu

from etpnav_amd import _lib  # noqa: E402
from etpnav_amd._lib import check, ptr  # noqa: E402
from tests import row_ref as rr  # noqa: E402

DEV = "cuda"
F64 = torch.float64
SHAPES = [(768, 1), (768, 3), (768, 5), (768, 257), (768, 385), (768, 1152), (768, 7680), (256, 5), (256, 385), (512, 5), (512, 385)]
FWD_ONLY = [(768, 16389)]
DTYPES = [(_lib.ETP_F32, "fp32"), (_lib.ETP_BF16, "bf16")]


def L():
    return _lib.lib()


def stream():
    return torch.cuda.current_stream().cuda_stream


def tdt(dtype):
    return torch.bfloat16 if dtype == _lib.ETP_BF16 else torch.float32


def nan(*shape, dtype=torch.float32):
    return torch.full(shape, float("nan"), device=DEV, dtype=dtype)


def grid(patterns, shift):
    """pytest params (dtype, H, M, backward?, pattern) over SHAPES + FWD_ONLY; pattern j of `patterns` cycles with the case
    index, shifted per dtype so the two dtypes see different shape / pattern pairs.  (test_ln_stream_fwd has no backward to
    skip and ignores the flag.)"""
    out = []
    for di, (dt, dn) in enumerate(DTYPES):
        for j, (H, M) in enumerate(SHAPES + FWD_ONLY):
            pat = patterns[(j + shift * di) % len(patterns)]
            bwd = (H, M) not in FWD_ONLY
            out.append(pytest.param(dt, H, M, bwd, pat, id=f"{dn}-H{H}-M{M}-{'-'.join(map(str, pat))}"))
    return out


@pytest.fixture(scope="module", autouse=True)
def report_worst():
    yield
    print("\nrow kernels, worst observed per bound class: " +
          ", ".join(f"{k} {v:.3g} ({n})" for k, (v, n) in rr.WORST.items()))


# ---- panorama fuse ---------------------------------------------------------------------------------------------------------
PANO_PATTERNS = [(depth, nav) for nav in ("zeros", "ones", "single", "random") for depth in ("depth", "nodepth")]


@pytest.mark.parametrize("dtype,H,M,bwd,pattern", grid(PANO_PATTERNS, 3))
def test_pano_embed_fwd_bwd(dtype, H, M, bwd, pattern):
    depth, navp = pattern[0] == "depth", pattern[1]
    torch.manual_seed(M * 7 + H + dtype)
    t = tdt(dtype)
    a = (torch.randn(M, H, device=DEV) * 2 + 0.3).to(t)
    d = (torch.randn(M, H, device=DEV) * 0.5 - 1.0).to(t) if depth else None
    loc = torch.randn(M, 4, device=DEV)
    nav = {"zeros": torch.zeros(M, dtype=torch.long, device=DEV), "ones": torch.ones(M, dtype=torch.long, device=DEV),
           "single": torch.zeros(M, dtype=torch.long, device=DEV), "random": torch.randint(0, 2, (M,), device=DEV)}[navp]
    if navp == "single":
        nav[-1] = 1                                   # PART 0 forms nav_emb[1]'s gradient as (all rows) - (nav-0 rows)
    sizes = [H, H, H, H, 4 * H, H, H, H, 2 * H, H, H, H]
    params = []
    for name, n in zip(rr.PANO_NAMES, sizes):
        if name.startswith("g_"):
            params.append(1.0 + 0.3 * torch.randn(n, device=DEV))
        elif name.startswith("b_") or name == "bias_loc":
            params.append(0.5 * torch.randn(n, device=DEV))
        else:
            params.append(torch.randn(n, device=DEV))
    PP = (ctypes.c_void_p * 12)(*[p.data_ptr() for p in params])
    y, stats = nan(M, H), nan(M, 8)
    check(L().etp_pano_embed_fwd(dtype, ptr(a), ptr(d), ptr(loc), ptr(nav), PP, ptr(y), ptr(stats), M, H, stream()), "pano_embed_fwd")
    torch.cuda.synchronize()
    p64 = {k: v.to(F64) for k, v in zip(rr.PANO_NAMES, params)}
    ref_y, ref_st = rr.pano_fwd(a.to(F64), None if d is None else d.to(F64), loc.to(F64), nav, p64)
    rr.check_pano_fwd(y, stats, ref_y, ref_st, depth)
    if not bwd:
        return
    dy = torch.randn(M, H, device=DEV)
    init = [torch.randn(n, device=DEV) for n in sizes]
    grads = [g.clone() for g in init]
    GG = (ctypes.c_void_p * 12)(*[g.data_ptr() for g in grads])
    da = nan(M, H, dtype=t)
    dd = nan(M, H, dtype=t) if depth else None
    check(L().etp_pano_embed_bwd(dtype, ptr(dy), ptr(a), ptr(d), ptr(loc), ptr(nav), ptr(stats), PP, GG, ptr(da), ptr(dd), M, H,
                                 stream()), "pano_embed_bwd")
    torch.cuda.synchronize()
    ref = rr.pano_bwd(dy, a, d, loc, nav, p64)
    rr.check_pano_bwd(da, dd, grads, init, ref, depth)


# ---- graph-node embedding --------------------------------------------------------------------------------------------------
GMAP_PATTERNS = [("zeros",), ("nonzero",), ("random",)]


@pytest.mark.parametrize("dtype,H,M,bwd,pattern", grid(GMAP_PATTERNS, 1))
def test_gmap_embed_fwd_bwd(dtype, H, M, bwd, pattern):
    torch.manual_seed(M * 5 + H + dtype)
    steps = 100                                       # max_action_steps
    img = torch.randn(M, H, device=DEV)
    if pattern[0] == "zeros":                         # step id 0 ([stop] and ghost nodes) goes through the block accumulator
        ids = torch.zeros(M, dtype=torch.long, device=DEV)
    elif pattern[0] == "nonzero":                     # every other id through global atomics
        ids = torch.randint(1, steps, (M,), device=DEV)
    else:
        ids = torch.randint(0, steps, (M,), device=DEV)
        ids[M // 2] = steps - 1
        ids[-1] = ids[0]
    pos = torch.randn(M, 7, device=DEV)
    step_emb = torch.randn(steps, H, device=DEV)
    w_pos, b_pos = torch.randn(H, 7, device=DEV) * 0.3, torch.randn(H, device=DEV) * 0.1
    gamma, beta = 1.0 + 0.3 * torch.randn(H, device=DEV), 0.5 * torch.randn(H, device=DEV)
    x, stats = nan(M, H), nan(M, 2)
    x_lp = nan(M, H, dtype=torch.bfloat16) if dtype == _lib.ETP_BF16 else None
    check(L().etp_gmap_embed_fwd(dtype, ptr(img), ptr(ids), ptr(pos), ptr(step_emb), ptr(w_pos), ptr(b_pos), ptr(gamma), ptr(beta),
                                 ptr(x), ptr(x_lp), ptr(stats), M, H, 7, stream()), "gmap_embed_fwd")
    torch.cuda.synchronize()
    args64 = [v.to(F64) for v in (img,)] + [ids] + [v.to(F64) for v in (pos, step_emb, w_pos, b_pos, gamma, beta)]
    ref_x, ref_st = rr.gmap_fwd(*args64)
    rr.check_gmap_fwd(x, x_lp, stats, ref_x, ref_st)
    if not bwd:
        return
    dx = torch.randn(M, H, device=DEV)
    init = {"d_step_emb": torch.randn(steps, H, device=DEV), "d_w_pos": torch.randn(H, 7, device=DEV),
            "d_b_pos": torch.randn(H, device=DEV), "dgamma": torch.randn(H, device=DEV), "dbeta": torch.randn(H, device=DEV)}
    got = {k: v.clone() for k, v in init.items()}
    check(L().etp_gmap_embed_bwd(dtype, ptr(dx), ptr(ids), ptr(pos), ptr(w_pos), ptr(b_pos), ptr(gamma), ptr(stats),
                                 ptr(got["d_step_emb"]), ptr(got["d_w_pos"]), ptr(got["d_b_pos"]), ptr(got["dgamma"]), ptr(got["dbeta"]),
                                 M, H, 7, stream()), "gmap_embed_bwd")
    torch.cuda.synchronize()
    ref = rr.gmap_bwd(dx, *args64)
    rr.check_gmap_bwd(got, init, ref, ids)


# ---- SAP head tail ---------------------------------------------------------------------------------------------------------
SAP_PATTERNS = [("null",), ("visited",), ("valid",), ("both",), ("all",), ("none",)]


def sap_masks(kind, M):
    vis = (torch.rand(M, device=DEV) < 0.3).to(torch.uint8)
    val = (torch.rand(M, device=DEV) < 0.8).to(torch.uint8)
    if kind == "all":                                 # every row masked
        vis = torch.ones(M, dtype=torch.uint8, device=DEV)
    elif kind == "none":                              # both masks given, none set
        vis, val = torch.zeros_like(vis), torch.ones_like(val)
    return (vis if kind in ("visited", "both", "all", "none") else None,
            val if kind in ("valid", "both", "all", "none") else None)


@pytest.mark.parametrize("dtype,H,M,bwd,pattern", grid(SAP_PATTERNS, 3))
def test_sap_tail_fwd_bwd(dtype, H, M, bwd, pattern):
    torch.manual_seed(M * 3 + H + dtype)
    t = tdt(dtype)
    r = torch.relu(torch.randn(M, H, device=DEV)).to(t)
    r[torch.arange(M, device=DEV) % 5 == 1] = 0       # all-zero ReLU rows
    gamma, beta = 1.0 + 0.3 * torch.randn(H, device=DEV), 0.5 * torch.randn(H, device=DEV)
    w2, b2 = torch.randn(H, device=DEV) * 0.05, torch.randn(1, device=DEV)
    vis, val = sap_masks(pattern[0], M)
    masked = rr.sap_masked(M, vis, val, DEV)
    logits, stats = nan(M), nan(M, 2)
    check(L().etp_sap_tail_fwd(dtype, ptr(r), ptr(gamma), ptr(beta), ptr(w2), ptr(b2), ptr(vis), ptr(val), ptr(logits), ptr(stats), M, H,
                               stream()), "sap_tail_fwd")
    torch.cuda.synchronize()
    p64 = [v.to(F64) for v in (gamma, beta, w2, b2)]
    ref_lg, ref_st = rr.sap_fwd(r.to(F64), *p64, visited=vis, valid=val)
    rr.check_sap_fwd(logits, stats, ref_lg, ref_st, masked)
    if not bwd:
        return
    dl = torch.randn(M, device=DEV)
    dl[masked] = float("nan")                         # whatever the loss left there must not leak into any gradient
    init = {"dgamma": torch.randn(H, device=DEV), "dbeta": torch.randn(H, device=DEV), "dw2": torch.randn(H, device=DEV),
            "db2": torch.randn(1, device=DEV)}
    got = {k: v.clone() for k, v in init.items()}
    dz = nan(M, H, dtype=t)
    check(L().etp_sap_tail_bwd(dtype, ptr(dl), ptr(r), ptr(gamma), ptr(beta), ptr(w2), ptr(stats), ptr(vis), ptr(val), ptr(dz),
                               ptr(got["dgamma"]), ptr(got["dbeta"]), ptr(got["dw2"]), ptr(got["db2"]), M, H, stream()), "sap_tail_bwd")
    torch.cuda.synchronize()
    ref = rr.sap_bwd(dl, r, *p64, visited=vis, valid=val)
    rr.check_sap_bwd(dz, got, init, ref, masked, r)


# ---- LayerNorm on the fp32 stream ------------------------------------------------------------------------------------------
# eps 1e-5: the XLM-R LayerNorms of workload c4 (PlannerConfig.rxr)
LN_PATTERNS = list(itertools.product(("y", "lp", "both"), ("stats", "nostats"), (1e-12, 1e-5)))


@pytest.mark.parametrize("dtype,H,M,bwd,pattern", grid(LN_PATTERNS, 5))
def test_ln_stream_fwd(dtype, H, M, bwd, pattern):
    outs, with_stats, eps = pattern
    torch.manual_seed(M * 11 + H + dtype)
    t = tdt(dtype)
    x = torch.randn(M, H, device=DEV) * 2 + 0.3
    x[torch.arange(M, device=DEV) % 3 == 1] += 50.0   # rows far from zero mean (a one-pass variance loses them)
    zero_row = M // 2 if M >= 3 else None
    if zero_row is not None:
        x[zero_row] = 0.0
    gamma, beta = 1.0 + 0.3 * torch.randn(H, device=DEV), 0.5 * torch.randn(H, device=DEV)
    y = nan(M, H) if outs in ("y", "both") else None
    y_lp = nan(M, H, dtype=t) if outs in ("lp", "both") else None
    stats = nan(M, 2) if with_stats == "stats" else None
    check(L().etp_ln_stream_fwd(dtype, ptr(x), ptr(gamma), ptr(beta), ptr(y), ptr(y_lp), ptr(stats), M, H, eps, stream()), "ln_stream_fwd")
    torch.cuda.synchronize()
    ref_y, ref_st = rr.ln_fwd(x.to(F64), gamma.to(F64), beta.to(F64), eps)
    rr.check_ln_fwd(y, y_lp, stats, ref_y, ref_st, zero_row, beta)
