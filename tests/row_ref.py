"""fp64 restatements of the fused row kernels and the comparators of their op-level tests (tests/test_row_kernels_gpu.py).

The restatements are built from oracle/planner_oracle.py's own `layer_norm` / `linear`; tests/test_row_ref_cpu.py pins each one to
the oracle's composite it restates, and tests/test_row_bounds_cpu.py shows that the comparators below can fail.

  pano_fwd / pano_bwd   forward_panorama vilmodel_cmt.py:695-711 from the img / dep projections on (embed.hip pano_embed_*)
  gmap_fwd / gmap_bwd   forward_navigation :728-730 (= GlobalMapEncoder.gmap_input_embedding)     (embed.hip gmap_embed_*)
  sap_fwd / sap_bwd     NextActionPrediction :651-661 after the ReLU, masked_fill_ :742-744          (embed.hip sap_tail_*)
  ln_fwd                BertLayerNorm :150-154, 189-193 on the fp32 stream, with its stats          (norm.hip ln_fwd_s)

Backward references go through autograd.  `stats` rows hold (mean, rstd = 1/sqrt(biased var + eps)) of each normalised row.

Comparators (each raises AssertionError and records its worst figure in WORST):
  close_fp32  max|got - ref| <= 2e-5 * max(1, max|ref|) per tensor, every element finite
  close_rstd  max|got - ref| / |ref| <= 1e-5
  close_bf16  |got - ref| <= ulp_bf16(ref) + 2e-5 * max|ref| per element (one bf16 ulp of the fp64 value), every element finite
  same_bits   bitwise equality (round-to-nearest-even copies, untouched buffers)
"""
import torch

from oracle import planner_oracle as po

F64 = torch.float64
EPS = 1e-12          # every LayerNorm of the fused embeddings and of the SAP head (vilmodel_cmt.py:59, 656, 702-708, 729)
FP32_REL = 2e-5
RSTD_REL = 1e-5
BF16_REL = 2e-5
# the order of etp_pano_embed_fwd's `params` / etp_pano_embed_bwd's `grads` (include/etpnav_hip.h)
PANO_NAMES = ("g_img", "b_img", "g_dep", "b_dep", "w_loc", "bias_loc", "g_loc", "b_loc", "nav_emb", "type1", "g_out", "b_out")

# worst figure seen per bound class: fp32 -> err / max(1, max|ref|); rstd -> relative; bf16 -> err in bf16 ulps of the fp64 value
WORST = {"fp32": (0.0, ""), "rstd": (0.0, ""), "bf16_ulps": (0.0, "")}


def _record(cls, value, name):
    if value > WORST[cls][0]:
        WORST[cls] = (value, name)


# ---- restatements ----------------------------------------------------------------------------------------------------------
def ln_stats(x, eps=EPS):
    """[..., 2]: mean and 1/sqrt(biased variance + eps) of each row (the `stats` rows of the kernels)."""
    mu = x.mean(-1, keepdim=True)
    var = ((x - mu) * (x - mu)).mean(-1, keepdim=True)
    return torch.cat([mu, 1.0 / torch.sqrt(var + eps)], -1)


def pano_fwd(a, d, loc, nav, p):
    """-> y [M, H], stats [M, 8] = (mean, rstd) of a, d, the angle projection and the branch sum.  `d` None: no depth
    branch (use_depth_embedding False, vilmodel_cmt.py:699-702); its stats columns are then NaN.  `p`: dict over PANO_NAMES
    (w_loc [H, 4], nav_emb [2, H])."""
    H = a.shape[-1]
    x = po.layer_norm(a, p["g_img"], p["b_img"], EPS)                                            # :698
    st = [ln_stats(a)]
    if d is not None:
        x = x + po.layer_norm(d, p["g_dep"], p["b_dep"], EPS)                                    # :699-702
        st.append(ln_stats(d))
    else:
        st.append(torch.full_like(st[0], float("nan")))
    lp = po.linear(loc, p["w_loc"].reshape(H, 4), p["bias_loc"])                                # :703-704
    x = x + po.layer_norm(lp, p["g_loc"], p["b_loc"], EPS) + p["nav_emb"].reshape(2, H)[nav] + p["type1"]   # :705-707
    st += [ln_stats(lp), ln_stats(x)]
    return po.layer_norm(x, p["g_out"], p["b_out"], EPS), torch.cat(st, -1)                   # :708-710


def pano_bwd(dy, a, d, loc, nav, p):
    """-> dict: da, dd (None without depth) and the gradient of every parameter in PANO_NAMES (zero for g_dep / b_dep
    without depth)."""
    a_ = a.detach().to(F64).requires_grad_(True)
    d_ = None if d is None else d.detach().to(F64).requires_grad_(True)
    q = {k: v.detach().to(F64).requires_grad_(True) for k, v in p.items()}
    y, _ = pano_fwd(a_, d_, loc.to(F64), nav, q)
    y.backward(dy.to(F64))
    out = {k: (q[k].grad if q[k].grad is not None else torch.zeros_like(q[k])) for k in PANO_NAMES}
    out["da"] = a_.grad
    out["dd"] = None if d_ is None else d_.grad
    return out


def gmap_fwd(img, step_ids, pos, step_emb, w_pos, b_pos, gamma, beta):
    """-> x [M, H], stats [M, 2] of the position projection."""
    lp = po.linear(pos, w_pos, b_pos)
    x = img + step_emb[step_ids] + po.layer_norm(lp, gamma, beta, EPS)
    return x, ln_stats(lp)


def gmap_bwd(dx, img, step_ids, pos, step_emb, w_pos, b_pos, gamma, beta):
    """-> dict: d_step_emb, d_w_pos, d_b_pos, dgamma, dbeta."""
    names = ("d_step_emb", "d_w_pos", "d_b_pos", "dgamma", "dbeta")
    q = [t.detach().to(F64).requires_grad_(True) for t in (step_emb, w_pos, b_pos, gamma, beta)]
    x, _ = gmap_fwd(img.to(F64), step_ids, pos.to(F64), *q)
    x.backward(dx.to(F64))
    return dict(zip(names, (t.grad for t in q)))


def sap_masked(M, visited, valid, device=None):
    """the rows the SAP tail sets to -inf (vilmodel_cmt.py:743-744); either mask may be None (not passed)."""
    m = torch.zeros(M, dtype=torch.bool, device=device)
    if visited is not None:
        m |= visited.bool()
    if valid is not None:
        m |= ~valid.bool()
    return m


def sap_fwd(r, gamma, beta, w2, b2, visited=None, valid=None):
    """r = relu(x.W1^T + b1) [M, H] -> logits [M], stats [M, 2] of r."""
    n = po.layer_norm(r, gamma, beta, EPS)                                                         # :656
    logit = po.linear(n, w2.reshape(1, -1), b2.reshape(1)).squeeze(-1)                           # :658
    return logit.masked_fill(sap_masked(r.shape[0], visited, valid, r.device), float("-inf")), ln_stats(r)


def sap_bwd(dlogits, r, gamma, beta, w2, b2, visited=None, valid=None):
    """-> dict: dz (gradient of the pre-ReLU input: d r * (r > 0)), dgamma, dbeta, dw2, db2.  dlogits of masked rows are
    ignored (masked_fill's backward drops them)."""
    r_ = r.detach().to(F64).requires_grad_(True)
    q = [t.detach().to(F64).requires_grad_(True) for t in (gamma, beta, w2, b2)]
    logit, _ = sap_fwd(r_, *q, visited=visited, valid=valid)
    masked = sap_masked(r.shape[0], visited, valid, r.device)
    logit.backward(torch.where(masked, torch.zeros_like(logit), dlogits.to(F64)))
    dz = r_.grad * (r_.detach() > 0)
    return dict(zip(("dz", "dgamma", "dbeta", "dw2", "db2"), (dz, *[t.grad for t in q])))


def ln_fwd(x, gamma, beta, eps):
    """-> y, stats [M, 2]."""
    return po.layer_norm(x, gamma, beta, eps), ln_stats(x, eps)


# ---- comparators -----------------------------------------------------------------------------------------------------------
def _f64(t):
    return t.detach().to(F64)


def close_fp32(name, got, ref, rel=FP32_REL):
    got, ref = _f64(got), _f64(ref)
    assert got.shape == ref.shape, (name, tuple(got.shape), tuple(ref.shape))
    assert bool(torch.isfinite(got).all()), f"{name}: {int((~torch.isfinite(got)).sum())} non-finite elements"
    scale = max(1.0, float(ref.abs().max())) if ref.numel() else 1.0
    err = float((got - ref).abs().max()) if ref.numel() else 0.0
    _record("fp32", err / scale, name)
    assert err <= rel * scale, f"{name}: max|got - ref| {err:.3e} > {rel:g} * {scale:.3g}"
    return err / scale


def close_rstd(name, got, ref, rel=RSTD_REL):
    got, ref = _f64(got), _f64(ref)
    assert bool(torch.isfinite(got).all()), f"{name}: non-finite rstd"
    err = float(((got - ref).abs() / ref.abs()).max())
    _record("rstd", err, name)
    assert err <= rel, f"{name}: relative error {err:.3e} > {rel:g}"
    return err


def ulp_bf16(ref):
    """one bf16 ulp at |ref| (8 significant bits): 2^(floor(log2|ref|) - 7); 0 where ref == 0."""
    _, e = torch.frexp(ref.abs())
    return torch.where(ref == 0, torch.zeros_like(ref), torch.ldexp(torch.ones_like(ref), (e - 8).to(torch.int32)))


def close_bf16(name, got, ref, rel=BF16_REL):
    """bf16 result without an fp32 twin: within one bf16 ulp of the fp64 value plus rel * max|ref|."""
    assert got.dtype == torch.bfloat16, (name, got.dtype)
    got, ref = _f64(got), _f64(ref)
    assert got.shape == ref.shape, (name, tuple(got.shape), tuple(ref.shape))
    assert bool(torch.isfinite(got).all()), f"{name}: {int((~torch.isfinite(got)).sum())} non-finite elements"
    ulp = ulp_bf16(ref)
    slack = rel * float(ref.abs().max())
    err = (got - ref).abs()
    ulps = float((torch.clamp(err - slack, min=0) / torch.where(ulp > 0, ulp, torch.ones_like(ulp))).max())
    _record("bf16_ulps", ulps, name)
    bad = err > ulp + slack
    assert not bool(bad.any()), f"{name}: {int(bad.sum())} elements beyond one bf16 ulp + {slack:.2e} (worst {ulps:.2f} ulps)"
    return ulps


def same_bits(name, got, want):
    assert got.dtype == want.dtype and got.shape == want.shape, (name, got.dtype, want.dtype)
    iv = {torch.float32: torch.int32, torch.bfloat16: torch.int16, torch.float64: torch.int64}[got.dtype]
    diff = got.contiguous().view(iv) != want.contiguous().view(iv)
    assert not bool(diff.any()), f"{name}: {int(diff.sum())} elements differ bitwise"


def rne_copy(name, lp, y):
    """lp must be the round-to-nearest-even copy of the kernel's own fp32 result y in lp's dtype."""
    same_bits(name, lp, y.to(lp.dtype))


def close_out(name, got, ref):
    """a row output stored in the operand dtype: bf16 bound for bf16, fp32 bound otherwise."""
    return close_bf16(name, got, ref) if got.dtype == torch.bfloat16 else close_fp32(name, got, ref)


def close_stats(name, got, ref, cols):
    """stats [M, k]: the mean columns against the fp32 bound, the rstd columns relative."""
    for c in cols:
        if c % 2 == 0:
            close_fp32(f"{name}[:, {c}] (mean)", got[:, c], ref[:, c])
        else:
            close_rstd(f"{name}[:, {c}] (rstd)", got[:, c], ref[:, c])


def accumulated(name, got, init, ref_grad):
    """a parameter gradient the kernel accumulates: got = init + ref."""
    return close_fp32(name, got, _f64(init) + _f64(ref_grad))


# ---- per-kernel checks (the GPU tests call these on the kernels' outputs; the CPU can-fail test on mutated references) -----
def check_pano_fwd(y, stats, ref_y, ref_stats, depth):
    """without depth, stats columns 2-3 are not written (they keep the NaN fill)"""
    close_fp32("pano y", y, ref_y)
    close_stats("pano stats", stats, ref_stats, (0, 1, 2, 3, 4, 5, 6, 7) if depth else (0, 1, 4, 5, 6, 7))
    if not depth:
        assert bool(torch.isnan(stats[:, 2:4]).all()), "pano stats[:, 2:4] written without depth"


def check_pano_bwd(da, dd, grads, init, ref, depth):
    """grads / init: lists in PANO_NAMES order (kernel result, buffer contents before the call)."""
    close_out("pano da", da, ref["da"])
    if depth:
        close_out("pano dd", dd, ref["dd"])
    for i, k in enumerate(PANO_NAMES):
        if not depth and k in ("g_dep", "b_dep"):
            same_bits(f"pano d{k} (no depth: untouched)", grads[i], init[i])
        else:
            accumulated(f"pano d{k}", grads[i], init[i], ref[k].reshape(-1))


def check_gmap_fwd(x, x_lp, stats, ref_x, ref_stats):
    close_fp32("gmap x", x, ref_x)
    if x_lp is not None:
        rne_copy("gmap x_lp", x_lp, x)
    close_stats("gmap stats", stats, ref_stats, (0, 1))


def check_gmap_bwd(got, init, ref, step_ids):
    """got / init / ref: dicts over d_step_emb, d_w_pos, d_b_pos, dgamma, dbeta.  Table rows no id names stay untouched."""
    named = torch.zeros(got["d_step_emb"].shape[0], dtype=torch.bool, device=step_ids.device)
    named[step_ids] = True
    named = named.to(got["d_step_emb"].device)
    same_bits("gmap d_step_emb (rows no id names)", got["d_step_emb"][~named], init["d_step_emb"][~named])
    accumulated("gmap d_step_emb", got["d_step_emb"], init["d_step_emb"], ref["d_step_emb"])
    for k in ("d_w_pos", "d_b_pos", "dgamma", "dbeta"):
        accumulated(f"gmap {k}", got[k], init[k], ref[k])


def check_sap_fwd(logits, stats, ref_logits, ref_stats, masked):
    lg = _f64(logits)
    assert bool(torch.isneginf(lg[masked]).all()), "sap logits: a masked row is not exactly -inf"
    assert bool(torch.isfinite(lg[~masked]).all()), "sap logits: an unmasked row is not finite"
    close_fp32("sap logits (unmasked rows)", lg[~masked], ref_logits[~masked])
    close_stats("sap stats", stats, ref_stats, (0, 1))


def check_sap_bwd(dz, got, init, ref, masked, r):
    """got / init / ref: dicts over dgamma, dbeta, dw2, db2.  dz exactly 0 on masked rows and where r == 0."""
    zero = masked[:, None] | (r == 0)
    assert bool((_f64(dz)[zero] == 0).all()), "sap dz: nonzero on a masked row or where r == 0"
    close_out("sap dz", dz, ref["dz"])
    for k in ("dgamma", "dbeta", "dw2", "db2"):
        accumulated(f"sap {k}", got[k], init[k], ref[k])


def check_ln_fwd(y, y_lp, stats, ref_y, ref_stats, zero_row, beta):
    """y and / or y_lp may be None (not passed).  The all-zero row comes out exactly beta."""
    if y is not None:
        close_fp32("ln y", y, ref_y)
        if zero_row is not None:
            same_bits("ln y (all-zero row)", y[zero_row], beta)
    if y_lp is not None:
        if y is not None:
            rne_copy("ln y_lp", y_lp, y)
        else:
            close_out("ln y_lp", y_lp, ref_y)
        if zero_row is not None:
            same_bits("ln y_lp (all-zero row)", y_lp[zero_row], beta.to(y_lp.dtype))
    if stats is not None:
        close_stats("ln stats", stats, ref_stats, (0, 1))
