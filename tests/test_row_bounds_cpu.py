"""The checks of tests/test_row_kernels_gpu.py must be ABLE TO FAIL.

These CPU tests run the per-kernel checks of tests/row_ref.py -- the ones every row-kernel GPU case calls -- on float64 reference
outputs stored in the kernels' output dtypes (bf16 mode) with 1e-6 relative noise, which must pass, and on mutations of them, each
of which must raise:
  * one bf16 element of da off by 2 ulps,
  * a bf16 copy truncated instead of rounded (gmap x_lp, LayerNorm y_lp),
  * the last row left NaN at M = 385 and at M = 257 (one row past the backward grid-stride trips),
  * one parameter gradient missing the last row's contribution,
  * the two nav_emb gradient rows swapped,
  * one masked logit finite,
  * a nonzero dz on a masked row.
"""
import functools

import pytest
import torch

from tests import row_ref as rr

F64 = torch.float64
BF = torch.bfloat16
H = 256


def _gen(seed):
    return torch.Generator().manual_seed(seed)


def noisy(ref, dtype, g):
    """the reference as a kernel would store it: 1e-6 relative noise, then rounded to the output dtype"""
    return (ref * (1.0 + 1e-6 * torch.randn(ref.shape, generator=g, dtype=F64))).to(dtype)


def truncated(x):
    """bf16 copy by truncation (the high 16 bits), not round-to-nearest-even"""
    return (x.contiguous().view(torch.int32) >> 16).to(torch.int16).view(BF)


@functools.lru_cache(maxsize=None)
def pano(M, depth=True):
    g = _gen(M)
    a = (torch.randn(M, H, generator=g, dtype=F64) * 2 + 0.3).to(BF).to(F64)
    d = (torch.randn(M, H, generator=g, dtype=F64) - 1.0).to(BF).to(F64) if depth else None
    loc = torch.randn(M, 4, generator=g, dtype=F64).float().to(F64)
    nav = torch.randint(0, 2, (M,), generator=g)
    sizes = [H, H, H, H, 4 * H, H, H, H, 2 * H, H, H, H]
    p = {k: torch.randn(n, generator=g, dtype=F64).float().to(F64) + (1.0 if k.startswith("g_") else 0.0)
         for k, n in zip(rr.PANO_NAMES, sizes)}
    dy = torch.randn(M, H, generator=g, dtype=F64).float().to(F64)
    ref_y, ref_st = rr.pano_fwd(a, d, loc, nav, p)
    ref = rr.pano_bwd(dy, a, d, loc, nav, p)
    init = [torch.randn(n, generator=g) for n in sizes]
    got = {"y": noisy(ref_y, torch.float32, g), "stats": noisy(ref_st, torch.float32, g),
           "da": noisy(ref["da"], BF, g), "dd": noisy(ref["dd"], BF, g) if depth else None,
           "grads": [(i.to(F64) + noisy(ref[k].reshape(-1), F64, g)).float() if depth or k not in ("g_dep", "b_dep") else i.clone()
                     for i, k in zip(init, rr.PANO_NAMES)]}
    return dict(a=a, d=d, loc=loc, nav=nav, p=p, dy=dy, ref_y=ref_y, ref_st=ref_st, ref=ref, init=init, got=got, depth=depth)


def check_pano(c, got=None):
    got = got or c["got"]
    rr.check_pano_fwd(got["y"], got["stats"], c["ref_y"], c["ref_st"], c["depth"])
    rr.check_pano_bwd(got["da"], got["dd"], got["grads"], c["init"], c["ref"], c["depth"])


def mutated(c, **kw):
    got = dict(c["got"])
    got["grads"] = list(got["grads"])
    got.update(kw)
    return got


@functools.lru_cache(maxsize=None)
def gmap(M):
    g = _gen(M + 1)
    img, pos = torch.randn(M, H, generator=g, dtype=F64), torch.randn(M, 7, generator=g, dtype=F64)
    ids = torch.randint(1, 40, (M,), generator=g)
    ids[::3] = 0
    w = [torch.randn(100, H, generator=g, dtype=F64), torch.randn(H, 7, generator=g, dtype=F64) * 0.3,
         torch.randn(H, generator=g, dtype=F64) * 0.1, torch.randn(H, generator=g, dtype=F64) + 1, torch.randn(H, generator=g, dtype=F64)]
    dx = torch.randn(M, H, generator=g, dtype=F64)
    ref_x, ref_st = rr.gmap_fwd(img, ids, pos, *w)
    ref = rr.gmap_bwd(dx, img, ids, pos, *w)
    init = {k: torch.randn(v.shape, generator=g) for k, v in ref.items()}
    x = noisy(ref_x, torch.float32, g)
    got = {"x": x, "x_lp": x.to(BF), "stats": noisy(ref_st, torch.float32, g),
           "grads": {k: (init[k].to(F64) + noisy(ref[k], F64, g)).float() for k in ref}}
    return dict(img=img, ids=ids, pos=pos, w=w, dx=dx, ref_x=ref_x, ref_st=ref_st, ref=ref, init=init, got=got)


def check_gmap(c, got=None):
    got = got or c["got"]
    rr.check_gmap_fwd(got["x"], got["x_lp"], got["stats"], c["ref_x"], c["ref_st"])
    rr.check_gmap_bwd(got["grads"], c["init"], c["ref"], c["ids"])


@functools.lru_cache(maxsize=None)
def sap(M):
    g = _gen(M + 2)
    r = torch.relu(torch.randn(M, H, generator=g, dtype=F64)).to(BF).to(F64)
    r[1::5] = 0
    p = [torch.randn(H, generator=g, dtype=F64) + 1, torch.randn(H, generator=g, dtype=F64),
         torch.randn(H, generator=g, dtype=F64) * 0.05, torch.randn(1, generator=g, dtype=F64)]
    vis = (torch.rand(M, generator=g) < 0.3).to(torch.uint8)
    val = (torch.rand(M, generator=g) < 0.8).to(torch.uint8)
    masked = rr.sap_masked(M, vis, val)
    ref_lg, ref_st = rr.sap_fwd(r, *p, visited=vis, valid=val)
    dl = torch.randn(M, generator=g, dtype=F64)
    dl[masked] = float("nan")
    ref = rr.sap_bwd(dl, r, *p, visited=vis, valid=val)
    init = {k: torch.randn(ref[k].shape, generator=g) for k in ("dgamma", "dbeta", "dw2", "db2")}
    got = {"logits": noisy(ref_lg, torch.float32, g), "stats": noisy(ref_st, torch.float32, g), "dz": noisy(ref["dz"], BF, g),
           "grads": {k: (init[k].to(F64) + noisy(ref[k], F64, g)).float() for k in init}}
    unmasked_lg, _ = rr.sap_fwd(r, *p)
    return dict(r=r, masked=masked, ref_lg=ref_lg, ref_st=ref_st, ref=ref, init=init, got=got, unmasked_lg=unmasked_lg)


def check_sap(c, got=None):
    got = got or c["got"]
    rr.check_sap_fwd(got["logits"], got["stats"], c["ref_lg"], c["ref_st"], c["masked"])
    rr.check_sap_bwd(got["dz"], got["grads"], c["init"], c["ref"], c["masked"], c["r"])


@functools.lru_cache(maxsize=None)
def ln(M):
    g = _gen(M + 3)
    x = (torch.randn(M, H, generator=g, dtype=F64) * 2 + 0.3).float().to(F64)
    x[1::3] += 50.0
    x[M // 2] = 0.0
    gamma, beta = torch.randn(H, generator=g) + 1, torch.randn(H, generator=g)
    ref_y, ref_st = rr.ln_fwd(x, gamma.to(F64), beta.to(F64), 1e-5)
    y = noisy(ref_y, torch.float32, g)
    y[M // 2] = beta
    return dict(ref_y=ref_y, ref_st=ref_st, beta=beta, zero=M // 2, got={"y": y, "y_lp": y.to(BF), "stats": noisy(ref_st, torch.float32, g)})


def check_ln(c, got=None):
    got = got or c["got"]
    rr.check_ln_fwd(got["y"], got["y_lp"], got["stats"], c["ref_y"], c["ref_st"], c["zero"], c["beta"])


@pytest.mark.parametrize("M", [385, 257])
def test_row_checks_accept_reference_outputs_with_small_noise(M):
    check_pano(pano(M, depth=True))
    check_pano(pano(M, depth=False))
    check_gmap(gmap(M))
    check_sap(sap(M))
    check_ln(ln(M))
    lp_alone = ln(M)["got"]["y"].to(F64).to(BF)            # a lone bf16 output against the one-ulp bound
    rr.check_ln_fwd(None, lp_alone, None, ln(M)["ref_y"], None, ln(M)["zero"], ln(M)["beta"])


def test_check_rejects_bf16_element_two_ulps_off():
    c = pano(385)
    da = c["got"]["da"].clone()
    i = int(c["ref"]["da"].abs().argmax())
    da.view(-1).view(torch.int16)[i] += 2
    with pytest.raises(AssertionError):
        check_pano(c, mutated(c, da=da))


def test_check_rejects_truncated_bf16_copies():
    c = gmap(385)
    got = dict(c["got"], x_lp=truncated(c["got"]["x"]))
    with pytest.raises(AssertionError):
        check_gmap(c, got)
    c = ln(385)
    with pytest.raises(AssertionError):
        check_ln(c, dict(c["got"], y_lp=truncated(c["got"]["y"])))


@pytest.mark.parametrize("M", [385, 257])
@pytest.mark.parametrize("what", ["pano y", "pano stats", "pano da", "gmap x", "sap logits", "sap dz", "ln y", "ln y_lp"])
def test_check_rejects_last_row_left_nan(M, what):
    kernel, out = what.split()
    c = {"pano": pano, "gmap": gmap, "sap": sap, "ln": ln}[kernel](M)
    t = c["got"][out].clone()
    t[-1] = float("nan")
    got = dict(c["got"], **{out: t})
    if kernel == "sap" and out == "logits":
        assert not bool(c["masked"][-1]), "the last row of this sample must be unmasked"
    with pytest.raises(AssertionError):
        {"pano": check_pano, "gmap": check_gmap, "sap": check_sap, "ln": check_ln}[kernel](c, got)


def test_check_rejects_gradient_missing_the_last_row():
    c = pano(385)
    dy = c["dy"].clone()
    dy[-1] = 0.0
    short = rr.pano_bwd(dy, c["a"], c["d"], c["loc"], c["nav"], c["p"])
    i = rr.PANO_NAMES.index("g_out")
    got = mutated(c)
    got["grads"][i] = (c["init"][i].to(F64) + short["g_out"]).float()
    with pytest.raises(AssertionError):
        check_pano(c, got)
    c = gmap(257)
    grads = dict(c["got"]["grads"])
    dx = c["dx"].clone()
    dx[-1] = 0.0
    short = rr.gmap_bwd(dx, c["img"], c["ids"], c["pos"], *c["w"])
    grads["d_w_pos"] = (c["init"]["d_w_pos"].to(F64) + short["d_w_pos"]).float()
    with pytest.raises(AssertionError):
        check_gmap(c, dict(c["got"], grads=grads))


def test_check_rejects_swapped_nav_emb_gradient_rows():
    c = pano(385)
    i = rr.PANO_NAMES.index("nav_emb")
    got = mutated(c)
    gn = got["grads"][i]
    got["grads"][i] = torch.cat([gn[H:], gn[:H]])
    with pytest.raises(AssertionError):
        check_pano(c, got)


def test_check_rejects_a_finite_masked_logit():
    c = sap(257)
    k = int(torch.nonzero(c["masked"])[0])
    lg = c["got"]["logits"].clone()
    lg[k] = float(c["unmasked_lg"][k])
    with pytest.raises(AssertionError):
        check_sap(c, dict(c["got"], logits=lg))


def test_check_rejects_nonzero_dz_on_a_masked_row():
    c = sap(257)
    k = int(torch.nonzero(c["masked"] & (c["r"] > 0).any(1))[0])      # a masked row that is not all zero
    dz = c["got"]["dz"].clone()
    col = int(torch.nonzero(c["r"][k] > 0)[0])
    dz[k, col] = 1e-3
    with pytest.raises(AssertionError):
        check_sap(c, dict(c["got"], dz=dz))
