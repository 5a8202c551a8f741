"""Pins tests/drop_ref.py without a GPU.

  the generator        drop_ref.mult against the oracle's DropSpec.mult and the library's etp_dropout_multipliers, bit for bit, at
                       p in {1e-6, 0.1, 0.4, 0.5}, several seeds and sites, n even and odd; drop_ref.mult_runs (drop_mult_run's two
                       branches) against the per-element form from even and odd starts; Site.rows / Site.flat against the flat list
  the restatements     each against the oracle block that takes `drop`, with the same DropSpec, forward and every gradient, at 1e-12:
                         text embedding      planner_oracle.forward_txt without encoder layers        (MODE_TXT, 0, SITE_EMBED)
                         panorama embedding  forward_panorama without encoder layers, identity views   (MODE_PANO, 0, SITE_EMBED)
                         SAP tail            forward_navigation without x-layers (test_row_ref_cpu's)  (MODE_NAV, 0, SITE_HEAD)
                         ln_bwd_s            x + _drop(dense) -> layer_norm (BertSelfOutput / BertOutput): d dense = dx * multiplier
                         cast_drop           forward_panorama's drop_env: _drop on the RGB features    (MODE_PANO, 0, SITE_ENV)
"""
import ctypes

import numpy as np
import pytest
import torch

from etpnav_amd import _lib
from oracle import planner_oracle as po
from tests import drop_ref as dr
from tests import reduce_ref as rf
from tests import row_ref as rr

F64 = torch.float64
TOL = 1e-12


def rel(a, b):
    return float((a - b).abs().max()) / max(1.0, float(b.abs().max()))


# ---- the generator -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("p", [1e-6, 0.1, 0.4, 0.5])
def test_multipliers_match_oracle_and_library(p):
    L = _lib.lib()
    for seed in (0, 1, dr.SEED, 2 ** 63 + 5, 2 ** 64 - 1):
        for (mode, layer, slot) in ((1, 0, 0), (3, 3, 7), (2, 11, 15), (4, 0, 5)):
            for n in (1, 10, 11, 1027):
                got = dr.mult(p, seed, mode, layer, slot, n)
                oracle = po.DropSpec(p, seed=seed).mult(p, mode, layer, slot, (n,)).numpy()
                lib = np.empty(n, dtype=np.float32)
                assert L.etp_dropout_multipliers(ctypes.c_float(p), seed, mode, layer, slot, n, lib.ctypes.data) == 0
                assert got.tobytes() == oracle.tobytes() == lib.tobytes(), (p, seed, mode, layer, slot, n)
                assert set(np.unique(got)) <= {np.float32(0.0), dr.inv_keep(p)}
    if p == 1e-6:
        assert dr.threshold(p) == 0 and bool((got > 1.0).all())          # nothing dropped, everything scaled


@pytest.mark.parametrize("N", [4, 8])
def test_runs_match_the_per_element_form(N):
    site = dr.Site(0.4, dr.SITES[1])
    starts = np.arange(0, 301)                                            # even and odd starts
    want = dr.mult_at(0.4, site.sseed, starts[:, None] + np.arange(N)[None])
    assert (dr.mult_runs(0.4, site.sseed, starts, N) == want).all()
    wrong = dr.mult_runs(0.4, site.sseed, starts, N, odd_as_even=True)
    assert (wrong[0::2] == want[0::2]).all() and (wrong[1::2] != want[1::2]).any()


def test_site_rows_is_the_flat_list():
    site = dr.Site(0.1, dr.SITES[1])
    flat = torch.from_numpy(dr.mult(0.1, dr.SEED, *dr.SITES[1], 7 * 256))
    assert torch.equal(site.rows(7, 256).reshape(-1), flat) and torch.equal(site.flat(7 * 256), flat)
    assert torch.equal(dr.Site(0.0, dr.SITES[0]).rows(3, 256), torch.ones(3, 256))
    assert 0.05 < float((flat == 0).double().mean()) < 0.15


# ---- the restatements ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("p", dr.RATES)
def test_text_restatement_matches_forward_txt(p):
    site = dr.Site(p, (po.MODE_TXT, 0, po.SITE_EMBED))
    B, Lt, H = 3, 9, 256
    c = dr.text_case(B, Lt, H, site, seed=1)
    cfg = po.PlannerConfig.r2r(hidden_size=H, vocab_size=rf.TEXT_VOCAB, num_l_layers=0)
    names = ("embeddings.word_embeddings.weight", "embeddings.position_embeddings.weight", "embeddings.token_type_embeddings.weight",
             "embeddings.LayerNorm.weight", "embeddings.LayerNorm.bias")
    type_table = torch.stack([c["type0"].to(F64), torch.zeros(H, dtype=F64)])
    P = dict(zip(names, (c["word"].to(F64), c["pos"].to(F64), type_table, c["gamma"].to(F64), c["beta"].to(F64))))
    P = {k: v.clone().requires_grad_(True) for k, v in P.items()}
    want = po.forward_txt(P, cfg, c["ids"], torch.ones(B, Lt, dtype=torch.bool), site.spec("p_hidden"))
    want.backward(c["dy"].to(F64))
    assert rel(c["y"], want.detach().reshape(B * Lt, H)) < TOL
    r = dr.text_backward(c, round_product=False)["ref"]
    gw = P[names[0]].grad.clone()
    gw[0] = 0                                                             # padding_idx 0 (test_reduce_ref_cpu)
    for k, g in (("dword", gw), ("dpos", P[names[1]].grad), ("dtype0", P[names[2]].grad[0]), ("dgamma", P[names[3]].grad),
                 ("dbeta", P[names[4]].grad)):
        assert rel(r[k], g) < TOL, k
    assert rel(dr.text_backward(c)["ref"]["dbeta"], r["dbeta"]) < 2 * dr.U    # the rounded product: one fp32 rounding per term


@pytest.mark.parametrize("depth", [True, False])
def test_pano_restatement_matches_forward_panorama(depth):
    site = dr.Site(0.4 if depth else 0.1, (po.MODE_PANO, 0, po.SITE_EMBED))
    B, V, H = 3, 5, 256
    M = B * V
    c = dr.pano_case(M, H, depth, torch.float32, site, seed=2)
    cfg = po.PlannerConfig(hidden_size=H, num_pano_layers=0, image_feat_size=H, depth_feat_size=H, use_depth_embedding=depth)
    e = "img_embeddings"
    keys = {"g_img": f"{e}.img_layer_norm.weight", "b_img": f"{e}.img_layer_norm.bias", "g_dep": f"{e}.dep_layer_norm.weight",
            "b_dep": f"{e}.dep_layer_norm.bias", "w_loc": f"{e}.loc_linear.weight", "bias_loc": f"{e}.loc_linear.bias",
            "g_loc": f"{e}.loc_layer_norm.weight", "b_loc": f"{e}.loc_layer_norm.bias", "nav_emb": f"{e}.nav_type_embedding.weight",
            "g_out": f"{e}.layer_norm.weight", "b_out": f"{e}.layer_norm.bias"}
    shapes = {"w_loc": (H, 4), "nav_emb": (2, H)}
    P = {v: c["p64"][k].reshape(shapes.get(k, (H,))) for k, v in keys.items() if depth or k not in ("g_dep", "b_dep")}
    P[f"{e}.img_linear.weight"], P[f"{e}.img_linear.bias"] = torch.eye(H, dtype=F64), torch.zeros(H, dtype=F64)
    if depth:
        P[f"{e}.dep_linear.weight"], P[f"{e}.dep_linear.bias"] = torch.eye(H, dtype=F64), torch.zeros(H, dtype=F64)
    P["embeddings.token_type_embeddings.weight"] = torch.stack([torch.zeros(H, dtype=F64), c["p64"]["type1"]])
    P = {k: v.clone().requires_grad_(True) for k, v in P.items()}
    a_ = c["a"].to(F64).reshape(B, V, H).requires_grad_(True)
    d_ = c["d"].to(F64).reshape(B, V, H).requires_grad_(True) if depth else torch.zeros(B, V, H, dtype=F64)
    want, _ = po.forward_panorama(P, cfg, a_, d_, c["loc"].to(F64).reshape(B, V, 4), c["nav"].reshape(B, V), torch.full((B,), V),
                                  site.spec("p_hidden"))
    want.backward(c["dy"].to(F64).reshape(B, V, H))
    assert rel(c["y"], want.detach().reshape(M, H)) < TOL
    r = dr.pano_backward(c, round_product=False)
    assert rel(r["da"], a_.grad.reshape(M, H)) < TOL
    if depth:
        assert rel(r["dd"], d_.grad.reshape(M, H)) < TOL
    for k, v in keys.items():
        if v in P:
            assert rel(r[k].reshape(-1), P[v].grad.reshape(-1)) < TOL, k
    assert rel(r["type1"], P["embeddings.token_type_embeddings.weight"].grad[1]) < TOL


@pytest.mark.parametrize("pattern", ["null", "both"])
def test_sap_restatement_matches_forward_navigation_head(pattern):
    site = dr.Site(0.4, (po.MODE_NAV, 0, po.SITE_HEAD))
    B, G, H = 3, 5, 256
    M = B * G
    c = dr.sap_case(M, H, pattern, torch.float32, site, seed=3)
    cfg = po.PlannerConfig(hidden_size=H, num_x_layers=0, graph_sprels=False)
    k = "global_encoder"
    z = lambda *s: torch.zeros(*s, dtype=F64)       # noqa: E731
    P = {f"{k}.gmap_pos_embeddings.0.weight": z(H, 7), f"{k}.gmap_pos_embeddings.0.bias": z(H), f"{k}.gmap_pos_embeddings.1.weight": z(H),
         f"{k}.gmap_pos_embeddings.1.bias": z(H), f"{k}.gmap_step_embeddings.weight": z(100, H),
         "global_sap_head.net.0.weight": torch.eye(H, dtype=F64), "global_sap_head.net.0.bias": z(H),
         "global_sap_head.net.2.weight": c["gamma"].to(F64), "global_sap_head.net.2.bias": c["beta"].to(F64),
         "global_sap_head.net.4.weight": c["w2"].to(F64).reshape(1, H), "global_sap_head.net.4.bias": c["b2"].to(F64)}
    P = {n: v.clone().requires_grad_(True) for n, v in P.items()}
    r_ = c["r"].to(F64).reshape(B, G, H).requires_grad_(True)
    vis = torch.zeros(B, G, dtype=torch.bool) if c["vis"] is None else c["vis"].bool().reshape(B, G)
    val = torch.ones(B, G, dtype=torch.bool) if c["val"] is None else c["val"].bool().reshape(B, G)
    out = po.forward_navigation(P, cfg, z(B, 4, H), torch.ones(B, 4, dtype=torch.bool), torch.zeros(B, G, dtype=torch.long), r_,
                                z(B, G, 7), val, vis, z(B, G, G), site.spec("p_head"))["global_logits"]
    dl = c["dl"].to(F64).reshape(B, G)
    out.backward(torch.where(torch.isfinite(out), dl, torch.zeros_like(dl)))
    lg, _ = dr.sap_forward(c)
    fin = torch.isfinite(lg)
    assert torch.equal(fin, torch.isfinite(out.detach().reshape(M))) and bool((~fin).any()) == (pattern == "both")
    assert rel(lg[fin], out.detach().reshape(M)[fin]) < TOL
    r = dr.sap_backward(c)
    assert rel(r["dz"], r_.grad.reshape(M, H)) < TOL
    for name, key in (("dgamma", "net.2.weight"), ("dbeta", "net.2.bias"), ("dw2", "net.4.weight"), ("db2", "net.4.bias")):
        assert rel(r[name].reshape(-1), P[f"global_sap_head.{key}"].grad.reshape(-1)) < TOL, name


def test_ln_operand_copy_is_the_gradient_of_the_dropped_dense():
    site = dr.Site(0.1, (po.MODE_TXT, 2, po.SITE_FFN_O))
    M, H = 7, 256
    g = torch.Generator().manual_seed(4)
    x, dense, dy = (torch.randn(M, H, generator=g, dtype=F64) for _ in range(3))
    gamma, beta = 1.0 + 0.3 * torch.randn(H, generator=g, dtype=F64), torch.randn(H, generator=g, dtype=F64)
    x_, dense_ = x.clone().requires_grad_(True), dense.clone().requires_grad_(True)
    s = x_ + po._drop(dense_, site.spec("p_hidden"), "p_hidden", site.mode, site.layer, site.slot)      # BertOutput :191-192
    po.layer_norm(s, gamma, beta, 1e-12).backward(dy)
    dx, _, _ = rf.ln_bwd(dy, s.detach(), gamma, 1e-12)
    assert rel(dx, x_.grad) < TOL                                                  # dx (the residual stream) is undropped
    assert rel(dx * site.rows(M, H).to(F64), dense_.grad) < TOL                     # dx_lp = dx * multiplier


def test_cast_restatement_matches_drop_env():
    site = dr.Site(0.4, (po.MODE_PANO, 0, po.SITE_ENV))
    src = dr.cast_case(1028, seed=5).to(F64).reshape(4, 257)
    want = po._drop(src, site.spec("p_env"), "p_env", po.MODE_PANO, 0, po.SITE_ENV)
    assert torch.equal(src * site.flat(1028).to(F64).reshape(4, 257), want)


# ---- GEMM epilogue -------------------------------------------------------------------------------------------------------------
from tests import gemm_ref as gr  # noqa: E402


@pytest.mark.parametrize("comp", dr.GEMM_COMPS)
def test_gemm_restatement_without_a_mask_is_gemm_ref(comp):
    c = dr.gemm_case(65, 72, 160, True, comp, seed=1)
    val, E = dr.gemm_ref(c, torch.ones(65, 72))
    want, Ew = gr.gemm_ref(c["A"], c["B"], alpha=c["alpha"], bias=c["bias"], R=c["R"], Z=c["Z"], act=c["act"], bf16=True, c_bf16=c["c_bf16"])
    for n in want:
        assert torch.equal(val[n], want[n]), n
        act = want[n] - (c["R"].to(F64) if (n == "C" and c["R"] is not None) else 0)        # the multiply's rounding is the only addition
        assert bool((E[n] >= Ew[n]).all()) and bool((E[n] <= Ew[n] * (1 + 1e-6) + 1.0001 * dr.U * act.abs()).all()), n


def test_gemm_restatements_match_the_oracle_blocks():
    """bias + mask + residual: x + _drop(linear(h)) (BertOutput :191-192, transformer.py:181); GELU + mask with Z = gelu'(v)
    undropped: _drop(gelu_erf(linear(f))) (transformer.py:180) and its autograd, which IS the MUL_Z composition:
    dv = m * gelu'(v) * dh"""
    site = dr.Site(0.4, (po.MODE_PANO, 1, po.SITE_FFN_I))
    M, N, K = 9, 24, 16
    g = torch.Generator().manual_seed(6)
    A, W, b = torch.randn(M, K, generator=g, dtype=F64), torch.randn(N, K, generator=g, dtype=F64), torch.randn(N, generator=g, dtype=F64)
    x, dh = torch.randn(M, N, generator=g, dtype=F64), torch.randn(M, N, generator=g, dtype=F64)
    m = site.rows(M, N)
    spec = site.spec("p_hidden")
    base = dict(M=M, N=N, K=K, bf16=False, c_bf16=False, alpha=1.0, A=A, B=W, bias=b, out_mode=0, C0=None)
    want = x + po._drop(po.linear(A, W, b), spec, "p_hidden", site.mode, site.layer, site.slot)
    val, _ = dr.gemm_ref(dict(base, act=gr.ACT_NONE, R=x, Z=None, comp="bias_res"), m)
    assert rel(val["C"], want) < TOL
    v = po.linear(A, W, b).requires_grad_(True)
    h = po._drop(po.gelu_erf(v), spec, "p_hidden", site.mode, site.layer, site.slot)
    h.backward(dh)
    val, _ = dr.gemm_ref(dict(base, act=gr.ACT_GELU_SAVEGRAD, R=None, Z=None, comp="savegrad"), m)
    assert rel(val["C"], h.detach()) < TOL
    z = val["Z"]                                                                 # gelu'(v), undropped
    assert rel(z, torch.autograd.functional.jvp(po.gelu_erf, v.detach(), torch.ones_like(v))[1]) < TOL
    # MUL_Z: the product here is dh itself (A = dh, B = identity, no bias)
    dgrad = dict(base, K=N, A=dh, B=torch.eye(N, dtype=F64), bias=torch.zeros(N, dtype=F64), act=gr.ACT_MUL_Z, R=None, Z=z, comp="mul_z")
    assert rel(dr.gemm_ref(dgrad, m)[0]["C"], v.grad) < TOL


# ---- attention -----------------------------------------------------------------------------------------------------------------
from tests import attn_ref as ar  # noqa: E402


@pytest.mark.parametrize("mask_mode,with_dist", [(0, True), (1, False)])
def test_attention_restatement_without_a_mask_is_attn_ref(mask_mode, with_dist):
    c = dr.attn_case(21, 37, 2, 3, True, mask_mode, with_dist, seed=1)
    val, E = dr.attn_ref(c, torch.ones(2, 3, 21, 37))
    want, Ew = ar.ref_of(c)
    for n in want:
        assert torch.equal(val[n], want[n]), n
        assert bool((E[n] >= Ew[n]).all()) and bool((E[n] <= Ew[n] * (1 + 1e-4)).all()), n       # + the multiply's 2^-24 terms


@pytest.mark.parametrize("mask_mode,with_dist", [(0, True), (1, False), (0, False)])
def test_attention_restatement_matches_bert_attention_core(mask_mode, with_dist):
    """oracle: probs = _drop(softmax(...), p_attn, site); ctx = probs V (vilmodel_cmt.py:127 / :346), gradients by autograd"""
    site = dr.Site(0.4, (po.MODE_NAV, 2, po.SITE_X_P))
    B, nh, Lq, Lk = 2, 3, 21, 37
    c = dr.attn_case(Lq, Lk, B, nh, False, mask_mode, with_dist, seed=2)
    m = dr.attn_index_mask(site, B, nh, Lq, Lk)
    assert torch.equal(m.reshape(-1), site.flat(B * nh * Lq * Lk))                      # row-major over [B, heads, Lq, Lk]
    q, k, v = (ar.merge_heads(c[n].to(F64)).reshape(B, -1, nh * 64).requires_grad_(True) for n in ("q", "k", "v"))
    if mask_mode == 0:
        add = po.extend_neg_masks(c["km"], F64)
    else:
        add = torch.zeros(B, 1, 1, Lk, dtype=F64).masked_fill(~c["km"][:, None, None, :], float("-inf"))
    w, b0 = torch.tensor(c["sp_w"], dtype=F64, requires_grad=True), torch.tensor(c["sp_b"], dtype=F64, requires_grad=True)
    if with_dist:
        add = add + (c["dist"].to(F64) * w + b0)[:, None]
    ctx = po.bert_attention_core(q * (c["alpha"] * 8.0), k, v, add, nh, site.spec("p_attn"), (site.mode, site.layer, site.slot))
    ctx.backward(ar.merge_heads(c["dctx"].to(F64)).reshape(B, -1, nh * 64))
    want = {"ctx": ctx.detach(), "dQ": q.grad, "dK": k.grad, "dV": v.grad}
    want = {n: ar.split_heads(t.reshape(-1, nh * 64), B, nh) for n, t in want.items()}
    val, _ = dr.attn_ref(c, m)
    for n, t in want.items():
        assert float((val[n] - t).abs().max()) <= TOL * max(1.0, float(t.abs().max())), n
    if with_dist:
        assert abs(float(val["d_sp_w"] - w.grad)) <= TOL * B * nh * Lq and abs(float(val["d_sp_b"] - b0.grad)) <= TOL * B * nh * Lq
