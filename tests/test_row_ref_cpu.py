"""The fp64 restatements of tests/row_ref.py are the oracle's operations: each is pinned here, on random inputs, to the oracle
composite it restates (oracle/planner_oracle.py), forward and every gradient, in float64 on the CPU.

  pano_fwd / pano_bwd  forward_panorama with num_pano_layers = 0, image_feat_size = depth_feat_size = hidden, identity
                       img_linear / dep_linear with zero biases (so a = rgb_fts, d = dep_fts), with and without depth
  gmap_fwd / gmap_bwd  gmap_input_embedding
  sap_fwd / sap_bwd    forward_navigation with num_x_layers = 0: zero step table and a zero position LayerNorm make its input
                       x = gmap_img_fts = r, and the square net.0 with identity weight and zero bias gives relu(r) = r
  ln_fwd               F.layer_norm and torch.var_mean
"""
import pytest
import torch

from oracle import planner_oracle as po
from tests import row_ref as rr

F64 = torch.float64
TOL = 1e-10


def _close(a, b, what):
    assert a.shape == b.shape, what
    assert torch.equal(torch.isfinite(a), torch.isfinite(b)), what
    fin = torch.isfinite(b)
    err = float((a[fin] - b[fin]).abs().max()) if bool(fin.any()) else 0.0
    assert err <= TOL * max(1.0, float(b[fin].abs().max())), (what, err)


def _rand(g, *shape, scale=1.0, shift=0.0):
    return torch.randn(*shape, generator=g, dtype=F64) * scale + shift


@pytest.mark.parametrize("depth", [True, False])
def test_pano_restatement_matches_forward_panorama(depth):
    g = torch.Generator().manual_seed(11 + depth)
    H, B, V = 256, 3, 5
    cfg = po.PlannerConfig(hidden_size=H, num_pano_layers=0, image_feat_size=H, depth_feat_size=H, use_depth_embedding=depth)
    e = "img_embeddings"
    P = {f"{e}.img_linear.weight": torch.eye(H, dtype=F64), f"{e}.img_linear.bias": torch.zeros(H, dtype=F64),
         f"{e}.img_layer_norm.weight": _rand(g, H, scale=0.3, shift=1.0), f"{e}.img_layer_norm.bias": _rand(g, H, scale=0.5),
         f"{e}.loc_linear.weight": _rand(g, H, 4), f"{e}.loc_linear.bias": _rand(g, H, scale=0.5),
         f"{e}.loc_layer_norm.weight": _rand(g, H, scale=0.3, shift=1.0), f"{e}.loc_layer_norm.bias": _rand(g, H, scale=0.5),
         f"{e}.nav_type_embedding.weight": _rand(g, 2, H), f"{e}.layer_norm.weight": _rand(g, H, scale=0.3, shift=1.0),
         f"{e}.layer_norm.bias": _rand(g, H, scale=0.5), "embeddings.token_type_embeddings.weight": _rand(g, 2, H)}
    if depth:
        P.update({f"{e}.dep_linear.weight": torch.eye(H, dtype=F64), f"{e}.dep_linear.bias": torch.zeros(H, dtype=F64),
                  f"{e}.dep_layer_norm.weight": _rand(g, H, scale=0.3, shift=1.0),
                  f"{e}.dep_layer_norm.bias": _rand(g, H, scale=0.5)})
    names = {"g_img": f"{e}.img_layer_norm.weight", "b_img": f"{e}.img_layer_norm.bias",
             "g_dep": f"{e}.dep_layer_norm.weight", "b_dep": f"{e}.dep_layer_norm.bias",
             "w_loc": f"{e}.loc_linear.weight", "bias_loc": f"{e}.loc_linear.bias",
             "g_loc": f"{e}.loc_layer_norm.weight", "b_loc": f"{e}.loc_layer_norm.bias",
             "nav_emb": f"{e}.nav_type_embedding.weight", "g_out": f"{e}.layer_norm.weight", "b_out": f"{e}.layer_norm.bias"}
    rgb = _rand(g, B, V, H, scale=2.0, shift=0.3)
    dep = _rand(g, B, V, H, scale=0.5, shift=-1.0)
    loc = _rand(g, B, V, 4)
    nav = torch.randint(0, 2, (B, V), generator=g)
    view_lens = torch.full((B,), V)
    # the oracle, with gradients of every parameter and of the two projected inputs
    Pg = {k: v.clone().requires_grad_(True) for k, v in P.items()}
    rgb_, dep_ = rgb.clone().requires_grad_(True), dep.clone().requires_grad_(True)
    y_or, _ = po.forward_panorama(Pg, cfg, rgb_, dep_, loc, nav, view_lens)
    dy = _rand(g, B, V, H)
    y_or.backward(dy)
    # the restatement on flat rows
    M = B * V
    p = {k: (P[v] if v in P else torch.zeros(H, dtype=F64)) for k, v in names.items()}
    p["type1"] = P["embeddings.token_type_embeddings.weight"][1]
    a, d = rgb.reshape(M, H), dep.reshape(M, H) if depth else None
    y, st = rr.pano_fwd(a, d, loc.reshape(M, 4), nav.reshape(M), p)
    _close(y, y_or.detach().reshape(M, H), "pano y")
    for c, t in ((0, a), (4, po.linear(loc.reshape(M, 4), p["w_loc"], p["bias_loc"]))):
        _close(st[:, c], t.mean(-1), f"stats {c}")
        _close(st[:, c + 1], 1 / torch.sqrt(t.var(-1, unbiased=False) + 1e-12), f"stats {c + 1}")
    assert bool(torch.isnan(st[:, 2:4]).all()) != depth
    ref = rr.pano_bwd(dy.reshape(M, H), a, d, loc.reshape(M, 4), nav.reshape(M), p)
    _close(ref["da"], rgb_.grad.reshape(M, H), "da")
    if depth:
        _close(ref["dd"], dep_.grad.reshape(M, H), "dd")
    for k, v in names.items():
        if v in P:
            _close(ref[k], Pg[v].grad, k)
        else:
            assert bool((ref[k] == 0).all()), k
    _close(ref["type1"], Pg["embeddings.token_type_embeddings.weight"].grad[1], "type1")


def test_gmap_restatement_matches_gmap_input_embedding():
    g = torch.Generator().manual_seed(5)
    H, B, G = 256, 3, 7
    cfg = po.PlannerConfig(hidden_size=H)
    k = "global_encoder"
    P = {f"{k}.gmap_pos_embeddings.0.weight": _rand(g, H, 7, scale=0.3), f"{k}.gmap_pos_embeddings.0.bias": _rand(g, H, scale=0.1),
         f"{k}.gmap_pos_embeddings.1.weight": _rand(g, H, scale=0.3, shift=1.0),
         f"{k}.gmap_pos_embeddings.1.bias": _rand(g, H, scale=0.5), f"{k}.gmap_step_embeddings.weight": _rand(g, 100, H)}
    img = _rand(g, B, G, H)
    ids = torch.randint(0, 100, (B, G), generator=g)
    ids[0, :3] = 0
    ids[1, :2] = ids[2, :2] = 99
    pos = _rand(g, B, G, 7)
    Pg = {n: v.clone().requires_grad_(True) for n, v in P.items()}
    x_or = po.gmap_input_embedding(Pg, cfg, img, ids, pos)
    dx = _rand(g, B, G, H)
    x_or.backward(dx)
    M = B * G
    args = (img.reshape(M, H), ids.reshape(M), pos.reshape(M, 7), P[f"{k}.gmap_step_embeddings.weight"],
            P[f"{k}.gmap_pos_embeddings.0.weight"], P[f"{k}.gmap_pos_embeddings.0.bias"], P[f"{k}.gmap_pos_embeddings.1.weight"],
            P[f"{k}.gmap_pos_embeddings.1.bias"])
    x, st = rr.gmap_fwd(*args)
    _close(x, x_or.detach().reshape(M, H), "gmap x")
    lp = po.linear(pos.reshape(M, 7), P[f"{k}.gmap_pos_embeddings.0.weight"], P[f"{k}.gmap_pos_embeddings.0.bias"])
    _close(st[:, 0], lp.mean(-1), "mean")
    _close(st[:, 1], 1 / torch.sqrt(lp.var(-1, unbiased=False) + 1e-12), "rstd")
    ref = rr.gmap_bwd(dx.reshape(M, H), *args)
    for name, key in (("d_step_emb", "gmap_step_embeddings.weight"), ("d_w_pos", "gmap_pos_embeddings.0.weight"),
                      ("d_b_pos", "gmap_pos_embeddings.0.bias"), ("dgamma", "gmap_pos_embeddings.1.weight"),
                      ("dbeta", "gmap_pos_embeddings.1.bias")):
        _close(ref[name], Pg[f"{k}.{key}"].grad, name)


@pytest.mark.parametrize("masks", ["none", "visited", "valid", "both"])
def test_sap_restatement_matches_forward_navigation_head(masks):
    g = torch.Generator().manual_seed(7)
    H, B, G = 256, 3, 9
    cfg = po.PlannerConfig(hidden_size=H, num_x_layers=0, graph_sprels=False)
    k = "global_encoder"
    P = {f"{k}.gmap_pos_embeddings.0.weight": _rand(g, H, 7), f"{k}.gmap_pos_embeddings.0.bias": _rand(g, H),
         f"{k}.gmap_pos_embeddings.1.weight": torch.zeros(H, dtype=F64), f"{k}.gmap_pos_embeddings.1.bias": torch.zeros(H, dtype=F64),
         f"{k}.gmap_step_embeddings.weight": torch.zeros(100, H, dtype=F64),
         "global_sap_head.net.0.weight": torch.eye(H, dtype=F64), "global_sap_head.net.0.bias": torch.zeros(H, dtype=F64),
         "global_sap_head.net.2.weight": _rand(g, H, scale=0.3, shift=1.0), "global_sap_head.net.2.bias": _rand(g, H, scale=0.5),
         "global_sap_head.net.4.weight": _rand(g, 1, H, scale=0.1), "global_sap_head.net.4.bias": _rand(g, 1)}
    r = torch.relu(_rand(g, B, G, H))
    r[1, 2] = 0.0                                                       # an all-zero ReLU row
    visited = torch.rand(B, G, generator=g) < 0.3
    valid = torch.rand(B, G, generator=g) < 0.8
    vis_or = visited if masks in ("visited", "both") else torch.zeros_like(visited)
    val_or = valid if masks in ("valid", "both") else torch.ones_like(valid)
    Pg = {n: v.clone().requires_grad_(True) for n, v in P.items()}
    r_ = r.clone().requires_grad_(True)
    txt = torch.zeros(B, 4, H, dtype=F64)
    out = po.forward_navigation(Pg, cfg, txt, torch.ones(B, 4, dtype=torch.bool), torch.zeros(B, G, dtype=torch.long), r_,
                                torch.zeros(B, G, 7, dtype=F64), val_or, vis_or, torch.zeros(B, G, G, dtype=F64))
    lg_or = out["global_logits"]
    dl = _rand(g, B, G)
    lg_or.backward(torch.where(torch.isfinite(lg_or), dl, torch.zeros_like(dl)))
    M = B * G
    vis = visited.reshape(M).to(torch.uint8) if masks in ("visited", "both") else None
    val = valid.reshape(M).to(torch.uint8) if masks in ("valid", "both") else None
    args = (P["global_sap_head.net.2.weight"], P["global_sap_head.net.2.bias"], P["global_sap_head.net.4.weight"].reshape(H),
            P["global_sap_head.net.4.bias"])
    lg, st = rr.sap_fwd(r.reshape(M, H), *args, visited=vis, valid=val)
    _close(lg, lg_or.detach().reshape(M), "logits")
    _close(st[:, 0], r.reshape(M, H).mean(-1), "mean")
    dl_nan = torch.where(rr.sap_masked(M, vis, val), torch.full((M,), float("nan"), dtype=F64), dl.reshape(M))
    ref = rr.sap_bwd(dl_nan, r.reshape(M, H), *args, visited=vis, valid=val)
    _close(ref["dz"], r_.grad.reshape(M, H), "dz")
    for name, key in (("dgamma", "net.2.weight"), ("dbeta", "net.2.bias"), ("dw2", "net.4.weight"), ("db2", "net.4.bias")):
        _close(ref[name].reshape(-1), Pg[f"global_sap_head.{key}"].grad.reshape(-1), name)
    assert bool((ref["dz"][rr.sap_masked(M, vis, val)] == 0).all()) and bool(torch.isfinite(ref["dz"]).all())


@pytest.mark.parametrize("eps", [1e-12, 1e-5])
def test_ln_restatement_matches_layer_norm(eps):
    g = torch.Generator().manual_seed(3)
    H, M = 256, 9
    x = _rand(g, M, H, scale=2.0)
    x[1] += 50.0
    x[4] = 0.0
    w, b = _rand(g, H, shift=1.0), _rand(g, H)
    y, st = rr.ln_fwd(x, w, b, eps)
    _close(y, torch.nn.functional.layer_norm(x, (H,), w, b, eps), "y")
    var, mean = torch.var_mean(x, -1, unbiased=False)
    _close(st[:, 0], mean, "mean")
    _close(st[:, 1], 1 / torch.sqrt(var + eps), "rstd")
    assert torch.equal(y[4], b)
