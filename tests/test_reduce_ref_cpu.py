"""Pins the fp64 restatements of tests/reduce_ref.py to the code they restate, in float64 at 1e-12:

  ln_bwd / ln_terms   autograd of oracle/planner_oracle.layer_norm and of torch.nn.functional.layer_norm; the closed form
                      rstd * (gy - mean(gy) - xhat * mean(gy * xhat)) the bounds and the emulation are written in
  text_fwd / _bwd     the oracle's text-embedding path (planner_oracle.forward_txt with no encoder layers) and its autograd; the padding
                      row of the word table gets no gradient
  ce                  torch.nn.functional.cross_entropy(reduction="sum", ignore_index=...) * scale and its autograd
  adamw               oracle/optim_oracle.adamw_step, both styles, with and without bias correction, clipping and skip
  gather_sum, colsum  plain loops
  bf16_rne(_bits)     torch's own fp32 -> bf16 conversion, bit for bit, over the special values and 2^20 random bit patterns
  launch geometry     ln_stage_blocks / ln_depth at the figures the kernel comments state
"""
import math

import pytest
import torch
import torch.nn.functional as F

from oracle import optim_oracle as oo
from oracle import planner_oracle as po
from tests import reduce_ref as rf

F64 = torch.float64


def rel(a, b):
    return float((a - b).abs().max()) / max(1e-300, float(b.abs().max()))


@pytest.mark.parametrize("M,H,eps", [(5, 256, 1e-12), (77, 768, 1e-5), (33, 1024, 1e-12)])
def test_ln_bwd_restatement(M, H, eps):
    torch.manual_seed(M)
    x, dy = torch.randn(M, H, dtype=F64) * 2 + 0.5, torch.randn(M, H, dtype=F64)
    gamma, beta, add = 1 + 0.3 * torch.randn(H, dtype=F64), torch.randn(H, dtype=F64), torch.randn(M, H, dtype=F64)
    dx, dg, db = rf.ln_bwd(dy, x, gamma, eps, add)
    # the oracle's layer_norm and torch's, through autograd
    for fn in (lambda a, g, b: po.layer_norm(a, g, b, eps), lambda a, g, b: F.layer_norm(a, (H,), g, b, eps)):
        x_, g_, b_ = x.clone().requires_grad_(True), gamma.clone().requires_grad_(True), beta.clone().requires_grad_(True)
        fn(x_, g_, b_).backward(dy)
        assert rel(dx, x_.grad + add) < 1e-12 and rel(dg, g_.grad) < 1e-12 and rel(db, b_.grad) < 1e-12
    # the closed form of the bounds / emulation
    t = rf.ln_terms(dy, x, gamma, eps)
    s1, s2 = t["gy"].mean(-1, keepdim=True), (t["gy"] * t["xh"]).mean(-1, keepdim=True)
    assert rel(t["rstd"] * (t["gy"] - s1 - t["xh"] * s2) + add, dx) < 1e-12
    assert rel((t["dy"] * t["xh"]).sum(0), dg) < 1e-12 and rel(t["dy"].sum(0), db) < 1e-12
    y, st = rf.ln_fwd(x, gamma, beta, eps)
    assert rel(y, F.layer_norm(x, (H,), gamma, beta, eps)) < 1e-12
    assert rel(st[:, 0], x.mean(-1)) < 1e-12 and rel(st[:, 1], 1 / torch.sqrt(x.var(-1, unbiased=False) + eps)) < 1e-12


def test_ln_geometry():
    assert rf.ln_stage_blocks(2560) == 640 and rf.ln_stage_blocks(4096) == 1024 and rf.ln_stage_blocks(4097) == 513
    assert rf.ln_stage_blocks(8192) == 1024 and rf.ln_stage_blocks(8192, 2048) == 1024 and rf.ln_stage_blocks(8192, 1) == 1
    assert rf.ln_stage_blocks(8192, 3) == 3 and rf.ln_stage_blocks(5, 3) == 2 and rf.ln_stage_blocks(1) == 1
    assert rf.ln_depth(8192, 1024, True) == 47                       # 2 + 3 + 8 + 2 + 32
    assert rf.ln_depth(124, 31, True) == 1 + 3 + 10 + 2 + 1          # 31 slabs: seven groups of four and three single adds
    assert rf.ln_depth(132, 33, True) == 1 + 3 + 8 + 2 + 2
    assert rf.ln_depth(2053, 128, False) == 5 + 3 + 128
    assert rf.ln_part_bytes(8192, 768) == 2 * 768 * 4 * 1024
    # every wave the same number of rows: blocks * rounds covers the row groups, and no block is empty
    for M in rf.LN_STAGE_M:
        for cap in rf.LN_GRIDS:
            b = rf.ln_stage_blocks(M, cap)
            assert 1 <= b <= 1024 and 4 * (b - 1) < M


@pytest.mark.parametrize("ignore_index", [-100, -1])
@pytest.mark.parametrize("B,G", [(7, 11), (17, 65), (1, 1)])
def test_ce_restatement(B, G, ignore_index):
    torch.manual_seed(B * G)
    logits = torch.randn(B, G, dtype=F64) * 3
    if G > 2:
        logits[:, 1] = float("-inf")
    labels = torch.randint(0, G, (B,))
    labels[labels == 1] = 0
    if B > 2:
        labels[1] = ignore_index
    l_ = logits.clone().requires_grad_(True)
    loss = F.cross_entropy(l_, labels, reduction="sum", ignore_index=ignore_index) * 0.37
    loss.backward()
    rl, rd, _ = rf.ce(logits, labels, 0.37, ignore_index)
    assert abs(float(rl) - float(loss)) <= 1e-12 * max(1.0, abs(float(loss)))
    assert float((rd - l_.grad).abs().max()) <= 1e-12
    labels[:] = ignore_index
    rl, rd, _ = rf.ce(logits, labels, 0.37, ignore_index)
    assert float(rl) == 0.0 and not bool((rd != 0).any())


@pytest.mark.parametrize("hf_style", [0, 1])
@pytest.mark.parametrize("correct_bias", [0, 1])
@pytest.mark.parametrize("max_norm", [0.0, 1.0])
def test_adamw_restatement(hf_style, correct_bias, max_norm):
    torch.manual_seed(5)
    n = 256
    cfg = rf.cfg_f32(lr=3e-3, beta1=0.9, beta2=0.999, eps=1e-8, weight_decay=0.01, step=1, hf_style=hf_style, correct_bias=correct_bias,
                     grad_scale=0.5, max_norm=max_norm)
    mask = torch.tensor([0, 1, 255, 1], dtype=torch.uint8)
    wd = cfg["weight_decay"] * torch.tensor([0.0, 1.0, 1.0, 1.0], dtype=F64).repeat_interleave(64)
    p = (torch.randn(n) * 0.3).to(F64)
    m, v = torch.zeros(n, dtype=F64), torch.zeros(n, dtype=F64)
    for step in (1, 2, 3):
        cfg["step"] = step
        g = (torch.randn(n) * (4.0 if step == 2 else 0.05)).to(F64)
        ss = float((g * g).sum())
        r = rf.adamw(p, g, m, v, cfg, ss, mask)
        oo.adamw_step(p, g, m, v, step, cfg["lr"], cfg["beta1"], cfg["beta2"], cfg["eps"], wd, bool(hf_style), bool(correct_bias),
                      cfg["grad_scale"], max_norm)
        assert rel(r["p"], p) < 1e-12 and rel(r["m"], m) < 1e-12 and rel(r["v"], v) < 1e-12, step
    before = (p.clone(), m.clone(), v.clone())
    r = rf.adamw(p, g, m, v, cfg, ss, mask, skip=True, steps_applied=3)
    oo.adamw_step(p, g, m, v, 4, cfg["lr"], cfg["beta1"], cfg["beta2"], cfg["eps"], wd, bool(hf_style), bool(correct_bias), 0.5, max_norm,
                  skip=True)
    assert all(torch.equal(a, b) for a, b in zip((r["p"], r["m"], r["v"]), before)) and torch.equal(p, before[0]) and r["counter"] == 3
    # the counted formulation uses counter + 1 and advances it
    r = rf.adamw(p, g, m, v, cfg, ss, mask, steps_applied=3)
    cfg["step"] = 4
    r4 = rf.adamw(p, g, m, v, cfg, ss, mask)
    assert r["counter"] == 4 and torch.equal(r["p"], r4["p"])
    # frozen bytes: state kept
    r = rf.adamw(p, g, m, v, cfg, ss, torch.tensor([2, 3, 0, 1], dtype=torch.uint8))
    assert torch.equal(r["p"][:128], p[:128]) and not torch.equal(r["p"][128:], p[128:])


def test_sums_restatements():
    torch.manual_seed(1)
    src, ptr, idx, w, init = rf.gather_case(5, 256, torch.float32, 3)
    out, mag, lens = rf.gather_sum(src, ptr, idx, w, init)
    want = init.to(F64).clone()
    for n in range(5):
        for j in range(int(ptr[n]), int(ptr[n + 1])):
            want[n] += float(w[j]) * src[int(idx[j])].to(F64)
    assert rel(out, want) < 1e-12 and int(lens[0]) == 0 and int(lens[-1]) == 0 and int(lens[1]) == 40
    assert bool((mag >= out.abs() - 1e-12).all())
    dy = torch.randn(65, 8)
    assert rel(rf.colsum(dy), sum(dy[r].to(F64) for r in range(65))) < 1e-12
    g = torch.randn(256)
    g[70] = float("nan")
    s, bad = rf.sumsq(g, torch.tensor([1, 2, 0, 255], dtype=torch.uint8))
    keep = torch.cat([g[:64], g[128:]]).to(F64)
    assert bad == 0 and abs(float(s) - float((keep * keep).sum())) < 1e-12
    assert rf.sumsq(g)[1] == 1


def test_bf16_rne_is_torchs_conversion():
    x = torch.cat([rf.cast_specials(), torch.randint(-2 ** 31, 2 ** 31 - 1, (1 << 20,), dtype=torch.int64).to(torch.int32).view(torch.float32)])
    mine, theirs = rf.bf16_rne_bits(x), x.to(torch.bfloat16).view(torch.int16)
    nan = torch.isnan(x)
    assert torch.equal(mine[~nan], theirs[~nan])
    assert bool(torch.isnan(rf.bf16_rne(x)[nan].float()).all())
    sp = rf.bf16_rne(rf.cast_specials()).float()
    assert math.isinf(float(sp[18])) and math.isinf(float(sp[19])) and float(sp[12]) == 1.0 and float(sp[13]) == 1.015625
    rf.check_cast("self", x.to(torch.bfloat16), x)


def test_text_embedding_restatement():
    cfg = po.PlannerConfig.r2r(vocab_size=rf.TEXT_VOCAB, num_l_layers=0, num_pano_layers=1, num_x_layers=1)
    P = {k: v.to(F64) for k, v in po.init_params(cfg, seed=4).items()}
    B, Lt, H = 3, 9, P["embeddings.LayerNorm.weight"].numel()
    g = torch.Generator().manual_seed(0)
    ids = rf.text_ids("edges", B, Lt, g)
    names = ("embeddings.word_embeddings.weight", "embeddings.position_embeddings.weight", "embeddings.token_type_embeddings.weight",
             "embeddings.LayerNorm.weight", "embeddings.LayerNorm.bias")
    P["embeddings.LayerNorm.weight"] = P["embeddings.LayerNorm.weight"] + 0.3 * torch.randn(H, generator=g, dtype=F64)
    P["embeddings.LayerNorm.bias"] = torch.randn(H, generator=g, dtype=F64)
    for k in names:
        P[k] = P[k].clone().requires_grad_(True)
    want = po.forward_txt(P, cfg, ids, torch.ones(B, Lt, dtype=torch.bool))
    dy = torch.randn(B, Lt, H, generator=g, dtype=F64)
    want.backward(dy)
    word, pos, typ, gamma, beta = (P[k].detach() for k in names)
    y, st, e = rf.text_fwd(ids, word, pos, typ[0], gamma, beta, cfg.layer_norm_eps)
    assert rel(y, want.detach()) < 1e-12
    r = rf.text_bwd(dy, ids, word, pos, typ[0], gamma, beta, cfg.layer_norm_eps)
    gw = P[names[0]].grad.clone()
    assert float(r["dword"][0].abs().max()) == 0.0 and float(gw[0].abs().max()) > 0      # padding_idx 0: the oracle's plain gather has no such row
    gw[0] = 0
    assert rel(r["dword"], gw) < 1e-12 and rel(r["dpos"], P[names[1]].grad) < 1e-12 and rel(r["dtype0"], P[names[2]].grad[0]) < 1e-12
    assert rel(r["dgamma"], P[names[3]].grad) < 1e-12 and rel(r["dbeta"], P[names[4]].grad) < 1e-12
