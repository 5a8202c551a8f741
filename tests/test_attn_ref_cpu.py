"""tests/attn_ref.py restates the attention operator; this file pins its values to the oracle's own attention
(oracle/planner_oracle.py `bert_attention_core`, vilmodel_cmt.py:112-137 / 330-351) in float64, values and autograd gradients, to
1e-12 relative.  The additive mask is formed as the oracle's callers form it: `extend_neg_masks` (+ the sprel bias of
`forward_navigation`, :732-736 / :391-393) for mask_mode 0, -inf on invalid keys as `pano_encoder_layer` fills them for mask_mode 1.
The oracle's core scales by 1/sqrt(64); another alpha goes in through the query (q * alpha * 8), and comes back out of dQ.
Also: etp_attn_family, the host-only query the GPU tests rely on, answers from the dispatch's own predicates (no kernel runs)."""
import ctypes

import pytest
import torch

from etpnav_amd import _lib
from oracle import planner_oracle as po
from tests import attn_ref as ar

F64 = torch.float64
REL = 1e-12


def oracle_attention(c):
    """-> dict like attn_ref's values, from bert_attention_core + autograd"""
    B, nh = c["B"], c["nh"]
    q, k, v = (ar.merge_heads(c[n].to(F64)).reshape(B, -1, nh * 64).requires_grad_(True) for n in ("q", "k", "v"))
    sc = c["alpha"] * 8.0
    km = c["km"] if c["km"] is not None else torch.ones(B, c["Lk"], dtype=torch.bool)
    if c["mask_mode"] == 0:
        add = po.extend_neg_masks(km, F64)
    else:
        add = torch.zeros(B, 1, 1, c["Lk"], dtype=F64).masked_fill(~km[:, None, None, :], float("-inf"))
    w = torch.tensor(c["sp_w"], dtype=F64, requires_grad=True)
    b0 = torch.tensor(c["sp_b"], dtype=F64, requires_grad=True)
    if c["dist"] is not None:
        add = add + (c["dist"].to(F64) * w + b0)[:, None]
    ctx = po.bert_attention_core(q * sc, k, v, add, nh)
    ctx.backward(ar.merge_heads(c["dctx"].to(F64)).reshape(B, -1, nh * 64))
    out = {"ctx": ctx.detach(), "dQ": q.grad, "dK": k.grad, "dV": v.grad}
    out = {n: ar.split_heads(t.reshape(-1, nh * 64), B, nh) for n, t in out.items()}
    if c["dist"] is not None:
        out["d_sp_w"], out["d_sp_b"] = w.grad, b0.grad
    return out


CASES = [(Lq, Lk, B, nh, mm, wd, alpha, spw, sd, rot, nm) for (Lq, Lk, B, nh, mm, wd, alpha, spw, sd, rot, nm)
         in ar.case_grid(ar.SHORT[:12] + [(64, 129), (130, 300)]) if B <= 3]


@pytest.mark.parametrize("bf16", [True, False])
@pytest.mark.parametrize("Lq,Lk,B,nh,mask_mode,with_dist,alpha,sp_w,seed,rot,null_mask", CASES)
def test_attn_ref_equals_the_oracle(Lq, Lk, B, nh, mask_mode, with_dist, alpha, sp_w, seed, rot, null_mask, bf16):
    c = ar.make_case(Lq, Lk, B, min(nh, 4), bf16, mask_mode, with_dist, alpha, sp_w, seed, rot, null_mask)
    val, E = ar.ref_of(c)
    want = oracle_attention(c)
    assert set(val) == set(want) == set(E)
    for n, t in want.items():
        scale = float(t.abs().max())
        if n.startswith("d_sp"):           # sums over B * heads * Lq rows of dS, each of which cancels to zero (d_sp_b is 0 exactly)
            scale = max(scale, float(B * min(nh, 4) * Lq))
        assert float((val[n] - t).abs().max()) <= REL * max(scale, 1e-3), n
        assert bool((E[n] > 0).all()) and E[n].shape == val[n].shape, n


def test_case_grids_cover_what_the_tests_claim():
    """every axis value of the tile edges on both axes; every mask pattern, both mask modes, both alphas, both sp_w, the NULL mask
    pointer and all three batch sizes appear in the short grid; the leading-tile mask appears under mask_mode 1 in the long grid."""
    need = {1, 15, 16, 17, 33, 48, 63, 64, 65, 80, 95, 96, 97, 113, 127, 128}
    assert need <= {s[0] for s in ar.SHORT} and need <= {s[1] for s in ar.SHORT}
    for s in [(1, 128), (128, 1), (80, 80), (36, 36), (16, 80), (97, 64), (64, 97)]:
        assert s in ar.SHORT
    assert {(s[0] + 15) // 16 for s in ar.SHORT} == set(range(1, 9)) == {(s[1] + 15) // 16 for s in ar.SHORT}
    assert ar.LONG == [(16, 512), (512, 512), (130, 300), (64, 129), (129, 64), (300, 70), (257, 255), (1, 640)]
    g = ar.case_grid(ar.SHORT)
    assert {x[4] for x in g} == {0, 1} and {x[6] for x in g} == {0.125, 0.2} and {x[7] for x in g} == {0.3, -1.7}
    assert {(x[2], x[3]) for x in g} == set(ar.BATCHES) and {x[5] for x in g} == {True, False} and {x[10] for x in g} == {True, False}
    kinds_of = lambda x: ar.make_case(x[0], x[1], x[2], 1, True, x[4], False, x[6], x[7], x[8], x[9], x[10])["kinds"] or []
    seen = {0: set(), 1: set()}
    for x in g:
        seen[x[4]] |= set(kinds_of(x))
    assert seen[0] == set(ar.MASKS) and seen[1] == set(ar.MASKS) - {"none"}
    lead1 = [x for x in ar.case_grid(ar.LONG, dist_ok=False) if x[4] == 1 and x[1] > 128 and "lead" in kinds_of(x)]
    assert len(lead1) >= 2, "too few long cases mask the whole leading 128-key tile under mask_mode 1"
    for x in lead1:
        c = ar.make_case(x[0], x[1], x[2], 1, True, 1, False, x[6], x[7], x[8], x[9], False)
        b = c["kinds"].index("lead")
        assert not bool(c["km"][b, :128].any()) and bool(c["km"][b, 128:].all())
    for mm in (0, 1):                      # under mask_mode 1 every row keeps a valid key
        for kind in ar.MASKS:
            for Lk in (1, 2, 16, 17, 128, 300):
                m = ar.key_mask(kind, Lk, mm, 128 if Lk > 128 else 16, torch.Generator().manual_seed(Lk))
                assert mm == 0 or bool(m.any())
                assert kind != "none" or mm == 1 or not bool(m.any())


def _desc(dtype, Lq, Lk, ldq=768, ldc=768, q=4096, dist=0):
    d = _lib.AttnDesc()
    d.dtype, d.B, d.heads, d.Lq, d.Lk, d.ldS = dtype, 2, 12, Lq, Lk, (Lk + 7) // 8 * 8
    d.Q, d.ldq, d.K, d.ldk, d.V, d.ldv = q, ldq, 8192, 768, 16384, 768     # never dereferenced: the query is host-only
    d.ldc = ldc
    if dist:
        d.dist, d.sp_w, d.sp_b = 4096, 4096, 4096
    return d


def test_attn_family_query_follows_the_dispatch_order():
    L = _lib.lib()
    fam = lambda *a, **k: L.etp_attn_family(ctypes.byref(_desc(*a, **k)))
    BF, F32 = _lib.ETP_BF16, _lib.ETP_F32
    assert fam(BF, 80, 80) == 2 and fam(BF, 128, 128, dist=1) == 2
    assert fam(BF, 16, 512) == 3 and fam(BF, 129, 64) == 3
    assert fam(BF, 16, 512, dist=1) == 0                    # the streaming kernels take no distance bias
    assert fam(F32, 64, 64) == 1 and fam(F32, 65, 64) == 0 and fam(F32, 16, 512) == 0
    assert fam(BF, 80, 80, q=4098) == 0 and fam(BF, 80, 80, ldq=772) == 0 and fam(BF, 16, 512, ldc=772) == 0     # alignment
    assert fam(F32, 36, 36, ldq=772) == 1 and fam(F32, 36, 36, ldq=770) == 0
    assert L.etp_attn_family(None) < 0
    with _lib.option("ATTN_ROWS", 0):
        assert fam(BF, 80, 80) == 1 and fam(BF, 16, 512) == 3
        with _lib.option("ATTN_FUSED", 0):
            assert fam(BF, 80, 80) == 0 and fam(BF, 16, 512) == 0 and fam(F32, 36, 36) == 0
    with _lib.option("ATTN_FLASH", 0):
        assert fam(BF, 16, 512) == 0 and fam(BF, 80, 80) == 2
    assert fam(BF, 80, 80) == 2
