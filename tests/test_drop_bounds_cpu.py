"""The comparators of the dropout-site tests can fail, and the right code passes them -- on every case shape of the GPU lists
(tests/drop_ref.py), without a GPU.

Planted mistakes.  For each case the output a kernel WITH the mistake would return is built from the fp64 restatement of the wrong
formula, rounded to the output dtype, and handed to exactly the checks the GPU file runs; they must raise.
  wrong mask (drop_ref.MASK_MISTAKES)   index shifted by one; row and column swapped; the two halves of a pair swapped; the site seed
                                        of another slot; inv_keep missing -- in the forward and in the backward
  wrong placement                       backward without the mask; backward with the mask of another site; sap_tail_bwd with only
                                        one of its two applications (either one); ln_bwd_s masking dx as well as dx_lp, or masking
                                        dy before the parameter sums
A mistake that names the same multiplier for every element of a shape is the right code there and cannot be told from it: row and
column swapped at M = 1 (and in the cast, whose index has no rows).  `planted` asserts that identity, for exactly those, and the
mistake is rejected at every other shape.  Row kernels have no leading dimension and start no run at an odd index (H % 256 == 0,
runs of four): those two mistakes of the issue's list do not exist in them.

GEMM epilogue (drop_ref.GEMM_INSTANCES x GEMM_COMPS): the wrong masks above plus the index with ldc; the mask before the
activation (SAVEGRAD; under MUL_Z and without an activation the mask commutes with the product: asserted equal instead), on the
stored Z, on the residual.  The vector path starts its runs of eight at even indices (N % 8 == 0) and the scalar path asks element
by element: the odd-start mistake does not exist there.  Attention (drop_ref.ATTN_*_G): the wrong masks, the index with ldS, the
odd-start branch replaced by the even one (differs exactly where Lk is odd; an identity, asserted, where Lk is even), the backward
without the mask, with another site's, with a shifted one -- and the one-hot probes' own checks reject a mask with swapped halves.

The right code.  fp32 emulations of the schedules (reduce_ref.emulate_text, emulate_ln_bwd; the cast is one multiply and one
rounding) and, where reduce_ref has no emulation (panorama, SAP tail: row_ref's tolerance classes), the reference rounded to the
output dtype pass every check, the exact read-out included.
"""
import pytest
import torch

from tests import drop_ref as dr
from tests import reduce_ref as rf
from tests import row_ref as rr

F64, F32 = torch.float64, torch.float32
BWD_MASKS = dr.MASK_MISTAKES + ("none", "other_site")


def rejected(fn):
    try:
        fn()
    except AssertionError:
        return True
    return False


def planted(site, M, H, kinds, flat=False):
    """(kind, wrong mask) for every kind whose mask differs from the right one somewhere; the others must be the identities above"""
    right = site.rows(M, H)
    for kind in kinds:
        wrong = site.rows(M, H, kind)
        if torch.equal(wrong, right):
            assert kind == "swap_rc" and (M == 1 or flat), (kind, M, H)
            continue
        yield kind, wrong


def ids(cases):
    return ["-".join(str(v) for v in c) for c in cases]


# ---- text embedding ------------------------------------------------------------------------------------------------------------
TEXT = dr.text_cases()


def check_text_forward(c, y, lp, stats, t):
    dr.zero_set("text y", y, c["m"])
    rf.check_text_fwd("text fwd", c, y, lp, stats)


@pytest.mark.parametrize("i", range(len(TEXT)), ids=ids(TEXT))
def test_text(i):
    dt, H, B, Lt, p, triple = TEXT[i]
    site, t = dr.Site(p, triple), dr.TDT[dt]
    c = dr.text_case(B, Lt, H, site, seed=100 + i)
    M = B * Lt
    ok, why = dr.readable("text y", c["y_plain"], c["by_plain"])
    assert ok, why
    # the right code: the fp32 schedule, then one fp32 multiply
    y32, st32, _ = rf.emulate_text(c, backward=False)
    y = y32 * c["m"]
    check_text_forward(c, y, y.to(t), st32, t)
    d = dr.text_backward(c)
    _, _, got = rf.emulate_text(d)
    rf.check_text_bwd("text bwd", d, got)
    # planted mistakes
    for kind, wrong in planted(site, M, H, dr.MASK_MISTAKES):
        yw = (c["y_plain"] * wrong.to(F64)).float()
        assert rejected(lambda: check_text_forward(c, yw, yw.to(t), st32, t)), f"forward, {kind}"
    for kind, wrong in planted(site, M, H, BWD_MASKS):
        gw = dr.text_got(dr.text_backward(c, wrong))
        assert rejected(lambda: rf.check_text_bwd("text bwd", d, gw)), f"backward, {kind}"
    assert rejected(lambda: rf.same_bits("y_lp", (y32 * c["m"]).to(t), (y32 * site.rows(M, H, "shift")).to(t))), "y_lp"
    if M <= dr.PROBE_ROWS:                                # the one-hot probe: dbeta = dy[row] * m[row]
        for kind, wrong in planted(site, M, H, ("shift", "swap_rc", "swap_halves", "other_slot", "none", "other_site")):
            assert any(rejected(lambda: dr.zero_set("dbeta", c["dy"].reshape(M, H)[r] * wrong[r], c["m"][r])) for r in range(M)), kind


# ---- panorama embedding --------------------------------------------------------------------------------------------------------
PANO = dr.pano_cases()


def check_pano_forward(c, y, stats):
    dr.zero_set("pano y", y, c["m"])
    rr.check_pano_fwd(y, stats, c["y"], c["st"], c["depth"])


@pytest.mark.parametrize("i", range(len(PANO)), ids=ids(PANO))
def test_pano(i):
    dt, H, M, depth, p, triple = PANO[i]
    site = dr.Site(p, triple)
    c = dr.pano_case(M, H, depth, dr.TDT[dt], site, seed=200 + i)
    ok, why = dr.readable("pano y", c["y_plain"], dr.pano_y_bound(c["a"].to(F64), None if c["d"] is None else c["d"].to(F64),
                                                                 c["loc"].to(F64), c["nav"], c["p64"]))
    assert ok, why
    stats = c["st"].float()
    if not depth:
        stats[:, 2:4] = float("nan")
    check_pano_forward(c, (c["y_plain"].float() * c["m"]), stats)                     # the right code: fp32 y, one fp32 multiply
    ref = dr.pano_backward(c)
    da, dd, grads = dr.pano_got(c, ref)
    rr.check_pano_bwd(da, dd, grads, c["init"], ref, depth)
    for kind, wrong in planted(site, M, H, dr.MASK_MISTAKES):
        yw = (c["y_plain"] * wrong.to(F64)).float()
        assert rejected(lambda: check_pano_forward(c, yw, stats)), f"forward, {kind}"
    for kind, wrong in planted(site, M, H, BWD_MASKS):
        daw, ddw, gw = dr.pano_got(c, dr.pano_backward(c, wrong))
        assert rejected(lambda: rr.check_pano_bwd(daw, ddw, gw, c["init"], ref, depth)), f"backward, {kind}"


# ---- SAP tail ------------------------------------------------------------------------------------------------------------------
SAP = dr.sap_cases()


@pytest.mark.parametrize("i", range(len(SAP)), ids=ids(SAP))
def test_sap(i):
    dt, H, M, pattern, p, triple = SAP[i]
    site = dr.Site(p, triple)
    c = dr.sap_case(M, H, pattern, dr.TDT[dt], site, seed=300 + i)
    masked, ones = c["masked"], torch.ones(M, H)
    ref_lg, ref_st = dr.sap_forward(c)
    rr.check_sap_fwd(ref_lg.float(), ref_st.float(), ref_lg, ref_st, masked)             # the right code
    ref = dr.sap_backward(c)
    dz, got = dr.sap_got(c, ref)
    rr.check_sap_bwd(dz, got, c["init"], ref, masked, c["r"])
    for kind, wrong in planted(site, M, H, dr.MASK_MISTAKES):
        lw = dr.sap_forward(c, wrong)[0].float()
        assert rejected(lambda: rr.check_sap_fwd(lw, ref_st.float(), ref_lg, ref_st, masked)), f"forward, {kind}"
    both = [(k, w, w) for k, w in planted(site, M, H, BWD_MASKS)]
    for kind, m_w, m_n in both + [("only dw2 masked", c["m"], ones), ("only dn masked", ones, c["m"])]:
        dzw, gw = dr.sap_got(c, dr.sap_backward(c, m_w, m_n))
        assert rejected(lambda: rr.check_sap_bwd(dzw, gw, c["init"], ref, masked, c["r"])), f"backward, {kind}"
    if M <= dr.PROBE_ROWS:                                # the probes: dw2 = dl * n * m, dbeta = dl * w2 * m of one row
        rows = [r for r in range(M) if not bool(masked[r])]
        assert rows
        for r in rows:
            dr.zero_set("dw2", 1.5 * c["n"][r] * c["m"][r], c["m"][r])
            dr.zero_set("dbeta", 1.5 * c["w2"] * c["m"][r], c["m"][r])
        for kind, wrong in planted(site, M, H, ("shift", "swap_rc", "swap_halves", "other_slot", "none", "other_site")):
            assert any(rejected(lambda: dr.zero_set("dw2", 1.5 * c["n"][r] * wrong[r], c["m"][r])) for r in rows), kind
            assert any(rejected(lambda: dr.zero_set("dbeta", 1.5 * c["w2"] * wrong[r], c["m"][r])) for r in rows), kind


# ---- ln_bwd_s ------------------------------------------------------------------------------------------------------------------
LN = dr.ln_cases()


@pytest.mark.parametrize("i", range(len(LN)), ids=ids(LN))
def test_ln(i):
    dt, H, M, slabs, with_add, p, triple = LN[i]
    site, t = dr.Site(p, triple), dr.TDT[dt]
    c = dr.ln_case(M, H, slabs, site, seed=400 + i)
    add = c["add"] if with_add else None
    blocks = dr.ln_blocks(M, slabs)
    dx, dg, db = rf.emulate_ln_bwd(c, blocks, slabs, add)                                  # the right code: the fp32 schedule
    dr.check_ln("ln", c, dx, (dx * c["m"]).to(t), dg, db, add)
    for kind, wrong in planted(site, M, H, dr.MASK_MISTAKES + ("none", "other_site")):
        assert rejected(lambda: dr.check_ln("ln", c, dx, (dx * wrong).to(t), dg, db, add)), kind
    assert rejected(lambda: dr.check_ln("ln", c, dx * c["m"], (dx * c["m"]).to(t), dg, db, add)), "dx masked as well"
    cm = dict(c, dy=(c["dy"] * c["m"]))
    _, dgm, dbm = rf.emulate_ln_bwd(cm, blocks, slabs, add)
    assert rejected(lambda: dr.check_ln("ln", c, dx, (dx * c["m"]).to(t), dgm, dbm, add)), "dgamma / dbeta from the masked dy"


# ---- cast_drop -----------------------------------------------------------------------------------------------------------------
CAST = dr.cast_cases()


@pytest.mark.parametrize("i", range(len(CAST)), ids=ids(CAST))
def test_cast(i):
    dt, n, p, triple = CAST[i]
    site, t = dr.cast_site(p, triple, n), dr.TDT[dt]
    src = dr.cast_case(n, seed=500 + i)
    assert bool((src != 0).all()) and bool(torch.isfinite(src * float(dr.inv_keep(p))).all())          # the read-out precondition
    m = site.flat(n)
    dr.check_cast("cast", (src * m).to(t), src, m)
    kinds = [k for k, _ in planted(site, 1, n, dr.MASK_MISTAKES, flat=True)]
    assert kinds == ["shift", "swap_halves", "other_slot", "no_inv_keep"]
    for kind in kinds:
        assert rejected(lambda: dr.check_cast("cast", (src * site.flat(n, kind)).to(t), src, m)), kind


# ---- GEMM epilogue -------------------------------------------------------------------------------------------------------------
from tests import gemm_ref as gr  # noqa: E402

GEMM = sorted({(M, N, K, bf16, comp, layout) for (_, _, _, _, _, _, _, bf16, shapes, Ks, layout) in dr.GEMM_INSTANCES
               for (M, N) in shapes for K in Ks for comp in dr.GEMM_COMPS})
GEMM_MASKS = ("ld",) + dr.MASK_MISTAKES + ("none", "other_site")


def gemm_emulate(c, m):
    """the epilogue's order in fp32 on an fp32 product (torch's own summation order), stored in the output dtypes"""
    f = torch.float32
    v = (c["A"] @ c["B"].t()) * torch.tensor(c["alpha"], dtype=f) + c["bias"]
    got = {}
    if c["act"] == gr.ACT_GELU_SAVEGRAD:
        got["Z"] = gr.gelu_grad(v.double()).float().to(torch.float16 if c["bf16"] else f)
        v = gr.gelu(v.double()).float()
    elif c["act"] == gr.ACT_MUL_Z:
        v = v * c["Z"]
    v = v * m
    if c["R"] is not None:
        v = v + c["R"]
    if c["out_mode"] == 1:
        v = v + c["C0"]
    got["C"] = v.to(torch.bfloat16 if c["c_bf16"] else f)
    return got


def gemm_wrong(c, val):
    """what a kernel that computes exactly `val` stores"""
    out = {"C": val["C"].to(torch.bfloat16 if c["c_bf16"] else torch.float32)}
    if "Z" in val:
        out["Z"] = val["Z"].to(torch.float16 if c["bf16"] else torch.float32)
    return out


@pytest.mark.parametrize("case", GEMM, ids=ids(GEMM))
def test_gemm(case):
    M, N, K, bf16, comp, layout = case
    site = dr.Site(dr.RATES[(M + K) // 64 % 2], dr.SITES[N % 2])
    ldc = N + 8 if layout == "pad" and N % 8 == 0 else ((N + 7) // 8 * 8 + (8 if layout == "pad" else 61))
    for out_mode in (0, 1) if (comp == "bias_res" and (M, N) == (65, 72) and K >= 160) else (0,):
        c = dr.gemm_case(M, N, K, bf16, comp, seed=1, out_mode=out_mode)
        ok, why = dr.gemm_readable(c)
        assert ok, why
        m = site.rows(M, N)
        dr.check_gemm("gemm", "cpu", c, gemm_emulate(c, m), m)                           # the right code
        for kind in GEMM_MASKS:
            wrong = site.rows(M, N, kind, ld=ldc)
            assert not torch.equal(wrong, m), kind
            assert rejected(lambda: dr.check_gemm("gemm", "cpu", c, gemm_wrong(c, dr.gemm_ref(c, wrong)[0]), m)), kind
        places = {"bias_res": ("on_r",), "savegrad": ("before_act", "on_z"), "mul_z": ()}[comp]
        for place in places:
            assert rejected(lambda: dr.check_gemm("gemm", "cpu", c, gemm_wrong(c, dr.gemm_ref(c, m, place)[0]), m)), place
        if comp == "mul_z":                              # the mask commutes with the product by Z: "before the activation" is the same value
            a, b = dr.gemm_ref(c, m, "before_act")[0]["C"], dr.gemm_ref(c, m)[0]["C"]
            assert float((a - b).abs().max()) <= 1e-12 * float(b.abs().max())


# ---- attention -----------------------------------------------------------------------------------------------------------------
from tests import attn_ref as ar  # noqa: E402

#        (grid, bf16, batched-GEMM bounds?, LDS-tile bounds?)
ATTN = [(x, True, False, False) for x in dr.ATTN_SHORT_G] + [(x, True, False, True) for x in dr.ATTN_SHORT_G] + \
       [(x, False, False, True) for x in dr.ATTN_F32_G] + [(x, True, False, False) for x in dr.ATTN_LONG_G] + \
       [(x, x[0] == 130, True, False) for x in dr.ATTN_GEMM_G]


def attn_emulate(c, m):
    """fp32 arithmetic in the operator's order with the bf16 roundings of the fused kernels (bf16 mode): the dropped probabilities
    before P.V and P^T.dO, dS before its two products, every output at its store"""
    f = torch.float32
    rb = (lambda x: x.bfloat16().float()) if c["bf16"] else (lambda x: x)
    q, k, v, do = (c[n].to(f) for n in ("q", "k", "v", "dctx"))
    add = torch.where(c["km"], 0.0, float("-inf") if c["mask_mode"] else -10000.0).to(f)[:, None, None, :]
    if c["dist"] is not None:
        add = add + (c["dist"] * c["sp_w"] + c["sp_b"])[:, None]
    P = torch.softmax(c["alpha"] * (q @ k.transpose(-1, -2)) + add, -1)
    Pd = rb(P * m)
    dP = (do @ v.transpose(-1, -2)) * m
    dS = rb(P * (dP - (P * dP).sum(-1, keepdim=True)))
    out = {"ctx": rb(Pd @ v), "dQ": rb(c["alpha"] * (dS @ k)), "dK": rb(c["alpha"] * (dS.transpose(-1, -2) @ q)), "dV": rb(Pd.transpose(-1, -2) @ do)}
    if c["dist"] is not None:
        out["d_sp_w"], out["d_sp_b"] = (dS.sum(1) * c["dist"]).sum(), dS.sum()
    return out


def attn_wrong(c, val):
    t = torch.bfloat16 if c["bf16"] else torch.float32
    return {n: (v.to(t) if n in ("ctx", "dQ", "dK", "dV") else v.float()) for n, v in val.items() if n != "P"}


@pytest.mark.parametrize("i", range(len(ATTN)), ids=[f"{j}-{'bf16' if a[1] else 'fp32'}-{a[0][0]}x{a[0][1]}-m{a[0][4]}" for j, a in enumerate(ATTN)])
def test_attention(i):
    (Lq, Lk, B, nh, mask_mode, with_dist, p, triple, seed), bf16, gemm, tile = ATTN[i]
    site = dr.Site(p, triple)
    c = dr.attn_case(Lq, Lk, B, nh, bf16, mask_mode, with_dist, seed)
    ldS = (Lk + 7) // 8 * 8 + 8
    m = dr.attn_index_mask(site, B, nh, Lq, Lk)
    val, E = dr.attn_ref(c, m, gemm=gemm, tile=tile)
    ar.check_all(attn_emulate(c, m), val, E, "attention", "cpu-drop")                   # the right code
    for kind in dr.ATTN_MASKS + ("none", "other_site"):
        wrong = dr.attn_index_mask(site, B, nh, Lq, Lk, kind, ldS=ldS)
        if torch.equal(wrong, m):
            assert kind == "even_branch" and Lk % 2 == 0, kind           # no run starts at an odd index when Lk is even
            continue
        got = attn_wrong(c, dr.attn_ref(c, wrong)[0])
        assert rejected(lambda: ar.check_all(got, val, E, "attention", "cpu-drop-wrong")), f"forward and backward, {kind}"
        if kind in ("none", "other_site", "shift"):                   # the backward alone regenerates another mask
            got = attn_wrong(c, dr.attn_ref(c, m, m_b=wrong)[0])
            assert torch.equal(got["ctx"], attn_wrong(c, val)["ctx"])
            assert rejected(lambda: ar.check_all(got, val, E, "attention", "cpu-drop-wrong")), f"backward only, {kind}"
    # the probes read what they claim: block 0 of the keys and of the queries
    pv, pdo = dr.probe_v(c, 0), dr.probe_do(c, 0)
    vj, Ej = dr.attn_ref(c, m, gemm=gemm, tile=tile, v=pv)
    dr.probe_ctx_check("ctx probe", c, 0, attn_wrong(c, vj)["ctx"], m, vj, Ej)
    vi, Ei = dr.attn_ref(c, m, gemm=gemm, tile=tile, dctx=pdo)
    dr.probe_dv_check("dV probe", c, 0, attn_wrong(c, vi)["dV"], m, vi, Ei)
    wrong = dr.attn_index_mask(site, B, nh, Lq, Lk, "swap_halves")
    assert rejected(lambda: dr.probe_ctx_check("ctx probe", c, 0, attn_wrong(c, dr.attn_ref(c, wrong, v=pv)[0])["ctx"], m, vj, Ej))
    assert rejected(lambda: dr.probe_dv_check("dV probe", c, 0, attn_wrong(c, dr.attn_ref(c, m, m_b=wrong, dctx=pdo)[0])["dV"], m, vi, Ei))
