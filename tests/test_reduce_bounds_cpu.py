"""The bounds of tests/reduce_ref.py can pass and can fail, without a GPU.

PASS: fp32 emulations of each kernel's schedule (the per-wave row sweeps, the 4-wave combine, slab chunks of 32 with four
accumulators, an atomic chain, AdamW's exact operation order, the fp32 powf of the counted entry point) stay inside the bound on every
element of every shape the GPU files run (they build their cases from the same lists of reduce_ref.py): the typed LayerNorm forward and
backward, both stream backward modes, the text embedding, the cross-entropy, colsum, gather_sum (N = 16389 included), sumsq and AdamW
(n = 4 194 304 + 1028 included; there the hyper-parameter pair and the counted flag alternate over the four formulation x bias-correction
combinations instead of being crossed with them).  The casts and scale_f32 are bit-exact comparisons and need no emulation.

FAIL: each mutation of the REFERENCE output listed below is rejected by the comparator the GPU files call.
"""
import pytest
import torch

from tests import reduce_ref as rf

F64 = torch.float64
TDT = {"fp32": torch.float32, "bf16": torch.bfloat16}


def rejected(fn):
    with pytest.raises(AssertionError):
        fn()


# ---- LayerNorm backward: every case of the GPU matrix --------------------------------------------------------------------------
def _ln_run(c, blocks, slabs, add, out_dtype):
    dx, dg, db = rf.emulate_ln_bwd(c, blocks, slabs, add, out_dtype)
    rf.check_ln_bwd("emulated ln_bwd", c, dx, None, dg, db, add)


def test_ln_typed_emulation_inside_bounds():
    for dt, H, M, eps, with_add, _ in rf.ln_typed_cases():
        blocks = rf.ln_typed_blocks(M)
        c = rf.ln_case(M, H, eps, blocks, False, seed=M + H, dtype=TDT[dt])
        _ln_run(c, blocks, False, c["add"] if with_add else None, TDT[dt])


def test_ln_fwd_emulation_inside_bounds():
    """the typed forward at every (dtype, H, M, eps) the GPU file runs, the forward-only M = 16389 included"""
    fwd_only = [(dt, H, M, rf.LN_EPS[i % 2]) for i, (dt, H) in enumerate((d, h) for d in ("fp32", "bf16") for h in rf.LN_H)
                for M in rf.LN_FWD_ONLY_M]
    for dt, H, M, eps in [c[:4] for c in rf.ln_typed_cases()] + fwd_only:
        g = torch.Generator().manual_seed(M + H)
        x = ((torch.randn(M, H, generator=g) * 1.5 + torch.randn(M, 1, generator=g)) * 2.0 ** torch.randint(-10, 4, (M, 1), generator=g).float())
        if M >= 3:
            x[M // 2] = 0.0
            x[M // 3] = 1000.0 + torch.randn(H, generator=g)
        x = x.to(TDT[dt])
        gamma, beta = 1.0 + 0.3 * torch.randn(H, generator=g), 0.5 * torch.randn(H, generator=g)
        y, st = rf.emulate_ln_fwd(x, gamma, beta, eps, TDT[dt])
        ref_y, ref_st = rf.ln_fwd(x, gamma, beta, eps)
        by, bst = rf.ln_fwd_bounds(x, gamma, beta, eps, ref_y, ref_st, dt == "bf16")
        rf.within(("emulated ln_fwd " + dt, "y"), y, ref_y, by)
        rf.within(("emulated ln_fwd " + dt, "stats"), st, ref_st, bst)
    # a variance divided by H - 1 and a forgotten beta are rejected (a bf16 y that truncates is NOT: the bound of a bf16 store is one ulp)
    rejected(lambda: rf.within(("mut", "y"), ref_y - beta.to(F64), ref_y, by))
    wrong = ref_st.clone(); wrong[:, 1] = 1.0 / torch.sqrt(x.to(F64).var(-1, unbiased=True) + eps)
    rejected(lambda: rf.within(("mut", "stats"), wrong, ref_st, bst))


def test_ln_atomic_emulation_inside_bounds():
    for dt, H, M, eps, outs, with_add, _ in rf.ln_atomic_cases():
        blocks = rf.ln_atomic_blocks(M)
        c = rf.ln_case(M, H, eps, blocks, False, seed=M + H + 1)
        _ln_run(c, blocks, False, c["add"] if with_add else None, TDT[dt] if outs == "lp" else torch.float32)


@pytest.mark.parametrize("M", rf.LN_STAGE_M)
def test_ln_stage_emulation_inside_bounds(M):
    for dt, H, M_, eps, grid, outs, with_add in rf.ln_stage_cases():
        if M_ != M:
            continue
        blocks = rf.ln_stage_blocks(M, grid)
        c = rf.ln_case(M, H, eps, blocks, True, seed=M + H + 2)
        assert c["depth"] == rf.ln_depth(M, blocks, True)
        _ln_run(c, blocks, True, c["add"] if with_add else None, TDT[dt] if outs == "lp" else torch.float32)


def test_ln_bound_is_tighter_than_one_row_at_8192():
    """the reason for a depth bound: at M = 8192 the bound of EVERY column is below an eighth of a sentinel row's term, while an
    order-free (M - 1) u bound would be larger than a typical row's share"""
    blocks = rf.ln_stage_blocks(8192)
    c = rf.ln_case(8192, 768, 1e-12, blocks, True, seed=3, with_add=False)
    assert c["depth"] == 47 and c["sent"] == [4092, 4096, 8191]
    t = (c["t"]["dy"] * c["t"]["xh"]).abs()
    assert bool((8 * c["bg"] < t[c["sent"]].min(0).values).all())
    assert float((rf.gam(8191) * t.sum(0)).median()) > float(t.median())


def test_ln_mutations_are_rejected():
    M, H = 4097, 768                                   # 513 blocks (17 chunks), two sweeps: rows 2052.. are the second
    blocks = rf.ln_stage_blocks(M)
    c = rf.ln_case(M, H, 1e-12, blocks, True, seed=9)
    add = c["add"]
    t = c["t"]["dy"] * c["t"]["xh"]
    ref_dx = c["dx0"] + add.to(F64)
    g0, b0 = c["init_g"].to(F64) + c["dgamma"], c["init_b"].to(F64) + c["dbeta"]
    rf.check_ln_bwd("reference", c, ref_dx, None, g0, b0, add)                                # the reference itself passes
    rejected(lambda: rf.check_ln_bwd("mut", c, None, None, g0 - t[M - 1], b0, add))          # dgamma missing the last row
    assert 4 * blocks in c["sent"]
    rejected(lambda: rf.check_ln_bwd("mut", c, None, None, g0 - t[4 * blocks], b0, add))     # ... the second sweep's first row
    rows = torch.arange(M)
    slab33 = ((rows // 4) % blocks) == 32
    rejected(lambda: rf.check_ln_bwd("mut", c, None, None, g0 - t[slab33].sum(0), b0 - c["t"]["dy"][slab33].sum(0), add))  # slab 33 dropped
    rejected(lambda: rf.check_ln_bwd("mut", c, None, None, g0 - t[slab33].sum(0), b0, add))
    rejected(lambda: rf.check_ln_bwd("mut", c, None, None, g0, b0 - c["t"]["dy"][slab33].sum(0), add))
    q = c["t"]
    s1, s2 = q["gy"].mean(-1, keepdim=True), (q["gy"] * q["xh"]).mean(-1, keepdim=True)
    wrong = q["rstd"] * (q["gy"] - s1 * H / (H - 1) - q["xh"] * s2) + add.to(F64)              # mean(g) divided by H - 1
    rejected(lambda: rf.check_ln_bwd("mut", c, wrong, None, None, None, add))
    rejected(lambda: rf.check_ln_bwd("mut", c, ref_dx + add.to(F64), None, None, None, add))  # add applied twice
    rejected(lambda: rf.check_ln_bwd("mut", c, None, None, c["init_g"].to(F64) + c["dbeta"], b0, add))   # dbeta where dgamma belongs
    # a bf16 copy that truncates instead of rounding to nearest even
    dx32 = ref_dx.float()
    trunc = (dx32.view(torch.int32) & -65536).view(torch.float32).to(torch.bfloat16)
    rejected(lambda: rf.check_ln_bwd("mut", c, dx32, trunc, None, None, add))


# ---- text embedding ------------------------------------------------------------------------------------------------------------
def test_text_emulation_inside_bounds():
    for i, (dt, H, B, L, kind, eps, bwd) in enumerate(rf.text_cases()):
        c = rf.text_reference(rf.text_case(B, L, H, kind, eps, seed=i), bwd)
        y, stats, got = rf.emulate_text(c, bwd)
        rf.check_text_fwd("emulated text_embed", c, y, y.to(TDT[dt]), stats)
        if bwd:
            rf.check_text_bwd("emulated text_embed", c, got)
    assert {k for _, _, B, L, k, _, _ in rf.text_cases() if (B, L) == (32, 80)} == set(rf.TEXT_IDS)


def test_text_mutations_are_rejected():
    B, L, H = 5, 24, 256
    c = rf.text_reference(rf.text_case(B, L, H, "edges", 1e-12, seed=3))
    ref = {k: c["init_" + k] .to(F64) + c["ref"][k] for k in ("dword", "dpos", "dtype0", "dgamma", "dbeta")}
    good = {k: v.float() for k, v in ref.items()}
    for k in ("dword", "dpos"):                          # rows the kernel must not touch hold their initial bits in a correct result
        good[k] = torch.where(c["ref"][k] == 0, c["init_" + k], good[k])
    rf.check_text_bwd("reference", c, good)
    dx = c["ref"]["dx"]

    def mut(**kw):
        return dict(good, **kw)

    pad = good["dword"].clone(); pad[0] += dx[:, 0].sum(0).float()
    rejected(lambda: rf.check_text_bwd("mut", c, mut(dword=pad)))                            # the padding word row receiving gradient
    wrong = c["init_dpos"].to(F64).clone()
    rows = torch.arange(B * L)
    wrong.index_add_(0, rows // L, dx.reshape(B * L, H))                                      # position taken as row // L
    rejected(lambda: rf.check_text_bwd("mut", c, mut(dpos=wrong.float())))
    rejected(lambda: rf.check_text_bwd("mut", c, mut(dtype0=(ref["dtype0"] - dx[:, L - 1].sum(0)).float())))   # dtype0 missing one position
    bit = good["dword"].clone()
    row = int((~c["named"]).nonzero()[-1])
    bit[row, 7] = torch.nextafter(bit[row, 7], torch.tensor(float("inf")))
    rejected(lambda: rf.check_text_bwd("mut", c, mut(dword=bit)))                            # an untouched word row changed in one bit
    past = good["dpos"].clone(); past[L, 0] = torch.nextafter(past[L, 0], torch.tensor(0.0))
    rejected(lambda: rf.check_text_bwd("mut", c, mut(dpos=past)))
    y32 = c["y"].float()
    trunc = (y32.view(torch.int32) & -65536).view(torch.float32).to(torch.bfloat16)
    rejected(lambda: rf.check_text_fwd("mut", c, y32, trunc, c["st"].float()))
    # the longest chains of the matrix, (B, L) = (2, 1030): dtype0 missing one position -- an ordinary one, a sentinel one, the last
    B, L = 2, 1030
    c = rf.text_reference(rf.text_case(B, L, H, "random", 1e-12, seed=4))
    assert c["sent"] == [1023, 1024, L + L - 1]
    ref0 = c["init_dtype0"].to(F64) + c["ref"]["dtype0"]
    dx = c["ref"]["dx"]
    for l in (517, 1023, 1024, L - 1):
        rejected(lambda: rf.within(("mut", "dtype0"), (ref0 - dx[:, l].sum(0)).float(), ref0, c["bounds"]["dtype0"]))
    t = c["t"]
    for row in c["sent"]:                                # ... and dgamma / dbeta missing a sentinel row
        rejected(lambda: rf.within(("mut", "dgamma"), c["init_dgamma"].to(F64) + c["ref"]["dgamma"] - (t["dy"] * t["xh"])[row],
                                   c["init_dgamma"].to(F64) + c["ref"]["dgamma"], c["bounds"]["dgamma"]))
        rejected(lambda: rf.within(("mut", "dbeta"), c["init_dbeta"].to(F64) + c["ref"]["dbeta"] - t["dy"][row],
                                   c["init_dbeta"].to(F64) + c["ref"]["dbeta"], c["bounds"]["dbeta"]))


# ---- cross-entropy -------------------------------------------------------------------------------------------------------------
def test_ce_emulation_inside_bounds():
    for i, (B, G, pat) in enumerate(rf.ce_cases()):
        logits, labels, scale, ii = rf.ce_case(B, G, pat, seed=i)
        loss, dl = rf.emulate_ce(logits, labels, scale, ii)
        rf.check_ce("emulated sap_ce", loss, dl, logits, labels, scale, ii)
    pats = {p[:2] for _, _, p in rf.ce_cases()}
    assert {(s, g) for s in (0.0, 80.0, -80.0) for g in ("none", "some", "all")} <= pats


def test_ce_mutations_are_rejected():
    B, G = 33, 130
    logits, labels, scale, ii = rf.ce_case(B, G, (80.0, "some", -1, "fixed"), seed=4)
    loss, dl, q = rf.ce(logits, labels, scale, ii)
    rf.check_ce("reference", loss, dl, logits, labels, scale, ii)
    ign = int((~q["keep"]).nonzero()[0])
    full = rf.ce(logits, torch.where(q["keep"], labels, torch.zeros_like(labels)), scale, ii)
    rejected(lambda: rf.check_ce("mut", full[0], dl, logits, labels, scale, ii))               # an ignored row contributing (loss)
    d2 = dl.clone(); d2[ign] = full[1][ign]
    rejected(lambda: rf.check_ce("mut", loss, d2, logits, labels, scale, ii))                  # ... (gradient)
    shifted = scale * (q["p"] - torch.roll(q["onehot"], 1, 1)) * q["keep"][:, None]
    rejected(lambda: rf.check_ce("mut", loss, shifted, logits, labels, scale, ii))             # the one-hot at y + 1
    rejected(lambda: rf.check_ce("mut", loss * scale, dl, logits, labels, scale, ii))          # scale applied twice
    rejected(lambda: rf.check_ce("mut", loss, dl * scale, logits, labels, scale, ii))
    d3 = dl.clone(); r, cidx = [int(v[0]) for v in torch.isneginf(logits).nonzero(as_tuple=True)]
    d3[r, cidx] = 1e-30
    rejected(lambda: rf.check_ce("mut", loss, d3, logits, labels, scale, ii))                  # a non-zero gradient in a -inf column
    rejected(lambda: rf.check_ce("mut", loss + float("nan"), dl, logits, labels, scale, ii))   # accumulated onto the NaN fill
    rejected(lambda: rf.check_ce("mut", loss + 1.0, dl, logits, labels, scale, ii))            # ... onto a previous loss
    # every row ignored: an exact zero is demanded
    lab = torch.full_like(labels, ii)
    rejected(lambda: rf.check_ce("mut", torch.tensor(1e-30), None, logits, lab, scale, ii))


# ---- sums and casts ------------------------------------------------------------------------------------------------------------
def test_colsum_emulation_inside_bounds_and_mutation():
    for M in rf.COLSUM_M:
        for N in rf.COLSUM_N:
            for dt in (torch.float32, torch.bfloat16):
                dy, init, bound, sent = rf.colsum_case(M, N, dt, seed=M * N)
                rf.within(("emulated colsum", "db"), rf.emulate_colsum(dy, init), init.to(F64) + rf.colsum(dy), bound)
    dy, init, bound, sent = rf.colsum_case(333, 776, torch.float32, seed=2)
    ref = init.to(F64) + rf.colsum(dy)
    rejected(lambda: rf.within(("mut", "db"), ref - dy[332].to(F64), ref, bound))                # missing row M - 1
    rejected(lambda: rf.within(("mut", "db"), ref - dy[320].to(F64), ref, bound))                # ... the last block's first row
    rejected(lambda: rf.within(("mut", "db"), rf.colsum(dy), ref, bound))                        # stored instead of accumulated


def test_gather_emulation_inside_bounds_and_mutation():
    for N in rf.GATHER_N:
        for H in rf.GATHER_H:
            for dt in (torch.float32, torch.bfloat16):
                for acc in (0, 1):
                    src, ptr, idx, w, init = rf.gather_case(N, H, dt, seed=N + H)
                    ref, mag, lens = rf.gather_sum(src, ptr, idx, w, init if acc else None)
                    got = rf.emulate_gather(src, ptr, idx, w, init, acc, dt)
                    rf.within(("emulated gather_sum", "out"), got, ref, rf.gather_bound(ref, mag, lens, acc, dt == torch.bfloat16))
    src, ptr, idx, w, init = rf.gather_case(5, 256, torch.float32, seed=1)
    ref, mag, lens = rf.gather_sum(src, ptr, idx, w, init)
    stored = rf.gather_sum(src, ptr, idx, w, None)[0]
    rejected(lambda: rf.within(("mut", "out"), stored, ref, rf.gather_bound(ref, mag, lens, 1, False)))   # storing instead of accumulating


def test_cast_mutations_are_rejected():
    x = torch.cat([rf.cast_specials(), torch.randn(1000)])
    rf.check_cast("reference", x.to(torch.bfloat16), x)
    trunc = (x.view(torch.int32) & -65536).view(torch.float32).to(torch.bfloat16)
    rejected(lambda: rf.check_cast("mut", trunc, x))                                             # truncation
    inf = x.to(torch.bfloat16).clone(); inf[torch.isnan(x)] = float("inf")
    rejected(lambda: rf.check_cast("mut", inf, x))                                               # NaN cast to inf


# ---- sum of squares ------------------------------------------------------------------------------------------------------------
def test_sumsq_emulation_inside_bound_and_mutation():
    for n in rf.SQNORM_N:
        for masked in (False, True):
            g = torch.randn(n) * 0.3
            g[-1] = 30.0                                           # the last float4 / second sweep carries a term far above the bound
            mask = rf.adamw_mask(n, seed=n) if masked else None
            if masked and n >= 1028:
                mask[-1] = 1
            start = 2.5
            ref = float(rf.sumsq(g, mask)[0]) + start
            b = rf.sumsq_bound(g, mask, start)
            assert 900.0 > 8 * b
            got = float(rf.emulate_sumsq(g, mask, start))
            assert abs(got - ref) <= b, (n, masked, abs(got - ref) / b)
            assert abs(ref - 900.0 - ref) > b                      # the last element dropped
            if masked and n >= 1028:
                unmasked = float(rf.sumsq(g, None)[0]) + start     # frozen blocks contributing
                assert abs(unmasked - ref) > b


# ---- AdamW ---------------------------------------------------------------------------------------------------------------------
HYPER = rf.HYPER


def _state(n, seed):
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(n, generator=g) * 0.3, torch.randn(n, generator=g) * 0.05, torch.rand(n, generator=g) * 0.01)


def test_adamw_emulation_inside_bounds():
    """exact operation order, three steps, both styles x bias correction x hyper-parameters x grad_scale, clipping and not, host and
    device (fp32 powf) bias corrections; includes elements whose update nearly cancels p.  Every size of ADAMW_N; at the largest
    (4 194 304 + 1028: second sweep, partial mask block) the hyper-parameter pair and the counted flag alternate over the four
    (formulation, bias correction) combinations instead of being crossed with them."""
    i = 0
    for n in rf.ADAMW_N:
        mask = rf.adamw_mask(n, seed=n)
        big = n > (1 << 20)
        for hf in (0, 1):
            for cb in (0, 1):
                for hi, (b1, b2, eps) in enumerate(HYPER):
                    for counted in (False, True):
                        if big and (hi != (hf + cb) % 2 or counted != bool(hf ^ cb)):
                            continue
                        gs = (1.0, 0.5, 1.0 / 65536)[i % 3]
                        mn = (0.0, 1.0, 5.0)[(i // 3) % 3]
                        i += 1
                        p, m, v = _state(n, i)
                        for step in (1, 2, 3):
                            cfg = rf.cfg_f32(lr=3e-3, beta1=b1, beta2=b2, eps=eps, weight_decay=0.01, step=step, hf_style=hf, correct_bias=cb,
                                             grad_scale=gs, max_norm=mn)
                            g = torch.randn(n) * (40.0 if step == 2 else 0.02) / gs
                            if step == 1:
                                m, v = torch.zeros(n), torch.zeros(n)
                                p[: n // 8] = 0.0                               # an all-zero parameter: the update is everything
                            if step == 3:
                                p[::7] = rf.adamw(p, g, m, v, cfg, None, mask)["upd"][::7].float()   # update nearly cancels p
                            ss = float(rf.emulate_sumsq(g, mask, 0.0))
                            r = rf.adamw(p, g, m, v, cfg, ss, mask, steps_applied=step - 1 if counted else None)
                            got = rf.emulate_adamw(p, g, m, v, cfg, ss, mask, counted_step=step if counted else None)
                            rf.check_adamw("emulated adamw", got, (p, m, v), r, cfg, counted)
                            p, m, v = got


def _adamw_setup(hf=0, cb=1, max_norm=1.0, gs=0.5, b2=0.999, eps=1e-8):
    n = 1028
    mask = rf.adamw_mask(n, seed=1)
    p, m, v = _state(n, 2)
    g = torch.randn(n) * 3.0
    cfg = rf.cfg_f32(lr=3e-3, beta1=0.9, beta2=b2, eps=eps, weight_decay=0.01, step=2, hf_style=hf, correct_bias=cb, grad_scale=gs,
                     max_norm=max_norm)
    ss = float(rf.sumsq(g, mask)[0])
    return n, mask, (p, m, v), g, cfg, ss


def _as_got(r):
    return (r["p"].float(), r["m"].float(), r["v"].float())


@pytest.mark.parametrize("hf", [0, 1])
def test_adamw_mutations_are_rejected(hf):
    n, mask, old, g, cfg, ss = _adamw_setup(hf=hf)
    r = rf.adamw(*old[:1], g, *old[1:], cfg, ss, mask)
    rf.check_adamw("reference", _as_got(r), old, r, cfg, False)

    def mutant(mask2=None, cfg2=None, ss2=None, **kw):
        return _as_got(rf.adamw(old[0], g, old[1], old[2], cfg2 or cfg, ss if ss2 is None else ss2, mask if mask2 is None else mask2, **kw))

    m2 = mask.clone(); m2[mask == 0] = 1
    rejected(lambda: rf.check_adamw("mut", mutant(m2), old, r, cfg, False))                    # decay applied under mask byte 0
    m2 = mask.clone(); m2[(mask == 2) | (mask == 3)] = 1
    rejected(lambda: rf.check_adamw("mut", mutant(m2), old, r, cfg, False))                    # a frozen block updated
    m2 = mask.clone(); m2[mask == 255] = 3
    rejected(lambda: rf.check_adamw("mut", mutant(m2), old, r, cfg, False))                    # byte 255 treated as frozen
    rejected(lambda: rf.check_adamw("mut", mutant(ss2=ss / cfg["grad_scale"] ** 2), old, r, cfg, False))   # clip without |grad_scale|
    c2 = dict(cfg, hf_style=1 - hf)
    rejected(lambda: rf.check_adamw("mut", mutant(cfg2=c2), old, r, cfg, False))               # the two formulations swapped
    # eps inside the square root
    q = rf.adamw(old[0], g, old[1], old[2], cfg, ss, mask)
    bc2 = 1 - cfg["beta2"] ** 2
    # (at the ABI's eps = 1e-8 and v ~ 1e-3 the two forms agree to 1e-6 relative of the update, below the bound: no elementwise bound can
    # tell them apart there, so the mutation is shown at eps = 1e-3, where sqrt(v + eps) and sqrt(v) + eps differ by tens of per cent)
    c3 = dict(cfg, eps=1e-3)
    q3 = rf.adamw(old[0], g, old[1], old[2], c3, ss, mask)
    den3 = torch.sqrt(q3["v"] + c3["eps"]) if hf else torch.sqrt(q3["v"] / bc2 + c3["eps"])
    pw3 = (old[0].to(F64) - q3["coef"] * q3["m"] / den3) * (1 - c3["lr"] * c3["weight_decay"]) if hf else q3["q"] - q3["coef"] * q3["m"] / den3
    pw3 = torch.where(q3["frozen"], old[0].to(F64), pw3)
    rejected(lambda: rf.check_adamw("mut", (pw3.float(), q3["m"].float(), q3["v"].float()), old, q3, c3, False))
    # the bias correction advanced across a skipped step: the counter says 1 applied update, a wrong kernel uses step 3
    rc = rf.adamw(old[0], g, old[1], old[2], cfg, ss, mask, steps_applied=1)
    rejected(lambda: rf.check_adamw("mut", mutant(steps_applied=2), old, rc, cfg, True))
    rs = rf.adamw(old[0], g, old[1], old[2], cfg, ss, mask, skip=True, steps_applied=1)
    assert rs["counter"] == 1
    rejected(lambda: rf.check_adamw("mut", _as_got(rc), old, rs, cfg, True))                   # a skipped step that updated
    # gradients: a frozen block's gradient left non-zero; zero_grads = 0 must leave them alone
    g_after = torch.zeros(n); g_after[rf.frozen_elems(mask, n)] = g[rf.frozen_elems(mask, n)]
    rejected(lambda: rf.check_grads_after("mut", g_after, g, 1))
    rejected(lambda: rf.check_grads_after("mut", torch.zeros(n), g, 0))
    rf.check_grads_after("reference", torch.zeros(n), g, 1)
    # shadow
    got = _as_got(r)
    n_shadow = 512
    sh_old = torch.randn(n).to(torch.bfloat16)
    good = sh_old.clone()
    live = ~r["frozen"][:n_shadow]
    good[:n_shadow][live] = rf.bf16_rne(got[0][:n_shadow])[live]
    rf.check_adamw("reference", got, old, r, cfg, False, good, sh_old, n_shadow)
    trunc = good.clone()
    trunc[:n_shadow][live] = (got[0][:n_shadow].view(torch.int32) & -65536).view(torch.float32).to(torch.bfloat16)[live]
    rejected(lambda: rf.check_adamw("mut", got, old, r, cfg, False, trunc, sh_old, n_shadow))  # the shadow truncated
    past = good.clone()
    lv = ~r["frozen"][n_shadow:n_shadow + 4]
    past[n_shadow:n_shadow + 4] = rf.bf16_rne(got[0][n_shadow:n_shadow + 4])
    assert bool(lv.any())
    rejected(lambda: rf.check_adamw("mut", got, old, r, cfg, False, past, sh_old, n_shadow))   # the shadow written past n_shadow


def test_adamw_bound_in_p_new_alone_would_fail():
    """why the bound is written in |p_old|, |p_new| and |update|: where the update nearly cancels p, u |p_new| is far below the
    rounding of the update itself"""
    n, mask, (p, m, v), g, cfg, ss = _adamw_setup(max_norm=0.0)
    p = rf.adamw(p, g, m, v, cfg, ss, None)["upd"].float()
    r = rf.adamw(p, g, m, v, cfg, ss, None)
    got = rf.emulate_adamw(p, g, m, v, cfg, ss, None)
    rf.check_adamw("emulated adamw", got, (p, m, v), r, cfg, False)
    err = (got[0].to(F64) - r["p"]).abs()
    assert bool((err > 16 * rf.U * r["p"].abs()).any())
