"""The comparator of the attention op tests (tests/attn_ref.py `close` + the bounds of `attn_ref`) can pass and can fail.

Pass: CPU emulations of the four families' rounding schedules -- every product and sum in float64, rounded to fp32 / bf16 exactly
where the kernels hold fp32 / store bf16 -- stay within ratio 1 of the bound on the full shape list of the GPU tests:

  rows    register-resident (attn_rows.hip): fp32 softmax, P and dS rounded to bf16 before their products, D = rowsum(P dP) from the
          unrounded P, every output rounded to bf16
  tile    LDS-tile (attn.hip attn_fwd_kernel / attn_bwd_kernel): the same with the STORED bf16 P in D and dS
  flash   streaming (attn.hip flash_*): online softmax over 128-key tiles, exp(s - m_run) rounded to bf16 per tile, fp32 rescale of
          the accumulator when a later tile raises the maximum, a fully excluded prefix contributes nothing; the backward recomputes
          P from lse and takes D = rowsum(dO * O) from the rounded O
  gemm    batched-GEMM in bf16 (planner.hip): alpha Q.K^T, P, dP and dS each stored in bf16 between the launches
  f32     any fp32 family: everything in fp32 (u = 0: only the fp32 term of the bound, and E_s on fully masked mask_mode 0 rows)

Fail: each mutation of MUTATIONS, applied to the emulation of the family it could happen in, must raise in the shapes listed beside
it (at least one of them with Lk >= 128).  A mutation is looked for in every shape of its list; a shape where it stays inside the
bound would fail this test, not be skipped.
"""
import pytest
import torch

from tests import attn_ref as ar

F64 = torch.float64
rb = lambda x: x.to(torch.bfloat16).to(F64)
rf = lambda x: x.to(torch.float32).to(F64)
T = lambda x: x.transpose(-1, -2)


def scores(c, mut, stored_bf16=False):
    """fp32 scores as the kernels form them: alpha q.k (+ rounded to bf16 on the bf16 batched-GEMM path), + key term, + bias"""
    q, k = c["q"].to(F64), c["k"].to(F64)
    alpha = 0.125 if mut == "alpha_fixed" else c["alpha"]
    s = rf(alpha * (q @ T(k)))
    if stored_bf16:
        s = rb(s)
    if c["km"] is not None:
        km = c["km"].clone()
        if mut == "mask_key0":
            km[:, 0] = True
        if mut == "mask_last":
            km[:, -1] = True
        neg = float("-inf") if (c["mask_mode"] or mut == "mode0_as_1") else -10000.0
        s = rf(s + torch.where(km, 0.0, neg).to(F64)[:, None, None, :])
    if c["dist"] is not None:
        dist = c["dist"].to(F64)
        if mut == "dist_batch0":
            dist = dist[:1].expand_as(dist)
        s = rf(s + rf(dist * c["sp_w"] + c["sp_b"])[:, None])
    if mut == "drop_key":                      # the valid key with the least total probability is never seen
        p = torch.softmax(s, -1).sum(2)                                      # [B, nh, Lk]
        if c["km"] is not None:
            p = p.masked_fill(~c["km"][:, None, :], float("inf"))
        kk = p.argmin(-1)                                                    # [B, nh]
        s = s.clone()
        s.scatter_(3, kk[:, :, None, None].expand(-1, -1, s.shape[2], 1), float("-inf"))
    return s


def emulate(c, family, mut=None):
    """-> dict like attn_ref's values (d_sp_* as the gradient alone, or as what a buffer holding D_INIT ends with: see `run`)"""
    bf = c["bf16"]
    r = rb if bf else rf
    stored = family in ("tile", "gemm")
    q, k, v, do = (c[n].to(F64) for n in ("q", "k", "v", "dctx"))
    alpha = 0.125 if mut == "alpha_fixed" else c["alpha"]
    s = scores(c, mut, stored_bf16=(family == "gemm" and bf))
    if family == "flash":
        Lk = s.shape[-1]
        m_run = torch.full(s.shape[:-1] + (1,), float("-inf"), dtype=F64)
        l_run = torch.zeros_like(m_run)
        acc = torch.zeros(s.shape[:-1] + (64,), dtype=F64)
        for k0 in range(0, Lk, 128):
            st = s[..., k0:k0 + 128]
            m_new = torch.maximum(m_run, st.amax(-1, keepdim=True))
            mref = torch.where(torch.isinf(m_new), torch.zeros_like(m_new), m_new)          # fully excluded prefix: no NaN
            e = rf(torch.exp(st - mref))
            scale = rf(torch.exp(m_run - mref))
            l_run = rf(l_run * scale + e.sum(-1, keepdim=True))
            if mut != "no_rescale":
                acc = acc * scale
            acc = rf(acc + rb(e) @ v[..., k0:k0 + 128, :])
            m_run = m_new
        ctx = r(acc / l_run)
        lse = rf(m_run + torch.log(l_run))
        p = rf(torch.exp(s - lse))
    else:
        mx = s.amax(-1, keepdim=True)
        e = rf(torch.exp(s - mx))
        p = rf(e / e.sum(-1, keepdim=True))
        ctx = None
    pb = r(p)
    if ctx is None:
        ctx = r(pb @ v)
    dv = r(T(pb) @ do)
    dp = rf(do @ T(v))
    if family == "gemm":
        dp = r(dp)
    ps = pb if stored else p
    D = rf((do * ctx).sum(-1, keepdim=True)) if family == "flash" else rf((ps * dp).sum(-1, keepdim=True))
    ds = r(ps * (dp - D))
    dq = r((1.0 if mut == "dq_no_alpha" else alpha) * (ds @ k))
    dk = r(alpha * (T(ds) @ q))
    if mut == "swap_heads_dk" and dk.shape[1] > 1:
        dk = dk[:, [1, 0] + list(range(2, dk.shape[1]))]
    if mut == "last_row_nan":
        ctx = ctx.clone()
        ctx[:, :, -1] = float("nan")
    out = {"ctx": ctx, "dQ": dq, "dK": dk, "dV": dv}
    if c["dist"] is not None:
        out["d_sp_w"] = rf((ds.sum(1) * c["dist"].to(F64)).sum())
        out["d_sp_b"] = rf(ds.sum())
    return out


def d_init(E):
    """what the d_sp_w / d_sp_b buffers hold before the call: a previous gradient a few bounds large, as the GPU test sets it (a
    store in place of the accumulation must not hide inside the bound of the sum)"""
    return (2.5 * float(E["d_sp_w"]), -3.0 * float(E["d_sp_b"])) if "d_sp_w" in E else None


def run(c, family, mut=None):
    """emulate + compare as the GPU test does; raises AssertionError beyond the bound"""
    val, E = ar.ref_of(c, gemm=(family == "gemm"))
    got = emulate(c, family, mut)
    init = d_init(E)
    if init and mut != "dw_stored":                        # the kernels accumulate into the buffers
        got["d_sp_w"], got["d_sp_b"] = rf(got["d_sp_w"] + init[0]), rf(got["d_sp_b"] + init[1])
    ar.check_all(got, val, E, f"{family} {c['Lq']}x{c['Lk']}", f"cpu-{family}-{'bf16' if c['bf16'] else 'fp32'}", init)


def small(x):
    """the grid's case with the batch cut to <= 3 entries and 2 heads (the CPU emulation walks the same generator)"""
    Lq, Lk, B, nh, mm, wd, alpha, spw, sd, rot, nm = x
    return (Lq, Lk, min(B, 3), 2, mm, wd, alpha, spw, sd, rot, nm)


def ids(g):
    return [f"{x[0]}x{x[1]}-B{x[2]}-m{x[4]}-{'dist' if x[5] else 'nodist'}-a{x[6]}-s{x[8]}{'-nullmask' if x[10] else ''}" for x in g]


SHORT_G = [small(x) for x in ar.case_grid(ar.SHORT)]
LONG_G = [small(x) for x in ar.case_grid(ar.LONG, dist_ok=False)]
LONG_GD = [small(x) for x in ar.case_grid(ar.LONG)]


@pytest.mark.parametrize("family", ["rows", "tile", "gemm"])
@pytest.mark.parametrize("x", SHORT_G, ids=ids(SHORT_G))
def test_bf16_schedules_stay_inside_the_bound_short(x, family):
    Lq, Lk, B, nh, mm, wd, alpha, spw, sd, rot, nm = x
    run(ar.make_case(Lq, Lk, B, nh, True, mm, wd, alpha, spw, sd, rot, nm), family)


@pytest.mark.parametrize("x", LONG_G, ids=ids(LONG_G))
def test_streaming_schedule_stays_inside_the_bound(x):
    Lq, Lk, B, nh, mm, wd, alpha, spw, sd, rot, nm = x
    run(ar.make_case(Lq, Lk, B, nh, True, mm, False, alpha, spw, sd, rot, nm), "flash")


@pytest.mark.parametrize("bf16", [True, False], ids=["bf16", "fp32"])
@pytest.mark.parametrize("x", LONG_GD, ids=ids(LONG_GD))
def test_batched_gemm_schedule_stays_inside_the_bound_long(x, bf16):
    Lq, Lk, B, nh, mm, wd, alpha, spw, sd, rot, nm = x
    run(ar.make_case(Lq, Lk, B, nh, bf16, mm, wd, alpha, spw, sd, rot, nm), "gemm" if bf16 else "f32")


@pytest.mark.parametrize("x", SHORT_G, ids=ids(SHORT_G))
def test_fp32_schedule_stays_inside_the_bound_short(x):
    Lq, Lk, B, nh, mm, wd, alpha, spw, sd, rot, nm = x
    run(ar.make_case(Lq, Lk, B, nh, False, mm, wd, alpha, spw, sd, rot, nm), "f32")


def test_worst_ratios_are_reported():
    """after the schedules above (pytest -s prints the table); every recorded ratio is <= 1 by construction of `close`"""
    print("\nattention bound, worst |emulation - fp64| / E per (schedule, tensor): " +
          ", ".join(f"{k} {v:.2f}" for k, (v, _) in sorted(ar.WORST.items()) if k.startswith("cpu-")))
    assert all(v <= 1.0 for k, (v, _) in ar.WORST.items() if k.startswith("cpu-"))


# ---- the comparator can fail ---------------------------------------------------------------------------------------------------
# (Lq, Lk, B, mask_mode, with_dist, alpha, mask pattern of batch entry 0 .. as a rotation, null mask)
def mcase(Lq, Lk, B=3, mm=0, wd=False, alpha=0.125, rot=0, nm=False, seed=0, spw=0.3):
    return ar.make_case(Lq, Lk, B, 2, True, mm, wd, alpha, spw, seed, rot, nm)


# rotations: MASKS = all, first, last, not0, tail, lead, none -> rot r gives batch entries the patterns r, r+1, r+2
MUTATIONS = {
    # name: (family, [case kwargs ...]) -- every listed case must raise
    "drop_key": ("rows", [dict(Lq=16, Lk=128), dict(Lq=80, Lk=80, wd=True), dict(Lq=113, Lk=16, mm=1)]),
    "drop_key_streaming": ("flash", [dict(Lq=512, Lk=512), dict(Lq=16, Lk=512, mm=1)]),
    "mask_key0": ("rows", [dict(Lq=16, Lk=128, rot=3), dict(Lq=36, Lk=36, rot=3, mm=1), dict(Lq=130, Lk=300, rot=3)]),
    "mask_last": ("rows", [dict(Lq=16, Lk=128, rot=4), dict(Lq=80, Lk=80, rot=4, mm=1), dict(Lq=64, Lk=129, rot=4)]),
    "mode0_as_1": ("rows", [dict(Lq=16, Lk=128, rot=6), dict(Lq=36, Lk=36, rot=6, wd=True)]),
    "alpha_fixed": ("rows", [dict(Lq=16, Lk=128, alpha=0.2), dict(Lq=80, Lk=80, alpha=0.2), dict(Lq=1, Lk=640, alpha=0.2, nm=True)]),
    "dist_batch0": ("rows", [dict(Lq=128, Lk=128, wd=True, nm=True), dict(Lq=16, Lk=16, wd=True, spw=-1.7, nm=True)]),
    "swap_heads_dk": ("rows", [dict(Lq=16, Lk=128), dict(Lq=15, Lk=17), dict(Lq=300, Lk=70)]),
    "dw_stored": ("rows", [dict(Lq=128, Lk=128, wd=True), dict(Lq=16, Lk=80, wd=True, B=1)]),
    "last_row_nan": ("rows", [dict(Lq=17, Lk=128), dict(Lq=97, Lk=64), dict(Lq=1, Lk=1)]),
    "no_rescale": ("flash", [dict(Lq=16, Lk=512, nm=True), dict(Lq=130, Lk=300, nm=True), dict(Lq=512, Lk=512, nm=True)]),
    "dq_no_alpha": ("rows", [dict(Lq=16, Lk=128), dict(Lq=80, Lk=80, alpha=0.2), dict(Lq=257, Lk=255)]),
}
MUT_PARAMS = [pytest.param(name, fam, kw, id=f"{name}-{kw['Lq']}x{kw['Lk']}") for name, (fam, cases) in MUTATIONS.items() for kw in cases]


def test_every_mutation_lists_a_long_key_axis():
    for name, (_, cases) in MUTATIONS.items():
        assert any(kw["Lk"] >= 128 for kw in cases), name


@pytest.mark.parametrize("name,family,kw", MUT_PARAMS)
def test_mutation_is_caught(name, family, kw):
    c = mcase(**kw)
    fam = "flash" if (family == "rows" and max(kw["Lq"], kw["Lk"]) > 128) else family
    run(c, fam)                                              # the clean emulation of the same case passes
    with pytest.raises(AssertionError):
        run(c, fam, name.replace("_streaming", ""))
