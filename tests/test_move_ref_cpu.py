"""tests/move_ref.py without a GPU.

PIN: the restatements equal the code they restate at 1e-12 -- the MLM loss and its gradient F.cross_entropy(reduction='none').mean()
and its autograd, gelu' torch's erf-GELU autograd in float64 (NaN at +-inf included), the sequence mask etpnav_amd.ops.gen_seq_masks,
the vp_gather ordering the recorded output of the trainer's own _vp_feature_variable (tests/golden/vp_inputs.npz).
REACH: each case reaches what it claims, on the reference alone -- second grid trip, tail length, label positions, -inf columns,
every pattern with both dtypes; every index schedule writes every element exactly once.
PASS: fp32 emulations of every kernel's schedule stay inside the bound on every case the GPU file runs.
FAIL: the planted mutations of the reference output are rejected by the comparators the GPU file calls.
"""
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from tests import move_ref as mv

F64 = torch.float64
TDT = mv.TDT


def rejected(fn):
    with pytest.raises(AssertionError):
        fn()


# ---- pins ----------------------------------------------------------------------------------------------------------------------
def test_vocab_ce_restatement_is_cross_entropy_mean():
    for i, (dt, V, ldv, Nm, pat) in enumerate(mv.vce_cases()):
        if V == 30522 and Nm == 5 or i % 9:
            continue
        c = mv.vce_reference(mv.vce_case(V, ldv, Nm, pat, seed=i), False)
        x = c["buf"][:, :V].to(F64).requires_grad_(True)
        k = c["scale"] * Nm                                             # scale = k / Nm: the mean, times what scale adds to it
        loss = F.cross_entropy(x, c["labels"], reduction="none").mean() * k
        loss.backward()
        loss = loss.detach()
        assert abs(float(loss) + c["start"] - float(c["loss"])) <= 1e-12 * max(1.0, abs(float(loss)))
        assert float((x.grad - c["dl"][:, :V]).abs().max()) <= 1e-12
        assert bool((c["dl"][:, V:] == 0).all())


def test_gelu_grad_is_torch_erf_gelu_autograd():
    d, z = mv.gelu_case(1000, torch.float32, seed=1)
    x = z.to(F64).requires_grad_(True)
    F.gelu(x).backward(d.to(F64))
    ref = mv.gelu_bwd(d, z)
    inf = torch.isinf(z)
    assert int(inf.sum()) == 4 and bool(torch.isnan(ref[inf]).all()) and bool(torch.isnan(x.grad[inf]).all())
    assert float((x.grad - ref)[~inf].abs().max()) <= 1e-12 * float(d.abs().max())
    assert abs(float(mv.gelu_grad(torch.tensor(mv.GELU_ZERO, dtype=F64)))) < 1e-9      # the zero of gelu' is where the list says


def test_seq_mask_is_gen_seq_masks():
    from etpnav_amd.ops import gen_seq_masks
    for i, (B, V) in enumerate(mv.SEQ_SHAPES):
        lens = mv.seq_lens(B, V, seed=i)
        assert torch.equal(mv.seq_mask(lens, V), gen_seq_masks(lens, V).to(torch.uint8))


def test_vp_gather_restatement_matches_the_recorded_trainer_output():
    from oracle.make_golden_vp import make_obs
    z = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "vp_inputs.npz"))
    obs = make_obs()
    for name, ck, pk in (("rgb_fts", "cand_rgb", "pano_rgb"), ("dep_fts", "cand_depth", "pano_depth"), ("loc_fts", "cand_angle_fts", "pano_angle_fts")):
        out, nav, lens = mv.vp_gather(*mv.vp_from_obs(obs, ck, pk))
        assert float((out.to(F64) - torch.from_numpy(z["out/" + name]).to(F64)).abs().max()) <= 1e-12
        assert np.array_equal(nav.numpy(), z["out/nav_types"]) and np.array_equal(lens.numpy(), z["out/view_lens"])


# ---- reach ---------------------------------------------------------------------------------------------------------------------
def test_vocab_ce_cases_reach_what_they_claim():
    cases = mv.vce_cases()
    assert {c[1] for c in cases} == set(mv.VCE_V) and len(cases) == 7 * 2 * 4 * 2 + 2 * 2 * 2
    for dt in ("fp32", "bf16"):
        mine = [c for c in cases if c[0] == dt]
        assert {c[4][0] for c in mine} == {0.0, 80.0, -80.0, "dom"} and {c[4][1] for c in mine} == {"mean", "fixed"}
        assert {c[4][2] for c in mine} == {0.0, 3.25}
        assert {(c[2] - c[1] == 16) for c in mine if c[1] == 30522} == {True, False}
    assert {c[3] for c in cases if c[1] == 30522} == {1, 5} and {c[3] for c in cases if c[1] != 30522} == set(mv.VCE_NM)
    seen = set()
    for i, (dt, V, ldv, Nm, pat) in enumerate(cases):
        assert ldv in (mv.round_up(V, 8), V + 16) and ldv >= V
        if V == 30522 and i % 2:
            continue
        c = mv.vce_case(V, ldv, Nm, pat, seed=i)
        s, y = c["buf"][:, :V], c["labels"]
        assert bool((c["buf"][:, V:] == mv.VCE_PAD).all()) and bool(((y >= 0) & (y < V)).all())
        assert bool(torch.isfinite(s.gather(1, y[:, None])).all())                      # no label names a -inf column
        if V > 2:
            assert bool(torch.isneginf(s).any(1).all())                                   # at least one -inf column in every row
        if Nm >= 3:
            assert int(y[0]) == 0 and int(y[-1]) == V - 1 and int(y[Nm // 2]) == int(s[Nm // 2].argmax())
        else:
            seen.add((int(y[0]) == 0, int(y[0]) == V - 1, int(y[0]) == int(s[0].argmax())))
        if pat[0] == "dom" and V > 2:
            top = s.topk(2, dim=1).values
            assert bool((top[:, 0] - top[:, 1] > mv.VCE_DOM - 30).any())
        p = mv.vce_reference(c, False)["q"]["p"]
        assert float(p[p > 0].min()) * c["scale"] > mv.TINY                               # no subnormal gradient
    assert {a for a, _, _ in seen} == {True, False} and {b for _, b, _ in seen} == {True, False} and any(c for _, _, c in seen)


def test_schedules_write_every_element_once_and_reach_their_second_trip():
    def run(kernel, n, trips=None, tail=None):
        count, blocks, tr, nt = mv.schedule(kernel, n)
        assert bool((count == 1).all()), (kernel, n)
        if trips is not None:
            assert (tr, nt) == (trips, tail), (kernel, n, tr, nt)
        return blocks
    assert [n % 4 for n in mv.COPY_N] == [1, 3, 0, 1, 3, 3] and [n % 4 for n in mv.ZERO_N] == [0, 1, 3, 0, 1, 3, 3]
    for n in mv.COPY_N:
        run("copy_f32", n, 2 if n > 4 * 2048 * 256 else (1 if n >= 4 else 0), n % 4)
    for n in mv.ZERO_N:
        run("zero_f32", n, 2 if n > 4 * 4096 * 256 else (1 if n >= 4 else 0), n % 4)
    assert run("copy_f32", mv.COPY_N[-1]) == 2048 and run("zero_f32", mv.ZERO_N[-1]) == 4096
    for n in mv.CASTTO_N:
        run("cast_drop", n, 2 if n > 4 * 4096 * 256 else 1, 0)
    assert 1028 // 4 % 256 != 0                                     # n / 4 no multiple of the block: the `i + 4 <= n` guard is exercised
    for n in mv.SUM_N:
        run("sum_steps", n, 2 if n == mv.SUM_BIG else 1, 0)
    for b in mv.REPEAT_BYTES:
        assert b % 16 == 0
        run("repeat_block", b // 16, 2 if b // 16 > 4096 * 256 else 1, 0)
    for n in mv.GELU_N:
        run("gelu_bwd", n, 2 if n > 2048 * 256 else 1, 0)
    assert mv.GELU_N[-1] - 2048 * 256 == 1029
    d, z = mv.gelu_case(mv.GELU_N[-1], torch.float32, seed=0)
    second = z[2048 * 256:]
    assert int(torch.isinf(second).sum()) == 2 and bool((second == 0).any()) and float(z[~torch.isinf(z)].abs().max()) == 10.0
    assert bool((z == mv.f32(mv.GELU_ZERO)).any())


def test_seq_and_vp_cases_reach_what_they_claim():
    for i, (B, V) in enumerate(mv.SEQ_SHAPES):
        lens = mv.seq_lens(B, V, seed=i)
        if B >= 5:
            assert lens[:5].tolist() == [0, 1, V - 1, V, V + 5]
    assert {int(mv.seq_lens(1, 1, s)) for s in range(5)} == {0, 1, 6}
    cases = mv.vp_cases()
    assert {(c[0], c[1], c[2]) for c in cases} == {(b, p, f) for b in mv.VP_B for p in mv.VP_P for f in mv.VP_F}
    assert {c[4] for c in cases} == set(mv.VP_MASKS) and {c[5] for c in cases} == {0, 3} and {c[6] for c in cases} == {True, False}
    assert {c[7] for c in cases} == {True, False}
    assert any(sum(c[3]) == 0 for c in cases) and any(c[1] in c[3] and 0 in c[3] and 1 in c[3] for c in cases)
    assert any(sum(c[3]) == 0 and c[4] == "all" for c in cases)                     # an output of zero rows only
    full = False
    for i, case in enumerate(cases):
        c = mv.vp_case(case, seed=i)
        assert max(1, max(c["lens"])) + case[5] == c["V"] and (c["cand"] is None) == (sum(case[3]) == 0)
        assert (c["stride"] == 0) == case[6] == (c["pano"].dim() == 2)
        full = full or (case[5] == 0 and c["V"] == case[1] + max(case[3]))
    assert full                                                                      # every view free AND P candidates: V = 2 P


# ---- emulations inside the bounds ----------------------------------------------------------------------------------------------
def test_vocab_ce_emulation_inside_bounds():
    for i, (dt, V, ldv, Nm, pat) in enumerate(mv.vce_cases()):
        c = mv.vce_reference(mv.vce_case(V, ldv, Nm, pat, seed=i), dt == "bf16")
        loss, dl = mv.emulate_vce(c, TDT[dt])
        mv.check_vce("emulated vocab_ce " + dt, c, loss, dl)


def test_gelu_emulation_inside_bounds():
    for i, (dt, n) in enumerate(mv.gelu_cases()):
        d, z = mv.gelu_case(n, TDT[dt], seed=i)
        mv.check_gelu("emulated gelu_bwd " + dt, mv.emulate_gelu(d, z), d, z)


def test_sum_steps_emulation_inside_bounds():
    for i, (dt, n, steps) in enumerate(mv.sum_cases()):
        src = mv.sum_case(n, steps, TDT[dt], seed=i)
        mv.check_sum("emulated sum_steps " + dt, mv.emulate_sum(src), src)
        if steps > 1:                                                # the planted cancellation is there
            ref, mag = mv.sum_steps(src)[::3], src.to(F64).abs().sum(0)[::3]
            assert float((ref.abs() / mag).max()) < 2.0 ** -6


# ---- mutations -----------------------------------------------------------------------------------------------------------------
def test_vocab_ce_mutations_are_rejected():
    V, ldv, Nm = 257, 264, 77
    for bf16 in (False, True):
        c = mv.vce_reference(mv.vce_case(V, ldv, Nm, (0.0, "mean", 3.25), seed=4), bf16)
        dt = torch.bfloat16 if bf16 else torch.float32
        cast = lambda t: mv.bf16_rne(t.float()) if bf16 else t.float()
        loss, dl, q, scale = c["loss"], c["dl"], c["q"], c["scale"]
        mv.check_vce("reference", c, loss, cast(dl))
        assert cast(dl).dtype == dt
        for shift in (1, -1):                                        # onehot in column y +- 1
            hot = torch.zeros(Nm, V, dtype=F64).scatter_(1, ((c["labels"] + shift) % V)[:, None], 1.0)
            wrong = dl.clone()
            wrong[:, :V] = scale * (q["p"] - hot)
            rejected(lambda: mv.check_vce("mut", c, loss, cast(wrong)))
        wrong = dl.clone()
        wrong[Nm - 1, ldv - 1] = 1e-30                               # a padding column that is not zero
        rejected(lambda: mv.check_vce("mut", c, loss, cast(wrong)))
        wrong = dl.clone()
        wrong[:, V:] = float("nan")                                  # ... or was never written
        rejected(lambda: mv.check_vce("mut", c, loss, cast(wrong)))
        s = q["s"]
        lse2 = q["mx"] + torch.log(torch.exp(s[:, :V - 1] - q["mx"]).sum(-1, keepdim=True))     # the last column dropped from the sum
        wrong = dl.clone()
        wrong[:, :V] = scale * (torch.exp(s - lse2) - q["onehot"])
        nll2 = (lse2 - s.gather(1, c["labels"][:, None])).squeeze(1)
        rejected(lambda: mv.check_vce("mut", c, loss, cast(wrong)))
        rejected(lambda: mv.check_vce("mut", c, c["start"] + scale * nll2.sum(), cast(dl)))
        rejected(lambda: mv.check_vce("mut", c, loss - c["start"], cast(dl)))                   # the loss without its start value
        rejected(lambda: mv.check_vce("mut", c, c["start"] + scale * (loss - c["start"]), cast(dl)))   # scale applied twice
        rejected(lambda: mv.check_vce("mut", c, loss, cast(dl * scale)))
        if bf16:                                                     # a bf16 store that truncates
            d32 = dl.float()
            rejected(lambda: mv.check_vce("mut", c, loss, (d32.view(torch.int32) & -65536).view(torch.float32).to(torch.bfloat16)))
    # a read of the padding: the pad value enters max and sum
    c = mv.vce_reference(mv.vce_case(V, ldv, 3, (0.0, "fixed", 0.0), seed=5), False)
    c2 = dict(c, V=ldv)
    c2["labels"] = c["labels"]
    loss2, dl2 = mv.emulate_vce(c2, torch.float32)
    rejected(lambda: mv.check_vce("mut", c, loss2, dl2))


def test_gelu_mutations_are_rejected():
    for dt in (torch.float32, torch.bfloat16):
        d, z = mv.gelu_case(4096, dt, seed=2)
        d64, z64 = d.to(F64), z.to(F64)
        cast = lambda t: t.to(dt)
        ref = mv.gelu_bwd(d, z)
        mv.check_gelu("reference", cast(ref), d, z)
        rejected(lambda: mv.check_gelu("mut", cast(d64 * mv.gelu(z64)), d, z))                  # gelu in place of gelu'
        t = 0.7978845608028654 * (z64 + 0.044715 * z64 ** 3)                                     # the tanh form's derivative
        dt_form = 0.5 * (1 + torch.tanh(t)) + 0.5 * z64 * (1 - torch.tanh(t) ** 2) * 0.7978845608028654 * (1 + 3 * 0.044715 * z64 ** 2)
        rejected(lambda: mv.check_gelu("mut", cast(d64 * dt_form), d, z))
        rejected(lambda: mv.check_gelu("mut", cast(torch.nan_to_num(ref)), d, z))                # the limit instead of inf * 0
        wrong = ref.clone()
        wrong[-3] = d64[-3]                                                                      # an element of the tail left as it was (z = -10)
        rejected(lambda: mv.check_gelu("mut", cast(wrong), d, z))


def test_sum_steps_mutations_are_rejected():
    for dt in (torch.float32, torch.bfloat16):
        src = mv.sum_case(1028, 5, dt, seed=3)
        ref = mv.sum_steps(src)
        cast = lambda t: t.to(dt)
        mv.check_sum("reference", cast(ref), src)
        rejected(lambda: mv.check_sum("mut", cast(ref - src[4].to(F64)), src))                   # one step dropped
        rejected(lambda: mv.check_sum("mut", cast(ref - src[0].to(F64)), src))
        rejected(lambda: mv.check_sum("mut", cast(ref + src[2].to(F64)), src))                   # a step counted twice
        wrong = cast(ref)
        wrong[-4:] = mv.payload((4,), dt)                                                        # the last float4 missing
        rejected(lambda: mv.check_sum("mut", wrong, src))
        one = mv.sum_case(1028, 1, dt, seed=4)
        wrong = one[0].clone()
        wrong[7] = wrong[7] * (1 + 2.0 ** -7)
        rejected(lambda: mv.check_sum("mut", wrong, one))                                        # steps = 1 is not a copy


def test_exact_kernel_mutations_are_rejected():
    src = mv.random_bytes(48, seed=1)
    want = mv.repeat_block(src, 3)
    mv.exact("reference", want, src.repeat(3))
    wrong = torch.cat([mv.payload((48,), torch.uint8), want[:96]])                               # block t written at t + 1
    rejected(lambda: mv.exact("mut", wrong, want))
    for n in (5, 1026, 1027):                                                                    # a tail of 1 .. 3 elements untouched
        x = mv.random_f32(n, seed=n)
        for name, want in (("copy", x), ("zero", torch.zeros(n))):
            wrong = want.clone()
            wrong[n - n % 4:] = mv.payload((n % 4,), torch.float32)
            rejected(lambda: mv.exact("mut " + name, wrong, want))
    x = mv.random_f32(1028, seed=7)
    for dt in (torch.float32, torch.bfloat16):
        good = x.clone() if dt == torch.float32 else mv.bf16_rne(x)
        mv.check_cast_to("reference", good, x)
        wrong = good.clone()
        wrong[-3:] = mv.payload((3,), dt)
        rejected(lambda: mv.check_cast_to("mut", wrong, x))
    trunc = (x.view(torch.int32) & -65536).view(torch.float32).to(torch.bfloat16)
    rejected(lambda: mv.check_cast_to("mut", trunc, x))
    assert int(mv.EXACT["mut"]) > 0
    for i, (B, V) in enumerate(mv.SEQ_SHAPES):
        lens = mv.seq_lens(B, V, seed=i)
        wrong = (torch.arange(V)[None, :] <= lens[:, None]).to(torch.uint8)                      # `<=` for `<`
        if bool((lens < V).any()):
            rejected(lambda: mv.exact("mut seq_mask", wrong, mv.seq_mask(lens, V)))
    assert bool((mv.seq_lens(1, 1, 0) < 1).any())


def test_vp_gather_mutations_are_rejected():
    hit = {"masked": 0, "offset": 0}
    for i, case in enumerate(mv.vp_cases()):
        c = mv.vp_case(case, seed=i)
        want = mv.vp_gather(c["cand"], c["cand_ptr"], c["pano"], c["mask"], c["V"])
        mv.check_vp("reference", *want, want)
        B, P, ks = c["B"], c["P"], case[3]
        # non-candidate views taken in masked order: the views whose mask byte is SET follow the candidates
        if case[4] == "some" and all(k + int(c["mask"][b].sum()) <= c["V"] for b, k in enumerate(ks)):
            wrong = mv.vp_gather(c["cand"], c["cand_ptr"], c["pano"], 1 - c["mask"], c["V"])
            rejected(lambda: mv.check_vp("mut", wrong[0], None, None, want))
            rejected(lambda: mv.check_vp("mut", *wrong, want))
            hit["masked"] += 1
        # candidate offset off by one episode: episode b reads the rows of episode b + 1
        if B == 3 and ks[0] > 0 and ks[1] > 0:
            ptr = c["cand_ptr"].clone()
            wrong = want[0].clone()
            wrong[0, :ks[0]] = c["cand"][int(ptr[1]):int(ptr[1]) + ks[0]] if int(ptr[1]) + ks[0] <= int(ptr[-1]) else 0
            rejected(lambda: mv.check_vp("mut", wrong, None, None, want))
            hit["offset"] += 1
    assert hit["masked"] >= 3 and hit["offset"] >= 1, hit
