"""tests/eval_ref.py without a GPU.

PIN: the float64 restatement of the validation tails equals the statements it restates -- F.cross_entropy(reduction='sum'),
scores.max(dim=-1)[1] and torch.argmax on the CPU (train_r2r.py:365-367, :424-427), ties, -inf labels and all -inf rows included -- and
reproduces tests/golden/pretrain_validate_small.npz, recorded from the real pre-training model.
REACH: the case lists hold what they claim: every tie pair with every label placement, both special rows, every ignore pattern.
PASS: the emulations of the three kernels' schedules (fp32 pair combine, vocab_ce's / sap_ce's sum order, double accumulation) stay
inside the bounds on every case the GPU file runs.
FAIL: the planted defects are rejected by the comparators the GPU file calls.
"""
import os
import tempfile

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from tests import eval_ref as ev

F64 = torch.float64


def rejected(fn):
    with pytest.raises(AssertionError):
        fn()


# ---- pins ------------------------------------------------------------------------------------------------------------------------
def test_tail_restatement_is_torch_cross_entropy_sum_and_argmax():
    for i, (V, ldv, Nm, shift, special) in enumerate(ev.vocab_cases()):
        if V == 30522 and Nm == 5 or (i % 5 and special is None):
            continue
        c = ev.vocab_case(V, ldv, Nm, shift, special, i)
        s, q = c["buf"][:, :V].to(F64), c["q"]
        want = F.cross_entropy(s, c["labels"], reduction="sum")
        got = q["nll"].sum()
        assert (torch.isnan(want) and torch.isnan(got)) or want == got or abs(float(want - got)) <= 1e-12 * abs(float(want)), (i, want, got)
        assert torch.equal(s.max(dim=-1)[1], q["pred"]) and torch.equal(torch.argmax(s, 1), q["pred"]), i
        assert torch.equal(c["buf"][:, :V].max(dim=-1)[1], q["pred"]), i                 # fp32 as the reference holds the scores
    for i, (B, G, pat, special) in enumerate(ev.sap_cases()):
        c = ev.sap_case(B, G, pat, special, i)
        s, q = c["logits"].to(F64), c["q"]
        want = F.cross_entropy(s, c["labels"], reduction="sum", ignore_index=c["ignore_index"])
        got = q["nll"].sum()
        assert (torch.isnan(want) and torch.isnan(got)) or want == got or abs(float(want - got)) <= 1e-12 * abs(float(want)), (i, want, got)
        assert torch.equal(torch.argmax(s, 1), q["pred"]) and torch.equal(torch.argmax(c["logits"], 1), q["pred"]), i


def test_special_rows_are_torchs():
    neg = float("-inf")
    s = torch.tensor([[1.0, 3.0, 3.0, neg], [neg, neg, neg, neg], [0.5, neg, 0.25, 0.5]])
    y = torch.tensor([1, 2, 1])
    q = ev.tail(s, y)
    assert q["pred"].tolist() == [1, 0, 0] == torch.argmax(s, 1).tolist() == s.max(dim=-1)[1].tolist()
    per_row = F.cross_entropy(s, y, reduction="none")
    assert torch.isnan(per_row[1]) and torch.isnan(q["nll"][1])                          # a row of only -inf
    assert torch.isposinf(per_row[2]) and torch.isposinf(q["nll"][2])                    # a label on a -inf logit
    assert abs(float(per_row[0]) - float(q["nll"][0])) < 1e-6


def test_restatement_reproduces_the_real_models_validation():
    z = np.load(ev.GOLDEN)
    for task, rows, keys in (("mlm", "n_word", ("loss", "acc")), ("sap", "n_data", ("gloss", "gacc"))):
        rec = (0.0, 0, 0, 0)
        for i in range(2):
            s = torch.from_numpy(z[f"{task}/scores/{i}" if task == "mlm" else f"{task}/logits/{i}"])
            y = torch.from_numpy(z[f"{task}/labels/{i}"])
            q = ev.tail(s, y, None if task == "mlm" else -100)
            new = ev.accumulate(rec, q["nll"], q["pred"], y, -100)
            assert abs(new[0] - rec[0] - float(z[f"{task}/loss_sum/{i}"])) <= 1e-5 * float(z[f"{task}/loss_sum/{i}"])   # the fixture's sum is fp32
            assert new[1] - rec[1] == int(z[f"{task}/n_correct/{i}"]) and new[2] - rec[2] == int(z[f"{task}/{rows}/{i}"])
            rec = new
        m = ev.metrics(rec, keys)
        assert abs(m[keys[0]] - float(z[f"{task}/{keys[0]}"])) <= 1e-5 * float(z[f"{task}/{keys[0]}"])
        assert m[keys[1]] == float(z[f"{task}/{keys[1]}"]) and 0 < m[keys[1]] < 1


def test_fixture_margins_allow_exact_counts():
    """a 3e-4 error of the scores (the step tolerance of tests/test_planner_gpu.py) cannot move an arg-max: no row is left out"""
    z = np.load(ev.GOLDEN)
    mlm = min(ev.top2_margin(z[f"mlm/scores/{i}"]) for i in range(2))
    sap = min(ev.top2_margin(np.where(np.isfinite(z[f"sap/logits/{i}"]), z[f"sap/logits/{i}"], -1e30)) for i in range(2))
    assert abs(ev.top2_margin(z["mlm/scores/0"]) - 0.0227) < 1e-4 and z["mlm/scores/0"].shape[0] == 13
    assert abs(ev.top2_margin(np.where(np.isfinite(z["sap/logits/0"]), z["sap/logits/0"], -1e30)) - 0.0027) < 1e-4
    assert mlm > 2 * 3e-4 and sap > 2 * 3e-4
    _, _, loaders = ev.val_loaders(z)
    for i in range(2):
        assert int((loaders["mlm"][i]["txt_labels"] != -1).sum()) == z[f"mlm/labels/{i}"].size
        assert loaders["mlm"][i]["txt_ids"] is loaders["sap"][i]["txt_ids"]              # copies of the same batch


# ---- reach -----------------------------------------------------------------------------------------------------------------------
def test_cases_reach_what_they_claim():
    seen, special = set(), set()
    shapes = set()
    for i, (V, ldv, Nm, shift, sp) in enumerate(ev.vocab_cases()):
        shapes.add((V, ldv, Nm))
        if V == 30522:
            assert Nm in (1, 5)
            continue                                                     # built by the emulation test below; same planting code
        c = ev.vocab_case(V, ldv, Nm, shift, sp, i)
        assert bool((c["buf"][:, V:] == 3e38).all())
        for r, a, b, place in c["planted"]:
            row = c["buf"][r, :V]
            if sp is None:
                assert row[a] == row[b] == row.max() and int(c["q"]["pred"][r]) == a
                y = int(c["labels"][r])
                assert {"winner": y == a, "loser": y == b, "elsewhere": y not in (a, b) or V < 3}[place]
                kind = "trips" if b - a == 256 else "waves" if (a, b) == (63, 64) else "lanes" if (a, b) == (5, 6) else "ends"
                seen.add((kind, place))
        if V > 3 and sp is None:
            assert bool(torch.isneginf(c["buf"][:, :V]).any(1).all()), i
        if sp:
            special.add(sp)
            r = Nm // 2
            assert torch.isposinf(c["q"]["nll"][r]) if sp == "label_neginf" else (torch.isnan(c["q"]["nll"][r]) and int(c["q"]["pred"][r]) == 0)
    assert seen == {(k, p) for k in ("trips", "waves", "lanes", "ends") for p in ev.PLACES}, sorted(seen)
    assert special == {"label_neginf", "all_neginf"}
    from tests import move_ref as mv
    assert shapes >= {(V, ldv, Nm) for _, V, ldv, Nm, _ in mv.vce_cases()}
    ign = set()
    for i, (B, G, pat, sp) in enumerate(ev.sap_cases()):
        c = ev.sap_case(B, G, pat, sp, i)
        k = c["q"]["keep"]
        ign.add("all" if not k.any() else "none" if k.all() else "some")
        if sp == "all_neginf":
            assert torch.isnan(c["q"]["nll"][B // 2]) and int(c["q"]["pred"][B // 2]) == 0
        if sp == "label_neginf":
            assert torch.isposinf(c["q"]["nll"][B // 2])
        for r, a, b, place in c["planted"]:
            if sp is None:
                assert int(c["q"]["pred"][r]) == a
    assert ign == {"all", "none", "some"}
    assert {(B, G) for B, G, _, _ in ev.sap_cases()} == {(b, g) for b in (1, 7, 16, 17, 33, 100) for g in (1, 2, 63, 64, 65, 130, 1000)}
    assert [n for n, _ in ev.accum_cases()][::2] == [1, 255, 256, 257, 1029]


# ---- pass: the kernels' schedules, emulated ----------------------------------------------------------------------------------------
def test_emulated_vocab_eval_is_inside_the_bounds_on_every_gpu_case():
    for i, (V, ldv, Nm, shift, sp) in enumerate(ev.vocab_cases()):
        c = ev.vocab_case(V, ldv, Nm, shift, sp, i)
        nll, pred = ev.emulate_vocab_eval(c["buf"], c["labels"], V)
        ev.check_rows(f"emulated vocab_eval {i}", nll, pred, c["q"], ev.vocab_depth(V))
        rec = ev.emulate_accum(ev.START, nll, pred, c["labels"], -1)
        ev.check_record(f"emulated vocab_eval {i} record", rec, ev.START, nll, pred, c["labels"], -1)


def test_emulated_sap_eval_is_inside_the_bounds_on_every_gpu_case():
    for i, (B, G, pat, sp) in enumerate(ev.sap_cases()):
        c = ev.sap_case(B, G, pat, sp, i)
        nll, pred = ev.emulate_sap_eval(c["logits"], c["labels"], c["ignore_index"])
        ev.check_rows(f"emulated sap_eval {i}", nll, pred, c["q"], ev.sap_depth(G))
        rec = ev.emulate_accum((0.0, 0, 0, 0), nll, pred, c["labels"], c["ignore_index"])
        ev.check_record(f"emulated sap_eval {i} record", rec, (0.0, 0, 0, 0), nll, pred, c["labels"], c["ignore_index"])


def test_emulated_accumulation_is_inside_the_bound_and_repeats():
    for i, (n, ii) in enumerate(ev.accum_cases()):
        rec = ev.START
        for nll, pred, labels in ev.accum_case(n, ii, 3000 + i):
            new = ev.emulate_accum(rec, nll, pred, labels, ii)
            assert new == ev.emulate_accum(rec, nll, pred, labels, ii)
            ev.check_record(f"emulated accum {n}/{ii}", new, rec, nll, pred, labels, ii)
            rec = new
        assert rec[2] == ev.START[2] + 2 * n
        assert ev.unpack_record(ev.pack_record(rec)) == rec


# ---- fail: planted defects ---------------------------------------------------------------------------------------------------------
def _vocab(i):
    V, ldv, Nm, shift, sp = ev.vocab_cases()[i]
    return ev.vocab_case(V, ldv, Nm, shift, sp, i)


def _first(pred):
    return next(i for i, c in enumerate(ev.vocab_cases()) if pred(*c))


def test_planted_defects_are_rejected():
    assert set(ev.MUTATIONS) == {"tie_high", "argmax_ldv", "mean_for_sum", "ignored_in_loss", "ignored_not_in_rows", "correct_on_ignored",
                                 "overwrite", "labels_shifted"}
    i = _first(lambda V, ldv, Nm, sh, sp: V == 257 and Nm == 77)
    c = _vocab(i)
    for m in ("tie_high", "argmax_ldv", "labels_shifted"):
        nll, pred = ev.emulate_vocab_eval(c["buf"], c["labels"], c["V"], mutate=m)
        rejected(lambda: ev.check_rows(m, nll, pred, c["q"], ev.vocab_depth(c["V"])))
    j = next(k for k, (B, G, pat, sp) in enumerate(ev.sap_cases()) if B == 100 and G == 130 and sp is None and pat[1] == "some")
    B, G, pat, sp = ev.sap_cases()[j]
    s = ev.sap_case(B, G, pat, sp, j)
    for m in ("tie_high", "labels_shifted"):
        nll, pred = ev.emulate_sap_eval(s["logits"], s["labels"], s["ignore_index"], mutate=m)
        rejected(lambda: ev.check_rows(m, nll, pred, s["q"], ev.sap_depth(G)))
    n, ii = 257, 2
    (nll, pred, labels), _ = ev.accum_case(n, ii, 3000)
    for m in ("mean_for_sum", "ignored_in_loss", "ignored_not_in_rows", "correct_on_ignored", "overwrite"):
        rec = ev.emulate_accum(ev.START, nll, pred, labels, ii, mutate=m)
        rejected(lambda: ev.check_record(m, rec, ev.START, nll, pred, labels, ii))
    ev.check_record("sound", ev.emulate_accum(ev.START, nll, pred, labels, ii), ev.START, nll, pred, labels, ii)
    # an ignored row that is not written as 0
    nll, pred = ev.emulate_sap_eval(s["logits"], s["labels"], s["ignore_index"])
    nll[(~s["q"]["keep"]).nonzero()[0]] = 1e-30
    rejected(lambda: ev.check_rows("ignored row", nll, pred, s["q"], ev.sap_depth(G)))


# ---- sum over the ranks --------------------------------------------------------------------------------------------------------------
def _rank_main(rank, path, out):
    import torch.distributed as dist
    from etpnav_amd.validate import sum_over_ranks
    dist.init_process_group("gloo", init_method=f"file://{path}", rank=rank, world_size=2)
    try:
        got = sum_over_ranks((1.5 + rank, 3 + rank, 2 ** 40 + 7 * rank))
        with open(f"{out}.{rank}", "w") as f:
            f.write(repr(got))
    finally:
        dist.destroy_process_group()


def test_sum_over_ranks_is_one_all_reduce_in_a_world_of_two_and_the_identity_alone():
    import torch.multiprocessing as mp
    from etpnav_amd.validate import sum_over_ranks
    assert sum_over_ranks((1.5, 3, 7)) == (1.5, 3, 7)
    with tempfile.TemporaryDirectory() as td:
        path, out = os.path.join(td, "store"), os.path.join(td, "out")
        ctx = mp.get_context("spawn")
        procs = [ctx.Process(target=_rank_main, args=(r, path, out)) for r in range(2)]
        for p in procs:
            p.start()
        for p in procs:
            p.join(120)
            assert p.exitcode == 0
        for r in range(2):
            assert eval(open(f"{out}.{r}").read()) == (4.0, 7.0, float(2 ** 41 + 7))
