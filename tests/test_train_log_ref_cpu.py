"""The restatements of tests/trainlog_ref.py without a GPU: the meter equals the recording of the REAL RunningMeter
(tests/golden/train_log_small.npz, tools/make_golden_train_log.py) bit for bit, the fp32 root rule equals numpy's float32 sqrt, the
emulation of the report's kernels stays inside the bounds the GPU test uses, and every planted mutation is rejected by the very
comparison the GPU test makes."""
import math
import os

import numpy as np
import pytest

from tests import trainlog_ref as tr

Z = np.load(tr.GOLDEN)


def replay(mutate=None):
    """the recorded calls through two restated meters -> per call (run, has, reported) of the meter that took it"""
    meters = [tr.Meter(float(Z["meter/smooth"]), mutate), tr.Meter(float(Z["meter/smooth"]), mutate)]
    out = []
    for t, v in zip(Z["meter/task"], Z["meter/loss"]):
        m = meters[int(t)]
        m(v, n_examples=3, n_in_units=17, n_loss_units=5)
        out.append((m.run if m.n_values else 0.0, int(m.n_values > 0), float(m.val)))
    return out, meters


def matches_recording(rows):
    return all(tr.bits64(r[0]) == tr.bits64(v) and r[1] == int(h) and tr.bits64(r[2]) == tr.bits64(p)
               for r, v, h, p in zip(rows, Z["meter/val"], Z["meter/has"], Z["meter/reported"]))


def test_the_fixture_holds_the_cases_the_meter_can_go_wrong_on():
    loss, task = Z["meter/loss"], Z["meter/task"]
    assert 40 <= len(loss) <= 48 and set(task.tolist()) == {0, 1} and loss.dtype == np.float32
    first1 = int(np.argmax(task == 1))
    assert np.isnan(loss[first1]) and Z["meter/has"][first1] == 0 and Z["meter/reported"][first1] == 0       # a NaN as the first value
    t0 = [i for i in range(len(loss)) if task[i] == 0]
    pairs = [(a, b) for a, b in zip(t0, t0[1:]) if loss[a] == np.inf and loss[b] == -np.inf]
    assert pairs and Z["meter/val"][pairs[0][1]] == np.inf                                                      # inf - inf skipped
    assert np.isnan(loss).sum() == 2 and len(set(loss.tolist())) < len(loss) - 1                              # exact repeats
    assert float(Z["meter/smooth"]) == 0.99


def test_meter_restatement_equals_the_real_running_meter_bit_for_bit():
    rows, meters = replay()
    assert matches_recording(rows)
    n = [int((Z["meter/task"] == t).sum()) for t in (0, 1)]
    for m, k in zip(meters, n):                 # the counters advance on every call, skipped or not; values + skips = calls
        assert m.n_values + m.n_skipped == k and m.record()[4:7] == (3 * k, 17 * k, 5 * k)
    assert sum(m.n_skipped for m in meters) == 3


@pytest.mark.parametrize("mutate", ["smooth_fp32", "fma", "nan_test_on_input", "first_against_zero", "skip_advances"])
def test_planted_meter_mutations_are_rejected(mutate):
    rows, _ = replay(mutate)
    assert not matches_recording(rows), mutate


@pytest.mark.skipif(not os.path.isdir(os.path.join(os.environ.get("ETP_REFERENCE", "/root/reference"), "pretrain_src")),
                    reason="the reference tree is not present")
def test_the_fixture_is_what_the_real_class_gives_today():
    import sys
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools"))
    import make_golden_train_log as mg
    RunningMeter = mg.running_meter()
    meters = [RunningMeter("a"), RunningMeter("b")]
    for i, (t, v) in enumerate(zip(Z["meter/task"], Z["meter/loss"])):
        m = meters[int(t)]
        m(float(v))
        assert tr.bits64(m.val) == tr.bits64(Z["meter/reported"][i]), i


def root_values():
    rng = np.random.RandomState(3)
    x = np.exp(rng.uniform(math.log(1e-45), math.log(3.4e38), 100000)).astype(np.float32)
    edge = np.array(tr.SUMSQ_CASES + [1e-45, 1.1754944e-38, 3.4028235e38, 4.0, 16777216.0, 16777218.0, -1.0, -0.0], dtype=np.float32)
    return np.concatenate([x, edge, np.nextafter(edge, np.float32(0))])


def test_fp32_root_rule_equals_numpys_float32_sqrt():
    x = root_values()
    with np.errstate(invalid="ignore"):
        want = np.sqrt(x)                                   # float32 in, float32 out: IEEE correctly rounded
        got = np.sqrt(x.astype(np.float64)).astype(np.float32)
    assert want.dtype == np.float32 and len(x) > 100000
    assert np.array_equal(got.view(np.int32), want.view(np.int32))
    for v in tr.SUMSQ_CASES + [1e-45, 3.0]:
        a, b = tr.f32_root(v), float(np.sqrt(np.float32(v)))
        assert (math.isnan(a) and math.isnan(b)) or a == b, v


def test_step_record_restatement_and_the_norm_without_its_root():
    rec, bad = tr.STEP_START, tr.STEP_START
    seen = []
    for i, (s, nf) in enumerate([(4.0, 0), (9.0, None), (float("inf"), 0), (16.0, 5), (float("nan"), None), (1.0, 0)]):
        rec = tr.step_record(rec, s, nf)
        bad = tr.step_record(bad, s, nf, mutate="no_root")
        seen.append(rec)
    assert seen[1][:6] == (3.0, 3.0, 5.0, 2, 0, -1)
    assert rec[1:6] == (3.0, 6.0, 6, 3, 3) and rec[0] == 1.0           # inf, the counted step and NaN are left out of max / sum
    assert bad[1:3] != rec[1:3]
    # the recorded clip_grad_norm_ results: the fp32 root of the float64 sum of squares, rounded to fp32 first, against torch's fp32
    # norm of norms -- both within gam32(n + tensors + 2) of the exact norm (sequential fp32 accumulation at worst), u = 2^-24
    for s in range(3):
        g = [Z[k] for k in sorted(Z.files) if k.startswith(f"grads/{s}/") and k.split("/")[-1].isdigit()]
        n = sum(x.size for x in g)
        sumsq = np.float32(math.fsum(float(v) ** 2 for x in g for v in x.reshape(-1).tolist()))
        k = n + len(g) + 2
        bound = 2 * (k * 2.0 ** -24 / (1 - k * 2.0 ** -24)) * float(Z[f"grads/{s}/norm"])
        assert abs(tr.f32_root(sumsq) - float(Z[f"grads/{s}/norm"])) <= bound
        assert abs(tr.f32_root(sumsq, "no_root") - float(Z[f"grads/{s}/norm"])) > bound


# ---- the report ------------------------------------------------------------------------------------------------------------------------
_CASE = {}


def case(t):
    if t not in _CASE:
        arena, off, lens, include = tr.report_case(t)
        _CASE[t] = (arena, off, lens, include, tr.report_ref(arena, off, lens))
    return _CASE[t]


def test_the_tables_cover_the_issues_list():
    tables = tr.report_tables()
    assert [len(t[0]) for t in tables] == tr.N_SEGS
    assert {n for _, lens, _ in tables for n in lens} == set(tr.LENS)
    for off, lens, include in tables:
        assert all(o % 4 == 0 for o in off) and all(a + n < b for a, n, b in zip(off, lens, off[1:])) and len(include) == len(off)
    assert any(0 in inc for _, _, inc in tables)
    assert tr.depth(1) == 1 + 6 + 3 + 1 + 6 and tr.depth(16384) == 64 + 16 and tr.depth(16383) == 65 + 16
    assert tr.depth(2 ** 20 + 64) == 64 + 6 + 3 + 2 + 6 and tr.seg_chunks(2 ** 20 + 64) == 65 and tr.seg_chunks(16385) == 2


@pytest.mark.parametrize("t", range(len(tr.N_SEGS)))
def test_emulated_kernels_stay_inside_the_bounds_and_the_gaps_would_show(t):
    arena, off, lens, include, ref = case(t)
    tr.assert_gaps_would_show(arena, off, lens, ref)
    got = tr.emulate(arena, off, lens)
    assert tr.check_report("emulation", got, ref, lens) <= 1.0
    n_seg = len(off)
    if n_seg > 5:
        assert ref[1][:4] == (0.0, 0.0, 0.0, 0)                                      # the all-zero segment
        assert abs(ref[2][0]) < 2.0 ** -9 * ref[2][4]                                  # the cancelling one
        assert [ref[s][3] for s in (3, 4, 5)] == [1, 1, 1] and lens[5] % 4
    tot, nf = tr.totals_ref([g[1] for g in got], [g[3] for g in got], include)
    assert nf == sum(r[3] for r, inc in zip(ref, include) if inc)
    if nf == 0:
        want = math.fsum(r[1] for r, inc in zip(ref, include) if inc)
        assert abs(tot - want) <= (2.0 ** -24 + tr.gam64(max(map(tr.depth, lens)) + tr.depth_total(n_seg))) * want
    else:
        assert math.isnan(tot)


@pytest.mark.parametrize("mutate", ["chunk_crosses", "tail_dropped", "nonfinite_in_sum", "absmax_signed"])
def test_planted_report_mutations_are_rejected(mutate):
    arena, off, lens, include, ref = case(2)
    with pytest.raises(AssertionError):
        tr.check_report(mutate, tr.emulate(arena, off, lens, mutate), ref, lens)


def test_ignoring_the_include_bytes_is_rejected():
    arena, off, lens, include, ref = case(1)              # two finite segments, the long one excluded
    got = tr.emulate(arena, off, lens)
    assert tr.totals_ref([g[1] for g in got], [g[3] for g in got], include) != \
        tr.totals_ref([g[1] for g in got], [g[3] for g in got], include, mutate="include_ignored")
