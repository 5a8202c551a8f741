"""etp_mlm_select (csrc/traj_batch.hip) on the MI355X against tests/mlm_select_ref.py, which tests/test_mlm_select_ref_cpu.py pins to the
host build of MlmStep.  n covers the wave (63 / 64 / 65), the workgroup chunk (255 / 256 / 257) and several chunks (1000, 8195); the
patterns are the crafted rows of the CPU file plus 15 % random with the labels 0 and vocab - 1 present.  All outputs sit in guarded
buffers, with sentinels behind `cap` and behind ptr_t[n].  Flagged launches are judged by their arrays alone: nothing downstream of them
is ever launched."""
import numpy as np
import pytest
import torch

from etpnav_amd import _lib
from tests import mlm_select_ref as ms

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
GUARD = 64
SIZES = (1, 63, 64, 65, 255, 256, 257, 1000, 8195)
I32_SENT, I64_SENT = -0x5A5A5A5B, -0x5A5A5A5A5A5A5A5B


class Out:
    """rows [cap], labels [cap], ptr_t [n + 1], status [2], each between GUARD sentinels; the outputs themselves start as 0xFF bytes"""

    def __init__(self, n, cap):
        self.n, self.cap = n, cap
        mk = lambda m, dt, sent: torch.full((m + 2 * GUARD,), sent, dtype=dt, device=DEV)
        self.bufs = {"rows": mk(cap, torch.int32, I32_SENT), "labels": mk(cap, torch.int64, I64_SENT),
                     "ptr_t": mk(n + 1, torch.int32, I32_SENT), "status": mk(2, torch.int32, I32_SENT)}
        self.len = {"rows": cap, "labels": cap, "ptr_t": n + 1, "status": 2}
        for k in self.bufs:
            self.view(k).fill_(-1)
        self.before = {k: v.clone() for k, v in self.bufs.items()}

    def view(self, k):
        return self.bufs[k][GUARD:GUARD + self.len[k]]

    def ptr(self, k):
        return self.view(k).data_ptr()

    def guards_intact(self, what, written):
        """nothing outside the outputs changed, and of rows / labels nothing at or behind `written`"""
        for k, b in self.bufs.items():
            keep = torch.ones_like(b, dtype=torch.bool)
            hi = written if k in ("rows", "labels") else self.len[k]
            keep[GUARD:GUARD + hi] = False
            assert torch.equal(b[keep], self.before[k][keep]), f"{what}: {k} was written outside [0, {hi})"

    def untouched(self, what):
        for k, b in self.bufs.items():
            assert torch.equal(b, self.before[k]), f"{what}: {k} was written by a refused call"


def launch(lab_dev, n, vocab, n_expected, cap, out, **ptrs):
    p = {k: out.ptr(k) for k in ("rows", "ptr_t", "labels", "status")}
    p.update(ptrs)
    rc = _lib.lib().etp_mlm_select(lab_dev.data_ptr() if lab_dev is not None else None, n, vocab, n_expected, cap, p["rows"], p["ptr_t"],
                                   p["labels"], p["status"], torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    return rc


def run(lab, vocab, n_expected, cap):
    n = lab.size
    out = Out(n, cap)
    dev = torch.from_numpy(lab).to(DEV)
    assert launch(dev, n, vocab, n_expected, cap, out) == 0, _lib.lib().etp_last_error()
    return out, {k: out.view(k).cpu().numpy() for k in out.bufs}


@pytest.fixture(scope="module")
def refs():
    return {(p, n): ms.select(ms.pattern(p, n)) for p in ms.PATTERNS for n in SIZES}


@pytest.mark.parametrize("n", SIZES)
def test_bit_equal_to_the_restatement(n, refs):
    for p in ms.PATTERNS:
        lab = ms.pattern(p, n)
        rows, ptr_t, labels, count = refs[(p, n)]
        if p == "random15" and count >= 2:
            assert 0 in labels and ms.VOCAB - 1 in labels
        what = f"{p}, n = {n}, Nm = {count}"
        runs = []
        for cap in (count, count + 5):
            out, got = run(lab, ms.VOCAB, count, cap)
            assert got["status"].tolist() == [0, count], (what, got["status"])
            assert np.array_equal(got["rows"][:count], rows) and np.array_equal(got["labels"][:count], labels), what
            assert np.array_equal(got["ptr_t"], ptr_t), what
            assert ms.safe(got["rows"], got["ptr_t"], got["labels"], n, ms.VOCAB, count) is None
            out.guards_intact(what, count)
            runs.append(got)
        out2, again = run(lab, ms.VOCAB, count, count + 5)                       # a second run: the same bits
        for k in again:
            assert np.array_equal(again[k], runs[1][k]), (what, k)


@pytest.mark.parametrize("n", (65, 257, 1000))
@pytest.mark.parametrize("case", ["count_above", "count_below", "label_minus_2", "label_vocab"])
def test_flagged_launches_stay_in_range(n, case):
    """the arrays of a flagged launch are inspected, never used"""
    vocab = 1000
    lab = ms.pattern("random15", n, vocab=vocab, seed=3)
    true = int((lab != -1).sum())
    n_expected, want = true, ms.ERR_LABEL
    if case == "count_above":                   # more masked entries than the step was sized for
        n_expected, want = max(0, true - 3), ms.ERR_COUNT
    elif case == "count_below":
        n_expected, want = true + 4, ms.ERR_COUNT
    elif case == "label_minus_2":
        lab[np.nonzero(lab != -1)[0][-1]] = -2
    else:
        lab[np.nonzero(lab != -1)[0][0]] = vocab
    cap = n_expected + 2
    out, got = run(lab, vocab, n_expected, cap)
    assert ms.flags(lab, vocab, n_expected) == want
    assert got["status"].tolist() == [want, true], (case, got["status"])
    assert ms.safe(got["rows"], got["ptr_t"], got["labels"], n, vocab, n_expected) is None, case
    out.guards_intact(case, n_expected)
    # what lies below min(true, n_expected) is still the selection (labels clamped)
    rows, _, labels, _ = ms.select(lab)
    m = min(true, n_expected)
    assert np.array_equal(got["rows"][:m], rows[:m]) and np.array_equal(got["labels"][:m], np.clip(labels[:m], 0, vocab - 1))


def test_both_flags_at_once_and_the_largest_n():
    n, vocab = 1 << 20, 77
    lab = np.full(n, -1, np.int32)
    lab[[0, 4097, n - 1]] = (5, 76, 0)
    out, got = run(lab, vocab, 3, 3)
    assert got["status"].tolist() == [0, 3] and got["rows"].tolist() == [0, 4097, n - 1] and got["labels"].tolist() == [5, 76, 0]
    assert got["ptr_t"][0] == 0 and got["ptr_t"][1] == 1 and got["ptr_t"][4098] == 2 and got["ptr_t"][n - 1] == 2 and got["ptr_t"][n] == 3
    out.guards_intact("n = 2^20", 3)
    lab[7] = -(1 << 31)
    out, got = run(lab, vocab, 3, 3)
    assert got["status"].tolist() == [ms.ERR_COUNT | ms.ERR_LABEL, 4]
    assert ms.safe(got["rows"], got["ptr_t"], got["labels"], n, vocab, 3) is None
    out.guards_intact("n = 2^20, flagged", 3)


def test_refusals_leave_the_fill_intact():
    lab = torch.from_numpy(ms.pattern("every7", 100)).to(DEV)
    n, count = 100, 15
    out = Out(n, count)
    cases = {"n 0": dict(n=0), "n beyond 2^20": dict(n=(1 << 20) + 1), "vocab 0": dict(vocab=0), "n_expected -1": dict(n_expected=-1),
             "n_expected above cap": dict(n_expected=count + 1), "NULL rows": dict(rows=None), "NULL ptr_t": dict(ptr_t=None),
             "NULL labels": dict(labels=None), "NULL status": dict(status=None), "misaligned rows": dict(rows=out.ptr("rows") + 2),
             "misaligned ptr_t": dict(ptr_t=out.ptr("ptr_t") + 1), "misaligned labels": dict(labels=out.ptr("labels") + 4),
             "misaligned status": dict(status=out.ptr("status") + 2)}
    for name, kw in cases.items():
        a = dict(n=n, vocab=ms.VOCAB, n_expected=count, cap=count)
        a.update({k: kw.pop(k) for k in list(kw) if k in a})
        assert launch(lab, a["n"], a["vocab"], a["n_expected"], a["cap"], out, **kw) == -1, name
        out.untouched(name)
    assert launch(None, n, ms.VOCAB, count, count, out) == -1
    out.untouched("NULL txt_labels")
    assert launch(lab, n, ms.VOCAB, count, count, out) == 0                    # and the same operands, accepted, write
    assert out.view("status").tolist() == [0, count]
