"""tests/mlm_select_ref.py (the numpy restatement of etp_mlm_select) pinned bit for bit to the host build it replaces: the nonzero /
cumsum statements of MlmStep's host route, run on CPU tensors.  Crafted rows, the recorded txt_labels of
tests/golden/pretrain_batch_small.npz, five planted mutations (each rejected wherever it can show), and the memory-safety predicate."""
import os

import numpy as np
import pytest
import torch

from tests import mlm_select_ref as ms

GOLDEN = os.path.join(os.path.dirname(__file__), "golden", "pretrain_batch_small.npz")


def host_build(txt_labels: torch.Tensor):
    """the statements of etpnav_amd.pretrain.MlmStep._select_host, on the CPU"""
    B, Lt = txt_labels.shape
    sel = (txt_labels != -1).reshape(-1)
    rows = torch.nonzero(sel).reshape(-1).to(torch.int32)
    ptr_t = torch.zeros(B * Lt + 1, dtype=torch.int32)
    ptr_t[1:] = torch.cumsum(sel.to(torch.int32), 0)
    labels = txt_labels.reshape(-1)[sel].to(torch.int64).contiguous()
    return rows.numpy(), ptr_t.numpy(), labels.numpy(), int(rows.numel())


def cases():
    out = {}
    for n in (1, 16, 63, 64, 65, 257, 1000):
        for p in ms.PATTERNS:
            out[f"{p}-{n}"] = ms.pattern(p, n).reshape(1, n)
    two = np.concatenate([ms.pattern("every7", 24), np.full(24, -1, np.int32)]).reshape(2, 24)      # two adjacent rows, one empty
    out["two_rows_second_empty"], out["two_rows_first_empty"] = two, two[::-1].copy()
    out["golden"] = np.load(GOLDEN)["mlm_all_txt_labels"]
    return out


CASES = cases()


def same(got, want, what):
    for g, w, name in zip(got[:3], want[:3], ("rows", "ptr_t", "labels")):
        assert g.dtype == w.dtype and g.shape == w.shape and np.array_equal(g, w), f"{what}: {name}"
    assert got[3] == want[3], f"{what}: count"


@pytest.mark.parametrize("name", list(CASES))
def test_restatement_equals_the_host_build(name):
    lab = CASES[name]
    same(ms.select(lab), host_build(torch.from_numpy(lab.astype(np.int64))), name)
    rows, ptr_t, labels, count = ms.select(lab)
    assert ms.safe(rows, ptr_t, labels, lab.size, ms.VOCAB, count) is None
    assert ms.flags(lab, ms.VOCAB, count) == 0


def test_golden_batch_is_what_the_loader_recorded():
    lab = CASES["golden"]
    assert lab.shape == (5, 16) and lab.dtype == np.int64 and (lab != -1).sum() >= 2 and (lab == -1).any()


@pytest.mark.parametrize("mutation", ms.MUTATIONS)
def test_planted_mutations_are_rejected(mutation):
    """every case with at least two selected entries shows every mutation (a single entry has no order to reverse); labels taken one
    position on differ wherever the neighbour is not masked or holds another token"""
    shown = 0
    for name, lab in CASES.items():
        want = host_build(torch.from_numpy(lab.astype(np.int64)))
        if want[3] < 2 or name.startswith("all-"):
            continue
        got = ms.select(lab, mutate=mutation)
        differs = any(g.shape != w.shape or not np.array_equal(g, w) for g, w in zip(got[:3], want[:3]))
        assert differs, f"{mutation} passes on {name}"
        shown += 1
    assert shown >= 10
    lab = CASES["all-257"]                 # all masked: the shifted labels differ as soon as two neighbours hold different tokens
    got, want = ms.select(lab, mutate=mutation), host_build(torch.from_numpy(lab.astype(np.int64)))
    assert any(not np.array_equal(g, w) for g, w in zip(got[:3], want[:3]))


def test_safety_predicate_and_flags():
    lab = ms.pattern("every7", 65)
    rows, ptr_t, labels, count = ms.select(lab)
    n = lab.size
    assert ms.safe(rows, ptr_t, labels, n, ms.VOCAB, count) is None
    bad = rows.copy(); bad[-1] = n
    assert "row outside" in ms.safe(bad, ptr_t, labels, n, ms.VOCAB, count)
    bad = rows.copy(); bad[0] = -1
    assert "row outside" in ms.safe(bad, ptr_t, labels, n, ms.VOCAB, count)
    bad = labels.copy(); bad[1] = ms.VOCAB
    assert "label outside" in ms.safe(rows, ptr_t, bad, n, ms.VOCAB, count)
    bad = labels.copy(); bad[1] = -1
    assert "label outside" in ms.safe(rows, ptr_t, bad, n, ms.VOCAB, count)
    bad = ptr_t.copy(); bad[5] = bad[4] - 1
    assert "decreases" in ms.safe(rows, bad, labels, n, ms.VOCAB, count)
    assert "exceeds" in ms.safe(rows, ptr_t, labels, n, ms.VOCAB, count - 1)
    assert "shorter" in ms.safe(rows, ptr_t, labels, n, ms.VOCAB, count + 1)
    assert ms.flags(lab, ms.VOCAB, count + 1) == ms.ERR_COUNT and ms.flags(lab, ms.VOCAB, count - 1) == ms.ERR_COUNT
    lab2 = lab.copy(); lab2[3] = -2
    assert ms.flags(lab2, ms.VOCAB, count + 1) == ms.ERR_LABEL          # -2 is selected (it is not -1): the count rises with it
    lab2 = lab.copy(); lab2[0] = ms.VOCAB
    assert ms.flags(lab2, ms.VOCAB, count) == ms.ERR_LABEL
    lab2[0] = ms.VOCAB - 1
    assert ms.flags(lab2, ms.VOCAB, count) == 0


def test_host_route_of_the_step_is_the_pinned_build():
    """the step's own fallback (select='host') holds the same statements this file runs"""
    import inspect
    from etpnav_amd import pretrain
    src = inspect.getsource(pretrain.MlmStep._select_host)
    for stmt in ("torch.nonzero(sel).reshape(-1).to(torch.int32)", "torch.cumsum(sel.to(torch.int32), 0)",
                 '(batch["txt_labels"] != -1).reshape(-1)', "[sel].to(torch.int64)"):
        assert stmt in src, stmt
    assert (pretrain.MLM_ERR_COUNT, pretrain.MLM_ERR_LABEL) == (ms.ERR_COUNT, ms.ERR_LABEL)
