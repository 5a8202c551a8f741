"""The one allocation route of etpnav_amd/step.py _Staging (_plan / _bind / load_batch), driven without a GPU: PlannerStep and MlmStep are
built over a stub engine whose ``buf`` hands out CPU byte tensors and whose library answers every byte query with a fixed formula of the
dimensions it is asked about (every other call succeeds and does nothing), in the manner of _StubLib in
tests/test_mlm_select_boundary_cpu.py.  What is under test is the host bookkeeping alone: which names are planned, what grows and when,
what a fixed step refuses, and that every tensor of the step is a contiguous view at offset 0 of its allocation."""
import contextlib
import types

import pytest
import torch

from etpnav_amd import pretrain
from etpnav_amd import step as step_mod
from etpnav_amd.synthetic import make_sap_batch

VOCAB, IMG, DEP, HIDDEN = 3000, 16, 8, 8
# the names whose plan has the text length in it (PlannerStep): what a batch that differs in L alone finds short
L_NAMES = {"in:txt_ids", "in:txt_masks", "txt", "d_txt", "st_txt", "ws_txt", "st_nav", "ws_nav"}


class _Lib:
    """etp_*_bytes(handle, dims...) = 64 + 8 * the product of the dimensions (4 * for a workspace); anything else returns 0"""

    queries = 0

    def __getattr__(self, name):
        if name.endswith("_bytes"):
            def nbytes(handle, *dims):
                self.queries += 1
                n = 1
                for x in dims:
                    n *= x
                return 64 + (4 if "_ws_" in name else 8) * n
            return nbytes
        return lambda *a: 0


class _Engine:
    def __init__(self):
        self.L, self.handle, self.device = _Lib(), None, torch.device("cpu")
        self.cconf = types.SimpleNamespace(hidden=HIDDEN, vocab=VOCAB, use_lang2visn=True, n_l=1)
        self.bufs = []                         # the size of every allocation, in order

    def require_gpu(self):
        pass

    def buf(self, nbytes):
        self.bufs.append(int(nbytes))
        return torch.zeros(int(nbytes), dtype=torch.uint8)

    def stream(self):
        return 0

    def scope(self, **kw):
        return contextlib.nullcontext()

    def release_aux(self):
        pass


def _batch(B, L, T, V, nc, seed, extra_masked=0):
    b = make_sap_batch(VOCAB, IMG, DEP, B, L, T, V, n_cand=nc, seed=seed)
    lab = torch.full_like(b["txt_ids"], -1)
    lab[:, 1] = b["txt_ids"][:, 1]
    for k in range(extra_masked):
        lab[0, 2 + k] = b["txt_ids"][0, 2 + k]
    b["txt_labels"] = lab
    return b


def _make(task, batch, **kw):
    eng = _Engine()
    model = types.SimpleNamespace(_engine=eng, config={}, drop_env_prob=0.0)
    if task == "sap":
        return step_mod.PlannerStep(model, batch, traj_nodes=False, **kw), eng
    return pretrain.MlmStep(model, batch, traj_nodes=False, **kw), eng


def _bound(step):
    """name -> the step's tensor of every planned name"""
    return {k: step.inp[k[3:]] if k.startswith("in:") else getattr(step, k) for k in step._pool}


@pytest.fixture
def syncs(monkeypatch):
    seen = []
    monkeypatch.setattr(torch.cuda, "synchronize", lambda device=None: seen.append(device))
    return seen


@pytest.mark.parametrize("task", ["sap", "mlm"])
def test_fixed_and_capacity_steps_bind_the_same(task, syncs):
    batch = _batch(3, 9, 2, 5, 3, seed=1)
    fixed, feng = _make(task, batch)
    cap, ceng = _make(task, batch, capacity=True)
    assert fixed._fixed and not cap._fixed and isinstance(fixed._pool, dict)
    assert list(fixed._pool) == list(cap._pool) and feng.bufs == ceng.bufs
    need = fixed._plan(fixed._d, batch)
    assert set(need) == set(fixed._pool)
    assert "row_nll" in need and "row_pred" in need and all("in:" + k in need for k, _, _ in step_mod.INPUTS[:fixed._n_inputs])
    for (k, a), (_, b) in zip(_bound(fixed).items(), _bound(cap).items()):
        assert a.shape == b.shape and a.dtype == b.dtype, k
        assert fixed._pool[k].numel() == cap._pool[k].numel() == max(need[k][0], 1), k
        if need[k][1] is not None:
            assert tuple(a.shape) == need[k][1] and a.dtype == need[k][2], k
    assert fixed.shape_key() == cap.shape_key() == tuple(fixed._d.values())
    if task == "sap":
        assert fixed.shape_key() == step_mod.PlannerStep.batch_shape_key(batch)
    assert fixed.regrows == cap.regrows == 0 and not syncs


@pytest.mark.parametrize("task", ["sap", "mlm"])
def test_a_fixed_step_takes_its_own_dimensions_only(task, syncs):
    batch = _batch(3, 9, 2, 5, 3, seed=1)
    step, eng = _make(task, batch)
    n_bufs, ptrs, d = len(eng.bufs), {k: t.data_ptr() for k, t in _bound(step).items()}, dict(step._d)
    others = {"B": _batch(2, 9, 2, 5, 3, seed=2), "L": _batch(3, 10, 2, 5, 3, seed=2), "R, G": _batch(3, 9, 3, 5, 3, seed=2),
              "V": _batch(3, 9, 2, 6, 3, seed=2)}
    if task == "mlm":
        others["Nm"] = _batch(3, 9, 2, 5, 3, seed=1, extra_masked=1)
    for what, other in others.items():
        with pytest.raises(ValueError, match="differ from this step's"):
            step.load_batch(other)
        assert step._d == d and {k: t.data_ptr() for k, t in _bound(step).items()} == ptrs, what
    if task == "sap":
        step.loss_scale = 0.125                # a caller's scale (MicroBatchedStep): a fixed load leaves it alone
    again, asked = _batch(3, 9, 2, 5, 3, seed=7), eng.L.queries
    step.load_batch(again)
    assert step.regrows == 0 and not syncs and len(eng.bufs) == n_bufs
    assert eng.L.queries == asked                          # the bound shape again: nothing is planned anew
    assert {k: t.data_ptr() for k, t in _bound(step).items()} == ptrs
    assert torch.equal(step.inp["rgb"], again["rgb_fts"]) and torch.equal(step.inp["txt_ids"], again["txt_ids"])
    if task == "sap":
        assert step.loss_scale == 0.125
        step.graphs = [1]
        with pytest.raises(RuntimeError, match="captured / recorded graphs"):
            step.load_batch(again)
        step.graphs = []


@pytest.mark.parametrize("capacity", [None, True])
def test_inputs_that_disagree_with_the_dimensions_are_refused(capacity, syncs):
    batch = _batch(3, 9, 2, 5, 3, seed=1)
    bad = dict(batch)
    bad["dep_fts"] = batch["dep_fts"][:, :-1]              # one view fewer than rgb_fts
    with pytest.raises(ValueError, match=r"batch\['dep_fts'\] has shape .* the batch's dimensions"):
        _make("sap", bad, capacity=capacity)
    step, _ = _make("sap", batch, capacity=capacity)
    d = dict(step._d)
    with pytest.raises(ValueError, match=r"batch\['dep_fts'\] has shape .* the batch's dimensions"):
        step.load_batch(bad)
    assert step._d == d and step.regrows == 0


def test_a_capacity_step_grows_what_is_short_and_counts_it_once(syncs):
    big, small, longer = _batch(3, 9, 2, 5, 3, seed=1), _batch(2, 7, 2, 4, 3, seed=2), _batch(3, 12, 2, 5, 3, seed=3)
    step, eng = _make("sap", small, capacity={k: v for k, v in zip("BLRVG", step_mod.PlannerStep.batch_shape_key(big))})
    assert step._cap == dict(zip("BLRVG", step_mod.PlannerStep.batch_shape_key(big))) and step.regrows == 0 and not syncs
    n_bufs, pool = len(eng.bufs), dict(step._pool)
    for b in (big, small):                                 # the capacity itself, then a shrink: nothing is allocated
        step.load_batch(b)
        assert step.regrows == 0 and not syncs and len(eng.bufs) == n_bufs
        assert all(step._pool[k] is t for k, t in pool.items())
        assert step.loss_scale == 1.0 / b["txt_ids"].shape[0]
        for k, t in _bound(step).items():                  # prefixes at offset 0
            assert t.is_contiguous() and t.data_ptr() == step._pool[k].data_ptr(), k
            assert t.numel() * t.element_size() <= step._pool[k].numel(), k
        assert tuple(step.txt.shape) == (*b["txt_ids"].shape, HIDDEN) and tuple(step.inp["rgb"].shape) == tuple(b["rgb_fts"].shape)
    assert step.txt.numel() * 4 < step._pool["txt"].numel()                  # the shrink really is one
    step.load_batch(longer)                                # L alone exceeds the capacity
    grown = {k for k, t in pool.items() if step._pool[k] is not t}
    assert grown == L_NAMES and len(eng.bufs) == n_bufs + len(L_NAMES)
    assert step.regrows == 1 and len(syncs) == 1
    assert step._cap == {**step._cap, "L": 12} and set(step._pool) == set(pool)
    need = step._plan(step._d, longer)
    for k, t in _bound(step).items():
        assert t.is_contiguous() and t.data_ptr() == step._pool[k].data_ptr() and step._pool[k].numel() >= need[k][0], k
    step.load_batch(longer)                                # the same shape again: nothing more
    assert step.regrows == 1 and len(syncs) == 1 and len(eng.bufs) == n_bufs + len(L_NAMES)


def test_mlm_selection_arrays_are_written_over_the_whole_allocation(syncs):
    big, small = _batch(3, 9, 2, 5, 3, seed=1, extra_masked=2), _batch(2, 7, 2, 4, 3, seed=2)
    step, _ = _make("mlm", small, capacity={"Nm": 5})
    assert step.Nm == 2 and step._pool["_rows"].numel() == 5 * 4
    assert step._pool["_arange"].view(torch.int32).tolist() == list(range(6)) and step._pool["_ones"].view(torch.float32).tolist() == [1.0] * 5
    step.load_batch(big)                                   # Nm = 5: within the capacity, the prefixes are already filled
    assert step.Nm == 5 and step._arange.tolist() == list(range(6)) and step._ones.tolist() == [1.0] * 5
    assert step.sel[0] is step._arange and step.selT[1].data_ptr() == step._arange.data_ptr() and step.selT[1].numel() == 5


def test_a_route_switched_on_a_live_mlm_step_is_planned_anew(syncs):
    batch = _batch(3, 9, 2, 5, 3, seed=1)
    step, _ = _make("mlm", batch, select="host")
    assert "_rows" not in step._pool and step.labels.dtype == torch.int64
    step.select = "device"
    step.load_batch(batch)                                 # the bound shape, but the device route's arrays are not planned yet
    assert step.labels.data_ptr() == step._pool["labels"].data_ptr() and step._rows.numel() == step.Nm == 3
    assert step._pool["_arange"].view(torch.int32).tolist() == list(range(4))
    step.select = "host"
    step.load_batch(batch)
    assert step.labels.tolist() == batch["txt_ids"][:, 1].tolist() and step.sel[1].tolist() == [1, 10, 19]
    step.select = "device"
    step.load_batch(batch)
    assert step.labels.data_ptr() == step._pool["labels"].data_ptr()
