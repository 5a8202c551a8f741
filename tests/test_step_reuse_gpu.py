"""Step objects that outlive their batch (etpnav_amd/step.py _Staging, capacity=...; PretrainDriver(reuse_steps=True)) on the MI355X.

One capacity PlannerStep and one capacity MlmStep run a sequence of six batches through load_batch with no synchronise in between (the
one load that has to grow synchronises by itself).  Along the sequence every one of B, L, R, V, G, Nm shrinks and grows; B = 1 occurs
once, batch 2 equals the capacity exactly, batch 4 exceeds it (regrows == 1).  Before each load the stashes, workspaces and API tensors
-- values only, COVERAGE.md's schedule matrix -- are overwritten with 0xFF bytes, so a stale read shows as NaN.  Each batch is compared
with a fresh fixed step built for that batch alone, same dropout seed and step_no, eval and dropout modes, fp32 and bf16:
forward tensors bit for bit, loss and every parameter gradient within the tolerance tests/test_sched_gpu.py uses for "same kernels,
other order of atomics" (|got - ref| <= tol * max(1, max|ref|), tol 1e-4 fp32 / 2e-3 bf16, loss 1e-5; all-zero stays all-zero).
That every side stream is joined when run_eager returns -- what the sync-free reuse rests on -- is test_sched_gpu.py's "ends joined"
check and is not shown again here.  A fixed step (no capacity) is the same route with its first batch as its capacity: it reloads a batch
of its dimensions in place with every pointer kept, refuses one more masked token and inputs that disagree with the batch's dimensions,
and carries the rows validate.sap_eval writes."""
import pytest
import torch

from etpnav_amd import _lib, pretrain
from etpnav_amd import pretrain_data as pdata
from etpnav_amd import step as step_mod
from tests.test_sched_gpu import compare, compare_loss, grad_slices

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
# (B, L, T, V, n_cand, batch seed, mask seed): R = B * T, G follows T and n_cand
SEQ = ((3, 19, 3, 9, 4, 11, 101), (1, 11, 2, 7, 3, 12, 102), (4, 24, 3, 11, 4, 13, 103), (2, 15, 2, 8, 3, 14, 104),
       (5, 28, 4, 12, 5, 15, 105), (3, 19, 3, 9, 4, 16, 106))
CAP_AT, GROWS_AT = 2, 4


def _batch(cfg, B, L, T, V, nc, bseed, mseed, pick=None):
    """one batch of the sequence; `pick`: the masked positions (default: drawn from mseed among the batch's own tokens)"""
    from etpnav_amd.synthetic import make_sap_batch
    b = make_sap_batch(cfg.vocab_size, cfg.image_feat_size, cfg.depth_feat_size, B, L, T, V, n_cand=nc, seed=bseed, ragged=True)
    lab = torch.full_like(b["txt_ids"], -1)
    if pick is None:
        g = torch.Generator().manual_seed(mseed)
        pick = (torch.rand(lab.shape, generator=g) < 0.25) & b["txt_masks"]
        pick[:, 1] = True
    lab[pick] = b["txt_ids"][pick]
    ids = b["txt_ids"].clone()
    ids[pick] = 103
    b["txt_ids"], b["txt_labels"] = ids, lab
    return b


@pytest.fixture(scope="module")
def case():
    from oracle.make_golden_pretrain import make_case
    cfg, P, _ = make_case()
    return cfg, P, [_batch(cfg, *spec) for spec in SEQ]


def dims(b):
    return {"B": b["txt_ids"].shape[0], "L": b["txt_ids"].shape[1], "R": b["rgb_fts"].shape[0], "V": b["rgb_fts"].shape[1],
            "G": b["gmap_step_ids"].shape[1], "Nm": int((b["txt_labels"] != -1).sum())}


def test_the_sequence_is_what_the_file_says(case):
    d = [dims(b) for b in case[2]]
    cap = d[CAP_AT]
    for k in step_mod.CAPACITY_KEYS:
        seq = [x[k] for x in d]
        assert any(a > b for a, b in zip(seq, seq[1:])) and any(a < b for a, b in zip(seq, seq[1:])), (k, seq)
        assert all(x[k] <= cap[k] for x in d[:GROWS_AT]) and d[GROWS_AT][k] > cap[k], (k, seq)
    assert [x["B"] for x in d].count(1) == 1 and len(d) >= 5


def _model(cfg, P, dtype):
    from etpnav_amd.planner import GlocalTextPathNavCMT
    m = GlocalTextPathNavCMT(cfg.to_dict(), dtype=dtype, device=DEV)
    m.load_state_dict(dict(P), strict=True)
    return m.eval()


def _make(task, model, batch, dropout, **kw):
    if task == "sap":
        return step_mod.PlannerStep(model, batch, dropout=dropout, drop_seed=5, grad_overwrite=False, **kw)
    return pretrain.MlmStep(model, batch, dropout=dropout, drop_seed=5, **kw)


FWD = {"sap": ("txt", "pano", "gimg", "logits"), "mlm": ("txt", "pano", "gimg")}


def _snap(task, step, model):
    """on-stream copies of what is compared: no synchronise"""
    out = {k: getattr(step, k).clone() for k in FWD[task] + ("loss",)}
    if task == "mlm":
        out["scores"] = step.scores().clone()
    out["grads"] = model._engine.grads.clone()
    return out


def _poison(step):
    for k, t in step._pool.items():
        if k in step._api_tensors(step._d) or k in step._byte_buffers(step._d):
            t.fill_(0xFF)


@pytest.mark.parametrize("dropout", [None, "config"], ids=["eval", "dropout"])
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["fp32", "bf16"])
@pytest.mark.parametrize("task", ["sap", "mlm"])
def test_one_capacity_step_runs_the_sequence(case, task, dtype, dropout):
    """KNOWN TO FAIL INTERMITTENTLY on task = sap, on one tensor and through the "all-zero stays all-zero" clause alone:
    `grad global_sap_head.net.4.bias`, one element.  It is zero in exact arithmetic for every input (the bias is added to all node logits
    in front of the softmax; its gradient is the sum over the nodes of softmax - onehot) and sap_tail_bwd_kernel adds it up with one float
    atomic per workgroup, so the order decides between 0.0 and a residue.  Measured on the MI355X with FRESH steps only, six runs of one
    batch each: batch 2 in fp32 0.0, 1.5e-8, 1.5e-8, 7.5e-9, 0.0, 1.5e-8; batch 3 in bf16 0.0, 3.0e-8, 1.5e-8, 1.5e-8, 3.0e-8, 0.0 --
    the route this test takes as its reference does not reproduce its own zero.  The reused step's values over three passes lie in the
    same sets (0.0, 0.0, 7.5e-9 and 3.0e-8, 1.5e-8, 3.0e-8).  In the one full run of this file 3 of the 24 sap comparisons tripped
    the clause (1.5e-8 .. 3.0e-8 against 0.0); every other tensor of every case was within 0.2 % of its bound, every forward tensor
    bit-identical.  The clause is kept as it was set."""
    cfg, P, batches = case
    model = _model(cfg, P, dtype)
    refs = []
    for k, b in enumerate(batches):                      # today's route: a step object per batch
        st = _make(task, model, b, dropout)
        st.step_no = 7 + k
        st.run_eager()
        torch.cuda.synchronize()
        refs.append(_snap(task, st, model))
        st.close()
    cap = dims(batches[CAP_AT])
    step = _make(task, model, batches[0], dropout, capacity=cap if task == "mlm" else {k: v for k, v in cap.items() if k != "Nm"})
    got = []
    try:
        assert step.regrows == 0
        for k, b in enumerate(batches):
            _poison(step)
            step.load_batch(b)
            assert step.regrows == (1 if k >= GROWS_AT else 0), (k, step.regrows)
            assert tuple(step.txt.shape) == (b["txt_ids"].shape[0], b["txt_ids"].shape[1], cfg.hidden_size) and step.txt.is_contiguous()
            assert step.txt.data_ptr() == step._pool["txt"].data_ptr() and step.inp["rgb"].data_ptr() == step._pool["in:rgb"].data_ptr()
            step.step_no = 7 + k
            step.run_eager()
            got.append(_snap(task, step, model))
        torch.cuda.synchronize()
        if task == "mlm":
            step.check_select()
        step.check_traj()
    finally:
        torch.cuda.synchronize()
        step.close()
    failures = _differences(task, dtype, model, got, refs)
    assert not failures, "\n".join(failures[:20])


def _differences(task, dtype, model, got, refs):
    """every snapshot of `got` against the fresh step's of `refs`: forward tensors bit for bit, loss and gradients within the file's
    tolerances -> the failures"""
    tol = 1e-4 if dtype == torch.float32 else 2e-3
    names = grad_slices(model)
    eng = model._engine
    offs = {n: (t.data_ptr() - eng.grads.data_ptr()) // 4 for n, t in names.items()}
    failures = []
    for k, (g, r) in enumerate(zip(got, refs)):
        for name in FWD[task] + (("scores",) if task == "mlm" else ()):
            if not torch.equal(g[name].view(torch.uint8), r[name].view(torch.uint8)):
                failures.append(f"batch {k}: {name} differs from the fresh step's bits "
                                f"({int((g[name] != r[name]).sum())} elements, {int(g[name].isnan().sum())} NaN)")
        bad, ratio = compare_loss("loss", g["loss"], r["loss"])
        print(f"{task} {dtype} batch {k}: loss {float(g['loss']):.7f} against {float(r['loss']):.7f} ({ratio:.3g} of the tolerance)")
        if bad:
            failures.append(f"batch {k}: {bad}")
        worst = 0.0
        for n, t in names.items():
            sl = slice(offs[n], offs[n] + t.numel())
            bad, ratio = compare(n, g["grads"][sl], r["grads"][sl], tol)
            worst = max(worst, ratio if ratio != float("inf") else 0.0)
            if bad:
                failures.append(f"batch {k}: {bad}")
        print(f"{task} {dtype} batch {k}: worst gradient |err| / tolerance {worst:.3g}")
    return failures


def _ptrs(step):
    """data_ptr() of every input, API tensor, stash and workspace of the step"""
    out = {"in:" + k: t.data_ptr() for k, t in step.inp.items()}
    out.update({k: getattr(step, k).data_ptr() for k in list(step._api_tensors(step._d)) + list(step._byte_buffers(step._d))})
    return out


@pytest.mark.parametrize("task", ["sap", "mlm"])
def test_a_fixed_step_reloads_a_batch_of_its_shape_in_place(case, task):
    """A fixed step (no capacity) run on batch 0, then loaded with a second batch of the same dimensions -- other seeds for every tensor,
    the masked positions of batch 0, so Nm is equal -- against a fresh step built for that second batch: the comparison and the
    tolerances of test_one_capacity_step_runs_the_sequence (its docstring's intermittent clause on task = sap included)."""
    cfg, P, batches = case
    dtype, dropout = torch.float32, "config"
    second = _batch(cfg, *SEQ[0][:5], 21, None, pick=batches[0]["txt_labels"] != -1)
    assert dims(second) == dims(batches[0]) and not torch.equal(second["rgb_fts"], batches[0]["rgb_fts"])
    model = _model(cfg, P, dtype)
    fresh = _make(task, model, second, dropout)
    fresh.step_no = 8
    fresh.run_eager()
    torch.cuda.synchronize()
    ref = _snap(task, fresh, model)
    fresh.close()
    step = _make(task, model, batches[0], dropout)
    try:
        assert step._fixed and step.regrows == 0
        step.step_no = 7
        step.run_eager()
        before = _ptrs(step)
        assert {"in:rgb", "in:txt_ids", "txt", "pano", "gimg", "st_txt", "ws_txt", "st_pano", "ws_pano"} <= set(before)
        _poison(step)
        step.load_batch(second)                          # accepted
        assert step.regrows == 0 and _ptrs(step) == before
        step.step_no = 8
        step.run_eager()
        got = _snap(task, step, model)
        torch.cuda.synchronize()
        if task == "mlm":
            step.check_select()
        step.check_traj()
    finally:
        torch.cuda.synchronize()
        step.close()
    failures = _differences(task, dtype, model, [got], [ref])
    assert not failures, "\n".join(failures[:20])


def test_a_fixed_step_refuses_what_it_was_not_built_for(case):
    cfg, P, batches = case
    model = _model(cfg, P, torch.float32)
    b = batches[0]
    more = dict(b)
    free = torch.nonzero((b["txt_labels"] == -1) & b["txt_masks"])[0]
    more["txt_labels"] = b["txt_labels"].clone()
    more["txt_labels"][free[0], free[1]] = b["txt_ids"][free[0], free[1]]
    assert {k: v for k, v in dims(more).items() if k != "Nm"} == {k: v for k, v in dims(b).items() if k != "Nm"}
    assert dims(more)["Nm"] == dims(b)["Nm"] + 1
    mlm = pretrain.MlmStep(model, b)
    try:
        with pytest.raises(ValueError, match="differ from this step's"):
            mlm.load_batch(more)                         # the same (B, L, R, V, G), one more masked token
    finally:
        mlm.close()
    short = dict(b)
    short["dep_fts"] = b["dep_fts"][:, :-1]              # one view fewer than rgb_fts
    with pytest.raises(ValueError, match=r"batch\['dep_fts'\] has shape .* the batch's dimensions"):
        step_mod.PlannerStep(model, short)
    sap = step_mod.PlannerStep(model, b)
    try:
        with pytest.raises(ValueError, match=r"batch\['dep_fts'\] has shape .* the batch's dimensions"):
            sap.load_batch(short)
    finally:
        torch.cuda.synchronize()
        sap.close()


def test_sap_eval_writes_into_the_rows_a_fixed_step_planned(case):
    from etpnav_amd.validate import EvalCounters, sap_eval
    cfg, P, batches = case
    model = _model(cfg, P, torch.float32)
    step = step_mod.PlannerStep(model, batches[0], dropout=None, zero_grads=False, grad_overwrite=False)
    try:
        B = batches[0]["txt_ids"].shape[0]
        assert step._fixed and tuple(step.row_nll.shape) == tuple(step.row_pred.shape) == (B,)
        assert step.row_nll.dtype == torch.float32 and step.row_pred.dtype == torch.int32
        at = (step.row_nll.data_ptr(), step.row_pred.data_ptr())
        assert at == (step._pool["row_nll"].data_ptr(), step._pool["row_pred"].data_ptr())
        counters = EvalCounters(DEV)
        for _ in range(2):
            step.run_eager(backward=False)
            sap_eval(step, counters)
            assert (step.row_nll.data_ptr(), step.row_pred.data_ptr()) == at
        torch.cuda.synchronize()
        loss_sum, _, n_rows = counters.read()
        assert n_rows == 2 * B and abs(loss_sum - 2.0 * float(step.row_nll.double().sum())) <= 1e-4 * abs(loss_sum)   # the rows were written
    finally:
        torch.cuda.synchronize()
        step.close()


def test_kernel_route_and_host_route_build_the_same_selection(case):
    cfg, P, batches = case
    model = _model(cfg, P, torch.float32)
    step = pretrain.MlmStep(model, batches[0], capacity=True)
    try:
        assert step.select == "device"
        for b in (batches[0], batches[3], batches[2]):
            step.select = "device"
            step.load_batch(b)
            torch.cuda.synchronize()
            step.check_select()
            dev = [t.clone() for t in step.sel + step.selT + (step.labels,)]
            step.select = "host"
            step.load_batch(b)
            torch.cuda.synchronize()
            host = list(step.sel + step.selT + (step.labels,))
            for name, d, h in zip(("sel ptr", "sel idx", "sel w", "selT ptr", "selT idx", "selT w", "labels"), dev, host):
                assert d.dtype == h.dtype and d.shape == h.shape and torch.equal(d, h), name
    finally:
        torch.cuda.synchronize()
        step.close()


def test_env_switch_and_no_masked_tokens(case, monkeypatch):
    cfg, P, batches = case
    model = _model(cfg, P, torch.float32)
    monkeypatch.setenv("ETP_MLM_SELECT", "0")
    st = pretrain.MlmStep(model, batches[0])
    monkeypatch.delenv("ETP_MLM_SELECT")
    assert st.select == "host"
    st.close()
    st = pretrain.MlmStep(model, batches[0], capacity=True)
    try:
        empty = dict(batches[1])
        empty["txt_labels"] = torch.full_like(empty["txt_labels"], -1)
        with pytest.raises(ValueError, match="no masked tokens in the batch"):
            st.load_batch(empty)
        with pytest.raises(ValueError, match="no masked tokens in the batch"):
            pretrain.MlmStep(model, empty)
        fixed = pretrain.MlmStep(model, batches[0])
        with pytest.raises(ValueError, match="differ from this step's"):
            fixed.load_batch(batches[1])
        fixed.load_batch(batches[0])                     # same shape: accepted
        fixed.close()
        sap = step_mod.PlannerStep(model, batches[0])
        with pytest.raises(ValueError, match="differ from this step's"):
            sap.load_batch(batches[1])
        sap.close()
    finally:
        torch.cuda.synchronize()
        st.close()


def test_planted_wrong_count_is_reported_by_check_select(case):
    cfg, P, batches = case
    model = _model(cfg, P, torch.float32)
    b = pdata.TrajBatch(batches[0])
    true = int((b["txt_labels"] != -1).sum())
    b.mlm_dev = {"txt_labels": b["txt_labels"].to(torch.int32).to(DEV), "n_masked": true}
    st = pretrain.MlmStep(model, b, capacity=True)
    try:
        torch.cuda.synchronize()
        st.check_select()
        assert st.Nm == true and st._lab_src is b.mlm_dev["txt_labels"]
        b.mlm_dev["n_masked"] = true + 1
        st.load_batch(b)                                 # staged, never run: nothing downstream of a flagged selection is launched
        torch.cuda.synchronize()
        with pytest.raises(_lib.EtpError, match=rf"ETP_MLM_ERR_COUNT: {true} entries .* n_masked = {true + 1}"):
            st.check_select()
    finally:
        torch.cuda.synchronize()
        st.close()


class _Counting:
    def __init__(self, monkeypatch):
        self.made = []
        outer = self

        class Sap(step_mod.PlannerStep):
            def __init__(self, *a, **kw):
                outer.made.append(("sap", kw.get("dropout") is not None, kw.get("capacity") is not None))
                super().__init__(*a, **kw)

        class Mlm(pretrain.MlmStep):
            def __init__(self, *a, **kw):
                outer.made.append(("mlm", kw.get("dropout") is not None, kw.get("capacity") is not None))
                super().__init__(*a, **kw)

        monkeypatch.setattr(step_mod, "PlannerStep", Sap)
        monkeypatch.setattr(pretrain, "MlmStep", Mlm)


@pytest.mark.parametrize("dtype,lr", [(torch.float32, 1e-4), (torch.bfloat16, 0.0)], ids=["fp32", "bf16"])
def test_driver_with_reused_steps_against_the_flag_off(case, dtype, lr, monkeypatch):
    """Four optimizer steps of mixed shapes and tasks, then validate(), flag on against flag off with the same seeds.  fp32 trains at
    1e-4.  bf16 runs the same four optimizer steps at learning rate 0: with a rate the flag-off driver does not reproduce ITSELF in
    bf16 (measured, two flag-off runs of this very schedule: losses 2.17039 against 2.17419 at the third step, 8.03332 against 8.03227
    at the fourth, validation gloss apart by 1.7e-3 -- an update that moves a master weight across a bf16 rounding boundary or not
    turns the atomics' last-bit noise into a 2^-8 relative step), so no bound on a trained bf16 trajectory could tell the two routes
    apart; at rate 0 every step, the optimizer's included, still runs and the issue's bounds hold per step."""
    cfg, P, batches = case
    count = _Counting(monkeypatch)
    runs = {}
    for reuse in (False, True):
        count.made.clear()
        model = _model(cfg, P, dtype)
        gen = torch.Generator().manual_seed(3)
        loaders = {"mlm": (batches[:4], 1, None), "sap": (batches[2:], 1, None)}
        drv = pretrain.PretrainDriver(model, loaders, learning_rate=lr, warmup_steps=2, num_train_steps=10, seed=4, generator=gen,
                                      reuse_steps=reuse, batch_size=2, max_txt_len=16)
        try:
            out = drv.run(4)
            tasks = [n for n, _ in out]
            before = {k: v.detach().clone() for k, v in model.state_dict().items()}
            log = drv.validate({"mlm": batches[:3], "sap": batches[3:]}, setname="_seen")
            torch.cuda.synchronize()
            after = model.state_dict()
            assert all(torch.equal(before[k], after[k]) for k in before), "validate() changed a parameter"
            made = list(count.made)
            if reuse:
                assert sorted(m for m in made if m[1]) == [(t, True, True) for t in sorted(set(tasks))], made   # ONE per task
                assert sorted(m for m in made if not m[1]) == [("mlm", False, True), ("sap", False, True)], made
                assert not drv._sap and not drv._sap_eval and len(drv._reused) == len(made)
                drv.check_steps()
                assert all(st.regrows >= 0 for st in drv._reused.values())
            else:
                assert all(not m[2] for m in made) and not drv._reused
            runs[reuse] = {"tasks": tasks, "losses": [float(l) for _, l in out], "log": log, "global_step": drv.global_step,
                           "micro": drv._micro, "made": made, "params": before}
        finally:
            torch.cuda.synchronize()
            drv.close()
    off, on = runs[False], runs[True]
    assert set(off["tasks"]) == {"mlm", "sap"}, "the plan of this seed mixes both tasks"
    assert off["tasks"] == on["tasks"] and (off["global_step"], off["micro"]) == (on["global_step"], on["micro"]) == (4, 0)
    print(f"{dtype}: constructions flag off {len(off['made'])}, flag on {len(on['made'])}; losses off {off['losses']} on {on['losses']}")
    print(f"{dtype}: validation off {off['log']} on {on['log']}")
    for a, b in zip(off["losses"], on["losses"]):
        assert abs(a - b) < 1e-5, (off["losses"], on["losses"])
    for k, v in off["log"].items():
        if k.endswith("tok_per_s"):
            continue
        if dtype == torch.float32 and k.endswith("acc"):
            assert on["log"][k] == v, (k, v, on["log"][k])
        else:
            assert abs(on["log"][k] - v) < (1e-5 if k.endswith("loss") else 1e-4 if dtype == torch.float32 else 2e-3), (k, v, on["log"][k])
    tol = 1e-4 if dtype == torch.float32 else 2e-3
    for k, v in off["params"].items():
        if v.is_floating_point():
            bad, _ = compare("parameter " + k, on["params"][k], v, tol)
            assert bad is None, bad
