"""The validation tails of csrc/eval_tail.hip through the C ABI, the MLM validation entry through the engine, and
PretrainDriver.validate / run against the real pre-training model's recorded validation -- with the fp64 restatements, derived bounds
and case lists of tests/eval_ref.py (tests/test_eval_ref_cpu.py pins, emulates and mutates the same lists on the CPU).

  etp_vocab_eval   vocab_eval_kernel    row_nll within e_lse + u |nll|, row_pred exactly the lowest-index arg-max
  etp_sap_eval     sap_eval_kernel      the same; ignored rows exactly 0, their arg-max still written
  etp_eval_accum   eval_accum_kernel    loss_sum within (n + 1) 2^-53 (|previous| + sum |nll|) of the float64 sum of the kernel's own rows,
                                        counts exact, two calls into a record that starts non-zero

Every operator output starts as a payload NaN / 0xFF inside a guarded buffer whose guards must survive, every input is compared with
its copy afterwards, and a second run is bit-identical, the record included.
"""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from etpnav_amd import _lib  # noqa: E402
from etpnav_amd._lib import check, ptr  # noqa: E402
from tests import eval_ref as ev  # noqa: E402
from tests import move_ref as mv  # noqa: E402

DEV = "cuda"
gptr, guarded, exact = mv.gptr, mv.guarded, mv.exact


def L():
    return _lib.lib()


def stream():
    return torch.cuda.current_stream().cuda_stream


def sync():
    torch.cuda.synchronize()


def row_outputs(n):
    """row_nll as payload NaN, row_pred as 0xFF bytes, both guarded -> (Guarded nll, Guarded bytes, int32 view)"""
    pred = guarded((n * 4,), torch.uint8)
    return guarded((n,)), pred, pred.t.view(torch.int32)


def record(rec):
    """a guarded 32-byte record holding `rec` -> (Guarded bytes, int64 view)"""
    g = guarded((32,), torch.uint8)
    v = g.t.view(torch.int64)
    v.copy_(ev.pack_record(rec, DEV))
    g.ref = g.buf.clone()
    return g, v


def run_accum(name, nll, pred, labels, ignore_index, before):
    """etp_eval_accum twice from the same record: inside its bound, counts exact, the second run bit for bit"""
    n = int(labels.numel())
    nll0, pred0, labels0 = nll.clone(), pred.clone(), labels.clone()
    out = []
    for _ in range(2):
        g, v = record(before)
        check(L().etp_eval_accum(ptr(nll), ptr(pred), ptr(labels), n, ignore_index, v.data_ptr(), stream()), "eval_accum")
        sync()
        g.check(name + " record")
        out.append(v.clone())
    got = ev.unpack_record(out[0])
    ev.check_record(name, got, before, nll, pred, labels, ignore_index)
    exact(name + " record (second run)", out[0], out[1])
    exact(name + " row_nll (read only)", nll, nll0)
    exact(name + " row_pred (read only)", pred, pred0)
    exact(name + " labels (read only)", labels, labels0)
    return got


# ---- etp_vocab_eval ------------------------------------------------------------------------------------------------------------------
VOCAB = ev.vocab_cases()


@pytest.mark.parametrize("i", range(len(VOCAB)), ids=[f"V{c[0]}-ld{c[1]}-Nm{c[2]}-{c[3]:g}-{c[4]}" for c in VOCAB])
def test_vocab_eval(i):
    V, ldv, Nm, shift, special = VOCAB[i]
    c = ev.vocab_case(V, ldv, Nm, shift, special, i)
    buf, labels = c["buf"].to(DEV), c["labels"].to(DEV)
    buf0, labels0 = buf.clone(), labels.clone()
    runs = []
    for _ in range(2):
        nll, pb, pred = row_outputs(Nm)
        check(L().etp_vocab_eval(ptr(buf), ptr(labels), Nm, V, ldv, gptr(nll), pred.data_ptr(), stream()), "vocab_eval")
        sync()
        nll.check("vocab_eval row_nll")
        pb.check("vocab_eval row_pred")
        ev.check_rows("etp_vocab_eval", nll.t, pred, c["q"], ev.vocab_depth(V))
        runs.append((nll.t.clone(), pred.clone()))
    exact("etp_vocab_eval row_nll (second run)", runs[0][0].view(torch.int32), runs[1][0].view(torch.int32))
    exact("etp_vocab_eval row_pred (second run)", runs[0][1], runs[1][1])
    exact("etp_vocab_eval logits (read only)", buf, buf0)
    exact("etp_vocab_eval labels (read only)", labels, labels0)
    run_accum("etp_vocab_eval + etp_eval_accum", runs[0][0], runs[0][1], labels, -1, ev.START)


# ---- etp_sap_eval --------------------------------------------------------------------------------------------------------------------
SAP = ev.sap_cases()


@pytest.mark.parametrize("i", range(len(SAP)), ids=[f"B{c[0]}-G{c[1]}-{c[2][0]:g}-{c[2][1]}-{c[2][2]}-{c[3]}" for c in SAP])
def test_sap_eval(i):
    B, G, pat, special = SAP[i]
    c = ev.sap_case(B, G, pat, special, i)
    logits, labels, ii = c["logits"].to(DEV), c["labels"].to(DEV), c["ignore_index"]
    logits0, labels0 = logits.clone(), labels.clone()
    runs = []
    for _ in range(2):
        nll, pb, pred = row_outputs(B)
        check(L().etp_sap_eval(ptr(logits), ptr(labels), B, G, ii, gptr(nll), pred.data_ptr(), stream()), "sap_eval")
        sync()
        nll.check("sap_eval row_nll")
        pb.check("sap_eval row_pred")
        ev.check_rows("etp_sap_eval", nll.t, pred, c["q"], ev.sap_depth(G))
        runs.append((nll.t.clone(), pred.clone()))
    exact("etp_sap_eval row_nll (second run)", runs[0][0].view(torch.int32), runs[1][0].view(torch.int32))
    exact("etp_sap_eval row_pred (second run)", runs[0][1], runs[1][1])
    exact("etp_sap_eval logits (read only)", logits, logits0)
    exact("etp_sap_eval labels (read only)", labels, labels0)
    got = run_accum("etp_sap_eval + etp_eval_accum", runs[0][0], runs[0][1], labels, ii, (0.0, 0, 0, 0))   # its own record
    keep = c["q"]["keep"]
    assert got[2] == B and got[3] == int(keep.sum())
    if special == "label_neginf" and bool(keep[B // 2]):
        assert got[0] == float("inf")
    if special == "all_neginf":
        assert np.isnan(got[0])
    if not bool(keep.any()):
        assert got[:2] == (0.0, 0)


# ---- etp_eval_accum ------------------------------------------------------------------------------------------------------------------
ACCUM = ev.accum_cases()


@pytest.mark.parametrize("i", range(len(ACCUM)), ids=[f"n{n}-ignore{ii}" for n, ii in ACCUM])
def test_eval_accum_two_calls_into_a_record_that_starts_non_zero(i):
    n, ii = ACCUM[i]
    rec = ev.START
    for nll, pred, labels in ev.accum_case(n, ii, 3000 + i):
        rec = run_accum("etp_eval_accum", nll.to(DEV), pred.to(DEV), labels.to(DEV), ii, rec)
    assert rec[2] == ev.START[2] + 2 * n


def test_refused_calls_leave_the_outputs_as_they_were():
    nll, pb, pred = row_outputs(4)
    g, v = record(ev.START)
    logits = torch.zeros(4, 8, device=DEV)
    labels = torch.zeros(4, dtype=torch.int64, device=DEV)
    X, s = L(), stream()
    calls = [X.etp_vocab_eval(ptr(logits), ptr(labels), 4, 9, 8, gptr(nll), pred.data_ptr(), s),          # ldv < V
             X.etp_vocab_eval(ptr(logits), ptr(labels), 4, 0, 8, gptr(nll), pred.data_ptr(), s),
             X.etp_vocab_eval(None, ptr(labels), 4, 8, 8, gptr(nll), pred.data_ptr(), s),
             X.etp_sap_eval(ptr(logits), ptr(labels), 0, 8, -100, gptr(nll), pred.data_ptr(), s),
             X.etp_sap_eval(ptr(logits), None, 4, 8, -100, gptr(nll), pred.data_ptr(), s),
             X.etp_eval_accum(gptr(nll), pred.data_ptr(), ptr(labels), 0, -100, v.data_ptr(), s),
             X.etp_eval_accum(gptr(nll), pred.data_ptr(), ptr(labels), 4, -100, v.data_ptr() + 4, s),
             X.etp_eval_accum(gptr(nll), pred.data_ptr(), ptr(labels), 4, -100, None, s)]
    sync()
    assert calls == [-1] * len(calls), calls
    nll.intact("refused: row_nll")
    pb.intact("refused: row_pred")
    g.intact("refused: record")


# ---- engine: MlmStep.run_eval against MlmStep.scores() and etp_mlm_fwd ---------------------------------------------------------------
def build_model(cfg, P, dtype):
    from etpnav_amd.planner import GlocalTextPathNavCMT
    m = GlocalTextPathNavCMT(cfg.to_dict(), dtype=dtype, device="cuda")
    m.load_state_dict({k: v for k, v in P.items()}, strict=True)
    return m.eval()


_FIX = {}


def fixture():
    """the recorded validation and its loaders, built once and left unchanged"""
    if not _FIX:
        z = np.load(ev.GOLDEN)
        _FIX["z"] = z
        _FIX["cfg"], _FIX["P"], _FIX["loaders"] = ev.val_loaders(z)
    return _FIX["z"], _FIX["cfg"], _FIX["P"], _FIX["loaders"]


def assert_margins(z):
    """the oracle's smallest top-2 margins on the first batch, 0.0227 (MLM, 13 rows) and 0.0027 (SAP, 3 rows), exceed twice the 3e-4
    the scores may be off: no row is left out of the count comparison"""
    sap = lambda i: np.where(np.isfinite(z[f"sap/logits/{i}"]), z[f"sap/logits/{i}"], -1e30)
    assert z["mlm/scores/0"].shape[0] == 13 and abs(ev.top2_margin(z["mlm/scores/0"]) - 0.0227) < 1e-4
    assert z["sap/logits/0"].shape[0] == 3 and abs(ev.top2_margin(sap(0)) - 0.0027) < 1e-4
    assert min(ev.top2_margin(z[f"mlm/scores/{i}"]) for i in range(2)) > 2 * 3e-4
    assert min(ev.top2_margin(sap(i)) for i in range(2)) > 2 * 3e-4


@pytest.mark.parametrize("dtype,atol", [(torch.float32, 3e-4), (torch.bfloat16, 1e-1)])
def test_mlm_eval_matches_its_scores_the_training_loss_and_the_oracle(dtype, atol):
    """atol: test_mlm_pretraining_step_matches_oracle's (tests/test_planner_gpu.py); its loss tolerance is 3 atol"""
    from etpnav_amd.pretrain import MlmStep
    from etpnav_amd.validate import EvalCounters
    z, cfg, P, loaders = fixture()
    model = build_model(cfg, P, dtype)
    counters = EvalCounters(DEV)
    for i, batch in enumerate(loaders["mlm"]):
        step = MlmStep(model, batch)
        counters.reset()
        step.run_eval(counters)
        sync()
        scores = step.scores().clone()
        nll, pred, labels = step.row_nll.clone(), step.row_pred.clone(), step.labels.clone()
        rec = counters.read_all()
        q = ev.tail(scores.cpu(), labels.cpu())
        ev.check_rows(f"etp_mlm_eval {dtype}", nll, pred, q, ev.vocab_depth(cfg.vocab_size))
        ev.check_record(f"etp_mlm_eval {dtype} record", rec, (0.0, 0, 0, 0), nll, pred, labels, -1)
        assert rec[2] == rec[3] == step.Nm == int(z[f"mlm/n_word/{i}"])
        # a second run: the same bits, rows and record
        counters.reset()
        step.run_eval(counters)
        sync()
        exact("etp_mlm_eval row_nll (second run)", step.row_nll.view(torch.int32), nll.view(torch.int32))
        exact("etp_mlm_eval row_pred (second run)", step.row_pred, pred)
        assert counters.read_all() == rec
        # the training forward on the same batch: the same logits, and its mean loss
        step.run_eager(backward=False)
        sync()
        exact("etp_mlm_fwd logits against etp_mlm_eval's", step.scores().contiguous().view(torch.int32), scores.contiguous().view(torch.int32))
        assert abs(float(nll.double().sum()) / step.Nm - step.loss.item()) < atol * 3
        if dtype == torch.float32:
            ref = torch.from_numpy(z[f"mlm/scores/{i}"])
            assert float((scores.cpu() - ref).abs().max()) < atol
            assert_margins(z)
            assert rec[1] == int(z[f"mlm/n_correct/{i}"])
            assert abs(rec[0] - float(z[f"mlm/loss_sum/{i}"])) < atol * 3 * step.Nm
        step.close()


# ---- driver ---------------------------------------------------------------------------------------------------------------------------
def _driver(model, loaders, **kw):
    from etpnav_amd.pretrain import PretrainDriver
    g = torch.Generator().manual_seed(1)
    return PretrainDriver(model, {"mlm": (loaders["mlm"], 1, lambda e: None), "sap": (loaders["sap"], 1, lambda e: None)},
                          learning_rate=2e-4, warmup_steps=4, num_train_steps=40, dropout=None, generator=g, **kw)


def test_validate_gives_the_real_models_dicts_and_leaves_the_training_state_alone():
    z, cfg, P, loaders = fixture()
    assert_margins(z)
    model = build_model(cfg, P, torch.float32)
    drv = _driver(model, loaders)
    drv.train_step("sap", loaders["sap"][0])                    # a trained-on state: moments, gradients and a SAP step in the cache
    drv.train_step("mlm", loaders["mlm"][0])
    model.load_state_dict({k: v for k, v in P.items()}, strict=True)      # the weights the fixture was recorded with
    sync()
    eng = model._engine
    snap = lambda: [eng.params.clone(), eng.grads.clone(), drv.opt.exp_avg.clone(), drv.opt.exp_avg_sq.clone()]
    before, state = snap(), (drv.global_step, drv._micro, dict(drv._sap))
    cached = next(iter(drv._sap.values()))                      # the training cache's SAP step: inputs, outputs, stash
    held = lambda: [cached.logits.clone(), cached.dlogits.clone(), cached.loss.clone(), cached.gemb.clone(), cached.st_nav.clone()] + \
        [v.clone() for v in cached.inp.values()]
    held0 = held()
    log = drv.validate({"mlm": loaders["mlm"], "sap": loaders["sap"]}, setname="_seen")
    sync()
    assert sorted(log) == sorted(f"val_seen_{t}_{k}" for t, ks in (("mlm", ("loss", "acc", "tok_per_s")), ("sap", ("gloss", "gacc", "tok_per_s")))
                                 for k in ks)
    # loss within the step tolerances (3 x 3e-4 MLM, 3e-4 SAP: test_planner_gpu / the driver test), counts exact in fp32
    assert abs(log["val_seen_mlm_loss"] - float(z["mlm/loss"])) < 3 * 3e-4
    assert abs(log["val_seen_sap_gloss"] - float(z["sap/gloss"])) < 3e-4
    assert log["val_seen_mlm_acc"] == float(z["mlm/acc"]) and log["val_seen_sap_gacc"] == float(z["sap/gacc"])
    assert log["val_seen_mlm_tok_per_s"] > 0 and log["val_seen_sap_tok_per_s"] > 0
    for name, a, b in zip(("parameters", "gradient arena", "exp_avg", "exp_avg_sq"), snap(), before):
        exact("validate leaves " + name, a.view(torch.int32), b.view(torch.int32))
    assert (drv.global_step, drv._micro) == state[:2] == (2, 0)
    assert len(state[2]) == 1 and list(drv._sap) == list(state[2]) and all(drv._sap[k] is v for k, v in state[2].items())
    for k, (a, b) in enumerate(zip(held(), held0)):
        exact(f"validate leaves the cached training step (tensor {k})", a, b)
    assert len(drv._sap_eval) >= 1 and not set(map(id, drv._sap_eval.values())) & set(map(id, drv._sap.values()))
    with pytest.raises(ValueError):
        drv.validate({"mrc": []})
    drv.close()


def test_run_with_valid_steps_validates_at_the_references_points():
    z, cfg, P, loaders = fixture()
    model = build_model(cfg, P, torch.float32)
    drv = _driver(model, loaders)
    saved = []
    drv.run(3, valid_steps=2, val_loaders={"sap": loaders["sap"]}, val2_loaders={"mlm": loaders["mlm"][:1]}, on_checkpoint=saved.append)
    sync()
    assert saved == [2, 3] and [g for g, _ in drv.val_logs] == [2, 3]
    for _, log in drv.val_logs:
        assert sorted(log) == ["val_seen_sap_gacc", "val_seen_sap_gloss", "val_seen_sap_tok_per_s", "val_unseen_mlm_acc",
                               "val_unseen_mlm_loss", "val_unseen_mlm_tok_per_s"]
        assert all(np.isfinite(v) for v in log.values())
    drv.close()
