"""The training log of csrc/trainlog.hip through the C ABI and the host layer (etpnav_amd/trainlog.py, FusedAdamW(norm_route="report"),
PretrainDriver(log_steps=...)) -- with the restatements, derived bounds and case lists of tests/trainlog_ref.py
(tests/test_train_log_ref_cpu.py pins, emulates and mutates the same lists on the CPU).

  etp_train_meter_loss   the recorded calls of the REAL RunningMeter replayed: every double and every counter of every record after
                         every call bit for bit; mask counts exact at every shape; other tasks' records untouched
  etp_train_meter_step   every (sumsq, nonfinite) pair of the list, the record after every call bit for bit
  etp_tensor_report      absmax / nonfinite exact, |sum - ref| <= gam64(d) sum|x|, |sumsq - ref| <= gam64(d) sum x^2 against the correctly
                         rounded float64 of the exact values; the totals bit for bit stage 3's restatement over the included records;
                         a second run bit-identical; outputs start as payload NaN / 0xFF inside guards that must survive
"""
import ctypes
import math
import struct

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from etpnav_amd import _lib  # noqa: E402
from etpnav_amd._lib import check, ptr  # noqa: E402
from tests import move_ref as mv  # noqa: E402
from tests import trainlog_ref as tr  # noqa: E402

DEV = "cuda"
gptr, guarded, exact = mv.gptr, mv.guarded, mv.exact


def L():
    return _lib.lib()


def stream():
    return torch.cuda.current_stream().cuda_stream


def sync():
    torch.cuda.synchronize()


def records(n, fmt, rows):
    """n 64-byte records inside a guarded byte buffer, holding `rows` -> (Guarded, int64 view [n, 8])"""
    g = guarded((n * 64,), torch.uint8)
    raw = b"".join(struct.pack(fmt, *r) for r in rows)
    g.t.copy_(torch.frombuffer(bytearray(raw), dtype=torch.uint8))
    g.ref = g.buf.clone()
    return g, g.t.view(torch.int64).view(n, 8)


def unpack(fmt, row):
    return struct.unpack(fmt, row.cpu().numpy().tobytes())


def same(a, b):
    """two records bit for bit; two NaNs count as equal whatever their payload"""
    if len(a) != len(b):
        return False
    for x, y in zip(a, b):
        if isinstance(x, float) or isinstance(y, float):
            if not (math.isnan(x) and math.isnan(y)) and tr.bits64(x) != tr.bits64(y):
                return False
        elif int(x) != int(y):
            return False
    return True


# ---- etp_train_meter_loss ----------------------------------------------------------------------------------------------------------------
OTHER = (1.25, -3.5, 7, 1, 40, 400, 30, 0)          # a third task's record: must come back as it was


def test_meter_replays_the_recorded_running_meter_bit_for_bit():
    z = np.load(tr.GOLDEN)
    sm = float(z["meter/smooth"])
    g, rec = records(3, tr.TASK_FMT, [(0.0,) * 2 + (0,) * 6, (0.0,) * 2 + (0,) * 6, OTHER])
    ref = [tr.Meter(sm), tr.Meter(sm)]
    loss = torch.from_numpy(z["meter/loss"]).to(DEV)
    rng = np.random.RandomState(2)
    masks = torch.from_numpy((rng.rand(len(loss), 3, 9) < 0.6)).to(DEV)
    counts = masks.sum(dim=(1, 2)).tolist()
    snaps, want = [], []
    for i, t in enumerate(z["meter/task"].tolist()):
        check(L().etp_train_meter_loss(loss[i:i + 1].data_ptr(), sm, ptr(masks[i]), 27, 3, 3 + t * (i % 5), rec[t].data_ptr(), stream()),
              "train_meter_loss")
        snaps.append(rec.clone())
        ref[t](z["meter/loss"][i], 3, counts[i], 3 + t * (i % 5))
        want.append((ref[0].record(), ref[1].record()))
    host = torch.stack(snaps).cpu()                   # the one read
    g.check("meter records")
    for i in range(len(want)):
        for t in (0, 1):
            got = unpack(tr.TASK_FMT, host[i, t])
            assert same(got, want[i][t]), (i, t, got, want[i][t])
        assert unpack(tr.TASK_FMT, host[i, 2]) == OTHER, i
        t = int(z["meter/task"][i])                  # and the recording itself: the meter's _val after this call
        got = unpack(tr.TASK_FMT, host[i, t])
        assert (got[2] > 0) == bool(z["meter/has"][i]) and (not got[2] or tr.bits64(got[0]) == tr.bits64(z["meter/val"][i])), i
    assert sum(r[3] for r in want[-1]) == 3


@pytest.mark.parametrize("B,Lt", tr.MASK_SHAPES)
def test_meter_counts_the_mask_bytes_exactly(B, Lt):
    rng = np.random.RandomState(B * 1000 + Lt)
    rnd = rng.randint(0, 2, (B, Lt)).astype(np.uint8) * rng.choice(np.array([1, 2, 255], dtype=np.uint8), (B, Lt))
    loss = torch.tensor([0.5], device=DEV)
    g, rec = records(2, tr.TASK_FMT, [OTHER, OTHER])
    total = OTHER[5]
    for pat in (np.zeros((B, Lt), np.uint8), np.ones((B, Lt), np.uint8), rnd):
        m = guarded((B * Lt,), torch.uint8, init=torch.from_numpy(pat.reshape(-1)).to(DEV))
        check(L().etp_train_meter_loss(ptr(loss), 0.99, gptr(m), B * Lt, B, B, rec[0].data_ptr(), stream()), "train_meter_loss")
        sync()
        m.intact("txt_masks (read only)")
        total += int((pat != 0).sum())
        assert unpack(tr.TASK_FMT, rec[0])[5] == total, (B, Lt)
    g.check("meter records")
    got = unpack(tr.TASK_FMT, rec[0])
    assert got[4] == OTHER[4] + 3 * B and got[6] == OTHER[6] + 3 * B and got[2] == OTHER[2] + 3 and got[1] == 0.5
    assert unpack(tr.TASK_FMT, rec[1]) == OTHER
    # n_mask_bytes = 0 reads nothing
    check(L().etp_train_meter_loss(ptr(loss), 0.99, gptr(m), 0, 0, 0, rec[1].data_ptr(), stream()), "train_meter_loss")
    sync()
    assert unpack(tr.TASK_FMT, rec[1])[4:7] == OTHER[4:7]


# ---- etp_train_meter_step ----------------------------------------------------------------------------------------------------------------
def test_step_record_over_every_sumsq_and_nonfinite_of_the_list():
    g, rec = records(2, tr.STEP_FMT, [tr.STEP_START, (9.0, 9.0, 9.0, 1, 0, -1, 0, 0)])
    cases = [(s, nf) for nf in tr.NONFINITE_CASES for s in tr.SUMSQ_CASES] + [(3.0, 0), (16777218.0, None), (1e-45, 0)]
    ss = torch.tensor([c[0] for c in cases], dtype=torch.float32, device=DEV)
    bad = torch.tensor([c[1] or 0 for c in cases], dtype=torch.int32, device=DEV)
    snaps, want, r = [], [], tr.STEP_START
    for i, (s, nf) in enumerate(cases):
        check(L().etp_train_meter_step(ss[i:i + 1].data_ptr(), None if nf is None else bad[i:i + 1].data_ptr(), rec[0].data_ptr(),
                                       stream()), "train_meter_step")
        snaps.append(rec.clone())
        r = tr.step_record(r, s, nf)
        want.append(r)
    host = torch.stack(snaps).cpu()
    g.check("step records")
    for i in range(len(cases)):
        got = unpack(tr.STEP_FMT, host[i, 0])
        assert same(got, want[i]), (cases[i], got, want[i])
        assert unpack(tr.STEP_FMT, host[i, 1]) == (9.0, 9.0, 9.0, 1, 0, -1, 0, 0)
    assert want[0][0] == 0.0 and want[3][0] == float(np.sqrt(np.float32(1e-38))) and want[-1][4] >= 9 and want[-1][5] == 6


# ---- etp_tensor_report -------------------------------------------------------------------------------------------------------------------
_CASE = {}


def case(t):
    """table t with its arena and its reference: computed once, shared, left unchanged"""
    if t not in _CASE:
        arena, off, lens, include = tr.report_case(t)
        _CASE[t] = (arena, off, lens, include, tr.report_ref(arena, off, lens))
    return _CASE[t]


def make_plan(off, lens, include, arena_len):
    n = len(off)
    plan = ctypes.c_void_p()
    check(L().etp_tensor_report_create((ctypes.c_int64 * n)(*off), (ctypes.c_int64 * n)(*lens),
                                       (ctypes.c_uint8 * n)(*include) if include is not None else None, n, arena_len, ctypes.byref(plan)),
          "tensor_report_create")
    return plan


def report_outputs(n_seg):
    recs = guarded((n_seg * 32,), torch.uint8)
    bad = guarded((4,), torch.uint8)
    return recs, guarded((1,)), bad


def unpack_records(recs, n_seg):
    b = recs.t.cpu().numpy().tobytes()
    return [struct.unpack_from(tr.TENSOR_FMT, b, 32 * s) for s in range(n_seg)]


@pytest.mark.parametrize("t", range(len(tr.N_SEGS)), ids=[f"nseg{n}" for n in tr.N_SEGS])
def test_tensor_report_tables(t):
    arena_np, off, lens, include, ref = case(t)
    tr.assert_gaps_would_show(arena_np, off, lens, ref)
    n_seg = len(off)
    arena = torch.from_numpy(arena_np).to(DEV)
    arena0 = arena.clone()
    plan = make_plan(off, lens, include, arena.numel())
    try:
        assert L().etp_tensor_report_chunks(plan) == tr.total_chunks(lens)
        runs = []
        for _ in range(2):
            recs, ss, bad = report_outputs(n_seg)
            check(L().etp_tensor_report(plan, ptr(arena), gptr(recs), gptr(ss), gptr(bad), stream()), "tensor_report")
            sync()
            for g, name in ((recs, "records"), (ss, "sumsq"), (bad, "nonfinite")):
                g.check("tensor_report " + name)
            runs.append((recs.t.clone(), ss.t.clone(), bad.t.clone()))
        for a, b, name in zip(runs[0], runs[1], ("records", "sumsq", "nonfinite")):
            exact(f"tensor_report {name} (second run)", a.view(torch.uint8), b.view(torch.uint8))
        exact("tensor_report arena (read only)", arena.view(torch.int32), arena0.view(torch.int32))
        got = unpack_records(recs, n_seg)
        assert all(r[4] == 0 for r in got)
        worst = tr.check_report(f"etp_tensor_report table {t}", [(r[0], r[1], r[2], r[3]) for r in got], ref, lens)
        print(f"\ntable {t}: {n_seg} segments, {tr.total_chunks(lens)} chunks, worst err / bound {worst:.4f}")
        # the totals: stage 3 in its own order over the included records, bit for bit
        tot, nf = tr.totals_ref([r[1] for r in got], [r[3] for r in got], include)
        got_tot, got_nf = float(ss.t.cpu()[0]), int(bad.t.view(torch.int32).cpu()[0])
        assert got_nf == nf == sum(r[3] for r, inc in zip(ref, include) if inc)
        assert (math.isnan(tot) and math.isnan(got_tot)) or struct.pack("<f", tot) == struct.pack("<f", got_tot), (tot, got_tot)
        if t == 1:                                  # the excluded long segment is far larger than the included one
            assert got_tot == float(np.float32(got[1][1])) and got[0][1] > 1e6 * got[1][1]
        # without the totals: the same records, and the pair is left alone
        recs2, ss2, bad2 = report_outputs(n_seg)
        check(L().etp_tensor_report(plan, ptr(arena), gptr(recs2), None, None, stream()), "tensor_report")
        check(L().etp_tensor_report(plan, ptr(arena), gptr(recs2), gptr(ss2), None, stream()), "tensor_report")
        sync()
        exact("tensor_report records (no totals)", recs2.t, recs.t)
        exact("tensor_report sumsq alone", ss2.t.view(torch.int32), ss.t.view(torch.int32))
        bad2.intact("tensor_report nonfinite (not asked for)")
    finally:
        sync()
        L().etp_tensor_report_destroy(plan)


def test_refused_calls_leave_the_outputs_as_they_were():
    recs, ss, bad = report_outputs(2)
    g, rec = records(1, tr.TASK_FMT, [OTHER])
    arena = torch.zeros(128, device=DEV)
    loss = torch.zeros(1, device=DEV)
    mask = torch.ones(8, dtype=torch.uint8, device=DEV)
    plan = make_plan([0, 64], [8, 8], None, 128)
    X, s = L(), stream()
    try:
        calls = [X.etp_tensor_report(plan, arena.data_ptr() + 4, gptr(recs), gptr(ss), gptr(bad), s),
                 X.etp_tensor_report(plan, None, gptr(recs), gptr(ss), gptr(bad), s),
                 X.etp_tensor_report(None, ptr(arena), gptr(recs), gptr(ss), gptr(bad), s),
                 X.etp_tensor_report(plan, ptr(arena), gptr(recs) + 4, gptr(ss), gptr(bad), s),
                 X.etp_train_meter_loss(ptr(loss), 1.0, ptr(mask), 8, 1, 1, rec[0].data_ptr(), s),
                 X.etp_train_meter_loss(ptr(loss), 0.99, ptr(mask), -1, 1, 1, rec[0].data_ptr(), s),
                 X.etp_train_meter_loss(ptr(loss), 0.99, None, 8, 1, 1, rec[0].data_ptr(), s),
                 X.etp_train_meter_step(None, None, rec[0].data_ptr(), s),
                 X.etp_train_meter_step(ptr(loss), None, rec[0].data_ptr() + 4, s)]
        sync()
        assert calls == [-1] * len(calls), calls
        for x, name in ((recs, "records"), (ss, "sumsq"), (bad, "nonfinite"), (g, "task record")):
            x.intact("refused: " + name)
    finally:
        X.etp_tensor_report_destroy(plan)


# ---- on a real step: the planner's gradient and parameter arenas -------------------------------------------------------------------------
def numpy_depth(n):
    """numpy's pairwise float64 sum: 8 accumulators over blocks of 128 (16 additions each, 3 to combine them), halving above, up to
    7 sequential additions for a remainder -- the reference's own chain on this test's large tensors"""
    return 27 + max(0, math.ceil(math.log2(max(n, 128) / 128)))


def check_against_numpy(name, rep, table, arena):
    """rep: TensorReport.read() of `arena` (a host float32 array): per table entry against numpy float64, the bound widened by the
    reference's own error"""
    from etpnav_amd.trainlog import table_segments
    names, off, lens = table_segments(table)
    assert list(rep) == [row[0] for row in table]
    for nm, o, n in zip(names, off, lens):
        x = arena[o:o + n]
        v = x.astype(np.float64)
        sm, amax, l2, nf = rep[nm]
        assert nf == 0 and bool(np.isfinite(x).all()), nm
        assert np.float32(amax) == np.abs(x).max(), nm
        k = tr.gam64(tr.depth(n)) + tr.gam64(numpy_depth(n))
        assert abs(sm - v.sum()) <= k * np.abs(v).sum(), (name, nm, sm, v.sum())
        sq = (v * v).sum()
        assert abs(l2 * l2 - sq) <= (k + 4 * tr.U64) * sq, (name, nm, l2 * l2, sq)      # sqrt and its square: 2u + u relative


def test_report_on_a_real_steps_gradient_and_parameter_arenas():
    from etpnav_amd.planner import GlocalTextPathNavCMT
    from etpnav_amd.step import PlannerStep
    from etpnav_amd.trainlog import TensorReport
    from oracle import planner_oracle as po
    from tests.golden_util import CASES, make_cfg
    cfg = make_cfg(**CASES["c1_single_episode"][0])
    batch = po.make_batch(cfg, seed=1234, B=4, L=33, V=19, G=10, ragged=True)
    model = GlocalTextPathNavCMT(cfg.to_dict(), dtype=torch.bfloat16, device=DEV)
    model.load_state_dict(po.init_params(cfg, seed=0), strict=True)
    step = PlannerStep(model, batch)
    step.run_eager()
    eng = model._engine
    rep = TensorReport(eng.table, eng.total, DEV)
    rep.run(eng.grads)
    grads = rep.read()
    total = float(rep.sumsq.item())
    rep.run(eng.params)
    params = rep.read()
    assert rep.first_nonfinite() is None and int(rep.nonfinite.item()) == 0
    g, p = eng.grads.cpu().numpy(), eng.params.cpu().numpy()
    check_against_numpy("gradient arena", grads, eng.table, g)
    check_against_numpy("parameter arena", params, eng.table, p)
    want = sum(r[2] ** 2 for r in grads.values())
    assert abs(total - want) <= 1e-6 * want and total > 0
    step.close()
    rep.close()


# ---- FusedAdamW(norm_route="report") -----------------------------------------------------------------------------------------------------
def close(a, b, atol=2e-6, rtol=1e-5):
    """tests/test_optim_gpu.py's tolerance"""
    a, b = a.float().cpu(), b.float().cpu()
    return bool(((a - b).abs() <= atol + rtol * b.abs()).all())


def optimizer_run(route, P, cfg, batch, freeze=()):
    """three optimizer steps on gradients of a real planner step, each held to the oracle; clipping is active at step 2 only (max_norm =
    half that step's norm, twice it otherwise) -> (sumsq bits per step, the optimizer, the model)"""
    from etpnav_amd.optim import FusedAdamW
    from etpnav_amd.planner import GlocalTextPathNavCMT
    from etpnav_amd.step import PlannerStep
    from oracle import optim_oracle as oo
    model = GlocalTextPathNavCMT(cfg.to_dict(), dtype=torch.bfloat16, device=DEV)
    model.load_state_dict(P, strict=True)
    for name, p in model.named_parameters():
        if name in freeze:
            p.requires_grad_(False)
    opt = FusedAdamW(model, lr=1e-3, hf_style=True, betas=(0.9, 0.98), eps=1e-6, weight_decay=0.01, max_grad_norm=5.0,
                     no_decay=FusedAdamW.reference_no_decay, norm_route=route)
    eng = model._engine
    step = PlannerStep(model, batch)
    p_ref = eng.params.detach().cpu().clone()
    m_ref, v_ref = torch.zeros_like(p_ref), torch.zeros_like(p_ref)
    wd = torch.full_like(p_ref, 0.01)
    for name, shape, off in eng.table:
        if FusedAdamW.reference_no_decay(name):
            wd[off:off + int(np.prod(shape))] = 0.0
    bits = []
    for t in (1, 2, 3):
        step.run_eager()
        sync()
        g = eng.grads.detach().cpu().clone()
        for name, shape, off in eng.table:
            if name in freeze:
                g[off:off + int(np.prod(shape))] = 0.0           # no .grad in the reference: not in the norm, not updated
        norm = float(g.double().norm())
        opt.max_grad_norm = 0.5 * norm if t == 2 else 2.0 * norm
        if route == "report":                                       # the norm pass twice over the same gradients: the same bits
            twice = []
            for _ in range(2):
                opt.sumsq.fill_(-1.0)
                opt._sqnorm(stream())
                twice.append(int(opt.sumsq.view(torch.int32).item()))
            assert twice[0] == twice[1] and opt.sumsq.item() > 0, twice
        frozen_before = {n: eng.params[o:o + int(np.prod(s))].clone() for n, s, o in eng.table if n in freeze}
        opt.step()
        sync()
        bits.append(int(opt.sumsq.view(torch.int32).item()))
        # the report: float64 sums rounded once to fp32; the atomic scan: fp32 sums of 4 * 256 * 8 strided lanes and 2048 atomics
        assert abs(float(opt.sumsq.item()) - norm * norm) <= (1e-6 if route == "report" else 1e-4) * norm * norm, (route, t)
        p_new = p_ref.clone()
        oo.adamw_step(p_new, g, m_ref, v_ref, t, 1e-3, 0.9, 0.98, 1e-6, wd, True, True, 1.0, opt.max_grad_norm)
        for name, shape, off in eng.table:                         # frozen: left alone
            if name in freeze:
                n = int(np.prod(shape))
                p_new[off:off + n] = p_ref[off:off + n]
                assert torch.equal(eng.params[off:off + n], frozen_before[name])
        p_ref = p_new
        assert close(eng.params, p_ref), (route, t)
    step.close()
    return bits, opt, model


def optimizer_case():
    from oracle import planner_oracle as po
    cfg = po.PlannerConfig.r2r(vocab_size=1024, num_l_layers=2, num_pano_layers=1, num_x_layers=1)     # tests/test_optim_gpu.py's sizes
    return cfg, po.init_params(cfg, seed=1), po.make_batch(cfg, B=2, L=12, V=9, G=6, seed=8, ragged=True)


def test_optimizer_report_route_against_the_atomic_route_and_the_oracle():
    cfg, P, batch = optimizer_case()
    a_bits, a_opt, _ = optimizer_run("atomic", P, cfg, batch)
    r_bits, r_opt, r_model = optimizer_run("report", P, cfg, batch)
    assert r_opt._report is not None and a_opt._report is None
    # the report route's norm is the float64 of its records, rounded once
    rep = r_opt.grad_report()
    assert struct.unpack("<f", struct.pack("<i", r_bits[2]))[0] == pytest.approx(sum(r[2] ** 2 for r in rep.values()), rel=1e-6)
    assert r_opt.first_nonfinite() is None
    # a planted NaN is named
    eng = r_model._engine
    names = [n for n, _, _ in eng.table]
    name, shape, off = eng.table[len(names) // 2]
    eng.grads[off + 3] = float("nan")
    r_opt.step()
    sync()
    assert r_opt.first_nonfinite() == name and r_opt.grad_report()[name][3] == 1
    assert int(r_opt.nonfinite.item()) == 1 and math.isnan(float(r_opt.sumsq.item()))
    assert sum(r[3] for r in r_opt.grad_report().values()) == 1


def test_optimizer_report_route_gives_the_same_bits_twice_and_leaves_frozen_names_out():
    cfg, P, batch = optimizer_case()
    freeze = ("embeddings.word_embeddings.weight",)
    _, opt, model = optimizer_run("report", P, cfg, batch, freeze)
    assert list(freeze) == opt.frozen_names and not all(opt._report.included)
    eng = model._engine
    # garbage in the frozen tensor's gradient, a NaN included: named by its record, kept out of the totals
    name, shape, off = next(r for r in eng.table if r[0] == freeze[0])
    eng.grads[off:off + 64] = 1e30
    eng.grads[off + 64] = float("nan")
    opt._sqnorm(stream())
    sync()
    rec = opt.grad_report()
    assert rec[name][3] == 1 and rec[name][1] == float(np.float32(1e30))
    assert int(opt.nonfinite.item()) == 0 and math.isfinite(float(opt.sumsq.item()))
    want = sum(r[2] ** 2 for n, r in rec.items() if n != name)
    assert float(opt.sumsq.item()) == pytest.approx(want, rel=1e-6)


# ---- PretrainDriver(log_steps=...) -------------------------------------------------------------------------------------------------------
def driver_run(log_steps, collect=None, box=None):
    from etpnav_amd.planner import GlocalTextPathNavCMT
    from etpnav_amd.pretrain import PretrainDriver
    from tests import eval_ref as ev
    cfg, P, loaders = ev.val_loaders()
    model = GlocalTextPathNavCMT(cfg.to_dict(), dtype=torch.float32, device=DEV)
    model.load_state_dict({k: v for k, v in P.items()}, strict=True)
    g = torch.Generator().manual_seed(1)
    drv = PretrainDriver(model, {"mlm": (loaders["mlm"], 1, lambda e: None), "sap": (loaders["sap"], 1, lambda e: None)},
                         learning_rate=2e-4, warmup_steps=4, num_train_steps=40, accum_steps=2, seed=5, generator=g,
                         log_steps=log_steps, on_log=collect)
    if box is not None:
        box.append(drv)
    out = drv.run(6)
    sync()
    return drv, out, loaders


def test_driver_logs_the_references_scalars_every_log_steps():
    seen, box = [], []
    drv, out, loaders = driver_run(2, lambda step, log: seen.append((step, dict(log), box[0].opt.sumsq.clone())), box)
    assert drv.task_losses == {} and drv.meter is not None
    assert [s for s, _, _ in seen] == [2, 4, 6] == [s for s, _ in drv.train_logs] and len(out) == 12
    # the values the meter was fed: train_step's returns of the logged run itself, read after the run.  (A second, identically seeded
    # run does NOT give the same bits: the loss tails add their rows with one float atomic per row, in any order -- tests/move_ref.py,
    # vocab_ce -- so two runs differ in the last fp32 bit of a loss from the first window on.  Measured: one fp32 ulp at micro-step 2.)
    items = [(name, float(t.item())) for name, t in out]
    # the second, identically seeded run without logging: the same task sequence, task_losses grows as before and holds what
    # train_step returned; before the first parameter update its losses are the logged run's up to the order of that row sum:
    # gam32(n + 1) relative on positive terms, n <= 4 * 33 rows
    drv2, out2, _ = driver_run(None)
    assert drv2.meter is None and drv2.train_logs == [] and sum(len(v) for v in drv2.task_losses.values()) == 12
    items2 = [(name, float(t.item())) for name, t in out2]
    assert [n for n, _ in items2] == [n for n, _ in items]
    for (n, a), (_, b) in zip(items[:2], items2[:2]):
        assert abs(a - b) <= 134 * 2.0 ** -24 * abs(a), (n, a, b)
    for name in ("mlm", "sap"):
        assert [float(t.item()) for t in drv2.task_losses[name]] == [v for n, v in items2 if n == name]
    # every logged loss/{task}: a Python RunningMeter fed those values
    meters = {"mlm": tr.Meter(0.99), "sap": tr.Meter(0.99)}
    counts = {n: [0, 0, 0] for n in meters}
    taken = {n: 0 for n in meters}
    logs = {s: log for s, log, _ in seen}
    for i, (name, v) in enumerate(items):
        meters[name](v)
        b = loaders[name][taken[name] % len(loaders[name])]
        taken[name] += 1
        B = b["txt_ids"].shape[0]
        counts[name][0] += B
        counts[name][1] += int(b["txt_masks"].sum())
        counts[name][2] += B if name == "sap" else int((b["txt_labels"] != -1).sum())
        if (i + 1) % 4 == 0:                                          # accum_steps 2, log_steps 2
            log = logs[(i + 1) // 2]
            for n, m in meters.items():
                assert tr.bits64(log[f"loss/{n}"]) == tr.bits64(m.val), (i, n, log[f"loss/{n}"], m.val)
    tasks, step = drv.meter.read_raw()
    for n, r in zip(drv.meter.names, tasks):
        assert list(r[4:7]) == counts[n] and r[2] + r[3] == taken[n] and r[3] == 0, (n, r, counts[n])
    assert step[3] == 6 and step[4] == 0 and step[5] == -1
    for s, log, sumsq in seen:
        assert log["grad_norm"] == tr.f32_root(float(sumsq.item())) and log["grad_norm"] > 0
        assert log["lr"] == drv.lr_history[s - 1] and log["nonfinite_steps"] == 0 and log["first_nonfinite_step"] == -1
        assert log["skipped_losses"] == 0
        for n in ("mlm", "sap"):
            for k in ("ex", "in", "loss"):
                assert isinstance(log[f"perf/{n}_{k}_per_s"], int) and log[f"perf/{n}_{k}_per_s"] >= 0
    assert sorted(seen[0][1]) == sorted(["loss/mlm", "loss/sap", "grad_norm", "lr", "skipped_losses", "nonfinite_steps",
                                         "first_nonfinite_step"] + [f"perf/{n}_{k}_per_s" for n in ("mlm", "sap") for k in ("ex", "in", "loss")])
    drv.close()
    drv2.close()
