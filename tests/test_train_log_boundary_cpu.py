"""CPU-side checks of the training log's boundary (in the style of tests/test_eval_boundary_cpu.py): the entry points of
csrc/trainlog.hip are declared and exported with the header's citations, every refusal the header lists comes back as
ETP_ERR_INVALID without a GPU (nothing is launched: the operands are addresses that are never read), the plan's launch geometry equals
the restated one for every table of the GPU list, the host layer fails loudly where a launch is needed, the driver has no meter unless
asked, and the build compiles the file under the row kernels' flags."""
import ctypes
import struct

import pytest
import torch

from etpnav_amd import _lib, build, trainlog
from tests import trainlog_ref as tr

P = 0x10000          # an aligned address; never dereferenced by a refused call
LOSS_ARGS = ["loss", "smooth", "txt_masks", "n_mask_bytes", "n_examples", "n_loss_units", "rec"]
STEP_ARGS = ["sumsq", "nonfinite", "rec"]
SCALARS = dict(smooth=0.99, n_mask_bytes=12, n_examples=3, n_loss_units=3)


def call(name, args, **kw):
    a = {k: P for k in args}
    a.update({k: v for k, v in SCALARS.items() if k in args})
    a.update(kw)
    return getattr(_lib.lib(), name)(*[a[k] for k in args], None)


def test_symbols_records_and_citations():
    protos = _lib.parse_header()
    for name, nargs in (("etp_train_meter_loss", 8), ("etp_train_meter_step", 4), ("etp_tensor_report_create", 6),
                        ("etp_tensor_report_chunks", 1), ("etp_tensor_report", 6), ("etp_tensor_report_destroy", 1)):
        assert name in _lib.declared_symbols() and hasattr(_lib.lib(), name) and len(protos[name][1]) == nargs, name
    assert protos["etp_train_meter_loss"][1][1] is ctypes.c_double and protos["etp_tensor_report_chunks"][0] is ctypes.c_int64
    hdr = open(_lib.HEADER).read()
    for s in ("} etp_train_task_record;", "} etp_train_step_record;", "} etp_tensor_record;", "#define ETP_TENSOR_REPORT_CHUNK 16384"):
        assert s in hdr, s
    assert (trainlog.TASK_RECORD_BYTES, trainlog.STEP_RECORD_BYTES, trainlog.TENSOR_RECORD_BYTES) == (64, 64, 32)
    assert [struct.calcsize(f) for f in (trainlog.TASK_FMT, trainlog.STEP_FMT, trainlog.TENSOR_FMT)] == [64, 64, 32]
    assert (trainlog.TASK_FMT, trainlog.STEP_FMT, trainlog.TENSOR_FMT, trainlog.CHUNK) == (tr.TASK_FMT, tr.STEP_FMT, tr.TENSOR_FMT, tr.CHUNK)
    doc = hdr[hdr.index("Pre-training log"):hdr.index("int etp_tensor_report_destroy")]
    for cite in ("train_r2r.py:229-317", "utils/logger.py:68-94", "train_r2r.py:259", "train_r2r.py:233-234", "train_r2r.py:282-284",
                 "train_r2r.py:286-289", "oracle/make_golden.py:69-73", "no atomics"):
        assert cite in doc, cite


LOSS_REFUSALS = {"NULL loss": dict(loss=None), "NULL txt_masks": dict(txt_masks=None), "NULL rec": dict(rec=None),
                 "smooth 1": dict(smooth=1.0), "smooth -0.01": dict(smooth=-0.01), "smooth nan": dict(smooth=float("nan")),
                 "smooth 1.5": dict(smooth=1.5), "n_mask_bytes -1": dict(n_mask_bytes=-1), "n_examples -1": dict(n_examples=-1),
                 "n_loss_units -1": dict(n_loss_units=-1), "rec off by 4": dict(rec=P + 4), "loss off by 2": dict(loss=P + 2)}
STEP_REFUSALS = {"NULL sumsq": dict(sumsq=None), "NULL rec": dict(rec=None), "rec off by 4": dict(rec=P + 4),
                 "sumsq off by 1": dict(sumsq=P + 1), "nonfinite off by 2": dict(nonfinite=P + 2)}


@pytest.mark.parametrize("name", list(LOSS_REFUSALS))
def test_meter_loss_refusals_come_back_before_anything_is_launched(name):
    assert call("etp_train_meter_loss", LOSS_ARGS, **LOSS_REFUSALS[name]) == -1, name
    assert b"train_meter_loss" in _lib.lib().etp_last_error()


@pytest.mark.parametrize("name", list(STEP_REFUSALS))
def test_meter_step_refusals_come_back_before_anything_is_launched(name):
    assert call("etp_train_meter_step", STEP_ARGS, **STEP_REFUSALS[name]) == -1, name
    assert b"train_meter_step" in _lib.lib().etp_last_error()


def create(off, lens, include=None, arena_len=None, n_seg=None, out=True):
    n = len(off)
    plan = ctypes.c_void_p()
    rc = _lib.lib().etp_tensor_report_create((ctypes.c_int64 * n)(*off) if off is not None else None,
                                             (ctypes.c_int64 * n)(*lens) if lens is not None else None,
                                             (ctypes.c_uint8 * n)(*include) if include is not None else None,
                                             n if n_seg is None else n_seg, tr.arena_len(off, lens) if arena_len is None else arena_len,
                                             ctypes.byref(plan) if out else None)
    return rc, plan


TABLE_REFUSALS = {"n_seg 0": dict(n_seg=0), "n_seg -3": dict(n_seg=-3), "NULL plan": dict(out=False), "arena_len 0": dict(arena_len=0),
                  "offset not a multiple of 4": dict(off=[0, 66]), "negative offset": dict(off=[-4, 64]), "length 0": dict(lens=[8, 0]),
                  "length -1": dict(lens=[-1, 8]), "overlap": dict(off=[0, 4], lens=[8, 8]), "descending": dict(off=[64, 0]),
                  "ends behind the arena": dict(arena_len=71), "offset behind the arena": dict(off=[0, 2 ** 40])}


@pytest.mark.parametrize("name", list(TABLE_REFUSALS))
def test_report_create_refuses_every_violated_table_rule(name):
    kw = dict(off=[0, 64], lens=[8, 8], arena_len=72)
    kw.update(TABLE_REFUSALS[name])
    rc, plan = create(**kw)
    assert rc == -1 and not plan.value, name
    assert b"tensor_report_create" in _lib.lib().etp_last_error()


def test_report_create_refuses_null_tables_and_report_refuses_bad_operands():
    L = _lib.lib()
    plan = ctypes.c_void_p()
    a = (ctypes.c_int64 * 1)(0)
    b = (ctypes.c_int64 * 1)(8)
    assert L.etp_tensor_report_create(None, b, None, 1, 8, ctypes.byref(plan)) == -1
    assert L.etp_tensor_report_create(a, None, None, 1, 8, ctypes.byref(plan)) == -1
    rc, plan = create([0, 64], [8, 8], arena_len=72)          # the table exactly fills the arena: accepted, no device needed
    assert rc == 0 and plan.value
    try:
        assert L.etp_tensor_report_chunks(plan) == 2 and L.etp_tensor_report_chunks(None) == -1
        for kw in (dict(plan=None), dict(arena=None), dict(rec=None), dict(arena=P + 4), dict(arena=P + 8), dict(rec=P + 4),
                   dict(sumsq=P + 2), dict(bad=P + 1)):
            args = dict(plan=plan, arena=P, rec=P, sumsq=P, bad=P)
            args.update(kw)
            assert L.etp_tensor_report(args["plan"], args["arena"], args["rec"], args["sumsq"], args["bad"], None) == -1, kw
            assert b"tensor_report" in L.etp_last_error()
    finally:
        assert L.etp_tensor_report_destroy(plan) == 0
    assert L.etp_tensor_report_destroy(None) == 0


@pytest.mark.parametrize("t", range(len(tr.N_SEGS)))
def test_the_plans_geometry_equals_the_restated_one(t):
    off, lens, include = tr.report_tables()[t]
    rc, plan = create(off, lens, include)
    assert rc == 0, _lib.lib().etp_last_error()
    try:
        assert _lib.lib().etp_tensor_report_chunks(plan) == tr.total_chunks(lens)
    finally:
        _lib.lib().etp_tensor_report_destroy(plan)
    for n in tr.LENS:                                          # one segment alone, every length of the list
        rc, plan = create([4], [n])
        assert rc == 0 and _lib.lib().etp_tensor_report_chunks(plan) == tr.seg_chunks(n)
        _lib.lib().etp_tensor_report_destroy(plan)


def test_table_segments_follow_the_engines_table():
    names, off, lens = trainlog.table_segments([("b", (3, 5), 64), ("a", (7,), 0), ("c", (2, 2, 2), 128)])
    assert (names, off, lens) == (["a", "b", "c"], [0, 64, 128], [7, 15, 8])


@pytest.mark.skipif(torch.cuda.is_available(), reason="CPU-only check")
def test_host_layer_fails_loudly_without_gpu():
    with pytest.raises(_lib.EtpError):
        trainlog.TrainMeter(["mlm", "sap"], "cpu")
    with pytest.raises(_lib.EtpError):
        trainlog.TrainMeter(["mlm", "sap"])
    with pytest.raises(_lib.EtpError):
        trainlog.TensorReport([("a", (7,), 0)], 8, "cpu")
    with pytest.raises(_lib.EtpError):
        trainlog.TensorReport([("a", (7,), 0)], 8)
    from etpnav_amd.optim import FusedAdamW
    model = _cpu_model()
    with pytest.raises(_lib.EtpError):                         # no quiet fall-back to the atomic route
        FusedAdamW(model, norm_route="report")
    with pytest.raises(ValueError):
        FusedAdamW(model, norm_route="host")
    opt = FusedAdamW(model)
    assert opt.norm_route == "atomic" and opt._report is None
    with pytest.raises(_lib.EtpError):
        opt.grad_report()


def _cpu_model():
    from etpnav_amd.planner import GlocalTextPathNavCMT, default_config
    return GlocalTextPathNavCMT(default_config(use_lang2visn_attn=True, vocab_size=64, num_l_layers=1, num_pano_layers=1, num_x_layers=1),
                                device="cpu")


def test_the_driver_has_no_meter_unless_asked():
    from etpnav_amd.pretrain import PretrainDriver
    model = _cpu_model()
    drv = PretrainDriver(model, {"mlm": [], "sap": []})
    assert drv.meter is None and drv.log_steps is None and drv.on_log is None and drv.train_logs == [] and drv.task_losses == {}
    assert drv.opt.norm_route == "atomic" and drv.opt.check_finite is False
    with pytest.raises(ValueError):
        PretrainDriver(model, {"mlm": []}, log_steps=0)
    if not torch.cuda.is_available():
        with pytest.raises(_lib.EtpError):                     # a meter lives on the device
            PretrainDriver(model, {"mlm": []}, log_steps=2)


def test_build_lists_the_file_with_its_flags_and_the_source_has_no_atomics():
    assert "trainlog.hip" in build.SOURCES and "trainlog.hip" in build.NO_PACKED_FP32
    assert "-fno-slp-vectorize" in build.PER_SOURCE_FLAGS["trainlog.hip"] and "-ffp-contract=off" in build.PER_SOURCE_FLAGS["trainlog.hip"]
    src = open(build.CSRC + "/trainlog.hip").read()
    code = "\n".join(line.split("//")[0] for line in src.splitlines())
    assert "atomic" not in code and "__shared__" in code
