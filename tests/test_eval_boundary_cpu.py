"""CPU-side checks of the validation boundary (in the style of tests/test_pano_store_boundary_cpu.py): the entry points of
csrc/eval_tail.hip and the two MLM validation entries are declared and exported, every refusal their header comments list comes back
as ETP_ERR_INVALID without a GPU (nothing is launched: the operands are addresses that are never read), the host layer fails loudly
where a launch is needed, PretrainDriver.run validates at the reference's points (train_r2r.py:319-332), and the build compiles the
file under the row kernels' flags."""
import ctypes

import pytest
import torch

from etpnav_amd import _lib, build, validate
from etpnav_amd.planner import default_config, make_c_config
from etpnav_amd.pretrain import PretrainDriver

P = 0x10000          # an aligned address; never dereferenced by a refused call
VOCAB_ARGS = ["logits", "labels", "Nm", "V", "ldv", "row_nll", "row_pred"]
SAP_ARGS = ["logits", "labels", "B", "G", "ignore_index", "row_nll", "row_pred"]
ACCUM_ARGS = ["row_nll", "row_pred", "labels", "n", "ignore_index", "acc"]
MLM_ARGS = ["txt", "txt_masks", "step_ids", "img", "pos", "gmask", "sel_ptr", "sel_idx", "sel_w", "labels", "B", "L", "G", "Nm", "stash",
            "row_nll", "row_pred", "acc"]
SCALARS = dict(Nm=5, V=100, ldv=104, B=3, G=9, L=7, n=5, ignore_index=-100)


def call(name, args, head=(), **kw):
    a = {k: P for k in args}
    a.update({k: v for k, v in SCALARS.items() if k in args})
    a.update(kw)
    return getattr(_lib.lib(), name)(*head, *[a[k] for k in args], None)


def pointers(args):
    return [k for k in args if k not in SCALARS]


def test_symbols_record_and_citations():
    protos = _lib.parse_header()
    for name, nargs in (("etp_vocab_eval", 8), ("etp_sap_eval", 8), ("etp_eval_accum", 7), ("etp_mlm_eval", 20), ("etp_mlm_stash_logits", 7)):
        assert name in _lib.declared_symbols() and hasattr(_lib.lib(), name) and len(protos[name][1]) == nargs, name
    hdr = open(_lib.HEADER).read()
    assert "double loss_sum;" in hdr and "} etp_eval_record;" in hdr and validate.RECORD_BYTES == 32
    doc = hdr[hdr.index("Pre-training validation"):hdr.index("int etp_mlm_stash_logits")]
    for cite in ("train_r2r.py:335-444", "train_r2r.py:365-367", "train_r2r.py:424-427", "train_r2r.py:366-368", "train_r2r.py:362",
                 "no NaN in the logits"):
        assert cite in doc, cite


VOCAB_REFUSALS = dict({f"NULL {k}": {k: None} for k in pointers(VOCAB_ARGS)}, **{"V 0": dict(V=0), "V -1": dict(V=-1), "Nm 0": dict(Nm=0),
                      "ldv < V": dict(ldv=99)})
SAP_REFUSALS = dict({f"NULL {k}": {k: None} for k in pointers(SAP_ARGS)}, **{"B 0": dict(B=0), "G 0": dict(G=0), "B -2": dict(B=-2)})
ACCUM_REFUSALS = dict({f"NULL {k}": {k: None} for k in pointers(ACCUM_ARGS)}, **{"n 0": dict(n=0), "n -1": dict(n=-1),
                      "acc off by 4": dict(acc=P + 4), "acc off by 1": dict(acc=P + 1)})


@pytest.mark.parametrize("name", list(VOCAB_REFUSALS))
def test_vocab_eval_refusals_come_back_before_anything_is_launched(name):
    assert call("etp_vocab_eval", VOCAB_ARGS, **VOCAB_REFUSALS[name]) == -1, name
    assert b"vocab_eval" in _lib.lib().etp_last_error()


@pytest.mark.parametrize("name", list(SAP_REFUSALS))
def test_sap_eval_refusals_come_back_before_anything_is_launched(name):
    assert call("etp_sap_eval", SAP_ARGS, **SAP_REFUSALS[name]) == -1, name
    assert b"sap_eval" in _lib.lib().etp_last_error()


@pytest.mark.parametrize("name", list(ACCUM_REFUSALS))
def test_eval_accum_refusals_come_back_before_anything_is_launched(name):
    assert call("etp_eval_accum", ACCUM_ARGS, **ACCUM_REFUSALS[name]) == -1, name
    assert b"eval_accum" in _lib.lib().etp_last_error()


def _planner(lang2visn):
    L = _lib.lib()
    c = make_c_config(default_config(use_lang2visn_attn=lang2visn, vocab_size=2048), torch.float32)
    h = L.etp_planner_create(ctypes.byref(c))
    assert h, L.etp_last_error()
    assert L.etp_planner_bind(h, P, None, P) == 0        # fake arenas: a refused call reads neither
    return h


def test_mlm_eval_and_stash_logits_refusals():
    L = _lib.lib()
    off, ldv = ctypes.c_int64(-1), ctypes.c_int64(-1)
    q = lambda h, **kw: L.etp_mlm_stash_logits(h, kw.get("B", 3), kw.get("L", 7), kw.get("G", 9), kw.get("Nm", 5),
                                               kw.get("off", ctypes.byref(off)), kw.get("ldv", ctypes.byref(ldv)))
    h = _planner(False)
    try:
        assert call("etp_mlm_eval", MLM_ARGS, head=(h,)) == -1 and b"use_lang2visn" in L.etp_last_error()
        assert q(h) == -1 and b"use_lang2visn" in L.etp_last_error()
    finally:
        L.etp_planner_destroy(h)
    assert call("etp_mlm_eval", MLM_ARGS, head=(None,)) == -1
    assert q(None) == -1
    h = _planner(True)
    try:
        bad = dict({f"NULL {k}": {k: None} for k in pointers(MLM_ARGS)}, **{"B 0": dict(B=0), "L 0": dict(L=0), "G 0": dict(G=0),
                   "Nm 0": dict(Nm=0), "acc off by 4": dict(acc=P + 4)})
        for name, kw in bad.items():
            assert call("etp_mlm_eval", MLM_ARGS, head=(h,), **kw) == -1, name
            assert b"etp_mlm_eval" in L.etp_last_error(), name
        for kw in (dict(B=0), dict(L=0), dict(G=0), dict(Nm=0), dict(off=None), dict(ldv=None)):
            assert q(h, **kw) == -1, kw
        assert (off.value, ldv.value) == (-1, -1)
        # the query agrees with the size query: the logits end inside the stash, on a 256-byte granule, ldv = round_up(vocab, 8)
        L.etp_mlm_stash_bytes.restype = ctypes.c_int64
        assert q(h) == 0 and ldv.value == 2048 and off.value % 256 == 0
        assert off.value + 5 * ldv.value * 4 <= L.etp_mlm_stash_bytes(h, 3, 7, 9, 5) - 256
    finally:
        L.etp_planner_destroy(h)


@pytest.mark.skipif(torch.cuda.is_available(), reason="CPU-only check")
def test_host_layer_fails_loudly_without_gpu():
    with pytest.raises(_lib.EtpError):
        validate.EvalCounters("cpu")
    from etpnav_amd.planner import GlocalTextPathNavCMT
    from oracle.make_golden_pretrain import make_case
    cfg, _, batch = make_case()
    model = GlocalTextPathNavCMT(default_config(use_lang2visn_attn=True, vocab_size=cfg.vocab_size, num_l_layers=1, num_pano_layers=1,
                                                num_x_layers=1), device="cpu")
    from etpnav_amd.pretrain import MlmStep
    with pytest.raises(_lib.EtpError):                    # valid input gets as far as the missing GPU
        MlmStep(model, batch)


class _StubDriver(PretrainDriver):
    """run()'s own logic over a stubbed step and a stubbed validate"""

    def __init__(self, accum_steps=1):
        self.accum_steps, self._micro, self.global_step = accum_steps, 0, 0
        self.meta = iter(lambda: ("mlm", None), None)
        self.val_logs, self.calls = [], []

    def train_step(self, name, batch):
        self._micro += 1
        if self._micro == self.accum_steps:
            self._micro, self.global_step = 0, self.global_step + 1
        return self.global_step

    def validate(self, val_loaders, setname=""):
        self.calls.append((self.global_step, setname, val_loaders))
        return {f"val{setname}_x": float(self.global_step)}


@pytest.mark.parametrize("accum", [1, 3])
def test_run_validates_at_the_references_points(accum):
    d = _StubDriver(accum)
    saved = []
    out = d.run(5, valid_steps=2, val_loaders="seen", val2_loaders="unseen", on_checkpoint=saved.append)
    assert len(out) == 5 * accum
    # every second optimizer step, seen then unseen, and once more after step 5 (:319-332)
    assert d.calls == [(g, s, l) for g in (2, 4, 5) for s, l in (("_seen", "seen"), ("_unseen", "unseen"))]
    assert saved == [2, 4, 5]
    assert d.val_logs == [(g, {"val_seen_x": float(g), "val_unseen_x": float(g)}) for g in (2, 4, 5)]
    d = _StubDriver(accum)
    d.run(4, valid_steps=2, val_loaders="seen", val2_loaders="unseen", on_checkpoint=saved.append)
    assert [c[0] for c in d.calls] == [2, 2, 4, 4]            # the last step was a multiple: no extra pass
    d = _StubDriver(accum)
    assert len(d.run(5)) == 5 * accum and d.calls == [] and d.val_logs == []    # the defaults: today's behaviour


def test_validate_refuses_an_unknown_task_before_touching_the_device():
    d = _StubDriver()
    with pytest.raises(ValueError, match="mrc"):              # as train_step does (MRC / OG are dead code in this fork)
        PretrainDriver.validate(d, {"mlm": [], "mrc": []})


def test_build_lists_the_file_with_the_row_kernel_flags():
    assert "eval_tail.hip" in build.SOURCES and "eval_tail.hip" in build.NO_PACKED_FP32
    assert "-fno-slp-vectorize" in build.PER_SOURCE_FLAGS["eval_tail.hip"]
    src = open(build.CSRC + "/eval_tail.hip").read()
    code = "\n".join(line.split("//")[0] for line in src.splitlines())
    assert "atomic" not in code and "__shared__" in code
    # one forward for training and validation
    pl = open(build.CSRC + "/planner.hip").read()
    assert pl.count("mlm_logits_fwd(") == 3
