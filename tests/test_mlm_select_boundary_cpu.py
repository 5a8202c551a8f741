"""CPU-side checks of the MLM selection's boundary (in the style of tests/test_traj_nodes_boundary_cpu.py): etp_mlm_select is declared
and exported with its two status codes, every refusal its header comment lists comes back as ETP_ERR_INVALID without a GPU (nothing is
launched: the operands are addresses that are never read), the host layer fails loudly without a GPU, and the loader's TrajBatch carries
``mlm_dev`` -- int32 [B, L] labels in the batch's one staging buffer plus the host-known count -- beside an unchanged dict."""
import types

import numpy as np
import pytest
import torch

from etpnav_amd import _lib, build, pretrain
from etpnav_amd import pretrain_data as pdata
from etpnav_amd import step as step_mod
from tests import mlm_select_ref as ms
from tests import pretrain_data_ref as ref

P = 0x10000          # an aligned address; never dereferenced by a refused call
ARGS = ["txt_labels", "n", "vocab", "n_expected", "cap", "rows", "ptr_t", "labels", "status"]
POINTERS = ["txt_labels", "rows", "ptr_t", "labels", "status"]


def call(**kw):
    a = {k: P for k in POINTERS}
    a.update(n=48, vocab=ms.VOCAB, n_expected=7, cap=9)
    a.update(kw)
    return _lib.lib().etp_mlm_select(*[a[k] for k in ARGS], None)


def test_symbol_codes_and_citations():
    protos = _lib.parse_header()
    assert "etp_mlm_select" in _lib.declared_symbols() and hasattr(_lib.lib(), "etp_mlm_select")
    assert len(protos["etp_mlm_select"][1]) == len(ARGS) + 1
    hdr = open(_lib.HEADER).read()
    assert f"#define ETP_MLM_ERR_COUNT {ms.ERR_COUNT}\n" in hdr and f"#define ETP_MLM_ERR_LABEL {ms.ERR_LABEL}\n" in hdr
    assert (pretrain.MLM_ERR_COUNT, pretrain.MLM_ERR_LABEL) == (ms.ERR_COUNT, ms.ERR_LABEL)
    doc = hdr[hdr.index("The MLM task's masked-row selection"):hdr.index("int etp_mlm_select")]
    assert "pretrain_cmt.py:141-163" in doc and "MlmStep.__init__" in doc and "torch.nonzero" in doc and "cumsum" in doc
    assert "no atomics" in doc and "no scratch" in doc


REFUSALS = {"n 0": dict(n=0), "n -1": dict(n=-1), "n 2^20 + 1": dict(n=(1 << 20) + 1), "vocab 0": dict(vocab=0), "vocab -5": dict(vocab=-5),
            "n_expected -1": dict(n_expected=-1), "n_expected above cap": dict(n_expected=10), "cap -1": dict(cap=-1, n_expected=0),
            "misaligned labels": dict(labels=P + 4)}
REFUSALS.update({f"NULL {k}": {k: None} for k in POINTERS})
REFUSALS.update({f"misaligned {k}": {k: P + 2} for k in POINTERS if k != "labels"})


@pytest.mark.parametrize("name", list(REFUSALS))
def test_refusals_come_back_before_anything_is_launched(name):
    assert call(**REFUSALS[name]) == -1, name
    assert b"etp_mlm_select" in _lib.lib().etp_last_error()


def test_kernel_keeps_the_files_idiom():
    src = open(build.CSRC + "/traj_batch.hip").read()
    k = src[src.index("void mlm_select_kernel"):src.index('extern "C" int etp_mlm_select')]
    assert "__ballot(" in k and "__popcll(" in k and "__syncthreads" not in k and "Add(" not in k
    assert "dim3(1), dim3(256)" in src[src.index('extern "C" int etp_mlm_select'):]       # one workgroup


@pytest.mark.skipif(torch.cuda.is_available(), reason="CPU-only check")
def test_host_layer_fails_loudly_without_a_gpu():
    from etpnav_amd.planner import GlocalTextPathNavCMT, default_config
    from oracle.make_golden_pretrain import make_case
    cfg, _, batch = make_case()
    model = GlocalTextPathNavCMT(default_config(use_lang2visn_attn=True, vocab_size=cfg.vocab_size, num_l_layers=1, num_pano_layers=1,
                                                num_x_layers=1), device="cpu")
    for kw in (dict(), dict(select="host"), dict(capacity=True), dict(capacity={"B": 4, "Nm": 9})):
        with pytest.raises(_lib.EtpError, match="no CPU fallback"):
            pretrain.MlmStep(model, batch, **kw)
    with pytest.raises(_lib.EtpError, match="no CPU fallback"):
        step_mod.PlannerStep(model, batch, capacity=True)


def test_step_arguments_are_checked_before_the_device_is_touched():
    from etpnav_amd.planner import GlocalTextPathNavCMT, default_config
    from oracle.make_golden_pretrain import make_case
    cfg, _, batch = make_case()
    model = GlocalTextPathNavCMT(default_config(use_lang2visn_attn=True, vocab_size=cfg.vocab_size, num_l_layers=1, num_pano_layers=1,
                                                num_x_layers=1), device="cpu")
    with pytest.raises(ValueError, match="select"):
        pretrain.MlmStep(model, batch, select="gpu")
    assert step_mod.CAPACITY_KEYS == ("B", "L", "R", "V", "G", "Nm")
    assert set(step_mod.INPUT_AXES) == {k for k, _, _ in step_mod.INPUTS}


class _StubLib:
    """stands in for the two launches of assemble: the staging and the views are what is under test"""

    def __init__(self):
        self.calls = []

    def etp_traj_views(self, *a):
        self.calls.append("etp_traj_views")
        return 0

    def etp_traj_pair_dists(self, *a):
        self.calls.append("etp_traj_pair_dists")
        return 0


def _stub_loader(monkeypatch):
    """MlmBatches over a store that lives on the CPU: everything of assemble but the two kernels runs"""
    index = ref.make_index()
    c = ref.corpus()
    lo = pdata.MlmBatches.__new__(pdata.MlmBatches)
    lo.index, lo.batch_size, lo.gen, lo.shuffle = index, 2, np.random.default_rng(0), False
    lo.device = torch.device("cpu")
    lo.img, lo.dep = torch.from_numpy(np.ascontiguousarray(c["img"])), torch.from_numpy(np.ascontiguousarray(c["dep"]))
    lo.view_loc_tab = torch.from_numpy(index.view_loc_tab)
    lo.status, lo._status_split = None, 0
    lo.vocab_range, lo.mask_id = pdata.VOCAB_RANGE, pdata.MASK_TOKEN_ID
    stub = _StubLib()
    monkeypatch.setattr(pdata._lib, "lib", lambda: stub)
    monkeypatch.setattr(torch.cuda, "current_stream", lambda device=None: types.SimpleNamespace(cuda_stream=0))
    monkeypatch.setattr(index.graphs, "dist_tab", torch.zeros(max(1, index.graphs.dist_len), dtype=torch.float64), raising=False)
    return lo, stub


def test_traj_batch_carries_mlm_dev_beside_an_unchanged_dict(monkeypatch):
    lo, stub = _stub_loader(monkeypatch)
    items = ref.js("mlm_items")
    b = lo.batch(items, ref.mlm_uniforms())
    assert stub.calls == ["etp_traj_views", "etp_traj_pair_dists"]
    assert isinstance(b, pdata.TrajBatch) and "mlm_dev" not in b and "mlm_labels" not in b
    md = b.mlm_dev
    assert sorted(md) == ["n_masked", "txt_labels"] and type(md["n_masked"]) is int
    tl = md["txt_labels"]
    assert tl.dtype == torch.int32 and tl.is_contiguous() and tuple(tl.shape) == tuple(b["txt_ids"].shape)
    # the host key stays exactly as it is: int64 on the host, and the device segment holds the same values
    host = b["txt_labels"]
    assert host.dtype == torch.int64 and host.device.type == "cpu" and torch.equal(host, tl.to(torch.int64))
    assert np.array_equal(host.numpy(), ref.fixture()["mlm_all_txt_labels"])
    assert md["n_masked"] == int((host != -1).sum()) > 0
    # one staging buffer: the segment is a view of the storage the other table views share, 16-byte aligned in it
    assert tl.untyped_storage().data_ptr() == b.traj_dev["step_off"].untyped_storage().data_ptr() == b["txt_ids"].untyped_storage().data_ptr()
    assert (tl.data_ptr() - tl.untyped_storage().data_ptr()) % 16 == 0
    # the restatement on the segment is the selection the step's host route builds from the host key
    rows, ptr_t, labels, count = ms.select(tl.numpy())
    assert count == md["n_masked"] and ms.flags(tl.numpy(), ms.VOCAB, count) == 0


def test_a_sap_batch_and_a_plain_dict_have_no_mlm_dev(monkeypatch):
    assert pdata.TrajBatch({"a": 1}).mlm_dev is None and getattr({"a": 1}, "mlm_dev", None) is None
    lo, _ = _stub_loader(monkeypatch)
    recs = [lo.index.record(i, None) for i in ref.js("mlm_items")[:2]]
    b = lo.assemble(recs, [r["txt"] for r in recs], np.zeros(len(recs), np.int64))
    assert b.mlm_dev is None and "txt_labels" not in b and b.traj_dev is not None
