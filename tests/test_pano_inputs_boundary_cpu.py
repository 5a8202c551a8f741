"""CPU-side checks of etp_pano_inputs' boundary (in the style of tests/test_pano_store_boundary_cpu.py): the entry point of
csrc/pano_inputs.hip is declared and exported, every refusal its header comment lists comes back as ETP_ERR_INVALID without a GPU
(nothing is launched: the operands are addresses that are never read), waypoint.panorama_inputs fails loudly where a launch is needed,
the build compiles the file under the row kernels' flags, and ETP.forward(mode='waypoint') without fuse_pano_inputs returns exactly the
reference's ten keys."""
from types import SimpleNamespace

import pytest
import torch

from etpnav_amd import _lib, build, graph_inputs
from etpnav_amd import waypoint as wp
from tests import pano_inputs_ref as pir

P = 0x10000          # an aligned address; never dereferenced by a refused call
ARGS = ["rgb_embedding", "depth_embedding", "cand_count", "cand_angle", "cand_angle_tab", "pano_angle_tab", "B", "V", "max_pred", "Frgb", "C",
        "HW", "rgb_fts", "dep_fts", "loc_fts", "nav_types", "view_lens", "cand_img", "status"]
SCALARS = ("B", "V", "max_pred", "Frgb", "C", "HW")
TEN_KEYS = ["cand_rgb", "cand_depth", "cand_angle_fts", "cand_img_idxes", "cand_angles", "cand_distances", "pano_rgb", "pano_depth",
            "pano_angle_fts", "pano_img_idxes"]


def call(**kw):
    a = {k: P for k in ARGS}
    a.update(B=2, V=16, max_pred=5, Frgb=512, C=128, HW=16)
    a.update(kw)
    return _lib.lib().etp_pano_inputs(*[a[k] for k in ARGS], None)


def test_symbol_flags_and_citations():
    protos = _lib.parse_header()
    assert "etp_pano_inputs" in _lib.declared_symbols() and hasattr(_lib.lib(), "etp_pano_inputs")
    assert len(protos["etp_pano_inputs"][1]) == len(ARGS) + 1
    hdr = open(_lib.HEADER).read()
    for sym, val in (("COUNT", pir.ERR_COUNT), ("ANGLE", pir.ERR_ANGLE), ("VIEWS", pir.ERR_VIEWS)):
        assert f"#define ETP_PINPUTS_ERR_{sym} {val}\n" in hdr
        assert getattr(wp, f"PINPUTS_ERR_{sym}") == val
    doc = hdr[hdr.index("The panorama encoder's inputs from the waypoint head's candidate table"):hdr.index("int etp_pano_inputs")]
    assert "Policy_ViewSelection_ETP.py:289-342" in doc and "ss_trainer_ETP.py:308-342" in doc


REFUSALS = {"Frgb 510": dict(Frgb=510), "Frgb 0": dict(Frgb=0), "Frgb -4": dict(Frgb=-4), "HW 0": dict(HW=0), "HW -16": dict(HW=-16),
            "V 11": dict(V=11), "V 0": dict(V=0), "max_pred 0": dict(max_pred=0), "max_pred -1": dict(max_pred=-1), "B 0": dict(B=0),
            "B -1": dict(B=-1), "C 0": dict(C=0),
            "misaligned rgb_embedding": dict(rgb_embedding=P + 8), "misaligned depth_embedding": dict(depth_embedding=P + 4),
            "misaligned rgb_fts": dict(rgb_fts=P + 8), "misaligned dep_fts": dict(dep_fts=P + 2), "misaligned loc_fts": dict(loc_fts=P + 1),
            "misaligned nav_types": dict(nav_types=P + 4), "misaligned view_lens": dict(view_lens=P + 4),
            "misaligned cand_count": dict(cand_count=P + 2), "misaligned cand_angle": dict(cand_angle=P + 1),
            "misaligned cand_angle_tab": dict(cand_angle_tab=P + 2), "misaligned pano_angle_tab": dict(pano_angle_tab=P + 2),
            "misaligned cand_img": dict(cand_img=P + 2), "misaligned status": dict(status=P + 2)}
REFUSALS.update({f"NULL {k}": {k: None} for k in ARGS if k not in SCALARS})


@pytest.mark.parametrize("name", list(REFUSALS))
def test_refusals_come_back_before_anything_is_launched(name):
    assert call(**REFUSALS[name]) == -1, name
    assert b"etp_pano_inputs" in _lib.lib().etp_last_error()


@pytest.mark.skipif(torch.cuda.is_available(), reason="CPU-only check")
def test_compute_fails_loudly_without_gpu():
    table = torch.from_numpy(pir.crafted_table(2, 0))
    cand = wp.CandidateTable(None, None, table, True)
    for V in (None, 16):
        with pytest.raises(_lib.EtpError):
            wp.panorama_inputs(torch.zeros(24, 512), torch.zeros(24, 128, 4, 4), cand, False, V=V)


def test_vp_feature_variable_hands_fused_inputs_on_and_is_unchanged_otherwise():
    five = {k: object() for k in wp.PANO_INPUT_KEYS}
    out = graph_inputs.vp_feature_variable({"pano_inputs": dict(five, status=1, cand_img=2)}, "cpu")
    assert list(out) == ["rgb_fts", "dep_fts", "loc_fts", "nav_types", "view_lens"] and all(out[k] is five[k] for k in five)
    with pytest.raises(_lib.EtpError):                        # without the key: the existing route, which needs a GPU
        graph_inputs.vp_feature_variable({"cand_rgb": []}, "cpu")


class _Tail:
    def __init__(self, table):
        self.table = torch.from_numpy(table)

    def __call__(self, rgb, dep):
        return None

    def candidates(self, logits, in_train, generator=None, uniforms=None):
        return wp.CandidateTable(None, None, self.table, True)


def test_flag_is_off_by_default_and_the_dict_has_exactly_todays_ten_keys(monkeypatch):
    from etpnav_amd.policy import ETP
    monkeypatch.setattr("etpnav_amd.policy.get_vlnbert_models", lambda **k: torch.nn.Identity())
    net = ETP(model_config=SimpleNamespace(task_type="r2r"), dtype=torch.float32, device="cpu")
    assert net.fuse_pano_inputs is False and net.pano_inputs_capacity is None
    B = 3
    obs = {}
    for a in range(12):
        suffix = "" if a == 0 else f"_{a * 30.0}"
        obs["rgb" + suffix], obs["depth" + suffix] = torch.zeros(B, 2, 2, 3), torch.zeros(B, 2, 2, 1)
    net.depth_encoder = lambda o: torch.zeros(o["depth"].shape[0], 128, 4, 4)
    net.rgb_encoder = lambda o: torch.zeros(o["rgb"].shape[0], 512)
    out = net(mode="waypoint", waypoint_predictor=_Tail(pir.crafted_table(B, 0)), observations=obs, in_train=False)
    assert list(out.keys()) == TEN_KEYS
    assert [len(x) for x in out["cand_angles"]] == [5, 0, 1] and tuple(out["pano_rgb"].shape) == (B, 12, 512)


def test_build_lists_the_file_with_the_row_kernel_flags():
    assert "pano_inputs.hip" in build.SOURCES and "pano_inputs.hip" in build.NO_PACKED_FP32
    assert "-fno-slp-vectorize" in build.PER_SOURCE_FLAGS["pano_inputs.hip"]
    src = open(build.CSRC + "/pano_inputs.hip").read()
    assert "atomic" not in src.replace("no atomics", "") and "__shared__" not in src
    for fn in ("sinf", "cosf", "expf", "__sinf", "__cosf"):
        assert fn + "(" not in src, fn
