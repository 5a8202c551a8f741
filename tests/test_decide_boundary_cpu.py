"""CPU-side checks of the rollout decision's boundary (in the style of tests/test_waypoint_boundary_cpu.py): etp_nav_decide is declared
and exported, every refusal its header comment lists comes back as ETP_ERR_INVALID without a GPU (nothing is launched: the operands
are addresses that are never read), the host mirror fails loudly without a GPU and the supporting changes keep their defaults."""
import inspect

import numpy as np
import pytest
import torch

from etpnav_amd import _lib
from etpnav_amd import decide, graph_inputs

P = 0x10000          # an aligned address; never dereferenced by a refused call


def call(**kw):
    a = dict(logits=P, node_pos=P, n_nodes=P, adj=P, ghost_pos=P, n_ghost=P, front_ptr=P, front_idx=P, cur_node=P, slot=P, uniforms=None,
             teacher=None, sample_ratio=0.0, force_stop=0, B=2, Nmax=4, Mmax=3, Fmax=5, G=8, stop_scores=P, S=2, record=P)
    a.update(kw)
    return _lib.lib().etp_nav_decide(a["logits"], a["node_pos"], a["n_nodes"], a["adj"], a["ghost_pos"], a["n_ghost"], a["front_ptr"],
                                     a["front_idx"], a["cur_node"], a["slot"], a["uniforms"], a["teacher"], a["sample_ratio"], a["force_stop"],
                                     a["B"], a["Nmax"], a["Mmax"], a["Fmax"], a["G"], a["stop_scores"], a["S"], a["record"], None)


def test_symbol_is_declared_and_exported():
    assert "etp_nav_decide" in _lib.declared_symbols() and hasattr(_lib.lib(), "etp_nav_decide")
    assert len(_lib.parse_header()["etp_nav_decide"][1]) == 23


REFUSALS = {
    "B 0": dict(B=0), "B -1": dict(B=-1),
    "G 258": dict(G=258), "G 0": dict(G=0), "Nmax 65": dict(Nmax=65), "Nmax 0": dict(Nmax=0), "Mmax 193": dict(Mmax=193), "Mmax -1": dict(Mmax=-1),
    "uniforms without teacher, sample_ratio > 0": dict(uniforms=P, sample_ratio=0.25),
    "misaligned logits": dict(logits=P + 2), "misaligned adj": dict(adj=P + 1), "misaligned slot": dict(slot=P + 2),
    "misaligned record": dict(record=P + 2), "misaligned table": dict(stop_scores=P + 2), "misaligned uniforms": dict(uniforms=P + 2, teacher=P),
    "misaligned teacher": dict(uniforms=P, teacher=P + 4),
    "NULL table": dict(stop_scores=None), "S 0": dict(S=0),
    "NULL logits": dict(logits=None), "NULL record": dict(record=None), "NULL slot": dict(slot=None),
    "NULL ghost arrays with Mmax > 0": dict(ghost_pos=None),
}


@pytest.mark.parametrize("name", list(REFUSALS))
def test_refusals_come_back_before_anything_is_launched(name):
    assert call(**REFUSALS[name]) == -1, name
    assert b"etp_nav_decide" in _lib.lib().etp_last_error()


@pytest.mark.skipif(torch.cuda.is_available(), reason="CPU-only check")
def test_compute_fails_loudly_without_gpu():
    d = decide.RolloutDecider(2, "cpu")
    g = graph_inputs.GraphMapLite(False, 0.5, True, 0)
    g.update_graph(None, 1, "0", np.zeros(3), 0.0, ["0_0"], [np.array([2.0, 0, 0])], [0.0], [None])
    with pytest.raises(_lib.EtpError):
        d.decide(torch.zeros(2, 3), [g, g], ["0", "0"], 0, "argmax")
    with pytest.raises(_lib.EtpError):
        decide.nav_decide(torch.zeros(1, 3), {"_dims": (1, 1, 1, 1)}, torch.zeros(1, dtype=torch.int32), torch.zeros(1, 64))


def test_host_mirror_bookkeeping_and_defaults():
    d = decide.RolloutDecider(4, "cpu", back_algo="control", consume_ghost=True, tryout=False, max_len=6)
    assert d.active == [0, 1, 2, 3] and d.prev_vp == [None] * 4
    d.prev_vp[2] = "5"
    d.pause(1)
    assert d.active == [0, 2, 3] and d.prev_vp == [None, "5", None]
    d.reset()
    assert d.active == [0, 1, 2, 3] and d.prev_vp == [None] * 4
    assert graph_inputs.GraphMapLite(False, 0.5, True, 0).node_stop_scores == {}
    for fn in (graph_inputs.assemble_on_device, graph_inputs.nav_gmap_variable):
        assert inspect.signature(fn).parameters["keep_compact"].default is False
    assert list(inspect.signature(d.decide).parameters)[:9] == ["nav_logits", "gmaps", "cur_vp", "stepk", "feedback", "sample_ratio",
                                                                "teacher_actions", "generator", "uniforms"]
    assert (decide.HDR, decide.STOP, decide.ERR_ACTION, decide.ERR_UNREACHABLE, decide.ERR_INPUT) == (8, 1, 2, 4, 8)


def test_env_actions_and_flags_from_a_record():
    g = graph_inputs.GraphMapLite(False, 0.5, True, 0)
    g.update_graph(None, 1, "0", np.zeros(3), 0.0, ["0_0"], [np.array([2.0, 0, 0])], [0.0], [None])
    g.update_graph("0", 2, "1", np.array([0.0, 0, 2.0]), 0.0, [], [], [], [])
    rec = np.array([[3, 3, 0, 1, 0, 0, 1, 0, 0, -1], [0, 0, 1, 1, 1, -1, 0, 0, -1, -1]], dtype=np.int32)
    go, stop = decide.env_actions_from_record(rec, [g, g], ["1", "1"], "control", True)
    assert go["action"]["act"] == 4 and go["action"]["front_vp"] == "0" and go["action"]["ghost_vp"] == "g0" and go["vis_info"] is None
    assert [vp for vp, _ in go["action"]["back_path"]] == ["0"]
    assert stop["action"]["act"] == 0 and stop["action"]["stop_vp"] == "1" and stop["action"]["back_path"] == []
    assert sorted(stop["vis_info"]) == ["ghosts", "nodes", "predict_ghost"]
    assert decide.env_actions_from_record(rec, [g, g], ["1", "1"], "teleport", True)[0]["action"]["back_path"] is None
    for flag in (decide.ERR_ACTION, decide.ERR_UNREACHABLE, decide.ERR_INPUT):
        bad = rec.copy()
        bad[1, 2] = flag
        with pytest.raises(ValueError):
            decide.raise_on_flags(bad)
    decide.raise_on_flags(rec)
