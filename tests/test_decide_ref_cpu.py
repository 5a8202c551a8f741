"""tests/decide_ref.py (the fp64 restatement the GPU tests of the rollout decision compare against) pinned down on the CPU:

  * where the reference tree is present (/root/reference, or $ETP_REFERENCE) and networkx is installed, it equals the REAL code on
    random rollouts: the reference trainer's own decision statements (ss_trainer_ETP.py:880-977, cut out by
    tools/make_golden_decide.py) on real GraphMap objects against episode_ref on GraphMapLite;
  * everywhere, it equals tests/golden/decide_small.npz (recorded from the real code by tools/make_golden_decide.py);
  * every deliberate error of decide_ref.MUTATIONS is rejected by that recording;
  * the bound of stop_prob holds an fp32 emulation of the kernel's schedule and rejects an error of two bounds;
  * the operator cases the GPU test runs can be drawn (their conditions hold by construction; no case is left out).
"""
import importlib.util
import os

import numpy as np
import pytest

from etpnav_amd.graph_inputs import GraphMapLite
from tests import decide_ref as dr

REF = os.environ.get("ETP_REFERENCE", "/root/reference")
HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.join(HERE, "golden", "decide_small.npz")


def _have_ref():
    if not os.path.isfile(os.path.join(REF, "vlnce_baselines", "ss_trainer_ETP.py")):
        return False
    return importlib.util.find_spec("networkx") is not None


needs_ref = pytest.mark.skipif(not _have_ref(), reason="the reference tree (or networkx) is not on this machine")


def lite(cfg):
    return lambda: GraphMapLite(False, cfg["loc_noise"], cfg["merge_ghost"], 0)


@pytest.fixture(scope="module")
def golden():
    return dr.load_fixture(GOLDEN)


@needs_ref
@pytest.mark.parametrize("seed", [1, 2, 3])
def test_restatement_equals_the_real_statements_on_random_rollouts(seed):
    spec = importlib.util.spec_from_file_location("make_golden_decide", os.path.join(os.path.dirname(HERE), "tools", "make_golden_decide.py"))
    tool = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(tool)
    gu, code = tool.load_graph_utils(REF), tool.decision_statements(REF)
    for consume, back in ((True, "control"), (False, "teleport")):
        cfg = dict(dr.CFG, consume_ghost=consume, back_algo=back, max_len=7)
        real = dr.drive(lambda: gu.GraphMap(False, cfg["loc_noise"], cfg["merge_ghost"], 0), dr.RandomPlan(seed), tool.ReferenceStep(code, cfg), 5, cfg)
        got = dr.drive(lite(cfg), dr.ReplayPlan(real), dr.RefStep(5, cfg), 5, cfg)
        dr.compare_logs(got, real, f"seed {seed} consume_ghost {consume}")
        assert sum(len(e["slots"]) for e in real) >= 12           # the rollouts do go on for a while


def test_restatement_equals_the_fixture(golden):
    log, cfg = golden
    assert cfg == dr.CFG
    got = dr.drive(lite(cfg), dr.ReplayPlan(log), dr.RefStep(4, cfg), 4, cfg)
    dr.compare_logs(got, log, "fixture")


def test_fixture_covers_what_it_claims(golden):
    log, cfg = golden
    assert cfg["consume_ghost"] and cfg["back_algo"] == "control" and len(log) == cfg["max_len"] == 6
    assert [e["slots"] for e in log] == [[0, 1, 2, 3], [0, 1, 2, 3], [0, 1, 3], [0, 3], [0, 3], [0, 3]]      # two episodes paused mid-way
    assert {e["feedback"] for e in log} == {"sample", "argmax"}
    assert log[1]["ghosts_after"][2] == [] and log[1]["a_t"][2] == dr.IGNORE and log[1]["actions"][2]["act"] == 0   # no ghost left
    assert all(a != 0 for a in log[5]["a_t"]) and all(x["act"] == 0 for x in log[5]["actions"])                  # the forced stop
    assert log[4]["actions"][1]["back_path"] == []                                                               # target == cur
    assert any(len(x["back_path"]) >= 4 for x in log[5]["actions"])
    assert log[1]["uniforms"][0][1] == cfg["sample_ratio"]
    l = np.array(log[4]["logits"][0])
    assert int((l == l.max()).sum()) == 2


@pytest.mark.parametrize("mut", dr.MUTATIONS)
def test_mutations_are_rejected_by_the_fixture(golden, mut):
    log, cfg = golden
    with pytest.raises((AssertionError, KeyError)):
        got = dr.drive(lite(cfg), dr.ReplayPlan(log), dr.RefStep(4, cfg, mut=mut), 4, cfg)
        dr.compare_logs(got, log, mut)


def test_operator_cases_meet_their_conditions():
    c = dr.make_case([1, 2, 17, 64], [0, 1, 5, 192], seed=3, sample=True, S=6, name="cpu")
    assert c["G"] == 257 and c["batch"]["_dims"][:3] == (4, 64, 192) and len(set(c["slots"].tolist())) == 4
    for b, r in enumerate(c["refs"]):
        again = dr.check_conditions(c["eps"][b], c["logits"][b], c["table"][c["slots"][b]], c["uniforms"][b], int(c["teacher"][b]),
                                    c["sample_ratio"], False, name=f"cpu[{b}]")
        assert dr.record_row(again, 64).tolist() == dr.record_row(r, 64).tolist()
    assert c["refs"][0]["flags"] == dr.STOP and c["refs"][0]["path"] == []          # one node, no ghost: stops where it stands


def test_bound_holds_fp32_and_rejects_two_bounds():
    rng = np.random.default_rng(5)
    for G in (1, 3, 40, 257):
        l = dr.random_logits(min(G - 1, 5) if G > 1 else 0, max(G - 1 - 5, 0), G, rng) if G > 1 else np.zeros(1, np.float32)
        ref, E = float(dr.softmax64(l)[0]), dr.stop_prob_bound(l)
        e = np.exp((l - l.max()).astype(np.float32)).astype(np.float32)           # fp32 emulation: serial sum, one division
        s = np.float32(0)
        for x in e:
            s = np.float32(s + x)
        assert dr.record("cpu/stop_prob", float(np.float32(e[0] / s)), ref, E, f"G={G}") <= 1.0
        if ref > 0:
            with pytest.raises(AssertionError):
                dr.record("cpu/stop_prob", ref + 2 * E, ref, E, "two bounds off")
    for key in [k for k in dr.WORST if k.startswith("cpu/")]:
        del dr.WORST[key]
