"""CPU-side checks of tests/rollout_ref.py (the reference of tests/test_rollout_gpu.py): the float64 restatement is held to torch's own
float64 F.cross_entropy chain and its autograd and to the recording of the reference trainer's statements
(tests/golden/rollout_loss_small.npz, tools/make_golden_rollout_loss.py); the host teacher of etpnav_amd.rollout equals the recorded
labels of both expert policies; an fp32 emulation of the kernels' schedule stays inside the derived bounds on every case of the GPU
list; and every planted mistake is rejected by the checks the GPU file uses."""
import json

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from etpnav_amd.graph_inputs import GraphMapLite
from tests import rollout_ref as rr

F64 = torch.float64


def torch_chain(steps, ml_weight, dtype=F64):
    """ss_trainer_ETP.py:820, :892, :1055 written with torch, and its autograd"""
    loss, total_actions, leaves = 0.0, 0.0, []
    for x, y in steps:
        x = x.to(dtype).requires_grad_(True)
        leaves.append(x)
        total_actions += x.shape[0]
        loss = loss + F.cross_entropy(x, y, reduction="sum", ignore_index=rr.IGNORE)
    loss = ml_weight * loss / total_actions
    loss.backward()
    return loss.detach(), [x.grad for x in leaves]


CASES = rr.cases()


@pytest.mark.parametrize("case", CASES, ids=[c[0] for c in CASES])
def test_restatement_equals_torch_float64(case):
    name, B, G, T, shift, ign, w = case
    steps = rr.make_steps(B, G, T, shift, ign, CASES.index(case))
    r = rr.reference(steps, w)
    loss, grads = torch_chain(steps, w)
    assert abs(r["loss"] - float(loss)) <= 1e-12 * max(1.0, abs(float(loss))), (name, r["loss"], float(loss))
    for a, b in zip(r["dlogits"], grads):
        assert float((a - b).abs().max()) <= 1e-12, name
    assert r["N"] == sum(rr.shrinking(B, T)) and len(steps) == T


def test_case_list_covers_what_it_names():
    assert sorted({(c[1], c[2]) for c in CASES}) == sorted((b, g) for b in rr.CASE_B for g in rr.CASE_G)
    assert {c[3] for c in CASES} == set(rr.CASE_T) and {c[4] for c in CASES} == set(rr.SHIFTS) and {c[5] for c in CASES} == set(rr.IGNORED)
    assert rr.shrinking(33, 15)[0] == 33 and rr.shrinking(33, 15)[-1] < 33 and min(rr.shrinking(1, 15)) == 1
    st = rr.stacked(rr.make_steps(rr.STACKED[1], rr.STACKED[2], rr.STACKED[0], 0.0, "none", 3))
    assert len(st) == 1 and st[0][0].shape[0] > 256          # more than one round of the forward kernel's 256 rows
    labels = torch.cat([y for c in CASES[:12] for _, y in rr.make_steps(c[1], c[2], c[3], c[4], c[5], CASES.index(c))])
    assert bool((labels == 0).any()) and bool((labels == rr.IGNORE).any())


def test_restatement_equals_the_recording():
    z, meta, steps = rr.load_fixture()
    w = meta["cfg"]["ml_weight"]
    assert [int(x.shape[0]) for x, _ in steps] == meta["active"] == [4, 4, 3, 1, 1]
    labels = torch.cat([y for _, y in steps])
    assert bool((labels == rr.IGNORE).any()) and bool((labels == 0).any())
    assert all(bool(torch.isneginf(x[:, 1]).all()) for x, _ in steps)          # -inf on the visited nodes
    r = rr.reference(steps, w)
    assert abs(r["loss"] - float(z["loss_f64"])) <= 1e-12
    for t, d in enumerate(r["dlogits"]):
        assert float((d - torch.from_numpy(z[f"dlogits_f64_{t}"])).abs().max()) <= 1e-12, t
    bl, bd = rr.fixture_fp32_bounds(r, w)
    t64 = lambda v: torch.tensor(v, dtype=F64)
    rr.within(("fixture", "loss_f32"), torch.from_numpy(z["loss_f32"]).reshape(()), t64(r["loss"]), t64(bl))
    for t, d in enumerate(r["dlogits"]):
        rr.within(("fixture", "dlogits_f32"), torch.from_numpy(z[f"dlogits_f32_{t}"]), d, bd[t])
    # the recording against torch run here: the statements are torch's
    loss, grads = torch_chain(steps, w)
    assert abs(float(loss) - float(z["loss_f64"])) <= 1e-12


def test_host_teacher_equals_the_recording_for_both_policies():
    z, meta, steps = rr.load_fixture()
    cfg = meta["cfg"]
    assert cfg == rr.PLAN_CFG
    log = rr.scripted_rollout(lambda: GraphMapLite(True, cfg["loc_noise"], cfg["merge_ghost"], cfg["ghost_aug"]), rr.package_teacher())
    assert [e["slots"] for e in log] == meta["slots"] and [e["vp_ids"] for e in log] == meta["vp_ids"]
    assert [e["no_vp_left"] for e in log] == meta["no_vp_left"]
    for t, e in enumerate(log):
        assert e["spl"] == z[f"labels_{t}"].tolist() and e["ndtw"] == z[f"labels_ndtw_{t}"].tolist(), t
        np.testing.assert_array_equal(e["logits"], z[f"logits_{t}"])
        assert json.loads(json.dumps(e["dists"])) == meta["dists"][t], t          # the distances the stub environments returned
    assert any(e["spl"] != e["ndtw"] for e in log)
    # another random stream picks another real position of the merged ghost somewhere: the generator argument is what draws
    other = rr.scripted_rollout(lambda: GraphMapLite(True, cfg["loc_noise"], cfg["merge_ghost"], cfg["ghost_aug"]), rr.package_teacher(seed=6))
    assert [e["spl"] for e in other] == [e["spl"] for e in log] or [e["dists"] for e in other] != [e["dists"] for e in log]


def test_teacher_raises_on_an_unknown_policy_and_on_ndtw_without_paths():
    from etpnav_amd.rollout import teacher_actions
    envs, _ = rr.plan_envs()
    envs.reset()
    g = GraphMapLite(True, 0.5, True, 0)
    g.update_graph(None, 1, "0", np.zeros(3), 0.0, ["0_0"], [np.array([2.0, 0, 0])], [0.0], [np.array([2.0, 0, 0])])
    ids = [[None, "0", "g0"]]
    assert teacher_actions([g], ids, [False], envs, "spl") == [2]
    with pytest.raises(NotImplementedError):
        teacher_actions([g], ids, [False], envs, "other")
    with pytest.raises(ValueError):
        teacher_actions([g], ids, [False], envs, "ndtw")


def check_all(name, loss, dls, rec, steps, w, upstream=1.0):
    rr.check_loss(name, loss, steps, w)
    rr.check_dlogits(name, dls, steps, w, upstream=upstream)
    rr.check_record(name, rec, steps)


@pytest.mark.parametrize("case", CASES, ids=[c[0] for c in CASES])
def test_fp32_emulation_stays_inside_the_bounds(case):
    name, B, G, T, shift, ign, w = case
    steps = rr.make_steps(B, G, T, shift, ign, CASES.index(case))
    loss, dls, rec = rr.emulate(steps, w)
    check_all("emulation " + name, loss, dls, rec, steps, w)


def test_fp32_emulation_of_the_stacked_call_and_an_upstream_gradient():
    T, B, G = rr.STACKED
    steps = rr.make_steps(B, G, T, 80.0, "some", 5)
    st = rr.stacked(steps)
    loss, dls, rec = rr.emulate(st, 0.37)
    check_all("emulation stacked", loss, dls, rec, st, 0.37)
    assert abs(float(loss) - float(rr.emulate(steps, 0.37)[0])) <= 2 * rr.loss_bound(rr.reference(steps, 0.37), 0.37)
    for up in (0.5, 0.3):
        _, dls, _ = rr.emulate(steps[:3], 0.37, upstream=up)
        rr.check_dlogits(f"emulation upstream {up}", dls, steps[:3], 0.37, upstream=up)


@pytest.mark.parametrize("mutation", rr.MUTATIONS)
def test_planted_mistakes_are_rejected(mutation):
    steps, w = rr.mutation_case()
    loss, dls, rec = rr.emulate(steps, w)
    check_all("mutation case, unmutated", loss, dls, rec, steps, w)
    loss, dls, rec = rr.emulate(steps, w, mutate=mutation)
    rejected = []
    for fn in (lambda: rr.check_loss(mutation, loss, steps, w), lambda: rr.check_dlogits(mutation, dls, steps, w),
               lambda: rr.check_record(mutation, rec, steps)):
        try:
            fn()
        except AssertionError:
            rejected.append(True)
    assert rejected, f"the planted mistake {mutation!r} passes every check of the GPU file"
