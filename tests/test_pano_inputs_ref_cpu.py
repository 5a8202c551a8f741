"""tests/pano_inputs_ref.py pinned to what it restates, without a GPU:

  * the recording of the real `mode == 'waypoint'` branch (tests/golden/waypoint_small.npz: its ten keys for eval and train, and the
    encoder-output tables they came from), fed through tests/move_ref.py's restatement of RLTrainer._vp_feature_variable (pinned to the
    real method by tests/golden/vp_inputs.npz): rgb_fts, loc_fts, nav_types, view_lens bit for bit.  dep_fts: the recording's pooled
    depth keys are fp32 (torch's own pool), so they are held to the restatement's float64 mean within pano_inputs_ref's fp32 bound;
    the same keys pooled in float64 from the recorded table (the branch's flip and pool, restated here) match within 1e-12;
  * waypoint._waypoint_tail_mode (the existing route) + move_ref's vp_from_obs / vp_gather on the crafted tables, both table modes;
  * the fused route's host values (cand_angles, cand_distances, cand_img_idxes, cand_angle_fts) against the existing route's, bit for
    bit; the vectorised host view lengths against the restatement's;
  * the conditions the issue asks of the case list, the angle-table identity, and every planted mutation rejected by the comparator.
"""
import math
import os
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from etpnav_amd import waypoint as wp
from tests import move_ref as mr
from tests import pano_inputs_ref as pir

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "waypoint_small.npz")


golden_tables, golden_table = pir.golden_tables, pir.golden_table


def obs_of(z, prefix):
    o = {k: [torch.from_numpy(z[f"{prefix}{k}_{j}"]) for j in range(3)] for k in ("cand_rgb", "cand_depth", "cand_angle_fts")}
    o["cand_img_idxes"] = [z[f"{prefix}cand_img_idxes_{j}"] for j in range(3)]
    for k in ("pano_rgb", "pano_depth", "pano_angle_fts"):
        o[k] = torch.from_numpy(z[prefix + k])
    return o


def through_vp(obs):
    """move_ref's restatement of _vp_feature_variable -> rgb, dep, loc, nav, lens (torch)"""
    out = {}
    for name, ck, pk in (("rgb_fts", "cand_rgb", "pano_rgb"), ("dep_fts", "cand_depth", "pano_depth"), ("loc_fts", "cand_angle_fts", "pano_angle_fts")):
        cand, cand_ptr, pano, mask, V = mr.vp_from_obs(obs, ck, pk)
        out[name], out["nav_types"], out["view_lens"] = mr.vp_gather(cand if cand.numel() else None, cand_ptr, pano, mask, V)
    return out


def assert_same_route(name, vp, ref, dep64=None):
    for k in ("rgb_fts", "loc_fts", "nav_types", "view_lens"):
        got = vp[k].numpy()
        assert got.dtype == ref[k].dtype and got.shape == ref[k].shape and got.tobytes() == ref[k].tobytes(), (name, k)
    d = vp["dep_fts"].numpy()
    assert d.dtype == np.float32 and (np.abs(d.astype(np.float64) - ref["dep_fts"]) <= ref["dep_bound"]).all(), (name, "dep_fts (fp32 pool)")
    if dep64 is not None:
        assert np.abs(dep64 - ref["dep_fts"]).max() <= 1e-12, (name, float(np.abs(dep64 - ref["dep_fts"]).max()))


@pytest.mark.parametrize("in_train", [False, True], ids=["eval", "train"])
def test_restatement_is_the_recorded_branch_through_vp_feature_variable(in_train):
    z = np.load(GOLDEN)
    prefix = "train_" if in_train else "eval_"
    rgb, dep = golden_tables(z)
    table = golden_table(z)
    obs = obs_of(z, prefix)
    img = [pir.img_of(int(a)) for a in table[5 if in_train else 1].ravel()]
    assert img == np.concatenate(obs["cand_img_idxes"]).tolist()               # the recovered indices are the recording's
    vp = through_vp(obs)
    V = pir.ref_length(table, in_train)
    assert V == vp["rgb_fts"].shape[1]
    ref = pir.pano_inputs(rgb, dep, table, in_train, V)
    assert ref["written"].all() and not ref["status"].any()
    # the depth keys once more in float64: the branch's flip and pool (:201-213, 289-290) on the recorded table, then the same gather
    d = torch.from_numpy(dep).double().reshape(3, 12, 128, 16)
    pooled = torch.cat((d[:, 0:1], torch.flip(d[:, 1:], [1])), 1).mean(-1)
    assert np.abs(pooled.numpy() - z[prefix + "pano_depth"]).max() < 1e-6
    _, cand_ptr, _, mask, _ = mr.vp_from_obs(obs, "cand_depth", "pano_depth")
    cand64 = torch.cat([pooled[j][torch.as_tensor(obs["cand_img_idxes"][j])] for j in range(3)], 0)
    dep64 = mr.vp_gather(cand64, cand_ptr, pooled, mask, V)[0].numpy()
    assert_same_route(prefix, vp, ref, dep64)
    assert ref["cand_img"].ravel().tolist() == img


class _Tail:
    """stand-in for the predictor: the table is given, nothing runs on a device"""

    def __init__(self, table):
        self.table = torch.from_numpy(table)

    def __call__(self, rgb, dep):
        return None

    def candidates(self, logits, in_train, generator=None, uniforms=None):
        return wp.CandidateTable(None, None, self.table, True)


def _net():
    pool = torch.nn.Sequential(torch.nn.AdaptiveAvgPool2d((1, 1)), torch.nn.Flatten(start_dim=2))
    idx, fts = wp.pano_constants()
    return SimpleNamespace(space_pool_rgb=pool, space_pool_depth=pool, pano_img_idxes=idx, pano_angle_fts=fts)


@pytest.mark.parametrize("in_train", [False, True], ids=["eval", "train"])
@pytest.mark.parametrize("B,shift", [(1, 0), (3, 1), (8, 0), (33, 3)])
def test_restatement_is_the_existing_route_on_crafted_tables(B, shift, in_train, monkeypatch):
    table = pir.crafted_table(B, shift)
    rgb, dep, _ = pir.make_inputs(B, (512, 128, 16))
    net = _net()
    old = wp._waypoint_tail_mode(net, _Tail(table), torch.from_numpy(rgb), torch.from_numpy(dep).reshape(12 * B, 128, 4, 4), B, in_train, None, None)
    vp = through_vp(old)
    V = pir.ref_length(table, in_train)
    ref = pir.pano_inputs(rgb, dep, table, in_train, V)
    assert V == vp["rgb_fts"].shape[1] and ref["written"].all()
    assert_same_route(f"B{B}", vp, ref)
    # the vectorised host lengths and views
    assert wp.host_view_lens(table, in_train).tolist() == ref["view_lens"].tolist()
    # the fused route's host values are the existing route's
    seen = {}
    monkeypatch.setattr(wp, "panorama_inputs", lambda *a, **k: seen.update(V=k["V"]) or "launched")
    net.fuse_pano_inputs = True
    new = wp._waypoint_tail_mode(net, _Tail(table), torch.from_numpy(rgb), torch.from_numpy(dep).reshape(12 * B, 128, 4, 4), B, in_train, None, None)
    assert list(new) == ["cand_angle_fts", "cand_img_idxes", "cand_angles", "cand_distances", "pano_angle_fts", "pano_img_idxes", "pano_inputs"]
    assert new["pano_inputs"] == "launched" and seen["V"] == V             # the reference's padded length, from the one table copy
    for j in range(B):
        assert new["cand_angles"][j] == old["cand_angles"][j] and new["cand_distances"][j] == old["cand_distances"][j]
        assert isinstance(new["cand_img_idxes"][j], np.ndarray) and new["cand_img_idxes"][j].tolist() == old["cand_img_idxes"][j].tolist()
        a, b = new["cand_angle_fts"][j], old["cand_angle_fts"][j]
        assert a.shape == b.shape and a.dtype == b.dtype and torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))
        assert ref["cand_img"][j, :len(old["cand_img_idxes"][j])].tolist() == old["cand_img_idxes"][j].tolist()
    assert torch.equal(new["pano_angle_fts"], old["pano_angle_fts"]) and new["pano_img_idxes"].tolist() == old["pano_img_idxes"].tolist()


def test_fused_route_refuses_a_malformed_table_and_a_short_capacity(monkeypatch):
    monkeypatch.setattr(wp, "panorama_inputs", lambda *a, **k: "launched")
    net = _net()
    net.fuse_pano_inputs = True
    rgb, dep = torch.zeros(12, 512), torch.zeros(12, 128, 4, 4)
    for row, col, val in ((0, 0, 6), (0, 0, -1), (1, 0, 120)):
        t = pir.crafted_table(1, 0)
        t[row, 0, col] = val
        with pytest.raises(wp._lib.EtpError):
            wp._waypoint_tail_mode(net, _Tail(t), rgb, dep, 1, False, None, None)
    net.pano_inputs_capacity = 13                             # "edges" needs 14 rows
    with pytest.raises(ValueError):
        wp._waypoint_tail_mode(net, _Tail(pir.crafted_table(1, 0)), rgb, dep, 1, False, None, None)
    net.pano_inputs_capacity = 14
    assert wp._waypoint_tail_mode(net, _Tail(pir.crafted_table(1, 0)), rgb, dep, 1, False, None, None)["pano_inputs"] == "launched"


def test_case_list_holds_what_the_kernel_can_get_wrong():
    pir.assert_case_conditions()
    assert len(pir.cases()) == len(pir.B_LIST) * len(pir.DIMS)


def test_angle_table_is_the_per_episode_call_bit_for_bit():
    assert pir.angle_table_identity() == 0
    cand_tab, pano_tab = pir.tables()
    assert cand_tab.shape == (120, 4) and pano_tab.shape == (12, 4) and cand_tab.dtype == pano_tab.dtype == np.float32


def test_malformed_episodes_are_flagged_and_left_alone():
    t = pir.crafted_table(8, 0)
    t[0, 1, 0], t[0, 2, 0], t[1, 4, 2] = 6, -1, 120            # count 6, count -1, angle 120 (episode 4: "distinct")
    rgb, dep, _ = pir.make_inputs(8, (16, 8, 16))
    ref = pir.pano_inputs(rgb, dep, t, False, 15)              # V = 15: episode 3 ("one_view", 16 rows) does not fit
    assert ref["status"].tolist() == [0, pir.ERR_COUNT, pir.ERR_COUNT, pir.ERR_VIEWS, pir.ERR_ANGLE, 0, 0, 0]
    assert ref["written"].tolist() == [True, False, False, False, False, True, True, True]
    assert wp.host_view_lens(t, False).tolist()[:5] == [14, -1, -1, 16, -1]
    assert (wp.PINPUTS_ERR_COUNT, wp.PINPUTS_ERR_ANGLE, wp.PINPUTS_ERR_VIEWS) == (pir.ERR_COUNT, pir.ERR_ANGLE, pir.ERR_VIEWS)


def _as_kernel_output(ref):
    got = {k: v.copy() for k, v in ref.items()}
    got["dep_fts"] = ref["dep_fts"].astype(np.float32)
    return got


@pytest.mark.parametrize("mutation", pir.MUTATIONS)
def test_comparator_rejects_every_planted_mutation(mutation):
    """the correct restatement, rounded to fp32, passes; the mutated one is rejected on at least one case of the GPU list"""
    rejected = 0
    for B, dims, shift in pir.cases():
        if B > 8:
            continue
        table = pir.crafted_table(B, shift)
        rgb, dep, cc = pir.make_inputs(B, dims)
        for in_train in (False, True):
            for V in (pir.ref_length(table, in_train), 16, 20):
                ref = pir.pano_inputs(rgb, dep, table, in_train, V)
                pir.check(f"correct B{B} {dims} V{V}", _as_kernel_output(ref), ref, cc)
                bad = pir.pano_inputs(rgb, dep, table, in_train, V, mutate=mutation)
                try:
                    pir.check(f"{mutation} B{B} {dims} V{V}", _as_kernel_output(bad), ref, cc)
                except AssertionError:
                    rejected += 1
    assert rejected > 0, mutation
