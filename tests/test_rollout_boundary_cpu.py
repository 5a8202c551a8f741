"""CPU-side checks of the rollout layer's boundary (in the style of tests/test_train_log_boundary_cpu.py): the entry points of
csrc/rollout_loss.hip are declared and exported with the header's citations, every refusal the header lists comes back as
ETP_ERR_INVALID without a GPU (nothing is launched: the operands are addresses that are never read), the host layer fails loudly where
a launch is needed, tests/rollout_ref.ScriptedEnvs offers the environment protocol, and the driver's control flow -- the pause
bookkeeping, not_done_index, the last step's forced stop, the early return when every environment is paused -- runs over stand-in
components."""
import ctypes
import struct
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from etpnav_amd import _lib, build, rollout
from tests import rollout_ref as rr

P = 0x10000          # an aligned address; never dereferenced by a refused call
FWD_ARGS = ["logits", "labels", "B", "G", "ignore_index", "rec", "row_nll"]
LOSS_ARGS = ["rec", "ml_weight", "loss", "log"]
BWD_ARGS = ["logits", "labels", "B", "G", "ignore_index", "rec", "ml_weight", "upstream", "dlogits"]
SCALARS = dict(B=3, G=5, ignore_index=-100, ml_weight=0.5)
ADDR = dict(logits=P, labels=P + 0x1000, rec=P + 0x2000, row_nll=P + 0x3000, loss=P + 0x4000, log=P + 0x5000, upstream=P + 0x6000,
            dlogits=P + 0x7000)


def call(name, args, **kw):
    a = {k: ADDR[k] for k in args if k in ADDR}
    a.update({k: v for k, v in SCALARS.items() if k in args})
    a.update(kw)
    return getattr(_lib.lib(), name)(*[a[k] for k in args], None)


def test_symbols_records_and_citations():
    protos = _lib.parse_header()
    for name, nargs in (("etp_rollout_ce_fwd", 8), ("etp_rollout_loss", 5), ("etp_rollout_ce_bwd", 10)):
        assert name in _lib.declared_symbols() and hasattr(_lib.lib(), name) and len(protos[name][1]) == nargs, name
    assert protos["etp_rollout_loss"][1][1] is ctypes.c_double and protos["etp_rollout_ce_bwd"][1][6] is ctypes.c_double
    assert protos["etp_rollout_ce_fwd"][1][4] is ctypes.c_int64
    hdr = open(_lib.HEADER).read()
    for s in ("} etp_rollout_record;", "} etp_rollout_log;"):
        assert s in hdr, s
    assert (rollout.RECORD_BYTES, rollout.LOG_BYTES) == (64, 24)
    assert [struct.calcsize(f) for f in (rollout.RECORD_FMT, rollout.LOG_FMT)] == [64, 24]
    doc = hdr[hdr.index("Fine-tuning rollout loss"):hdr.index("int etp_rollout_ce_bwd")]
    for cite in ("ss_trainer_ETP.py:820, :892, :1055-1057", "no atomics", "etp_sap_eval's order", "n_actions == 0 gives exactly 0"):
        assert cite in doc, cite
    rec = rollout.unpack_record(struct.pack(rollout.RECORD_FMT, 1.5, 12, 9, 5, 1, 0, 0, 0))
    assert rec == {"loss_sum": 1.5, "n_actions": 12, "n_counted": 9, "n_steps": 5, "n_nonfinite": 1}


FWD_REFUSALS = {"NULL logits": dict(logits=None), "NULL labels": dict(labels=None), "NULL rec": dict(rec=None), "B 0": dict(B=0),
                "B -1": dict(B=-1), "G 0": dict(G=0), "logits off by 2": dict(logits=P + 2), "labels off by 4": dict(labels=P + 0x1004),
                "rec off by 4": dict(rec=P + 0x2004), "row_nll off by 1": dict(row_nll=P + 0x3001), "row_nll inside rec": dict(row_nll=P + 0x2008),
                "rec inside row_nll": dict(row_nll=P + 0x2000 - 8)}
LOSS_REFUSALS = {"NULL rec": dict(rec=None), "NULL loss": dict(loss=None), "rec off by 4": dict(rec=P + 0x2004), "loss off by 2": dict(loss=P + 0x4002),
                 "log off by 4": dict(log=P + 0x5004), "loss is rec": dict(loss=P + 0x2000), "loss inside rec": dict(loss=P + 0x2000 + 60),
                 "log overlaps rec": dict(log=P + 0x2000 + 56), "loss inside log": dict(loss=P + 0x5000 + 16)}
BWD_REFUSALS = {"NULL logits": dict(logits=None), "NULL labels": dict(labels=None), "NULL rec": dict(rec=None), "NULL dlogits": dict(dlogits=None),
                "B 0": dict(B=0), "G 0": dict(G=0), "G -2": dict(G=-2), "dlogits off by 2": dict(dlogits=P + 0x7002),
                "upstream off by 1": dict(upstream=P + 0x6001), "rec off by 4": dict(rec=P + 0x2004), "labels off by 4": dict(labels=P + 0x1004),
                "logits off by 1": dict(logits=P + 1), "dlogits over rec": dict(dlogits=P + 0x2000 - 16)}


@pytest.mark.parametrize("name", list(FWD_REFUSALS))
def test_forward_refusals_come_back_before_anything_is_launched(name):
    assert call("etp_rollout_ce_fwd", FWD_ARGS, **FWD_REFUSALS[name]) == -1, name
    assert b"rollout_ce_fwd" in _lib.lib().etp_last_error()


@pytest.mark.parametrize("name", list(LOSS_REFUSALS))
def test_loss_refusals_come_back_before_anything_is_launched(name):
    assert call("etp_rollout_loss", LOSS_ARGS, **LOSS_REFUSALS[name]) == -1, name
    assert b"rollout_loss" in _lib.lib().etp_last_error()


@pytest.mark.parametrize("name", list(BWD_REFUSALS))
def test_backward_refusals_come_back_before_anything_is_launched(name):
    assert call("etp_rollout_ce_bwd", BWD_ARGS, **BWD_REFUSALS[name]) == -1, name
    assert b"rollout_ce_bwd" in _lib.lib().etp_last_error()


@pytest.mark.skipif(torch.cuda.is_available(), reason="CPU-only check")
def test_host_layer_fails_loudly_without_gpu():
    for make in (lambda: rollout.RolloutLoss("cpu"), lambda: rollout.RolloutLoss(), lambda: rollout.RolloutLog("cpu"), lambda: rollout.RolloutLog()):
        with pytest.raises(_lib.EtpError):
            make()
    comp = rollout.Components()
    with pytest.raises(_lib.EtpError):
        comp.loss("cpu")
    # the default components are the package's routes: each needs the device when it first launches
    envs = rr.ScriptedEnvs([[0, 0, 0]], [[5, 0, 0]])
    drv = rollout.RolloutDriver(StubNet(1), None, envs, rollout.RolloutConfig(max_len=2, hidden=768), obs_batch, "cpu")
    with pytest.raises(_lib.EtpError):
        drv.rollout("train", 1.0, 0.5)


def test_add_after_total_raises_before_anything_is_launched():
    loss = rollout.RolloutLoss.__new__(rollout.RolloutLoss)          # no device: the refusal comes before any launch
    loss._closed = True
    with pytest.raises(RuntimeError, match="after total"):
        loss.add(torch.zeros(2, 3), [0, 1])
    with pytest.raises(RuntimeError, match="already taken"):
        loss.total(1.0)


def test_build_lists_the_file_with_its_flags_and_the_source_has_no_atomics():
    assert "rollout_loss.hip" in build.SOURCES and "rollout_loss.hip" in build.NO_PACKED_FP32
    assert "-fno-slp-vectorize" in build.PER_SOURCE_FLAGS["rollout_loss.hip"] and "-ffp-contract=off" in build.PER_SOURCE_FLAGS["rollout_loss.hip"]
    src = open(build.CSRC + "/rollout_loss.hip").read()
    code = "\n".join(line.split("//")[0] for line in src.splitlines())
    assert "atomic" not in code and "__shared__" in code


# ---- the environment protocol -----------------------------------------------------------------------------------------------------------
def test_scripted_envs_offer_the_protocol():
    envs, ref = rr.plan_envs()
    for name in ("num_envs", "resume_all", "reset", "step", "pause_at", "current_episodes", "call", "call_at"):
        assert hasattr(envs, name), name
    envs.resume_all()
    obs = envs.reset()
    assert envs.num_envs == 4 == len(obs) and all("instruction" in o for o in obs)
    assert [e.episode_id for e in envs.current_episodes()] == ["r0e0", "r0e1", "r0e2", "r0e3"] and set(ref) == {f"r0e{s}" for s in range(4)}
    po = envs.call(["get_pos_ori"] * 4)
    assert [p.tolist() for p, _ in po] == [rr.PLAN[s]["start"] for s in range(4)] and all(o == 0.0 for _, o in po)
    assert envs.call_at(1, "current_dist_to_goal") == pytest.approx(np.linalg.norm([2, 0, 2.5]))
    assert envs.call_at(0, "point_dist_to_goal", {"pos": [8, 0, 0]}) == pytest.approx(1.0)
    assert envs.call_at(2, "get_cand_real_pos", {"angle": 0.0, "forward": 2.0}).tolist() == [40.0, 0.0, -2.0]
    assert envs.call_at(3, "ghost_dist_to_ref", {"ghost_vp_pos": [("g0", [62, 0, 0]), ("g2", [58, 0, 0.1])], "ref_path": ref["r0e3"]}) == "g2"
    stop = lambda p: {"action": {"act": 0, "stop_pos": p}}
    go = lambda p: {"action": {"act": 4, "ghost_pos": p}}
    out = envs.step([go([1, 0, 0]), stop([20, 0, 0]), go([41, 0, 0]), stop([60, 0, 0])])
    assert [o[2] for o in out] == [False, True, False, True] and out[0][3]["steps_taken"] == 1
    assert out[0][3]["position"]["distance"][-1] == pytest.approx(np.linalg.norm([7, 0, 1]))
    envs.pause_at(3); envs.pause_at(1)
    assert envs.num_envs == 2 and [e.slot for e in envs.current_episodes()] == [0, 2]
    assert envs.call(["get_pos_ori"] * 2)[1][0].tolist() == [41.0, 0.0, 0.0]
    envs.resume_all()
    assert envs.num_envs == 4 and len(envs.reset()) == 4 and envs.current_episodes()[0].episode_id == "r1e0"


# ---- the driver over stand-in components ----------------------------------------------------------------------------------------------
def obs_batch(observations):
    return {"instruction": torch.from_numpy(np.stack([o["instruction"] for o in observations])),
            "slot": torch.tensor([o["slot"] for o in observations])}


class StubNet:
    """the four modes with the shapes the driver hands on; the text embedding of environment s is filled with s, so the rows the
    navigation call receives name the environments that are still running"""

    def __init__(self, n):
        self.calls, self.nav_slots, self.grad = [], [], []
        self.fuse_pano_inputs = False
        self.w = torch.nn.Parameter(torch.ones(()))

    def train(self):
        self.calls.append("train()")

    def __call__(self, mode=None, **kw):
        self.calls.append(mode)
        self.grad.append(torch.is_grad_enabled())
        if mode == "language":
            ids = kw["txt_ids"]
            return torch.arange(ids.shape[0], dtype=torch.float32)[:, None, None].expand(ids.shape[0], ids.shape[1], 4).contiguous()
        if mode == "waypoint":
            B = kw["observations"]["instruction"].shape[0]
            assert kw["observations"]["slot"].shape[0] == B
            return {"cand_angles": [[0.0]] * B, "cand_distances": [[2.0]] * B, "B": B, "in_train": kw["in_train"]}
        if mode == "panorama":
            B = kw["rgb_fts"].shape[0]
            return torch.zeros(B, 2, 4), torch.ones(B, 2, dtype=torch.bool)
        if mode == "navigation":
            self.nav_slots.append([int(v) for v in kw["txt_embeds"][:, 0, 0].tolist()])
            assert kw["txt_masks"].shape[0] == kw["txt_embeds"].shape[0] == kw["gmap_masks"].shape[0]
            return {"global_logits": self.w * torch.zeros(kw["gmap_masks"].shape[0], 3)}
        raise NotImplementedError(mode)


class StubComponents(rollout.Components):
    def __init__(self, stop_at):
        self.stop_at, self.calls, self.adds = stop_at, [], []

    def maps(self, num_envs, device, has_real_pos, loc_noise, merge_ghost, ghost_aug):
        comp = self
        self.calls.append(("maps", num_envs, has_real_pos, ghost_aug))

        class Maps:
            active = list(range(num_envs))
            gmaps = property(lambda m: [SimpleNamespace(ghost_real_pos={"g0": [[0.0, 0.0, 0.0]]}, slot=s) for s in m.active])

            def identify_node(m, cur_pos, cur_heading, ang, dis):
                assert len(cur_pos) == len(cur_heading) == len(ang) == len(m.active)
                return ["0"] * len(m.active), [["0_0"]] * len(m.active), [[np.zeros(3)]] * len(m.active)

            def update(m, prev_vp, step_ids, cur_vp, cur_pos, cur_heading, cand_pos, cur_rows, cand_rows, cand_real_pos=None, generator=None):
                assert len(prev_vp) == len(cur_vp) == len(cur_rows) == len(cand_real_pos) == len(m.active)
                comp.calls.append(("update", step_ids, list(m.active), cand_real_pos[0] is not None))

            def nav_inputs(m):
                B = len(m.active)
                return {"gmap_masks": torch.ones(B, 3, dtype=torch.bool), "compact": {}, "no_vp_left": [False] * B,
                        "gmap_vp_ids": [[None, "0", "g0"]] * B}

            def img_fts(m, store, G):
                return torch.zeros(len(m.active), G, 4)

            def pause(m, i):
                comp.calls.append(("pause", "maps", i, m.active.pop(i)))
        return Maps()

    def store(self, capacity_rows, hidden, device):
        self.calls.append(("store", capacity_rows, hidden))
        comp = self

        class Store:
            def append(s, pano_embeds, pano_masks, nav_types, n_cand):
                B = pano_embeds.shape[0]
                return list(range(B)), [[B + i] for i in range(B)]

            def check(s):
                comp.calls.append(("store.check",))
        return Store()

    def decider(self, num_envs, device, back_algo, consume_ghost, tryout, max_len):
        comp = self

        class Decider:
            active, prev_vp = list(range(num_envs)), [None] * num_envs

            def decide(d, nav_logits, gmaps, cur_vp, stepk, feedback, sample_ratio=None, teacher_actions=None, generator=None, uniforms=None,
                       compact=None):
                comp.calls.append(("decide", stepk, feedback, list(d.active), teacher_actions))
                acts = []
                for s in d.active:
                    stop = comp.stop_at.get(s) == stepk or stepk == max_len - 1          # RolloutDecider's force_stop
                    acts.append({"action": {"act": 0, "stop_pos": [0.0, 0.0, 0.0]} if stop else {"act": 4, "ghost_pos": [float(stepk + 1), 0.0, 0.0]}})
                return np.array([a["action"]["act"] for a in acts]), acts

            def pause(d, i):
                d.prev_vp.pop(i)
                comp.calls.append(("pause", "decider", i, d.active.pop(i)))
        return Decider()

    def loss(self, device):
        comp = self

        class Loss:
            closed = False

            def add(l, nav_logits, teacher):
                assert not l.closed
                comp.adds.append((int(nav_logits.shape[0]), list(teacher)))
                l.acc = getattr(l, "acc", 0.0) + nav_logits.sum() + float(nav_logits.shape[0])

            def total(l, ml_weight, log=None):
                l.closed = True
                v = ml_weight * l.acc
                if log is not None:
                    log.values.append(float(v.detach()) if torch.is_tensor(v) else float(v))
                return v
        return Loss()

    def log(self, device):
        class Log:
            values = []

            def reset(l):
                l.values = []

            def read(l):
                return float(np.mean(l.values))
        return Log()

    def vp_feature_variable(self, wp_outputs, device):
        B = wp_outputs["B"]
        return {"rgb_fts": torch.zeros(B, 2, 4), "dep_fts": torch.zeros(B, 2, 4), "loc_fts": torch.zeros(B, 2, 4),
                "nav_types": torch.ones(B, 2, dtype=torch.int64), "view_lens": torch.full((B,), 2)}


def make_driver(stop_at, n=3, max_len=6, **kw):
    envs = rr.ScriptedEnvs([[10.0 * s, 0, 0] for s in range(n)], [[10.0 * s + 9, 0, 0] for s in range(n)])
    net, comp = StubNet(n), StubComponents(stop_at)
    drv = rollout.RolloutDriver(net, "predictor", envs, rollout.RolloutConfig(max_len=max_len, hidden=4, waypoint_aug=True), obs_batch, "cpu",
                                components=comp, **kw)
    return drv, envs, net, comp


def test_environments_finish_at_steps_1_3_and_the_last():
    done = []
    drv, envs, net, comp = make_driver({0: 1, 1: 3}, on_done=lambda slot, ep, info, view: done.append((slot, ep.episode_id, info["steps_taken"], view.slot)))
    loss = drv.rollout("train", 0.5, 0.25)
    assert drv.steps_run == 6 and envs.num_envs == 0
    assert net.nav_slots == [[0, 1, 2], [0, 1, 2], [1, 2], [1, 2], [2], [2]]          # not_done_index gathers the text rows
    assert [c[3] for c in comp.calls if c[0] == "decide"] == net.nav_slots
    assert [c[1:3] for c in comp.calls if c[0] == "update"] == [(k + 1, s) for k, s in enumerate(net.nav_slots)]
    assert all(c[3] for c in comp.calls if c[0] == "update")                          # training: the candidates' real positions are asked for
    assert done == [(0, "r0e0", 2, 0), (1, "r0e1", 4, 1), (2, "r0e2", 6, 2)]              # once per episode, the ORIGINAL slot, its own view
    assert [a[0] for a in comp.adds] == [3, 3, 2, 2, 1, 1] and all(a[1] == [2] * a[0] for a in comp.adds)   # far from the goal: the ghost's column
    assert float(loss) == 0.5 * 12 and drv.log.values == [6.0]
    # the pause calls reach envs, maps and decider with the same index, in the same order (:1036-1044)
    pauses = [c for c in comp.calls if c[0] == "pause"]
    assert pauses == [("pause", "maps", 0, 0), ("pause", "decider", 0, 0), ("pause", "maps", 0, 1), ("pause", "decider", 0, 1),
                      ("pause", "maps", 0, 2), ("pause", "decider", 0, 2)]
    assert [c for c in envs.calls if c[0] == "pause_at"] == [("pause_at", 0, 0), ("pause_at", 0, 1), ("pause_at", 0, 2)]
    # statement order of one step, and the language call once before the loop
    assert net.calls[:5] == ["language", "waypoint", "panorama", "navigation", "waypoint"] and net.calls.count("language") == 1
    assert all(net.grad) and ("maps", 3, True, 0.0) in comp.calls and ("store", 6 * 3 * 17, 4) in comp.calls


def test_two_environments_that_finish_together_are_paused_from_the_back():
    drv, envs, net, comp = make_driver({0: 0, 2: 0}, max_len=3)
    drv.rollout("train", 1.0, 0.0)
    assert net.nav_slots == [[0, 1, 2], [1], [1]]
    assert [c for c in envs.calls if c[0] == "pause_at"] == [("pause_at", 2, 2), ("pause_at", 0, 0), ("pause_at", 0, 1)]
    assert [c[1:] for c in comp.calls if c[0] == "pause"][:4] == [("maps", 2, 2), ("decider", 2, 2), ("maps", 0, 0), ("decider", 0, 0)]


def test_the_last_step_forces_the_stop_and_the_loop_ends_there():
    drv, envs, net, comp = make_driver({}, n=2, max_len=4)
    drv.rollout("train", 1.0, 0.0)
    assert drv.steps_run == 4 and envs.num_envs == 0 and [c[1] for c in comp.calls if c[0] == "decide"] == [0, 1, 2, 3]
    assert [c[1] for c in envs.calls if c[0] == "step"] == [[4, 4], [4, 4], [4, 4], [0, 0]]


def test_an_all_paused_start_returns_at_once():
    drv, envs, net, comp = make_driver({}, skip_episode=lambda ep: True)
    assert drv.rollout("eval") is None
    assert net.calls == [] and comp.calls == [] and envs.num_envs == 0 and drv.steps_run == 0
    assert [c for c in envs.calls if c[0] == "pause_at"] == [("pause_at", 2, 2), ("pause_at", 1, 1), ("pause_at", 0, 0)]


def test_eval_skips_finished_episodes_builds_no_graph_and_takes_no_loss():
    done = []
    drv, envs, net, comp = make_driver({0: 0}, max_len=3, skip_episode=lambda ep: ep.slot == 1, on_done=lambda s, ep, info, v: done.append(s))
    assert drv.rollout("eval") is None
    # slot 1 is paused before the loop; the text rows are then numbered over the environments that run (:784, :809)
    assert net.nav_slots == [[0, 1], [1], [1]] and done == [0, 1] and comp.adds == [] and drv.loss is None and drv.log is None
    assert not any(net.grad) and [c[2] for c in comp.calls if c[0] == "decide"] == ["argmax"] * 3
    assert ("maps", 2, False, 0) in comp.calls and not any(c[3] for c in comp.calls if c[0] == "update")
    assert [c[4] for c in comp.calls if c[0] == "decide"] == [None] * 3              # no teacher in evaluation
    with pytest.raises(NotImplementedError):
        drv.rollout("infer")
    with pytest.raises(ValueError):
        drv.rollout("train")


def test_train_interval_is_the_reference_loop_and_reads_the_log_once():
    drv, envs, net, comp = make_driver({0: 1}, n=2, max_len=3)
    order = []
    opt = SimpleNamespace(zero_grad=lambda: order.append("zero_grad"), step=lambda: order.append(("step", float(net.w.grad))))
    logs = drv.train_interval(2, 0.5, 0.25, opt, reducer=lambda: order.append("reduce"))
    # per rollout B = 2, 2, 1: acc = 5, loss = 2.5; d loss / d w = 0 (the stub's logits are w * 0)
    assert logs == {"IL_loss": 2.5} and drv.log.values == [2.5, 2.5]
    assert order == ["zero_grad", "reduce", ("step", 0.0), "zero_grad", "reduce", ("step", 0.0)]
    assert [c for c in comp.calls if c[0] == "store.check"] == [("store.check",)] * 2 and net.calls[0] == "train()"
    assert envs.round == 1                                                            # two rollouts: two resets
