"""The fine-tuning rollout as one object (vlnce_baselines/ss_trainer_ETP.py:764-1057, :482-511): ``RolloutDriver`` is the loop of
``rollout(mode)`` for 'train' and 'eval' in the reference's statement order, composed from the routes of this package, and
``RolloutLoss`` keeps the rollout's imitation loss, its scale and the ``IL_loss`` log on the device (csrc/rollout_loss.hip), so the host
never waits for a loss value.  There is no CPU fallback: the loss and every default component need an MI355X.

    loss = RolloutLoss(device); loss.reset()                        # per rollout
    loss.add(nav_logits, teacher_actions)                           # per step: loss += F.cross_entropy(..., reduction='sum',
                                                                    #   ignore_index=-100); total_actions += num_envs   (:892, :820)
    total = loss.total(ml_weight, log=il_log)                       # ml_weight * loss / total_actions (:1055) and the log's append (:1057)
    total.backward()                                                # etp_rollout_ce_bwd per step; the scale is read on the device

    driver = RolloutDriver(net, waypoint_predictor, envs, RolloutConfig(...), obs_to_batch, device)
    logs = driver.train_interval(interval, ml_weight, sample_ratio, optimizer)      # {'IL_loss': mean over the interval}, one copy
    driver.rollout('eval')                                          # arg-max feedback under no_grad; on_done per finished episode

Environment protocol -- exactly what the reference calls on ``self.envs`` (habitat's VectorEnv offers it; nothing of habitat is imported):

    envs.num_envs                      the number of environments that are not paused
    envs.resume_all()                  :772
    envs.reset() -> [observation]      :773, one per environment
    envs.step(env_actions) -> [(observation, reward, done, info)]          :979; env_actions as RolloutDecider builds them
    envs.pause_at(i)                   :1040 (and the pre-pause of :781-790)
    envs.current_episodes() -> [episode]                                   :782, :984; ``episode.episode_id`` is read for 'ndtw'
    envs.call(names) -> [result]       names = ['get_pos_ori'] * num_envs -> (position, orientation) per environment   (:759)
    envs.call_at(i, name, kwargs=None) 'get_cand_real_pos' {'angle', 'forward'} (:856), 'current_dist_to_goal' (:282),
                                       'point_dist_to_goal' {'pos'} (:291), 'ghost_dist_to_ref' {'ghost_vp_pos', 'ref_path'} (:298)

Habitat's ``extract_instruction_tokens`` / ``batch_obs`` / ``apply_obs_transforms_batch`` (:776-779, :1050-1052) come in as one callable
``obs_to_batch(observations) -> batch`` (a dict of device tensors with 'instruction' and the rgb / depth views), and the orientation the
simulator returns becomes a heading through ``heading_of`` (the reference's ``heading_from_quaternion``; the default takes a scalar
heading as it is).  The metrics of :982-1007 and the path record of :1010-1033 are simulator data: per finished episode the driver calls
``on_done(slot, episode, info, gmap_view)`` and the caller computes them.  ``skip_episode(episode) -> bool`` gives the pre-pause of
:781-790.  ``VIDEO_OPTION`` is not covered.
"""
from __future__ import annotations

import random as _random
import struct
from dataclasses import dataclass
from typing import Callable, Dict, List, Optional, Sequence

import numpy as np
import torch

from . import _lib
from ._lib import check, ptr

RECORD_BYTES = 64           # etp_rollout_record {double loss_sum; int64 n_actions, n_counted, n_steps, n_nonfinite, reserved[3]}
LOG_BYTES = 24              # etp_rollout_log {double sum; int64 n, n_nonfinite}
RECORD_FMT, LOG_FMT = "<dqqqqqqq", "<dqq"
IGNORE_INDEX = -100         # ss_trainer_ETP.py:287, :892
_NO_GPU = "the rollout loss (etp_rollout_ce_fwd) needs an MI355X (cuda/hip device); no CPU fallback exists"


def _device(device) -> torch.device:
    dev = torch.device(device if device is not None else "cuda")
    if dev.type != "cuda" or not torch.cuda.is_available():
        raise _lib.EtpError(_NO_GPU)
    return dev if dev.index is not None else torch.device("cuda", torch.cuda.current_device())


def _stream(dev) -> int:
    return torch.cuda.current_stream(dev).cuda_stream


# ---- operator level: one launch each, nothing synchronises ------------------------------------------------------------------------
def rollout_ce_fwd(logits: torch.Tensor, labels: torch.Tensor, rec: torch.Tensor, ignore_index: int = IGNORE_INDEX,
                   row_nll: Optional[torch.Tensor] = None) -> None:
    """etp_rollout_ce_fwd: logits fp32 [B, G], labels int64 [B], rec int64 [8] (the 64-byte record), all on the device"""
    B, G = logits.shape
    check(_lib.lib().etp_rollout_ce_fwd(ptr(logits), ptr(labels), B, G, int(ignore_index), ptr(rec), ptr(row_nll), _stream(logits.device)),
          "etp_rollout_ce_fwd")


def rollout_loss(rec: torch.Tensor, ml_weight: float, loss: torch.Tensor, log: Optional[torch.Tensor] = None) -> None:
    """etp_rollout_loss: loss fp32 [1]; log int64 [3] (the 24-byte log) or None"""
    check(_lib.lib().etp_rollout_loss(ptr(rec), float(ml_weight), ptr(loss), ptr(log), _stream(rec.device)), "etp_rollout_loss")


def rollout_ce_bwd(logits: torch.Tensor, labels: torch.Tensor, rec: torch.Tensor, ml_weight: float, upstream: Optional[torch.Tensor] = None,
                   ignore_index: int = IGNORE_INDEX, dlogits: Optional[torch.Tensor] = None) -> torch.Tensor:
    """etp_rollout_ce_bwd -> dlogits fp32 [B, G]"""
    B, G = logits.shape
    if dlogits is None:
        dlogits = torch.empty(B, G, dtype=torch.float32, device=logits.device)
    check(_lib.lib().etp_rollout_ce_bwd(ptr(logits), ptr(labels), B, G, int(ignore_index), ptr(rec), float(ml_weight), ptr(upstream),
                                        ptr(dlogits), _stream(logits.device)), "etp_rollout_ce_bwd")
    return dlogits


def unpack_record(b: bytes) -> Dict[str, float]:
    s, na, nc, ns, nf = struct.unpack(RECORD_FMT, b)[:5]
    return {"loss_sum": s, "n_actions": na, "n_counted": nc, "n_steps": ns, "n_nonfinite": nf}


class RolloutLog:
    """``self.logs['IL_loss']`` of one interval (:496, :1057) as a 24-byte device record: ``RolloutLoss.total(..., log=this)`` adds a
    value without a copy, ``read`` is one device-to-host copy and gives ``np.mean`` over the values (:476) as ``sum / n``."""

    def __init__(self, device=None):
        self.buf = torch.zeros(3, dtype=torch.int64, device=_device(device))

    def reset(self) -> None:
        self.buf.zero_()

    def read_raw(self):
        """one copy -> (sum, n, n_nonfinite)"""
        return struct.unpack(LOG_FMT, self.buf.cpu().numpy().tobytes())

    def read(self) -> float:
        s, n, _ = self.read_raw()
        return s / n if n else float("nan")          # np.mean([]) is nan


class _RolloutLossFn(torch.autograd.Function):
    """the rollout's scalar loss as a function of every step's nav_logits; backward launches etp_rollout_ce_bwd per step with the
    incoming gradient as the device-side `upstream`"""

    @staticmethod
    def forward(ctx, owner, rec, ml_weight, value, steps, *logits):
        ctx.rec, ctx.ml_weight, ctx.steps, ctx.ignore_index = rec, ml_weight, steps, owner.ignore_index
        return value.reshape(()).clone()

    @staticmethod
    def backward(ctx, d_loss):
        up = d_loss.detach().to(torch.float32).reshape(1).contiguous()
        grads = []
        for i, (x, y) in enumerate(ctx.steps):
            grads.append(rollout_ce_bwd(x, y, ctx.rec, ctx.ml_weight, up, ctx.ignore_index) if ctx.needs_input_grad[5 + i] else None)
        return (None, None, None, None, None, *grads)


class RolloutLoss:
    """``loss`` and ``total_actions`` of one rollout (:807-808) on the device.  ``add`` is one launch per step, ``total`` one launch per
    rollout; neither synchronises.  With autograd on, ``total(...).backward()`` gives every step's ``nav_logits`` its gradient through
    etp_rollout_ce_bwd; under ``torch.no_grad()`` no graph is built and no logits are kept.  ``record()`` is one device-to-host copy, for
    tests and logging only."""

    def __init__(self, device=None, ignore_index: int = IGNORE_INDEX):
        self.device = _device(device)
        self.ignore_index = int(ignore_index)
        self.L = _lib.lib()
        self.reset()

    def reset(self) -> None:
        # a fresh record per rollout: the graph of an earlier rollout may still read its own in a later backward
        self.rec = torch.zeros(RECORD_BYTES // 8, dtype=torch.int64, device=self.device)
        self._steps: List[tuple] = []           # (detached fp32 logits, labels) per step, for the backward launches
        self._inputs: List[torch.Tensor] = []   # the graph's inputs: the steps' logits as handed in
        self._closed = False

    def add(self, nav_logits: torch.Tensor, teacher_actions) -> None:
        """one step (:892, :820).  ``nav_logits`` [B, G] on the device (fp32; another float dtype is cast), ``teacher_actions`` [B]: a
        tensor or a host sequence, -100 = ignored.  A stacked (T*B) call is taken as it is."""
        if self._closed:
            raise RuntimeError("RolloutLoss.add after total(): the rollout's divisor is taken; reset() starts the next rollout")
        if not (torch.is_tensor(nav_logits) and nav_logits.dim() == 2 and nav_logits.is_floating_point()):
            raise ValueError("nav_logits is a float tensor [B, G]")
        if nav_logits.device != self.device:
            raise ValueError(f"the loss lives on {self.device}; so must nav_logits")
        x = nav_logits if nav_logits.dtype == torch.float32 else nav_logits.float()
        x = x.contiguous()
        y = torch.as_tensor(teacher_actions).to(device=self.device, dtype=torch.int64).contiguous()
        if tuple(y.shape) != (x.shape[0],):
            raise ValueError(f"teacher_actions holds one label per row (got {tuple(y.shape)} for {x.shape[0]} rows)")
        xd = x.detach()
        rollout_ce_fwd(xd, y, self.rec, self.ignore_index)
        if torch.is_grad_enabled() and x.requires_grad:
            self._steps.append((xd, y))
            self._inputs.append(x)

    def total(self, ml_weight: float, log: Optional[RolloutLog] = None) -> torch.Tensor:
        """-> the rollout's loss, a scalar fp32 tensor on the device (:1055); ``log``: the value is added to it (:1057)"""
        if self._closed:
            raise RuntimeError("RolloutLoss.total was already taken for this rollout; reset() starts the next one")
        self._closed = True
        value = torch.empty(1, dtype=torch.float32, device=self.device)
        rollout_loss(self.rec, ml_weight, value, None if log is None else log.buf)
        if torch.is_grad_enabled() and self._inputs:
            return _RolloutLossFn.apply(self, self.rec, float(ml_weight), value, tuple(self._steps), *self._inputs)
        return value.reshape(())

    def record(self) -> Dict[str, float]:
        """one device-to-host copy -> loss_sum, n_actions, n_counted, n_steps, n_nonfinite"""
        return unpack_record(self.rec.cpu().numpy().tobytes())


# ---- the teacher (host) ---------------------------------------------------------------------------------------------------------------
def teacher_actions(gmaps: Sequence, batch_gmap_vp_ids: Sequence[Sequence], batch_no_vp_left: Sequence[bool], envs, expert_policy: str = "spl",
                    rng=None, ref_path: Optional[Callable] = None) -> List[int]:
    """``_teacher_action_new`` (ss_trainer_ETP.py:278-306) on the host, for both expert policies -> one label per active environment
    (0 = stop, -100 = ignored, otherwise the column of the target ghost).  ``gmaps``: GraphMapViews (or any map with
    ``ghost_real_pos``); ``rng``: what draws ``random.choice`` (a ``random.Random``; default the ``random`` module, as the reference);
    ``ref_path(episode)``: the ground-truth locations of 'ndtw' (``self.gt_data[str(episode.episode_id)]['locations']``)."""
    rng = _random if rng is None else rng
    out: List[int] = []
    cur_episodes = envs.current_episodes() if expert_policy == "ndtw" else None
    for i, (gmap_vp_ids, gmap, no_vp_left) in enumerate(zip(batch_gmap_vp_ids, gmaps, batch_no_vp_left)):
        if envs.call_at(i, "current_dist_to_goal") < 1.5:
            out.append(0)
        elif no_vp_left:
            out.append(IGNORE_INDEX)
        elif expert_policy == "spl":
            ghost_vp_pos = [(vp, rng.choice(pos)) for vp, pos in gmap.ghost_real_pos.items()]
            dist = [envs.call_at(i, "point_dist_to_goal", {"pos": p[1]}) for p in ghost_vp_pos]
            out.append(list(gmap_vp_ids).index(ghost_vp_pos[int(np.argmin(dist))][0]))
        elif expert_policy == "ndtw":
            if ref_path is None:
                raise ValueError("expert_policy 'ndtw' needs ref_path(episode): the episode's ground-truth locations")
            ghost_vp_pos = [(vp, rng.choice(pos)) for vp, pos in gmap.ghost_real_pos.items()]
            target = envs.call_at(i, "ghost_dist_to_ref", {"ghost_vp_pos": ghost_vp_pos, "ref_path": ref_path(cur_episodes[i])})
            out.append(list(gmap_vp_ids).index(target))
        else:
            raise NotImplementedError(expert_policy)
    return out


# ---- the driver ---------------------------------------------------------------------------------------------------------------------------
@dataclass
class RolloutConfig:
    """what ``rollout`` reads of the trainer's config: IL.max_traj_len (``self.max_len``), MODEL.task_type ('rxr' pads with 1, :775),
    IL.waypoint_aug, IL.ghost_aug, IL.loc_noise, MODEL.merge_ghost, MODEL.consume_ghost, IL.back_algo, IL.tryout and not ALLOW_SLIDING
    (:907), IL.expert_policy; ``hidden``: the planner's width (the embedding store's row length)"""
    max_len: int = 15
    instr_pad_id: int = 0
    waypoint_aug: bool = True
    ghost_aug: float = 0.0
    loc_noise: float = 0.5
    merge_ghost: bool = True
    consume_ghost: bool = True
    back_algo: str = "control"
    tryout: bool = True
    expert_policy: str = "spl"
    hidden: int = 768
    max_candidates: int = 16                    # per step and environment: the embedding store's capacity is max_len * num_envs * (1 + this)


class Components:
    """what the driver builds per rollout, as factories, so the control flow can run over stand-ins (tests/test_rollout_boundary_cpu.py).
    The defaults are this package's routes, unchanged."""

    def maps(self, num_envs, device, has_real_pos, loc_noise, merge_ghost, ghost_aug):
        from .graph_inputs import DeviceGraphMaps
        return DeviceGraphMaps(num_envs, device, has_real_pos, loc_noise, merge_ghost, ghost_aug)

    def store(self, capacity_rows, hidden, device):
        from .graph_inputs import EmbedStore
        return EmbedStore(capacity_rows, hidden, device)

    def decider(self, num_envs, device, back_algo, consume_ghost, tryout, max_len):
        from .decide import RolloutDecider
        return RolloutDecider(num_envs, device, back_algo, consume_ghost, tryout, max_len)

    def loss(self, device):
        return RolloutLoss(device)

    def log(self, device):
        return RolloutLog(device)

    def vp_feature_variable(self, wp_outputs, device):
        from .graph_inputs import vp_feature_variable
        return vp_feature_variable(wp_outputs, device)


class RolloutDriver:
    """``rollout(mode)`` of the reference's trainer for 'train' and 'eval' (:764-1057) and ``_train_interval`` (:482-511).

    ``net``: etpnav_amd.policy.ETP with both encoders attached (``net.fuse_pano_inputs`` is honoured: the waypoint call and
    ``vp_feature_variable`` follow it); ``waypoint_predictor``: the native BinaryDistPredictorTRM; ``envs``: the protocol of the module
    docstring; ``config``: a RolloutConfig; ``obs_to_batch``, ``heading_of``, ``on_done``, ``skip_episode``, ``ref_path``: module
    docstring.  ``rng`` draws the teacher's ``random.choice``, ``generator`` (torch) the decision's uniforms, ``noise_generator`` (numpy)
    the ghost jitter.  ``trace``: a list that receives, per step, what the step decided (tests; None = nothing is kept)."""

    def __init__(self, net, waypoint_predictor, envs, config: RolloutConfig, obs_to_batch: Callable, device=None,
                 heading_of: Optional[Callable] = None, on_done: Optional[Callable] = None, skip_episode: Optional[Callable] = None,
                 ref_path: Optional[Callable] = None, rng=None, generator=None, noise_generator=None, components: Optional[Components] = None,
                 trace: Optional[list] = None):
        self.net, self.waypoint_predictor, self.envs, self.config = net, waypoint_predictor, envs, config
        self.obs_to_batch = obs_to_batch
        self.device = torch.device(device if device is not None else "cuda")
        self.heading_of = heading_of if heading_of is not None else float
        self.on_done, self.skip_episode, self.ref_path = on_done, skip_episode, ref_path
        self.rng, self.generator, self.noise_generator = rng, generator, noise_generator
        self.components = components if components is not None else Components()
        self.trace = trace
        self.maps = self.store = self.decider = self.loss = None
        self.log = None                          # the interval's IL_loss log: made by the first training rollout
        self.steps_run = 0

    # ---- :758-762 ----
    def get_pos_ori(self):
        pos_ori = self.envs.call(["get_pos_ori"] * self.envs.num_envs)
        return [x[0] for x in pos_ori], [x[1] for x in pos_ori]

    # ---- :428-438 ----
    def _pause_envs(self, batch, envs_to_pause):
        if len(envs_to_pause) > 0:
            state_index = list(range(self.envs.num_envs))
            for idx in reversed(envs_to_pause):
                state_index.pop(idx)
                self.envs.pause_at(idx)
            for k, v in batch.items():
                batch[k] = v[state_index]
        return batch

    def rollout(self, mode: str, ml_weight: Optional[float] = None, sample_ratio: Optional[float] = None, uniforms=None):
        """one rollout.  'train': sampled feedback, -> the rollout's loss (a device scalar with autograd history; ``backward`` is the
        caller's, or ``train_interval``'s).  'eval': arg-max feedback under ``torch.no_grad()``, -> None.  ``uniforms``: per step a
        [num_envs at that step, 2] array that fixes the decision's draws (tests)."""
        if mode == "train":
            feedback = "sample"
            if ml_weight is None or sample_ratio is None:
                raise ValueError("mode 'train' needs ml_weight and sample_ratio")
        elif mode == "eval":
            feedback = "argmax"
        else:
            raise NotImplementedError(mode)
        envs = self.envs
        envs.resume_all()
        observations = envs.reset()
        batch = self.obs_to_batch(observations)
        if mode == "eval" and self.skip_episode is not None:
            env_to_pause = [i for i, ep in enumerate(envs.current_episodes()) if self.skip_episode(ep)]
            batch = self._pause_envs(batch, env_to_pause)
        if envs.num_envs == 0:
            return None
        if mode == "train":
            return self._loop(mode, feedback, batch, ml_weight, sample_ratio, uniforms)
        with torch.no_grad():
            return self._loop(mode, feedback, batch, ml_weight, sample_ratio, uniforms)

    def _loop(self, mode, feedback, batch, ml_weight, sample_ratio, uniforms):
        net, envs, cfg, dev, comp = self.net, self.envs, self.config, self.device, self.components
        train = mode == "train"
        # encode instructions (:798-805)
        all_txt_ids = batch["instruction"]
        all_txt_masks = (all_txt_ids != cfg.instr_pad_id)
        all_txt_embeds = net(mode="language", txt_ids=all_txt_ids, txt_masks=all_txt_masks)

        num_envs = envs.num_envs
        not_done_index = list(range(num_envs))
        have_real_pos = train
        ghost_aug = cfg.ghost_aug if train else 0
        self.maps = maps = comp.maps(num_envs, dev, have_real_pos, cfg.loc_noise, cfg.merge_ghost, ghost_aug)
        self.store = store = comp.store(cfg.max_len * num_envs * (1 + cfg.max_candidates), cfg.hidden, dev)
        self.decider = decider = comp.decider(num_envs, dev, cfg.back_algo, cfg.consume_ghost, cfg.tryout, cfg.max_len)
        self.loss = loss = comp.loss(dev) if train else None
        if train and self.log is None:
            self.log = comp.log(dev)
        self.steps_run = 0

        for stepk in range(cfg.max_len):
            self.steps_run += 1
            txt_masks = all_txt_masks[not_done_index]
            txt_embeds = all_txt_embeds[not_done_index]

            # cand waypoint prediction (:825-830)
            wp_outputs = net(mode="waypoint", waypoint_predictor=self.waypoint_predictor, observations=batch,
                             in_train=(train and cfg.waypoint_aug))

            # pano encoder (:833-839, :864-865)
            vp_inputs = comp.vp_feature_variable(wp_outputs, dev)
            pano_embeds, pano_masks = net(mode="panorama", **vp_inputs)
            cur_rows, cand_rows = store.append(pano_embeds, pano_masks, vp_inputs["nav_types"], [len(a) for a in wp_outputs["cand_angles"]])

            # vp_id, vp_pos of the current node and the candidates (:842-850)
            cur_pos, cur_ori = self.get_pos_ori()
            cur_heading = [self.heading_of(o) for o in cur_ori]
            cur_vp, cand_vp, cand_pos = maps.identify_node(cur_pos, cur_heading, wp_outputs["cand_angles"], wp_outputs["cand_distances"])
            if train:
                cand_real_pos = [[envs.call_at(i, "get_cand_real_pos", {"angle": ang, "forward": dis})
                                  for ang, dis in zip(wp_outputs["cand_angles"][i], wp_outputs["cand_distances"][i])]
                                 for i in range(envs.num_envs)]
            else:
                cand_real_pos = [None] * envs.num_envs
            maps.update(decider.prev_vp, stepk + 1, cur_vp, cur_pos, cur_heading, cand_pos, cur_rows, cand_rows, cand_real_pos,
                        generator=self.noise_generator)

            # navigation (:871-879)
            nav_inputs = maps.nav_inputs()
            nav_inputs["gmap_img_fts"] = maps.img_fts(store, nav_inputs["gmap_masks"].shape[1])
            compact = nav_inputs.pop("compact")
            no_vp_left = nav_inputs.pop("no_vp_left")
            nav_outs = net(mode="navigation", txt_embeds=txt_embeds, txt_masks=txt_masks, **nav_inputs)
            nav_logits = nav_outs["global_logits"]
            gmaps = maps.gmaps

            # teacher and loss (:889-892)
            teacher = None
            if train:
                teacher = teacher_actions(gmaps, nav_inputs["gmap_vp_ids"], no_vp_left, envs, cfg.expert_policy, self.rng, self.ref_path)
                loss.add(nav_logits, teacher)

            # determine action, make equiv action (:894-977)
            cpu_a_t, env_actions = decider.decide(nav_logits, gmaps, cur_vp, stepk, feedback, sample_ratio, teacher,
                                                  generator=self.generator, uniforms=None if uniforms is None else uniforms[stepk],
                                                  compact=compact)
            if self.trace is not None:
                self.trace.append(dict(stepk=stepk, slots=list(not_done_index), cur_vp=list(cur_vp), teacher=teacher, nav_logits=nav_logits.detach(),
                                       a_t=[int(a) for a in cpu_a_t], env_actions=env_actions))

            outputs = envs.step(env_actions)
            observations, _, dones, infos = [list(x) for x in zip(*outputs)]

            # finished episodes: the caller's metrics (:982-1033), then pause (:1035-1044)
            if sum(dones) > 0:
                if self.on_done is not None:
                    curr_eps = envs.current_episodes()
                    for i in range(envs.num_envs):
                        if dones[i]:
                            self.on_done(not_done_index[i], curr_eps[i], infos[i], gmaps[i])
                for i in reversed(list(range(envs.num_envs))):
                    if dones[i]:
                        not_done_index.pop(i)
                        envs.pause_at(i)
                        observations.pop(i)
                        maps.pause(i)
                        decider.pause(i)

            if envs.num_envs == 0:
                break

            # obs for next step (:1049-1052)
            batch = self.obs_to_batch(observations)

        if train:
            return loss.total(ml_weight, log=self.log)          # :1055-1057
        return None

    def check(self) -> None:
        """what only the device saw during the last rollout, raised in one copy (EmbedStore.check); call it after the backward"""
        if self.store is not None:
            self.store.check()

    def train_interval(self, interval: int, ml_weight: float, sample_ratio: float, optimizer, reducer: Optional[Callable] = None) -> Dict[str, float]:
        """``_train_interval`` (:482-511): per iteration zero the gradients, run the rollout, backward, (``reducer()``: the gradient
        exchange of a data-parallel run), ``optimizer.step()`` -- FusedAdamW or any torch optimizer.  -> {'IL_loss': np.mean over the
        interval} read in ONE device-to-host copy at the end; no loss value is copied before."""
        if hasattr(self.net, "train"):
            self.net.train()                                    # :483; the frozen encoders keep their own mode (:485-490)
        for enc in (getattr(self.net, "rgb_encoder", None), getattr(self.net, "depth_encoder", None), self.waypoint_predictor):
            if hasattr(enc, "eval"):
                enc.eval()
        if self.log is not None:
            self.log.reset()                                    # self.logs = defaultdict(list) (:496)
        for _ in range(interval):
            optimizer.zero_grad()
            loss = self.rollout("train", ml_weight, sample_ratio)
            if loss is None:
                continue
            loss.backward()
            if reducer is not None:
                reducer()
            optimizer.step()
            self.check()
        return {"IL_loss": self.log.read() if self.log is not None else float("nan")}
