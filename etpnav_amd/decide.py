"""The rollout decision (the last stage of a rollout step): node logits -> environment actions.

The reference's trainer, after ``forward_navigation`` (vlnce_baselines/ss_trainer_ETP.py:880-977): softmax, one ``.item()`` per
episode for ``gmap.node_stop_scores``, ``Categorical.sample`` / ``rand_like`` / ``where`` (or ``argmax``), a ``.cpu()``, and a Python
loop over ``gmap.shortest_path`` / ``front_to_ghost_dist`` / ``node_stop_scores`` -- B + 1 host synchronisations and, behind
``shortest_path``, networkx all-pairs Dijkstra after every graph update.  Here: one launch (``etp_nav_decide``, csrc/decide.hip)
on the compact graph arrays ``nav_gmap_variable`` uploaded anyway, and ONE device-to-host copy of an int32 record per episode.

    decider = RolloutDecider(num_envs, device, back_algo, consume_ghost, tryout, max_len)      # once per rollout; reset() to reuse
    nav_inputs = nav_gmap_variable(gmaps, cur_vp, cur_pos, cur_heading, device, keep_compact=True)
    cpu_a_t, env_actions = decider.decide(nav_logits, gmaps, cur_vp, stepk, feedback, sample_ratio, teacher_actions,
                                          compact=nav_inputs.pop("compact"))
    ... decider.prev_vp is the trainer's prev_vp; decider.pause(i) beside envs.pause_at(i)

``feedback == 'sample'`` draws by inverse CDF from two uniforms per episode (``uniforms`` [B,2], or ``torch.rand`` with ``generator``):
the distribution of ``Categorical.sample`` and of ``rand_like(...) <= sample_ratio``, not torch's random stream.
"""
from __future__ import annotations

from typing import List, Optional, Sequence

import numpy as np
import torch

from . import _lib
from ._lib import check, ptr
from .graph_inputs import MAX_NODES, pack_batch, pack_episode

HDR = 8                                   # ETP_DECIDE_HDR
STOP, ERR_ACTION, ERR_UNREACHABLE, ERR_INPUT = 1, 2, 4, 8      # ETP_DECIDE_*
COMPACT_KEYS = ("node_pos", "n_nodes", "adj", "ghost_pos", "n_ghost", "front_ptr", "front_idx", "cur_node")


def pack_for_decide(gmaps: Sequence, cur_vp: Sequence[str]) -> dict:
    """the compact arrays of ``pack_batch`` the decision reads (the pose is not among them)"""
    zero = np.zeros(3)
    return pack_batch([pack_episode(g, cur_vp[i], zero, 0.0) for i, g in enumerate(gmaps)])


def nav_decide(logits: torch.Tensor, compact: dict, slot: torch.Tensor, stop_scores: torch.Tensor,
               uniforms: Optional[torch.Tensor] = None, teacher: Optional[torch.Tensor] = None, sample_ratio: float = 0.0,
               force_stop: bool = False, record: Optional[torch.Tensor] = None) -> torch.Tensor:
    """One launch of etp_nav_decide -> record [B, HDR + Nmax] int32 on the device (layout: include/etpnav_hip.h).  ``compact``: device
    tensors of ``pack_batch`` with its ``_dims``; ``stop_scores`` [S,64] fp32 is updated in place."""
    if logits.device.type != "cuda":
        raise _lib.EtpError("etp_nav_decide needs an MI355X (cuda/hip device); no CPU fallback exists")
    L = _lib.lib()
    B, Nmax, Mmax, Fmax = compact["_dims"]
    if logits.dim() != 2 or logits.shape[0] != B or logits.dtype != torch.float32:
        raise ValueError(f"logits must be fp32 [B={B}, G]")
    if stop_scores.dim() != 2 or stop_scores.shape[1] != MAX_NODES or stop_scores.dtype != torch.float32:
        raise ValueError("stop_scores must be fp32 [S, 64]")
    G = int(logits.shape[1])
    if record is None:
        record = torch.empty(B, HDR + Nmax, dtype=torch.int32, device=logits.device)
    c = compact
    check(L.etp_nav_decide(ptr(logits), ptr(c["node_pos"]), ptr(c["n_nodes"]), ptr(c["adj"]), ptr(c["ghost_pos"]), ptr(c["n_ghost"]),
                           ptr(c["front_ptr"]), ptr(c["front_idx"]), ptr(c["cur_node"]), ptr(slot), ptr(uniforms), ptr(teacher),
                           float(sample_ratio), int(bool(force_stop)), B, Nmax, Mmax, Fmax, G, ptr(stop_scores),
                           int(stop_scores.shape[0]), ptr(record), torch.cuda.current_stream(logits.device).cuda_stream),
          "etp_nav_decide")
    return record


def raise_on_flags(rec: np.ndarray) -> None:
    for i, f in enumerate(rec[:, 2].tolist()):
        if f & ERR_INPUT:
            raise ValueError(f"episode {i}: graph arrays out of range (nodes, ghosts, G, cur_node, slot or fronts)")
        if f & ERR_ACTION:
            raise ValueError(f"episode {i}: action {int(rec[i, 0])} is neither 0 nor one of the episode's ghosts")
        if f & ERR_UNREACHABLE:
            raise ValueError(f"episode {i}: node {int(rec[i, 4])} cannot be reached from the current node")


def env_actions_from_record(rec: np.ndarray, gmaps: Sequence, cur_vp: Sequence[str], back_algo: str, tryout: bool) -> List[dict]:
    """The dicts of ss_trainer_ETP.py:920-974 from the records (host only, no device access)."""
    out = []
    for i, gmap in enumerate(gmaps):
        r = rec[i]
        nodes = list(gmap.node_pos.keys())
        path = [nodes[k] for k in r[HDR:HDR + int(r[6])].tolist()]
        back_path = [(vp, gmap.node_pos[vp]) for vp in path] if back_algo == "control" else None
        if int(r[2]) & STOP:
            stop_vp = nodes[int(r[3])]
            stop_pos = gmap.node_pos[stop_vp]
            out.append({"action": {"act": 0, "cur_vp": cur_vp[i], "stop_vp": stop_vp, "stop_pos": stop_pos, "back_path": back_path,
                                   "tryout": tryout},
                        "vis_info": {"nodes": list(gmap.node_pos.values()), "ghosts": list(gmap.ghost_aug_pos.values()),
                                     "predict_ghost": stop_pos}})
        else:
            ghost_vp = list(gmap.ghost_pos.keys())[int(r[5])]
            front_vp = nodes[int(r[4])]
            out.append({"action": {"act": 4, "cur_vp": cur_vp[i], "front_vp": front_vp, "front_pos": gmap.node_pos[front_vp],
                                   "ghost_vp": ghost_vp, "ghost_pos": gmap.ghost_aug_pos[ghost_vp], "back_path": back_path,
                                   "tryout": tryout},
                        "vis_info": None})
    return out


class RolloutDecider:
    """Host mirror of the decision loop.  Holds what the reference keeps in Python between steps: the stop-score table (on the
    device, one row per ORIGINAL environment), ``not_done_index`` (``active``) and ``prev_vp``."""

    def __init__(self, num_envs: int, device, back_algo: str = "control", consume_ghost: bool = True, tryout: bool = True,
                 max_len: int = 15):
        self.num_envs, self.device = int(num_envs), torch.device(device)
        self.back_algo, self.consume_ghost, self.tryout, self.max_len = back_algo, bool(consume_ghost), bool(tryout), int(max_len)
        self.stop_scores = None
        self.reset()

    def reset(self) -> None:
        if self.device.type == "cuda":
            if self.stop_scores is None:
                self.stop_scores = torch.empty(self.num_envs, MAX_NODES, dtype=torch.float32, device=self.device)
            self.stop_scores.fill_(float("-inf"))
        self.active = list(range(self.num_envs))
        self.prev_vp: List[Optional[str]] = [None] * self.num_envs

    def pause(self, i: int) -> None:
        """``not_done_index.pop(i)`` / ``prev_vp.pop(i)`` (ss_trainer_ETP.py:1036-1044); the episode's table row stays behind, unused"""
        self.active.pop(i)
        self.prev_vp.pop(i)

    def decide(self, nav_logits, gmaps, cur_vp, stepk, feedback, sample_ratio=None, teacher_actions=None, generator=None,
               uniforms=None, compact=None):
        if self.stop_scores is None:
            raise _lib.EtpError("etp_nav_decide needs an MI355X (cuda/hip device); no CPU fallback exists")
        B = len(gmaps)
        if B != len(self.active) or B != len(cur_vp):
            raise ValueError(f"{B} graphs, {len(cur_vp)} viewpoints, {len(self.active)} active environments")
        dev = self.device
        if feedback == "sample":
            if sample_ratio is None or teacher_actions is None:
                raise ValueError("feedback 'sample' needs sample_ratio and teacher_actions")
            if uniforms is None:
                uniforms = torch.rand(B, 2, device=dev, generator=generator)
            uniforms = torch.as_tensor(uniforms, dtype=torch.float32).to(dev).contiguous()
            teacher = torch.as_tensor(teacher_actions).to(device=dev, dtype=torch.int64).contiguous()
        elif feedback == "argmax":
            uniforms = teacher = None
        else:
            raise NotImplementedError(feedback)
        if compact is None:
            batch = pack_for_decide(gmaps, cur_vp)
            compact = {k: torch.from_numpy(batch[k]).to(dev) for k in COMPACT_KEYS}
            compact["_dims"] = batch["_dims"]
        slot = torch.tensor(self.active, dtype=torch.int32).to(dev)
        logits = nav_logits.detach().to(torch.float32).contiguous()
        rec = nav_decide(logits, compact, slot, self.stop_scores, uniforms, teacher, float(sample_ratio or 0.0),
                         stepk == self.max_len - 1).cpu().numpy()        # the one host synchronisation of the step
        raise_on_flags(rec)
        env_actions = env_actions_from_record(rec, gmaps, cur_vp, self.back_algo, self.tryout)
        stop_probs = rec[:, 7].copy().view(np.float32)
        for i, gmap in enumerate(gmaps):
            if hasattr(gmap, "node_stop_scores"):
                gmap.node_stop_scores[cur_vp[i]] = float(stop_probs[i])
            act = env_actions[i]["action"]
            if act["act"] == 4:
                self.prev_vp[i] = act["front_vp"]
                if self.consume_ghost:
                    gmap.delete_ghost(act["ghost_vp"])
        return rec[:, 0].astype(np.int64), env_actions
