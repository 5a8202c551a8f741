"""float64 restatement, case lists, emulations, derived bounds and scripted environments for the fine-tuning rollout loss of
csrc/rollout_loss.hip and the driver of etpnav_amd/rollout.py (tests/test_rollout_gpu.py runs them on the device,
tests/test_rollout_ref_cpu.py and tests/test_rollout_boundary_cpu.py pin, emulate and drive them without a GPU):

  rollout_ce_fwd_kernel (etp_rollout_ce_fwd), rollout_loss_kernel (etp_rollout_loss), rollout_ce_bwd_kernel (etp_rollout_ce_bwd)

A rollout is a list of steps (logits [B_t, G_t] fp32 with -inf entries, labels [B_t] int64).  The reference (ss_trainer_ETP.py:820, :892,
:1055):  N = sum_t B_t;  loss = ml_weight * sum_t sum_b nll_tb / N;  dlogits_t = (ml_weight / N) (softmax - onehot) on the kept rows.

Bounds, without a multiplier.  u = 2^-24, u53 = 2^-53, gam(k) = k u / (1 - k u), gam64(k) the same with u53.  Nothing is fitted to what a
kernel returns.

  row nll: eval_ref.nll_bound at the depth of etp_sap_eval, ceil(G / 64) + 6 (the kernel computes max / sum / lse in its order): e_row.
  loss:    the kernel adds the R = sum_t (kept rows of step t) fp32 nll values in double, one after the other, onto the record (R + T
           additions counting the per-launch add), then one double product and one double quotient, then ONE rounding to fp32:
               b = |ml_weight| / N (sum e_row + gam64(R + T + 2) sum |nll|),   bound = b + u (|loss| + b)
  dlogits: reduce_ref.ce_bounds' dlogits bound with s = ml_weight / N in place of the host scale covers lse, the exponential, the
           subtraction and the product; the kernel's s is the double quotient rounded once to fp32, which scales every element by
           (1 + d), |d| <= u (1 + u53):   bdl + u (|dlogits| + bdl) + 2 u53 |dlogits|;  one more u (|dlogits| + bdl) when an `upstream`
           that is no power of two multiplies s.  Ignored rows and -inf columns that no label points at must be exactly 0.
  counts (n_actions, n_counted, n_steps, n_nonfinite) and everything a second run returns (bit for bit): exact.
  against a torch fp32 recording (the fixture's fp32 keys) the reference's own fp32 error is added: its rows' lse at the worst-case depth
  G of any summation order, and its accumulation of B_t rows per step and T steps in fp32, gam(B + T) s sum |nll|.
"""
import json
import math
import os
import random
from types import SimpleNamespace

import numpy as np
import torch

from tests import eval_ref as er
from tests import reduce_ref as rf
from tests.reduce_ref import F64, U, cdiv, gam

F32 = torch.float32
U53 = 2.0 ** -53
IGNORE = -100
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "rollout_loss_small.npz")
WORST = {}


def gam64(k):
    return k * U53 / (1.0 - k * U53)


def within(key, got, ref, bound):
    try:
        return rf.within(key, got, ref, bound)
    finally:
        WORST[key] = max(WORST.get(key, 0.0), rf.WORST.get(key, 0.0))


def worst_table():
    rows = [f"  {k[0]:<56}{k[1]:<14}{v:8.3f}" for k, v in sorted(WORST.items())]
    return "\n".join([f"  {'case':<56}{'tensor':<14}err/bound"] + rows)


# ---- float64 restatement ---------------------------------------------------------------------------------------------------------
def reference(steps, ml_weight, ignore_index=IGNORE, upstream=1.0):
    """-> dict: loss (float), dlogits [per step, float64], q [per step: reduce_ref.ce's row pieces], N, counted, s"""
    N = sum(int(x.shape[0]) for x, _ in steps)
    s = ml_weight / N
    total, dl, qs, counted = 0.0, [], [], 0
    for x, y in steps:
        _, _, q = rf.ce(x, y, 1.0, ignore_index)
        total += float(q["nll"].sum())
        counted += int(q["keep"].sum())
        dl.append(torch.where(q["keep"][:, None], (s * upstream) * (q["p"] - q["onehot"]), torch.zeros_like(q["s"])))
        qs.append(q)
    return {"loss": ml_weight * total / N, "dlogits": dl, "q": qs, "N": N, "counted": counted, "s": s, "sum": total}


def loss_bound(r, ml_weight):
    e_rows, mag, R = 0.0, 0.0, 0
    for q in r["q"]:
        G = q["s"].shape[1]
        e_rows += float(er.nll_bound(q, er.sap_depth(G)).sum())
        mag += float(q["nll"].abs().sum())
        R += int(q["keep"].sum())
    b = abs(ml_weight) / r["N"] * (e_rows + gam64(R + len(r["q"]) + 2) * mag)
    return b + U * (abs(r["loss"]) + b)


def dlogits_bounds(r, upstream=1.0):
    out = []
    for q, ref in zip(r["q"], r["dlogits"]):
        B, G = q["s"].shape
        _, bdl = rf.ce_bounds(q, B, G, r["s"] * upstream)
        b = bdl + U * (ref.abs() + bdl) + 2 * U53 * ref.abs()
        m = math.frexp(abs(upstream))[0] if upstream else 0.5
        if m != 0.5:                       # not a power of two: the product s * upstream rounds once more
            b = b + U * (ref.abs() + bdl)
        out.append(b)
    return out


# ---- the checks both test files use ------------------------------------------------------------------------------------------------
def check_loss(name, loss, steps, ml_weight, ignore_index=IGNORE):
    r = reference(steps, ml_weight, ignore_index)
    got = torch.as_tensor(loss).detach().cpu().reshape(())
    assert got.dtype == F32, (name, got.dtype)
    if r["counted"] == 0:
        assert float(got) == 0.0, f"{name}: loss {float(got)} with every row ignored"
    t = lambda v: torch.tensor(v, dtype=F64)
    within((name, "loss"), got, t(r["loss"]), t(loss_bound(r, ml_weight)))
    return r


def check_dlogits(name, dlogits, steps, ml_weight, ignore_index=IGNORE, upstream=1.0):
    r = reference(steps, ml_weight, ignore_index, upstream)
    assert len(dlogits) == len(steps), f"{name}: {len(dlogits)} gradients for {len(steps)} steps"
    for t, (d, (x, _), q, ref, b) in enumerate(zip(dlogits, steps, r["q"], r["dlogits"], dlogits_bounds(r, upstream))):
        d = d.detach().cpu()
        assert d.dtype == F32 and tuple(d.shape) == tuple(x.shape), (name, t, d.dtype, tuple(d.shape))
        zero = (~q["keep"])[:, None] | torch.isneginf(x.cpu())
        assert bool((d[zero.expand_as(d)] == 0).all()), f"{name} step {t}: dlogits non-zero on an ignored row or in a -inf column"
        within((name, "dlogits"), d, ref, b)
    return r


def check_record(name, rec, steps, before=None, calls=None, ignore_index=IGNORE, row_nll=None):
    """rec: dict of RolloutLoss.record / unpack; counts exact; loss_sum against the float64 sum of the rows' reference nll within the
    rows' bound (or, with the kernel's own row_nll, within the double chain alone)"""
    r = reference(steps, 1.0, ignore_index)
    b0 = before or {"loss_sum": 0.0, "n_actions": 0, "n_counted": 0, "n_steps": 0, "n_nonfinite": 0}
    want = (b0["n_actions"] + r["N"], b0["n_counted"] + r["counted"], b0["n_steps"] + (len(steps) if calls is None else calls), b0["n_nonfinite"])
    got = (rec["n_actions"], rec["n_counted"], rec["n_steps"], rec["n_nonfinite"])
    assert got == want, f"{name}: counts (n_actions, n_counted, n_steps, n_nonfinite) {got}, expected {want}"
    t = lambda v: torch.tensor(v, dtype=F64)
    if row_nll is not None:
        own, mag = 0.0, abs(b0["loss_sum"])
        for (x, y), nll in zip(steps, row_nll):
            keep = y.cpu() != ignore_index
            own += float(nll.cpu().to(F64)[keep].sum())
            mag += float(nll.cpu().to(F64)[keep].abs().sum())
        within((name, "loss_sum"), t(rec["loss_sum"]), t(b0["loss_sum"] + own), t(gam64(r["counted"] + len(steps) + 1) * mag))
        return r
    e_rows = sum(float(er.nll_bound(q, er.sap_depth(q["s"].shape[1])).sum()) for q in r["q"])
    mag = abs(b0["loss_sum"]) + sum(float(q["nll"].abs().sum()) for q in r["q"])
    within((name, "loss_sum"), t(rec["loss_sum"]), t(b0["loss_sum"] + r["sum"]), t(e_rows + gam64(r["counted"] + len(steps) + 1) * mag))
    return r


# ---- fp32 emulation of the kernels' schedule; `mutate` plants one defect ----------------------------------------------------------
MUTATIONS = ("scale_n_counted", "scale_last_step", "per_step_mean", "no_ml_weight", "ml_weight_twice", "ignored_in_grad", "onehot_plus",
             "onehot_minus", "neginf_grad", "step_dropped")


def emulate(steps, ml_weight, ignore_index=IGNORE, upstream=1.0, mutate=None):
    """-> (loss fp32 tensor, [dlogits fp32], record dict): rows in etp_sap_eval's order (eval_ref.emulate_sap_eval), the kept rows added
    in row order in double, (ml_weight * sum) / N in double, one rounding; s = fp32(ml_weight / N) * upstream"""
    if mutate == "step_dropped":
        steps = steps[:1] + steps[2:] if len(steps) > 1 else steps[:0]
    acc, N, counted, nonfinite, lses = 0.0, 0, 0, 0, []
    for x, y in steps:
        x = x.cpu().to(F32)
        nll, _ = er.emulate_sap_eval(x, y.cpu(), ignore_index)
        keep = y.cpu() != ignore_index
        step_sum = 0.0
        for b in range(x.shape[0]):
            if bool(keep[b]):
                step_sum += float(nll[b])          # Python floats are doubles: the kernel's row-order additions
                counted += 1
                nonfinite += 0 if math.isfinite(float(nll[b])) else 1
        if mutate == "per_step_mean":
            step_sum = step_sum / x.shape[0]
        acc += step_sum
        N += int(x.shape[0])
    div = {"scale_n_counted": max(counted, 1), "scale_last_step": int(steps[-1][0].shape[0]) if steps else 1, "per_step_mean": 1}.get(mutate, N)
    w = {"no_ml_weight": 1.0, "ml_weight_twice": ml_weight * ml_weight}.get(mutate, ml_weight)
    loss = torch.tensor((w * acc) / div if div else 0.0, dtype=F64).to(F32)
    s = torch.tensor(w / div if div else 0.0, dtype=F64).to(F32) * torch.tensor(upstream, dtype=F32)
    dls = []
    for x, y in steps:
        x, y = x.cpu().to(F32), y.cpu()
        B, G = x.shape
        mx = x.max(-1).values
        lse = er._lse32(x, mx, 64)[:, None]
        keep = y != ignore_index
        if mutate == "ignored_in_grad":
            keep = torch.ones_like(keep)
        col = torch.where(y != ignore_index, y, torch.zeros_like(y)) + {"onehot_plus": 1, "onehot_minus": -1}.get(mutate, 0)
        onehot = torch.zeros(B, G, dtype=F32)
        ok = (col >= 0) & (col < G)
        onehot[torch.arange(B)[ok], col[ok]] = 1.0
        p = torch.exp(x - lse)
        if mutate == "neginf_grad":
            p = torch.where(torch.isneginf(x), torch.full_like(p, 1e-3), p)
        dls.append(torch.where(keep[:, None], s * (p - onehot), torch.zeros(B, G, dtype=F32)))
    rec = {"loss_sum": acc, "n_actions": N, "n_counted": counted, "n_steps": len(steps), "n_nonfinite": nonfinite}
    return loss, dls, rec


# ---- cases -------------------------------------------------------------------------------------------------------------------------------
CASE_B = (1, 7, 16, 17, 33)
CASE_G = (1, 2, 63, 64, 65, 130)
CASE_T = (1, 3, 15)
SHIFTS = (0.0, 80.0, -80.0)
IGNORED = ("none", "some", "all")
WEIGHTS = (1.0, 0.37, -2.5)
STACKED = (15, 33, 65)                      # one stacked call: T * B rows of G columns


def shrinking(B, T):
    """B_t of a T-step rollout that starts with B environments and loses them at an even pace down to one"""
    return [max(1, B - (t * B) // T) for t in range(T)]


def cases():
    """(name, B, G, T, shift, ignored, ml_weight): every (B, G) once, T / shift / ignored / weight rotating through their lists"""
    out = []
    for i, (B, G) in enumerate((b, g) for b in CASE_B for g in CASE_G):
        T, shift, ign, w = CASE_T[i % 3], SHIFTS[(i // 3) % 3], IGNORED[(i + i // 6) % 3], WEIGHTS[(i // 2) % 3]
        out.append((f"B{B} G{G} T{T} shift{shift:+.0f} ignored-{ign} w{w}", B, G, T, shift, ign, w))
    return out


def make_steps(B, G, T, shift, ign, seed, device="cpu"):
    """reduce_ref.ce_case per step: logits N(0, 3) + shift with -inf columns that no label points at (G > 2), labels at column 0 and
    G - 1, none / some / all rows ignored"""
    steps = []
    for t, Bt in enumerate(shrinking(B, T)):
        x, y, _, _ = rf.ce_case(Bt, G, (shift, ign, IGNORE, "fixed"), seed * 131 + t, device)
        steps.append((x.contiguous(), y.contiguous()))
    return steps


def stacked(steps):
    return [(torch.cat([x for x, _ in steps], 0).contiguous(), torch.cat([y for _, y in steps], 0).contiguous())]


def mutation_case():
    """a rollout on which every planted mistake shows: shrinking B, ignored rows, -inf columns, ml_weight that is neither 0 nor +-1"""
    steps = make_steps(7, 9, 3, 0.0, "some", 77)
    assert [int(x.shape[0]) for x, _ in steps] == [7, 5, 3] and any(bool((y == IGNORE).any()) for _, y in steps)
    assert all(bool(torch.isneginf(x).any()) for x, _ in steps)
    return steps, 0.37


# ---- the fixture ---------------------------------------------------------------------------------------------------------------------------
def load_fixture(path=GOLDEN):
    z = np.load(path, allow_pickle=False)
    meta = json.loads(str(z["meta"]))
    steps = [(torch.from_numpy(z[f"logits_{t}"]), torch.from_numpy(z[f"labels_{t}"])) for t in range(meta["T"])]
    return z, meta, steps


def fixture_fp32_bounds(r, ml_weight):
    """what is added against the torch fp32 recording: (loss, [dlogits]) -- the reference's own rows at the worst-case depth G and its
    fp32 accumulation over B rows and T steps"""
    s, T = abs(r["s"]), len(r["q"])
    e_rows, mag, Bmax, dl = 0.0, 0.0, 0, []
    for q, ref in zip(r["q"], r["dlogits"]):
        B, G = q["s"].shape
        e_rows += float(er.nll_bound(q, G + 6).sum())
        mag += float(q["nll"].abs().sum())
        Bmax = max(Bmax, B)
        fin = torch.isfinite(q["s"])
        span = torch.where(fin, (q["s"] - q["mx"]).abs(), torch.zeros_like(q["s"])).max(-1, keepdim=True).values
        e_lse = (2 * U + U * span) + gam(G + 6) + 2 * U * torch.log(q["sum"]).abs() + U * q["lse"].abs()
        sl = torch.where(fin, (q["s"] - q["lse"]).abs(), torch.zeros_like(q["s"]))
        b = s * (q["p"] * (e_lse + U * sl + 2 * U) + 4 * U * (q["p"] - q["onehot"]).abs())
        dl.append(torch.where(q["keep"][:, None], b, torch.zeros_like(b)))
    return s * e_rows + gam(Bmax + T + 2) * s * mag + U * abs(r["loss"]), dl


# ---- scripted environments ---------------------------------------------------------------------------------------------------------------
class Episode(SimpleNamespace):
    pass


class ScriptedEnvs:
    """The environment protocol of etpnav_amd/rollout.py over point agents: an agent teleports to ``ghost_pos`` (act 4) or ``stop_pos``
    (act 0) and is done on ``act == 0``; distances are Euclidean to the episode's goal; observations come from ``make_obs(slot, step,
    pos)`` (default: a token row drawn from the seed).  Every distance a query returned is appended to ``queries``."""

    def __init__(self, starts, goals, seed=0, make_obs=None, ref_paths=None, text_len=8, vocab=50):
        self.starts = [np.asarray(p, dtype=np.float64) for p in starts]
        self.goals = [np.asarray(p, dtype=np.float64) for p in goals]
        self.ref_paths = ref_paths
        self.seed, self.make_obs, self.text_len, self.vocab = seed, make_obs, text_len, vocab
        self.n_total = len(self.starts)
        self.round = -1
        self.active = list(range(self.n_total))
        self.pos = [p.copy() for p in self.starts]
        self.steps = [0] * self.n_total
        self.paths = [[] for _ in range(self.n_total)]
        self.queries, self.calls = [], []

    @property
    def num_envs(self):
        return len(self.active)

    def resume_all(self):
        self.calls.append(("resume_all",))
        self.active = list(range(self.n_total))

    def _obs(self, s):
        if self.make_obs is not None:
            return self.make_obs(s, self.steps[s], self.pos[s])
        g = np.random.default_rng([self.seed, max(self.round, 0), s])
        ids = g.integers(2, self.vocab, self.text_len)
        ids[self.text_len - 1 - (s % 3):] = 0                  # padding of different lengths
        return {"instruction": ids.astype(np.int64), "slot": s, "step": self.steps[s]}

    def reset(self):
        self.calls.append(("reset",))
        self.round += 1
        self.pos = [p.copy() for p in self.starts]
        self.steps = [0] * self.n_total
        self.paths = [[p.copy()] for p in self.starts]
        return [self._obs(s) for s in self.active]

    def current_episodes(self):
        return [Episode(episode_id=f"r{self.round}e{s}", slot=s) for s in self.active]

    def pause_at(self, i):
        self.calls.append(("pause_at", i, self.active[i]))
        self.active.pop(i)

    def step(self, actions):
        assert len(actions) == len(self.active), (len(actions), len(self.active))
        self.calls.append(("step", [a["action"]["act"] for a in actions]))
        out = []
        for s, a in zip(self.active, actions):
            act = a["action"]
            self.pos[s] = np.asarray(act["stop_pos"] if act["act"] == 0 else act["ghost_pos"], dtype=np.float64).copy()
            self.steps[s] += 1
            self.paths[s].append(self.pos[s].copy())
            dist = [float(np.linalg.norm(p - self.goals[s])) for p in self.paths[s]]
            info = {"steps_taken": self.steps[s], "position": {"position": [p.tolist() for p in self.paths[s]], "distance": dist},
                    "collisions": {"count": 0}}
            out.append((self._obs(s), 0.0, act["act"] == 0, info))
        return out

    def call(self, names):
        assert list(names) == ["get_pos_ori"] * len(self.active), names
        return [(self.pos[s].copy(), 0.0) for s in self.active]

    def call_at(self, i, name, kwargs=None):
        s = self.active[i]
        if name == "current_dist_to_goal":
            d = float(np.linalg.norm(self.pos[s] - self.goals[s]))
        elif name == "point_dist_to_goal":
            d = float(np.linalg.norm(np.asarray(kwargs["pos"], dtype=np.float64) - self.goals[s]))
        elif name == "get_cand_real_pos":
            a, f = float(kwargs["angle"]), float(kwargs["forward"])
            return self.pos[s] + np.array([-f * np.sin(a), 0.0, -f * np.cos(a)])
        elif name == "ghost_dist_to_ref":
            ref = np.asarray(kwargs["ref_path"], dtype=np.float64).reshape(-1, 3)
            ds = [float(np.linalg.norm(ref - np.asarray(p, dtype=np.float64), axis=1).min()) for _, p in kwargs["ghost_vp_pos"]]
            self.queries.append((s, name, ds))
            return kwargs["ghost_vp_pos"][int(np.argmin(ds))][0]
        else:
            raise NotImplementedError(name)
        self.queries.append((s, name, d))
        return d


# ---- the scripted rollout of the fixture (tools/make_golden_rollout_loss.py records it on the real GraphMap) -------------------------------
# per slot: start, goal, and per step the candidates' positions and where the agent goes (a ghost's position, or None = stop)
PLAN = {
    0: dict(start=[0, 0, 0], goal=[8, 0, 1],
            cands=[[[2, 0, 0], [0, 0, 2]], [[4, 0, 0], [0.2, 0, 2.1]], [[6, 0, 0], [4, 0, 2]], [[8, 0, 0]], [[10, 0, 0]]],
            go=[[2, 0, 0], [4, 0, 0], [6, 0, 0], [8, 0, 0], None]),
    1: dict(start=[20, 0, 0], goal=[22, 0, 2.5],
            cands=[[[22, 0, 0], [20, 0, 2]], [[22, 0, 2], [24, 0, 0]], [[22, 0, 4]]],
            go=[[22, 0, 0], [22, 0, 2], None]),
    2: dict(start=[40, 0, 0], goal=[45, 0, 0],
            cands=[[[42, 0, 0]], [[40.1, 0, 0]]],
            go=[[42, 0, 0], None]),
    3: dict(start=[60, 0, 0], goal=[60, 0, 10], ref=[[60, 0, 0], [58, 0, 0], [58, 0, 5], [60, 0, 10]],      # the reference path takes a detour
            cands=[[[62, 0, 0], [60, 0, 2], [58, 0, 0]], [[60, 0, 4], [62, 0, 2]], [[60, 0, 6]]],
            go=[[60, 0, 2], [60, 0, 4], None]),
}
PLAN_CFG = dict(max_len=5, loc_noise=0.5, merge_ghost=True, ghost_aug=0, ml_weight=0.37, logits_seed=11, choice_seed=5)
PLAN_ACTIVE = [4, 4, 3, 1, 1]


def plan_envs():
    n = len(PLAN)
    ref = {f"r0e{s}": PLAN[s].get("ref", np.linspace(PLAN[s]["start"], PLAN[s]["goal"], 6).tolist()) for s in range(n)}
    return ScriptedEnvs([PLAN[s]["start"] for s in range(n)], [PLAN[s]["goal"] for s in range(n)], ref_paths=ref), ref


def real_pos_of(pos, k):
    """where the simulator says candidate k really is: beside the estimate, differently for every candidate"""
    return np.asarray(pos, dtype=np.float64) + np.array([0.05 * (k + 1), 0.0, -0.03 * (k + 1)])


def scripted_rollout(make_gmap, teacher_fn):
    """PLAN on maps from make_gmap() (the reference's GraphMap or GraphMapLite, has_real_pos on) and ScriptedEnvs.
    teacher_fn(policy, gmaps, vp_ids, no_vp_left, envs, ref_paths) -> labels.  -> the log: per step slots, vp_ids, no_vp_left, logits
    (fp32, -inf on the visited nodes and the padding), the labels of both policies and the distances the environments returned."""
    envs, ref = plan_envs()
    envs.resume_all()
    envs.reset()
    gmaps = [make_gmap() for _ in range(envs.num_envs)]
    prev_vp = [None] * envs.num_envs
    g = np.random.default_rng(PLAN_CFG["logits_seed"])
    log = []
    for stepk in range(PLAN_CFG["max_len"]):
        slots = list(envs.active)
        pos = [p for p, _ in envs.call(["get_pos_ori"] * envs.num_envs)]
        cur_vp = []
        for i, s in enumerate(slots):
            c = [np.asarray(p, dtype=np.float64) for p in PLAN[s]["cands"][stepk]]
            vp = str(len(gmaps[i].node_pos))
            gmaps[i].update_graph(prev_vp[i], stepk + 1, vp, pos[i].copy(), 0.0, [f"{vp}_{k}" for k in range(len(c))], c, [0.0] * len(c),
                                  [real_pos_of(p, k) for k, p in enumerate(c)])
            cur_vp.append(vp)
        vp_ids = [[None] + list(m.node_pos.keys()) + list(m.ghost_pos.keys()) for m in gmaps]
        no_vp_left = [len(m.ghost_pos) == 0 for m in gmaps]
        B, G = len(slots), max(len(v) for v in vp_ids)
        logits = np.full((B, G), -np.inf, dtype=np.float32)
        for i, m in enumerate(gmaps):
            n = len(m.node_pos)
            logits[i, 0] = np.float32(2.0 * g.standard_normal())
            logits[i, 1 + n:len(vp_ids[i])] = (2.0 * g.standard_normal(len(m.ghost_pos))).astype(np.float32)
        q0 = len(envs.queries)
        labels = {p: [int(x) for x in teacher_fn(p, gmaps, vp_ids, no_vp_left, envs, ref)] for p in ("spl", "ndtw")}
        dists = [[s, name, d] for s, name, d in envs.queries[q0:]]
        log.append(dict(stepk=stepk, slots=slots, vp_ids=[[v for v in ids[1:]] for ids in vp_ids], no_vp_left=no_vp_left,
                        logits=logits, spl=labels["spl"], ndtw=labels["ndtw"], dists=dists))
        actions = []
        for i, s in enumerate(slots):
            go = PLAN[s]["go"][stepk]
            if go is None:
                actions.append({"action": {"act": 0, "stop_pos": gmaps[i].node_pos[cur_vp[i]]}})
                continue
            gvp = min(gmaps[i].ghost_mean_pos, key=lambda k: float(np.linalg.norm(gmaps[i].ghost_mean_pos[k] - np.asarray(go, dtype=np.float64))))
            actions.append({"action": {"act": 4, "ghost_pos": gmaps[i].ghost_aug_pos[gvp]}})
            prev_vp[i] = cur_vp[i]
            gmaps[i].delete_ghost(gvp)
        dones = [o[2] for o in envs.step(actions)]
        for i in reversed(range(len(slots))):
            if dones[i]:
                envs.pause_at(i); gmaps.pop(i); prev_vp.pop(i)
        if envs.num_envs == 0:
            break
    return log


def package_teacher(seed=None):
    """teacher_fn of scripted_rollout from etpnav_amd.rollout.teacher_actions, one random stream per policy"""
    from etpnav_amd.rollout import teacher_actions
    seed = PLAN_CFG["choice_seed"] if seed is None else seed
    rngs = {"spl": random.Random(seed), "ndtw": random.Random(seed + 1)}

    def fn(policy, gmaps, vp_ids, no_vp_left, envs, ref):
        return teacher_actions(gmaps, vp_ids, no_vp_left, envs, policy, rngs[policy], lambda ep: ref[str(ep.episode_id)])
    return fn


# ---- the loop written out from the public pieces, with torch's loss ----------------------------------------------
def hand_composed_rollout(net, predictor, envs, cfg, obs_to_batch, device, ml_weight, sample_ratio, uniforms, rng, mode="train"):
    """What a user composes today from the package's routes, statement by statement as INTEGRATION.md tells it, the loss being
    F.cross_entropy(reduction='sum', ignore_index=-100) with the host-side scale and .item().  -> (loss tensor or None, trace)"""
    import torch.nn.functional as F
    from etpnav_amd import graph_inputs as gi
    from etpnav_amd import rollout as ro
    from etpnav_amd.decide import RolloutDecider
    train = mode == "train"
    feedback = "sample" if train else "argmax"
    envs.resume_all()
    batch = obs_to_batch(envs.reset())
    ids = batch["instruction"]
    masks = ids != cfg.instr_pad_id
    embeds = net(mode="language", txt_ids=ids, txt_masks=masks)
    n = envs.num_envs
    not_done = list(range(n))
    maps = gi.DeviceGraphMaps(n, device, train, cfg.loc_noise, cfg.merge_ghost, cfg.ghost_aug if train else 0)
    store = gi.EmbedStore(cfg.max_len * n * 17, cfg.hidden, device)
    decider = RolloutDecider(n, device, cfg.back_algo, cfg.consume_ghost, cfg.tryout, cfg.max_len)
    loss, total_actions, trace = 0.0, 0.0, []
    for stepk in range(cfg.max_len):
        total_actions += envs.num_envs
        wp = net(mode="waypoint", waypoint_predictor=predictor, observations=batch, in_train=(train and cfg.waypoint_aug))
        vp = gi.vp_feature_variable(wp, device)
        pano_embeds, pano_masks = net(mode="panorama", **vp)
        cur_rows, cand_rows = store.append(pano_embeds, pano_masks, vp["nav_types"], [len(a) for a in wp["cand_angles"]])
        po = envs.call(["get_pos_ori"] * envs.num_envs)
        cur_pos, cur_heading = [x[0] for x in po], [float(x[1]) for x in po]
        cur_vp, _, cand_pos = maps.identify_node(cur_pos, cur_heading, wp["cand_angles"], wp["cand_distances"])
        real = [[envs.call_at(i, "get_cand_real_pos", {"angle": a, "forward": d}) for a, d in zip(wp["cand_angles"][i], wp["cand_distances"][i])]
                for i in range(envs.num_envs)] if train else [None] * envs.num_envs
        maps.update(decider.prev_vp, stepk + 1, cur_vp, cur_pos, cur_heading, cand_pos, cur_rows, cand_rows, real)
        nav = maps.nav_inputs()
        nav["gmap_img_fts"] = maps.img_fts(store, nav["gmap_masks"].shape[1])
        compact, no_vp_left = nav.pop("compact"), nav.pop("no_vp_left")
        logits = net(mode="navigation", txt_embeds=embeds[not_done], txt_masks=masks[not_done], **nav)["global_logits"]
        teacher = None
        if train:
            teacher = ro.teacher_actions(maps.gmaps, nav["gmap_vp_ids"], no_vp_left, envs, cfg.expert_policy, rng)
            loss = loss + F.cross_entropy(logits.float(), torch.tensor(teacher).to(device), reduction="sum", ignore_index=IGNORE)
        a_t, env_actions = decider.decide(logits, maps.gmaps, cur_vp, stepk, feedback, sample_ratio, teacher,
                                          uniforms=None if uniforms is None else uniforms[stepk], compact=compact)
        trace.append(dict(stepk=stepk, slots=list(not_done), cur_vp=list(cur_vp), teacher=teacher, nav_logits=logits.detach(),
                          a_t=[int(a) for a in a_t], env_actions=env_actions))
        outputs = envs.step(env_actions)
        observations, _, dones, _ = [list(x) for x in zip(*outputs)]
        for i in reversed(range(envs.num_envs)):
            if dones[i]:
                not_done.pop(i); envs.pause_at(i); observations.pop(i); maps.pause(i); decider.pause(i)
        if envs.num_envs == 0:
            break
        batch = obs_to_batch(observations)
    if not train:
        return None, trace
    loss = ml_weight * loss / total_actions
    return loss, trace
