"""Write tests/golden/decide_small.npz from the REAL reference code (build container only; needs the reference tree and networkx).

    python tools/make_golden_decide.py [--reference /root/reference]

Runs, on the CPU, a scripted 6-step rollout of 4 episodes on the real GraphMap (vlnce_baselines/models/graph_utils.py) and, at every
step, the reference trainer's OWN decision statements, cut out of RLTrainer.rollout (vlnce_baselines/ss_trainer_ETP.py) with `ast`
at generation time and executed unchanged (the way oracle/ref_trainer_fns.py runs the trainer's method bodies):
  * nav_probs = F.softmax(nav_logits, 1) and the loop that fills gmap.node_stop_scores               :880-882
  * the `if feedback == 'sample'` node                                                               :895-902
  * cpu_a_t, env_actions = [], use_tryout and the `for i, gmap in enumerate(self.gmaps)` node        :903-977
While they run, torch.distributions.Categorical is a recording stand-in that draws by inverse CDF from the stored u0 and
torch.rand_like returns the stored u1 (the pattern of tools/make_golden_waypoint.py).

The rollout (tests/decide_ref.CFG: consume_ghost on, back_algo 'control', max_len 6; feedback 'sample' at steps 0-3, 'argmax' at 4-5):
  slot 0   random walk to the end: sampled actions at steps 0 and 2, u1 == sample_ratio exactly at step 1 (the teacher's ghost, not the
           sampled one), two ghosts with exactly equal maximal logits at step 4, the forced stop of step 5 under a ghost's arg-max
  slot 1   random; samples action 0 at step 2 with a high stop probability and is paused mid-way
  slot 2   its only ghost is consumed at step 0, the candidate of step 1 falls on the first node: no ghost left, teacher = ignore_index
  slot 3   integer coordinates: one-hot logits at steps 0 and 2 (two stop scores of exactly 1), a ghost with two exactly equidistant
           fronts chosen at step 1, a front that is the current node at step 4, a four-hop path back at the forced stop
No program text of the reference goes into the file: the plan's inputs (poses, candidate positions, logits, teacher labels, uniforms)
and the recorded decisions, as one JSON string, plus the configuration.  The conditions the GPU replay rests on
(tests/decide_ref.check_conditions) are asserted at every step, and every mutation of decide_ref.MUTATIONS must change the log.
"""
import argparse
import ast
import importlib.util
import json
import os
import sys
import types

import numpy as np
import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from etpnav_amd.graph_inputs import GraphMapLite, pack_episode  # noqa: E402
from tests import decide_ref as dr  # noqa: E402

OUT = os.path.join(ROOT, "tests", "golden", "decide_small.npz")
LINES = {880: ast.Assign, 881: ast.For, 895: ast.If, 903: ast.Assign, 906: ast.Assign, 907: ast.Assign, 908: ast.For}


def load_graph_utils(ref):
    for name in ("habitat", "habitat.tasks", "habitat.tasks.utils", "habitat.utils", "habitat.utils.geometry_utils"):
        sys.modules.setdefault(name, types.ModuleType(name))
    sys.modules["habitat.tasks.utils"].cartesian_to_polar = lambda x, y: (np.hypot(x, y), np.arctan2(y, x))
    sys.modules["habitat.utils.geometry_utils"].quaternion_rotate_vector = None
    sys.modules["habitat.utils.geometry_utils"].quaternion_from_coeff = None
    try:
        import matplotlib.pyplot  # noqa: F401
    except Exception:
        sys.modules.setdefault("matplotlib", types.ModuleType("matplotlib"))
        sys.modules.setdefault("matplotlib.pyplot", types.ModuleType("matplotlib.pyplot"))
    spec = importlib.util.spec_from_file_location("ref_graph_utils_decide", os.path.join(ref, "vlnce_baselines", "models", "graph_utils.py"))
    gu = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(gu)
    return gu


def decision_statements(ref):
    """the statements of RLTrainer.rollout's step loop named in the module docstring, compiled unchanged"""
    path = os.path.join(ref, "vlnce_baselines", "ss_trainer_ETP.py")
    tree = ast.parse(open(path).read())
    rollout = next(n for n in ast.walk(tree) if isinstance(n, ast.FunctionDef) and n.name == "rollout")
    loop = next(n for n in ast.walk(rollout) if isinstance(n, ast.For) and isinstance(n.target, ast.Name) and n.target.id == "stepk")
    picked = [n for n in loop.body if n.lineno in LINES]
    assert [type(n) for n in picked] == [LINES[n.lineno] for n in picked] and len(picked) == len(LINES), [n.lineno for n in picked]
    assert picked[0].targets[0].id == "nav_probs" and picked[3].targets[0].id == "cpu_a_t" and picked[-1].end_lineno == 977
    return compile(ast.fix_missing_locations(ast.Module(body=picked, type_ignores=[])), path, "exec")


class RecordingCategorical:
    """stand-in for torch.distributions.Categorical: sample() is the inverse CDF at the stored u0 of every row"""
    u0 = None

    def __init__(self, probs):
        self.probs = probs

    def sample(self):
        p = self.probs.double().numpy()
        act = []
        for b in range(p.shape[0]):
            cdf = np.cumsum(p[b])
            last = int(np.nonzero(p[b] > 0)[0][-1])
            act.append(min(int(np.searchsorted(cdf, float(RecordingCategorical.u0[b]) * cdf[-1], side="right")), last))
        return torch.tensor(act, dtype=torch.long)


class ReferenceStep:
    """decide_step of decide_ref.drive: the reference's own statements on real GraphMap objects"""

    def __init__(self, code, cfg=dr.CFG, check=False):
        self.code, self.cfg, self.check = code, cfg, check

    def __call__(self, gmaps, cur_vp, prev_vp, active, logits, teacher, uni, feedback, stepk):
        cfg = self.cfg
        if self.check:
            for i, g in enumerate(gmaps):
                ep = pack_episode(g, cur_vp[i], np.zeros(3), 0.0)
                row = np.full(64, -dr.INF)
                row[:len(g.node_stop_scores)] = list(g.node_stop_scores.values())
                sample = feedback == "sample"
                dr.check_conditions(ep, logits[i], row, uni[i] if sample else None, int(teacher[i]) if sample else None,
                                    cfg["sample_ratio"], stepk == cfg["max_len"] - 1, name=f"step {stepk} slot {active[i]}")
        NS = types.SimpleNamespace
        me = NS(gmaps=gmaps, max_len=cfg["max_len"],
                config=NS(IL=NS(tryout=cfg["tryout"], back_algo=cfg["back_algo"]), VIDEO_OPTION=[], MODEL=NS(consume_ghost=cfg["consume_ghost"]),
                          TASK_CONFIG=NS(SIMULATOR=NS(HABITAT_SIM_V0=NS(ALLOW_SLIDING=False)))))
        ns = {"torch": torch, "F": F, "np": np, "self": me, "nav_logits": torch.from_numpy(np.ascontiguousarray(logits)),
              "cur_vp": cur_vp, "feedback": feedback, "sample_ratio": cfg["sample_ratio"], "teacher_actions": torch.from_numpy(teacher.copy()),
              "stepk": stepk, "no_vp_left": [len(g.ghost_pos) == 0 for g in gmaps], "prev_vp": prev_vp, "mode": "eval",
              "nav_inputs": {"gmap_vp_ids": [[None] + list(g.node_pos.keys()) + list(g.ghost_pos.keys()) for g in gmaps]}}
        RecordingCategorical.u0 = uni[:, 0]
        real_cat, real_rand = torch.distributions.Categorical, torch.rand_like
        torch.distributions.Categorical = RecordingCategorical
        torch.rand_like = lambda t, **k: torch.from_numpy(uni[:, 1].copy())
        try:
            exec(self.code, ns)
        finally:
            torch.distributions.Categorical, torch.rand_like = real_cat, real_rand
        return ns["cpu_a_t"], ns["env_actions"]


def cell_midpoint(l, k):
    p = dr.softmax64(l)
    assert p[k] >= 1e-3, (k, p[k])
    cdf = np.concatenate(([0.0], np.cumsum(p)))
    return np.float32(0.5 * (cdf[k] + cdf[k + 1]) / cdf[-1])


class GoldenPlan(dr.RandomPlan):
    """the rollout of the module docstring"""
    A = np.array([30.0, 0.0, 0.0])
    CANDS3 = [[[1, 0, 1], [2, 0, 0]], [[1, 0, 1], [4, 0, 0]], [[1, 0, 3]], [[3, 0, 3], [2.1, 0, 0.1]], [[5, 0, 3]], [[7, 0, 3]]]
    GO3 = [[2, 0, 0], [1, 0, 1], [1, 0, 3], [3, 0, 3], [5, 0, 3], [4, 0, 0]]     # the ghost slot 3 heads for (step 5: the arg-max under the forced stop)

    def __init__(self):
        super().__init__(seed=20, argmax_from=4)

    def start(self, s):
        return self.A if s == 3 else [20.0, 0.0, 0.0] if s == 2 else super().start(s)

    def cands(self, s, stepk, cur_pos):
        if s == 3:
            return [self.A + c for c in self.CANDS3[stepk]]
        if s == 2:
            return [[22.0, 0.0, 0.0]] if stepk == 0 else [[20.1, 0.0, 0.0]]
        c = super().cands(s, stepk, cur_pos)
        return c if len(c) >= 2 else c + [cur_pos + [0.0, 0.0, 2.5]]

    def policy(self, s, stepk, gmap, cur_vp):
        rng = self.rng
        n, m = len(gmap.node_pos), len(gmap.ghost_pos)
        ghosts = list(gmap.ghost_pos.keys())
        l = np.full(1 + n + m, -dr.INF, dtype=np.float32)
        l[0] = np.float32(rng.standard_normal() - 1.0)
        l[1 + n:] = (1.5 * rng.standard_normal(m)).astype(np.float32)
        if s == 2:
            if m == 0:
                return l, dr.IGNORE, np.array([0.5, 0.0], dtype=np.float32)          # teacher = ignore_index, taken, no ghost left
            return l, 0, np.array([cell_midpoint(l, 1 + n), 0.9], dtype=np.float32)    # sampled: the only ghost
        if s == 3:
            want = next(g for g in ghosts if np.allclose(gmap.ghost_aug_pos[g], self.A + self.GO3[stepk]))
            k = 1 + n + ghosts.index(want)
            if stepk in (0, 2):
                l[1:] = -dr.INF                                                        # one-hot: stop_prob is exactly 1
                l[0] = 0.0
            if stepk >= 4:
                l[k] = np.float32(l.max() + 1.0)                                       # the arg-max
            return l, k, np.array([0.5, 0.0], dtype=np.float32)                        # sample steps: the teacher's label
        if s == 1:
            if stepk == 2:
                l[0] = np.float32(l[1 + n:].max() + 3.0)
                return l, 1 + n, np.array([cell_midpoint(l, 0), 0.9], dtype=np.float32)  # samples the stop
            k = 1 + n + int(np.argmax(l[1 + n:]))
            return l, 0, np.array([cell_midpoint(l, k), 0.9], dtype=np.float32)        # samples a ghost
        # slot 0
        order = np.argsort(-l[1 + n:])
        k0, k1 = 1 + n + int(order[0]), 1 + n + int(order[1])
        if stepk in (0, 2):
            return l, 0, np.array([cell_midpoint(l, k0), 0.9], dtype=np.float32)       # sampled ghost (the teacher says stop)
        if stepk == 1:
            return l, k1, np.array([cell_midpoint(l, k0), 0.25], dtype=np.float32)     # u1 == sample_ratio: the teacher's ghost
        if stepk == 3:
            return l, k0, np.array([cell_midpoint(l, 0), 0.0], dtype=np.float32)       # the teacher's ghost; the sample would stop
        if stepk == 4:
            l[max(k0, k1)] = l[min(k0, k1)] = np.float32(l.max() + 0.5)                # exactly equal maxima
        else:
            l[k1] = np.float32(l.max() + 0.5)                                          # a ghost leads at the forced stop
        return l, 0, np.array([0.5, 0.5], dtype=np.float32)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reference", default="/root/reference")
    a = ap.parse_args()
    gu = load_graph_utils(a.reference)
    code = decision_statements(a.reference)
    cfg = dr.CFG
    log = dr.drive(lambda: gu.GraphMap(False, cfg["loc_noise"], cfg["merge_ghost"], 0), GoldenPlan(), ReferenceStep(code, check=True), 4)
    log = json.loads(json.dumps(log))
    # ---- what the rollout must contain ----
    assert len(log) == 6 and [e["slots"] for e in log] == [[0, 1, 2, 3], [0, 1, 2, 3], [0, 1, 3], [0, 3], [0, 3], [0, 3]], [e["slots"] for e in log]
    assert [e["feedback"] for e in log] == ["sample"] * 4 + ["argmax"] * 2
    assert log[1]["a_t"][2] == dr.IGNORE and log[1]["actions"][2]["act"] == 0 and log[1]["ghosts_after"][2] == []
    assert log[2]["a_t"][1] == 0 and log[5]["a_t"][0] != 0 and log[5]["actions"][0]["act"] == 0
    assert log[1]["actions"][3]["front_vp"] == "0" and log[4]["actions"][1]["back_path"] == [] and log[4]["actions"][1]["front_vp"] == "4"
    assert [x[0] for x in log[5]["actions"][1]["back_path"]] == ["4", "3", "2", "0"] and log[5]["actions"][1]["stop_vp"] == "0"
    assert [sc for _, sc in log[5]["stop_scores"][1]][0] == 1.0 == [sc for _, sc in log[5]["stop_scores"][1]][2]
    # ---- the restatement replays it, every mutation changes it ----
    lite = lambda: GraphMapLite(False, cfg["loc_noise"], cfg["merge_ghost"], 0)
    dr.compare_logs(dr.drive(lite, dr.ReplayPlan(log), dr.RefStep(4), 4), log, "restatement")
    for mut in dr.MUTATIONS:
        try:
            dr.compare_logs(dr.drive(lite, dr.ReplayPlan(log), dr.RefStep(4, mut=mut), 4), log, mut)
        except (AssertionError, KeyError, IndexError, StopIteration):
            continue
        raise AssertionError(f"mutation {mut} passes the recording")
    np.savez_compressed(OUT, log=np.array(json.dumps(log)), cfg=np.array(json.dumps(cfg)))
    print(f"{OUT}: {os.path.getsize(OUT)} bytes; cpu_a_t per step {[e['a_t'] for e in log]}")


if __name__ == "__main__":
    main()
