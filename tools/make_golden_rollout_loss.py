"""Write tests/golden/rollout_loss_small.npz from the REAL reference code (build container only; needs the reference tree and networkx).

    python tools/make_golden_rollout_loss.py [--reference /root/reference]

Runs, on the CPU, the scripted 5-step rollout of 4 environments of tests/rollout_ref.PLAN on the real GraphMap
(vlnce_baselines/models/graph_utils.py, has_real_pos on) with rollout_ref.ScriptedEnvs standing in for the simulator, and executes the
reference trainer's OWN statements, cut out of vlnce_baselines/ss_trainer_ETP.py with `ast` at generation time and run unchanged (the
way tools/make_golden_decide.py runs the decision statements):
  * the whole method _teacher_action_new                                                            :278-306, for 'spl' and for 'ndtw'
  * total_actions += self.envs.num_envs                                                             :820
  * the `if mode == 'train'` node around loss += F.cross_entropy(..., reduction='sum', ignore_index=-100)      :891-892
  * the `if mode == 'train'` node behind the loop: loss = ml_weight * loss / total_actions, self.loss, self.logs['IL_loss']   :1054-1057
once on the fp32 logits and once on their float64 copies; autograd gives dlogits of both.

The rollout: active environments 4, 4, 3, 1, 1; slot 0 merges a candidate into an existing ghost at step 1 (two real positions:
random.choice matters) and is within 1.5 of its goal at the last step (label 0); slot 1 stands within 1.5 of its goal at step 2 (label 0);
slot 2 consumes its only ghost and its next candidate falls on a visited node: no ghost left, label -100; slot 3 is stopped by the script
while the teacher names a ghost.  Logits are N(0, 2) on [stop] and the ghosts, -inf on the visited nodes and the padding.

No program text of the reference goes into the file: the steps' logits and labels, the labels of both expert policies with the distances
the stub environments returned, the viewpoint names, and the recorded losses and gradients, plus the plan's configuration as JSON.
"""
import argparse
import ast
import json
import os
import random
import sys
import types
from collections import defaultdict

import numpy as np
import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
from etpnav_amd.graph_inputs import GraphMapLite  # noqa: E402
from make_golden_decide import load_graph_utils  # noqa: E402
from tests import rollout_ref as rr  # noqa: E402

OUT = rr.GOLDEN
NS = types.SimpleNamespace


def trainer_tree(ref):
    path = os.path.join(ref, "vlnce_baselines", "ss_trainer_ETP.py")
    return path, ast.parse(open(path).read())


def teacher_method(ref):
    """_teacher_action_new, compiled unchanged -> the function; `random` and `torch` are supplied by the caller's namespace"""
    path, tree = trainer_tree(ref)
    fn = next(n for n in ast.walk(tree) if isinstance(n, ast.FunctionDef) and n.name == "_teacher_action_new")
    assert (fn.lineno, fn.end_lineno) == (278, 306), (fn.lineno, fn.end_lineno)
    return compile(ast.fix_missing_locations(ast.Module(body=[fn], type_ignores=[])), path, "exec")


def loss_statements(ref):
    """-> (step code: :820 and the If of :891, tail code: the If of :1054), compiled unchanged"""
    path, tree = trainer_tree(ref)
    rollout = next(n for n in ast.walk(tree) if isinstance(n, ast.FunctionDef) and n.name == "rollout")
    loop = next(n for n in ast.walk(rollout) if isinstance(n, ast.For) and isinstance(n.target, ast.Name) and n.target.id == "stepk")
    step = [n for n in loop.body if n.lineno in (820, 891)]
    assert [type(n) for n in step] == [ast.AugAssign, ast.If] and step[1].end_lineno == 892 and step[0].target.id == "total_actions"
    tail = [n for n in rollout.body if n.lineno == 1054]
    assert len(tail) == 1 and isinstance(tail[0], ast.If) and tail[0].end_lineno == 1057
    mk = lambda body: compile(ast.fix_missing_locations(ast.Module(body=body, type_ignores=[])), path, "exec")
    return mk(step), mk(tail)


def reference_teacher(code, seed):
    """teacher_fn of rollout_ref.scripted_rollout from the reference's method; one random stream per policy, seeded as package_teacher's"""
    rngs = {"spl": random.Random(seed), "ndtw": random.Random(seed + 1)}
    shim = NS(tensor=lambda x: NS(cuda=lambda: torch.tensor(x)))          # torch.tensor(teacher_actions).cuda() without a GPU

    def fn(policy, gmaps, vp_ids, no_vp_left, envs, ref):
        ns = {"random": rngs[policy], "np": np, "torch": shim}
        exec(code, ns)
        me = NS(envs=envs, gmaps=gmaps, config=NS(IL=NS(expert_policy=policy)), gt_data={k: {"locations": v} for k, v in ref.items()})
        return ns["_teacher_action_new"](me, vp_ids, no_vp_left).tolist()
    return fn


def run_loss(step_code, tail_code, log, dtype, ml_weight):
    """the reference's statements over the recorded steps -> (loss, [dlogits], IL_loss log)"""
    me = NS(envs=NS(num_envs=0), loss=0.0, logs=defaultdict(list))
    ns = {"F": F, "torch": torch, "self": me, "mode": "train", "loss": 0.0, "total_actions": 0.0, "ml_weight": ml_weight}
    leaves = []
    for e in log:
        x = torch.from_numpy(e["logits"]).to(dtype).requires_grad_(True)
        leaves.append(x)
        me.envs.num_envs = len(e["slots"])
        ns.update(nav_logits=x, teacher_actions=torch.tensor(e["spl"], dtype=torch.int64))
        exec(step_code, ns)
    exec(tail_code, ns)
    me.loss.backward()
    assert ns["total_actions"] == sum(rr.PLAN_ACTIVE) and len(me.logs["IL_loss"]) == 1
    return ns["loss"].detach(), [x.grad for x in leaves], me.logs["IL_loss"]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reference", default="/root/reference")
    a = ap.parse_args()
    gu = load_graph_utils(a.reference)
    cfg = rr.PLAN_CFG
    log = rr.scripted_rollout(lambda: gu.GraphMap(True, cfg["loc_noise"], cfg["merge_ghost"], cfg["ghost_aug"]),
                              reference_teacher(teacher_method(a.reference), cfg["choice_seed"]))
    # ---- what the rollout must contain ----
    assert [len(e["slots"]) for e in log] == rr.PLAN_ACTIVE, [e["slots"] for e in log]
    labels = [x for e in log for x in e["spl"]]
    assert rr.IGNORE in labels and 0 in labels and any(x > 0 for x in labels), labels
    assert log[1]["spl"][2] == rr.IGNORE and log[1]["no_vp_left"][2] and log[2]["spl"][1] == 0 and log[4]["spl"][0] == 0
    assert all(np.isneginf(e["logits"][:, 1]).all() for e in log), "the first visited node carries -inf"
    assert any(e["spl"] != e["ndtw"] for e in log), "the two expert policies never disagree"
    # ---- the package's restatement replays it on GraphMapLite ----
    lite = rr.scripted_rollout(lambda: GraphMapLite(True, cfg["loc_noise"], cfg["merge_ghost"], cfg["ghost_aug"]), rr.package_teacher())
    for e, f in zip(log, lite):
        assert (e["spl"], e["ndtw"], e["vp_ids"], e["slots"]) == (f["spl"], f["ndtw"], f["vp_ids"], f["slots"]), (e["stepk"], e, f)
        assert json.dumps(e["dists"]) == json.dumps(f["dists"]), e["stepk"]
    step_code, tail_code = loss_statements(a.reference)
    out = {}
    for name, dtype in (("f32", torch.float32), ("f64", torch.float64)):
        loss, grads, il = run_loss(step_code, tail_code, log, dtype, cfg["ml_weight"])
        assert loss.dtype == dtype and float(loss) == il[0]
        out[f"loss_{name}"] = loss.numpy()
        for t, gr in enumerate(grads):
            out[f"dlogits_{name}_{t}"] = gr.numpy()
    for t, e in enumerate(log):
        out[f"logits_{t}"] = e["logits"]
        out[f"labels_{t}"] = np.asarray(e["spl"], dtype=np.int64)
        out[f"labels_ndtw_{t}"] = np.asarray(e["ndtw"], dtype=np.int64)
    meta = dict(T=len(log), cfg=cfg, active=rr.PLAN_ACTIVE, slots=[e["slots"] for e in log], vp_ids=[e["vp_ids"] for e in log],
                no_vp_left=[e["no_vp_left"] for e in log], dists=[e["dists"] for e in log])
    out["meta"] = np.array(json.dumps(meta))
    np.savez_compressed(OUT, **out)
    print(f"{OUT}: {os.path.getsize(OUT)} bytes; labels {[e['spl'] for e in log]} / ndtw {[e['ndtw'] for e in log]}; "
          f"loss fp32 {float(out['loss_f32']):.9g} float64 {float(out['loss_f64']):.17g}")


if __name__ == "__main__":
    main()
