"""Generate the fixtures of tests/test_oracle_vs_reference.py and of the schedule test in tests/test_features_sched_cpu.py
from the REAL reference (needs it at ETPNAV_REFERENCE; build container only):

    python oracle/make_golden_refcheck.py

  tests/golden/refcheck_step.npz      the reference planner's loss, global logits and parameter gradients on the small ragged
                                      r2r case (weights seed 3, batch seed 7): every gradient as (sum, abs-max, L2) plus
                                      N_SAMPLE values at fixed strided indices (the whole set is 563 MB)
  tests/golden/refcheck_graph.npz     packed episodes and _nav_gmap_variable outputs of random rollouts through the REAL
                                      GraphMap (GRAPH_SEEDS)
  tests/golden/refcheck.json          key set / shapes / tied tensors of the REAL pre-training model's state dict, the REAL
                                      GraphMap's state after the has_real_pos + ghost_aug drives (GHOST_AUG_SEEDS), and the
                                      reference's warm-up-linear schedule values (SCHED_STEPS)

The drives (graph_state_after_ghost_aug_drive) are shared with the tests, which run them on GraphMapLite.
TEST INFRASTRUCTURE ONLY.
"""
from __future__ import annotations

import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from oracle import planner_oracle as po  # noqa: E402

GOLDEN = os.path.join(ROOT, "tests", "golden")
N_SAMPLE = 512
GRAPH_SEEDS = list(range(30, 42))
GHOST_AUG_SEEDS = [3, 4, 5, 6]
SCHED_STEPS = list(range(0, 1300, 37))


def step_case():
    cfg = po.PlannerConfig.r2r()
    P = po.init_params(cfg, seed=3)
    batch = po.make_batch(cfg, B=2, L=10, V=13, G=6, seed=7, ragged=True)
    return cfg, P, batch


def sample_idx(n: int) -> np.ndarray:
    if n <= N_SAMPLE:
        return np.arange(n)
    return np.unique(np.linspace(0, n - 1, N_SAMPLE).astype(np.int64))


def graph_case(seed):
    """(steps, merge_ghost) of one random rollout"""
    return 2 + seed % 9, bool(seed % 2)


def graph_state_after_ghost_aug_drive(cls, seed):
    """Drive a GraphMap-like class with has_real_pos and ghost_aug on (graph_utils.py:213-214,225-226,236-237,245-252) and
    return every dict of the graph as plain JSON-compatible values (dict order kept)."""
    rng = np.random.RandomState(seed)
    np.random.seed(1000 + seed)                          # the jitter draws from the global generator in both classes
    g = cls(True, 0.5, bool(seed % 2), 0.3)              # has_real_pos, loc_noise, merge_ghost, ghost_aug
    pos, heading, prev = np.array([0.3, 0.2, -0.4]), 1.0, None
    for k in range(6):
        n = rng.randint(2, 6)
        cur_vp, cand_vp, cand_pos = g.identify_node(pos, heading, list(rng.uniform(0, 6.28, n)), list(rng.uniform(0.3, 2.0, n)))
        real = [p + rng.normal(0, 0.05, 3) for p in cand_pos]
        g.update_graph(prev, k + 1, cur_vp, pos, float(k), cand_vp, cand_pos, [float(10 * k + i) for i in range(n)], real)
        prev = cur_vp
        if k == 5:
            break        # compare right after an update (the reference leaves a deleted ghost in ghost_aug_pos until the next one)
        ghosts = list(g.ghost_pos.keys())
        gv = ghosts[rng.randint(len(ghosts))]
        pos, heading = np.array(g.ghost_real_pos[gv][0], dtype=np.float64), rng.uniform(0, 6.28)
        g.delete_ghost(gv)
    if hasattr(g, "graph_nx"):
        edges = {tuple(sorted((u, v))): w for u, v, w in g.graph_nx.edges(data="weight")}
    else:
        edges = dict(g.edges)
    arr = lambda d: [[k, np.asarray(v, dtype=np.float64).tolist()] for k, v in d.items()]
    return {
        "edges": [[u, v, float(w)] for (u, v), w in edges.items()],
        "node_pos": list(g.node_pos), "node_stepId": [[k, int(v)] for k, v in g.node_stepId.items()],
        "ghost_cnt": int(g.ghost_cnt),
        "ghost_mean_pos": arr(g.ghost_mean_pos), "ghost_aug_pos": arr(g.ghost_aug_pos),
        "ghost_pos": arr(g.ghost_pos), "ghost_real_pos": arr(g.ghost_real_pos),
        "ghost_fronts": [[k, list(v)] for k, v in g.ghost_fronts.items()],
        "ghost_embeds": [[k, float(v[0]), int(v[1])] for k, v in g.ghost_embeds.items()],
    }


def make_step():
    from oracle import ref_harness as rh
    cfg, P, batch = step_case()
    ro, rg = rh.reference_step(rh.build_reference_model(cfg, P), batch)
    d = {"out.loss": ro["loss"].detach().float().numpy(), "out.global_logits": ro["global_logits"].detach().float().numpy()}
    for k, g in rg.items():
        f = g.detach().double().reshape(-1)
        d[f"gfp.{k}"] = np.array([float(f.sum()), float(f.abs().max()), float(f.norm())])
        d[f"gsm.{k}"] = f[torch.from_numpy(sample_idx(f.numel()))].float().numpy()
    np.savez_compressed(os.path.join(GOLDEN, "refcheck_step.npz"), **d)


def make_graph(gu):
    from oracle import graph_oracle as go
    from oracle.make_golden_graph import reference_batch_outputs
    from etpnav_amd.graph_inputs import pack_episode
    z = {}
    for seed in GRAPH_SEEDS:
        steps, merge = graph_case(seed)
        real = go.simulate(gu.GraphMap, seed, steps, merge_ghost=merge)
        a = pack_episode(real[0], real[1], real[2], real[3])
        for k in ("n_nodes", "n_ghost", "cur_node", "node_pos", "node_step", "adj", "ghost_pos"):
            z[f"s{seed}/{k}"] = np.asarray(a[k])
        z[f"s{seed}/ghost_front_ptr"] = np.cumsum([0] + [len(f) for f in a["ghost_fronts"]]).astype(np.int64)
        z[f"s{seed}/ghost_front_idx"] = np.array([x for f in a["ghost_fronts"] for x in f], dtype=np.int64)
        ref = reference_batch_outputs(gu, [real[0]], [real[1]], [real[2]], [real[3]])
        for k in ("gmap_step_ids", "gmap_visited_masks", "gmap_pos_fts", "gmap_pair_dists"):
            z[f"s{seed}/{k}"] = ref[k][0].numpy()
    np.savez_compressed(os.path.join(GOLDEN, "refcheck_graph.npz"), **z)


def make_json(gu):
    import importlib.util
    from oracle import ref_harness as rh
    from oracle import ref_pretrain_harness as rp
    cfg = po.PlannerConfig.r2r(vocab_size=512, num_l_layers=1, num_pano_layers=1, num_x_layers=1, use_lang2visn_attn=True)
    sd = rp.build_pretrain_model(cfg, po.init_params(cfg, seed=5)).state_dict()
    owner = {}
    for k, v in sd.items():
        owner.setdefault(v.data_ptr(), []).append(k)
    spec = importlib.util.spec_from_file_location("ref_sched", os.path.join(rh.REF, "pretrain_src/pretrain_src/optim/sched.py"))
    ref = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(ref)

    class O:
        learning_rate = 5e-5; warmup_steps = 100; num_train_steps = 1000
    doc = {
        "pretrain_state_dict": {"keys": [[k, list(v.shape)] for k, v in sd.items()],
                                "tied": [ks for ks in owner.values() if len(ks) > 1]},
        "ghost_aug_drive": {str(s): graph_state_after_ghost_aug_drive(gu.GraphMap, s) for s in GHOST_AUG_SEEDS},
        "sched": {"steps": SCHED_STEPS, "get_lr_sched": [ref.get_lr_sched(s, O) for s in SCHED_STEPS],
                  "warmup_linear": [ref.warmup_linear(s, 100, 1000) for s in SCHED_STEPS]},
    }
    with open(os.path.join(GOLDEN, "refcheck.json"), "w") as f:
        json.dump(doc, f, indent=0)


def main():
    from oracle import ref_harness as rh
    from oracle.make_golden_graph import load_reference_graph_utils
    assert rh.reference_available(), f"needs the reference at {rh.REF}"
    gu = load_reference_graph_utils()
    make_step()
    make_graph(gu)
    make_json(gu)
    for n in ("refcheck_step.npz", "refcheck_graph.npz", "refcheck.json"):
        print(n, os.path.getsize(os.path.join(GOLDEN, n)) // 1024, "KiB")


if __name__ == "__main__":
    main()
