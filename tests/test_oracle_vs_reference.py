"""Oracle against outputs of the REAL reference stored under tests/golden/refcheck* (generator oracle/make_golden_refcheck.py,
run where the reference exists)."""
import json
import os

import numpy as np
import pytest
import torch

from oracle import planner_oracle as po
from oracle import make_golden_refcheck as mr

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def _refcheck():
    with open(os.path.join(GOLDEN, "refcheck.json")) as f:
        return json.load(f)


def test_oracle_equals_reference_small():
    """Every gradient as strided samples (abs 2e-5, as every element was held to) plus its abs-max and L2, which an elementwise
    2e-5 bound implies to within 2e-5 and 2e-5 * sqrt(numel)."""
    z = np.load(os.path.join(GOLDEN, "refcheck_step.npz"))
    cfg, P, batch = mr.step_case()
    oo, og = po.step_with_grads(P, cfg, batch)
    assert abs(float(z["out.loss"]) - float(oo["loss"])) < 1e-5
    ref = torch.from_numpy(z["out.global_logits"])
    fin = torch.isfinite(ref)
    assert torch.equal(torch.isfinite(oo["global_logits"]), fin)
    assert float((ref[fin] - oo["global_logits"][fin]).abs().max()) < 2e-5
    names = [k[4:] for k in z.files if k.startswith("gfp.")]
    assert sorted(names) == sorted(og), "gradient set differs from the reference's"
    for k in names:
        g = og[k].detach().double().reshape(-1)
        smp = torch.from_numpy(z[f"gsm.{k}"]).double()
        assert float((g[torch.from_numpy(mr.sample_idx(g.numel()))] - smp).abs().max()) < 2e-5, k
        fp = z[f"gfp.{k}"]
        assert abs(float(g.abs().max()) - fp[1]) < 2e-5, k
        assert abs(float(g.norm()) - fp[2]) < 2e-5 * g.numel() ** 0.5, k


def test_saved_pretraining_checkpoint_loads_strictly_into_the_real_model():
    """etpnav_amd.checkpoint.pretrain_state_dict writes exactly the key set of the reference pre-training model
    (utils/save.py:23-46): what a strict load into the REAL GlocalTextPathCMTPreTraining checks -- the same keys, the same
    shapes (the real model's state dict is stored in tests/golden/refcheck.json) -- and the loaded model then reproduces the
    planner's own parameters: every value as given, and the tensors the real model ties (decoder = word embeddings) equal."""
    from etpnav_amd import checkpoint as ck
    from etpnav_amd.planner import GlocalTextPathNavCMT
    ref = _refcheck()["pretrain_state_dict"]
    cfg = po.PlannerConfig.r2r(vocab_size=512, num_l_layers=1, num_pano_layers=1, num_x_layers=1, use_lang2visn_attn=True)
    P = po.init_params(cfg, seed=2)
    m = GlocalTextPathNavCMT(cfg.to_dict(), dtype=torch.float32, device="cpu")
    m.load_state_dict(P, strict=True)
    got = ck.pretrain_state_dict(m)
    want = {k: tuple(shape) for k, shape in ref["keys"]}
    assert not set(want) - set(got) and not set(got) - set(want)          # missing, unexpected
    assert {k: tuple(v.shape) for k, v in got.items()} == want
    for k, v in P.items():
        name = k if k.startswith(("mlm_head.", "global_sap_head.")) else "bert." + k
        assert torch.equal(got[name], v), k
    assert ["bert.embeddings.word_embeddings.weight", "mlm_head.predictions.decoder.weight"] in [sorted(t) for t in ref["tied"]]
    for tied in ref["tied"]:
        assert all(torch.equal(got[tied[0]], got[k]) for k in tied[1:]), tied


@pytest.mark.parametrize("seed", list(range(30, 42)))
def test_graph_assembly_randomised_against_the_real_classes(seed):
    """Beyond the committed golden episodes: random rollouts through the REAL GraphMap and through GraphMapLite must pack
    identically, and the oracle's assembly must equal the trainer's REAL _nav_gmap_variable on them (the real side's packed
    episodes and outputs stored in tests/golden/refcheck_graph.npz)."""
    from oracle import graph_oracle as go
    from etpnav_amd.graph_inputs import GraphMapLite, pack_episode
    z = np.load(os.path.join(GOLDEN, "refcheck_graph.npz"))
    a = {k: z[f"s{seed}/{k}"] for k in ("n_nodes", "n_ghost", "cur_node", "node_pos", "node_step", "adj", "ghost_pos",
                                         "ghost_front_ptr", "ghost_front_idx", "gmap_step_ids", "gmap_visited_masks",
                                         "gmap_pos_fts", "gmap_pair_dists")}
    steps, merge = mr.graph_case(seed)
    lite = go.simulate(GraphMapLite, seed, steps, merge_ghost=merge)
    b = pack_episode(lite[0], lite[1], lite[2], lite[3])
    assert a["n_nodes"] == b["n_nodes"] and a["n_ghost"] == b["n_ghost"] and a["cur_node"] == b["cur_node"]
    for k in ("node_pos", "node_step", "adj", "ghost_pos"):
        assert a[k].shape == np.asarray(b[k]).shape and np.allclose(a[k], b[k], atol=1e-12), k
    ptr, idx = a["ghost_front_ptr"], a["ghost_front_idx"]
    assert [idx[ptr[i]:ptr[i + 1]].tolist() for i in range(len(ptr) - 1)] == b["ghost_fronts"]
    L = 1 + b["n_nodes"] + b["n_ghost"]
    got = go.assemble(b, G=L)
    assert np.array_equal(got["gmap_step_ids"], a["gmap_step_ids"])
    assert np.array_equal(got["gmap_visited_masks"], a["gmap_visited_masks"])
    assert np.abs(got["gmap_pos_fts"] - a["gmap_pos_fts"]).max() < 2e-6
    assert np.abs(got["gmap_pair_dists"] - a["gmap_pair_dists"]).max() < 2e-6


@pytest.mark.parametrize("seed", [3, 4, 5, 6])
def test_graph_map_lite_with_real_positions_and_ghost_jitter_against_the_real_class(seed):
    """The two GraphMap options the rollout driver above leaves off: has_real_pos (training keeps the simulator's positions of the
    candidates per ghost, graph_utils.py:213-214,225-226,236-237) and ghost_aug (position jitter from np.random, :245-252).  Both
    classes are driven with the same candidates and the same numpy seed; every dict of the graph must agree (the real class's
    state stored in tests/golden/refcheck.json)."""
    from etpnav_amd.graph_inputs import GraphMapLite
    a = _refcheck()["ghost_aug_drive"][str(seed)]                          # the REAL class after the same drive
    b = json.loads(json.dumps(mr.graph_state_after_ghost_aug_drive(GraphMapLite, seed)))
    edges_a, edges_b = ({(u, v): w for u, v, w in x["edges"]} for x in (a, b))
    assert edges_a.keys() == edges_b.keys() and all(abs(edges_a[k] - edges_b[k]) < 1e-12 for k in edges_a)
    assert a["node_pos"] == b["node_pos"] and dict(a["node_stepId"]) == dict(b["node_stepId"]) and a["ghost_cnt"] == b["ghost_cnt"]
    for name in ("ghost_mean_pos", "ghost_aug_pos", "ghost_pos", "ghost_real_pos"):
        da, db = a[name], b[name]
        assert [k for k, _ in da] == [k for k, _ in db], name
        assert all(np.allclose(np.asarray(va), np.asarray(vb), atol=1e-12) for (_, va), (_, vb) in zip(da, db)), name
    assert dict((k, v) for k, v in a["ghost_fronts"]) == dict((k, v) for k, v in b["ghost_fronts"])
    assert {k: (e, c) for k, e, c in a["ghost_embeds"]} == {k: (e, c) for k, e, c in b["ghost_embeds"]}
