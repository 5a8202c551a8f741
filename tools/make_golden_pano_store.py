"""Write tests/golden/pano_store_small.npz from the REAL reference code (build container only; needs the reference tree and networkx).

    python tools/make_golden_pano_store.py --reference <root of the reference tree>

A T = 3, B = 2, V = 6, H = 256 rollout of the store's part of RLTrainer.rollout through the real GraphMap
(vlnce_baselines/models/graph_utils.py) with float64 tensors and merge_ghost on: per step the masked panorama mean and the candidate
selection (vlnce_baselines/ss_trainer_ETP.py:838-839, 864-865), update_graph (:866-869) and the stacked gmap_img_fts of
_nav_gmap_variable (:360-365).  The plan (PLAN below) makes candidates fall on a visited node (an edge, no row used), join an
earlier ghost (ghost embeddings of two and three rows, across steps), open new ghosts, one step without candidates, and ghosts
deleted before the next update as consume_ghost does.  Recorded: the inputs (pano_embeds, fp32-representable, 1e30 at masked-out views;
masks; nav_types; the plan), per step gmap_img_fts padded to G entries with the entry counts, and d pano_embeds of every step for the
loss sum_t (gmap_img_fts_t * W_t).sum() with W from the recorded seed (tests/pano_store_ref.fixture_w).  The file holds data only.
The restatement (tests/pano_store_ref.route) must reproduce the recording to 1e-12 or nothing is written.
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from etpnav_amd.graph_inputs import GraphMapLite  # noqa: E402
from tests import pano_store_ref as pr  # noqa: E402
from tools.make_golden_decide import load_graph_utils  # noqa: E402

OUT = os.path.join(ROOT, "tests", "golden", "pano_store_small.npz")
T, B, V, H, G, LOC_NOISE, SEED, W_SEED = 3, 2, 6, 256, 8, 0.5, 20261019, 77
PLAN = [
    dict(cur_pos=[[0, 0, 0], [0, 0, 10]], prev_vp=[None, None], delete=[None, None],
         cand_pos=[[[1.5, 0, 0], [0, 0, 1.5]], [[1, 0, 10], [0, 0, 11], [1.2, 0, 10.1]]]),               # episode 1: the third joins g0
    dict(cur_pos=[[1.5, 0, 0], [0, 0, 11]], prev_vp=["0", "0"], delete=["g0", "g1"],
         cand_pos=[[[0.1, 0, 0.1], [0.1, 0, 1.4], [3, 0, 0]], []]),                                      # edge to node 0, joins g1, new g2 | none
    dict(cur_pos=[[3, 0, 0], [1, 0, 10.5]], prev_vp=["1", "1"], delete=["g2", None],
         cand_pos=[[[0.05, 0, 1.45]], [[1.1, 0, 10.05], [5, 0, 5]]]),                                    # g1 holds three rows | g0 three, new g2
]


def inputs():
    rng = np.random.default_rng(SEED)
    pano = rng.standard_normal((T, B, V, H)).astype(np.float32).astype(np.float64)
    masks, types = np.zeros((T, B, V), np.uint8), np.zeros((T, B, V), np.int64)
    for t in range(T):
        for b in range(B):
            k = len(PLAN[t]["cand_pos"][b])
            n = min(V, k + 2 + (t + b) % 2)
            masks[t, b, :n] = 1
            types[t, b, np.sort(rng.permutation(n)[:k])] = 1       # candidates interleaved with panorama views
            types[t, b, n:] = 2
    pano[masks == 0] = pr.BIG
    return pano, masks, types


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reference", required=True)
    a = ap.parse_args()
    gu = load_graph_utils(a.reference)
    pano, masks, types = inputs()
    W = pr.fixture_w(W_SEED, T, B, G, H)
    x = [torch.tensor(pano[t], requires_grad=True) for t in range(T)]
    per_step = []

    def embeds(t, b):
        if b == 0:                                                 # the trainer's statements, once per step for the batch
            m = torch.tensor(masks[t].astype(np.float64))
            per_step.append((x[t] * m[..., None]).sum(1) / m.sum(1, keepdim=True))     # the masked mean, multiplied by the mask as the trainer does
        return per_step[t][b], x[t][b][torch.tensor(types[t][b]) == 1]

    def stacked(gmap):                                             # ss_trainer_ETP.py:351-365
        names = pr.entry_names(gmap)                               # nodes, then ghosts; a zero row for [stop] in front
        f = [gmap.get_node_embeds(vp) for vp in names]
        return torch.stack([torch.zeros_like(f[0])] + f, dim=0), names

    snaps, _, _ = pr.replay_plan(PLAN, lambda: gu.GraphMap(False, LOC_NOISE, True, 0), embeds=embeds, snap=stacked)
    fts, n_entries, loss = np.zeros((T, B, G, H)), np.zeros((T, B), np.int32), 0.0
    names = []
    for t in range(T):
        for b in range(B):
            f, nm = snaps[t][b]
            n_entries[t, b] = f.shape[0]
            fts[t, b, :f.shape[0]] = f.detach().numpy()
            loss = loss + (f * torch.tensor(W[t, b, :f.shape[0]])).sum()
        names.append([snaps[t][b][1] for b in range(B)])
    loss.backward()
    d_pano = np.stack([x[t].grad.numpy() for t in range(T)])

    # ---- the restatement reproduces the recording; the plan shows what it is meant to ----
    entries, alloc, R = pr.replay_plan(PLAN, lambda: GraphMapLite(False, LOC_NOISE, True, 0), snap=pr.entry_rows)
    r_fts, r_d, _ = pr.route(pano, masks, types, entries, alloc, R, W)
    for t in range(T):
        for b in range(B):
            n = n_entries[t, b]
            assert len(entries[t][b]) == n and np.abs(r_fts[t][b, :n] - fts[t, b, :n]).max() < 1e-12, (t, b)
    assert np.abs(r_d - d_pano).max() < 1e-12
    sizes = sorted({len(rows) for t in range(T) for b in range(B) for rows, _ in entries[t][b]})
    assert sizes == [0, 1, 2, 3], sizes
    assert R > sum(len(rows) for b in range(B) for rows, _ in entries[T - 1][b]), "no row went unused (edge / deleted ghost)"
    np.savez_compressed(OUT, pano=pano, masks=masks, types=types, plan=np.array(json.dumps(PLAN)), names=np.array(json.dumps(names)),
                        loc_noise=LOC_NOISE, w_seed=W_SEED, G=G, fts=fts, n_entries=n_entries, d_pano=d_pano)
    print(f"{OUT}: {os.path.getsize(OUT)} bytes; T={T} B={B} V={V} H={H}, rows {R}, entries {n_entries.tolist()}")


if __name__ == "__main__":
    main()
