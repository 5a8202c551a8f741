"""Write tests/golden/gmap_update_small.npz from the REAL reference code (build container only; needs the reference tree and networkx).

    python tools/make_golden_gmap_update.py --reference <root of the reference tree>

Drives the real GraphMap (vlnce_baselines/models/graph_utils.py) through multi-step rollouts and records, for every step, the inputs
of the update (slots, previous node, pose, candidate positions, rows of the embedding store, the ghost deleted before it) and the
state after it: node order, edges, ghost ids in order, the position of every absorbed candidate, mean positions, fronts, row
lists, ghost_cnt and, where has_real_pos is on, the real positions.  Three runs of three episodes and six steps each
(tests/gmap_update_ref.random_calls: candidates near earlier nodes and earlier candidates, so edges and merges occur; most steps
move to a ghost, which is deleted before the next update, as consume_ghost does):
  run 0  merge_ghost on        run 1  merge_ghost off        run 2  merge_ghost on, has_real_pos on for episode 1
The embeddings handed to the reference are 1-tuples holding a row number: its running sum ``ghost_embeds[g][0] + cembeds`` then IS the
list of absorbed rows.  ghost_aug is 0 (the reference draws from numpy's global stream).  No program text of the reference goes into
the file: one JSON string of inputs and recorded states.  The restatement (tests/gmap_update_ref.RefBatch) must replay the recording
exactly -- discrete state and every double -- and its conditions must hold, or nothing is written.
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from tests import gmap_update_ref as gr  # noqa: E402
from tools.make_golden_decide import load_graph_utils  # noqa: E402

OUT = os.path.join(ROOT, "tests", "golden", "gmap_update_small.npz")
RUNS = [dict(seed=11, merge_ghost=True, real=[]), dict(seed=12, merge_ghost=False, real=[]), dict(seed=13, merge_ghost=True, real=[1])]
LOC_NOISE, B, STEPS = 0.5, 3, 6


def real_state(g):
    ghosts = list(g.ghost_pos.keys())
    return dict(nodes=list(g.node_pos.keys()), node_pos=[np.asarray(p, dtype=np.float64).tolist() for p in g.node_pos.values()],
                node_step=[int(x) for x in g.node_stepId.values()],
                edges=sorted([min(u, v, key=int), max(u, v, key=int), float(w)] for u, v, w in g.graph_nx.edges(data="weight")),
                ghosts=ghosts, ghost_pos=[[np.asarray(p, dtype=np.float64).tolist() for p in g.ghost_pos[k]] for k in ghosts],
                ghost_mean=[np.asarray(g.ghost_mean_pos[k], dtype=np.float64).tolist() for k in ghosts],
                ghost_fronts=[list(g.ghost_fronts[k]) for k in ghosts], ghost_rows=[[int(r) for r in g.ghost_embeds[k][0]] for k in ghosts],
                ghost_cnt=int(g.ghost_cnt),
                ghost_real_pos=[[list(map(float, p)) for p in g.ghost_real_pos[k]] for k in ghosts] if g.has_real_pos else None)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reference", required=True)
    a = ap.parse_args()
    gu = load_graph_utils(a.reference)
    log = []
    kinds = set()
    for run in RUNS:
        calls, _ = gr.random_calls(B, STEPS, None, run["seed"])
        slots = calls[0]["slot"].tolist()
        gmaps = {s: gu.GraphMap(b in run["real"], LOC_NOISE, run["merge_ghost"], 0) for b, s in enumerate(slots)}
        ref = gr.RefBatch(B, LOC_NOISE, run["merge_ghost"], 0.0)
        steps = []
        deleted_middle = False
        for c in calls:
            real_pos = [[(c["cand_pos"][b, k] + [0.01, 0.0, -0.01]).tolist() for k in range(int(c["n_cand"][b]))] for b in range(B)]
            states = []
            for b, s in enumerate(slots):
                g, K, d = gmaps[s], int(c["n_cand"][b]), int(c["del_ghost"][b])
                if d >= 0:
                    deleted_middle |= d < len(g.ghost_pos) - 1
                    g.delete_ghost(list(g.ghost_pos.keys())[d])
                vp = str(len(g.node_pos))
                prev = None if c["prev_node"][b] < 0 else str(int(c["prev_node"][b]))
                g.update_graph(prev, int(c["step_id"][b]), vp, c["cur_pos"][b].copy(), (int(c["cur_row"][b]),), [f"{vp}_{k}" for k in range(K)],
                               [c["cand_pos"][b, k].copy() for k in range(K)], [(int(c["cand_row"][b, k]),) for k in range(K)], real_pos[b])
                states.append(real_state(g))
            step = dict(slot=slots, prev_node=c["prev_node"].tolist(), step_id=c["step_id"].tolist(), cur_pos=c["cur_pos"].tolist(),
                        cur_heading=c["cur_heading"].astype(np.float64).tolist(), cand_pos=[c["cand_pos"][b, :int(c["n_cand"][b])].tolist() for b in range(B)],
                        cand_row=[c["cand_row"][b, :int(c["n_cand"][b])].tolist() for b in range(B)], cur_row=c["cur_row"].tolist(),
                        del_ghost=c["del_ghost"].tolist(), cand_real_pos=real_pos, after=states)
            step = json.loads(json.dumps(step))
            # ---- the restatement replays the step exactly ----
            o = ref.update(**gr.call_from_fixture(step))
            assert (o["record"][:, 2] == 0).all()
            kinds |= {int(x) >> 24 for x in o["record"][:, gr.HDR:].ravel() if x >= 0}
            for b, s in enumerate(slots):
                want = dict(step["after"][b])
                want.pop("ghost_real_pos")
                got = json.loads(json.dumps(gr.slot_state(ref.slots[s])))
                assert got == want, (run, b, [k for k in want if got[k] != want[k]])
            steps.append(step)
        assert deleted_middle, "no deletion in front of a remaining ghost"
        gr.check_conditions(ref.margins, LOC_NOISE, f"run seed {run['seed']}")
        log.append(dict(loc_noise=LOC_NOISE, merge_ghost=run["merge_ghost"], has_real_pos=[b in run["real"] for b in range(B)], steps=steps))
    assert kinds == {gr.EDGE, gr.NEW, gr.MERGED}, kinds
    np.savez_compressed(OUT, log=np.array(json.dumps(log)))
    print(f"{OUT}: {os.path.getsize(OUT)} bytes; {len(log)} runs x {STEPS} steps x {B} episodes")


if __name__ == "__main__":
    main()
