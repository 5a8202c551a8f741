"""Pins tests/gmap_update_ref.py, the fp64 restatement the GPU tests of csrc/gmap_update.hip compare against: it replays the recording of
the REAL GraphMap (tests/golden/gmap_update_small.npz, tools/make_golden_gmap_update.py) with every double equal, it equals GraphMapLite
+ pack_batch + pack_img_csr element for element on simulate_rollout episodes, the conditions of the GPU comparison hold for every rollout of
gmap_update_ref.ROLLOUTS -- the one table both this file and the GPU test build their calls from (no candidate is excluded), and every mutation in gmap_update_ref.MUTATIONS changes its outputs."""
import json
import os

import numpy as np
import pytest

from etpnav_amd.graph_inputs import GraphMapLite, pack_batch, pack_episode, pack_img_csr
from etpnav_amd.synthetic import simulate_rollout
from tests import gmap_update_ref as gr

FIXTURE = os.path.join(os.path.dirname(__file__), "golden", "gmap_update_small.npz")


def test_replays_the_recording_of_the_real_graphmap():
    log = gr.load_fixture(FIXTURE)
    assert [r["merge_ghost"] for r in log] == [True, False, True] and any(any(r["has_real_pos"]) for r in log)
    kinds, deletions = set(), 0
    for r, run in enumerate(log):
        ref = gr.RefBatch(3, run["loc_noise"], run["merge_ghost"], 0.0)
        for t, step in enumerate(run["steps"]):
            o = ref.update(**gr.call_from_fixture(step))
            assert (o["record"][:, 2] == 0).all()
            kinds |= {int(x) >> 24 for x in o["record"][:, gr.HDR:].ravel() if x >= 0}
            deletions += sum(d >= 0 for d in step["del_ghost"])
            for b, s in enumerate(step["slot"]):
                want = dict(step["after"][b])
                want.pop("ghost_real_pos")
                got = json.loads(json.dumps(gr.slot_state(ref.slots[s])))
                for k in want:                                 # lists of doubles compare with ==: equal as doubles
                    assert got[k] == want[k], f"run {r} step {t} episode {b}: {k}"
                assert o["record"][b, :2].tolist() == [len(want["nodes"]), len(want["ghosts"])]
        assert gr.check_conditions(ref.margins, run["loc_noise"], f"run {r}") > 0
    assert kinds == {gr.EDGE, gr.NEW, gr.MERGED} and deletions >= 6


class AsGraphMap:
    """one slot of a RefBatch behind the interface simulate_rollout drives (identify_node / update_graph / delete_ghost)"""

    def __init__(self, batch, slot, row_offset):
        self.batch, self.slot, self.row_offset, self.pending, self.out = batch, slot, row_offset, -1, None
        self.lite = GraphMapLite(False, batch.loc_noise, batch.merge, 0)

    node_pos = property(lambda self: {str(i): p for i, p in enumerate(self.batch.slots[self.slot].node_pos)})
    ghost_pos = property(lambda self: {f"g{g}": p for g, p in zip(self.batch.slots[self.slot].gid, self.batch.slots[self.slot].gpos)})
    ghost_aug_pos = property(lambda self: {f"g{g}": p for g, p in zip(self.batch.slots[self.slot].gid, self.batch.slots[self.slot].gaug)})

    def identify_node(self, *a):
        _, _, cand_pos = self.lite.identify_node(*a)          # the positions; the names count THIS map's nodes
        vp = str(len(self.node_pos))
        return vp, [f"{vp}_{k}" for k in range(len(cand_pos))], cand_pos

    def delete_ghost(self, vp):
        self.pending = list(self.ghost_pos.keys()).index(vp)

    def update_graph(self, prev_vp, step_id, cur_vp, cur_pos, cur_row, cand_vp, cand_pos, cand_rows, _):
        K = len(cand_pos)
        cand = np.zeros((1, gr.KMAX, 3)); cand[0, :K] = np.asarray(cand_pos).reshape(K, 3)
        rows = np.full((1, gr.KMAX), -1, np.int32); rows[0, :K] = np.asarray(cand_rows) + self.row_offset
        self.out = self.batch.update(np.array([self.slot], np.int32), np.array([-1 if prev_vp is None else int(prev_vp)], np.int32),
                                     np.array([step_id], np.int32), np.asarray(cur_pos, dtype=np.float64).reshape(1, 3), np.zeros(1, np.float32),
                                     cand, np.array([K], np.int32), np.array([cur_row + self.row_offset], np.int32), rows,
                                     np.array([self.pending], np.int32))
        self.pending = -1


@pytest.mark.parametrize("merge", [True, False])
def test_equals_graphmaplite_pack_batch_and_pack_img_csr(merge):
    seeds = [3, 4, 5, 6]
    batch = gr.RefBatch(len(seeds), 0.5, merge, 0.0)
    lites, offsets, R = [], [], 0
    for s, seed in enumerate(seeds):
        lite, cur_vp, pos, heading, store = simulate_rollout(GraphMapLite, seed, 7, merge_ghost=merge, rows_mode=True)
        made = []
        simulate_rollout(lambda *a: made.append(AsGraphMap(batch, s, R)) or made[-1], seed, 7, merge_ghost=merge, rows_mode=True)
        want = pack_batch([pack_episode(lite, cur_vp, pos, 0.0)])
        B, Nmax, Mmax, Fmax = want["_dims"]
        got = made[0].out
        assert got["record"][0, :4].tolist() == [want["n_nodes"][0], want["n_ghost"][0], 0, want["cur_node"][0]]
        for k in ("n_nodes", "n_ghost", "cur_node", "cur_pos"):
            assert np.array_equal(got[k], want[k]), k
        assert np.array_equal(got["node_pos"][:, :Nmax], want["node_pos"]) and not got["node_pos"][:, Nmax:].any()
        assert np.array_equal(got["node_step"][:, :Nmax], want["node_step"]) and not got["node_step"][:, Nmax:].any()
        assert np.array_equal(got["adj"][:, :Nmax, :Nmax], want["adj"])
        assert (got["adj"][:, Nmax:] == -1).all() and (got["adj"][:, :, Nmax:] == -1).all()
        assert np.array_equal(got["ghost_pos"][:, :Mmax], want["ghost_pos"][:, :Mmax]) and not got["ghost_pos"][:, Mmax:].any()
        assert np.array_equal(got["front_ptr"][:, :Mmax + 1], want["front_ptr"]) and (got["front_ptr"][:, Mmax + 1:] == want["front_ptr"][0, -1]).all()
        nf = int(want["front_ptr"][0, -1])
        assert np.array_equal(got["front_idx"][:, :nf], want["front_idx"][:, :nf]) and not got["front_idx"][:, nf:].any()
        lites.append(lite); offsets.append(R)
        R += len(store)
    G = max(1 + len(l.node_pos) + len(l.ghost_pos) for l in lites) + 2
    fwd, bwd = pack_img_csr(lites, offsets, G, R)
    gf, gb, status = batch.embed_csr(list(range(len(seeds))), G, R)
    assert not status.any()
    for a, b in zip(list(gf) + list(gb), list(fwd) + list(bwd)):
        assert a.dtype == b.numpy().dtype and np.array_equal(a, b.numpy())
    with pytest.raises(ValueError):
        pack_img_csr(lites, offsets, G - 3 - min(len(l.ghost_pos) for l in lites) - 64, R)
    assert batch.embed_csr([0], 2, R)[2].tolist() == [gr.ERR_CAPACITY]


@pytest.mark.parametrize("name", list(gr.ROLLOUTS))
def test_conditions_of_the_gpu_comparison_hold_for_every_rollout_of_the_table(name):
    calls, _, B, S = gr.rollout(name)                          # exactly the calls tests/test_gmap_update_gpu.py runs
    _, steps, K, _, _ = gr.ROLLOUTS[name]
    for merge in (True, False):
        ref = gr.RefBatch(S, 0.5, merge, 0.3)
        for c in calls:
            assert (ref.update(**c)["record"][:, 2] == 0).all()
        n = gr.check_conditions(ref.margins, 0.5, f"{name} merge {merge}")      # asserts: 0 candidates are excluded
        assert n >= (B * steps * K if K else 0)


def test_grid_of_the_table_and_crafted_rollouts():
    assert {(v[0], v[2]) for v in gr.ROLLOUTS.values()} >= {(B, K) for B in (1, 3, 8) for K in (0, 1, 5, 16)}
    assert all(v[4] >= v[0] for v in gr.ROLLOUTS.values())
    ref = gr.RefBatch(1, 5.0, True, 0.0)
    for c, want in zip(gr.lattice_calls(), gr.LATTICE_CODES):
        o = ref.update(**c)
        assert o["record"][0, gr.HDR:gr.HDR + len(want)].tolist() == want
    assert ref.slots[0].gfront == [[1, 1, 1], [2]] and ref.slots[0].gid == [1, 2] and ref.slots[0].gmean[0].tolist() == [43.5, 0.0, 0.0]
    assert ref.slots[0].edges == {(0, 0): 0.0, (0, 1): 8.0, (1, 2): np.sqrt(425.0), (2, 2): 0.0, (2, 3): 3.0}
    gr.check_conditions(ref.margins, 5.0, "lattice")
    # the merge-heavy rollout: exact by construction; it ends at the absorbed-candidate capacity with a tail of > 256 entries
    ref = gr.RefBatch(1, 5.0, True, 0.0)
    for i, c in enumerate(gr.merge_heavy_calls()):
        o = ref.update(**c)
        assert o["record"][0, :6].tolist() == [i + 1, 2, 0, i, 2, 16 * (i + 1)]
    s = ref.slots[0]
    assert [len(f) for f in s.gfront] == [121, 391] and s.gmean[0].tolist() == [1000.0, 0.0, 0.0] and s.gmean[1].tolist() == [2000.0, 0.0, 0.0]
    gr.check_conditions(ref.margins, 5.0, "merge-heavy")
    more = dict(gr.merge_heavy_calls()[0], prev_node=np.array([31], np.int32), n_cand=np.array([1], np.int32))
    assert ref.update(**more)["record"][0, 2] == gr.ERR_CAPACITY and ref.update(**dict(more, n_cand=np.array([0], np.int32)))["record"][0, 2] == 0


def run_all(mut):
    """every output of the lattice calls and of one random rollout with deletions, under a mutation (None: none)"""
    outs = []
    for calls, S, ln in ((gr.lattice_calls(), 1, 5.0), (gr.rollout("mutations")[0], 3, 0.5)):
        ref = gr.RefBatch(S, ln, True, 0.0, mut=mut)
        for c in calls:
            o = ref.update(**c)
            outs += [o[k] for k in sorted(o)]
        f, b, st = ref.embed_csr(list(range(S)), 64, 200)
        outs += list(f) + list(b)
    return outs


@pytest.mark.parametrize("mut", gr.MUTATIONS)
def test_mutations_are_rejected(mut):
    base, got = run_all(None), run_all(mut)
    assert any(a.shape != b.shape or not np.array_equal(a, b) for a, b in zip(base, got)), f"mutation {mut} changes nothing"


def test_capacity_and_malformed_input_leave_the_slot_alone():
    ref = gr.RefBatch(2, 0.5, True, 0.0)
    c = gr.random_calls(1, 1, 2, 0, S=2)[0][0]
    ref.update(**c)
    before = json.dumps(gr.slot_state(ref.slots[int(c["slot"][0])]))
    for bad in (dict(prev_node=np.array([5], np.int32)), dict(prev_node=np.array([-2], np.int32)), dict(del_ghost=np.array([7], np.int32)),
                dict(n_cand=np.array([17], np.int32)), dict(n_cand=np.array([-1], np.int32)), dict(slot=np.array([2], np.int32))):
        o = ref.update(**dict(c, **bad))
        assert o["record"][0, :gr.HDR].tolist() == [0, 0, gr.ERR_INPUT, -1, 0, 0, 0, 0] and (o["record"][0, gr.HDR:] == -1).all()
        assert o["n_nodes"][0] == 0 and json.dumps(gr.slot_state(ref.slots[int(c["slot"][0])])) == before
