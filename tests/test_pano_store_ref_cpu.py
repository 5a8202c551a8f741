"""Pins tests/pano_store_ref.py, the fp64 restatement that tests/test_pano_store_gpu.py holds csrc/pano_store.hip and
graph_inputs.EmbedStore to:
  * against torch autograd (float64) of the trainer's own expressions (vlnce_baselines/ss_trainer_ETP.py:838-839, 864-865), 1e-12;
  * against tests/golden/pano_store_small.npz, recorded from the real GraphMap (tools/make_golden_pano_store.py), 1e-12;
  * against graph_inputs.GraphMapLite in tensor mode, 1e-12;
  * an fp32 emulation of each kernel's schedule stays inside the derived bounds on every shape of the GPU test's lists, and those
    lists hold what they are meant to hold;
  * every planted mutation is rejected."""
import json
import os

import numpy as np
import pytest
import torch

from etpnav_amd.graph_inputs import GraphMapLite
from tests import pano_store_ref as pr

FIXTURE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "pano_store_small.npz")


@pytest.fixture(scope="module")
def fx():
    z = np.load(FIXTURE)
    d = {k: z[k] for k in z.files}
    d["plan"], d["names"] = json.loads(str(d["plan"])), json.loads(str(d["names"]))
    T, B, V, H = d["pano"].shape
    d["W"] = pr.fixture_w(int(d["w_seed"]), T, B, int(d["G"]), H)
    d["entries"], d["alloc"], d["R"] = pr.replay_plan(d["plan"], lambda: GraphMapLite(False, float(d["loc_noise"]), True, 0), snap=pr.entry_rows)
    return d


def torch_literal(x, masks, types, d_mean, d_cand):
    """the trainer's expressions under float64 autograd -> (avg_pano_embeds, [cand_embeds], d pano_embeds)"""
    pano = torch.tensor(x, dtype=torch.float64, requires_grad=True)
    m = torch.tensor(masks.astype(np.float64))
    nav_types = torch.tensor(types)
    avg = (pano * m[..., None]).sum(1) / m.sum(1, keepdim=True)             # multiplied by the mask, as the trainer does
    cands = [pano[i][nav_types[i] == 1] for i in range(x.shape[0])]
    loss = (avg * torch.tensor(d_mean)).sum()
    for c, d in zip(cands, d_cand):
        loss = loss + (c * torch.tensor(d)).sum()
    loss.backward()
    return avg.detach().numpy(), [c.detach().numpy() for c in cands], pano.grad.numpy()


@pytest.mark.parametrize("H,B,V", [(256, 3, 5), (256, 8, 13), (512, 3, 36), (768, 8, 64), (256, 1, 1)])
def test_kernels_restated_match_the_trainers_expressions(H, B, V):
    c = pr.make_case(H, B, V)
    store, st = pr.fwd(c["x"], c["masks"], c["types"], c["base"], c["ncand"], np.full((c["R"], H), 7.0))
    assert not st.any()
    d_store = c["d_store"].astype(np.float64)
    d_mean = d_store[c["base"]]
    d_cand = [d_store[c["base"][b] + 1:c["base"][b] + 1 + c["ncand"][b]] for b in range(B)]
    avg, cands, grad = torch_literal(c["x"], c["masks"], c["types"], d_mean, d_cand)
    assert np.abs(store[c["base"]] - avg).max() < 1e-12
    for b in range(B):
        assert np.array_equal(store[c["base"][b] + 1:c["base"][b] + 1 + c["ncand"][b]], cands[b])
    rows = pr.written_rows(c)
    rest = np.setdiff1d(np.arange(c["R"]), rows)
    assert len(rows) == B + c["ncand"].sum() and (store[rest] == 7.0).all()
    got = pr.bwd(d_store, c["masks"], c["types"], c["base"], c["ncand"], V)
    assert np.abs(got - grad).max() < 1e-12
    assert (got[c["masks"] == 0] == 0).all()
    acc = pr.bwd(d_store, c["masks"], c["types"], c["base"], c["ncand"], V, d_pano=np.ones((B, V, H)), accumulate=1)
    assert np.abs(acc - (1.0 + grad)).max() < 1e-12


def test_case_lists_hold_what_the_gpu_test_needs():
    assert len(pr.CASES) == 45
    counts, lens, full = set(), {}, set()
    for H, B, V in pr.CASES:
        c = pr.make_case(H, B, V)
        n = c["masks"].sum(1)
        assert not pr.flags(c["masks"], c["types"], c["base"], c["ncand"], c["R"]).any()
        assert n.max() == V and (B == 1 or n.min() == 1)                        # view lengths from 1 to V
        assert (c["x"][c["masks"] == 0] == np.float32(pr.BIG)).all() and np.isfinite(c["x"]).all()
        rows = pr.written_rows(c)
        assert len(set(rows.tolist())) == len(rows) and rows.max() < c["R"] - 1 and rows.min() >= 2        # disjoint, guards at both ends
        if B > 1:
            assert (np.diff(c["base"]) < 0).any() and len(rows) < rows.max() - rows.min() + 1             # out of order, with gaps
        for b in range(B):
            cv = np.nonzero(c["types"][b] == 1)[0]
            counts.add(len(cv))
            if len(cv) == V:
                full.add(V)
            if 0 < len(cv) < n[b] and (np.diff(cv) > 1).any() | (cv[0] > 0):
                lens[V] = True                                                   # candidates are not simply the first views
    assert counts >= {0, 1, 5, 16} and full >= {1, 5, 13} and set(lens) >= {5, 13, 36, 64}
    for name, (c, flag) in pr.malformed_cases().items():
        st = pr.flags(c["masks"], c["types"], c["base"], c["ncand"], c["R"])
        assert st.tolist() == [0, flag, 0], (name, st)
    # R exactly fitting passes, one row short flags the episode that ends there
    c = pr.make_case(256, 3, 5)
    top = int((c["base"] + 1 + c["ncand"]).max())
    assert not pr.flags(c["masks"], c["types"], c["base"], c["ncand"], top).any()
    assert (pr.flags(c["masks"], c["types"], c["base"], c["ncand"], top - 1) == pr.ERR_ROW).sum() == 1


@pytest.mark.parametrize("H,B,V", pr.CASES)
def test_fp32_schedule_stays_inside_the_bounds(H, B, V):
    c = pr.make_case(H, B, V)
    a = (c["x"], c["masks"], c["types"], c["base"], c["ncand"])
    want, _ = pr.fwd(*a, np.zeros((c["R"], H)))
    got, _ = pr.fwd(*a, np.zeros((c["R"], H), np.float32), dtype=np.float32)
    bound = pr.fwd_bound(*a, c["R"])
    assert (np.abs(got.astype(np.float64) - want) <= bound).all()
    assert (bound[c["base"]] > 0).all() and not np.delete(bound, c["base"], axis=0).any()   # candidate rows: exact
    b = a[1:]
    want = pr.bwd(c["d_store"], *b, V)
    got = pr.bwd(c["d_store"], *b, V, dtype=np.float32)
    assert (np.abs(got.astype(np.float64) - want) <= pr.bwd_bound(c["d_store"], *b, V)).all()
    old = np.random.default_rng(1).standard_normal((B, V, H)).astype(np.float32)
    want = pr.bwd(c["d_store"], *b, V, d_pano=old, accumulate=1)
    got = pr.bwd(c["d_store"], *b, V, d_pano=old, accumulate=1, dtype=np.float32)
    assert (np.abs(got.astype(np.float64) - want) <= pr.bwd_bound(c["d_store"], *b, V, d_pano=old, accumulate=1)).all()


def test_route_restated_matches_the_recording_of_the_real_graphmap(fx):
    fts, d_pano, store = pr.route(fx["pano"], fx["masks"], fx["types"], fx["entries"], fx["alloc"], fx["R"], fx["W"])
    T, B = fx["n_entries"].shape
    for t in range(T):
        for b in range(B):
            n = fx["n_entries"][t, b]
            assert len(fx["entries"][t][b]) == n
            assert np.abs(fts[t][b, :n] - fx["fts"][t, b, :n]).max() < 1e-12 and (fts[t][b, n:] == 0).all()
    assert np.abs(d_pano - fx["d_pano"]).max() < 1e-12
    # the recording holds what it is for: ghosts of two and three rows, a step without candidates, rows nothing reads, and a
    # step-0 gradient that carries what step 2 sent back
    assert sorted({len(r) for t in range(T) for b in range(B) for r, _ in fx["entries"][t][b]}) == [0, 1, 2, 3]
    assert any(len(c) == 0 for s in fx["plan"] for c in s["cand_pos"])
    _, detached, _ = pr.route(fx["pano"], fx["masks"], fx["types"], fx["entries"], fx["alloc"], fx["R"], fx["W"], mut="detach_steps")
    assert np.abs(detached[0] - fx["d_pano"][0]).max() > 1e-3 and np.array_equal(detached[T - 1], d_pano[T - 1])


def test_route_restated_matches_graphmaplite_in_tensor_mode(fx):
    T, B, V, H = fx["pano"].shape
    x = [torch.tensor(fx["pano"][t], requires_grad=True) for t in range(T)]
    def embeds(t, b):
        m = torch.tensor(fx["masks"][t].astype(np.float64))
        avg = (x[t] * m[..., None]).sum(1) / m.sum(1, keepdim=True)
        return avg[b], x[t][b][torch.tensor(fx["types"][t][b]) == 1]

    def stacked(g):
        f = [g.get_node_embeds(vp) for vp in pr.entry_names(g)]
        return torch.stack([torch.zeros_like(f[0])] + f, dim=0), pr.entry_names(g)

    snaps, _, _ = pr.replay_plan(fx["plan"], lambda: GraphMapLite(False, float(fx["loc_noise"]), True, 0), embeds=embeds, snap=stacked)
    fts, d_pano, _ = pr.route(fx["pano"], fx["masks"], fx["types"], fx["entries"], fx["alloc"], fx["R"], fx["W"])
    loss = 0.0
    for t in range(T):
        for b in range(B):
            f, names = snaps[t][b]
            assert names == fx["names"][t][b]
            assert np.abs(f.detach().numpy() - fts[t][b, :len(f)]).max() < 1e-12
            loss = loss + (f * torch.tensor(fx["W"][t, b, :len(f)])).sum()
    loss.backward()
    assert np.abs(np.stack([v.grad.numpy() for v in x]) - d_pano).max() < 1e-12


@pytest.mark.parametrize("mut", pr.MUTATIONS)
def test_planted_mutations_are_rejected(fx, mut):
    """each mutation moves the route's outputs off the recording by far more than any bound of the GPU test"""
    a = (fx["pano"], fx["masks"], fx["types"], fx["entries"], fx["alloc"], fx["R"], fx["W"])
    fts, d_pano, _ = pr.route(*a, mut=mut)
    fb, db = pr.route_fwd_bound(*a), pr.route_bwd_bound(*a)
    T, B = fx["n_entries"].shape
    off_f = max(float((np.abs(fts[t][b, :fx["n_entries"][t, b]] - fx["fts"][t, b, :fx["n_entries"][t, b]]) - fb[t][b, :fx["n_entries"][t, b]]).max())
                for t in range(T) for b in range(B))
    off_d = float((np.abs(d_pano - fx["d_pano"]) - db).max())
    if mut in ("bwd_no_mean_on_cand", "detach_steps"):          # backward-only errors: the forward is untouched and the gradient is off
        assert off_f <= 0 and off_d > 1e-3, (mut, off_f, off_d)
    else:
        assert off_f > 1e-3, (mut, off_f)
    # and the unmutated route sits inside both bounds with room to spare (they are bounds on fp32 error, the route is fp64)
    fts, d_pano, _ = pr.route(*a)
    assert float(np.abs(d_pano - fx["d_pano"]).max()) < 1e-12 and (db >= 0).all() and db.max() < 1e-4
    assert all(f.max() < 1e-4 for f in fb)


def test_operator_mutations_are_rejected_on_the_operator_cases():
    c = pr.make_case(256, 8, 13)
    a = (c["x"], c["masks"], c["types"], c["base"], c["ncand"])
    want, _ = pr.fwd(*a, np.zeros((c["R"], 256)))
    bound = pr.fwd_bound(*a, c["R"])
    for mut in ("mean_all_v", "div_by_v", "cand_reversed", "cand_by_mask", "base_off_by_one"):
        got, _ = pr.fwd(*a, np.zeros((c["R"], 256)), mut=mut)
        assert (np.abs(got - want) > bound + 1e-3).any(), mut
    want = pr.bwd(c["d_store"], *a[1:], 13)
    got = pr.bwd(c["d_store"], *a[1:], 13, mut="bwd_no_mean_on_cand")
    assert (np.abs(got - want) > pr.bwd_bound(c["d_store"], *a[1:], 13) + 1e-3).any()
