"""tests/traj_nodes_ref.py (the numpy restatement of etp_traj_nodes_fwd / _bwd from the integer tables) pinned to everything that already
states GlobalMapEncoder._aggregate_gmap_features (pretrain_src/pretrain_src/model/vilmodel.py:585-619): graph_inputs.pack_traj_csr applied
densely, the oracle's loop, the recording of the real method (tests/golden/traj_agg.npz); graph_inputs.traj_descriptors and the tables the
native loaders cache pinned to the restatement's own tables; and the mutations those pins must reject.  No GPU."""
import os

import numpy as np
import pytest
import torch

from tests import traj_nodes_ref as tr
from etpnav_amd.graph_inputs import pack_traj_csr, traj_descriptors

HERE = os.path.dirname(os.path.abspath(__file__))


def _csr(traj, V, G):
    return pack_traj_csr(traj["traj_vp_lens"], traj["traj_vpids"], traj["traj_cand_vpids"], traj["gmap_vpids"], V, G)


def _cases():
    """(name, traj, V, G): the crafted samples at three view counts and random trajectories with slots beyond V"""
    out = []
    for V in (1, 5, 7):
        t = tr.crafted(V)
        out.append((f"crafted V={V}", t, V, 9))
    rng = np.random.RandomState(5)
    for k in range(6):
        V = int(rng.randint(1, 8))
        t = tr.random_traj(rng, int(rng.randint(1, 5)), V, [1, 2, 5, 3], [0, 1, 5, 9])
        out.append((f"random {k}", t, V, max(len(g) for g in t["gmap_vpids"]) + (k % 2)))
    return out


CASES = _cases()


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


@pytest.mark.parametrize("name,traj,V,G", CASES, ids=[c[0] for c in CASES])
def test_restatement_equals_pack_traj_csr_applied_densely(name, traj, V, G):
    """forward and backward, float64 to rounding and the fp32 loop bit for bit; no status word set; padding and [stop] exact zeros"""
    rng = np.random.RandomState(1)
    tb = tr.tables(traj, G)
    B, R, H = len(traj["traj_vpids"]), len(tb["step_vp"]), 6
    pano, dg = tr.scaled_rows(rng, R * V, H), tr.scaled_rows(rng, B * G, H)
    f, b = _csr(traj, V, G)
    for dtype in (np.float64, np.float32):
        out, st, mag, terms = tr.forward(pano, tb, V, dtype)
        want = tr.dense_csr(f, pano, B * G, dtype)
        dp, stb, _, _ = tr.backward(dg, tb, V, dtype)
        wantb = tr.dense_csr(b, dg, R * V, dtype)
        assert not st.any() and not stb.any()
        if dtype == np.float32:
            assert np.array_equal(_bits(out), _bits(want)) and np.array_equal(_bits(dp), _bits(wantb))
        else:
            assert np.abs(out - want).max() <= 1e-15 * max(1.0, np.abs(want).max())
            assert np.abs(dp - wantb).max() <= 1e-15 * max(1.0, np.abs(wantb).max())
    pf = np.asarray(f[0])
    assert np.array_equal(terms, pf[1:] - pf[:-1])
    for i in range(B):
        ln = len(traj["gmap_vpids"][i])
        assert not out[i * G].any() and not out[i * G + ln:(i + 1) * G].any()


@pytest.mark.parametrize("name,traj,V,G", CASES, ids=[c[0] for c in CASES])
def test_backward_is_the_exact_adjoint(name, traj, V, G):
    """<F x, y> = <x, F^T y> in float64, and the backward of a one-hot gradient is the forward's column: the same weights, entry for entry"""
    rng = np.random.RandomState(2)
    tb = tr.tables(traj, G)
    B, R = len(traj["traj_vpids"]), len(tb["step_vp"])
    x, y = rng.standard_normal((R * V, 3)), rng.standard_normal((B * G, 3))
    fx, bty = tr.forward(x, tb, V)[0], tr.backward(y, tb, V)[0]
    assert abs((fx * y).sum() - (x * bty).sum()) <= 1e-12 * max(1.0, np.abs(fx * y).sum())
    F = tr.forward(np.eye(R * V), tb, V)[0]                     # [B*G, R*V]: the operator itself
    Ft = tr.backward(np.eye(B * G), tb, V)[0]                   # [R*V, B*G]
    assert np.array_equal(F.T, Ft)


def test_restatement_equals_the_oracle_on_25_random_trajectories():
    """the trajectories of test_trajectory_csr_equals_oracle_aggregation_on_random_trajectories, against the oracle's loop"""
    from oracle import planner_oracle as po
    rng = np.random.RandomState(0)
    for trial in range(25):
        B, V, H = rng.randint(1, 5), rng.randint(3, 9), 4
        lens, vpids, cands, gvps, embeds = [], [], [], [], []
        for i in range(B):
            T = rng.randint(1, 6)
            names = [f"n{i}_{k}" for k in range(8)]
            path = [names[rng.randint(0, 4)] for _ in range(T)]
            ep_lens = [int(rng.randint(1, V + 1)) for _ in range(T)]
            mx = max(ep_lens)
            ep_c = [[names[rng.randint(0, 8)] for _ in range(rng.randint(0, mx + 1))] for _ in range(T)]
            seen = []
            for t in range(T):
                for vp in [path[t]] + ep_c[t]:
                    if vp not in seen:
                        seen.append(vp)
            lens.append(ep_lens); vpids.append(path); cands.append(ep_c); gvps.append([None] + seen)
            embeds.append(torch.from_numpy(rng.standard_normal((T, V, H)).astype(np.float32)))
        flat = torch.cat(embeds, 0)
        traj = {"traj_step_lens": [len(e) for e in embeds], "traj_vp_lens": lens, "traj_vpids": vpids, "traj_cand_vpids": cands,
                "gmap_vpids": gvps}
        want = po.aggregate_gmap_features(flat, traj).numpy()
        G = want.shape[1]
        tb = tr.tables(traj, G)
        out, st, _, _ = tr.forward(flat.reshape(-1, H).numpy(), tb, V)
        assert not st.any()
        assert np.abs(out.reshape(B, G, H) - want).max() < 1e-5, trial
        assert tr.same_up_to_renaming(tb, _desc(traj, G)), trial


def test_restatement_equals_the_recording_of_the_real_method():
    from oracle.make_golden_traj import make_case
    want = np.load(os.path.join(HERE, "golden", "traj_agg.npz"))["out"]
    embeds, lens, vpids, cands, gvps = make_case()
    V, H = embeds[0].shape[1], embeds[0].shape[2]
    G = want.shape[1] + 2
    traj = {"traj_vp_lens": [l.tolist() for l in lens], "traj_vpids": vpids, "traj_cand_vpids": cands, "gmap_vpids": gvps}
    out, st, _, _ = tr.forward(torch.cat(embeds, 0).reshape(-1, H).numpy(), tr.tables(traj, G), V)
    out = out.reshape(len(embeds), G, H)
    assert not st.any()
    assert np.abs(out[:, :want.shape[1]] - want).max() < 1e-6
    assert not out[:, want.shape[1]:].any() and not out[:, 0].any()


def _desc(traj, G):
    d = traj_descriptors(traj, G, "cpu")
    out = {k: d[k].numpy() for k in d if k != "Kmax"}
    assert out["cand_vp"].shape[1] == d["Kmax"] and all(v.dtype == np.int32 for v in out.values())
    return out


@pytest.mark.parametrize("name,traj,V,G", CASES, ids=[c[0] for c in CASES])
def test_traj_descriptors_are_the_restatements_tables(name, traj, V, G):
    """the same tables up to the renaming of ids, -1 in [stop] and in every padding entry; so the restatement gives the same result on both"""
    tb, d = tr.tables(traj, G), _desc(traj, G)
    assert tr.same_up_to_renaming(tb, d) and tr.same_up_to_renaming(d, tb)
    for t in range(len(d["step_vp"])):
        assert (d["cand_vp"][t, d["cand_count"][t]:] == -1).all()
    for i, ln in enumerate(d["gmap_len"]):
        assert d["gmap_id"][i, 0] == -1 and (d["gmap_id"][i, ln:] == -1).all()
    rng = np.random.RandomState(3)
    pano = rng.standard_normal((len(tb["step_vp"]) * V, 4))
    d["view_lens"] = tb["view_lens"]
    assert np.array_equal(tr.forward(pano, tb, V)[0], tr.forward(pano, d, V)[0])


def test_traj_descriptors_refuse_what_the_kernels_cannot_take():
    t = tr.crafted(5)
    with pytest.raises(ValueError, match="graph entries"):
        traj_descriptors(t, 7, "cpu")
    t["traj_cand_vpids"][0][0] = ["g"] * 65
    with pytest.raises(ValueError, match="at most 64"):
        traj_descriptors(t, 9, "cpu")
    t = tr.crafted(5)
    t["traj_cand_vpids"][0] = t["traj_cand_vpids"][0][:-1]
    with pytest.raises(ValueError, match="different batches"):
        traj_descriptors(t, 9, "cpu")


def test_cached_record_tables_equal_traj_descriptors_on_the_fixture_corpus():
    """R2RTextPathIndex.record caches step_vp / cand_vp as graph indices in gmap_idx's index space: with gmap_idx they are
    traj_descriptors of the record's own string lists up to the renaming of ids, for every item and every end index"""
    from tests import pretrain_data_ref as rf
    index = rf.make_index()
    n = 0
    for i in range(len(index)):
        for e in range(len(index.data[i]["path"])):
            rec = index.record(i, e)
            T, G = len(rec["traj_vpids"]), len(rec["gmap_vpids"])
            assert rec["step_vp"].dtype == np.int32 and rec["cand_vp"].dtype == np.int32 and rec["step_vp"].shape == (T,)
            assert rec["cand_vp"].shape == (T, max(1, max(len(c) for c in rec["traj_cand_vpids"])))
            mine = {"step_off": np.array([0, T], np.int32), "step_vp": rec["step_vp"], "cand_vp": rec["cand_vp"],
                    "cand_count": np.array([len(c) for c in rec["traj_cand_vpids"]], np.int32), "gmap_id": rec["gmap_idx"][None],
                    "gmap_len": np.array([G], np.int32)}
            traj = {"traj_vpids": [rec["traj_vpids"]], "traj_cand_vpids": [rec["traj_cand_vpids"]], "gmap_vpids": [rec["gmap_vpids"]]}
            assert tr.same_up_to_renaming(mine, _desc(traj, G)), (i, e)
            for t, c in enumerate(rec["traj_cand_vpids"]):
                assert (rec["cand_vp"][t, len(c):] == -1).all()
            n += 1
    assert n >= 8


def _mutation_inputs():
    """crafted(5) + a random batch: every planted mutation changes some row of one of them"""
    V = 5
    traj = tr.concat(tr.crafted(V), tr.random_traj(np.random.RandomState(9), 3, V, [5, 2, 3], [0, 1, 5, 7]))
    G = max(len(g) for g in traj["gmap_vpids"]) + 1
    tb = tr.tables(traj, G)
    rng = np.random.RandomState(4)
    return traj, tb, V, G, tr.scaled_rows(rng, len(tb["step_vp"]) * V, 6), tr.scaled_rows(rng, len(traj["traj_vpids"]) * G, 6)


@pytest.mark.parametrize("mutation", tr.FWD_MUTATIONS)
def test_forward_pins_reject_planted_mutations(mutation):
    traj, tb, V, G, pano, _ = _mutation_inputs()
    want = tr.dense_csr(_csr(traj, V, G)[0], pano, len(traj["traj_vpids"]) * G)
    good, bad = tr.forward(pano, tb, V)[0], tr.forward(pano, tb, V, mutate=mutation)[0]
    tol = 1e-15 * np.abs(want).max()
    assert np.abs(good - want).max() <= tol
    assert np.abs(bad - want).max() > 1e-6 * np.abs(want).max(), mutation


def test_backward_in_descending_node_order_is_caught_at_bit_level():
    """two nodes read a row in (A) + (B): adding them in the other order moves last bits only, and the fp32 pin sees it"""
    traj, tb, V, G, _, dg = _mutation_inputs()
    R = len(tb["step_vp"])
    want = tr.dense_csr(_csr(traj, V, G)[1], dg, R * V, np.float32)
    good = tr.backward(dg, tb, V, np.float32)[0]
    bad, _, _, terms = tr.backward(dg, tb, V, np.float32, mutate="descending_nodes")
    assert (terms == 2).any()
    assert np.array_equal(_bits(good), _bits(want))
    assert not np.array_equal(_bits(bad), _bits(want))
    assert np.abs(bad.astype(np.float64) - want).max() <= 2.0 ** -22 * np.abs(want).max()      # ... and nothing but last bits


def test_status_words_of_the_restatement():
    """each device flag planted once: the flagged rows / steps keep the fill and carry the flag, every other row is unchanged"""
    V, G = 5, 9
    traj = tr.crafted(V)
    base = tr.tables(traj, G)
    rng = np.random.RandomState(6)
    R, B = len(base["step_vp"]), len(traj["traj_vpids"])
    pano, dg = tr.scaled_rows(rng, R * V, 4), tr.scaled_rows(rng, B * G, 4)
    good_f, good_b = tr.forward(pano, base, V, np.float32)[0], tr.backward(dg, base, V, np.float32)[0]
    fill_f, fill_b = np.full((B * G, 4), 7.0, np.float32), np.full((R * V, 4), 7.0, np.float32)
    plants = {"steps": ("step_off", 4, R + 1, tr.ERR_STEPS, 3), "count": ("cand_count", 1, 6, tr.ERR_COUNT, 0),
              "views": ("view_lens", 4, V + 1, tr.ERR_VIEWS, 1), "len": ("gmap_len", 3, G + 1, tr.ERR_LEN, 3)}
    for name, (key, at, value, flag, sample) in plants.items():
        tb = {k: v.copy() for k, v in base.items()}
        tb[key][at] = value
        out, st, _, _ = tr.forward(pano, tb, V, np.float32, fill=fill_f)
        dp, stb, _, _ = tr.backward(dg, tb, V, np.float32, fill=fill_b)
        rows = np.zeros(B * G, bool)
        rows[sample * G:(sample + 1) * G] = True
        steps = np.zeros(R, bool)
        steps[base["step_off"][sample]:base["step_off"][sample + 1]] = True
        assert (st[rows] == flag).all() and not st[~rows].any(), name
        assert (stb[steps] == flag).all() and not stb[~steps].any(), name
        assert (out[rows] == 7.0).all() and np.array_equal(out[~rows], good_f[~rows]), name
        srows = np.repeat(steps, V)
        assert (dp[srows] == 7.0).all() and np.array_equal(dp[~srows], good_b[~srows]), name
    tb = {k: v.copy() for k, v in base.items()}
    tb["gmap_id"][0, 5] = 999                                   # a listed node that nothing visits or names
    out, st, _, _ = tr.forward(pano, tb, V, np.float32, fill=fill_f)
    assert st[5] == tr.ERR_NODE and st.sum() == tr.ERR_NODE and (out[5] == 7.0).all()
    assert np.array_equal(np.delete(out, 5, 0), np.delete(good_f, 5, 0))
