"""The device-resident map on the MI355X: etp_gmap_update / etp_gmap_embed_csr (csrc/gmap_update.hip) and graph_inputs.DeviceGraphMaps
against the fp64 restatement tests/gmap_update_ref.py (pinned by tests/test_gmap_update_ref_cpu.py).  Every random rollout here is
built by gmap_update_ref.rollout(name) from the table gmap_update_ref.ROLLOUTS; the CPU test asserts, for every entry of that table,
that no candidate sits where a last-bit difference could change a discrete outcome.

Record, counts, node_step, front_ptr / front_idx, cur_node and both CSRs' ptr / idx are exact.  node_pos, adj, ghost_pos and the CSR
weights are BIT-EQUAL after the fp32 cast: the kernel's arithmetic is the restatement's correctly rounded double operations in the
same order (contraction off).  Every output is pre-filled with a sentinel (NaN bits / -777) and carries a guard row behind its B
episodes; the guards must come back intact.  Every case is a handful of launches on a few episodes (milliseconds)."""
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from etpnav_amd import _lib, decide, graph_inputs  # noqa: E402
from etpnav_amd._lib import check, ptr  # noqa: E402
from etpnav_amd.graph_inputs import DeviceGraphMaps, GraphMapLite  # noqa: E402
from tests import decide_ref as dr  # noqa: E402
from tests import gmap_update_ref as gr  # noqa: E402

DEV = "cuda"
SENT = -777
HERE = os.path.dirname(os.path.abspath(__file__))
FIXTURE = os.path.join(HERE, "golden", "gmap_update_small.npz")
DECIDE_FIXTURE = os.path.join(HERE, "golden", "decide_small.npz")
OUT_SHAPES = {"node_pos": (gr.GN, 3), "node_step": (gr.GN,), "n_nodes": (), "adj": (gr.GN, gr.GN), "ghost_pos": (gr.GM, 3), "n_ghost": (),
              "front_ptr": (gr.GM + 1,), "front_idx": (gr.FMAX,), "cur_node": (), "cur_pos": (3,), "cur_heading": (), "record": (gr.HDR + gr.KMAX,)}
FLOAT_OUT = ("node_pos", "adj", "ghost_pos", "cur_pos", "cur_heading")


def stream():
    return torch.cuda.current_stream().cuda_stream


class Dev:
    """S slot records on the device, driven through the C ABI directly"""

    def __init__(self, S, loc_noise, merge, aug):
        self.S, self.loc_noise, self.merge, self.aug = S, loc_noise, merge, aug
        self.nbytes = int(_lib.lib().etp_gmap_slot_bytes())
        self.state = torch.full((S * self.nbytes,), 0x5A, dtype=torch.uint8, device=DEV)      # garbage until reset
        self.reset(list(range(S)))

    def reset(self, slots):
        t = torch.tensor(slots, dtype=torch.int32, device=DEV)
        check(_lib.lib().etp_gmap_reset(ptr(self.state), self.S, ptr(t), len(slots), stream()), "etp_gmap_reset")

    def image(self):
        return self.state.cpu().numpy().reshape(self.S, self.nbytes).copy()

    def update(self, slot, prev_node, step_id, cur_pos, cur_heading, cand_pos, n_cand, cur_row, cand_row, del_ghost, noise=None, Kmax=gr.KMAX):
        B = len(slot)
        up = lambda x, dt: torch.from_numpy(np.ascontiguousarray(x, dtype=dt)).to(DEV)
        i = [up(x, np.int32) for x in (slot, prev_node, step_id, n_cand, cur_row, cand_row, del_ghost)]
        cp, cq, hd = up(cur_pos, np.float64), up(cand_pos, np.float64), up(cur_heading, np.float32)
        nz = None if noise is None else up(noise, np.float64)
        out = {}
        for k, shp in OUT_SHAPES.items():                     # B episodes + one guard row, all pre-filled
            if k in FLOAT_OUT:
                out[k] = torch.full((B + 1,) + shp, float("nan"), dtype=torch.float32, device=DEV)
            else:
                out[k] = torch.full((B + 1,) + shp, SENT, dtype=torch.int32, device=DEV)
        if Kmax != gr.KMAX:
            out["record"] = torch.full((B + 1, gr.HDR + Kmax), SENT, dtype=torch.int32, device=DEV)
        check(_lib.lib().etp_gmap_update(ptr(self.state), self.S, ptr(i[0]), ptr(i[1]), ptr(i[2]), ptr(cp), ptr(hd), ptr(cq), ptr(i[3]), ptr(i[4]),
                                         ptr(i[5]), ptr(i[6]), ptr(nz), self.loc_noise, int(self.merge), self.aug, B, Kmax,
                                         *[ptr(out[k]) for k in OUT_SHAPES], stream()), "etp_gmap_update")
        res = {k: v.cpu().numpy() for k, v in out.items()}
        for k, v in res.items():                              # the guard row behind the episodes
            g = v[B:]
            assert np.isnan(g).all() if k in FLOAT_OUT else (g == SENT).all(), f"guard of {k} overwritten"
        return {k: v[:B] for k, v in res.items()}

    def embed_csr(self, slot, G, R, nnz):
        B = len(slot)
        sl = torch.tensor(slot, dtype=torch.int32, device=DEV)
        i32 = lambda n: torch.full((n + 4,), SENT, dtype=torch.int32, device=DEV)
        f32 = lambda n: torch.full((n + 4,), float("nan"), dtype=torch.float32, device=DEV)
        t = [i32(B * G + 1), i32(nnz), f32(nnz), i32(R + 1), i32(R), f32(R), i32(B)]
        check(_lib.lib().etp_gmap_embed_csr(ptr(self.state), self.S, ptr(sl), B, G, R, *[ptr(x) for x in t], stream()), "etp_gmap_embed_csr")
        h = [x.cpu().numpy() for x in t]
        for x, n in zip(h, (B * G + 1, nnz, nnz, R + 1, R, R, B)):
            assert (np.isnan(x[n:]).all() if x.dtype == np.float32 else (x[n:] == SENT).all()), "guard behind a CSR array overwritten"
        return h


def bits(a):
    return np.ascontiguousarray(a).view(np.int32) if a.dtype == np.float32 else a


def assert_same(got, want, name):
    for k in OUT_SHAPES:
        assert got[k].dtype == want[k].dtype and got[k].shape == want[k].shape, (name, k)
        if not np.array_equal(bits(got[k]), bits(want[k])):
            bad = np.argwhere(bits(got[k]) != bits(want[k]))
            raise AssertionError(f"{name}: {k} differs at {bad[:4].tolist()}: got {got[k][tuple(bad[0])]!r}, want {want[k][tuple(bad[0])]!r}")


def assert_csr(dev, ref, slot, G, R, name):
    (pf, xf, wf), (pb, xb, wb), st = ref.embed_csr(slot, G, R)
    h = dev.embed_csr(slot, G, R, max(len(xf), 1))
    B = len(slot)
    assert np.array_equal(h[6][:B], st), (name, h[6][:B], st)
    assert np.array_equal(h[0][:B * G + 1], pf) and np.array_equal(h[1][:len(xf)], xf), f"{name}: forward CSR"
    assert np.array_equal(bits(h[2][:len(wf)]), bits(wf)), f"{name}: forward weights"
    assert np.array_equal(h[3][:R + 1], pb) and np.array_equal(h[4][:len(xb)], xb), f"{name}: transposed CSR"
    assert np.array_equal(bits(h[5][:len(wb)]), bits(wb)), f"{name}: transposed weights"


# ---- operator level ---------------------------------------------------------------------------------------------------------------------
GRID = [n for n in gr.ROLLOUTS if n.startswith("B")]           # B in {1, 3, 8} x K in {0, 1, 5, 16}, six steps each, and B = 8 with 0 .. 6


@pytest.mark.parametrize("aug", [0.0, 0.3])
@pytest.mark.parametrize("merge", [True, False])
@pytest.mark.parametrize("name", GRID)
def test_rollouts_against_the_restatement(name, merge, aug):
    calls, R, B, S = gr.rollout(name)
    dev, ref = Dev(S, 0.5, merge, aug), gr.RefBatch(S, 0.5, merge, aug)
    for t, c in enumerate(calls):
        want, got = ref.update(**c), dev.update(**c)
        assert (want["record"][:, 2] == 0).all()
        assert_same(got, want, f"step {t}")
        if t in (0, len(calls) - 1):
            G = int((1 + want["n_nodes"] + want["n_ghost"]).max()) + (t % 2)
            assert_csr(dev, ref, c["slot"].tolist(), G, R + 3, f"step {t}")


def test_merges_shift_a_tail_of_more_than_256_entries_up_to_the_absorbed_capacity():
    dev, ref = Dev(1, 5.0, True, 0.0), gr.RefBatch(1, 5.0, True, 0.0)
    calls = gr.merge_heavy_calls()
    for t, c in enumerate(calls):
        want, got = ref.update(**c), dev.update(**c)
        assert_same(got, want, f"merge-heavy call {t}")
    assert got["record"][0, :6].tolist() == [32, 2, 0, 31, 2, gr.FMAX] and got["front_ptr"][0, :3].tolist() == [0, 121, 512]
    assert_csr(dev, ref, [0], 40, 17 * 32 + 5, "512 absorbed")
    before = dev.image()
    more = dict(calls[0], prev_node=np.array([31], np.int32), n_cand=np.array([1], np.int32))      # absorbed + 1 > ETP_GMAP_FMAX
    want, got = ref.update(**more), dev.update(**more)
    assert want["record"][0, 2] == gr.ERR_CAPACITY
    assert_same(got, want, "513th absorbed candidate")
    assert np.array_equal(dev.image(), before), "a refused update wrote the state"
    none = dict(more, n_cand=np.array([0], np.int32))
    assert_same(dev.update(**none), ref.update(**none), "no candidate: room for the node")


def test_embed_csr_flags_an_unreset_record_without_indexing_it():
    dev = Dev(2, 0.5, True, 0.0)
    c = one_call(0, -1, 1, [0, 0, 0], [[2.0, 0, 0]])
    dev.update(**c)
    hdr = torch.tensor([-3, 150, 0], dtype=torch.int32).view(torch.uint8).to(DEV)                  # slot 1: n = -3, m = 150, as garbage would be
    dev.state[2 * dev.nbytes - 12:] = hdr
    h = dev.embed_csr([0, 1], 8, 10, 2)
    assert h[6][:2].tolist() == [0, gr.ERR_INPUT] and h[0][:17].tolist() == [0, 0, 1] + [2] * 14 and h[1][:2].tolist() == [0, 1]


def test_lattice_cases_are_exact():
    dev, ref = Dev(1, 5.0, True, 0.0), gr.RefBatch(1, 5.0, True, 0.0)
    for t, (c, codes) in enumerate(zip(gr.lattice_calls(), gr.LATTICE_CODES)):
        want, got = ref.update(**c), dev.update(**c)
        assert want["record"][0, gr.HDR:gr.HDR + len(codes)].tolist() == codes
        assert_same(got, want, f"lattice call {t}")
    assert got["front_idx"][0, :4].tolist() == [1, 1, 1, 2] and got["ghost_pos"][0, 0].tolist() == [43.5, 0.0, 0.0]
    assert got["adj"][0, 0, 0] == 0.0 and got["adj"][0, 0, 1] == 8.0 and got["adj"][0, 2, 3] == 3.0 and got["adj"][0, 0, 2] == -1.0


def test_fixture_replayed_through_the_host_mirror():
    for r, run in enumerate(gr.load_fixture(FIXTURE)):
        ref = gr.RefBatch(3, run["loc_noise"], run["merge_ghost"], 0.0)
        for has_real in sorted(set(run["has_real_pos"])):     # has_real_pos is one flag per DeviceGraphMaps: replay once per value
            maps = DeviceGraphMaps(3, DEV, has_real, run["loc_noise"], run["merge_ghost"], 0.0)
            for t, step in enumerate(run["steps"]):
                c = gr.call_from_fixture(step)
                if has_real == sorted(set(run["has_real_pos"]))[0]:
                    want = ref.update(**c)
                for b, v in enumerate(maps.gmaps):
                    if step["del_ghost"][b] >= 0:
                        v.delete_ghost(list(v.ghost_pos)[step["del_ghost"][b]])
                cur_vp = [str(len(v.node_pos)) for v in maps.gmaps]
                rec = maps.update([None if p < 0 else str(p) for p in step["prev_node"]], step["step_id"], cur_vp, step["cur_pos"], step["cur_heading"],
                                  step["cand_pos"], step["cur_row"], step["cand_row"], step["cand_real_pos"])
                if has_real == sorted(set(run["has_real_pos"]))[0]:
                    assert np.array_equal(rec, want["record"])
                    got = {k: v.cpu().numpy() for k, v in maps.compact().items() if k != "_dims"}
                    assert_same(dict(got, record=rec), want, f"run {r} step {t}")
                for b, v in enumerate(maps.gmaps):
                    a = step["after"][b]
                    assert list(v.node_pos) == a["nodes"] and list(v.ghost_pos) == a["ghosts"] and v.ghost_cnt == a["ghost_cnt"]
                    assert [p.tolist() for p in v.node_pos.values()] == a["node_pos"] and list(v.node_stepId.values()) == a["node_step"]
                    assert [[p.tolist() for p in ps] for ps in v.ghost_pos.values()] == a["ghost_pos"]
                    assert [p.tolist() for p in v.ghost_mean_pos.values()] == a["ghost_mean"] == [p.tolist() for p in v.ghost_aug_pos.values()]
                    assert list(v.ghost_fronts.values()) == a["ghost_fronts"]
                    if has_real and run["has_real_pos"][b]:
                        assert list(v.ghost_real_pos.values()) == a["ghost_real_pos"]


def test_slots_pauses_untouched_records_and_determinism():
    S = 6
    calls, R, _, _ = gr.rollout("slots")                     # a permutation prefix of 6 slots: non-contiguous, out of order
    dev, ref = Dev(S, 0.5, True, 0.3), gr.RefBatch(S, 0.5, True, 0.3)
    keep = [0, 1, 2, 3]
    for t, c in enumerate(calls):
        if t == 2:
            keep = [3, 1]                                     # two environments paused, the rest permuted
        c = {k: (v[keep] if isinstance(v, np.ndarray) and v.shape[:1] == (4,) else v) for k, v in c.items()}
        before = dev.image()
        snapshot = dev.state.clone()
        want, got = ref.update(**c), dev.update(**c)
        assert_same(got, want, f"step {t}")
        after = dev.image()
        named = set(c["slot"].tolist())
        for s in range(S):
            assert (s in named) != np.array_equal(before[s], after[s]), f"step {t}: slot {s} {'unchanged' if s in named else 'written'}"
        dev.state.copy_(snapshot)                             # a second run from a copy of the same state: the same bits everywhere
        again = dev.update(**c)
        assert_same(again, got, f"step {t} rerun")
        assert np.array_equal(dev.image(), after)
    assert_csr(dev, ref, c["slot"].tolist(), 40, R, "paused")  # rows of paused episodes have no owner
    dev.reset([int(c["slot"][0])])
    img = dev.image()
    assert not np.array_equal(img[int(c["slot"][0])], after[int(c["slot"][0])]) and np.array_equal(img[int(c["slot"][1])], after[int(c["slot"][1])])


def one_call(slot, prev, step, pos, cands, del_ghost=-1, row0=0):
    K = len(cands)
    cand = np.zeros((1, gr.KMAX, 3)); cand[0, :K] = np.asarray(cands, dtype=np.float64).reshape(K, 3)
    rows = np.full((1, gr.KMAX), -1, np.int32); rows[0, :K] = row0 + 1 + np.arange(K)
    i32 = lambda x: np.array([x], np.int32)
    return dict(slot=i32(slot), prev_node=i32(prev), step_id=i32(step), cur_pos=np.asarray([pos], dtype=np.float64), cur_heading=np.zeros(1, np.float32),
                cand_pos=cand, n_cand=i32(K), cur_row=i32(row0), cand_row=rows, del_ghost=i32(del_ghost), noise=None)


def test_capacity_and_malformed_input_are_flagged_with_the_slot_unchanged():
    dev, ref = Dev(2, 0.5, True, 0.0), gr.RefBatch(2, 0.5, True, 0.0)
    for i in range(64):                                       # slot 1: a chain of 64 nodes; the 64th succeeds
        c = one_call(1, i - 1, i + 1, [3.0 * i, 0, 0], [], row0=210 + i)
        want, got = ref.update(**c), dev.update(**c)
    assert_same(got, want, "64th node")
    assert got["record"][0, :4].tolist() == [64, 0, 0, 63] and got["adj"][0, 62, 63] == 3.0
    for t in range(12):                                       # slot 0: 12 x 16 far-apart candidates = 192 ghosts
        c = one_call(0, t - 1, t + 1, [0, 0, 100.0 * t], [[10.0 * (k + 1), 0, 100.0 * t] for k in range(16)], row0=17 * t)
        want, got = ref.update(**c), dev.update(**c)
        assert_same(got, want, f"ghost call {t}")
    assert got["record"][0, :6].tolist() == [12, 192, 0, 11, 192, 192]
    assert_csr(dev, ref, [0, 1], 257, 280, "full")
    before = dev.image()
    flagged = [(one_call(1, 63, 65, [500.0, 0, 0], []), gr.ERR_CAPACITY),                              # the 65th node
               (one_call(0, 11, 13, [0, 0, 5000.0], [[7.0, 0, 5000.0]]), gr.ERR_CAPACITY),             # the 193rd ghost
               (one_call(0, 12, 13, [0, 0, 5000.0], []), gr.ERR_INPUT), (one_call(0, -2, 13, [0, 0, 5000.0], []), gr.ERR_INPUT),
               (one_call(0, 11, 13, [0, 0, 5000.0], [], del_ghost=192), gr.ERR_INPUT), (one_call(0, 11, 13, [0, 0, 5000.0], [], del_ghost=-5), gr.ERR_INPUT),
               (dict(one_call(0, 11, 13, [0, 0, 5000.0], []), n_cand=np.array([17], np.int32)), gr.ERR_INPUT),
               (dict(one_call(0, 11, 13, [0, 0, 5000.0], []), n_cand=np.array([-1], np.int32)), gr.ERR_INPUT),
               (one_call(2, -1, 1, [0, 0, 0], []), gr.ERR_INPUT), (one_call(-1, -1, 1, [0, 0, 0], []), gr.ERR_INPUT)]
    for c, flag in flagged:
        want, got = ref.update(**c), dev.update(**c)
        assert want["record"][0, 2] == flag
        assert_same(got, want, f"flag {flag}")
        assert np.array_equal(dev.image(), before), "a refused update wrote the state"
    c = one_call(0, 11, 13, [0, 0, 5000.0], [[7.0, 0, 5000.0]], del_ghost=5, row0=300)               # with the deletion there is room again
    assert_same(dev.update(**c), ref.update(**c), "delete then add")
    # a smaller record stride
    d2, r2 = Dev(1, 0.5, True, 0.0), gr.RefBatch(1, 0.5, True, 0.0)
    c = one_call(0, -1, 1, [0, 0, 0], [[1, 0, 0], [1.2, 0, 0], [0.2, 0, 0]])
    c5 = dict(c, cand_pos=c["cand_pos"][:, :5].copy(), cand_row=c["cand_row"][:, :5].copy(), Kmax=5)
    want, got = r2.update(**c5), d2.update(**c5)
    assert got["record"].shape == (1, 13) and np.array_equal(got["record"], want["record"])
    assert [x >> 24 for x in got["record"][0, 8:11]] == [gr.NEW, gr.MERGED, gr.EDGE]


# ---- integration: the consumers see what they saw from pack_batch ---------------------------------------------------------------------
def test_assemble_decide_and_img_fts_equal_the_host_route_bit_for_bit():
    B, steps, H = 3, 5, 256
    calls, R, _, _ = gr.rollout("integration")
    maps = DeviceGraphMaps(B, DEV, False, 0.5, True, 0.0)
    lites = [GraphMapLite(False, 0.5, True, 0) for _ in range(B)]
    gen = torch.Generator().manual_seed(5)
    store = torch.randn(R, H, generator=gen).to(DEV).requires_grad_(True)
    tab_a = torch.full((B, 64), float("-inf"), device=DEV)
    tab_b = tab_a.clone()
    for t, c in enumerate(calls):
        ks = c["n_cand"].tolist()
        cur_vp = [str(t)] * B
        for b in range(B):
            if c["del_ghost"][b] >= 0:
                gvp = list(lites[b].ghost_pos)[c["del_ghost"][b]]
                lites[b].delete_ghost(gvp); maps.gmaps[b].delete_ghost(gvp)
            lites[b].update_graph(None if c["prev_node"][b] < 0 else str(c["prev_node"][b]), t + 1, cur_vp[b], c["cur_pos"][b], int(c["cur_row"][b]),
                                  [f"{t}_{k}" for k in range(ks[b])], [c["cand_pos"][b, k] for k in range(ks[b])],
                                  [int(x) for x in c["cand_row"][b, :ks[b]]], None)
        maps.update([None if p < 0 else str(p) for p in c["prev_node"]], t + 1, cur_vp, c["cur_pos"], c["cur_heading"],
                    [c["cand_pos"][b, :ks[b]] for b in range(B)], c["cur_row"].tolist(), [c["cand_row"][b, :ks[b]].tolist() for b in range(B)])
        for b in range(B):
            assert list(maps.gmaps[b].ghost_pos) == list(lites[b].ghost_pos) and maps.gmaps[b].ghost_fronts == lites[b].ghost_fronts
        want = graph_inputs.nav_gmap_variable(lites, cur_vp, c["cur_pos"], c["cur_heading"].tolist(), DEV, keep_compact=True)
        got = maps.nav_inputs()
        assert got["gmap_vp_ids"] == want["gmap_vp_ids"] and got["no_vp_left"] == want["no_vp_left"]
        for k in ("gmap_step_ids", "gmap_masks", "gmap_visited_masks", "gmap_pos_fts", "gmap_pair_dists"):
            assert got[k].dtype == want[k].dtype and torch.equal(got[k], want[k]), f"step {t}: {k}"
        G = got["gmap_masks"].shape[1]
        logits = torch.randn(B, G, generator=gen).to(DEV).masked_fill(~got["gmap_masks"], float("-inf"))
        slot = torch.arange(B, dtype=torch.int32, device=DEV)
        ra = decide.nav_decide(logits, want["compact"], slot, tab_a)
        rb = decide.nav_decide(logits, got["compact"], slot, tab_b)
        assert torch.equal(ra[:, :decide.HDR], rb[:, :decide.HDR]) and torch.equal(tab_a, tab_b), f"step {t}: decision"
        n = want["compact"]["_dims"][1]
        assert torch.equal(ra[:, decide.HDR:decide.HDR + n], rb[:, decide.HDR:decide.HDR + n]) and bool((rb[:, decide.HDR + n:] == -1).all())
        if t in (1, steps - 1):
            fa = graph_inputs.gather_rows(store, lites, [0] * B, G)
            fb = maps.img_fts(store, G)
            assert fb.shape == fa.shape == (B, G, H) and torch.equal(fa, fb), f"step {t}: gmap_img_fts"
            w = torch.randn(B, G, H, generator=gen).to(DEV)
            ga, = torch.autograd.grad((fa * w).sum(), store)
            gb, = torch.autograd.grad((fb * w).sum(), store)
            assert torch.equal(ga, gb) and bool(ga.abs().sum() > 0), f"step {t}: gradient with respect to the store"
    with pytest.raises(ValueError):
        maps.nav_inputs(G=2)
    with pytest.raises(ValueError):
        maps.img_fts(store, 2)
    with pytest.raises(ValueError, match="rows"):             # a store too short for the rows the maps hold
        maps.img_fts(store[:R - 1], 64)
    # what the kernel would flag is refused before the launch: records and views stay as they were
    image, views = maps.state.clone(), [(list(v.node_pos), list(v.ghost_pos), v.pending_delete) for v in maps.gmaps]
    n = len(maps.gmaps[0].node_pos)
    with pytest.raises(ValueError):
        maps.update([str(n - 1), str(n), None], steps + 1, [str(n)] * B, np.zeros((B, 3)), [0.0] * B, [[]] * B, [R, R + 1, R + 2], [[]] * B)
    assert torch.equal(maps.state, image) and views == [(list(v.node_pos), list(v.ghost_pos), v.pending_delete) for v in maps.gmaps]


class LazyMaps:
    """DeviceGraphMaps behind decide_ref.drive, which updates one GraphMap at a time: the per-environment proxies queue their
    update_graph calls and the batch runs in one etp_gmap_update once every active environment has queued its own"""

    def __init__(self, num_envs, cfg):
        self.maps = DeviceGraphMaps(num_envs, DEV, False, cfg["loc_noise"], cfg["merge_ghost"], 0.0)
        self.d = decide.RolloutDecider(num_envs, DEV, cfg["back_algo"], cfg["consume_ghost"], cfg["tryout"], cfg["max_len"])
        self.cfg, self.queue, self.made, self.launches = cfg, {}, 0, 0

    def make(self):
        self.made += 1
        return Proxy(self, self.made - 1)

    def flush(self):
        if len(self.queue) == len(self.maps.active) and self.queue:
            q = [self.queue[s] for s in self.maps.active]
            self.queue = {}
            self.maps.update([x[0] for x in q], [x[1] for x in q], [x[2] for x in q], [x[3] for x in q], [0.0] * len(q), [x[4] for x in q],
                             [0] * len(q), [list(range(len(x[4]))) for x in q])
            self.launches += 1

    def pause(self, i):
        self.d.pause(i); self.maps.pause(i)

    def __call__(self, gmaps, cur_vp, prev_vp, active, logits, teacher, uni, feedback, stepk):
        self.flush()
        assert self.maps.active == active == self.d.active
        nav = self.maps.nav_inputs()
        assert nav["gmap_masks"].shape[1] == logits.shape[1]
        sample = feedback == "sample"
        a_t, env_actions = self.d.decide(torch.from_numpy(logits).to(DEV), self.maps.gmaps, cur_vp, stepk, feedback,
                                         self.cfg["sample_ratio"] if sample else None, torch.from_numpy(teacher).to(DEV) if sample else None,
                                         uniforms=torch.from_numpy(uni).to(DEV) if sample else None, compact=nav.pop("compact"))
        prev_vp[:] = self.d.prev_vp
        return a_t, env_actions


class Proxy:
    def __init__(self, owner, slot):
        self.__dict__.update(owner=owner, slot=slot)

    def update_graph(self, prev_vp, step_id, cur_vp, cur_pos, cur_embeds, cand_vp, cand_pos, cand_embeds, cand_real_pos):
        self.owner.queue[self.slot] = (prev_vp, step_id, cur_vp, np.asarray(cur_pos, dtype=np.float64), [np.asarray(p, dtype=np.float64) for p in cand_pos])

    def __getattr__(self, name):
        self.owner.flush()
        return getattr(self.owner.maps.views[self.slot], name)


def test_rollout_decider_on_the_views_replays_the_decide_fixture():
    log, cfg = dr.load_fixture(DECIDE_FIXTURE)
    lazy = LazyMaps(4, cfg)
    got = dr.drive(lazy.make, dr.ReplayPlan(log), lazy, 4, cfg)
    dr.compare_logs(got, log, "RolloutDecider on DeviceGraphMaps views")
    assert lazy.launches == len(log)
