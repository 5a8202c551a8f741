"""The rollout decision on the MI355X: etp_nav_decide against the fp64 restatement (tests/decide_ref.py) at operator level, and
GraphMapLite + RolloutDecider replaying tests/golden/decide_small.npz (recorded from the reference's own statements on real GraphMap
objects by tools/make_golden_decide.py).

Operator cases (decide_ref.make_case; every episode drawn until decide_ref.check_conditions holds, none left out), each with
feedback 'sample' (uniforms + teacher) and 'argmax', slots a permutation prefix of S = B + 2 rows:
  B=1   n=64 m=192            G = 257: the second trip of the 256-thread loops, every limit at once
  B=3   n=1,2,17 m=0,1,5      G = 23 = 1 + n + m of the largest, and G = 32 with a -inf tail
  B=8   n, m cycling through {1,2,17,64} x {0,1,5,192}, G = 257
  B=33  n=1,2,17 m=0,1,5 cycling, G = 23, force_stop on
Actions, greedy actions, flags, stop nodes, targets, ghosts, path lengths and paths are exact; stop_prob (in the record and in the
table) within decide_ref.stop_prob_bound, no multiplier.  The record (pre-filled with NaN bits) and the table sit between guard rows
of a sentinel; guards, the table's other rows and the other columns of the episodes' own rows must come back bit for bit.  A second
run from the same table state is bit-identical.  Each call is bracketed by _lib.profiled: exactly one launch of nav_decide_kernel.

Crafted rows (exact by construction, compared with episode_ref directly): duplicate maxima in the logits and in the pre-filled
table, u0 = 0 and u0 = 1 - 2^-24, one-hot rows, u1 == sample_ratio and one ulp above it, teacher = ignore_index with no ghost left,
target == cur; the three error flags.

ETP_DECIDE_BOUNDS_OUT=<path> writes the worst ratio there (profiles/decide_op_bounds.txt is such a file).
"""
import functools
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from etpnav_amd import _lib  # noqa: E402
from etpnav_amd import decide, graph_inputs  # noqa: E402
from etpnav_amd.graph_inputs import GraphMapLite, pack_batch  # noqa: E402
from tests import decide_ref as dr  # noqa: E402

DEV = "cuda"
SENTINEL = -777
GUARD = 4
NAN_BITS = 0x7FC00000
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "decide_small.npz")
NS, MS = (1, 2, 17, 64), (0, 1, 5, 192)
OP_CASES = {
    "B1_all_limits": dict(ns=[64], ms=[192]),
    "B3_exact_G": dict(ns=[1, 2, 17], ms=[0, 1, 5]),
    "B3_padded_G": dict(ns=[1, 2, 17], ms=[0, 1, 5], G=32),
    "B8_G257": dict(ns=[NS[i % 4] for i in range(8)], ms=[MS[(i + i // 4) % 4] for i in range(8)], G=257),
    "B33_force_stop": dict(ns=[NS[i % 3] for i in range(33)], ms=[MS[i % 3] for i in range(33)], force_stop=True),
}


@pytest.fixture(scope="module", autouse=True)
def report_worst():
    yield
    lines = ["# tests/test_decide_gpu.py: worst |got - fp64| / bound of stop_prob (bound: tests/decide_ref.py, no multiplier)"]
    lines += [f"{k:28s} {v[0]:.4f}   {v[1]}" for k, v in sorted(dr.WORST.items())]
    print("\n" + "\n".join(lines))
    out = os.environ.get("ETP_DECIDE_BOUNDS_OUT")
    if out:
        with open(out, "w") as f:
            f.write("\n".join(lines) + "\n")


@functools.lru_cache(maxsize=None)
def op_case(name, sample):
    kw = OP_CASES[name]
    return dr.make_case(seed=sum(map(ord, name)) + int(sample), sample=sample, S=len(kw["ns"]) + 2, name=name, **kw)


def upload(batch):
    c = {k: torch.from_numpy(batch[k]).to(DEV) for k in decide.COMPACT_KEYS}
    c["_dims"] = batch["_dims"]
    return c


def run(batch, logits, table, slots, uniforms, teacher, sample_ratio, force_stop):
    """one guarded, profiled launch -> (record [B,R] int64, table after [S,64] fp32 numpy, raw guarded buffers)"""
    B, Nmax = batch["_dims"][0], batch["_dims"][1]
    R, S = decide.HDR + Nmax, table.shape[0]
    rec_buf = torch.full((GUARD + B + GUARD, R), SENTINEL, dtype=torch.int32, device=DEV)
    rec_buf[GUARD:GUARD + B] = NAN_BITS
    tab_buf = torch.full((GUARD + S + GUARD, 64), float(SENTINEL), dtype=torch.float32, device=DEV)
    tab_buf[GUARD:GUARD + S] = torch.from_numpy(table).to(DEV)
    rec, tab = rec_buf[GUARD:GUARD + B], tab_buf[GUARD:GUARD + S]
    c = upload(batch)
    args = (torch.from_numpy(logits).to(DEV), c, torch.from_numpy(np.asarray(slots, dtype=np.int32)).to(DEV), tab,
            None if uniforms is None else torch.from_numpy(uniforms).to(DEV), None if teacher is None else torch.from_numpy(teacher).to(DEV),
            sample_ratio, force_stop)
    torch.cuda.synchronize()
    with _lib.profiled() as p:
        decide.nav_decide(*args, record=rec)
        torch.cuda.synchronize()
    assert p.launches == {"nav_decide_kernel": 1}, p.launches
    assert bool((rec_buf[:GUARD] == SENTINEL).all()) and bool((rec_buf[GUARD + B:] == SENTINEL).all()), "record guard rows"
    assert bool((tab_buf[:GUARD] == SENTINEL).all()) and bool((tab_buf[GUARD + S:] == SENTINEL).all()), "table guard rows"
    return rec.cpu().numpy().astype(np.int64), tab.cpu().numpy(), (rec_buf.cpu().numpy(), tab_buf.cpu().numpy())


def check_against(name, rec, tab, table_before, slots, eps, logits, refs, Nmax):
    want_tab = table_before.copy()
    for b, r in enumerate(refs):
        want = dr.record_row(r, Nmax)
        got = rec[b].copy()
        sp = float(np.array([got[7]], dtype=np.int64).astype(np.int32).view(np.float32)[0])
        got[7] = 0
        assert got.tolist() == want.tolist(), f"{name}[{b}]: record {got.tolist()} against {want.tolist()}"
        E = dr.stop_prob_bound(logits[b])
        dr.record("nav_decide/stop_prob", sp, r["stop_prob"], E, f"{name}[{b}]")
        cell = tab[slots[b], eps[b]["cur_node"]]
        assert np.float32(cell).view(np.int32) == np.float32(sp).view(np.int32), f"{name}[{b}]: the table holds {cell}, the record {sp}"
        want_tab[slots[b], eps[b]["cur_node"]] = cell
    assert (tab.view(np.int32) == want_tab.view(np.int32)).all(), f"{name}: other slots' rows or other columns of the table changed"


@pytest.mark.parametrize("sample", [True, False], ids=["sample", "argmax"])
@pytest.mark.parametrize("name", list(OP_CASES))
def test_operator_against_fp64(name, sample):
    c = op_case(name, sample)
    a = (c["batch"], c["logits"], c["table"], c["slots"], c["uniforms"], c["teacher"], c["sample_ratio"], c["force_stop"])
    rec, tab, raw = run(*a)
    check_against(name, rec, tab, c["table"], c["slots"], c["eps"], c["logits"], c["refs"], c["batch"]["_dims"][1])
    rec2, tab2, raw2 = run(*a)
    assert (raw[0] == raw2[0]).all() and (raw[1].view(np.int32) == raw2[1].view(np.int32)).all(), f"{name}: the second run differs"


def crafted_batch():
    """eight episodes on two fixed graphs (n = 5, m = 3 and n = 5, m = 0), logits / table / uniforms set by hand"""
    rng = np.random.default_rng(77)
    g = dr.random_episode(5, 3, rng, cur=2)
    g["ghost_fronts"][1] = [2, 0]
    g["ghost_pos"][1] = g["node_pos"][2] + [0.3, 0.0, 0.2]                 # ghost 1's nearest front is the current node
    g0 = dict(dr.random_episode(5, 0, rng, cur=4))
    G, ratio = 12, np.float32(0.25)
    rows = []

    def add(ep, l, row, u=None, t=None, force=False, note=""):
        full = np.full(G, -dr.INF, dtype=np.float32)
        full[:len(l)] = l
        tr = np.full(64, -dr.INF, dtype=np.float32)
        tr[:len(row)] = row
        rows.append(dict(ep=ep, l=full, row=tr, u=u, t=t, note=note))

    base = np.array([0.5, -dr.INF, -dr.INF, -dr.INF, -dr.INF, -dr.INF, 1.0, 0.25, -1.0], dtype=np.float32)
    dup = base.copy(); dup[6] = dup[8] = 2.0                                # exactly equal maxima at ghosts 0 and 2
    add(g, dup, [0.5, 0.75, 0.0, 0.75, 0.125], u=(0.999, 0.9), t=0, note="duplicate maxima; u0 near 1")
    first = base.copy(); first[0] = -dr.INF                                 # u0 = 0: the first entry with p > 0 is ghost 0
    add(g, first, [0.1, 0.2, 0.3, 0.2, 0.1], u=(0.0, 0.9), t=0, note="u0 = 0")
    add(g, base, [0.1, 0.2, 0.3, 0.2, 0.1], u=(1.0 - 2.0 ** -24, 0.9), t=0, note="u0 = 1 - 2^-24: the last p > 0, not the -inf tail")
    hot0 = np.full(9, -dr.INF, dtype=np.float32); hot0[0] = 3.0
    add(g, hot0, [1.0, 0.5, -dr.INF, 1.0, 0.5], u=(0.7, 0.9), t=7, note="one-hot stop: p0 = 1, ties the table's maxima 0 and 3")
    hotg = np.full(9, -dr.INF, dtype=np.float32); hotg[7] = -2.0
    add(g, hotg, [0.1, 0.2, 0.3, 0.2, 0.1], u=(0.3, 0.9), t=0, note="one-hot ghost 1: p0 = 0, front == cur, empty path")
    add(g, base, [0.1, 0.2, 0.3, 0.2, 0.1], u=(0.05, float(ratio)), t=8, note="u1 == sample_ratio: the teacher's ghost")
    add(g, base, [0.1, 0.2, 0.3, 0.2, 0.1], u=(0.05, float(np.nextafter(ratio, np.float32(1)))), t=8, note="u1 one ulp above: the sample (0)")
    add(g0, np.array([0.0] + [-dr.INF] * 5, dtype=np.float32), [0.1, 0.2, 0.3, 0.2, -dr.INF], u=(0.5, 0.0), t=dr.IGNORE,
        note="ignore_index, no ghost left; stop node == cur")
    return rows, float(ratio)


def test_crafted_rows():
    rows, ratio = crafted_batch()
    B = len(rows)
    eps = [r["ep"] for r in rows]
    batch = pack_batch(eps)
    logits = np.stack([r["l"] for r in rows])
    slots = np.array([7, 2, 5, 0, 3, 6, 1, 4], dtype=np.int32)
    table = np.full((9, 64), -dr.INF, dtype=np.float32)
    table[8, :5] = 0.99                                                     # a row no episode owns
    uni = np.array([r["u"] for r in rows], dtype=np.float32)
    teacher = np.array([r["t"] for r in rows], dtype=np.int64)
    for b, r in enumerate(rows):
        table[slots[b]] = r["row"]
    refs = [dr.episode_ref(r["ep"], r["l"], r["row"], uni[b], int(teacher[b]), ratio, False) for b, r in enumerate(rows)]
    # what the rows were crafted for, on the restatement
    assert (refs[0]["greedy"], refs[0]["action"]) == (6, 8) and refs[1]["action"] == 6 and refs[2]["action"] == 8
    assert refs[3]["stop_prob"] == 1.0 and refs[3]["stop_node"] == 0 and refs[3]["flags"] == dr.STOP and refs[3]["action"] == 0
    assert refs[4]["stop_prob"] == 0.0 and refs[4]["action"] == 7 and refs[4]["target"] == 2 and refs[4]["path"] == []
    assert refs[5]["action"] == 8 and refs[6]["action"] == 0
    assert refs[7]["action"] == dr.IGNORE and refs[7]["flags"] == dr.STOP and refs[7]["stop_node"] == 4 and refs[7]["path"] == []
    rec, tab, _ = run(batch, logits, table, slots, uni, teacher, ratio, False)
    check_against("crafted", rec, tab, table, slots, eps, logits, refs, batch["_dims"][1])
    # argmax feedback with the forced stop on the same rows: the lowest of equal maxima, in the logits and in the table
    refs = [dr.episode_ref(r["ep"], r["l"], r["row"], None, None, 0.0, True) for r in rows]
    assert refs[0]["greedy"] == 6 and refs[0]["stop_node"] == 1 and all(r["flags"] == dr.STOP for r in refs)
    rec, tab, _ = run(batch, logits, table, slots, None, None, 0.0, True)
    check_against("crafted argmax + force_stop", rec, tab, table, slots, eps, logits, refs, batch["_dims"][1])


def test_error_flags_leave_the_rest_alone():
    rng = np.random.default_rng(9)
    ok = dr.random_episode(4, 2, rng, cur=1)
    cut = dr.random_episode(4, 2, rng, cur=0)
    cut["adj"][:] = -1.0
    cut["adj"][0, 1] = cut["adj"][1, 0] = 1.5                              # nodes 2 and 3 cannot be reached from 0
    cut["ghost_fronts"] = [[3], [2]]
    eps = [ok, ok, cut, ok]
    batch = pack_batch(eps)
    batch["n_nodes"] = batch["n_nodes"].copy()
    batch["n_nodes"][3] = 0                                                 # malformed episode
    G = 7
    logits = np.tile(np.array([0.0, -dr.INF, -dr.INF, -dr.INF, -dr.INF, 1.0, 2.0], dtype=np.float32), (4, 1))
    uni = np.tile(np.array([0.5, 0.0], dtype=np.float32), (4, 1))
    teacher = np.array([6, 2, 5, 0], dtype=np.int64)                        # a ghost; a visited node; a ghost behind the cut; -
    slots = np.array([0, 1, 2, 3], dtype=np.int32)
    table = np.full((4, 64), -dr.INF, dtype=np.float32)
    rec, tab, _ = run(batch, logits, table, slots, uni, teacher, 0.25, False)
    assert rec[:, 2].tolist() == [0, dr.ERR_ACTION, dr.ERR_UNREACHABLE, dr.ERR_INPUT], rec[:, 2].tolist()
    assert rec[1, 0] == 2 and rec[1, 4:7].tolist() == [-1, -1, 0] and rec[2, 4:7].tolist() == [3, 0, 0]
    assert rec[3].tolist() == [-1, -1, dr.ERR_INPUT, -1, -1, -1, 0, 0] + [-1] * 4
    assert np.isneginf(tab[3]).all() and np.isfinite(tab[0, 1])              # the malformed episode's row is untouched
    for b in (1, 2, 3):
        with pytest.raises(ValueError):
            decide.raise_on_flags(rec[b:b + 1])
    decide.raise_on_flags(rec[:1])


# ---- host level: GraphMapLite + RolloutDecider replay the recorded rollout -----------------------------------------------------------
class DeviceStep:
    """decide_step of decide_ref.drive around RolloutDecider; even steps pass the compact tensors nav_gmap_variable kept, odd
    steps let the decider upload its own"""

    def __init__(self, num_envs, cfg, counter=None):
        self.d = decide.RolloutDecider(num_envs, DEV, cfg["back_algo"], cfg["consume_ghost"], cfg["tryout"], cfg["max_len"])
        self.cfg, self.counter = cfg, counter

    def pause(self, i):
        self.d.pause(i)

    def __call__(self, gmaps, cur_vp, prev_vp, active, logits, teacher, uni, feedback, stepk):
        assert self.d.active == active and self.d.prev_vp == prev_vp
        compact = None
        if stepk % 2 == 0:
            cur_pos = [g.node_pos[cur_vp[i]] for i, g in enumerate(gmaps)]
            nav = graph_inputs.nav_gmap_variable(gmaps, cur_vp, cur_pos, [0.0] * len(gmaps), DEV, keep_compact=True)
            compact = nav.pop("compact")
            assert nav["gmap_masks"].shape[1] == logits.shape[1]
        nav_logits = torch.from_numpy(logits).to(DEV)
        sample = feedback == "sample"
        if self.counter is not None:
            torch.cuda.synchronize()
            del self.counter[:]
        a_t, env_actions = self.d.decide(nav_logits, gmaps, cur_vp, stepk, feedback, self.cfg["sample_ratio"] if sample else None,
                                         torch.from_numpy(teacher).to(DEV) if sample else None,
                                         uniforms=torch.from_numpy(uni).to(DEV) if sample else None, compact=compact)
        if self.counter is not None:
            assert self.counter == ["cpu"], f"step {stepk}: device-to-host copies {self.counter}"
        prev_vp[:] = self.d.prev_vp
        return a_t, env_actions


def test_rollout_decider_replays_the_fixture_with_one_host_copy_per_step(monkeypatch):
    log, cfg = dr.load_fixture(GOLDEN)
    copies = []
    for fn in ("cpu", "tolist", "item", "numpy", "nonzero"):
        real = getattr(torch.Tensor, fn)

        def counted(self, *a, _real=real, _fn=fn, **k):
            if self.is_cuda:
                copies.append(_fn)
            return _real(self, *a, **k)
        monkeypatch.setattr(torch.Tensor, fn, counted)
    step = DeviceStep(4, cfg, counter=copies)
    got = dr.drive(lambda: GraphMapLite(False, cfg["loc_noise"], cfg["merge_ghost"], 0), dr.ReplayPlan(log), step, 4, cfg)
    dr.compare_logs(got, log, "RolloutDecider")
    # the table holds what the graphs' dicts hold, in the rows of the ORIGINAL environments; paused rows stay behind
    tab = step.d.stop_scores.cpu().numpy()
    for slot, idx in ((0, 0), (3, 1)):
        sc = [x[1] for x in got[-1]["stop_scores"][idx]]
        assert np.allclose(tab[slot, :len(sc)], sc, rtol=0, atol=0) and np.isneginf(tab[slot, len(sc):]).all()
    assert np.isfinite(tab[1, :3]).all() and np.isfinite(tab[2, :2]).all()
    step.d.reset()
    assert bool(torch.isneginf(step.d.stop_scores).all()) and step.d.active == [0, 1, 2, 3]


def test_decider_raises_on_an_action_that_is_no_ghost():
    cfg = dr.CFG
    g = GraphMapLite(False, 0.5, True, 0)
    g.update_graph(None, 1, "0", np.zeros(3), 0.0, ["0_0", "0_1"], [np.array([2.0, 0, 0]), np.array([0.0, 0, 2.0])], [0.0, 0.0], [None, None])
    d = decide.RolloutDecider(1, DEV, cfg["back_algo"], True, True, 6)
    logits = torch.tensor([[0.0, 5.0, -1.0, -2.0]], device=DEV)              # the arg-max is the visited node
    with pytest.raises(ValueError):
        d.decide(logits, [g], ["0"], 0, "argmax")
    assert list(g.ghost_pos) == ["g0", "g1"] and d.prev_vp == [None]        # nothing was applied
    with pytest.raises(NotImplementedError):
        d.decide(logits, [g], ["0"], 0, "beam")
