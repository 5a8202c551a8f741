"""fp64 restatement of the device-resident map (etp_gmap_update / etp_gmap_embed_csr, include/etpnav_hip.h; GraphMap.update_graph,
vlnce_baselines/models/graph_utils.py:193-254 with _localize :163-175 and delete_ghost :185-191) that the tests of
csrc/gmap_update.hip and graph_inputs.DeviceGraphMaps compare against.

RefSlot is one environment's map: the visited nodes, the edges, the ghosts in order with every absorbed candidate's position, front
and store row.  RefBatch drives S of them the way the kernel's arguments do and returns, per call, the compact arrays with the
kernel's fixed strides (64 / 192 / FMAX), the record, and on request both CSRs over the embedding store.

Arithmetic: every step is one IEEE double operation in the order numpy uses on the reference's expressions -- a distance is
sqrt((dx*dx + dy*dy) + dz*dz) (``((q - k) ** 2).sum() ** 0.5`` on three elements, calc_position_distance), a ghost's mean is
(((p0 + p1) + p2) ...) / count (np.mean(list, axis=0)) -- so a kernel built from the same correctly rounded operations returns the
same bits, and the fp32 casts of both sides are equal.

check_conditions asserts, on this restatement alone, what makes the discrete outcome independent of last-bit differences between
numpy's scalar ``**`` and a multiplication / sqrt: every candidate's nearest-key distance lies outside loc_noise * (1 +- 1e-6)
(or is an exact lattice tie) and is separated from the second nearest by more than 1e-9 relative (or is an exact lattice tie).

`mut` plants one of MUTATIONS; the CPU test shows each one is rejected.
"""
import numpy as np

GN, GM, FMAX, HDR, KMAX = 64, 192, 512, 8, 16
ERR_CAPACITY, ERR_INPUT, ERR_ROW = 1, 2, 4
EDGE, NEW, MERGED = 1, 2, 3
MUTATIONS = ("last_min", "lt_not_le", "mean_of_means", "no_front_on_merge", "no_row_on_merge", "ghosts_first", "delete_swaps_last",
             "edge_to_candidate", "skip_new_node")


def code(kind, target):
    return (kind << 24) | int(target)


def dist(a, b):
    dx, dy, dz = np.float64(b[0]) - np.float64(a[0]), np.float64(b[1]) - np.float64(a[1]), np.float64(b[2]) - np.float64(a[2])
    return float(np.sqrt((dx * dx + dy * dy) + dz * dz))


def nearest(q, keys, mut=None):
    """_localize's scan: (index, distance) of the first minimum below 10000 in list order, (None, 10000.) without one"""
    best, bi = 10000.0, None
    for i, k in enumerate(keys):
        d = dist(q, k)
        if d < best or (mut == "last_min" and d == best and bi is not None):
            best, bi = d, i
    return bi, best


class RefSlot:
    def __init__(self):
        self.node_pos, self.node_step, self.node_row = [], [], []
        self.edges = {}                                       # (i, j), i <= j -> length
        self.gid, self.gpos, self.gsum, self.gmean, self.gfront, self.grow = [], [], [], [], [], []
        self.gaug = []
        self.ghost_cnt = 0

    def absorbed(self):
        return sum(len(f) for f in self.gfront)

    def delete(self, g, mut=None):
        lists = (self.gid, self.gpos, self.gsum, self.gmean, self.gfront, self.grow)
        if mut == "delete_swaps_last":
            for l in lists:
                l[g] = l[-1]
                l.pop()
        else:
            for l in lists:
                l.pop(g)

    def update(self, prev, step_id, cur_pos, cands, cur_row, cand_rows, loc_noise, merge, mut=None, margins=None):
        """-> (new node index, [record code per candidate]); margins (a list) collects check_conditions' figures"""
        cur_pos = np.asarray(cur_pos, dtype=np.float64).copy()
        cur = len(self.node_pos)
        if prev >= 0:
            self.edges[(prev, cur)] = dist(self.node_pos[prev], cur_pos)
        self.node_pos.append(cur_pos); self.node_step.append(int(step_id)); self.node_row.append(int(cur_row))
        out = []
        within = (lambda d: d < loc_noise) if mut == "lt_not_le" else (lambda d: d <= loc_noise)
        for q, row in zip(cands, cand_rows):
            q = np.asarray(q, dtype=np.float64).copy()
            nodes = self.node_pos[:-1] if mut == "skip_new_node" else self.node_pos
            ni, nd = nearest(q, nodes, mut)
            gi, gd = nearest(q, self.gmean, mut) if merge else (None, 10000.0)
            if margins is not None:
                margins.append(("node", q, [dist(q, k) for k in nodes]))
            on_node = ni is not None and within(nd)
            on_ghost = gi is not None and within(gd)
            if mut == "ghosts_first" and on_ghost:
                on_node = False
            if on_node:
                w = dist(cur_pos, q) if mut == "edge_to_candidate" else dist(cur_pos, self.node_pos[ni])
                self.edges[(min(cur, ni), max(cur, ni))] = w
                out.append(code(EDGE, ni))
                continue
            if margins is not None and merge:
                margins.append(("ghost", q, [dist(q, k) for k in self.gmean]))
            if on_ghost:
                self.gpos[gi].append(q)
                self.gsum[gi] = self.gsum[gi] + q
                if mut == "mean_of_means":
                    self.gmean[gi] = (self.gmean[gi] + q) / 2.0
                else:
                    self.gmean[gi] = self.gsum[gi] / np.float64(len(self.gpos[gi]))
                if mut != "no_front_on_merge":
                    self.gfront[gi].append(cur)
                if mut != "no_row_on_merge":
                    self.grow[gi].append(int(row))
                if mut in ("no_front_on_merge", "no_row_on_merge"):      # keep the two lists of one length
                    n = min(len(self.gfront[gi]), len(self.grow[gi]))
                    self.gfront[gi], self.grow[gi] = self.gfront[gi][:n], self.grow[gi][:n]
                out.append(code(MERGED, self.gid[gi]))
            else:
                self.gid.append(self.ghost_cnt); self.gpos.append([q]); self.gsum.append(q.copy()); self.gmean.append(q.copy())
                self.gfront.append([cur]); self.grow.append([int(row)])
                out.append(code(NEW, self.ghost_cnt))
                self.ghost_cnt += 1
        return cur, out

    def jitter(self, noise, aug):
        """ghost_aug_pos from standard normals noise [>= m, 3] (or None)"""
        self.gaug = []
        for g, mean in enumerate(self.gmean):
            v = np.array(mean, dtype=np.float64)
            if aug != 0 and noise is not None:
                z = np.asarray(noise[g], dtype=np.float64) * np.array([aug, 0.0, aug])
                v = v + np.clip(z, -aug, aug)
            self.gaug.append(v)


def check_conditions(margins, loc_noise, name=""):
    """module docstring; -> number of candidate scans checked"""
    for kind, q, ds in margins:
        if not ds:
            continue
        d = np.sort(np.asarray(ds))
        lattice = bool((np.asarray(q) == np.round(np.asarray(q))).all())
        assert abs(d[0] - loc_noise) > 1e-6 * loc_noise or (lattice and d[0] == loc_noise), \
            f"{name}: nearest {kind} at {d[0]!r}, within 1e-6 of loc_noise {loc_noise}"
        if len(d) > 1 and d[0] <= 2 * loc_noise:
            assert d[1] - d[0] > 1e-9 * max(d[0], 1e-300) or (lattice and d[1] == d[0]), \
                f"{name}: the two nearest {kind}s are {d[1] - d[0]:.3g} apart at {d[0]:.6g}"
    return len(margins)


class RefBatch:
    """S maps driven through the kernel's arguments"""

    def __init__(self, S, loc_noise, merge_ghost, ghost_aug, mut=None):
        self.S, self.loc_noise, self.merge, self.aug, self.mut = S, float(loc_noise), bool(merge_ghost), float(ghost_aug), mut
        self.slots = [RefSlot() for _ in range(S)]
        self.margins = []

    def reset(self, slots):
        for s in slots:
            if 0 <= s < self.S:
                self.slots[s] = RefSlot()

    def update(self, slot, prev_node, step_id, cur_pos, cur_heading, cand_pos, n_cand, cur_row, cand_row, del_ghost, noise=None, Kmax=KMAX):
        B = len(slot)
        cand_pos = np.asarray(cand_pos, dtype=np.float64).reshape(B, Kmax, 3)
        cand_row = np.asarray(cand_row).reshape(B, Kmax)
        o = {"node_pos": np.zeros((B, GN, 3), np.float32), "node_step": np.zeros((B, GN), np.int32), "n_nodes": np.zeros(B, np.int32),
             "adj": np.full((B, GN, GN), -1.0, np.float32), "ghost_pos": np.zeros((B, GM, 3), np.float32), "n_ghost": np.zeros(B, np.int32),
             "front_ptr": np.zeros((B, GM + 1), np.int32), "front_idx": np.zeros((B, FMAX), np.int32), "cur_node": np.zeros(B, np.int32),
             "cur_pos": np.asarray(cur_pos, dtype=np.float64).reshape(B, 3).astype(np.float32),
             "cur_heading": np.asarray(cur_heading, dtype=np.float32).reshape(B).copy(),
             "record": np.full((B, HDR + Kmax), -1, np.int32)}
        for b in range(B):
            sl, K, prev, dl = int(slot[b]), int(n_cand[b]), int(prev_node[b]), int(del_ghost[b])
            err = 0
            if not (0 <= sl < self.S and 0 <= K <= Kmax):
                err = ERR_INPUT
            else:
                s = self.slots[sl]
                n, m = len(s.node_pos), len(s.gid)
                if not (-1 <= prev < n and -1 <= dl < m):
                    err = ERR_INPUT
                else:
                    gone = len(s.gfront[dl]) if dl >= 0 else 0
                    if n + 1 > GN or m - (dl >= 0) + K > GM or s.absorbed() - gone + K > FMAX:
                        err = ERR_CAPACITY
            if err:
                o["record"][b, :HDR] = [0, 0, err, -1, 0, 0, 0, 0]
                continue
            if dl >= 0:
                s.delete(dl, self.mut)
            cur, codes = s.update(prev, step_id[b], np.asarray(cur_pos, dtype=np.float64).reshape(B, 3)[b], cand_pos[b, :K], cur_row[b],
                                  cand_row[b, :K], self.loc_noise, self.merge, self.mut, self.margins)
            s.jitter(None if noise is None else np.asarray(noise, dtype=np.float64).reshape(B, GM, 3)[b], self.aug)
            n, m = len(s.node_pos), len(s.gid)
            o["n_nodes"][b], o["n_ghost"][b], o["cur_node"][b] = n, m, cur
            o["node_pos"][b, :n] = np.asarray(s.node_pos)
            o["node_step"][b, :n] = s.node_step
            for (i, j), w in s.edges.items():
                o["adj"][b, i, j] = o["adj"][b, j, i] = np.float32(w)
            if m:
                o["ghost_pos"][b, :m] = np.asarray(s.gaug)
            q = 0
            for g, fr in enumerate(s.gfront):
                o["front_idx"][b, q:q + len(fr)] = fr
                q += len(fr)
                o["front_ptr"][b, g + 1] = q
            o["front_ptr"][b, m + 1:] = q
            o["record"][b, :HDR] = [n, m, 0, cur, s.ghost_cnt, q, 0, 0]
            o["record"][b, HDR:HDR + K] = codes
        return o

    def embed_csr(self, slot, G, R):
        """-> (ptr_f, idx_f, w_f), (ptr_b, idx_b, w_b), status: graph_inputs.pack_img_csr from the slots"""
        ptr_f, idx_f, w_f, status = [0], [], [], []
        rev = [[] for _ in range(R)]
        for b, sl in enumerate(slot):
            st = 0
            entries = []
            if not 0 <= sl < self.S:
                st = ERR_INPUT
            else:
                s = self.slots[sl]
                if 1 + len(s.node_pos) + len(s.gid) > G:
                    st = ERR_CAPACITY if s.node_pos else 0
                else:
                    entries = [([r], 1.0) for r in s.node_row] + [(rows, 1.0 / len(rows)) for rows in s.grow]
            for t in range(G):
                if 1 <= t <= len(entries):
                    rows, w = entries[t - 1]
                    for r in rows:
                        if 0 <= r < R:
                            idx_f.append(r); w_f.append(w); rev[r].append((b * G + t, w))
                        else:
                            idx_f.append(0); w_f.append(0.0); st |= ERR_ROW
                ptr_f.append(len(idx_f))
            status.append(st)
        ptr_b, idx_b, w_b = [0], [], []
        for r in rev:
            assert len(r) <= 1, "a store row with two owners"
            for n, w in r:
                idx_b.append(n); w_b.append(w)
            ptr_b.append(len(idx_b))
        i32, f32 = (lambda x: np.asarray(x, dtype=np.int32)), (lambda x: np.asarray(x, dtype=np.float32))
        return (i32(ptr_f), i32(idx_f), f32(w_f)), (i32(ptr_b), i32(idx_b), f32(w_b)), i32(status)


# ---- scripted rollouts the CPU and GPU tests share --------------------------------------------------------------------------------------
def random_calls(B, steps, Kfix, seed, S=None):
    """A list of per-call argument dicts for RefBatch.update / etp_gmap_update: B episodes walk for `steps` calls; every call has
    Kfix candidates (or, Kfix None, 0 .. 6) at 0.6 .. 2.5 from the agent, some of them near an earlier node or an earlier candidate
    so that edges and merges occur; each episode then moves to one of its ghosts (del_ghost of the next call), as the rollout does.
    The driver needs the ghost counts, so it runs a RefBatch(merge on, loc_noise 0.5) of its own to choose the deletions; the calls
    are valid for any configuration with at least as many ghosts (merge off)."""
    rng = np.random.default_rng(seed)
    S = B if S is None else S
    slots = rng.permutation(S)[:B].astype(np.int32)
    shadow = RefBatch(S, 0.5, True, 0.0)
    pos = np.stack([np.array([10.0 * b + rng.uniform(-1, 1), 0.2, rng.uniform(-1, 1)]) for b in range(B)])
    prev = np.full(B, -1, np.int32)
    dele = np.full(B, -1, np.int32)
    seen = [[] for _ in range(B)]
    row = 0
    calls = []
    for t in range(steps):
        K = np.full(B, Kfix, np.int32) if Kfix is not None else rng.integers(0, 7, B).astype(np.int32)
        cand = np.zeros((B, KMAX, 3))
        cand_row = np.full((B, KMAX), -1, np.int32)
        cur_row = np.zeros(B, np.int32)
        for b in range(B):
            cur_row[b] = row; row += 1
            for k in range(int(K[b])):
                u = rng.random()
                if seen[b] and u < 0.3:
                    base = seen[b][int(rng.integers(len(seen[b])))]
                    cand[b, k] = base + rng.uniform(-0.2, 0.2, 3) * [1, 0, 1]
                else:
                    a, d = rng.uniform(0, 2 * np.pi), rng.uniform(0.6, 2.5)
                    cand[b, k] = pos[b] + [d * np.sin(a), 0.0, d * np.cos(a)]
                seen[b].append(cand[b, k].copy())
                cand_row[b, k] = row; row += 1
            seen[b].append(pos[b].copy())
        c = dict(slot=slots.copy(), prev_node=prev.copy(), step_id=np.full(B, t + 1, np.int32), cur_pos=pos.copy(),
                 cur_heading=rng.uniform(0, 2 * np.pi, B).astype(np.float32), cand_pos=cand, n_cand=K, cur_row=cur_row, cand_row=cand_row,
                 del_ghost=dele.copy(), noise=rng.standard_normal((B, GM, 3)))
        calls.append(c)
        o = shadow.update(**c)
        assert (o["record"][:, 2] == 0).all()
        for b in range(B):
            m = int(o["n_ghost"][b])
            prev[b] = o["cur_node"][b]
            if m and rng.random() < 0.8:
                g = int(rng.integers(m))
                dele[b] = g
                pos[b] = np.asarray(shadow.slots[slots[b]].gmean[g]) + [0.0, rng.uniform(-0.05, 0.05), 0.0]
            else:
                dele[b] = -1
                a = rng.uniform(0, 2 * np.pi)
                pos[b] = pos[b] + [3.0 * np.sin(a), 0.0, 3.0 * np.cos(a)]
    return calls, row


# Every random rollout the tests run, CPU and GPU alike, comes from this one table: name -> (B, steps, K, seed, S).  The CPU test asserts
# check_conditions for each of them (merge on and off), so the GPU comparison never meets a sequence that was not checked.
ROLLOUTS = {f"B{B}_K{K}": (B, 6, K, 1000 * B + 10 * K, B + 2) for B in (1, 3, 8) for K in (0, 1, 5, 16)}
ROLLOUTS.update(B8_mixed=(8, 6, None, 806, 10), slots=(4, 4, 5, 404, 6), integration=(3, 5, None, 306, 3), mutations=(3, 6, None, 306, 3))


def rollout(name):
    """-> (calls, store rows, B, S) of ROLLOUTS[name]"""
    B, steps, K, seed, S = ROLLOUTS[name]
    calls, rows = random_calls(B, steps, K, seed, S=S)
    return calls, rows, B, S


def merge_heavy_calls():
    """One slot, loc_noise 5, merge on, integer coordinates (every sum and mean exact): ghost 0 at A = (1000,0,0), ghost 1 at
    P = (2000,0,0), every candidate exactly on one of them; nodes at (0,0,10 i), far from both.  Calls 0 .. 16 put one candidate on A
    and 271 on P; calls 17 .. 31 alternate A, P, A, P ...: every merge into ghost 0 shifts a tail of more than 256 entries (ghost 1's
    list), the second entry per thread of the kernel's shift.  After call 31 the slot holds 512 absorbed candidates, its capacity.
    -> the 32 calls; one more candidate must then be refused, a call without candidates must pass."""
    A, P = [1000.0, 0.0, 0.0], [2000.0, 0.0, 0.0]
    calls, row = [], 0
    for i in range(32):
        cands = ([A] + [P] * 15) if i == 0 else [P] * 16 if i < 17 else [A, P] * 8
        cand = np.array(cands, dtype=np.float64)[None]
        rows = (row + 1 + np.arange(16, dtype=np.int32))[None]
        i32 = lambda x: np.array([x], np.int32)
        calls.append(dict(slot=i32(0), prev_node=i32(i - 1), step_id=i32(i + 1), cur_pos=np.array([[0.0, 0.0, 10.0 * i]]), cur_heading=np.zeros(1, np.float32),
                          cand_pos=cand, n_cand=i32(16), cur_row=i32(row), cand_row=rows, del_ghost=i32(-1), noise=None))
        row += 17
    return calls


def lattice_calls():
    """Crafted cases on integer / dyadic coordinates (every distance exact in double), one slot, loc_noise 5, merge on:
      call 0  node 0 at the origin; candidate (3,0,4): distance exactly 5 = loc_noise from node 0 -> EDGE to node 0 (`<=`);
              candidate (20,0,0) -> ghost 0
      call 1  node 1 at (0,0,8) (prev 0): candidate (0,0,4): 4 from node 0 and from node 1 -> EDGE to node 0 (the earlier one);
              candidates (40,0,0) and (44,0,0): the second merges into the ghost the first created -> duplicate front 1, mean (42,0,0);
              candidate (46.5,0,0): 6.5 from the first position but 4.5 from the mean -> merges only because the previous merge moved
              the mean from 40 to 42.
      call 2  node 2 at (20,0,3) (prev 1), 3 from ghost 0: candidate (20,0,1) is 2 from node 2 and 1 from ghost 0 -> EDGE to node 2
              (visited nodes are tested before ghosts); candidate (60,0,0) -> ghost 2
      call 3  ghost 0 (index 0 of three) is deleted: ghosts 1 and 2 keep their order; node 3 at (20,0,0) (prev 2), no candidates."""
    z = lambda *rows: np.array(list(rows) + [[0, 0, 0]] * (KMAX - len(rows)), dtype=np.float64)[None]
    mk = lambda prev, step, pos, cands, rows0, dele=-1: dict(
        slot=np.array([0], np.int32), prev_node=np.array([prev], np.int32), step_id=np.array([step], np.int32),
        cur_pos=np.array([pos], dtype=np.float64), cur_heading=np.zeros(1, np.float32), cand_pos=z(*cands),
        n_cand=np.array([len(cands)], np.int32), cur_row=np.array([rows0], np.int32),
        cand_row=np.array([[rows0 + 1 + k if k < len(cands) else -1 for k in range(KMAX)]], np.int32), del_ghost=np.array([dele], np.int32), noise=None)
    return [mk(-1, 1, [0, 0, 0], [[3, 0, 4], [20, 0, 0]], 0),
            mk(0, 2, [0, 0, 8], [[0, 0, 4], [40, 0, 0], [44, 0, 0], [46.5, 0, 0]], 3),
            mk(1, 3, [20, 0, 3], [[20, 0, 1], [60, 0, 0]], 8), mk(2, 4, [20, 0, 0], [], 11, dele=0)]


LATTICE_CODES = [[code(EDGE, 0), code(NEW, 0)], [code(EDGE, 0), code(NEW, 1), code(MERGED, 1), code(MERGED, 1)],
                 [code(EDGE, 2), code(NEW, 2)], []]


def load_fixture(path):
    import json
    return json.loads(str(np.load(path)["log"]))


def call_from_fixture(step, Kmax=KMAX):
    """the arguments of one recorded step (tests/golden/gmap_update_small.npz) for RefBatch.update / etp_gmap_update"""
    B = len(step["slot"])
    cand = np.zeros((B, Kmax, 3))
    rows = np.full((B, Kmax), -1, np.int32)
    for b in range(B):
        k = len(step["cand_pos"][b])
        if k:
            cand[b, :k] = step["cand_pos"][b]
            rows[b, :k] = step["cand_row"][b]
    i32 = lambda x: np.asarray(x, dtype=np.int32)
    return dict(slot=i32(step["slot"]), prev_node=i32(step["prev_node"]), step_id=i32(step["step_id"]), cur_pos=np.asarray(step["cur_pos"], dtype=np.float64),
                cur_heading=np.asarray(step["cur_heading"], dtype=np.float32), cand_pos=cand, n_cand=i32([len(c) for c in step["cand_pos"]]),
                cur_row=i32(step["cur_row"]), cand_row=rows, del_ghost=i32(step["del_ghost"]), noise=None)


def slot_state(s):
    """a RefSlot in the fixture's terms (JSON-able; doubles survive JSON bit for bit through repr)"""
    return dict(nodes=[str(i) for i in range(len(s.node_pos))], node_pos=[p.tolist() for p in s.node_pos], node_step=list(s.node_step),
                edges=sorted([str(i), str(j), w] for (i, j), w in s.edges.items()), ghosts=[f"g{g}" for g in s.gid],
                ghost_pos=[[p.tolist() for p in ps] for ps in s.gpos], ghost_mean=[p.tolist() for p in s.gmean],
                ghost_fronts=[[str(f) for f in fr] for fr in s.gfront], ghost_rows=[list(r) for r in s.grow], ghost_cnt=s.ghost_cnt)
