"""fp64 restatement of csrc/pano_store.hip (etp_pano_store_fwd / etp_pano_store_bwd) and of the store route built on it
(graph_inputs.EmbedStore + the embedding CSR + etp_gather_sum), with the shape lists the CPU and the GPU tests share and the
element-wise bounds both hold results to.

What is restated (vlnce_baselines/ss_trainer_ETP.py:838-839, 864-869; models/graph_utils.py:206,224,233,272-276; :360-365):
  row base_b          = sum of the unmasked views / their count
  row base_b + 1 + j  = the j-th view with nav_types == 1, in view order
  d pano[b,v]         = mask ? d_store[base_b] / len_b : 0   (+ d_store[base_b + 1 + rank(v)] on a candidate view)
  gmap_img_fts[b,g]   = sum over the entry's rows of w * row, w = 1 / rows (a visited node: its one row)

Bounds, u = 2^-24, gam(n) = n u / (1 - n u), no multiplier:
  mean row       gam(n_b) * sum_v |x_v| / n_b        n_b - 1 additions and one division
  candidate row  exact
  backward       u |t| + u |t + c|                   t the quotient, c the candidate term; exact where at most one term is present and
                                                     it is c (a copy) or nothing; a lone quotient carries u |t|, which the formula gives
  accumulate     + u |old + (t + c)|                 one more addition
The route's bounds propagate these through the gather's chain (route_fwd_bound, route_bwd_bound).

MUTATIONS names the planted errors the CPU test must see rejected; every restated function takes ``mut``."""
import numpy as np

U = 2.0 ** -24
ERR_EMPTY, ERR_MASKED, ERR_COUNT, ERR_ROW = 1, 2, 4, 8
KMAX, VMAX = 16, 64
HS, BS, VS = (256, 512, 768), (1, 3, 8), (1, 5, 13, 36, 64)
CASES = [(H, B, V) for H in HS for B in BS for V in VS]          # the GPU test's operator grid; the CPU test emulates each in fp32
CAND_COUNTS = (0, 1, 5, 16)                                      # and all V views where V <= 16
BIG = 1e30                                                       # what masked-out views hold: finite, so the reference's x * 0 ignores it too
MUTATIONS = ("mean_all_v", "div_by_v", "cand_reversed", "cand_by_mask", "bwd_no_mean_on_cand", "base_off_by_one", "detach_steps")


def gam(n):
    n = np.asarray(n, dtype=np.float64)
    return n * U / (1.0 - n * U)


# ---- the two kernels ---------------------------------------------------------------------------------------------------------------
def flags(masks, types, base, ncand, R):
    """status [B] of the episode checks, shared by both directions"""
    masks, types = np.asarray(masks) != 0, np.asarray(types)
    st = np.zeros(len(base), dtype=np.int32)
    for b in range(len(base)):
        cand = types[b] == 1
        k = int(cand.sum())
        st[b] = (ERR_EMPTY if not masks[b].any() else 0) | (ERR_MASKED if (cand & ~masks[b]).any() else 0) | \
                (ERR_COUNT if k != int(ncand[b]) else 0) | (ERR_ROW if (int(base[b]) < 0 or int(base[b]) + 1 + k > R) else 0)
    return st


def fwd(x, masks, types, base, ncand, store, mut=None, dtype=np.float64):
    """-> (store after the call, status).  ``store`` [R,H] is copied; with dtype float32 every operation is rounded to fp32 in the
    kernel's order (sequential sum in view order, one division): the emulation of its schedule."""
    x, store = np.asarray(x, dtype=dtype), np.array(store, dtype=dtype)
    masks, types = np.asarray(masks) != 0, np.asarray(types)
    st = flags(masks, types, base, ncand, store.shape[0])
    B, V, H = x.shape
    for b in range(B):
        if st[b]:
            continue
        r0 = int(base[b]) + (1 if mut == "base_off_by_one" else 0)
        use = np.ones(V, bool) if mut == "mean_all_v" else masks[b]
        acc = np.zeros(H, dtype=dtype)
        for v in range(V):
            if use[v]:
                acc = (acc + x[b, v]).astype(dtype)
        store[r0] = (acc / dtype(V if mut == "div_by_v" else masks[b].sum())).astype(dtype)
        cv = np.nonzero(types[b] == 1)[0]
        if mut == "cand_by_mask":
            cv = np.nonzero(masks[b])[0][:len(cv)]
        if mut == "cand_reversed":
            cv = cv[::-1]
        for j, v in enumerate(cv):
            store[r0 + 1 + j] = x[b, v]
    return store, st


def fwd_bound(x, masks, types, base, ncand, R):
    """[R,H] bound of the forward's rows against the fp64 values (0 on candidate rows and on rows the call leaves alone)"""
    x, masks = np.abs(np.asarray(x, dtype=np.float64)), np.asarray(masks) != 0
    st = flags(masks, types, base, ncand, R)
    out = np.zeros((R, x.shape[2]))
    for b in range(x.shape[0]):
        if not st[b]:
            n = masks[b].sum()
            out[int(base[b])] = gam(n) * x[b][masks[b]].sum(0) / n
    return out


def bwd_terms(d_store, masks, types, base, ncand, V, mut=None, dtype=np.float64):
    """-> (t, c, status): the quotient and the candidate term of every view, [B,V,H] each (zeros where absent or malformed)"""
    d_store = np.asarray(d_store, dtype=dtype)
    masks, types = np.asarray(masks) != 0, np.asarray(types)
    st = flags(masks, types, base, ncand, d_store.shape[0])
    B, H = len(base), d_store.shape[1]
    t, c = np.zeros((B, V, H), dtype=dtype), np.zeros((B, V, H), dtype=dtype)
    for b in range(B):
        if st[b]:
            continue
        r0 = int(base[b])
        rank = 0
        for v in range(V):
            is_cand = types[b, v] == 1
            if masks[b, v] and not (is_cand and mut == "bwd_no_mean_on_cand"):
                t[b, v] = (d_store[r0] / dtype(masks[b].sum())).astype(dtype)
            if is_cand:
                c[b, v] = d_store[r0 + 1 + rank]
                rank += 1
    return t, c, st


def bwd(d_store, masks, types, base, ncand, V, d_pano=None, accumulate=0, mut=None, dtype=np.float64):
    """-> d_pano [B,V,H].  accumulate == 0: everything is written (zeros on padding and malformed episodes); accumulate == 1: added to
    ``d_pano``, malformed episodes left alone."""
    t, c, st = bwd_terms(d_store, masks, types, base, ncand, V, mut, dtype)
    val = (t + c).astype(dtype)
    if not accumulate:
        return val
    out = np.array(d_pano, dtype=dtype)
    ok = st == 0
    out[ok] = (out[ok] + val[ok]).astype(dtype)
    return out


def bwd_bound(d_store, masks, types, base, ncand, V, d_pano=None, accumulate=0):
    t, c, st = bwd_terms(d_store, masks, types, base, ncand, V)
    bound = np.where(t != 0, U * np.abs(t) + np.where(c != 0, U * np.abs(t + c), 0.0), 0.0)
    if accumulate:
        ok = (st == 0)[:, None, None]
        bound = np.where(ok, bound + U * np.abs(np.asarray(d_pano, dtype=np.float64) + t + c), 0.0)
    return bound


# ---- the operator cases ------------------------------------------------------------------------------------------------------------
def make_case(H, B, V, seed=0):
    """One operator case: view lengths from 1 to V, candidate counts cycling through CAND_COUNTS (and V itself where V <= 16, clipped to
    the view length), candidates interleaved with panorama views, BIG at masked-out views, bases out of episode order with gaps.
    -> dict(x f32 [B,V,H], masks u8, types i64, base i32, ncand i32, R, d_store f32 [R,H])"""
    rng = np.random.default_rng([H, B, V, seed])
    lens = np.unique(np.linspace(1, V, B).round().astype(int)) if B > 1 else np.array([V])
    lens = np.resize(lens, B)
    lens[-1] = V
    if B > 1:
        lens[0] = 1
    counts = list(CAND_COUNTS) + ([V] if V <= KMAX else [])
    masks = np.zeros((B, V), np.uint8)
    types = np.zeros((B, V), np.int64)
    ncand = np.zeros(B, np.int32)
    for b in range(B):
        masks[b, :lens[b]] = 1
        k = min(counts[(b + V) % len(counts)] if b else counts[-1], int(lens[b]), KMAX)
        pick = np.sort(rng.permutation(int(lens[b]))[:k])           # interleaved: any subset of the unmasked views
        types[b, pick] = 1
        types[b, lens[b]:] = 2                                     # padding carries another type, never 1
        ncand[b] = k
    x = rng.standard_normal((B, V, H)).astype(np.float32)
    x[masks == 0] = BIG
    order = rng.permutation(B)
    base = np.zeros(B, np.int32)
    r = 2
    for b in order:                                                # out of episode order, one or two spare rows between blocks
        base[b] = r
        r += 1 + int(ncand[b]) + 1 + int(b % 2)
    R = r + 1
    d_store = rng.standard_normal((R, H)).astype(np.float32)
    return dict(x=x, masks=masks, types=types, base=base, ncand=ncand, R=R, d_store=d_store)


def written_rows(case):
    rows = []
    for b in range(len(case["base"])):
        rows += list(range(int(case["base"][b]), int(case["base"][b]) + 1 + int(case["ncand"][b])))
    return np.array(sorted(rows))


def malformed_cases(H=256, V=6):
    """name -> (case of three well-formed episodes with episode 1 made malformed, the expected flag of episode 1)"""
    out = {}
    for name, flag in (("empty", ERR_EMPTY), ("masked_cand", ERR_MASKED), ("count_low", ERR_COUNT), ("count_high", ERR_COUNT),
                       ("base_negative", ERR_ROW), ("rows_past_end", ERR_ROW)):
        rng = np.random.default_rng(7)
        c = dict(x=rng.standard_normal((3, V, H)).astype(np.float32), masks=np.ones((3, V), np.uint8), types=np.zeros((3, V), np.int64),
                 base=np.array([0, 4, 8], np.int32), ncand=np.array([2, 2, 2], np.int32), R=11)
        c["types"][:, [1, 4]] = 1
        c["masks"][:, [2, 5]] = 0                                  # a hole in the middle: masks need not be prefixes
        if name == "empty":
            c["masks"][1] = 0; c["types"][1] = 0; c["ncand"][1] = 0
        elif name == "masked_cand":
            c["types"][1, 4] = 0; c["types"][1, 5] = 1
        elif name == "count_low":
            c["ncand"][1] = 1
        elif name == "count_high":
            c["ncand"][1] = 3
        elif name == "base_negative":
            c["base"][1] = -1
        else:
            c["base"] = np.array([0, 9, 4], np.int32)               # 9 + 1 + 2 > 11, and episode 2 sits where episode 1 would
        c["d_store"] = rng.standard_normal((c["R"], H)).astype(np.float32)
        out[name] = (c, flag)
    return out


def fixture_w(seed, T, B, G, H):
    """W_t of the fixture's loss sum_t (gmap_img_fts_t * W_t).sum(), fp32-representable, from the recorded seed"""
    return np.random.default_rng(seed).standard_normal((T, B, G, H)).astype(np.float32).astype(np.float64)


# ---- the store route ---------------------------------------------------------------------------------------------------------------
def allocate(rows_used, ncand):
    """EmbedStore's row allocation: 1 + n_cand[b] consecutive rows per episode, in episode order, behind the rows used so far"""
    base = rows_used + np.concatenate([[0], np.cumsum(1 + np.asarray(ncand, dtype=np.int64))[:-1]])
    return base.astype(np.int32), [[int(base[b]) + 1 + j for j in range(int(k))] for b, k in enumerate(ncand)], int(rows_used + len(ncand) + np.sum(ncand))


def replay_plan(plan, make_map, embeds=None, snap=None):
    """Drive one map per episode (``make_map()``: anything with GraphMap's update_graph / delete_ghost) through the fixture's plan.
    embeds None: device-store mode, the maps are given ROW numbers (allocate); otherwise embeds(t, b) -> (cur, cand list) is given.
    -> (snap(map) per step and episode, the (base, n_cand) of every step, the rows used)"""
    B = len(plan[0]["cur_pos"])
    maps = [make_map() for _ in range(B)]
    out, alloc, used = [], [], 0
    for t, step in enumerate(plan):
        ncand = [len(c) for c in step["cand_pos"]]
        base, cand_rows, used = allocate(used, ncand)
        alloc.append((base, np.asarray(ncand, dtype=np.int32)))
        for b, g in enumerate(maps):
            if step["delete"][b] is not None:
                g.delete_ghost(step["delete"][b])
            vp = str(len(g.node_pos))
            cur, cand = (int(base[b]), cand_rows[b]) if embeds is None else embeds(t, b)
            g.update_graph(step["prev_vp"][b], t + 1, vp, np.asarray(step["cur_pos"][b], dtype=np.float64), cur,
                           [f"{vp}_{k}" for k in range(ncand[b])], [np.asarray(p, dtype=np.float64) for p in step["cand_pos"][b]], cand,
                           [None] * ncand[b])
        out.append([snap(g) for g in maps])
    return out, alloc, used


def entry_names(g):
    return list(g.node_pos.keys()) + list(g.ghost_pos.keys())


def entry_rows(g):
    """the (rows, weight) of every entry [stop, nodes, ghosts] of a GraphMapLite in device-store mode"""
    return [([], 1.0)] + [g.embed_rows(v) for v in entry_names(g)]


def route(pano, masks, types, entries, alloc, R, W, mut=None):
    """The store route in fp64: per step t fwd() into one store, gmap_img_fts_t [B,G,H] by the entries' weighted row sums, and the
    gradient of sum_t (gmap_img_fts_t * W_t).sum() with respect to every step's pano_embeds.
    -> (fts [T] of [B,G_t,H], d_pano [T,B,V,H], store [R,H])"""
    T, B, V, H = pano.shape
    store = np.zeros((R + 1, H))                                  # one spare row: only the off-by-one mutation reaches it
    fts = []
    d_store = np.zeros((T, R, H))                                 # d_store[t]: what step t's gather sends back
    for t in range(T):
        base, ncand = alloc[t]
        store, st = fwd(pano[t], masks[t], types[t], base, ncand, store, mut=mut if mut in MUTATIONS[:4] + ("base_off_by_one",) else None)
        assert not st.any(), st
        G = W[t].shape[1]
        f = np.zeros((B, G, H))
        for b in range(B):
            for g, (rows, w) in enumerate(entries[t][b]):
                for r in rows:
                    f[b, g] += w * store[r]
                    d_store[t, r] += w * W[t][b, g]
        fts.append(f)
    d_pano = np.zeros((T, B, V, H))
    for s in range(T):
        base, ncand = alloc[s]
        lo, hi = int(base[0]), int(base[-1]) + 1 + int(ncand[-1])
        total = d_store[s] if mut == "detach_steps" else d_store[s:].sum(0)
        d_pano[s] = bwd(total[lo:hi], masks[s], types[s], base - lo, ncand, V, mut=mut if mut == "bwd_no_mean_on_cand" else None)
    return fts, d_pano, store[:R]


def route_fwd_bound(pano, masks, types, entries, alloc, R, W):
    """[T] of [B,G,H]: a c-row entry is sum_j fl(w) * row_j accumulated in fp32 (c + 1 roundings per term: w, the product, c - 1
    additions), each row carrying its own forward bound"""
    T, B, V, H = pano.shape
    row_abs, row_err = np.zeros((R, H)), np.zeros((R, H))
    out = []
    store = np.zeros((R, H))
    for t in range(T):
        base, ncand = alloc[t]
        store, _ = fwd(pano[t], masks[t], types[t], base, ncand, store)
        row_err += fwd_bound(pano[t], masks[t], types[t], base, ncand, R)
        row_abs = np.abs(store)
        f = np.zeros((B, W[t].shape[1], H))
        for b in range(B):
            for g, (rows, w) in enumerate(entries[t][b]):
                c = len(rows)
                for r in rows:
                    f[b, g] += gam(c + 1) * w * row_abs[r] + w * row_err[r] * (1 + gam(c + 1))
        out.append(f)
    return out


def route_bwd_bound(pano, masks, types, entries, alloc, R, W):
    """[T,B,V,H]: d_store[r] is the fp32 sum over the later steps of fl(w) * W (two roundings per term and one per addition:
    gam(2 + steps - 1) on the sum of magnitudes); the backward kernel then adds u |t| + u |t + c| and passes the incoming errors on
    (the quotient's through one more rounding)."""
    T, B, V, H = pano.shape
    mag = np.zeros((T, R, H))
    val = np.zeros((T, R, H))
    for t in range(T):
        for b in range(B):
            for g, (rows, w) in enumerate(entries[t][b]):
                for r in rows:
                    mag[t, r] += w * np.abs(W[t][b, g]); val[t, r] += w * W[t][b, g]
    out = np.zeros((T, B, V, H))
    for s in range(T):
        base, ncand = alloc[s]
        lo, hi = int(base[0]), int(base[-1]) + 1 + int(ncand[-1])
        e_rows = gam(2 + (T - s) - 1) * mag[s:].sum(0)[lo:hi]
        d = val[s:].sum(0)[lo:hi]
        own = bwd_bound(d, masks[s], types[s], base - lo, ncand, V)
        e_t, e_c, _ = bwd_terms(e_rows, masks[s], types[s], base - lo, ncand, V)
        out[s] = own + e_t * (1 + 2 * U) + e_c * (1 + U)
    return out
