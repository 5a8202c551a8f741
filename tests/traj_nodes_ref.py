"""numpy restatement of the trajectory node features (etp_traj_nodes_fwd / etp_traj_nodes_bwd, csrc/traj_batch.hip) straight from the
integer tables, the planted mutations its pins must reject, and the crafted / random trajectories the tests share.

    tables(traj, G)                     the integer tables from string lists (independent of graph_inputs.traj_descriptors: names are
                                        numbered per sample in sorted order, so the two agree only up to a renaming of ids)
    forward(pano, tb, ...)              gmap_img_fts [B*G, H] + status [B*G]; dtype float64, or float32 as the ordered loop
                                        acc = w * x + acc from +0 with w = float32(1.0 / n); also sum |w x| and the terms per row
    backward(dg, tb, ...)               d_pano [R*V, H] + status [R], from the rules (A) / (B) per panorama row -- not from forward's lists
    dense_csr(fwd or bwd, src, n_out)   graph_inputs.pack_traj_csr's arrays applied as etp_gather_sum applies them

float32 loop: the product w * x is exact in float64 and the sum is rounded to 53 bits before it is rounded to 24, where the kernels
round once (a fused multiply-add).  The two differ only where the 53-bit sum lands exactly on a tie of the fp32 grid, about 2^-29 per
operation; the GPU tests hold the kernels to etp_gather_sum's bits and to the float64 result, not to this loop's bits.
"""
import numpy as np

ERR_COUNT, ERR_VIEWS, ERR_LEN, ERR_STEPS, ERR_NODE = 1, 8, 1, 16, 32
FWD_MUTATIONS = ["first_visit", "beyond_dropped_from_count", "weight_1_over_K", "later_visited_gets_candidates", "padding_nonzero"]
BWD_MUTATIONS = ["descending_nodes"]


def tables(traj, G):
    vpids, cands, gvps, lens = traj["traj_vpids"], traj["traj_cand_vpids"], traj["gmap_vpids"], traj["traj_vp_lens"]
    B, R = len(vpids), sum(len(p) for p in vpids)
    K = max(1, max((len(c) for s in cands for c in s), default=0))
    tb = {"step_off": np.zeros(B + 1, np.int32), "step_vp": np.full(R, -1, np.int32), "view_lens": np.zeros(R, np.int64),
          "cand_count": np.zeros(R, np.int32), "cand_vp": np.full((R, K), -1, np.int32), "gmap_id": np.full((B, G), -1, np.int32),
          "gmap_len": np.zeros(B, np.int32)}
    r = 0
    for i in range(B):
        names = sorted({vp for vp in vpids[i]} | {c for s in cands[i] for c in s} | {vp for vp in gvps[i] if vp is not None})
        num = {vp: 3 * k + 1 for k, vp in enumerate(names)}          # any distinct non-negative ids do
        for t, vp in enumerate(vpids[i]):
            tb["step_vp"][r], tb["view_lens"][r], tb["cand_count"][r] = num[vp], int(lens[i][t]), len(cands[i][t])
            tb["cand_vp"][r, :len(cands[i][t])] = [num[c] for c in cands[i][t]]
            r += 1
        tb["step_off"][i + 1] = r
        tb["gmap_len"][i] = len(gvps[i])
        tb["gmap_id"][i, :len(gvps[i])] = [-1 if vp is None else num[vp] for vp in gvps[i]]
    return tb


def same_up_to_renaming(a, b):
    """two sets of tables describe the same batch: equal shapes, counts and offsets, and per sample ONE bijection of ids carries
    step_vp, the live cand_vp slots and gmap_id[1:len] of `a` to those of `b`"""
    for k in ("step_off", "cand_count", "gmap_len"):
        if not np.array_equal(np.asarray(a[k]), np.asarray(b[k])):
            return False
    if any(np.asarray(a[k]).shape != np.asarray(b[k]).shape for k in ("step_vp", "cand_vp", "gmap_id")):
        return False
    off = np.asarray(a["step_off"])
    for i in range(len(off) - 1):
        pairs = []
        for t in range(off[i], off[i + 1]):
            pairs.append((int(a["step_vp"][t]), int(b["step_vp"][t])))
            pairs += [(int(a["cand_vp"][t, j]), int(b["cand_vp"][t, j])) for j in range(int(a["cand_count"][t]))]
        ln = int(a["gmap_len"][i])
        if a["gmap_id"][i, 0] != -1 or b["gmap_id"][i, 0] != -1:
            return False
        pairs += [(int(a["gmap_id"][i, g]), int(b["gmap_id"][i, g])) for g in range(1, ln)]
        f, inv = {}, {}
        for x, y in pairs:
            if x < 0 or y < 0 or f.setdefault(x, y) != y or inv.setdefault(y, x) != x:
                return False
    return True


def sample_status(tb, b, V):
    """the flags every wave of sample b raises (node rows and steps alike)"""
    R, G = len(tb["step_vp"]), tb["gmap_id"].shape[1]
    K = tb["cand_vp"].shape[1]
    t0, t1, ln = int(tb["step_off"][b]), int(tb["step_off"][b + 1]), int(tb["gmap_len"][b])
    err = ERR_LEN if ln < 1 or ln > G else 0
    if t0 < 0 or t1 > R or t1 <= t0:
        return err | ERR_STEPS
    if any(k < 0 or k > K for k in tb["cand_count"][t0:t1]):
        err |= ERR_COUNT
    if any(n < 1 or n > V for n in tb["view_lens"][t0:t1]):
        err |= ERR_VIEWS
    return err


def _weight(n, dtype):
    """the weight is an fp32 operand of both routes, float32(1.0 / n): the float64 restatement uses that value, not 1 / n"""
    w = np.float32(1.0 / float(n))
    return w if dtype == np.float32 else float(w)


def _fma(acc, w, x, dtype):
    if dtype == np.float32:
        return (np.float64(w) * x.astype(np.float64) + acc.astype(np.float64)).astype(np.float32)
    return w * x + acc


def _index(tb, t0, t1):
    """-> ({id: its steps, ascending}, {id: the slots (t, j) that name it, t then j ascending}) of the steps t0 .. t1-1"""
    visits, slots = {}, {}
    for t in range(t0, t1):
        visits.setdefault(int(tb["step_vp"][t]), []).append(t)
        for j in range(int(tb["cand_count"][t])):
            slots.setdefault(int(tb["cand_vp"][t, j]), []).append((t, j))
    return visits, slots


def forward(pano, tb, V, dtype=np.float64, fill=None, mutate=None):
    """pano [R*V, H] -> (out [B*G, H], status [B*G], mag [B*G, H] = sum |w x| in float64, terms [B*G])"""
    B, G = tb["gmap_id"].shape
    H = pano.shape[1]
    out = np.zeros((B * G, H), dtype) if fill is None else np.array(fill, dtype=dtype, copy=True)
    status, mag, terms = np.zeros(B * G, np.int32), np.zeros((B * G, H)), np.zeros(B * G, np.int64)
    x_of = lambda t, j: pano[t * V + j].astype(dtype)
    for b in range(B):
        err = sample_status(tb, b, V)
        if err:
            status[b * G:(b + 1) * G] = err
            continue
        t0, t1, ln = int(tb["step_off"][b]), int(tb["step_off"][b + 1]), int(tb["gmap_len"][b])
        visits, named = _index(tb, t0, t1)
        for g in range(G):
            row = b * G + g
            acc = np.zeros(H, dtype)
            if 1 <= g < ln:
                vp = int(tb["gmap_id"][b, g])
                vis = visits.get(vp, []) if vp >= 0 else []
                slots = named.get(vp, []) if vp >= 0 else []
                if mutate == "later_visited_gets_candidates" and vis:
                    extra = [(t, j) for t, j in slots if t < vis[-1]]
                else:
                    extra = []
                if vis:
                    t = vis[0] if mutate == "first_visit" else vis[-1]
                    n = int(tb["view_lens"][t])
                    src, div = [(t, j) for j in range(n)] + [s for s in extra if s[1] < int(tb["view_lens"][s[0]])], n + len(extra)
                elif slots:
                    live = [(t, j) for t, j in slots if j < int(tb["view_lens"][t])]
                    src, div = live, len(live) if mutate == "beyond_dropped_from_count" else len(slots)
                    if mutate == "weight_1_over_K":
                        div = tb["cand_vp"].shape[1]
                    div = max(div, 1)
                else:
                    status[row] = ERR_NODE
                    continue
                w = _weight(div, dtype)
                for t, j in src:
                    acc = _fma(acc, w, x_of(t, j), dtype)
                    mag[row] += np.abs(float(w) * pano[t * V + j].astype(np.float64))
                terms[row] = len(src)
            elif mutate == "padding_nonzero" and g >= ln:
                acc = acc + dtype(1e-3)
            out[row] = acc
    return out, status, mag, terms


def backward(dg, tb, V, dtype=np.float64, fill=None, mutate=None):
    """dg [B*G, H] -> (d_pano [R*V, H], status [R], mag [R*V, H], terms [R*V]); rules (A) and (B) per panorama row"""
    B, G = tb["gmap_id"].shape
    R, H = len(tb["step_vp"]), dg.shape[1]
    out = np.zeros((R * V, H), dtype) if fill is None else np.array(fill, dtype=dtype, copy=True)
    status, mag, terms = np.zeros(R, np.int32), np.zeros((R * V, H)), np.zeros(R * V, np.int64)
    off, index = tb["step_off"], {}
    for r in range(R):
        owners = [b for b in range(B) if off[b] <= r < off[b + 1]]
        status[r] = sample_status(tb, owners[0], V) if len(owners) == 1 else ERR_STEPS
        if status[r]:
            continue
        b = owners[0]
        t0, t1, ln = int(off[b]), int(off[b + 1]), int(tb["gmap_len"][b])
        if b not in index:
            index[b] = _index(tb, t0, t1) + ({int(tb["gmap_id"][b, g]): g for g in range(ln - 1, 0, -1)},)     # the first g of an id
        visits, named, listed = index[b]
        n = int(tb["view_lens"][r])
        for j in range(V):
            reads = []
            if j < n:
                vp = int(tb["step_vp"][r])
                if vp >= 0 and visits[vp][-1] == r and vp in listed:                                   # (A)
                    reads.append((listed[vp], n))
                if j < int(tb["cand_count"][r]):                                                       # (B)
                    c = int(tb["cand_vp"][r, j])
                    if c >= 0 and c not in visits and c in listed:
                        reads.append((listed[c], len(named[c])))
            reads.sort(reverse=mutate == "descending_nodes")
            acc = np.zeros(H, dtype)
            for g, div in reads:
                w = _weight(div, dtype)
                acc = _fma(acc, w, dg[b * G + g].astype(dtype), dtype)
                mag[r * V + j] += np.abs(float(w) * dg[b * G + g].astype(np.float64))
            out[r * V + j], terms[r * V + j] = acc, len(reads)
    return out, status, mag, terms


def dense_csr(csr, src, n_out, dtype=np.float64):
    """out[n] = sum_q w[q] * src[idx[q]], q ascending from +0 -- etp_gather_sum over pack_traj_csr's arrays"""
    p, idx, w = (np.asarray(x) for x in csr)
    out = np.zeros((n_out, src.shape[1]), dtype)
    for n in range(n_out):
        for q in range(int(p[n]), int(p[n + 1])):
            wq = np.float32(w[q]) if dtype == np.float32 else float(np.float32(w[q]))
            out[n] = _fma(out[n], wq, src[idx[q]].astype(dtype), dtype)
    return out


def gam(n, u=2.0 ** -24):
    """Higham's gamma_n: the relative error bound of n rounded operations in a row"""
    return n * u / (1 - n * u)


# ---- trajectories ------------------------------------------------------------------------------------------------------------------
def crafted(V):
    """One sample per case of the contract, for V >= 1 views (lengths are clipped to V): -> traj dict.
      s0  a viewpoint visited twice (the earlier visit's step feeds nothing: its one candidate is a visited node), a ghost seen from three
          steps and twice within one step, a candidate that is visited later
      s1  slots at and beyond view_len, a candidate that is visited later, a node order with (A)'s node after (B)'s
      s2  gmap_len = 1: only [stop]
      s3  one step, no candidates; the reverse node order of s1 ((A)'s node first)"""
    n = lambda x: max(1, min(V, x))
    vpids = [["a", "b", "c", "b"], ["p", "q", "r"], ["z"], ["m"]]
    lens = [[n(3), n(5), n(4), n(2)], [n(2), n(3), n(1)], [n(2)], [n(4)]]
    cands = [[["g", "b", "g"], ["a"], ["g", "h"], ["g", "c"]],
             [["u", "q", "u", "u"], ["r", "w", "w", "w", "u"], ["x", "y"]],
             [[]],
             [["k", "l"]]]
    gvps = [[None, "a", "b", "c", "g", "h"],
            [None, "u", "w", "x", "y", "p", "q", "r"],          # ghosts first: (B)'s node before (A)'s
            [None],
            [None, "m", "k", "l"]]                               # visited first: (A)'s node before (B)'s
    return {"traj_step_lens": [len(p) for p in vpids], "traj_vp_lens": lens, "traj_vpids": vpids, "traj_cand_vpids": cands, "gmap_vpids": gvps}


def random_traj(rng, B, V, steps, ks, names_per_sample=8):
    """B random samples: `steps[i]` steps, candidate counts drawn from `ks` (slots may exceed the valid views and V), revisits, repeated
    candidates, candidates visited later, a shuffled node order"""
    lens, vpids, cands, gvps = [], [], [], []
    for i in range(B):
        T = steps[i % len(steps)]
        names = [f"n{i}_{k}" for k in range(names_per_sample)]
        path = [names[rng.randint(0, max(1, names_per_sample // 2))] for _ in range(T)]
        ep_lens = [int(rng.randint(1, V + 1)) for _ in range(T)]
        ep_c = [[names[rng.randint(0, names_per_sample)] for _ in range(int(ks[rng.randint(0, len(ks))]))] for _ in range(T)]
        seen = []
        for t in range(T):
            for vp in [path[t]] + ep_c[t]:
                if vp not in seen:
                    seen.append(vp)
        seen = [seen[k] for k in rng.permutation(len(seen))]
        lens.append(ep_lens); vpids.append(path); cands.append(ep_c); gvps.append([None] + seen)
    return {"traj_step_lens": [len(p) for p in vpids], "traj_vp_lens": lens, "traj_vpids": vpids, "traj_cand_vpids": cands, "gmap_vpids": gvps}


def concat(a, b):
    return {k: list(a[k]) + list(b[k]) for k in a}


def scaled_rows(rng, rows, H):
    """standard normals with row scales 2^-10 .. 2^3"""
    return (rng.standard_normal((rows, H)) * np.exp2(rng.randint(-10, 4, size=(rows, 1)))).astype(np.float32)
