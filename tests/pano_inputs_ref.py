"""numpy restatement of etp_pano_inputs (csrc/pano_inputs.hip), its cases, its comparator and the mutations that comparator must reject.

    pano_inputs(rgb, dep, table, in_train, V)   (rgb [12B,F] fp32 clockwise, dep [12B,C,HW] fp32 clockwise, table [7,B,max_pred] int32)
        -> the seven outputs: rgb_fts, dep_fts (float64 mean), loc_fts, nav_types, view_lens, cand_img, status, and dep_bound

It restates vlnce_baselines/models/Policy_ViewSelection_ETP.py:289-342 followed by vlnce_baselines/ss_trainer_ETP.py:308-342 as one
function of the encoders' outputs and the candidate table; tests/test_pano_inputs_ref_cpu.py pins it to the recording of the real branch
(tests/golden/waypoint_small.npz, through tests/move_ref.py's restatement of _vp_feature_variable, itself pinned to the real method) and
to waypoint._waypoint_tail_mode on the crafted tables below.

Bound of dep_fts.  The kernel adds a channel's HW values in index order into one fp32 accumulator (HW - 1 roundings; the first add onto
0.0f is exact) and divides once (one rounding): with u = 2^-24 and gam(k) = k u / (1 - k u) as in tests/reduce_ref.py,

    |got - ref| <= gam(HW) * mean|x| + u * |ref|

per element, no multiplier.  gam(HW - 1) (1 + u) <= gam(HW) covers the sum's error carried through the division; the second term is
the division's own rounding (the bound holds for any order of the HW additions, so torch's own pool is inside it too).  A padding row
has mean|x| = ref = 0: its bound is 0.  Every other output is exact.
"""
import math

import numpy as np
import torch

from etpnav_amd import waypoint as wp
from tests.reduce_ref import U, gam

ERR_COUNT, ERR_ANGLE, ERR_VIEWS = 1, 2, 4
MUTATIONS = ("slot", "no_wrap", "no_plus5", "free_clockwise", "dup_twice", "eval_in_train", "no_division", "cand_last", "pad_nav",
             "pad_values")
WORST = {}


def tables():
    """(cand_angle_tab [120,4], pano_angle_tab [12,4]) fp32, as the host layer builds them"""
    return wp.cand_angle_table().numpy().copy(), wp.pano_constants()[1].numpy().copy()


def img_of(a, mutate=None):
    i = 12 - (a // 10 if mutate == "no_plus5" else (a + 5) // 10)
    return i if (i != 12 or mutate == "no_wrap") else 0


def pano_inputs(rgb, dep, table, in_train, V, mutate=None):
    """-> dict of the seven outputs (+ dep_bound, written [B] bool).  Rows of a flagged episode (written False) hold zeros here and are
    compared by nobody: the kernel leaves the caller's fill there."""
    rgb, dep, table = np.asarray(rgb), np.asarray(dep), np.asarray(table)
    B, mp = table.shape[1], table.shape[2]
    F, C, HW = rgb.shape[1], dep.shape[1], dep.shape[2]
    assert rgb.shape[0] == dep.shape[0] == 12 * B and rgb.dtype == dep.dtype == np.float32
    cand_tab, pano_tab = tables()
    ang_row = 1 if (not in_train or mutate == "eval_in_train") else 5
    out = {"rgb_fts": np.zeros((B, V, F), np.float32), "dep_fts": np.zeros((B, V, C), np.float64), "loc_fts": np.zeros((B, V, 4), np.float32),
           "nav_types": np.zeros((B, V), np.int64), "view_lens": np.zeros(B, np.int64), "cand_img": np.full((B, mp), -1, np.int32),
           "status": np.zeros(B, np.int32), "dep_bound": np.zeros((B, V, C), np.float64), "written": np.zeros(B, bool)}
    d64 = dep.astype(np.float64)
    mean = d64.sum(-1) if mutate == "no_division" else d64.mean(-1)             # [12B, C]
    mag = np.abs(d64).mean(-1)
    for b in range(B):
        k = int(table[0, b, 0])
        if k < 0 or k > mp:
            out["status"][b] = ERR_COUNT
            continue
        ang = [int(a) for a in table[ang_row, b, :k]]
        if any(a < 0 or a > 119 for a in ang):
            out["status"][b] |= ERR_ANGLE
        imgs = [img_of(a, mutate) for a in ang if 0 <= a <= 119]
        n = (k + 12 - len(imgs)) if mutate == "dup_twice" else (k + 12 - len(set(imgs) & set(range(12))))
        if n > V:
            out["status"][b] |= ERR_VIEWS
        if out["status"][b]:
            continue
        free = [i for i in range(12) if i not in imgs]
        if mutate == "free_clockwise":
            free = free[:1] + free[:0:-1] if free and free[0] == 0 else free[::-1]
        rows = [(i, 1, cand_tab[a]) for i, a in zip(imgs, ang)]
        frees = [(i, 0, pano_tab[i]) for i in free]
        rows = (frees + rows) if mutate == "cand_last" else (rows + frees)
        rows = rows[:n] if mutate == "dup_twice" else rows
        assert len(rows) == n or mutate is not None, (b, len(rows), n)
        for v, (i, nav, loc) in enumerate(rows[:V]):
            src = b * 12 + (i % 12 if mutate == "slot" else (12 - i) % 12)
            out["rgb_fts"][b, v] = rgb[src]
            out["dep_fts"][b, v] = mean[src]
            out["dep_bound"][b, v] = gam(HW) * mag[src] + U * np.abs(mean[src])
            out["loc_fts"][b, v] = loc
            out["nav_types"][b, v] = nav
        if mutate == "pad_nav":
            out["nav_types"][b, n:] = 1
        if mutate == "pad_values" and n < V:
            out["rgb_fts"][b, V - 1, F - 1] = 1.0
        out["view_lens"][b] = n
        out["cand_img"][b, :k] = imgs
        out["written"][b] = True
    return out


# ---- comparator (tests/test_pano_inputs_gpu.py uses this and nothing else for the operator's outputs) ----------------------------------
def _bits_equal(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


def check(name, got, ref, const_channel=None):
    """got: dict of numpy arrays as the kernel left them (flagged episodes: whatever the buffers held).  Every written episode: rgb_fts,
    loc_fts, nav_types, view_lens, cand_img bit for bit; dep_fts within dep_bound on every element (padding rows: bound 0, and their
    bits must be +0.0); `const_channel`: a channel whose HW values are equal and short enough that every partial sum is exact -- its mean
    is that value, bit for bit.  status is exact for every episode."""
    assert _bits_equal(got["status"], ref["status"]), f"{name}: status {got['status'].tolist()} != {ref['status'].tolist()}"
    w = ref["written"]
    for k in ("rgb_fts", "loc_fts", "nav_types", "view_lens", "cand_img"):
        assert got[k].dtype == ref[k].dtype and got[k].shape == ref[k].shape, (name, k, got[k].dtype, got[k].shape, ref[k].shape)
        assert _bits_equal(got[k][w], ref[k][w]), f"{name}: {k} differs bitwise in {int((got[k][w] != ref[k][w]).sum())} elements"
    g = got["dep_fts"]
    assert g.dtype == np.float32 and g.shape == ref["dep_fts"].shape, (name, g.dtype, g.shape)
    g, r, bnd = g[w].astype(np.float64), ref["dep_fts"][w], ref["dep_bound"][w]
    assert np.isfinite(g).all(), f"{name}: dep_fts holds {int((~np.isfinite(g)).sum())} non-finite elements"
    err = np.abs(g - r)
    ratio = np.where(bnd > 0, err / np.maximum(bnd, 1e-300), np.where(err > 0, np.inf, 0.0))
    worst = float(ratio.max()) if ratio.size else 0.0
    WORST[name] = max(WORST.get(name, 0.0), worst)
    assert worst <= 1.0, f"{name}: dep_fts {int((ratio > 1).sum())} of {ratio.size} elements beyond their bound, worst err / bound {worst:.3g}"
    pad = np.arange(ref["dep_fts"].shape[1])[None, :] >= ref["view_lens"][:, None]
    assert not got["dep_fts"][w][pad[w]].view(np.int32).any(), f"{name}: a padding row of dep_fts is not +0.0"
    if const_channel is not None:
        assert _bits_equal(got["dep_fts"][w][..., const_channel], r[..., const_channel].astype(np.float32)), \
            f"{name}: the constant channel's mean is not the constant"
    return worst


# ---- cases ------------------------------------------------------------------------------------------------------------------------
MAX_PRED = 5
# crafted episodes: (name, eval angles, train angles) -- the count is shared by the two modes, as in etp_waypoint_tail's table
CRAFTED = (
    ("edges", (4, 5, 114, 115, 119), (119, 0, 5, 64, 65)),          # the wrap 12 -> 0 and both edges of (a + 5) / 10; views {0, 11, 1}
    ("k0", (), ()),
    ("k1", (57,), (3,)),
    ("one_view", (55, 57, 59, 61, 64), (64, 55, 60, 58, 62)),        # five candidates in view 6: view_len 16
    ("distinct", (0, 24, 48, 72, 96), (96, 3, 50, 17, 110)),         # five views: view_len 12; train: table order is not angle order
    ("zero", (0,), (115,)),
    ("pairs", (10, 12, 100, 101), (34, 35, 36, 80)),
    ("k3", (118, 30, 31), (29, 89, 90)),
)
B_LIST = (1, 3, 8, 33)
DIMS = ((512, 128, 16), (16, 8, 16), (260, 6, 1))                     # (Frgb, C, HW)
V_MODES = ("ref", 16, 20)


def crafted_table(B, shift=0, seed=0):
    """[7, B, 5] int32: episode b is CRAFTED[(b + shift) % 8] for b < 16, random (K 0 .. 5, any angles) beyond; distances random"""
    rng = np.random.default_rng(1000 + 10 * seed + B)
    t = np.full((7, B, MAX_PRED), -1, np.int32)
    for b in range(B):
        if b < 16:
            _, ev, tr = CRAFTED[(b + shift) % len(CRAFTED)]
        else:
            k = int(rng.integers(0, MAX_PRED + 1))
            ev, tr = rng.integers(0, 120, k), rng.integers(0, 120, k)
        k = len(ev)
        t[0, b, 0] = k
        t[1, b, :k], t[5, b, :k] = ev, tr
        t[2, b, :k], t[6, b, :k] = rng.integers(0, 12, k), rng.integers(0, 12, k)
        cc = np.array([img_of(int(a)) for a in ev], dtype=np.int32)
        t[4, b, :k], t[3, b, :k] = cc, (12 - cc) % 12
    return t


def cases():
    """(B, (Frgb, C, HW), shift): every B x dims; tests/test_pano_inputs_gpu.py runs each at V in V_MODES and in both table modes"""
    return [(B, d, i + j) for i, B in enumerate(B_LIST) for j, d in enumerate(DIMS)]


def make_inputs(B, dims, seed=0):
    """rgb [12B, F], dep [12B, C, HW] fp32: depth channels carry scales 2^-10 .. 2^3, channel C // 2 is constant per view (a 4-bit
    value, so every partial sum of up to 16 of them is exact) -> rgb, dep, const_channel"""
    F, C, HW = dims
    rng = np.random.default_rng(77 + 13 * seed + B + F)
    rgb = rng.standard_normal((12 * B, F)).astype(np.float32)
    scale = 2.0 ** ((np.arange(C) * 5) % 14 - 10)
    dep = (rng.standard_normal((12 * B, C, HW)) * scale[None, :, None]).astype(np.float32)
    cc = C // 2
    dep[:, cc, :] = ((1.0 + (np.arange(12 * B) % 7) / 8.0) * scale[cc])[:, None].astype(np.float32)
    return rgb, dep, cc


# ---- the recording of the real branch (tests/golden/waypoint_small.npz) ---------------------------------------------------------------
def golden_tables(z):
    """clockwise rgb [36, 512] / dep [36, 128, 16] fp32 as the encoders emitted them, from the id-indexed (counter-clockwise) tables"""
    B = 3
    cw = [(12 - s) % 12 for s in range(12)]                    # clockwise slot s holds counter-clockwise view (12 - s) % 12
    rgb = z["rgb_table"].astype(np.float32).reshape(B, 12, 512)[:, cw].reshape(12 * B, 512)
    dep = z["depth_cw"].astype(np.float32).reshape(12 * B, 128, 16)
    assert np.array_equal(z["depth_table"].astype(np.float32).reshape(B, 12, 2048)[:, cw].reshape(12 * B, 128, 16), dep)
    return rgb, dep


def golden_table(z):
    """the candidate table [7, 3, 5] behind the recording: angle indices back from cand_angles = 2 pi - a / 120 * 2 pi (:308)"""
    t = np.full((7, 3, 5), -1, np.int32)
    for row, prefix in ((1, "eval_"), (5, "train_")):
        for j in range(3):
            ang = z[f"{prefix}cand_angles_{j}"]
            a = np.rint(120 * (1 - ang / (2 * math.pi))).astype(np.int64) % 120
            assert np.abs((2 * math.pi - a / 120 * 2 * math.pi) - ang).max() < 1e-5
            k = len(a)
            if row == 1:
                t[0, j, 0] = k
            assert t[0, j, 0] == k
            t[row, j, :k] = a
            t[row + 1, j, :k] = np.rint(z[f"{prefix}cand_distances_{j}"] / 0.25).astype(np.int64) - 1
    return t


def ref_length(table, in_train):
    return max(12, int(wp.host_view_lens(table, in_train).max()))


def view_len(angles):
    return len(angles) + 12 - len({img_of(a) for a in angles})


def assert_case_conditions():
    """what the issue asks of the case list, on the reference alone"""
    by = {n: (e, t) for n, e, t in CRAFTED}
    assert view_len(by["k0"][0]) == 12 and len(by["k1"][0]) == 1
    assert len({img_of(a) for a in by["one_view"][0]}) == 1 and view_len(by["one_view"][0]) == 16 and view_len(by["one_view"][1]) == 16
    assert len({img_of(a) for a in by["distinct"][0]}) == 5 and view_len(by["distinct"][0]) == 12
    seen = {a for _, e, t in CRAFTED for a in e + t}
    assert {4, 5, 114, 115, 119, 0} <= seen
    assert [img_of(a) for a in (4, 5, 114, 115, 119, 0)] == [0, 11, 1, 0, 0, 0]
    tr = by["distinct"][1]
    assert list(tr) != sorted(tr) and list(tr) != sorted(tr, reverse=True)
    assert any(e != t for _, e, t in CRAFTED)
    for B, _, shift in cases():                                       # every B sees a table whose two modes differ
        t = crafted_table(B, shift)
        assert (t[1] != t[5]).any() or int(t[0, :, 0].max()) == 0, (B, shift)
    names = {CRAFTED[(b + s) % len(CRAFTED)][0] for B, _, s in cases() for b in range(min(B, 16))}
    assert names == set(by), names


def angle_table_identity(draws=20000, seed=5):
    """the 120-row table equals angle_feature_torch(a.float() / 120 * 2 pi) bit for bit for tensors of 1 .. 5 indices -> mismatches"""
    tab = wp.cand_angle_table()
    g = torch.Generator().manual_seed(seed)
    ks = torch.randint(1, 6, (draws,), generator=g).tolist()
    idx = torch.randint(0, 120, (sum(ks),), generator=g)
    bad, o = 0, 0
    for k in ks:
        a = idx[o:o + k]
        o += k
        f = wp.angle_feature_torch(a.float() / 120 * 2 * math.pi)
        bad += int((f.contiguous().view(torch.int32) != tab[a].contiguous().view(torch.int32)).any())
    return bad
