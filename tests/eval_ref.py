"""fp64 restatements, case lists, emulations and derived bounds for the validation tails of csrc/eval_tail.hip
(tests/test_eval_gpu.py runs them through the C ABI, tests/test_eval_ref_cpu.py pins and emulates them without a GPU):

  vocab_eval_kernel (etp_vocab_eval), sap_eval_kernel (etp_sap_eval), eval_accum_kernel (etp_eval_accum)

and the two-batch validation loaders of tests/golden/pretrain_validate_small.npz (tools/make_golden_pretrain_validate.py).
Both test files take every case from the lists of this module and from nowhere else.

Semantics (torch on the CPU, pinned in tests/test_eval_ref_cpu.py): ties of the maximum go to the lowest column; a label on a -inf
logit gives nll = +inf; a row of only -inf gives pred 0 and a NaN nll; ignored rows (SAP) have nll 0 and still an arg-max.

Bounds, without a multiplier.  u = 2^-24, gam(k) = k u / (1 - k u) (tests/reduce_ref.py).  Nothing is fitted to what a kernel returns.

  row nll: the kernels compute lse in vocab_ce_kernel's / sap_ce_kernel's order, so the e_lse term of move_ref.vce_reference /
    reduce_ref.ce_bounds applies at the chain depth d = ceil(V / 256) + 6 + 3 (vocab), ceil(G / 64) + 6 (SAP):
        e_sum = 2u + u max|s - mx| + gam(d)            relative error of sum_k exp(s_k - mx)
        e_lse = e_sum + 2u |log sum| + u |lse|         absolute error of lse
    and nll = lse - s[y] is one more rounded subtraction of an exactly read logit:  e_lse + u |nll|.
    Rows whose reference is +inf or NaN must BE +inf / NaN; ignored rows must be exactly 0; pred is exact.
  loss_sum: against the float64 sum of the kernel's OWN row_nll (kept rows) plus the record's previous value.  Every partial sum is
    a double, the chain (ceil(n / 256) sequential adds, 8 tree levels, the add onto the record) is shorter than n + 1 roundings:
        (n + 1) 2^-53 (|previous| + sum_r |nll_r|)
    -- the previous value of the record is one more summand; with a zeroed record this is (n + 1) 2^-53 sum |nll|.
  n_correct, n_rows, n_counted, and everything a second run returns (bit for bit): exact.
"""
import os
import struct

import numpy as np
import torch

from tests import move_ref as mv
from tests import reduce_ref as rf
from tests.reduce_ref import F64, U, cdiv, gam

F32 = torch.float32
NO_COL = 0x7FFFFFFF
U53 = 2.0 ** -53
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "pretrain_validate_small.npz")
WORST = {}


# ---- float64 restatement ---------------------------------------------------------------------------------------------------------
def argmax_lowest(s):
    """lowest column of the row maximum, written without torch.argmax / max(dim) (those are what it is pinned to)"""
    mx = s.max(-1, keepdim=True).values
    cols = torch.arange(s.shape[-1], device=s.device).expand_as(s)
    return torch.where(s == mx, cols, torch.full_like(cols, NO_COL)).min(-1).values


def tail(logits, labels, ignore_index=None):
    """logits [n, C] (any float dtype; -inf allowed, no NaN), labels [n] int64 -> dict of float64 row pieces:
    nll (0 on ignored rows, +inf for a label on -inf, NaN for a row of only -inf), pred (int64), keep, and what the bound uses"""
    s = logits.to(F64)
    n, C = s.shape
    keep = torch.ones(n, dtype=torch.bool, device=s.device) if ignore_index is None else labels != ignore_index
    mx = s.max(-1, keepdim=True).values
    sm = torch.exp(s - mx).sum(-1, keepdim=True)
    lse = mx + torch.log(sm)
    y = torch.where(keep, labels, torch.zeros_like(labels))
    nll = (lse - s.gather(1, y[:, None])).squeeze(1)
    nll = torch.where(keep, nll, torch.zeros_like(nll))
    return {"nll": nll, "pred": argmax_lowest(s), "keep": keep, "s": s, "mx": mx, "sum": sm, "lse": lse}


def nll_bound(q, depth):
    """per-row bound of the fp32 nll (module docstring); rows with a non-finite reference get 0 (they are asserted apart)"""
    s, lse, mx, sm, nll = q["s"], q["lse"], q["mx"], q["sum"], q["nll"]
    fin = torch.isfinite(s)
    span = torch.where(fin, (s - mx).abs(), torch.zeros_like(s)).max(-1, keepdim=True).values
    e_sum = (2 * U + U * span) + gam(depth)
    e_lse = (e_sum + 2 * U * torch.log(sm).abs() + U * lse.abs()).squeeze(1)
    b = e_lse + U * nll.abs()
    return torch.where(torch.isfinite(nll) & q["keep"], b, torch.zeros_like(b))


def vocab_depth(V):
    return cdiv(V, 256) + 6 + 3


def sap_depth(G):
    return cdiv(G, 64) + 6


def accumulate(record, nll, pred, labels, ignore_index):
    """the record after one etp_eval_accum call, in float64 / exact integers.  record = (loss_sum, n_correct, n_rows, n_counted)"""
    keep = labels != ignore_index
    loss = float(nll.to(F64)[keep].sum()) if bool(keep.any()) else 0.0
    correct = int((keep & (pred.to(torch.int64) == labels)).sum())
    return (record[0] + loss, record[1] + correct, record[2] + int(labels.numel()), record[3] + int(keep.sum()))


def metrics(record, keys):
    """the reference's val_log without the time field (train_r2r.py:373-377, :433-441)"""
    return {keys[0]: record[0] / record[2], keys[1]: record[1] / record[2]}


# ---- comparators -----------------------------------------------------------------------------------------------------------------
def within(key, got, ref, bound):
    try:
        return rf.within(key, got, ref, bound)
    finally:
        WORST[key] = max(WORST.get(key, 0.0), rf.WORST.get(key, 0.0))


def check_rows(name, nll, pred, q, depth):
    """nll [n] fp32, pred [n] int32 of a kernel (or an emulation) against tail()'s q"""
    assert nll.dtype == F32 and pred.dtype == torch.int32, (name, nll.dtype, pred.dtype)
    nll, pred = nll.cpu(), pred.cpu()
    ref = q["nll"]
    bad = int((pred.to(torch.int64) != q["pred"]).sum())
    assert bad == 0, f"{name}: {bad} of {pred.numel()} arg-max columns differ from the lowest-index arg-max"
    inf, nan = torch.isposinf(ref), torch.isnan(ref)
    assert bool(torch.isposinf(nll[inf]).all()), f"{name}: a label on a -inf logit did not give +inf"
    assert bool(torch.isnan(nll[nan]).all()), f"{name}: a row of only -inf did not give NaN"
    ign = ~q["keep"]
    assert bool((nll[ign] == 0).all()), f"{name}: an ignored row's nll is not 0"
    fin = ~(inf | nan)
    if bool(fin.any()):
        within((name, "row_nll"), nll[fin], ref[fin], nll_bound(q, depth)[fin])


def check_record(name, got, before, nll, pred, labels, ignore_index):
    """got / before: records; nll / pred: what the kernel itself wrote per row (the loss bound is against ITS float64 sum)"""
    n = int(labels.numel())
    want = accumulate(before, nll.cpu(), pred.cpu(), labels.cpu(), ignore_index)
    assert tuple(got[1:]) == tuple(want[1:]), f"{name}: counts (n_correct, n_rows, n_counted) {tuple(got[1:])}, expected {tuple(want[1:])}"
    keep = labels.cpu() != ignore_index
    mag = abs(before[0]) + float(nll.cpu().to(F64)[keep].abs().sum())
    if not np.isfinite(want[0]):
        assert (np.isnan(want[0]) and np.isnan(got[0])) or got[0] == want[0], f"{name}: loss_sum {got[0]}, expected {want[0]}"
        return
    t = lambda v: torch.tensor(v, dtype=F64)
    within((name, "loss_sum"), t(got[0]), t(want[0]), t((n + 1) * U53 * mag))


def unpack_record(t):
    """a [4] int64 tensor holding the 32-byte record -> (loss_sum, n_correct, n_rows, n_counted)"""
    return struct.unpack("<dqqq", t.cpu().contiguous().numpy().tobytes())


def pack_record(rec, device="cpu"):
    return torch.from_numpy(np.frombuffer(struct.pack("<dqqq", *rec), dtype=np.int64).copy()).to(device)


# ---- emulations of the kernels' schedules (fp32 rows, double accumulation); `mutate` plants one defect --------------------------
def _pair_take(v, c, ov, oc, high=False):
    tie = (oc > c) if high else (oc < c)
    take = (ov > v) | ((ov == v) & tie)
    return torch.where(take, ov, v), torch.where(take, oc, c)


def _strided_argmax(s, lanes, high=False):
    """s [n, C] fp32 -> per-thread (value, column) [n, lanes]: the first column as it is, then strict > (>= for the planted defect)"""
    n, C = s.shape
    J = cdiv(C, lanes)
    pad = torch.full((n, J * lanes - C), float("-inf"), dtype=F32)
    x = torch.cat([s, pad], 1).reshape(n, J, lanes)
    col = torch.arange(J * lanes).reshape(1, J, lanes).expand(n, J, lanes)
    live = col < C
    v = torch.full((n, lanes), float("-inf"), dtype=F32)
    c = torch.full((n, lanes), NO_COL, dtype=torch.int64)
    for j in range(J):
        xj, cj, lj = x[:, j], col[:, j], live[:, j]
        take = lj & ((c == NO_COL) | ((xj >= v) if high else (xj > v)))
        v, c = torch.where(take, xj, v), torch.where(take, cj, c)
    return v, c


def _wave_argmax(v, c, high=False):
    idx = torch.arange(64)
    for o in (32, 16, 8, 4, 2, 1):
        v, c = _pair_take(v, c, v[:, idx ^ o], c[:, idx ^ o], high)
    return v[:, 0], c[:, 0]


def _lse32(s, mx, lanes):
    n, C = s.shape
    J = cdiv(C, lanes)
    e = torch.cat([torch.exp(s - mx[:, None]), torch.zeros(n, J * lanes - C, dtype=F32)], 1).reshape(n, J, lanes)
    acc = torch.zeros(n, lanes, dtype=F32)
    for j in range(J):
        acc = acc + e[:, j]
    w = rf._wave_sum32(acc.reshape(n * (lanes // 64), 64)).reshape(n, lanes // 64)
    tot = w[:, 0]
    for k in range(1, lanes // 64):
        tot = tot + w[:, k]
    return mx + torch.log(tot)


def _row_nll32(s, lse, labels, keep, shift=0):
    n, C = s.shape
    y = labels + shift
    ok = keep & (y >= 0) & (y < C)
    nll = lse - s.gather(1, torch.where(ok, y, torch.zeros_like(y))[:, None]).squeeze(1)
    nll = torch.where(ok, nll, torch.full_like(nll, float("nan")))
    return torch.where(keep, nll, torch.zeros_like(nll))


def emulate_vocab_eval(buf, labels, V, mutate=None):
    """vocab_eval_kernel: 256 strided threads, the pair butterfly per wave, the four waves' pairs in order, then vocab_ce's sum"""
    high = mutate == "tie_high"
    s = buf[:, :(buf.shape[1] if mutate == "argmax_ldv" else V)].to(F32)
    n = s.shape[0]
    v, c = _strided_argmax(s, 256, high)
    wv, wc = _wave_argmax(v.reshape(n * 4, 64), c.reshape(n * 4, 64), high)
    wv, wc = wv.reshape(n, 4), wc.reshape(n, 4)
    mx, col = wv[:, 0], wc[:, 0]
    for w in range(1, 4):
        mx, col = _pair_take(mx, col, wv[:, w], wc[:, w], high)
    s = buf[:, :V].to(F32)
    lse = _lse32(s, s.max(-1).values if mutate == "argmax_ldv" else mx, 256)
    keep = torch.ones(n, dtype=torch.bool)
    return _row_nll32(s, lse, labels, keep, 1 if mutate == "labels_shifted" else 0), col.to(torch.int32)


def emulate_sap_eval(logits, labels, ignore_index, mutate=None):
    """sap_eval_kernel: one wave per row"""
    high = mutate == "tie_high"
    s = logits.to(F32)
    v, c = _strided_argmax(s, 64, high)
    mx, col = _wave_argmax(v, c, high)
    lse = _lse32(s, mx, 64)
    keep = labels != ignore_index
    return _row_nll32(s, lse, labels, keep, 1 if mutate == "labels_shifted" else 0), col.to(torch.int32)


def emulate_accum(record, nll, pred, labels, ignore_index, mutate=None):
    """eval_accum_kernel: thread t adds rows t, t + 256, ... in double, the LDS tree (128, 64, ..., 1), thread 0 adds to the record"""
    n = int(labels.numel())
    keep = labels != ignore_index
    use = torch.ones_like(keep) if mutate == "ignored_in_loss" else keep
    hit = (pred.to(torch.int64) == labels) & (torch.ones_like(keep) if mutate == "correct_on_ignored" else keep)
    J = cdiv(n, 256)
    x = torch.zeros(J * 256, dtype=F64)
    x[:n] = torch.where(use, nll.to(F64), torch.zeros(n, dtype=F64))
    x = x.reshape(J, 256)
    acc = torch.zeros(256, dtype=F64)
    for j in range(J):
        # a skipped row adds nothing (not even +0.0); adding +0.0 to a double changes no bit but -0.0's sign, which no sum here has
        acc = acc + x[j]
    o = 128
    while o > 0:
        acc = torch.cat([acc[:o] + acc[o:2 * o], acc[o:]])
        o >>= 1
    loss = float(acc[0])
    if mutate == "mean_for_sum":
        loss = loss / max(int(keep.sum()), 1)
    rows = int(keep.sum()) if mutate == "ignored_not_in_rows" else n
    new = (loss, int(hit.sum()), rows, int(keep.sum()))
    if mutate == "overwrite":
        return new
    return (record[0] + new[0], record[1] + new[1], record[2] + new[2], record[3] + new[3])


MUTATIONS = ("tie_high", "argmax_ldv", "mean_for_sum", "ignored_in_loss", "ignored_not_in_rows", "correct_on_ignored", "overwrite",
             "labels_shifted")


# ---- cases -----------------------------------------------------------------------------------------------------------------------
SHIFTS = (0.0, 80.0, -80.0)
PLACES = ("winner", "loser", "elsewhere")
START = (3.25, 7, 11, 9)               # a record that starts non-zero


def tie_pairs(C, stride, k):
    """column pairs that hold the planted double maximum: one thread's two trips, two waves (vocab) / two trips (SAP), two lanes,
    first and last column"""
    pairs = [(k % stride, k % stride + stride), (63, 64), (5, 6), (0, C - 1)]
    return [(a, b) for a, b in pairs if a < b < C]


def plant_ties(s, labels, stride, idx, neginf=True):
    """s [n, C] fp32 (modified in place): on two rows of three, the row maximum twice, the label on the winner (lower column), the
    loser or elsewhere; a -inf column is kept in the row where there is room.  -> the planted rows' (row, a, b, place)"""
    n, C = s.shape
    planted = []
    for r in range(n):
        pairs = tie_pairs(C, stride, 3 + 7 * (idx + r))
        if r % 3 == 2 or not pairs:
            continue
        combo = idx + r
        a, b = pairs[combo % len(pairs)]
        place = PLACES[(combo // len(pairs)) % 3]
        fin = s[r][torch.isfinite(s[r])]
        m = float(fin.max()) + 1.5
        s[r, a] = s[r, b] = m
        if place == "elsewhere" and C >= 3:
            y = next(c for c in range(C) if c not in (a, b))
            s[r, y] = m - 2.0
        else:
            y = b if place == "loser" else a
        labels[r] = y
        if neginf and C > 3:
            s[r, next(c for c in reversed(range(C)) if c not in (a, b, y))] = float("-inf")
        planted.append((r, a, b, place))
    return planted


def vocab_cases():
    """(V, ldv, Nm, shift, special) on move_ref.vce_cases()' shapes; special: None, 'label_neginf' or 'all_neginf' (one row)"""
    shapes = []
    for _, V, ldv, Nm, _ in mv.vce_cases():
        if (V, ldv, Nm) not in shapes:
            shapes.append((V, ldv, Nm))
    out = [(V, ldv, Nm, SHIFTS[i % 3], None) for i, (V, ldv, Nm) in enumerate(shapes)]
    out += [(257, 264, 3, 0.0, "label_neginf"), (257, 273, 3, 0.0, "all_neginf"), (1000, 1000, 1, 80.0, "label_neginf"),
            (63, 64, 1, 0.0, "all_neginf")]
    return out


def vocab_case(V, ldv, Nm, shift, special, idx):
    c = mv.vce_case(V, ldv, Nm, (shift, "mean", 0.0), 1000 + idx)
    buf, labels = c["buf"], c["labels"]
    s = buf[:, :V].clone()
    planted = plant_ties(s, labels, 256, idx)
    r = Nm // 2
    if special == "label_neginf":
        labels[r] = (int(argmax_lowest(s[r:r + 1].to(F64))) + 1) % V
        s[r, labels[r]] = float("-inf")
    elif special == "all_neginf":
        s[r] = float("-inf")
    buf[:, :V] = s
    return {"V": V, "ldv": ldv, "Nm": Nm, "buf": buf, "labels": labels, "planted": planted, "q": tail(s, labels)}


def sap_cases():
    """(B, G, pattern, special) on reduce_ref.ce_cases()"""
    out = [(B, G, p, None) for B, G, p in rf.ce_cases()]
    p = rf.CE_PATTERNS
    out += [(7, 65, p[0], "label_neginf"), (33, 130, p[3], "all_neginf"), (1, 64, p[1], "label_neginf"), (1, 2, p[0], "all_neginf")]
    return out


def sap_case(B, G, pattern, special, idx):
    logits, labels, _, ignore_index = rf.ce_case(B, G, pattern, 2000 + idx)
    keep = labels != ignore_index
    tmp = labels.clone()
    planted = plant_ties(logits, tmp, 64, idx, neginf=False)
    labels = torch.where(keep, tmp, labels)            # ignored rows stay ignored; their arg-max still meets the tie
    r = B // 2
    if special == "label_neginf":
        labels[r] = (int(argmax_lowest(logits[r:r + 1].to(F64))) + 1) % G
        logits[r, labels[r]] = float("-inf")
    elif special == "all_neginf":
        logits[r] = float("-inf")
        if labels[r] == ignore_index:
            labels[r] = 0
    return {"B": B, "G": G, "logits": logits, "labels": labels, "ignore_index": ignore_index, "planted": planted,
            "q": tail(logits, labels, ignore_index)}


ACCUM_N = (1, 255, 256, 257, 1029)


def accum_cases():
    """(n, ignore_index): -100 names no column; 2 is a column, so an ignored row's pred can equal its label"""
    return [(n, ii) for n in ACCUM_N for ii in (-100, 2)]


def accum_case(n, ignore_index, seed):
    """two batches of n rows: nll over many binades (non-zero on the ignored rows too: they must not be added), pred == label on
    about half of the rows, ignored ones included"""
    g = torch.Generator().manual_seed(seed)
    out = []
    for _ in range(2):
        nll = (torch.rand(n, generator=g) * 12) * 2.0 ** torch.randint(-8, 6, (n,), generator=g).float()
        labels = torch.randint(0, 9, (n,), generator=g)
        labels[torch.rand(n, generator=g) < 0.3] = ignore_index
        if n > 1:
            labels[n // 2] = ignore_index
        pred = torch.where(torch.rand(n, generator=g) < 0.5, labels.clamp_min(0), torch.randint(0, 9, (n,), generator=g)).to(torch.int32)
        if ignore_index >= 0 and n > 1:
            pred[n // 2] = ignore_index                  # an ignored row whose pred equals its label
        out.append((nll.to(F32), pred, labels))
    return out


# ---- the validation loaders of the golden fixture ----------------------------------------------------------------------------------
VAL_SEEDS = ((5, 99), (6, 100))        # (batch seed, mask seed): oracle.make_golden_pretrain.make_case() and a second batch


def val_case():
    """-> cfg, P, [batch0, batch1] with the labels the reference saw (before the fixture's label edits)"""
    from oracle import make_golden_pretrain as mg
    from etpnav_amd.synthetic import make_sap_batch
    cfg, P, first = mg.make_case()
    b = mg.CASE["batch"]
    batches = [first]
    for bseed, mseed in VAL_SEEDS[1:]:
        batch = make_sap_batch(cfg.vocab_size, cfg.image_feat_size, cfg.depth_feat_size, b["B"], b["L"], b["T"], b["V"],
                               n_cand=b["n_cand"], seed=bseed, ragged=b["ragged"])
        g = torch.Generator().manual_seed(mseed)
        lab = torch.full_like(batch["txt_ids"], -1)
        pick = (torch.rand(lab.shape, generator=g) < 0.25) & batch["txt_masks"]
        pick[:, 1] = True
        lab[pick] = batch["txt_ids"][pick]
        ids = batch["txt_ids"].clone()
        ids[pick] = 103
        batch["txt_ids"], batch["txt_labels"] = ids, lab
        batches.append(batch)
    return cfg, P, batches


def val_loaders(fixture=None):
    """-> cfg, P, {'mlm': [2 batches], 'sap': [2 batches]} carrying the fixture's edited labels (copies of the two batches: labels do
    not enter the forward)"""
    z = fixture if fixture is not None else np.load(GOLDEN)
    cfg, P, batches = val_case()
    mlm, sap = [], []
    for i, b in enumerate(batches):
        m, s = dict(b), dict(b)
        lab = b["txt_labels"].clone()
        lab[lab != -1] = torch.from_numpy(z[f"mlm/labels/{i}"])
        m["txt_labels"] = lab
        s["labels"] = torch.from_numpy(z[f"sap/labels/{i}"])
        mlm.append(m)
        sap.append(s)
    return cfg, P, {"mlm": mlm, "sap": sap}


def top2_margin(scores):
    t = torch.as_tensor(scores).to(F64).topk(2, dim=-1).values
    return float((t[:, 0] - t[:, 1]).min())
