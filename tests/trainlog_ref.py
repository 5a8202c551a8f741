"""Restatements, case lists, launch geometry and derived bounds for the training log of csrc/trainlog.hip
(tests/test_train_log_gpu.py runs the kernels through the C ABI and the host layer, tests/test_train_log_ref_cpu.py pins, emulates
and mutates the same lists without a GPU, tests/test_train_log_boundary_cpu.py checks the geometry against the library's own).

  Meter        RunningMeter.__call__ (pretrain_src/pretrain_src/utils/logger.py:77-81) on Python floats, with the record's counters.
               Python's float IS the kernel's double, so the comparison is bit for bit.
  f32_root     grad_norm = (float)sqrt((double)sumsq): the correctly rounded fp32 root.
  step_record  the step record's update (etp_train_meter_step).
  report_ref   per-segment sum and sum of squares as the CORRECTLY ROUNDED float64 of the exact values (math.fsum; the square of a
               float is exact in float64), abs-max and non-finite count exactly, and the two magnitudes the bounds scale with.
  geometry     chunks per segment and d, the longest chain of additions any one term of a segment goes through on the device:
                   ceil(n4 / 256) vectors of 4 elements per thread, + 1 for the scalar tail        (n = min(len, 16384), n4 = n // 4)
                   + 6 levels of the wave's shuffle tree + 3 additions over the four waves
                   + ceil(chunks / 64) partials per lane of stage 2 + 6 levels of its tree
  Bounds (u = 2^-53, gam64(k) = k u / (1 - k u), Higham 2002 eq. 4.4: any order of summation whose longest chain is d):
                   |sum - ref| <= gam64(d) sum|x|        |sumsq - ref| <= gam64(d) sum x^2
               with no multiplier; absmax and nonfinite exact.  The reference itself is within u/2 relative of the exact value, which
               is absorbed by counting the accumulator's first addition (to +0, exact) as a rounding: d counts terms, not roundings.
  totals_ref   stage 3 restated in its own order (lane-strided over the included segments, then the xor tree): bit for bit.
  emulate      stages 1 and 2 in numpy in the kernels' order, with planted mutations for the CPU tests.

Nothing below is fitted to what a kernel returns.
"""
import math
import os
import struct

import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "train_log_small.npz")
CHUNK = 16384
U64 = 2.0 ** -53
TASK_FMT, STEP_FMT, TENSOR_FMT = "<ddqqqqqq", "<dddqqqqq", "<ddfiq"
MASK_SHAPES = [(1, 1), (3, 9), (5, 64), (5, 65), (32, 100), (7, 1030)]
SUMSQ_CASES = [0.0, 1.0, 2.0, 1e-38, 3e38, float("inf"), float("nan")]
NONFINITE_CASES = [None, 0, 5]
LENS = [1, 3, 4, 5, 255, 256, 257, 1023, 1025, 16383, 16384, 16385, 2 * 16384, 3 * 16384 + 1, 2 ** 20 + 64]
N_SEGS = [1, 2, 307, 700]


def gam64(k):
    return k * U64 / (1.0 - k * U64)


# ---- the meter -------------------------------------------------------------------------------------------------------------------------
class Meter:
    """RunningMeter of logger.py:68-94 on Python floats plus the counters of etp_train_task_record.  mutate: one planted error of
    tests/test_train_log_ref_cpu.py (None = the kernel's semantics)."""

    def __init__(self, smooth=0.99, mutate=None):
        self.sm, self.mutate = float(smooth), mutate
        self.run = self.last = 0.0
        self.n_values = self.n_skipped = self.n_examples = self.n_in_units = self.n_loss_units = 0

    def __call__(self, value, n_examples=0, n_in_units=0, n_loss_units=0):
        value = float(np.float32(value))                   # the device loss is one fp32; (double)*loss is exact
        sm = float(np.float32(self.sm)) if self.mutate == "smooth_fp32" else self.sm
        first = self.n_values == 0 and self.mutate != "first_against_zero"
        if first:
            val = value
        elif self.mutate == "fma":                         # run*sm kept exact inside the sum: a contracted a*b + c*d, one rounding less
            val = fma_emulated(self.run, sm, value * (1.0 - sm))
        else:
            val = value * (1.0 - sm) + self.run * sm
        skip = math.isnan(value) if self.mutate == "nan_test_on_input" else math.isnan(val)
        if skip:
            self.n_skipped += 1
            if self.mutate == "skip_advances":
                self.n_values += 1
        else:
            self.run = val
            self.n_values += 1
        self.last = value
        self.n_examples += n_examples
        self.n_in_units += n_in_units
        self.n_loss_units += n_loss_units

    @property
    def val(self):
        return self.run if self.n_values > 0 else 0

    def record(self):
        return (self.run, self.last, self.n_values, self.n_skipped, self.n_examples, self.n_in_units, self.n_loss_units, 0)


def fma_emulated(a, b, c):
    """round(a*b + c) with the product kept exact (fractions): what a contracted multiply-add would give"""
    from fractions import Fraction
    if not all(map(math.isfinite, (a, b, c))):
        return a * b + c
    return float(Fraction(a) * Fraction(b) + Fraction(c))


def bits64(x):
    return struct.unpack("<q", struct.pack("<d", float(x)))[0]


def same_record(a, b):
    """two task / step records bit for bit (NaN payloads included)"""
    return len(a) == len(b) and all((bits64(x) == bits64(y)) if isinstance(x, float) or isinstance(y, float) else int(x) == int(y)
                                    for x, y in zip(a, b))


# ---- the step record -------------------------------------------------------------------------------------------------------------------
def f32_root(sumsq, mutate=None):
    """(float)sqrt((double)sumsq) of one fp32 value, as a Python float holding an fp32 value"""
    s = float(np.float32(sumsq))
    if mutate == "no_root":
        return float(np.float32(s))
    with np.errstate(invalid="ignore", over="ignore"):
        return float(np.float32(np.sqrt(np.float64(s))))


STEP_START = (0.0, 0.0, 0.0, 0, 0, -1, 0, 0)


def step_record(rec, sumsq, nonfinite, mutate=None):
    last, mx, sm, n, nbad, first, r0, r1 = rec
    gn = f32_root(sumsq, mutate)
    n += 1
    if math.isfinite(gn) and not nonfinite:
        mx, sm = max(mx, gn), sm + gn
    else:
        nbad += 1
        first = n if first < 0 else first
    return (gn, mx, sm, n, nbad, first, r0, r1)


# ---- the report: geometry ----------------------------------------------------------------------------------------------------------------
def cdiv(a, b):
    return -(-a // b)


def seg_chunks(length):
    return cdiv(length, CHUNK)


def total_chunks(lens):
    return sum(seg_chunks(n) for n in lens)


def depth(length):
    """d of the module docstring for a segment of `length` elements"""
    chain = lambda n: cdiv(n // 4, 256) * 4 + (1 if n % 4 else 0)          # thread 0: the most vectors, and the tail
    last = length - (seg_chunks(length) - 1) * CHUNK
    return max(chain(min(length, CHUNK)), chain(last)) + 6 + 3 + cdiv(seg_chunks(length), 64) + 6


def depth_total(n_seg):
    return cdiv(n_seg, 64) + 6


# ---- the report: tables and data of the GPU list -----------------------------------------------------------------------------------------
GAP = [float("nan"), 3e38, -3e38]


def report_tables():
    """-> [(off, lens, include)]: one table per n_seg of N_SEGS, lengths drawn from LENS (every length is used; the longest ones once),
    offsets multiples of 4 with at least one gap element on either side of every segment"""
    out = []
    small = [n for n in LENS if n <= 1025]
    for t, n_seg in enumerate(N_SEGS):
        rng = np.random.RandomState(100 + t)
        if n_seg == 1:
            lens = [2 ** 20 + 64]
        elif n_seg == 2:
            lens = [3 * 16384 + 1, 5]
        else:
            lens = [small[i] for i in rng.randint(0, len(small), n_seg)]
            fixed = LENS if n_seg == 307 else [16385, 1, 2 * 16384, 3]
            for k, n in zip(np.linspace(0, n_seg - 1, len(fixed)).astype(int), fixed):      # first and last positions included
                lens[k] = n
            lens[2], lens[5] = 1023, 1025                # the cancelling triples; a scalar tail for the planted -inf
        off, pos = [], 4
        for i, n in enumerate(lens):
            off.append(pos)
            pos = (pos + n + 1 + 3) // 4 * 4 + (0, 4, 64)[i % 3]
        include = [1] * n_seg if n_seg < 3 else [int(b) for b in (rng.rand(n_seg) < 0.7)]
        if n_seg == 2:
            include = [0, 1]                             # the long segment stays out of the totals
        out.append((off, lens, include))
    return out


def arena_len(off, lens):
    return off[-1] + lens[-1] + 4


def report_case(t):
    """table t of report_tables() with its arena: gaps hold NaN / +3e38 / -3e38, values carry row scales 2^-20 .. 2^20 (rows of 64
    elements); segment 1 (where there is one) is all zeros, segment 2 has every third sum cancelling to 2^-10 of its terms, and
    non-finite values sit first (segment 3), last (segment 4) and in the scalar tail (segment 5, or the only segment)."""
    off, lens, include = report_tables()[t]
    rng = np.random.RandomState(7 + t)
    A = arena_len(off, lens)
    arena = np.array([GAP[i % 3] for i in range(min(A, 3 * 4096))], dtype=np.float32)
    arena = np.resize(arena, A)
    n_seg = len(off)
    for s, (o, n) in enumerate(zip(off, lens)):
        x = rng.standard_normal(n).astype(np.float32)
        scale = 2.0 ** rng.randint(-20, 21, cdiv(n, 64)).astype(np.float64)
        x = (x * np.repeat(scale, 64)[:n]).astype(np.float32)
        if n_seg > 5 and s == 1:
            x[:] = 0.0
        if (n_seg > 5 and s == 2) or (n_seg == 2 and s == 0):
            k = n // 3
            a, b = x[0:3 * k:3].astype(np.float64), x[1:3 * k:3].astype(np.float64)
            x[2:3 * k:3] = (-(a + b) * (1.0 - 2.0 ** -10)).astype(np.float32)
        if n_seg > 5 and s == 3:
            x[0] = np.nan
        if n_seg > 5 and s == 4:
            x[-1] = np.inf
        if (n_seg > 5 and s == 5) or n_seg == 1:
            if n % 4:
                x[4 * (n // 4)] = -np.inf
            else:
                x[n - 1] = -np.inf
                x[n // 2] = np.nan
        arena[o:o + n] = x
    return arena, off, lens, include


def seg_ref(x):
    """one segment's reference: (sum, sumsq, absmax, nonfinite, sum|x|, sum x^2 as a float) -- fsum: correctly rounded"""
    x = np.asarray(x, dtype=np.float32)
    fin = np.isfinite(x)
    v = x[fin].astype(np.float64)
    sq = v * v
    return (math.fsum(v.tolist()), math.fsum(sq.tolist()), float(np.max(np.abs(x[fin]))) if v.size else 0.0, int((~fin).sum()),
            math.fsum(np.abs(v).tolist()), math.fsum(sq.tolist()))


def report_ref(arena, off, lens):
    return [seg_ref(arena[o:o + n]) for o, n in zip(off, lens)]


def assert_gaps_would_show(arena, off, lens, ref=None):
    """on the reference alone: reading one element on either side of any segment changes nonfinite or absmax"""
    ref = ref if ref is not None else report_ref(arena, off, lens)
    for s, (o, n) in enumerate(zip(off, lens)):
        for lo, hi in ((o - 1, o + n), (o, o + n + 1)):
            g = arena[lo] if lo < o else arena[hi - 1]
            changed = (not np.isfinite(g)) or abs(float(g)) > ref[s][2]
            assert changed, (s, lo, hi, float(g), ref[s][2])


def check_report(name, got, ref, lens):
    """got: [(sum, sumsq, absmax, nonfinite)] per segment against report_ref's rows; -> the worst err / bound"""
    worst = 0.0
    for s, (g, r, n) in enumerate(zip(got, ref, lens)):
        assert g[3] == r[3], f"{name}: segment {s} (len {n}): nonfinite {g[3]}, reference {r[3]}"
        assert struct.pack("<f", g[2]) == struct.pack("<f", r[2]), f"{name}: segment {s} (len {n}): absmax {g[2]!r}, reference {r[2]!r}"
        d = depth(n)
        for what, gv, rv, mag in (("sum", g[0], r[0], r[4]), ("sumsq", g[1], r[1], r[5])):
            err, bound = abs(gv - rv), gam64(d) * mag
            assert err <= bound, f"{name}: segment {s} (len {n}, d {d}): {what} {gv!r}, reference {rv!r}: err {err:.3e} > bound {bound:.3e}"
            if bound > 0:
                worst = max(worst, err / bound)
    return worst


def xor_tree(v):
    """the wave's shuffle tree on 64 values: v[l] += v[l ^ o] for o = 32 .. 1, all lanes at once; -> lane 0's value"""
    v = np.array(v)
    idx = np.arange(64)
    for o in (32, 16, 8, 4, 2, 1):
        v = v + v[idx ^ o]
    return v[0]


def totals_ref(sumsq, nonfinite, include, mutate=None):
    """stage 3 from the records' own sumsq / nonfinite: -> (the fp32 total as a Python float, or NaN; the int total)"""
    lanes, nf = np.zeros(64, dtype=np.float64), 0
    for s, (q, b, inc) in enumerate(zip(sumsq, nonfinite, include)):
        if inc or mutate == "include_ignored":
            lanes[s % 64] += q
            nf += int(b)
    tot = xor_tree(lanes)
    with np.errstate(over="ignore"):
        return (float("nan") if nf else float(np.float32(tot))), nf


# ---- the report: stages 1 and 2 in the kernels' order --------------------------------------------------------------------------------------
def _chunk_partial(x, mutate):
    n = len(x)
    n4 = n // 4
    fin = np.isfinite(x)
    take = np.ones(n, dtype=bool) if mutate == "nonfinite_in_sum" else fin
    with np.errstate(invalid="ignore", over="ignore"):
        v = np.where(take, x, np.float32(0)).astype(np.float64)
        a = np.where(fin, x if mutate == "absmax_signed" else np.abs(x), np.float32(0)).astype(np.float32)
        iters = cdiv(n4, 256)
        pad = lambda z, fill: np.concatenate([z[:4 * n4], np.full(iters * 1024 - 4 * n4, fill, dtype=z.dtype)]).reshape(iters, 256, 4)
        V, Q, Am, Nf = pad(v, 0.0), pad(v * v, 0.0), pad(a, np.float32(0)), pad((~fin).astype(np.int64), 0)
        sm, sq = np.zeros(256), np.zeros(256)
        for i in range(iters):
            for e in range(4):
                sm = sm + V[i, :, e]
                sq = sq + Q[i, :, e]
        am = Am.max(axis=(0, 2)) if iters else np.zeros(256, dtype=np.float32)
        am = np.maximum(am, np.float32(0))
        nf = Nf.sum(axis=(0, 2)) if iters else np.zeros(256, dtype=np.int64)
        if mutate != "tail_dropped":
            for t in range(n - 4 * n4):
                sm[t] += v[4 * n4 + t]
                sq[t] += v[4 * n4 + t] ** 2
                am[t] = max(am[t], a[4 * n4 + t])
                nf[t] += int(not fin[4 * n4 + t])
        w_sm = [xor_tree(sm[w * 64:(w + 1) * 64]) for w in range(4)]
        w_sq = [xor_tree(sq[w * 64:(w + 1) * 64]) for w in range(4)]
        return (((w_sm[0] + w_sm[1]) + w_sm[2]) + w_sm[3], ((w_sq[0] + w_sq[1]) + w_sq[2]) + w_sq[3], float(am.max()), int(nf.sum()))


def emulate(arena, off, lens, mutate=None):
    """-> [(sum, sumsq, absmax, nonfinite)] per segment, stages 1 and 2 in the kernels' order.  mutate: 'chunk_crosses' (a segment's last
    chunk reads one element of the gap behind it), 'tail_dropped', 'nonfinite_in_sum', 'absmax_signed'."""
    out = []
    for o, n in zip(off, lens):
        parts = []
        for c in range(seg_chunks(n)):
            lo = o + c * CHUNK
            hi = min(lo + CHUNK, o + n)
            if mutate == "chunk_crosses" and hi == o + n:
                hi += 1                                  # the segment's last chunk runs one element into the gap
            parts.append(_chunk_partial(arena[lo:hi], mutate))
        lanes_s, lanes_q = np.zeros(64), np.zeros(64)
        with np.errstate(invalid="ignore", over="ignore"):
            for c, p in enumerate(parts):
                lanes_s[c % 64] += p[0]
                lanes_q[c % 64] += p[1]
            out.append((float(xor_tree(lanes_s)), float(xor_tree(lanes_q)), max(p[2] for p in parts), sum(p[3] for p in parts)))
    return out
