"""Op-level tests of the MLM loss tail and the data-movement kernels through the C ABI, against the fp64 restatements, derived bounds
and case lists of tests/move_ref.py (tests/test_move_ref_cpu.py pins, emulates and mutates the same lists on the CPU):

  etp_vocab_ce        vocab_ce_kernel<T>        loss within its bound (atomics), dlogits elementwise, padding / -inf columns exactly 0
  etp_gelu_bwd        gelu_bwd_kernel<T>        in place; z read only; NaN exactly where z = +-inf
  etp_sum_steps       sum_steps_kernel<T>       steps = 1 bit for bit
  etp_repeat_block, etp_copy_f32, etp_memset_async (three branches), etp_cast_f32_to, etp_seq_mask, etp_vp_gather     bit for bit

Every output starts as a payload NaN (0xFF for bytes) inside a guarded buffer whose guards must survive bit for bit, every read-only
input is compared with its copy afterwards, and a second run must be bit-identical (for etp_vocab_ce: dlogits; its loss goes through
atomics and is held to its bound twice).  Refused calls return ETP_ERR_INVALID and leave the fill intact.

After its last test the module prints the worst err / bound per (entry point, tensor) and the differing elements of the exact kernels,
and writes the table to profiles/move_op_bounds.txt (the committed file is the MI355X run's).  That run: 245 tests in 4.9 s wall time
(pytest's own figure, case construction and fp64 references included); worst err / bound 1.000 for etp_sum_steps (fp32, steps = 2: one
rounding of a sum just above a power of two IS the bound; bf16: a round-to-nearest tie is exactly the half ulp), 0.999 / 0.680 for
etp_vocab_ce's bf16 / fp32 dlogits, 0.415 / 0.394 for its loss, 0.995 / 0.009 for etp_gelu_bwd bf16 / fp32; 0 differing elements in
every exact comparison.
"""
import os
import time

import pytest
import torch

pytestmark = pytest.mark.gpu

from etpnav_amd import _lib  # noqa: E402
from etpnav_amd._lib import check, ptr  # noqa: E402
from tests import move_ref as mv  # noqa: E402

DEV = "cuda"
TDT = mv.TDT
EDT = {"fp32": _lib.ETP_F32, "bf16": _lib.ETP_BF16}
INVALID = -1
gptr, guarded = mv.gptr, mv.guarded


def L():
    return _lib.lib()


def stream():
    return torch.cuda.current_stream().cuda_stream


def sync():
    torch.cuda.synchronize()


def ids(cases):
    return ["-".join(str(v) for v in c).replace(" ", "") for c in cases]


@pytest.fixture(scope="module", autouse=True)
def report():
    t0 = time.time()
    yield
    text = ("data movement and MLM tail, worst err / bound per (entry point, tensor) and differing elements of the exact kernels\n"
            f"(tests/test_move_kernels_gpu.py on {torch.cuda.get_device_name(0)}, {time.time() - t0:.1f} s)\n" + mv.table() + "\n")
    print("\n" + text)
    try:
        with open(os.path.join(_lib.ROOT, "profiles", "move_op_bounds.txt"), "w") as f:
            f.write(text)
    except OSError:                                                     # a read-only checkout keeps the committed table
        pass


# ---- etp_vocab_ce --------------------------------------------------------------------------------------------------------------
VCE = mv.vce_cases()


@pytest.mark.parametrize("i", range(len(VCE)), ids=ids(VCE))
def test_vocab_ce(i):
    dt, V, ldv, Nm, pat = VCE[i]
    c = mv.vce_reference(mv.vce_case(V, ldv, Nm, pat, seed=i, device=DEV), dt == "bf16")
    buf0, labels0 = c["buf"].clone(), c["labels"].clone()
    start = torch.tensor([c["start"]], device=DEV)
    runs = []
    for _ in range(2):
        loss, dl = guarded((1,), init=start), guarded((Nm, ldv), TDT[dt])
        check(L().etp_vocab_ce(EDT[dt], ptr(c["buf"]), ptr(c["labels"]), gptr(loss), gptr(dl), Nm, V, ldv, c["scale"], stream()), "vocab_ce")
        sync()
        loss.check("vocab_ce loss")
        dl.check("vocab_ce dlogits")
        mv.check_vce("etp_vocab_ce " + dt, c, loss.t, dl.t)
        runs.append(dl)
    mv.exact("etp_vocab_ce dlogits (second run)", runs[0].t, runs[1].t)
    mv.exact("etp_vocab_ce logits (read only)", c["buf"], buf0)
    mv.exact("etp_vocab_ce labels (read only)", c["labels"], labels0)


# ---- etp_gelu_bwd --------------------------------------------------------------------------------------------------------------
GELU = mv.gelu_cases()


@pytest.mark.parametrize("i", range(len(GELU)), ids=ids(GELU))
def test_gelu_bwd(i):
    dt, n = GELU[i]
    d0, z = mv.gelu_case(n, TDT[dt], seed=i, device=DEV)
    z0 = z.clone()
    runs = []
    for _ in range(2):
        d = guarded((n,), TDT[dt], init=d0)
        check(L().etp_gelu_bwd(EDT[dt], gptr(d), ptr(z), n, stream()), "gelu_bwd")
        sync()
        d.check("gelu_bwd d")
        mv.check_gelu("etp_gelu_bwd " + dt, d.t, d0, z0)
        runs.append(d)
    finite = ~torch.isinf(z0.float())                                   # (a NaN's payload is not part of the contract)
    mv.exact("etp_gelu_bwd d (second run)", runs[0].t[finite], runs[1].t[finite])
    mv.exact("etp_gelu_bwd z (read only)", z, z0)


# ---- etp_sum_steps -------------------------------------------------------------------------------------------------------------
SUM = mv.sum_cases()


@pytest.mark.parametrize("i", range(len(SUM)), ids=ids(SUM))
def test_sum_steps(i):
    dt, n, steps = SUM[i]
    src = mv.sum_case(n, steps, TDT[dt], seed=i, device=DEV)
    src0 = src.clone()
    runs = []
    for _ in range(2):
        dst = guarded((n,), TDT[dt])
        check(L().etp_sum_steps(EDT[dt], ptr(src), gptr(dst), n, steps, stream()), "sum_steps")
        sync()
        dst.check("sum_steps dst")
        runs.append(dst)
    mv.check_sum("etp_sum_steps " + dt, dst.t, src0)
    mv.exact("etp_sum_steps dst (second run)", runs[0].t, runs[1].t)
    mv.exact("etp_sum_steps src (read only)", src, src0)


# ---- etp_repeat_block ----------------------------------------------------------------------------------------------------------
REPEAT = [(b, T) for b in mv.REPEAT_BYTES for T in mv.REPEAT_T]


@pytest.mark.parametrize("case", REPEAT, ids=ids(REPEAT))
def test_repeat_block(case):
    nbytes, T = case
    src = mv.random_bytes(nbytes, seed=nbytes + T, device=DEV)
    src0 = src.clone()
    runs = []
    for _ in range(2):
        dst = guarded((nbytes * T,), torch.uint8)
        check(L().etp_repeat_block(ptr(src), gptr(dst), nbytes, T, stream()), "repeat_block")
        sync()
        dst.check("repeat_block dst")
        mv.exact("etp_repeat_block", dst.t, mv.repeat_block(src0, T))
        runs.append(dst)
    mv.exact("etp_repeat_block (second run)", runs[0].t, runs[1].t)
    mv.exact("etp_repeat_block src (read only)", src, src0)


# ---- etp_copy_f32 --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", mv.COPY_N)
def test_copy_f32(n):
    src = mv.random_f32(n, seed=n, device=DEV)
    src0 = src.clone()
    runs = []
    for _ in range(2):
        dst = guarded((n,))
        check(L().etp_copy_f32(ptr(src), gptr(dst), n, stream()), "copy_f32")
        sync()
        dst.check("copy_f32 dst")
        mv.exact("etp_copy_f32", dst.t, src0)
        runs.append(dst)
    mv.exact("etp_copy_f32 (second run)", runs[0].t, runs[1].t)
    mv.exact("etp_copy_f32 src (read only)", src, src0)
    same = guarded((n,))
    check(L().etp_copy_f32(gptr(same), gptr(same), n, stream()), "copy_f32 onto itself")
    sync()
    same.intact("etp_copy_f32 src == dst")


# ---- etp_memset_async: the zeroing kernel, the runtime's memset for what the kernel cannot take, a non-zero value ------------------
@pytest.mark.parametrize("n", mv.ZERO_N)
def test_memset_zero_kernel_path(n):
    """value 0, 16-byte aligned, bytes % 4 == 0: zero_f32_kernel"""
    runs = []
    for _ in range(2):
        dst = guarded((n,))
        p = dst.buf.data_ptr() + 4 * mv.rf.GUARD                        # (an empty view has no address of its own)
        assert p % 16 == 0 and (n == 0 or p == dst.t.data_ptr())
        check(L().etp_memset_async(p, 0, 4 * n, stream()), "memset (kernel path)")
        sync()
        dst.check("memset dst")
        mv.exact("etp_memset_async value 0, aligned (zero_f32)", dst.t, torch.zeros(n, device=DEV))
        runs.append(dst)
    mv.exact("etp_memset_async value 0, aligned (second run)", runs[0].t, runs[1].t)


@pytest.mark.parametrize("n", (5, 1027, 4 * 4096 + 3))
def test_memset_other_branches(n):
    odd = guarded((n,), torch.uint8)                                    # value 0, bytes % 4 != 0
    assert n % 4 != 0
    check(L().etp_memset_async(gptr(odd), 0, n, stream()), "memset (odd byte count)")
    off = guarded((n,))                                                 # value 0, pointer 4 bytes off a 16-byte boundary
    check(L().etp_memset_async(off.t[1:].data_ptr(), 0, 4 * (n - 1), stream()), "memset (pointer offset by 4)")
    val = guarded((4 * n,), torch.uint8)                                # value 0xA5, aligned, bytes % 4 == 0
    check(L().etp_memset_async(gptr(val), 0xA5, 4 * n, stream()), "memset (value 0xA5)")
    sync()
    for g, name in ((odd, "odd"), (off, "offset"), (val, "value")):
        g.check("memset " + name)
    mv.exact("etp_memset_async value 0, bytes % 4 != 0", odd.t, torch.zeros(n, dtype=torch.uint8, device=DEV))
    want = torch.zeros(n, device=DEV)
    want[:1] = mv.payload((1,), torch.float32, DEV)
    mv.exact("etp_memset_async value 0, pointer offset by 4", off.t, want)
    mv.exact("etp_memset_async value 0xA5", val.t, torch.full((4 * n,), 0xA5, dtype=torch.uint8, device=DEV))


# ---- etp_cast_f32_to -----------------------------------------------------------------------------------------------------------
CASTTO = [(dt, n) for n in mv.CASTTO_N for dt in ("fp32", "bf16")]


@pytest.mark.parametrize("case", CASTTO, ids=ids(CASTTO))
def test_cast_f32_to(case):
    dt, n = case
    src = mv.random_f32(n, seed=n + 1, device=DEV)
    src0 = src.clone()
    runs = []
    for _ in range(2):
        dst = guarded((n,), TDT[dt])
        check(L().etp_cast_f32_to(EDT[dt], ptr(src), gptr(dst), n, stream()), "cast_f32_to")
        sync()
        dst.check("cast_f32_to dst")
        mv.check_cast_to("etp_cast_f32_to", dst.t, src0)
        runs.append(dst)
    keep = ~torch.isnan(src0)
    mv.exact("etp_cast_f32_to (second run)", runs[0].t[keep], runs[1].t[keep])
    mv.exact("etp_cast_f32_to src (read only)", src, src0)


# ---- etp_seq_mask --------------------------------------------------------------------------------------------------------------
SEQ = [(B, V, two) for (B, V) in mv.SEQ_SHAPES for two in (0, 1)]


@pytest.mark.parametrize("case", SEQ, ids=ids(SEQ))
def test_seq_mask(case):
    B, V, two = case
    lens = mv.seq_lens(B, V, seed=mv.SEQ_SHAPES.index((B, V))).to(DEV)
    lens0 = lens.clone()
    want = mv.seq_mask(lens0, V)
    runs = []
    for _ in range(2):
        m1, m2 = guarded((B, V), torch.uint8), guarded((B, V), torch.uint8) if two else None
        check(L().etp_seq_mask(ptr(lens), gptr(m1), gptr(m2), B, V, stream()), "seq_mask")
        sync()
        for g in (m1, m2):
            if g is not None:
                g.check("seq_mask")
                mv.exact("etp_seq_mask", g.t, want)
        runs.append(m1)
    mv.exact("etp_seq_mask (second run)", runs[0].t, runs[1].t)
    mv.exact("etp_seq_mask lens (read only)", lens, lens0)


# ---- etp_vp_gather -------------------------------------------------------------------------------------------------------------
VP = mv.vp_cases()


@pytest.mark.parametrize("i", range(len(VP)), ids=ids(VP))
def test_vp_gather(i):
    case = VP[i]
    c = mv.vp_case(case, seed=i, device=DEV)
    B, P, F, V = c["B"], c["P"], c["F"], c["V"]
    keep = {k: c[k].clone() for k in ("cand", "cand_ptr", "pano", "mask") if c[k] is not None}
    want = mv.vp_gather(c["cand"], c["cand_ptr"], c["pano"], c["mask"], V)
    runs = []
    for _ in range(2):
        out = guarded((B, V, F))
        gn, nav = mv.guarded_i64((B, V)) if case[7] else (None, None)
        gl, lens = mv.guarded_i64((B,)) if case[7] else (None, None)
        check(L().etp_vp_gather(ptr(c["cand"]), ptr(c["cand_ptr"]), ptr(c["pano"]), c["stride"], ptr(c["mask"]), B, P, F, V, gptr(out),
                                gptr(gn), gptr(gl), stream()), "vp_gather")
        sync()
        for g in (out, gn, gl):
            if g is not None:
                g.check("vp_gather")
        mv.check_vp("etp_vp_gather", out.t, nav, lens, want)
        runs.append(out)
    mv.exact("etp_vp_gather (second run)", runs[0].t, runs[1].t)
    for k, v in keep.items():
        mv.exact(f"etp_vp_gather {k} (read only)", c[k], v)


# ---- refusals ------------------------------------------------------------------------------------------------------------------
def test_refusals_launch_nothing():
    """NULL pointers, ldv < V, n % 4 != 0, steps <= 0, bytes % 16 != 0 and misaligned pointers: ETP_ERR_INVALID from the host-side
    checks, every output still holding its fill"""
    f, b, s = _lib.ETP_F32, _lib.ETP_BF16, stream()
    n = 64
    src = torch.randn(2 * n + 4, device=DEV)
    lp_src = src.to(torch.bfloat16)
    labels = torch.zeros(4, dtype=torch.int64, device=DEV)
    lens = torch.ones(4, dtype=torch.int64, device=DEV)
    out, lp, loss = guarded((2 * n + 4,)), guarded((2 * n + 4,), torch.bfloat16), guarded((1,))
    by = guarded((16 * n,), torch.uint8)
    o, o1, s1 = gptr(out), out.t[1:].data_ptr(), src[1:].data_ptr()       # o1 / s1: 4 bytes off a 16-byte boundary
    lp8 = lp.t[4:].data_ptr()                                               # bf16: 8 bytes off
    X = L()
    calls = [
        X.etp_vocab_ce(f, None, ptr(labels), gptr(loss), o, 4, 8, 8, 1.0, s),
        X.etp_vocab_ce(f, ptr(src), None, gptr(loss), o, 4, 8, 8, 1.0, s),
        X.etp_vocab_ce(f, ptr(src), ptr(labels), None, o, 4, 8, 8, 1.0, s),
        X.etp_vocab_ce(f, ptr(src), ptr(labels), gptr(loss), None, 4, 8, 8, 1.0, s),
        X.etp_vocab_ce(f, ptr(src), ptr(labels), gptr(loss), o, 4, 9, 8, 1.0, s),          # ldv < V
        X.etp_vocab_ce(b, ptr(src), ptr(labels), gptr(loss), gptr(lp), 4, 17, 16, 1.0, s),
        X.etp_vocab_ce(f, ptr(src), ptr(labels), gptr(loss), o, 0, 8, 8, 1.0, s),
        X.etp_gelu_bwd(f, None, ptr(src), n, s),
        X.etp_gelu_bwd(f, o, None, n, s),
        X.etp_sum_steps(f, None, o, n, 2, s),
        X.etp_sum_steps(f, ptr(src), None, n, 2, s),
        X.etp_sum_steps(f, ptr(src), o, n - 2, 2, s),                                      # n % 4 != 0
        X.etp_sum_steps(b, ptr(lp_src), gptr(lp), n - 1, 2, s),
        X.etp_sum_steps(f, ptr(src), o, n, 0, s),                                          # steps <= 0
        X.etp_sum_steps(f, ptr(src), o, n, -1, s),
        X.etp_sum_steps(f, s1, o, n, 2, s),                                                # misaligned
        X.etp_sum_steps(f, ptr(src), o1, n, 2, s),
        X.etp_sum_steps(b, ptr(lp_src), lp8, n, 2, s),
        X.etp_repeat_block(None, gptr(by), 64, 2, s),
        X.etp_repeat_block(ptr(src), None, 64, 2, s),
        X.etp_repeat_block(ptr(src), gptr(by), 40, 2, s),                                  # bytes % 16 != 0
        X.etp_repeat_block(s1, gptr(by), 64, 2, s),
        X.etp_repeat_block(ptr(src), by.t[8:].data_ptr(), 64, 2, s),
        X.etp_copy_f32(None, o, n, s),
        X.etp_copy_f32(ptr(src), None, n, s),
        X.etp_copy_f32(s1, o, n, s),
        X.etp_copy_f32(ptr(src), o1, n, s),
        X.etp_cast_f32_to(f, None, o, n, s),
        X.etp_cast_f32_to(b, ptr(src), None, n, s),
        X.etp_cast_f32_to(b, ptr(src), gptr(lp), n - 3, s),                                # n % 4 != 0
        X.etp_cast_f32_to(f, ptr(src), o, n + 1, s),
        X.etp_cast_f32_to(f, s1, o, n, s),
        X.etp_cast_f32_to(b, ptr(src), lp8, n, s),
        X.etp_seq_mask(None, gptr(by), None, 4, 8, s),
        X.etp_seq_mask(ptr(lens), None, gptr(by), 4, 8, s),
        X.etp_seq_mask(ptr(lens), gptr(by), None, 0, 8, s),
        X.etp_memset_async(None, 0, 16, s),
        X.etp_memset_async(gptr(by), 0, -4, s),
    ]
    sync()
    assert calls == [INVALID] * len(calls), calls
    for g, name in ((out, "fp32 output"), (lp, "bf16 output"), (loss, "loss"), (by, "byte output")):
        g.intact("refused call, " + name)
