"""Every GEMM kernel instance of etp_gemm / etp_gemm_group (csrc/gemm.hip, csrc/gemm_mm32.hip) on the MI355X against the fp64
restatement of tests/gemm_ref.py, element by element under its derived bound -- and ASSERTED BY NAME: every launch is bracketed with
the per-launch profiler (etpnav_amd._lib.profiled) and the case states which instance it expects, e.g. `gemm_dma<bf16,f32,NT,64x64,s3>`.
A dispatch threshold that moves a case to another kernel fails the case.

Every case: outputs NaN-filled (or random under out_mode 1 / 2), C / Z / a_colsum inside buffers of sentinels whose guard rows and
guard columns (columns N .. ldc - 1 included) must be intact afterwards, a second run bit-identical (except out_mode 2: atomics).  Operands carry
row scales 2^-10 .. 2^3 and one exactly-zero row each (gemm_ref.make_operands): the bound is elementwise, so the small rows are
checked as tightly as the large ones.  Reference sites: every nn.Linear / torch.matmul of
vlnce_baselines/models/etp/vilmodel_cmt.py and their autograd (include/etpnav_hip.h, etp_gemm_desc).

Contract cases that failed on the library before the vectorised epilogue required N % 8 == 0 and before split / batched products
refused R, Z and activations: test_ragged_n_leaves_pad_columns_alone (pad columns N .. round_up(N, 8) - 1 of C and Z were written) and the
"ksplit 2 / batch 2 with R / Z / act" entries of test_refusals (such calls were accepted and launched).
Epilogue dropout: tests/test_drop_gemm_gpu.py (etp_gemm_drop)."""
import ctypes
import functools
import itertools

import pytest
import torch

pytestmark = pytest.mark.gpu

from etpnav_amd import _lib  # noqa: E402
from etpnav_amd._lib import GemmDesc  # noqa: E402
from tests import gemm_ref as gr  # noqa: E402

DEV = "cuda"
BF, F32 = _lib.ETP_BF16, _lib.ETP_F32
NAN = float("nan")
STOR = gr.STOR                                        # (trans_a, trans_b): NT, NN, TN
assert (gr.ACT_GELU, gr.ACT_RELU, gr.ACT_GELU_BWD, gr.ACT_RELU_BWD, gr.ACT_GELU_SAVEGRAD, gr.ACT_MUL_Z) == \
    (_lib.ACT_GELU, _lib.ACT_RELU, _lib.ACT_GELU_BWD, _lib.ACT_RELU_BWD, _lib.ACT_GELU_SAVEGRAD, _lib.ACT_MUL_Z)


def L():
    return _lib.lib()


@pytest.fixture(scope="module", autouse=True)
def report_worst_ratios():
    """after the file's last test: the worst |got - ref| / bound per (instance, tensor) of this run (`pytest -s` shows it;
    profiles/gemm_op_bounds.txt is this table from the MI355X).  <instance>/acc: the plain fp32-C cases alone, i.e. the accumulation term."""
    yield
    print()
    for key, (w, _) in sorted(gr.WORST.items()):
        print(f"{w:8.4f}  {key}")


def stream():
    return torch.cuda.current_stream().cuda_stream


def rup(x, m):
    return (x + m - 1) // m * m


inst = gr.inst


def set_opts(etp_opt, opts):
    for k in ("GEMM_TILE", "MM32", "MM32_GROUP", "GROUP_TILE", "GEMM_XCD", "MM32_K2", "GEMM_WIDE", "GEMM_SMALL"):
        etp_opt(k, opts.get(k))


# ---- operands on the device -----------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=64)
def operands(M, N, K, bf16, seed):
    A, B, _, _ = gr.make_operands(M, N, K, bf16, seed)
    return A.to(DEV), B.to(DEV)


def store(X, trans, bf16):
    """logical [rows, K] values -> the stored operand (a [rows, ld] or [K, ld] buffer whose ld exceeds the extent by one 16-byte
    chunk, the excess holding 3.0) and ld"""
    t = torch.bfloat16 if bf16 else torch.float32
    epc = 8 if bf16 else 4
    rows, K = X.shape
    if trans:
        ld = rup(rows, epc) + epc
        buf = torch.full((max(K, 1), ld), 3.0, device=DEV, dtype=t)
        buf[:K, :rows] = X.t().to(t)
    else:
        ld = rup(K, epc) + epc
        buf = torch.full((rows, ld), 3.0, device=DEV, dtype=t)
        buf[:, :K] = X.to(t)
    return buf, ld


def out_layout(N, ld):
    """leading dimension and first column of an output inside its guard buffer: 'pad' = 16-byte aligned rows with 64 spare columns
    (the vectorised epilogue when N % 8 == 0), 'odd' = an odd leading dimension and an unaligned base (the scalar epilogue)"""
    if ld == "pad":
        return rup(N, 8) + 64, 8
    assert ld == "odd"
    return rup(N, 8) + 61, 3


def z_dtype(act, bf16):
    if not bf16:
        return torch.float32
    return torch.float16 if act in (gr.ACT_GELU_SAVEGRAD, gr.ACT_MUL_Z) else torch.bfloat16


def asked(descs, n):
    """etp_gemm_instance: the name the host-side query gives for what is about to be launched"""
    buf = ctypes.create_string_buffer(96)
    rc = L().etp_gemm_instance(descs, n, buf, 96)
    return buf.value.decode() if rc >= 0 else (rc, L().etp_last_error())


def launch(d, expect, what):
    assert asked(ctypes.byref(d), 1) == expect, f"{what}: etp_gemm_instance names {asked(ctypes.byref(d), 1)}"
    with _lib.profiled() as p:
        rc = L().etp_gemm(ctypes.byref(d), stream())
        torch.cuda.synchronize()
    assert rc == 0, (what, rc, L().etp_last_error())
    assert p.launches == {expect: 1}, f"{what}: expected one launch of {expect}, the library ran {p.launches}"


def run_case(expect, M, N, K, ta, tb, bf16, c_bf16, alpha=1.0, bias=False, R=False, act=0, out_mode=0, ksplit=1, ld="pad",
             colsum=False, seed=0, rerun=True):
    """one product through etp_gemm: name, values under the bound, guards, second run.  -> the C it left (a copy)"""
    what = f"{expect} {M}x{N}x{K} alpha {alpha} bias {bias} R {R} act {act} out_mode {out_mode} ksplit {ksplit} ld {ld} colsum {colsum}"
    alpha = gr.f32(alpha)
    listed(M, N, K, bf16)
    A, B = operands(M, N, K, bf16, seed)
    ep = {k: (None if v is None else v.to(DEV)) for k, v in
          gr.make_epilogue(M, N, act, bf16, c_bf16, seed, with_bias=bias, with_r=R, with_c0=out_mode > 0).items()}
    As, lda = store(A, ta, bf16)
    Bs, ldb = store(B, tb, bf16)
    ct = torch.bfloat16 if c_bf16 else torch.float32
    ldc, col0 = out_layout(N, ld)
    Cg = gr.guarded_2d(M, N, ldc, ct, DEV, col0)
    Rg = Zg = Sg = None
    if R:
        Rg = gr.guarded_2d(M, N, ldc + 8, ct, DEV, col0)
        Rg.flat.fill_(1.0)                    # (read only: its surroundings need no sentinel, and SENTINEL + a small value rounds back to it in bf16)
        Rg.view.copy_(ep["R"])
        r_before = Rg.flat.clone()
    if act != gr.ACT_NONE and act != gr.ACT_RELU:
        Zg = gr.guarded_2d(M, N, ldc + 16, z_dtype(act, bf16), DEV, col0)
    if colsum:
        Sg = gr.Guarded(M + 16, 8, (M,), (1,), torch.float32, DEV)
        s_old = torch.randn(M, device=DEV)
    d = GemmDesc()
    d.A, d.B, d.C = As.data_ptr(), Bs.data_ptr(), Cg.view.data_ptr()
    d.M, d.N, d.K, d.lda, d.ldb, d.ldc = M, N, K, lda, ldb, ldc
    d.trans_a, d.trans_b, d.dtype, d.c_dtype = ta, tb, BF if bf16 else F32, BF if c_bf16 else F32
    d.batch, d.batch_inner, d.ksplit, d.alpha = 1, 1, ksplit, alpha
    d.bias = ep["bias"].data_ptr() if bias else None
    d.R, d.ldr = (Rg.view.data_ptr(), ldc + 8) if R else (None, 0)
    d.Z, d.ldz = (Zg.view.data_ptr(), ldc + 16) if Zg is not None else (None, 0)
    d.act, d.out_mode = act, out_mode
    d.a_colsum = Sg.view.data_ptr() if colsum else None
    val, E = gr.gemm_ref(A, B, alpha=alpha, bias=ep["bias"], R=ep["R"], C0=ep["C0"], Z=ep["Z"], act=act, out_mode=out_mode,
                         ksplit=ksplit, bk=64 if bf16 else 32, bf16=bf16, c_bf16=c_bf16, colsum_old=s_old if colsum else None)
    first = None
    for it in range(2 if rerun and out_mode != 2 else 1):
        Cg.view.copy_(ep["C0"]) if out_mode else Cg.view.fill_(NAN)
        if Zg is not None:
            Zg.view.copy_(ep["Z"]) if act in gr.ACT_READS_Z else Zg.view.fill_(NAN)
        if colsum:
            Sg.view.copy_(s_old)
        launch(d, expect, what)
        got = {"C": Cg.view.clone()}
        if act in gr.ACT_WRITES_Z:
            got["Z"] = Zg.view.clone()
        if colsum:
            got["a_colsum"] = Sg.view.clone()
        for g in (Cg, Zg, Sg):
            if g is not None:
                g.intact(what)
        if Rg is not None:
            gr.same_bits(what + " R and its surroundings (read only)", Rg.flat, r_before)
        if act in gr.ACT_READS_Z:
            gr.same_bits(what + " Z (read only)", Zg.view.float().contiguous(), ep["Z"])
        if first is None:
            first = got
            gr.check_all(got, val, E, what, expect)
            if not (bias or R or act or out_mode or c_bf16 or colsum) and alpha == 1.0:
                gr.close(got["C"], val["C"], E["C"], what, expect + "/acc")     # the accumulation term alone: (K + 2) 2^-24 S + 2 roundings
        else:
            gr.same_bits(what + " second run", got["C"], first["C"])
            if "Z" in got:
                assert torch.equal(got["Z"], first["Z"]), what + " second run Z"
    return first["C"]


# ---- the instance list ------------------------------------------------------------------------------------------------------------
# (tests/gemm_ref.py holds the lists: tests/test_gemm_dispatch_cpu.py asks etp_gemm_instance for the same instances without a GPU)
REG, DMA, MM32, GROUPS, MM32_GROUPS, SINGLES = gr.REG, gr.DMA, gr.MM32, gr.GROUPS, gr.MM32_GROUPS, gr.SINGLES
ids = lambda xs: [x["name"] for x in xs]


def k_list(c):
    return gr.k_list(c["kind"], c["bf16"], c["S"])


MATRIX = set(gr.shape_matrix())


def listed(M, N, K, bf16):
    """the CPU emulations (tests/test_gemm_bounds_cpu.py) run over gemm_ref.shape_matrix(): nothing is launched here that is not in it"""
    assert (M, N, K, bf16) in MATRIX, f"{(M, N, K, bf16)} is missing from gemm_ref.shape_matrix()"


@pytest.mark.parametrize("c", SINGLES, ids=ids(SINGLES))
def test_instance(c, etp_opt):
    """One kernel instance on its shape list: whole tiles with every reduction length of its list (register-staged: K = 0, 8, 40, 64,
    72, 160; LDS-DMA: 2, STAGES - 1, STAGES, STAGES + 1 and 12 slabs), tiles_m < tiles_n, ragged in both directions, and -- gemm.hip's
    kernels, mm32 takes whole tiles only -- N = 20 and N = BN + 4 with 16-byte aligned rows and with an odd leading dimension."""
    set_opts(etp_opt, c["opts"])
    sh = gr.tile_shapes(c["BM"], c["BN"])
    ks = k_list(c)
    a = (c["name"],)
    kw = dict(ta=c["ta"], tb=c["tb"], bf16=c["bf16"], c_bf16=c["c_bf16"])
    for K in ks:
        run_case(*a, *sh["whole"], K, **kw)
    run_case(*a, *sh["wide"], ks[1], seed=1, **kw)
    run_case(*a, *sh["wide"], ks[3], seed=1, bias=True, alpha=0.5, **kw)
    if c["kind"].startswith("mm32"):
        return
    for i, K in enumerate(ks if c["kind"] == "reg" else (ks[0], ks[3])):
        run_case(*a, *sh["ragged"], K, seed=2, bias=i % 2 == 1, **kw)
    for j, key in enumerate(("n20", "nbn4")):
        for i, ld in enumerate(("pad", "odd")):
            K = ks[(2 * j + i + 2) % len(ks)]
            run_case(*a, *sh[key], K, seed=3, ld=ld, bias=i == 1, **kw)
            if c["ta"] and c["tb"] and c["kind"] == "dma":
                run_case(*a, *sh[key], K, seed=3, ld=ld, colsum=True, out_mode=1, **kw)


@pytest.mark.parametrize("c", SINGLES, ids=ids(SINGLES))
def test_xcd_tile_map_is_a_permutation(c, etp_opt):
    """tile_of_block's XCD-aware order against the plain one on grids of 10 workgroups (5 x 2 tiles, and 2 x 5 -- with ragged edges for
    gemm.hip's kernels, whole tiles for mm32 -- the map is the identity below 9 workgroups): each under the bound, NaN fill gone
    everywhere, a second run bit-identical, and on / off bit-identical to each other."""
    mm32 = c["kind"].startswith("mm32")
    K = gr.xcd_k(c["kind"], c["bf16"])
    for M, N in gr.xcd_shapes(c["BM"], c["BN"], mm32):
        out = []
        for xcd in ("1", "0"):
            set_opts(etp_opt, dict(c["opts"], GEMM_XCD=xcd))
            out.append(run_case(c["name"], M, N, K, c["ta"], c["tb"], c["bf16"], c["c_bf16"], bias=True))
        gr.same_bits(f"{c['name']} {M}x{N}: XCD map on / off", out[0], out[1])


def test_default_dispatch(etp_opt):
    """The library's own choice, nothing forced but ETP_MM32=0 where gemm.hip is meant: a reduction that is no whole number of
    slabs or shorter than two takes the register-staged kernel; few 64x64 tiles and >= 4 slabs take 32x64; mm32 takes whole tiles."""
    set_opts(etp_opt, {"MM32": "0"})
    for K, bf16 in ((72, True), (64, True), (40, False), (32, False)):
        run_case(inst("gemm", bf16, bf16, 0, 0, 64, 64, 0), 65, 72, K, 0, 0, bf16, bf16)
    run_case(inst("gemm_dma", True, True, 0, 0, 32, 64, 4), 65, 72, 256, 0, 0, True, True)
    run_case(inst("gemm_dma", True, True, 0, 1, 32, 64, 4), 32, 64, 320, 0, 1, True, True)
    run_case(inst("gemm_dma", True, True, 0, 0, 64, 64, 3), 65, 72, 192, 0, 0, True, True)       # < 4 slabs: ring of three
    run_case(inst("gemm_dma", True, False, 1, 1, 64, 64, 4), 65, 72, 256, 1, 1, True, False)     # TN never takes 32x64
    run_case(inst("gemm_dma", True, True, 0, 0, 64, 64, 4), 31, 72, 256, 0, 0, True, True)       # M < 32 neither
    run_case(inst("gemm_dma", False, False, 0, 0, 64, 64, 4), 65, 72, 128, 0, 0, False, False)
    set_opts(etp_opt, {})
    run_case(inst("gemm_dma", True, True, 0, 0, 32, 64, 4), 64, 64, 256, 0, 0, True, True)       # mm32 wants 128-row tiles
    run_case(inst("gemm", True, True, 0, 0, 64, 64, 0), 128, 128, 72, 0, 0, True, True)


LONG = [next(x for x in SINGLES if x["name"] == n) for n in
        ("gemm<bf16,bf16,NT,64x64,s0>", "gemm_dma<bf16,bf16,NN,64x64,s4>", "gemm_dma<f32,f32,TN,128x128,s2>", "mm32<bf16,f32,TN,128x128,s2>",
         "mm32<bf16,bf16,NT,128x64,s3,k2>")]


@pytest.mark.parametrize("c", LONG, ids=ids(LONG))
def test_long_reduction(c, etp_opt):
    """K = 3072 (48 bf16 slabs, 96 fp32 slabs) once per main-loop family: the bound grows with K, the error must not outgrow it"""
    set_opts(etp_opt, c["opts"])
    run_case(c["name"], 2 * c["BM"], c["BN"], 3072, c["ta"], c["tb"], c["bf16"], c["c_bf16"], bias=True, alpha=0.5)


# ---- defect 1 --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("bf16,c_bf16", [(True, True), (True, False), (False, False)])
@pytest.mark.parametrize("act", [gr.ACT_NONE, gr.ACT_GELU, gr.ACT_GELU_SAVEGRAD])
def test_ragged_n_leaves_pad_columns_alone(bf16, c_bf16, act, etp_opt):
    """N % 8 != 0 with a leading dimension that admits 16-byte accesses (ldc % 8 == 0, ldc >= round_up(N, 8), no bias): columns
    N .. round_up(N, 8) - 1 of C and of Z belong to the caller.  (The vectorised epilogue tested `col < N` per 8-column chunk and then
    stored the whole chunk: it wrote them.  Such products take the scalar epilogue now.)"""
    for tile, name in (("64s3", "gemm_dma"), ("64r", "gemm")):
        set_opts(etp_opt, {"GEMM_TILE": tile, "MM32": "0"})
        for N in (20, 68):
            for out_mode in (0, 1):
                run_case(inst(name, bf16, c_bf16, 0, 0, 64, 64, 3 if name == "gemm_dma" else 0), 65, N, 128, 0, 0, bf16, c_bf16, act=act,
                         out_mode=out_mode, R=True)


# ---- epilogues -------------------------------------------------------------------------------------------------------------------
EPI = [("dma", {"GEMM_TILE": "64s3", "MM32": "0"}, "gemm_dma", 64, 64, 3, False, (65, 72, 192), "pad", True),
       ("dma-f32", {"GEMM_TILE": "64s3", "MM32": "0"}, "gemm_dma", 64, 64, 3, False, (65, 72, 96), "pad", False),
       ("reg", {"GEMM_TILE": "64r", "MM32": "0"}, "gemm", 64, 64, 0, False, (65, 72, 72), "pad", True),
       ("scalar", {"GEMM_TILE": "64s3", "MM32": "0"}, "gemm_dma", 64, 64, 3, False, (65, 68, 192), "odd", True),
       ("mm32-128", {"MM32": "128"}, "mm32", 128, 128, 2, False, (128, 128, 256), "pad", True),
       ("mm32-64", {"MM32": "64"}, "mm32", 128, 64, 3, False, (128, 128, 256), "pad", True),
       ("mm32-264", {"MM32": "264"}, "mm32", 128, 64, 3, True, (128, 128, 256), "pad", True),
       ("mm32-262", {"MM32": "262"}, "mm32", 128, 64, 2, True, (128, 128, 256), "pad", True)]


@pytest.mark.parametrize("act", gr.ACTS)
@pytest.mark.parametrize("e", EPI, ids=[e[0] for e in EPI])
def test_epilogue_matrix(e, act, etp_opt):
    """act x bias x R x alpha {1, 0.5, -1.7} x out_mode {0, 1} x C dtype on one LDS-DMA class (bf16 and fp32 operands), the
    register-staged kernel, the scalar epilogue (odd leading dimensions) and each mm32 class.  R is in the OUTPUT dtype (fp32 beside
    bf16 operands when C is fp32); out_mode 1 starts from random contents and, with a bf16 C, rounds once."""
    _, opts, kind, BM, BN, S, k2, (M, N, K), ld, bf16 = e
    set_opts(etp_opt, opts)
    tb = act % 2                                                     # NT and NN alternate with the activation
    for c_bf16 in ((True, False) if bf16 else (False,)):
        name = inst(kind, bf16, c_bf16, 0, tb, BM, BN, S, k2)
        for i, (bias, R, alpha, out_mode) in enumerate(itertools.product((False, True), (False, True), (1.0, 0.5, -1.7), (0, 1))):
            run_case(name, M, N, K, 0, tb, bf16, c_bf16, alpha=alpha, bias=bias, R=R, act=act, out_mode=out_mode, ld=ld, seed=i % 3)


# ---- batched products -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("bf16", [True, False], ids=["bf16", "f32"])
@pytest.mark.parametrize("ta,tb", STOR, ids=["NT", "NN", "TN"])
@pytest.mark.parametrize("K", [64, 128, 200])
def test_batched_products(K, ta, tb, bf16, etp_opt):
    """batch = 6 as 2 x 3 (batch_inner = 3) with six distinct strides: operands are head slices of wide row buffers (inner stride 64
    resp. 72 columns inside rows of 576 / 640: the [rows, 3H] layout of a fused QKV projection; with K > 64 the slices overlap, which
    reading allows), C entries lie apart with gaps of sentinels between them.  Every batch entry under the bound; N = 40 takes the
    vectorised epilogue, N = 20 the scalar one."""
    set_opts(etp_opt, {"MM32": "0"})
    t = torch.bfloat16 if bf16 else torch.float32
    bk = 64 if bf16 else 32
    dma = K % bk == 0 and K >= 2 * bk
    name = inst("gemm_dma" if dma else "gemm", bf16, bf16, ta, tb, 64, 64, (4 if K >= 4 * bk else 3) if dma else 0)
    M = 70
    gen = torch.Generator().manual_seed(K + 2 * ta + tb)
    for N in (40, 20):
        def operand(rows, trans, ld, s_in, asym):
            # logical [2, 3, rows, K] gathered from a [R, ld] buffer: entry (zo, zi) starts at zo * s_out + zi * s_in
            ext_r, ext_c = (K, rows) if trans else (rows, K)
            s_out = (ext_r + 3) * ld
            R_ = 2 * (ext_r + 3)
            assert 2 * s_in + ext_c <= ld
            x = torch.randn(R_, ld, generator=gen)
            x = ((x * 0.1 + 0.01) if asym else x) * gr.row_scales(R_, gen)[:, None]
            buf = x.to(t).to(DEV)
            v = buf.view(-1).as_strided((2, 3, ext_r, ext_c), (s_out, s_in, ld, 1))
            return buf, (v.transpose(-1, -2) if trans else v).float(), s_out
        Abuf, A, sAo = operand(M, ta, 576, 64, False)
        Bbuf, B, sBo = operand(N, tb, 640, 72, True)
        ldc = rup(N, 8) + 8
        sCi, sCo = M * ldc + 16, 3 * (M * ldc + 16) + 40
        Cg = gr.Guarded(2 * sCo + 64, 24, (2, 3, M, N), (sCo, sCi, ldc, 1), t, DEV)
        Cg.view.fill_(NAN)
        d = GemmDesc()
        d.A, d.B, d.C = Abuf.data_ptr(), Bbuf.data_ptr(), Cg.view.data_ptr()
        d.M, d.N, d.K, d.lda, d.ldb, d.ldc = M, N, K, 576, 640, ldc
        d.trans_a, d.trans_b, d.dtype, d.c_dtype = ta, tb, BF if bf16 else F32, BF if bf16 else F32
        d.batch, d.batch_inner, d.ksplit, d.alpha = 6, 3, 1, gr.f32(0.125)
        d.sAo, d.sAi, d.sBo, d.sBi, d.sCo, d.sCi = sAo, 64, sBo, 72, sCo, sCi
        assert len({sAo, 64, sBo, 72, sCo, sCi}) == 6
        what = f"{name} batch 2x3 {M}x{N}x{K}"
        listed(M, N, K, bf16)
        launch(d, name, what)
        val, E = gr.gemm_ref(A, B, alpha=gr.f32(0.125), bf16=bf16)
        gr.close(Cg.view, val["C"], E["C"], what, f"{name}/C")
        Cg.intact(what)
        first = Cg.view.clone()
        Cg.view.fill_(NAN)
        launch(d, name, what)
        gr.same_bits(what + " second run", Cg.view.clone(), first)


# ---- split-K ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("ksplit", [2, 4])
@pytest.mark.parametrize("tokens", [512, 1024])
def test_split_k_through_the_dma_kernel(tokens, ksplit, etp_opt):
    """The planner's split weight gradient: bf16, TN, fp32 atomics (out_mode 2) into random contents, whole slabs per split, with and
    without the fused bias gradient (a_colsum, which every split adds its share to), bias present (first split only)."""
    set_opts(etp_opt, {"MM32": "0"})
    name = inst("gemm_dma", True, False, 1, 1, 64, 64, 4)
    for colsum in (False, True):
        for M, N in ((136, 72), (64, 20)):
            run_case(name, M, N, tokens, 1, 1, True, False, bias=True, out_mode=2, ksplit=ksplit, colsum=colsum,
                     ld="pad" if colsum else "odd")


@pytest.mark.parametrize("bf16", [True, False], ids=["bf16", "f32"])
def test_split_k_through_the_register_staged_kernel(bf16, etp_opt):
    """K = 130 in four splits of one 64-wide slab each leaves the last split EMPTY (it must add nothing, not even the bias); K = 1000
    splits unevenly (K % ksplit != 0 in slabs).  fp32 operands split in 32-wide slabs: K = 130 gives 64 + 64 + 2 + 0 as well."""
    set_opts(etp_opt, {"MM32": "0"})
    for ta, tb in ((1, 1), (0, 0)):
        name = inst("gemm", bf16, False, ta, tb, 64, 64, 0)
        for K, ksplit in ((130, 4), (1000, 4), (1000, 2)):
            if not ta and K % 8:
                K = 136                                            # row-major operands need K a multiple of the chunk: 64 + 64 + 8 + 0
            run_case(name, 65, 72, K, ta, tb, bf16, False, bias=True, alpha=0.5, out_mode=2, ksplit=ksplit)


# ---- groups -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [2, 5, 8])
@pytest.mark.parametrize("c", GROUPS + MM32_GROUPS, ids=ids(GROUPS + MM32_GROUPS))
def test_groups(c, n, etp_opt):
    """etp_gemm_group with n problems whose K arrive in an order the launcher's sort changes (and once uniform): stores and
    accumulates alternate between the members, every second one carries a_colsum (TN), ragged and N % 8 != 0 members in gemm.hip's
    classes.  EVERY problem's C is compared with ITS reference -- a C pointer taken from the caller's order instead of the sorted one
    would land one problem's result in another's buffer -- and every guard is checked."""
    set_opts(etp_opt, c["opts"])
    bf16, c_bf16, ta, tb = c["bf16"], c["c_bf16"], c["ta"], c["tb"]
    bk = 64 if bf16 else 32
    ct = torch.bfloat16 if c_bf16 else torch.float32
    for uniform in (False, True):
        Ks = [256 * bk // 64] * n if uniform else [k * bk // 64 for k in gr.GROUP_K[:n]]
        descs, chk, keep = (GemmDesc * n)(), [], []
        for i, ((M, N), K) in enumerate(zip(gr.group_members(c['BM'], c['BN'], c.get('whole', False), n), Ks)):
            A, B = operands(M, N, K, bf16, 10 + i)
            As, lda = store(A, ta, bf16)
            Bs, ldb = store(B, tb, bf16)
            ldc, col0 = out_layout(N, "pad")
            Cg = gr.guarded_2d(M, N, ldc, ct, DEV, col0)
            out_mode = i % 2
            C0 = torch.randn(M, N, device=DEV).to(ct).float()
            Cg.view.copy_(C0) if out_mode else Cg.view.fill_(NAN)
            colsum = bool(ta and tb and i % 2 == 0)
            Sg = s_old = None
            if colsum:
                Sg = gr.Guarded(M + 16, 8, (M,), (1,), torch.float32, DEV)
                s_old = torch.randn(M, device=DEV)
                Sg.view.copy_(s_old)
            d = descs[i]
            d.A, d.B, d.C = As.data_ptr(), Bs.data_ptr(), Cg.view.data_ptr()
            d.M, d.N, d.K, d.lda, d.ldb, d.ldc = M, N, K, lda, ldb, ldc
            d.trans_a, d.trans_b, d.dtype, d.c_dtype = ta, tb, BF if bf16 else F32, BF if c_bf16 else F32
            d.batch, d.batch_inner, d.ksplit, d.alpha, d.out_mode = 1, 1, 1, 1.0, out_mode
            d.a_colsum = Sg.view.data_ptr() if colsum else None
            keep.append((As, Bs))
            chk.append((A, B, C0, out_mode, Cg, Sg, s_old, (M, N, K)))
        what = f"{c['name']} n {n} K {Ks}"
        first = None
        for it in range(2):                                # the second run, from the same initial contents, must leave the same bits
            for (A, B, C0, out_mode, Cg, Sg, s_old, dims) in chk:
                listed(*dims, bf16)
                Cg.view.copy_(C0) if out_mode else Cg.view.fill_(NAN)
                if Sg is not None:
                    Sg.view.copy_(s_old)
            assert asked(descs, n) == c["name"], f"{what}: etp_gemm_instance names {asked(descs, n)}"
            with _lib.profiled() as p:
                rc = L().etp_gemm_group(descs, n, stream())
                torch.cuda.synchronize()
            assert rc == 0, (what, L().etp_last_error())
            assert p.launches == {c["name"]: 1}, f"{what}: expected one launch of {c['name']}, the library ran {p.launches}"
            if first is not None:
                for i, (x, y) in enumerate(zip(first, chk)):
                    gr.same_bits(f"{what} member {i} second run", y[4].view.clone(), x)
                break
            first = [x[4].view.clone() for x in chk]
            for i, (A, B, C0, out_mode, Cg, Sg, s_old, dims) in enumerate(chk):
                val, E = gr.gemm_ref(A, B, C0=C0 if out_mode else None, out_mode=out_mode, bk=bk, bf16=bf16, c_bf16=c_bf16, colsum_old=s_old)
                got = {"C": Cg.view}
                if Sg is not None:
                    got["a_colsum"] = Sg.view
                    Sg.intact(what)
                gr.check_all(got, val, E, f"{what} member {i} {dims}", c["name"])
                Cg.intact(f"{what} member {i} {dims}")


# ---- refusals ---------------------------------------------------------------------------------------------------------------------
def plain_desc(M=64, N=64, K=128, ta=0, tb=0, bf16=True, c_bf16=None):
    """a valid descriptor over fresh buffers (C NaN-filled) -> (desc, C, keep-alive list)"""
    c_bf16 = bf16 if c_bf16 is None else c_bf16
    A, B = operands(M, N, K, bf16, 0)
    As, lda = store(A, ta, bf16)
    Bs, ldb = store(B, tb, bf16)
    C = torch.full((M, N), NAN, device=DEV, dtype=torch.bfloat16 if c_bf16 else torch.float32)
    d = GemmDesc()
    d.A, d.B, d.C = As.data_ptr(), Bs.data_ptr(), C.data_ptr()
    d.M, d.N, d.K, d.lda, d.ldb, d.ldc = M, N, K, lda, ldb, N
    d.trans_a, d.trans_b, d.dtype, d.c_dtype = ta, tb, BF if bf16 else F32, BF if c_bf16 else F32
    d.batch, d.batch_inner, d.ksplit, d.alpha = 1, 1, 1, 1.0
    return d, C, [As, Bs]


def refused(call, outs, what):
    with _lib.profiled() as p:
        rc = call()
        torch.cuda.synchronize()
    assert rc == -1, f"{what}: returned {rc}, expected ETP_ERR_INVALID (-1)"
    assert p.launches == {}, f"{what}: refused, yet launched {p.launches}"
    for o in outs:
        assert bool(torch.isnan(o).all()), f"{what}: a refused call wrote its output"


def test_refusals():
    """Every combination the contract of include/etpnav_hip.h excludes returns ETP_ERR_INVALID from a host-side argument check
    (desc_to_args / prepare_args / the group launcher's loop, all before the first launch) and leaves the NaN fill intact."""
    one = lambda d: (lambda: L().etp_gemm(ctypes.byref(d), stream()))
    aux = lambda M=64, N=64, t=torch.bfloat16: torch.full((M, N), NAN, device=DEV, dtype=t)
    d, C, k = plain_desc(ta=1, tb=0)
    refused(one(d), [C], "(A trans, B row) storage")
    d, C, k = plain_desc()
    d.lda = d.lda + 4
    refused(one(d), [C], "lda no multiple of the 16-byte chunk")
    d, C, k = plain_desc()
    d.A = d.A + 2
    refused(one(d), [C], "misaligned A")
    d, C, k = plain_desc(c_bf16=False)
    d.ksplit = 2
    refused(one(d), [C], "ksplit > 1 without out_mode 2")
    d, C, k = plain_desc()
    d.out_mode = 2
    refused(one(d), [C], "out_mode 2 with a bf16 C")
    d, C, k = plain_desc(bf16=False)
    d.c_dtype = BF
    refused(one(d), [C], "fp32 operands with a bf16 C")
    cs = torch.full((64,), NAN, device=DEV)
    d, C, k = plain_desc(c_bf16=False)
    d.a_colsum = cs.data_ptr()
    refused(one(d), [C, cs], "a_colsum on an NT product")
    d, C, k = plain_desc(K=72, ta=1, tb=1, c_bf16=False)
    d.a_colsum = cs.data_ptr()
    refused(one(d), [C, cs], "a_colsum on a reduction the LDS-DMA kernel does not take")
    for act in (gr.ACT_GELU, gr.ACT_GELU_BWD, gr.ACT_RELU_BWD, gr.ACT_GELU_SAVEGRAD, gr.ACT_MUL_Z):
        d, C, k = plain_desc()
        d.act = act
        refused(one(d), [C], f"activation {act} without Z")
    # defects 2 and 3: a residual, Z or an activation on a split or batched product
    for split in (True, False):
        for field in ("R", "Z", "act"):
            d, C, k = plain_desc(c_bf16=False)
            outs = [C]
            if split:
                d.ksplit, d.out_mode = 2, 2
            else:
                d.batch, d.batch_inner = 2, 1          # both entries on the same operands and the same C: legal strides
            if field == "R":
                R = torch.zeros(64, 64, device=DEV)
                d.R, d.ldr = R.data_ptr(), 64
            elif field == "Z":
                Z = aux()
                d.Z, d.ldz = Z.data_ptr(), 64
                outs.append(Z)
            else:
                d.act = gr.ACT_RELU
            refused(one(d), outs, f"{'ksplit 2' if split else 'batch 2'} with {field}")
    # groups
    def group(mods, n=2):
        arr, outs, keep = (GemmDesc * n)(), [], []
        for i in range(n):
            d, C, k = plain_desc(M=64, N=64, K=128, ta=1, tb=1, c_bf16=False)
            ctypes.memmove(ctypes.byref(arr[i]), ctypes.byref(d), ctypes.sizeof(GemmDesc))
            outs.append(C)
            keep.append(k)
        mods(arr)
        return (lambda: L().etp_gemm_group(arr, n, stream())), outs, keep

    def mixed_dtype(arr): arr[1].dtype = F32
    def mixed_storage(arr): arr[1].trans_a = 0
    def batched(arr): arr[1].batch = 2
    def split(arr): arr[0].ksplit, arr[0].out_mode = 2, 2
    def short(arr): arr[1].K = 64
    for mods, what in ((mixed_dtype, "mixed operand dtypes"), (mixed_storage, "mixed storage classes"), (batched, "a batched member"),
                       (split, "a split member"), (short, "a member shorter than two slabs")):
        call, outs, keep = group(mods)
        refused(call, outs, "group: " + what)
    call, outs, keep = group(lambda arr: None, n=9)
    refused(call, outs, "group: n = 9")


# ---- the list ---------------------------------------------------------------------------------------------------------------------
def test_every_listed_instance_is_launched_and_named(etp_opt):
    """Counts the instance names the profiler reports against the list above: every register-staged, LDS-DMA, mm32, gemm_group and
    mm32_group instance named in COVERAGE.md's GEMM matrix runs at least once under its own name."""
    want = [c["name"] for c in SINGLES + GROUPS + MM32_GROUPS]
    assert len(want) == len(set(want)) == 18 + 29 + 12 + 20 + 8 + 2, len(want)
    seen = set()
    for c in SINGLES:
        set_opts(etp_opt, c["opts"])
        K = 256 if c["kind"] != "reg" else 72
        d, C, keep = plain_desc(2 * c["BM"], c["BN"], K, c["ta"], c["tb"], c["bf16"], c["c_bf16"])
        with _lib.profiled() as p:
            rc = L().etp_gemm(ctypes.byref(d), stream())
            torch.cuda.synchronize()
        assert rc == 0 and not bool(torch.isnan(C).any()), c["name"]
        seen |= set(p.launches)
    for c in GROUPS + MM32_GROUPS:
        set_opts(etp_opt, c["opts"])
        arr, keep = (GemmDesc * 2)(), []
        for i in range(2):
            d, C, k = plain_desc(2 * c["BM"], c["BN"], 256, c["ta"], c["tb"], c["bf16"], c["c_bf16"])
            ctypes.memmove(ctypes.byref(arr[i]), ctypes.byref(d), ctypes.sizeof(GemmDesc))
            keep.append((C, k))
        with _lib.profiled() as p:
            rc = L().etp_gemm_group(arr, 2, stream())
            torch.cuda.synchronize()
        assert rc == 0 and not any(bool(torch.isnan(C).any()) for C, _ in keep), c["name"]
        seen |= set(p.launches)
    missing = sorted(set(want) - seen)
    assert not missing and seen == set(want), (missing, sorted(seen - set(want)))
