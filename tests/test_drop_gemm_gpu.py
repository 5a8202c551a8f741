"""Dropout in the GEMM epilogue at operator level, through etp_gemm_drop, on the kernel instances the planner runs it on -- each
ASSERTED BY NAME (etp_gemm_instance before the launch, the per-launch profiler around it), against tests/drop_ref.py's fp64
restatement (gemm_ref.gemm_ref with the mask between the activation and the residual) under its elementwise bound.

The three compositions the planner launches with a mask (drop_ref.gemm_comp):
  bias_res   bias + mask + residual into an fp32 C          linear_fwd_s
  savegrad   ETP_ACT_GELU_SAVEGRAD + mask                   Z must be bit-identical to the unmasked launch
  mul_z      ETP_ACT_MUL_Z + mask                           the FFN dgrad
on (drop_ref.GEMM_INSTANCES): mm32 128x128 s2, 128x64 s3 and 128x64 s3 k2; gemm_dma 64x64 s3 in bf16 and fp32; the register-staged
64x64 in bf16 and fp32; the scalar epilogue at N = 69 (odd: element indices of both parities start the rows) on gemm_dma with
aligned rows and on the register-staged kernel with an odd leading dimension.  Shapes: whole tiles (2 BM x BN) and ragged
(BM + 1, BN + 8) with ldc = N + 8, out_mode 0, and one out_mode 1 case.  mm32 takes whole tiles and whole 64-slabs only (two at
least, the k2 class four): its reduction lengths are 128 and 192 (k2: 256 and 384) and it has no ragged shape; gemm_dma in bf16
takes 128 and 192; everything else K = 64 and 160.

Every case:
  mask read-out, exact   C == R (+ old C; 0 without them) exactly where multiplier(row * N + col) == 0, every element compared;
                         drop_ref.gemm_readable shows on the reference alone that no kept element can read so
  values                 C and Z under the bound; Z of savegrad bit-identical to the plain launch's
  plain entry            etp_gemm_drop with NULL and with p = 0 leaves the bits of etp_gemm; p = 1e-6 scales everything by 1 / (1 - p)
  harness                NaN-filled outputs inside sentinel buffers (guard rows, guard columns N .. ldc - 1), R and the Z operand
                         unchanged, a second run bit for bit
Refusals: a mask with ksplit 2 or batch 2 is ETP_ERR_INVALID and writes nothing; so is a site outside its ranges.  The group
launcher has no `_drop` entry point: etp_gemm_group cannot be handed a mask at this ABI (desc_to_args leaves GemmArgs::drop at p = 0).
"""
import ctypes

import pytest
import torch

pytestmark = pytest.mark.gpu

from etpnav_amd import _lib  # noqa: E402
from etpnav_amd._lib import GemmDesc  # noqa: E402
from tests import drop_ref as dr  # noqa: E402
from tests import gemm_ref as gr  # noqa: E402

DEV = "cuda"
BF, F32 = _lib.ETP_BF16, _lib.ETP_F32
NAN = float("nan")
INVALID = -1


def L():
    return _lib.lib()


def stream():
    return torch.cuda.current_stream().cuda_stream


def rup(x, m):
    return (x + m - 1) // m * m


def set_opts(etp_opt, opts):
    for k in gr.GEMM_SWITCHES:
        etp_opt(k, opts.get(k))


@pytest.fixture(scope="module", autouse=True)
def leave_the_global_generators_alone():
    """every operand here comes from its own seeded generator; other files draw from torch's global ones without seeding them, so this
    file hands them back as it found them"""
    cpu, gpu = torch.get_rng_state(), torch.cuda.get_rng_state()
    yield
    assert torch.equal(torch.get_rng_state(), cpu) and torch.equal(torch.cuda.get_rng_state(), gpu), "a case drew from a global generator"


@pytest.fixture(scope="module", autouse=True)
def report_worst():
    yield
    print("\nGEMM epilogue dropout, worst err / bound per (instance, tensor):")
    for (k, n), v in sorted(dr.WORST.items(), key=str):
        print(f"  {v:8.4f}  {k}/{n}")


def store(X, trans, bf16):
    """logical [rows, K] values -> the stored operand with one spare 16-byte chunk per row (holding 3.0) and its leading dimension"""
    t = torch.bfloat16 if bf16 else torch.float32
    epc = 8 if bf16 else 4
    rows, K = X.shape
    if trans:
        ld = rup(rows, epc) + epc
        buf = torch.full((K, ld), 3.0, device=DEV, dtype=t)
        buf[:, :rows] = X.t().to(t)
    else:
        ld = rup(K, epc) + epc
        buf = torch.full((rows, ld), 3.0, device=DEV, dtype=t)
        buf[:, :K] = X.to(t)
    return buf, ld


def z_dtype(bf16):
    return torch.float16 if bf16 else torch.float32


class Launch:
    """one product's buffers and descriptor; run(site) launches it into fresh NaN-filled outputs and returns {"C", "Z"}"""

    def __init__(self, c, ta, tb, layout):
        self.c = c
        M, N, bf16 = c["M"], c["N"], c["bf16"]
        self.ct = torch.bfloat16 if c["c_bf16"] else torch.float32
        # ta = 0 always here; B is stored [N, K] (NT) or [K, N] (NN)
        self.As, lda = store(c["A"].to(DEV), ta, bf16)
        self.Bs, ldb = store(c["B"].to(DEV), tb, bf16)
        ldc, col0 = (N + 8, 8) if layout == "pad" else (rup(N, 8) + 61, 3)
        if layout == "pad" and N % 8:
            ldc = rup(N, 8) + 8
        self.Cg = gr.guarded_2d(M, N, ldc, self.ct, DEV, col0)
        self.Rg = self.Zg = None
        if c["R"] is not None:
            self.Rg = gr.guarded_2d(M, N, ldc + 8, self.ct, DEV, col0)
            self.Rg.flat.fill_(1.0)
            self.Rg.view.copy_(c["R"].to(DEV))
            self.r_before = self.Rg.flat.clone()
        if c["act"] in (gr.ACT_GELU_SAVEGRAD, gr.ACT_MUL_Z):
            self.Zg = gr.guarded_2d(M, N, ldc + 16, z_dtype(bf16), DEV, col0)
        self.bias = c["bias"].to(DEV)
        d = self.d = GemmDesc()
        d.A, d.B, d.C = self.As.data_ptr(), self.Bs.data_ptr(), self.Cg.view.data_ptr()
        d.M, d.N, d.K, d.lda, d.ldb, d.ldc = M, N, c["K"], lda, ldb, ldc
        d.trans_a, d.trans_b, d.dtype, d.c_dtype = ta, tb, BF if bf16 else F32, BF if c["c_bf16"] else F32
        d.batch, d.batch_inner, d.ksplit, d.alpha = 1, 1, 1, c["alpha"]
        d.bias = self.bias.data_ptr()
        d.R, d.ldr = (self.Rg.view.data_ptr(), ldc + 8) if self.Rg is not None else (None, 0)
        d.Z, d.ldz = (self.Zg.view.data_ptr(), ldc + 16) if self.Zg is not None else (None, 0)
        d.act, d.out_mode = c["act"], c["out_mode"]
        self.ldc = ldc

    def run(self, expect, what, site=None, plain=False):
        c = self.c
        self.Cg.view.copy_(c["C0"].to(DEV)) if c["out_mode"] else self.Cg.view.fill_(NAN)
        if self.Zg is not None:
            self.Zg.view.copy_(c["Z"].to(DEV)) if c["act"] == gr.ACT_MUL_Z else self.Zg.view.fill_(NAN)
        buf = ctypes.create_string_buffer(96)
        assert L().etp_gemm_instance(ctypes.byref(self.d), 1, buf, 96) >= 0 and buf.value.decode() == expect, \
            f"{what}: etp_gemm_instance names {buf.value.decode()}, the case means {expect}"
        s = None if site is None else _lib.DropSite(site.p, site.seed, site.mode, site.layer, site.slot)
        with _lib.profiled() as p:
            if plain:
                rc = L().etp_gemm(ctypes.byref(self.d), stream())
            else:
                rc = L().etp_gemm_drop(ctypes.byref(self.d), stream(), None if s is None else ctypes.byref(s))
            torch.cuda.synchronize()
        assert rc == 0, (what, rc, L().etp_last_error())
        assert p.launches == {expect: 1}, f"{what}: expected one launch of {expect}, the library ran {p.launches}"
        for g in (self.Cg, self.Zg):
            if g is not None:
                g.intact(what)
        if self.Rg is not None:
            gr.same_bits(what + " R and its surroundings (read only)", self.Rg.flat, self.r_before)
        got = {"C": self.Cg.view.clone()}
        if c["act"] == gr.ACT_GELU_SAVEGRAD:
            got["Z"] = self.Zg.view.clone()
        if c["act"] == gr.ACT_MUL_Z:
            gr.same_bits(what + " Z (read only)", self.Zg.view.float().contiguous(), c["Z"].to(DEV))
        return got


def same(what, a, b):
    for n in a:
        gr.same_bits(f"{what} {n}", a[n].float().contiguous(), b[n].float().contiguous())


def one_case(name, iid, c, tb, layout, site, seed_note=""):
    what = f"{name} {c['comp']} {c['M']}x{c['N']}x{c['K']} out_mode {c['out_mode']} p {site.p} site {(site.mode, site.layer, site.slot)}"
    ok, why = dr.gemm_readable(c)
    assert ok, why
    ln = Launch(c, 0, tb, layout)
    m = site.rows(c["M"], c["N"], device=DEV)
    got = ln.run(name, what, site)
    same(what + " second run", ln.run(name, what, site), got)
    dr.check_gemm(what, name, c, got, m)
    plain = ln.run(name, what + " plain", plain=True)
    if "Z" in got:
        gr.same_bits(what + ": Z undropped, the bits of the unmasked launch", got["Z"].float().contiguous(), plain["Z"].float().contiguous())
    same(what + " NULL against etp_gemm", ln.run(name, what, None), plain)
    same(what + " p = 0 against etp_gemm", ln.run(name, what, dr.Site(0.0, (site.mode, site.layer, site.slot))), plain)
    tiny = ln.run(name, what, dr.Site(dr.P_TINY, (site.mode, site.layer, site.slot)))
    val, E = dr.gemm_ref(c, torch.full((c["M"], c["N"]), float(dr.inv_keep(dr.P_TINY)), device=DEV))
    for n in val:
        gr.close(tiny[n], val[n], E[n], f"{what} p = 1e-6 {n}", f"{name}/{n} p=1e-6")
    return ln


CASES = [(inst, comp) for inst in dr.GEMM_INSTANCES for comp in dr.GEMM_COMPS]


@pytest.mark.parametrize("inst,comp", CASES, ids=[f"{i[0]}-{c}" for i, c in CASES])
def test_epilogue_dropout(inst, comp, etp_opt):
    iid, opts, kern, BM, BN, S, k2, bf16, shapes, Ks, layout = inst
    set_opts(etp_opt, opts)
    act, c_bf16, (ta, tb) = dr.gemm_comp(comp, bf16)
    name = gr.inst(kern, bf16, c_bf16, ta, tb, BM, BN, S, k2)
    i = 0
    for (M, N) in shapes:
        for K in Ks:
            site = dr.Site(dr.RATES[i % 2], dr.SITES[(i // 2 + dr.GEMM_COMPS.index(comp)) % 2])
            one_case(name, iid, dr.gemm_case(M, N, K, bf16, comp, seed=i), tb, layout, site)
            i += 1


def test_out_mode_1_with_a_mask(etp_opt):
    """C += m * (A B^T + bias) + R: accepted with a mask; the old C joins after the residual"""
    set_opts(etp_opt, {"GEMM_TILE": "64s3", "MM32": "0"})
    for bf16, K in ((False, 160), (True, 192)):
        c = dr.gemm_case(65, 72, K, bf16, "bias_res", seed=9, out_mode=1)
        one_case(gr.inst("gemm_dma", bf16, False, 0, 0, 64, 64, 3), "dma", c, 0, "pad", dr.Site(0.4, dr.SITES[1]))


def test_refusals(etp_opt):
    """a mask on a split or a batched product, and a site outside its ranges: ETP_ERR_INVALID, nothing written"""
    set_opts(etp_opt, {"MM32": "0"})
    c = dr.gemm_case(65, 72, 128, True, "bias_res", seed=3)
    c["R"] = None
    site = dr.Site(0.1, dr.SITES[0])

    def refused(what, s, needle=None, **fields):
        ln = Launch(c, 0, 0, "pad")
        ln.Cg.view.fill_(NAN)
        for k, v in fields.items():
            setattr(ln.d, k, v)
        rc = L().etp_gemm_drop(ctypes.byref(ln.d), stream(), ctypes.byref(s))
        torch.cuda.synchronize()
        assert rc == INVALID and (needle is None or needle in L().etp_last_error()), (what, rc, L().etp_last_error())
        assert bool(torch.isnan(ln.Cg.view.float()).all()), what + ": the NaN fill was written"
        ln.Cg.intact(what)

    good = _lib.DropSite(site.p, site.seed, site.mode, site.layer, site.slot)
    refused("ksplit 2", good, b"dropout", ksplit=2, out_mode=2, bias=None)
    refused("batch 2", good, b"dropout", batch=2, bias=None)
    for bad in ((1.0, 1, 0, 0), (-0.5, 1, 0, 0), (0.1, 1, 0, 16), (0.1, -1, 0, 0)):
        refused(f"site {bad}", _lib.DropSite(bad[0], dr.SEED, bad[1], bad[2], bad[3]))
