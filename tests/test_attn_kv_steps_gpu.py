"""Op-level tests of the per-episode K/V indirection (etp_attn_fwd_kv / etp_attn_bwd_kv, include/etpnav_hip.h) on the MI355X: B = T * kv_mod
stacked episodes, episode e reads keys / values / key mask of instruction e % kv_mod inside the kernels.  12 heads.

  Lk in {129, 200, 512} x Lq in {5, 64, 128}      streaming kernels (family 3: attn.hip flash_*)
  Lk in {80, 128}       x Lq in {5, 64}           register-resident kernels (family 2: attn_rows.hip), per-step mode only
  kv_mod in {1, 3} x T in {1, 2, 5}; both mask modes (cycling with the case index); per instruction one mask pattern of
  tests/attn_kv_steps.KINDS -- under mask_mode 1 a fully masked LEADING key tile and the last key only valid are in every kv_mod = 3 case
  and alternate over the kv_mod = 1 cases.  Every case asserts its family through etp_attn_family.

Bit identity (sum_steps = 0): ctx, dQ, dK, dV are the SAME BITS as etp_attn_fwd / etp_attn_bwd on K, V and masks replicated T times
  -- the same kernels on the same values.  Outputs start as NaN, sit at leading dimension H + 64 between guard rows holding a
  sentinel that must survive.
Summed mode (sum_steps = 1, family 3): dK / dV [kv_mod * Lk rows] within sum_t E_t of the fp64 reference (tests/attn_kv_steps.py;
  tests/test_attn_kv_steps_cpu.py shows that this bound passes the kernel's schedule and catches a dropped episode, a missing modulo and
  a wrong mask); dQ still bit-identical to the per-step call; a second run bit-identical (no atomics); rows >= kv_mod * Lk of an
  allocation sized for the per-step output untouched.
Refusals: ETP_ERR_INVALID and nothing launched (the NaN fill is still there) for sum_steps = 1 on family 2, B % kv_mod != 0, fp32,
  ATTN_FLASH = 0.
"""
import ctypes

import pytest
import torch

pytestmark = pytest.mark.gpu

from etpnav_amd import _lib  # noqa: E402
from etpnav_amd._lib import AttnDesc, AttnBwdDesc, check  # noqa: E402
from tests import attn_ref as ar  # noqa: E402
from tests import attn_kv_steps as ks  # noqa: E402

DEV = "cuda"
SENTINEL = -777.0
GUARD = 8
NH = 12
H = NH * 64
LD = H + 64
BF = torch.bfloat16
ETP_ERR_INVALID = -1


def L():
    return _lib.lib()


def stream():
    return torch.cuda.current_stream().cuda_stream


class Guarded:
    """[rows, H] output at leading dimension LD inside a buffer with GUARD rows before and `tail` + GUARD rows after: the output region
    starts as NaN, everything else holds SENTINEL and must come back bit-identical."""

    def __init__(self, rows, tail=0):
        self.rows = rows
        self.buf = torch.full((rows + tail + 2 * GUARD, LD), SENTINEL, device=DEV, dtype=BF)
        self.buf[GUARD:GUARD + rows, :H] = float("nan")
        self.ptr = self.buf.data_ptr() + GUARD * LD * 2

    def out(self):
        return self.buf[GUARD:GUARD + self.rows, :H]

    def check(self, name):
        got = self.buf.clone()
        got[GUARD:GUARD + self.rows, :H] = SENTINEL
        ar.same_bits(f"{name}: guard rows / extra columns / rows behind the output", got, torch.full_like(got, SENTINEL))

    def untouched(self):
        return bool(torch.isnan(self.out().float()).all())


def run(c, how, sum_steps=0, expect=None, want_rc=0, dtype=_lib.ETP_BF16, kv_mod=None):
    """one forward + backward on fresh buffers.  how: 'replicated' (etp_attn_fwd / etp_attn_bwd on the T-fold copy) or 'kv'.
    -> dict ctx, dQ [B, heads, Lq, 64], dK, dV [B or kv_mod, heads, Lk, 64]; with want_rc != 0: the return codes and whether anything
    was written."""
    B, Lq, Lk, M = c["B"], c["Lq"], c["Lk"], c["kv_mod"]
    kv_mod = M if kv_mod is None else kv_mod
    t = BF if dtype == _lib.ETP_BF16 else torch.float32
    src = ks.replicated(c) if how == "replicated" else c
    qm = ar.merge_heads(c["q"]).to(DEV).to(t).contiguous()
    kv = torch.cat([ar.merge_heads(src["k"]), ar.merge_heads(src["v"])], 1).to(DEV).to(t).contiguous()      # K | V halves of [rows, 2H]
    km = None if src["km"] is None else src["km"].to(DEV).contiguous()
    dctx = ar.merge_heads(c["dctx"]).to(DEV).to(t).contiguous()
    ldS = (Lk + 7) // 8 * 8
    P = torch.full((B, NH, Lq, ldS), float("nan"), device=DEV, dtype=t)
    dP = torch.full_like(P, float("nan"))
    nkv = M if (how == "kv" and sum_steps) else B
    ctx, dq = Guarded(B * Lq), Guarded(B * Lq)
    dk, dv = Guarded(nkv * Lk, (B - nkv) * Lk), Guarded(nkv * Lk, (B - nkv) * Lk)
    d = AttnDesc()
    d.dtype, d.B, d.heads, d.Lq, d.Lk, d.ldS = dtype, B, NH, Lq, Lk, ldS
    d.Q, d.ldq, d.K, d.ldk, d.V, d.ldv = qm.data_ptr(), H, kv.data_ptr(), 2 * H, kv.data_ptr() + H * kv.element_size(), 2 * H
    d.P, d.ctx, d.ldc = P.data_ptr(), ctx.ptr, LD
    d.keymask, d.mask_mode = (None if km is None else km.data_ptr()), c["mask_mode"]
    d.alpha = c["alpha"]
    if expect is not None:
        fam = L().etp_attn_family(ctypes.byref(d))
        assert fam == expect, f"this case meant family {expect}, the dispatch takes family {fam}"
    bd = AttnBwdDesc()
    bd.f = d
    bd.dctx, bd.ldd, bd.dP = dctx.data_ptr(), H, dP.data_ptr()
    bd.dQ, bd.lddq, bd.dK, bd.lddk, bd.dV, bd.lddv = dq.ptr, LD, dk.ptr, LD, dv.ptr, LD
    if how == "replicated":
        check(L().etp_attn_fwd(ctypes.byref(d), stream()), "attn_fwd")
        check(L().etp_attn_bwd(ctypes.byref(bd), stream()), "attn_bwd")
    elif want_rc == 0:
        check(L().etp_attn_fwd_kv(ctypes.byref(d), kv_mod, stream()), "attn_fwd_kv")
        check(L().etp_attn_bwd_kv(ctypes.byref(bd), kv_mod, sum_steps, stream()), "attn_bwd_kv")
    else:
        rcs = []
        if not sum_steps:              # (sum_steps is a backward argument: that refusal has a forward that runs)
            rcs.append(L().etp_attn_fwd_kv(ctypes.byref(d), kv_mod, stream()))
        rcs.append(L().etp_attn_bwd_kv(ctypes.byref(bd), kv_mod, sum_steps, stream()))
        msg = L().etp_last_error().decode()
        torch.cuda.synchronize()
        written = not all(g.untouched() for g in ((dq, dk, dv) if sum_steps else (ctx, dq, dk, dv)))
        for n, g in (("ctx", ctx), ("dQ", dq), ("dK", dk), ("dV", dv)):
            g.check(n)
        return rcs, written, msg
    torch.cuda.synchronize()
    out = {}
    for n, g, nb in (("ctx", ctx, B), ("dQ", dq, B), ("dK", dk, nkv), ("dV", dv, nkv)):
        g.check(f"{how} {n}")
        assert bool(torch.isfinite(g.out().float()).all()), f"{how} {n}: part of the NaN fill is left"
        out[n] = ar.split_heads(g.out(), nb, NH).contiguous()
    return out


def grid(lqs, lks):
    out = []
    for Lk in lks:
        for Lq in lqs:
            for kv_mod in (1, 3):
                for T in (1, 2, 5):
                    i = len(out)
                    # kv_mod 3: rot 0 -> lead | last | not0 under mode 1; kv_mod 1: lead and last alternate
                    out.append((Lq, Lk, kv_mod, T, (i + i // 6) % 2, 0 if kv_mod == 3 else (i // 6) % 2, i))
    return out


FLASH_G = grid((5, 64, 128), (129, 200, 512))
ROWS_G = grid((5, 64), (80, 128))
ids = lambda g: [f"{x[0]}x{x[1]}-mod{x[2]}-T{x[3]}-m{x[4]}-r{x[5]}" for x in g]


def test_the_grids_cover_both_mask_modes_and_the_two_named_masks():
    for g in (FLASH_G, ROWS_G):
        for kv_mod in (1, 3):
            sub = [x for x in g if x[2] == kv_mod]
            assert {x[4] for x in sub} == {0, 1}
            kinds = {k for x in sub if x[4] == 1 for k in ks.make_steps_case(*x[:4], 1, 1, 0, x[5])["kinds"]}
            assert {"lead", "last"} <= kinds, (kv_mod, kinds)


def case(x):
    Lq, Lk, kv_mod, T, mm, rot, i = x
    return ks.make_steps_case(Lq, Lk, kv_mod, T, NH, mm, seed=i % 3, rot=rot, alpha=0.2 if i % 5 == 3 else 0.125, null_mask=(i % 11 == 7))


def bit_identity(x, family):
    c = case(x)
    want = run(c, "replicated", expect=family)
    got = run(c, "kv", expect=family)
    for n in ("ctx", "dQ", "dK", "dV"):
        ar.same_bits(f"{x} {n}: indirection against the replicated operands", got[n], want[n])
    return c, got


@pytest.mark.parametrize("x", FLASH_G, ids=ids(FLASH_G))
def test_streaming_per_step_is_bit_identical_to_replicated_operands(x):
    bit_identity(x, 3)


@pytest.mark.parametrize("x", ROWS_G, ids=ids(ROWS_G))
def test_register_resident_per_step_is_bit_identical_to_replicated_operands(x):
    bit_identity(x, 2)


@pytest.mark.parametrize("x", FLASH_G, ids=ids(FLASH_G))
def test_streaming_summed_gradient(x):
    c = case(x)
    step = run(c, "kv", expect=3)
    got = run(c, "kv", sum_steps=1, expect=3)
    assert got["dK"].shape == (c["kv_mod"], NH, c["Lk"], 64)
    val, E = ks.summed_ref(c, device=DEV)
    worst = {}
    for n in ("dK", "dV"):
        r = ((got[n].double() - val[n + "_sum"]).abs() / E[n + "_sum"]).max()
        worst[n] = float(r)
    print(f"summed {x[:4]} mode {x[4]}: worst |got - fp64| / bound  dK {worst['dK']:.3f}  dV {worst['dV']:.3f}")
    for n in ("dK", "dV"):
        ar.close(got[n], val[n + "_sum"], E[n + "_sum"], f"summed {x} {n}", f"streaming summed/{n}")
    ar.same_bits(f"{x} dQ: summed call against the per-step call", got["dQ"], step["dQ"])
    ar.same_bits(f"{x} ctx: summed call against the per-step call", got["ctx"], step["ctx"])
    if c["T"] == 1:                    # one step: the sum IS the per-step gradient
        for n in ("dK", "dV"):
            ar.same_bits(f"{x} {n}: T = 1", got[n], step[n])
    again = run(c, "kv", sum_steps=1, expect=3)
    for n in ("ctx", "dQ", "dK", "dV"):
        ar.same_bits(f"{x} {n} of a second run", again[n], got[n])


def refused(rcs, written, msg, what):
    assert all(rc == ETP_ERR_INVALID for rc in rcs), f"{what}: return codes {rcs} ({msg})"
    assert not written, f"{what}: refused, yet an output buffer was written"


def test_refusals(etp_opt):
    rows = ks.make_steps_case(64, 80, 3, 2, NH, 0, seed=0)
    flash = ks.make_steps_case(64, 200, 3, 2, NH, 0, seed=0)
    assert run(rows, "kv", expect=2)["dK"].shape[0] == 6               # the per-step call of that shape runs ...
    refused(*run(rows, "kv", sum_steps=1, expect=2, want_rc=ETP_ERR_INVALID), "sum_steps = 1 on the register-resident family")
    refused(*run(flash, "kv", expect=3, want_rc=ETP_ERR_INVALID, kv_mod=4), "B % kv_mod != 0")
    refused(*run(flash, "kv", sum_steps=1, expect=3, want_rc=ETP_ERR_INVALID, kv_mod=4), "B % kv_mod != 0, summed")
    refused(*run(flash, "kv", expect=3, want_rc=ETP_ERR_INVALID, kv_mod=0), "kv_mod = 0")
    refused(*run(flash, "kv", expect=0, want_rc=ETP_ERR_INVALID, dtype=_lib.ETP_F32), "fp32")
    refused(*run(flash, "kv", sum_steps=1, expect=0, want_rc=ETP_ERR_INVALID, dtype=_lib.ETP_F32), "fp32, summed")
    etp_opt("ATTN_FLASH", 0)
    refused(*run(flash, "kv", expect=0, want_rc=ETP_ERR_INVALID), "ATTN_FLASH = 0")
    refused(*run(flash, "kv", sum_steps=1, expect=0, want_rc=ETP_ERR_INVALID), "ATTN_FLASH = 0, summed")
