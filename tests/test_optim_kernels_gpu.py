"""Op-level tests of optim.hip (adamw_kernel, adamw_bump_kernel, sqnorm_kernel) against the float64 restatement and the ELEMENTWISE
derived bounds of tests/reduce_ref.py, through etp_adamw_step, etp_adamw_step_counted, etp_grad_sqnorm and etp_grad_sqnorm_masked.

The reference is restarted from the kernel's own p, m, v (and from the kernel's own fp32 sumsq) at every step, so errors do not compound
and each step is judged alone.  The hyper-parameters are the fp32 values the ABI carries.  Sizes: 64, 1028, 2^18 and 4 194 304 + 1028
(n % 64 = 4: a partial last mask block, and a second grid-stride sweep of the 4096 x 256 x 4 elements one sweep covers); the masked norm
at 2 097 152 + 1028 for the same reason.  Mask bytes come from {0, 1, 2, 3, 255}; the mask has ceil(n / 64) bytes inside a guarded
buffer.  Nothing here uses atomics except sumsq / nonfinite: p, m, v, the shadow and the gradients of a second run from the same state
are compared bit for bit; sumsq where a single workgroup runs (n <= 1024).
"""
import ctypes
import math

import pytest
import torch

pytestmark = pytest.mark.gpu

from etpnav_amd import _lib  # noqa: E402
from etpnav_amd._lib import check, ptr  # noqa: E402
from tests import reduce_ref as rf  # noqa: E402

Guarded, gptr = rf.Guarded, rf.gptr
INVALID = -1


def L():
    return _lib.lib()


def stream():
    return torch.cuda.current_stream().cuda_stream

DEV = "cuda"
F64 = torch.float64
HYPER = rf.HYPER


@pytest.fixture(scope="module", autouse=True)
def report_worst():
    yield
    print("\noptimizer, worst err / bound per (entry point, tensor):\n" + rf.worst_table())
    print("\nnot asserted: p of the counted entry point (fp32 powf on the device) over the bound of etp_adamw_step (host double, no powf term):\n" +
          "\n".join(f"  {k[0]:<48}{k[1]:<20}{v:8.3f}" for k, v in sorted(rf.NOTES.items())))


def c_cfg(cfg):
    return _lib.AdamwCfg(lr=cfg["lr"], beta1=cfg["beta1"], beta2=cfg["beta2"], eps=cfg["eps"], weight_decay=cfg["weight_decay"],
                         step=cfg["step"], hf_style=cfg["hf_style"], correct_bias=cfg["correct_bias"], grad_scale=cfg["grad_scale"],
                         max_norm=cfg["max_norm"])


def state(n, seed):
    g = torch.Generator().manual_seed(seed)
    p = torch.randn(n, generator=g) * 0.3
    p[: max(4, n // 8)] = 0.0
    return [Guarded((n,), init=t.to(DEV)) for t in (p, torch.zeros(n), torch.zeros(n))]


def live_count(mask, n):
    return n if mask is None else int((~rf.frozen_elems(mask, n)).sum())


def sqnorm(g, n, mask, start=0.0, with_nonfinite=True):
    sumsq = Guarded((1,), init=torch.tensor([start], device=DEV))
    bad = Guarded((1,), torch.int32, init=torch.zeros(1, dtype=torch.int32, device=DEV)) if with_nonfinite else None
    if mask is None:
        check(L().etp_grad_sqnorm(ptr(g), n, gptr(sumsq), gptr(bad), stream()), "grad_sqnorm")
    else:
        check(L().etp_grad_sqnorm_masked(ptr(g), n, ptr(mask), gptr(sumsq), gptr(bad), stream()), "grad_sqnorm_masked")
    torch.cuda.synchronize()
    sumsq.check("sumsq")
    if bad is not None:
        bad.check("nonfinite")
    return sumsq, bad


CASES = rf.adamw_cases()


@pytest.mark.parametrize("case", CASES, ids=["-".join(str(v) for v in c) for c in CASES])
def test_adamw_three_steps(case):
    n, hf, cb, h, gs, max_norm, shadow_kind, with_mask, zero_grads = case
    b1, b2, eps = HYPER[h]
    # (n = 64 is ONE mask byte: the seed walks it through the five values, a wholly frozen arena among them)
    mask_g = Guarded((rf.cdiv(n, 64),), torch.uint8, init=rf.adamw_mask(n, seed=n + 4 * hf + 2 * cb + h, device=DEV)) if with_mask else None
    mask = mask_g.t if with_mask else None
    n_shadow = {"half": (n // 2) // 4 * 4, "all": n, "zero": 0, "null": 0}[shadow_kind]
    P, M, V = state(n, n + hf)
    torch.manual_seed(n + 3 * hf + cb)
    sh_init = torch.randn(n, device=DEV).to(torch.bfloat16)
    shadow = None if shadow_kind == "null" else Guarded((n,), torch.bfloat16, init=sh_init)
    clipped = []
    for step in (1, 2, 3):
        cfg = rf.cfg_f32(lr=3e-3, beta1=b1, beta2=b2, eps=eps, weight_decay=0.01, step=step, hf_style=hf, correct_bias=cb, grad_scale=gs,
                         max_norm=max_norm)
        target = 50.0 if step == 2 else 0.3                                     # |g| * grad_scale: clips (max_norm 1, 5) at step 2 only
        live = live_count(mask, n)
        g0 = torch.randn(n, device=DEV) * (target / (math.sqrt(max(live, 1)) * cfg["grad_scale"]))
        if step == 3:                                                           # elements whose update nearly cancels p
            q = rf.adamw(P.t, g0, M.t, V.t, cfg, float((g0.double() ** 2).sum()) if max_norm > 0 else None, mask)
            P.t[1::7] = q["upd"][1::7].float()
        sumsq, bad = sqnorm(g0, n, mask)
        ss = float(sumsq.t)
        want, _ = rf.sumsq(g0, mask)
        assert abs(ss - float(want)) <= rf.sumsq_bound(g0, mask, 0.0) and int(bad.t) == 0
        old = (P.t.clone(), M.t.clone(), V.t.clone())
        sh_old = None if shadow is None else shadow.t.clone()
        r = rf.adamw(*old[:1], g0, *old[1:], cfg, ss if max_norm > 0 else None, mask)
        clipped.append(max_norm > 0 and math.sqrt(ss) * cfg["grad_scale"] > max_norm)
        results = []
        for rerun in range(2):
            for gd, o in zip((P, M, V), old):
                gd.t.copy_(o)
            if shadow is not None:
                shadow.t.copy_(sh_old)
            g = Guarded((n,), init=g0)
            cc = c_cfg(cfg)
            check(L().etp_adamw_step(gptr(P), gptr(g), gptr(M), gptr(V), gptr(shadow), n_shadow, ptr(mask), n, ctypes.byref(cc),
                                     gptr(sumsq) if max_norm > 0 else None, gptr(bad), zero_grads, stream()), "adamw_step")
            torch.cuda.synchronize()
            for gd, name in ((P, "p"), (M, "m"), (V, "v"), (g, "grads"), (shadow, "shadow"), (mask_g, "mask")):
                if gd is not None:
                    gd.check("adamw " + name)
            results.append([t.clone() for t in (P.t, M.t, V.t, g.t)] + ([] if shadow is None else [shadow.t.clone()]))
        for a, b in zip(*results):
            rf.same_bits("adamw (second run from the same state)", a, b)
        name = f"etp_adamw_step {'hf' if hf else 'torch'} b2={b2}"
        rf.check_adamw(name, (P.t, M.t, V.t), old, r, cfg, False, None if shadow is None else shadow.t, sh_old, n_shadow)
        rf.check_grads_after(name, g.t, g0, zero_grads)
    assert clipped == [False, max_norm > 0 and live > 0, False]


@pytest.mark.parametrize("n", rf.COUNTED_N)
@pytest.mark.parametrize("hf,h,cb", rf.COUNTED)
def test_adamw_counted_follows_applied_steps(n, hf, h, cb):
    """apply, apply, skip, apply: the counter reads 1, 2, 2, 3 and the fourth call uses t = 3; a skipped FIRST step leaves everything but
    the gradients alone and the counter at 0"""
    b1, b2, eps = HYPER[h]
    mask = rf.adamw_mask(n, seed=n + 1, device=DEV)
    P, M, V = state(n, n + 11)
    shadow = Guarded((n,), torch.bfloat16, init=torch.randn(n, device=DEV).to(torch.bfloat16))
    counter = Guarded((1,), torch.int32, init=torch.zeros(1, dtype=torch.int32, device=DEV))
    skip = torch.zeros(1, dtype=torch.int32, device=DEV)
    cfg = rf.cfg_f32(lr=3e-3, beta1=b1, beta2=b2, eps=eps, weight_decay=0.01, step=-5, hf_style=hf, correct_bias=cb, grad_scale=0.5,
                     max_norm=0.0)
    name = f"etp_adamw_step_counted {'hf' if hf else 'torch'} b2={b2}"
    torch.manual_seed(n + h)

    def call(skipped):
        g0 = torch.randn(n, device=DEV) * 0.02
        g = Guarded((n,), init=g0)
        skip.fill_(7 if skipped else 0)
        old = (P.t.clone(), M.t.clone(), V.t.clone())
        sh_old, before = shadow.t.clone(), int(counter.t)
        cc = c_cfg(cfg)
        check(L().etp_adamw_step_counted(gptr(P), gptr(g), gptr(M), gptr(V), gptr(shadow), n, ptr(mask), n, ctypes.byref(cc), None, ptr(skip), 1,
                                         gptr(counter), stream()), "adamw_step_counted")
        torch.cuda.synchronize()
        for gd in (P, M, V, g, shadow, counter):
            gd.check(name)
        r = rf.adamw(old[0], g0, old[1], old[2], cfg, None, mask, skip=skipped, steps_applied=before)
        rf.check_adamw(name, (P.t, M.t, V.t), old, r, cfg, True, shadow.t, sh_old, n)
        rf.check_grads_after(name, g.t, g0, 1)
        assert int(counter.t) == r["counter"]
        if not skipped and cb:
            # for the record only: the same result against the bound WITHOUT the device-powf term (what etp_adamw_step is held to)
            host = rf.adamw_bounds(*old, r, cfg, False)[0]
            err = (P.t.to(F64) - r["p"]).abs()
            rf.note((name, f"t={r['step']}"), float((err / host.clamp_min(1e-300))[host > 0].max()))
        return old, g0, r

    call(True)                                                                    # a skipped first step
    assert int(counter.t) == 0
    seen = []
    for skipped in (False, False, True, False):
        old, g0, r = call(skipped)
        seen.append(int(counter.t))
    assert seen == [1, 2, 2, 3] and r["step"] == 3
    # the fourth update is etp_adamw_step(step = 3)'s, within the same bound
    P2, M2, V2 = (Guarded((n,), init=o) for o in old)
    g = Guarded((n,), init=g0)
    cc = c_cfg(dict(cfg, step=3))
    check(L().etp_adamw_step(gptr(P2), gptr(g), gptr(M2), gptr(V2), None, 0, ptr(mask), n, ctypes.byref(cc), None, None, 1, stream()), "adamw_step")
    torch.cuda.synchronize()
    rf.check_adamw(name + " vs step=3", (P2.t, M2.t, V2.t), old, r, cfg, False)


@pytest.mark.parametrize("n,masked,nbad", rf.sqnorm_cases())
def test_grad_sqnorm(n, masked, nbad):
    torch.manual_seed(n + nbad)
    g = torch.randn(n, device=DEV) * 0.3
    g[-1] = 30.0                                                         # the last float4 carries a term far above the bound
    mask_g = Guarded((rf.cdiv(n, 64),), torch.uint8, init=rf.adamw_mask(n, seed=n, device=DEV)) if masked else None   # guard bytes: frozen
    mask = mask_g.t if masked else None
    if masked:
        mask[-1] = 1
        if n >= 1028:
            mask[3] = 2
            g[3 * 64 + 5] = float("nan")                                 # a frozen block contributes to neither output, NaN or not
            g[3 * 64 + 6] = float("inf")
    specials = [float("nan"), float("inf"), float("-inf"), float("nan"), float("-inf")]
    spots = [n - 2, (2097152 + 40) if n > 2097152 else 0, 1, n // 2 // 64 * 64, 2][:nbad]   # last float4; second sweep; ...
    if masked and n >= 1028:
        for s in spots:
            mask[s // 64] = 255
    for s, v in zip(spots, specials):
        g[min(s, n - 1)] = v
    nbad = len({min(s, n - 1) for s in spots})
    start = 2.5
    sumsq, bad = sqnorm(g, n, mask, start)
    want, count = rf.sumsq(g, mask)
    assert int(bad.t) == count == nbad
    if nbad == 0:
        b = rf.sumsq_bound(g, mask, start)
        assert 900.0 > 8 * b
        ratio = abs(float(sumsq.t) - (float(want) + start)) / b
        rf._record(("etp_grad_sqnorm" + ("_masked" if masked else ""), "sumsq"), ratio)
        assert ratio <= 1.0, ratio
        again, _ = sqnorm(g, n, mask, start, with_nonfinite=False)       # nonfinite NULL is accepted
        if n <= 1024:
            rf.same_bits("sumsq (second run, one workgroup)", again.t, sumsq.t)
        assert abs(float(again.t) - (float(want) + start)) <= b
    else:
        assert not math.isfinite(float(sumsq.t))


def test_optimizer_refusals():
    n = 1028
    P, M, V = state(n, 1)
    g = Guarded((n,), init=torch.randn(n, device=DEV))
    shadow = Guarded((n,), torch.bfloat16)
    sumsq = torch.ones(1, device=DEV)
    counter = Guarded((1,), torch.int32, init=torch.zeros(1, dtype=torch.int32, device=DEV))
    base = dict(lr=1e-3, beta1=0.9, beta2=0.999, eps=1e-8, weight_decay=0.01, step=1, hf_style=0, correct_bias=1, grad_scale=1.0, max_norm=0.0)

    def step(cfg, n_=n, n_shadow=0, ss=None, p=None):
        cc = c_cfg(rf.cfg_f32(**cfg))
        return L().etp_adamw_step(gptr(P) if p is None else p, gptr(g), gptr(M), gptr(V), gptr(shadow), n_shadow, None, n_, ctypes.byref(cc), ss,
                                  None, 1, stream())

    cc = c_cfg(rf.cfg_f32(**dict(base, max_norm=1.0)))
    calls = [step(base, n_=n - 2), step(base, n_shadow=n + 4), step(dict(base, beta1=1.0)), step(dict(base, beta2=1.5)), step(dict(base, step=0)),
             step(dict(base, max_norm=1.0), ss=None), step(base, p=P.t[1:].data_ptr(), n_=n - 4),
             L().etp_adamw_step_counted(gptr(P), gptr(g), gptr(M), gptr(V), None, 0, None, n, ctypes.byref(cc), None, None, 1, gptr(counter), stream()),
             L().etp_grad_sqnorm(ptr(g.t), n - 2, ptr(sumsq), None, stream()), L().etp_grad_sqnorm(g.t[1:].data_ptr(), n - 4, ptr(sumsq), None, stream())]
    torch.cuda.synchronize()
    assert calls == [INVALID] * len(calls), calls
    for gd, name in ((P, "p"), (M, "m"), (V, "v"), (g, "grads"), (shadow, "shadow"), (counter, "counter")):
        gd.intact("refused optimizer call, " + name)
    assert float(sumsq) == 1.0
    # the same clipping call with the norm is accepted (and step = 0 is fine when a counter drives the bias correction)
    cc = c_cfg(rf.cfg_f32(**dict(base, max_norm=1.0, step=0)))
    check(L().etp_adamw_step_counted(gptr(P), gptr(g), gptr(M), gptr(V), None, 0, None, n, ctypes.byref(cc), ptr(sumsq), None, 1, gptr(counter),
                                     stream()), "adamw_step_counted")
    torch.cuda.synchronize()
    assert int(counter.t) == 1
