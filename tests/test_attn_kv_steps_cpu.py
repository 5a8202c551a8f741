"""CPU side of the per-episode K/V indirection with the in-kernel step sum (tests/attn_kv_steps.py has the cases, the reference and the
emulation; tests/test_attn_kv_steps_gpu.py runs the kernels).

  * the new entry points are declared in include/etpnav_hip.h and exported by the built library, and the host-only
    etp_nav_kv_steps_mode answers from the kernel family of the cross-attention descriptor;
  * the bound of the summed gradient -- sum_t E_dK_t, sum_t E_dV_t of tests/attn_ref.py, no multiplier (attn_kv_steps.py's docstring
    says why that is valid) -- can pass and can fail: a float64 emulation of the summed kernel's rounding schedule (bf16 P and dS,
    fp32 accumulation over all T episodes, one bf16 store) stays inside it on EVERY element, and three mutations fall outside it:
    one episode dropped, episode e reading instruction b instead of b % kv_mod, the key mask of the wrong instruction.
"""
import ctypes

import pytest
import torch

from etpnav_amd import _lib
from tests import attn_ref as ar
from tests import attn_kv_steps as ks

NEW_SYMBOLS = ("etp_attn_fwd_kv", "etp_attn_bwd_kv", "etp_nav_kv_steps_mode", "etp_nav_bwd_kv_steps_sum")


def test_new_entry_points_are_declared_and_exported():
    declared = _lib.declared_symbols()
    L = _lib.lib()
    for n in NEW_SYMBOLS:
        assert n in declared, f"{n} is not declared in include/etpnav_hip.h"
        assert hasattr(L, n), f"{n} is not exported by the library"
    protos = _lib.parse_header()
    assert len(protos["etp_attn_fwd_kv"][1]) == 3 and len(protos["etp_attn_bwd_kv"][1]) == 4
    assert protos["etp_nav_bwd_kv_steps_sum"][1] == protos["etp_nav_bwd_kv_steps"][1]      # the same arguments; only d_kv's shape differs


def _planner(dtype):
    from etpnav_amd.planner import make_c_config, default_config
    L = _lib.lib()
    c = make_c_config(default_config("r2r", vocab_size=512, num_l_layers=1, num_pano_layers=1, num_x_layers=1), dtype)
    h = L.etp_planner_create(ctypes.byref(c))
    assert h, L.etp_last_error()
    return L, h


def test_steps_mode_follows_the_cross_attention_family(etp_opt):
    """host only, launches nothing: 1 where the register-resident kernels run, 2 where the streaming kernels run, 0 otherwise"""
    L, h = _planner(torch.bfloat16)
    try:
        mode = lambda B, Lt, G, Bt: L.etp_nav_kv_steps_mode(h, B, Lt, G, Bt)
        assert mode(6, 80, 16, 2) == 1 and mode(6, 128, 128, 3) == 1
        assert mode(6, 129, 16, 2) == 2 and mode(48, 512, 32, 16) == 2 and mode(6, 80, 130, 2) == 2
        assert mode(6, 512, 16, 4) == 0                       # B is not a multiple of Bt
        etp_opt("ATTN_FLASH", 0)
        assert mode(6, 512, 16, 2) == 0 and mode(6, 80, 16, 2) == 1
        etp_opt("ATTN_FLASH", None)
        etp_opt("ATTN_ROWS", 0)
        assert mode(6, 80, 16, 2) == 0 and mode(6, 512, 16, 2) == 2
    finally:
        L.etp_planner_destroy(h)
    L, h = _planner(torch.float32)
    try:
        assert L.etp_nav_kv_steps_mode(h, 6, 80, 16, 2) == 0 and L.etp_nav_kv_steps_mode(h, 6, 512, 16, 2) == 0
    finally:
        L.etp_planner_destroy(h)


# (Lq, Lk, kv_mod, T, mask_mode, rot): the GPU test's axes, two heads; every instruction mask pattern of attn_kv_steps.KINDS appears
CASES = [(5, 129, 3, 2, 1, 0), (64, 200, 3, 5, 0, 0), (128, 512, 1, 5, 1, 0), (64, 129, 1, 2, 0, 1), (5, 512, 3, 5, 1, 2),
         (128, 200, 3, 2, 0, 2), (64, 512, 3, 1, 1, 1), (70, 300, 2, 3, 0, 3)]
ids = lambda g: [f"{x[0]}x{x[1]}-mod{x[2]}-T{x[3]}-m{x[4]}-r{x[5]}" for x in g]


def case(x, seed=0):
    Lq, Lk, kv_mod, T, mm, rot = x
    return ks.make_steps_case(Lq, Lk, kv_mod, T, 2, mm, seed, rot)


def check(c, got, val, E, name):
    for n in ("dV_sum", "dK_sum"):          # every element: attn_ref.close takes the maximum over the whole tensor
        ar.close(got[n], val[n], E[n], f"{name} {n}", f"cpu-steps-sum/{n}")


@pytest.mark.parametrize("x", CASES, ids=ids(CASES))
def test_summed_schedule_stays_inside_the_summed_bound(x):
    c = case(x)
    val, E = ks.summed_ref(c)
    got = ks.emulate_summed(c)
    assert got["dK_sum"].shape == (c["kv_mod"], 2, c["Lk"], 64)
    check(c, got, val, E, f"summed {x}")


MUT_CASES = [x for x in CASES if x[2] >= 2 and x[3] >= 2]


@pytest.mark.parametrize("mut", ["drop_episode", "no_modulo", "wrong_mask"])
@pytest.mark.parametrize("x", MUT_CASES, ids=ids(MUT_CASES))
def test_mutations_of_the_summed_schedule_fall_outside_the_bound(x, mut):
    c = case(x)
    val, E = ks.summed_ref(c)
    got = ks.emulate_summed(c, mut)
    with pytest.raises(AssertionError):
        check(c, got, val, E, f"{mut} {x}")


def test_there_are_mutation_cases_on_a_long_key_axis():
    assert len(MUT_CASES) >= 4 and any(x[1] >= 512 for x in MUT_CASES)
