"""CPU-side checks of the waypoint head's boundary (in the style of tests/test_boundary_cpu.py): the new symbols are exported, the
engine's parameter table equals the reference key list recorded in the fixture, the module's parameters are views of one arena with
the fused Q | K | V operands adjacent, and the package fails loudly without a GPU.  No kernel is launched here."""
import ctypes
import os

import numpy as np
import pytest
import torch

from etpnav_amd import _lib
from etpnav_amd import waypoint as wp
from tests import waypoint_ref as wr

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "waypoint_small.npz")
NEW = ("etp_ring_attn_fwd", "etp_waypoint_tail", "etp_waypoint_create", "etp_waypoint_destroy", "etp_waypoint_param_count",
       "etp_waypoint_param_info", "etp_waypoint_arena_elems", "etp_waypoint_matrix_elems", "etp_waypoint_bind",
       "etp_waypoint_refresh_weights", "etp_waypoint_ws_bytes", "etp_waypoint_fwd")


def test_new_symbols_are_declared_and_exported():
    L = _lib.lib()
    names = _lib.declared_symbols()
    for n in NEW:
        assert n in names and hasattr(L, n), n


def test_parameter_table_equals_the_reference_key_list():
    keys = [str(k) for k in np.load(GOLDEN)["keys"]]
    for dtype in (torch.float32, torch.bfloat16):
        table = wp.param_table(dtype)
        assert [n for n, _, _ in table] == keys
        assert [s for _, s, _ in table] == [s for _, s in wr.param_shapes()]
        spans = sorted((off, int(np.prod(s))) for _, s, off in table)
        assert all(a + n <= b for (a, n), (b, _) in zip(spans, spans[1:])) and all(a % 64 == 0 for a, _ in spans)
    assert sum(int(np.prod(s)) for _, s, _ in table) == 17614200


def test_module_tree_loads_strictly_and_fuses_qkv():
    m = wp.BinaryDistPredictorTRM(device="cpu", dtype=torch.float32)
    assert list(m.state_dict().keys()) == [k for k, _ in wr.param_shapes()]
    W = wr.make_weights(2)
    m.load_state_dict(W, strict=True)
    for k, v in m.state_dict().items():
        assert torch.equal(v, W[k]), k
    short = dict(W)
    del short["mergefeats_LayerNorm.bias"]
    with pytest.raises(RuntimeError):
        m.load_state_dict(short, strict=True)
    sd = dict(m.named_parameters())
    for l in range(2):
        p = f"waypoint_TRM.bert.encoder.layer.{l}.attention.self."
        for kind in ("weight", "bias"):
            q, k, v = (sd[p + f"{n}.{kind}"] for n in ("query", "key", "value"))
            assert k.data_ptr() == q.data_ptr() + q.numel() * 4 and v.data_ptr() == k.data_ptr() + k.numel() * 4
    # the matrices the forward uses lead the arena (the bf16 shadow region); the unused visual_merge weight is outside it
    n_matrix = m.n_matrix
    base = m.arena.data_ptr()
    assert (sd["vis_classifier.2.weight"].data_ptr() - base) // 4 < n_matrix <= (sd["visual_merge.0.weight"].data_ptr() - base) // 4
    assert all(not p.requires_grad for p in m.parameters())


@pytest.mark.skipif(torch.cuda.is_available(), reason="CPU-only check")
def test_compute_fails_loudly_without_gpu():
    m = wp.BinaryDistPredictorTRM(device="cpu", dtype=torch.float32)
    with pytest.raises(_lib.EtpError):
        m(None, torch.zeros(12, 128, 4, 4))
    with pytest.raises(_lib.EtpError):
        wp.waypoint_tail(torch.zeros(1, 120, 12))
    with pytest.raises(_lib.EtpError):
        wp.ring_attn(*(torch.zeros(12, 768) for _ in range(4)), 1)


def test_argument_validation_without_launching():
    L = _lib.lib()
    assert L.etp_ring_attn_fwd(0, None, 768, None, 768, None, 768, None, 768, 1, 1, 0.125, None) == -1
    assert b"null" in L.etp_last_error()
    assert L.etp_waypoint_tail(None, 1, 5, 7.0, 5.0, None, None, None, None, None, None, None, None, None, None, None) == -1
    assert not L.etp_waypoint_create(7)
    h = L.etp_waypoint_create(_lib.ETP_BF16)
    try:
        assert L.etp_waypoint_param_count(h) == 42
        assert L.etp_waypoint_ws_bytes(h, 0) == 0 and L.etp_waypoint_ws_bytes(h, 8) > 0
        assert L.etp_waypoint_fwd(h, None, 1, None, None, None) == -1            # not bound
        info = _lib.ParamInfo()
        assert L.etp_waypoint_param_info(h, 42, ctypes.byref(info)) == -1
    finally:
        L.etp_waypoint_destroy(h)


def test_policy_keeps_refusing_waypoint_mode_without_encoders():
    from etpnav_amd.policy import ETP
    assert ETP.forward.__defaults__ is not None
    stub = ETP.__new__(ETP)
    torch.nn.Module.__init__(stub)
    stub.depth_encoder = stub.rgb_encoder = None
    with pytest.raises(NotImplementedError):
        ETP.forward(stub, mode="waypoint")
