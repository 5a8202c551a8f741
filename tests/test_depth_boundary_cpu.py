"""CPU-side checks of the depth encoder's boundary (in the style of tests/test_clip_boundary_cpu.py): the new symbols are exported, the
engine's parameter table is the state dict of habitat's ResNetEncoder with its shapes (162 tensors, 7 069 408 parameters at the shipped
size), the module's parameters are frozen views of one arena and load strictly, every refusal of the create call and of the host-checked
entry points, and the package fails loudly without a GPU.  No kernel is launched here."""
import ctypes

import numpy as np
import pytest
import torch

from etpnav_amd import _lib
from etpnav_amd import depth as dp
from tests import depth_ref as dr

NEW = ("etp_depth_stem", "etp_gn_stats", "etp_gn_apply", "etp_maxpool3x3s2", "etp_conv_rows", "etp_depth_create", "etp_depth_destroy",
       "etp_depth_param_count", "etp_depth_param_info", "etp_depth_arena_elems", "etp_depth_matrix_elems", "etp_depth_out_channels",
       "etp_depth_bind", "etp_depth_refresh_weights", "etp_depth_ws_bytes", "etp_depth_fwd", "etp_depth_fwd_views", "etp_depth_set_probe")
INVALID = -1


def _blocks(*b):
    return (ctypes.c_int * 4)(*b)


def test_new_symbols_are_declared_and_exported():
    L = _lib.lib()
    names = _lib.declared_symbols()
    for n in NEW:
        assert n in names and hasattr(L, n), n


def test_parameter_table_is_the_state_dict():
    for dtype in (torch.float32, torch.bfloat16):
        table = dp.param_table(dtype)
        assert len(table) == 162
        assert [(n, s) for n, s, _ in table] == dr.param_shapes(*dr.FULL)
        assert sum(int(np.prod(s)) for _, s, _ in table) == 7069408
        spans = sorted((off, int(np.prod(s))) for _, s, off in table)
        assert all(a + n <= b for (a, n), (b, _) in zip(spans, spans[1:])) and all(a % 64 == 0 for a, _ in spans)
    for S, bp, blocks in dr.ENGINE_CASES + ((192, 32, (1, 1, 1, 1)),):
        small = dp.param_table(torch.float32, S, bp, blocks)
        assert [(n, s) for n, s, _ in small] == dr.param_shapes(S, bp, blocks), (S, bp, blocks)
    assert dict((n, s) for n, s, _ in small)["compression.0.weight"] == (228, 1024, 3, 3)      # round(2048 / 9)


def test_module_tree_loads_strictly():
    S, bp, blocks = dr.ENGINE_CASES[1]
    m = dp.DepthEncoder(device="cpu", dtype=torch.float32, image_size=S, base_planes=bp, blocks=blocks)
    assert list(m.state_dict().keys()) == [k for k, _ in dr.param_shapes(S, bp, blocks)]
    assert m.output_shape == (2048, 1, 1)
    W = dr.make_weights(S, bp, blocks, 2)
    m.load_state_dict(W, strict=True)
    for k, v in m.state_dict().items():
        assert torch.equal(v, W[k]), k
    short = dict(W)
    del short["compression.1.bias"]
    with pytest.raises(RuntimeError):
        m.load_state_dict(short, strict=True)
    with pytest.raises(RuntimeError):
        m.load_state_dict(dict(W, extra=torch.zeros(1)), strict=True)
    # every parameter is a frozen view of the one arena; the GEMM matrices lead it (the packed region), everything fp32-only follows
    base = m.arena.data_ptr()
    for k, p in m.named_parameters():
        off = (p.data_ptr() - base) // 4
        assert 0 <= off and off + p.numel() <= m.total and off % 64 == 0, k
        assert (off < m.n_matrix) == (p.dim() == 4 and k != "backbone.conv1.0.weight"), k
    assert all(not p.requires_grad for p in m.parameters()) and not m.training
    with pytest.raises(TypeError):
        m.double()
    feats = torch.zeros(2, 128, 4, 4)
    assert m({"depth_features": feats}) is feats                                              # resnet_encoders.py:83-84
    assert dp.DepthEncoder(device="cpu", dtype=torch.float32).output_shape == (128, 4, 4)


def test_create_refusals():
    L = _lib.lib()
    ok = _blocks(3, 4, 6, 3)
    for args in ((7, 256, 32, ok), (0, 0, 32, ok), (0, 32, 32, ok), (0, 96, 32, ok), (0, 320, 32, ok), (0, -64, 32, ok), (0, 256, 24, ok),
                 (0, 256, 64, ok), (0, 256, 0, ok), (0, 256, 32, None), (0, 256, 32, _blocks(0, 4, 6, 3)), (0, 256, 32, _blocks(3, 4, 7, 3)),
                 (1, 256, 32, _blocks(3, 4, 6, -1))):
        assert not L.etp_depth_create(*args), args[:3]
        assert b"etp_depth_create" in L.etp_last_error()
    with pytest.raises(_lib.EtpError):
        dp.DepthEncoder(device="cpu", image_size=96)
    with pytest.raises(_lib.EtpError):
        dp.DepthEncoder(device="cpu", base_planes=24)
    with pytest.raises(_lib.EtpError):
        dp.DepthEncoder(device="cpu", blocks=(3, 4, 6))
    for S, cc in ((64, 2048), (128, 512), (192, 228), (256, 128)):
        h = L.etp_depth_create(1, S, 16, _blocks(1, 1, 1, 1))
        assert h and L.etp_depth_param_count(h) == 3 + 4 * 12 + 3 and L.etp_depth_out_channels(h) == cc
        L.etp_depth_destroy(h)


def test_engine_refusals_without_launching():
    L = _lib.lib()
    h = L.etp_depth_create(_lib.ETP_BF16, 64, 16, _blocks(1, 1, 1, 1))
    try:
        assert L.etp_depth_ws_bytes(h, 0) == 0 and L.etp_depth_ws_bytes(h, -1) == 0 and L.etp_depth_ws_bytes(h, 3) > 0
        assert L.etp_depth_ws_bytes(h, 3) % 256 == 0 and L.etp_depth_ws_bytes(h, 6) > L.etp_depth_ws_bytes(h, 3)
        info = _lib.DepthTensorInfo()
        n = L.etp_depth_param_count(h)
        assert L.etp_depth_param_info(h, n, ctypes.byref(info)) == INVALID and L.etp_depth_param_info(h, -1, ctypes.byref(info)) == INVALID
        assert L.etp_depth_param_info(h, 0, None) == INVALID
        buf = torch.zeros(4096, dtype=torch.uint8)
        p = (buf.data_ptr() + 255) // 256 * 256
        assert L.etp_depth_fwd(h, p, 1, p, p, None) == INVALID                      # not bound
        assert L.etp_depth_refresh_weights(h, None) == INVALID
        assert L.etp_depth_bind(h, None, p) == INVALID and L.etp_depth_bind(h, p, None) == INVALID
        assert L.etp_depth_bind(h, p + 16, p) == INVALID and L.etp_depth_bind(h, p, p + 16) == INVALID
        assert L.etp_depth_bind(h, p, p) == 0
        views = (ctypes.c_void_p * 12)(*([p] * 12))
        refused = [L.etp_depth_fwd(h, None, 1, p, p, None), L.etp_depth_fwd(h, p, 0, p, p, None), L.etp_depth_fwd(h, p, 1, None, p, None),
                   L.etp_depth_fwd(h, p, 1, p, None, None), L.etp_depth_fwd(h, p + 4, 1, p, p, None), L.etp_depth_fwd(h, p, 1, p + 4, p, None),
                   L.etp_depth_fwd(h, p, 1, p, p + 16, None), L.etp_depth_fwd_views(h, None, 1, p, p, None),
                   L.etp_depth_fwd_views(h, views, 0, p, p, None), L.etp_depth_fwd_views(h, views, 1, None, p, None),
                   L.etp_depth_set_probe(h, p + 4), L.etp_depth_set_probe(None, p),
                   L.etp_depth_fwd(h, p, 1 << 24, p, p, None)]                      # the im2col rows would pass 2^31 elements
        views[5] = None
        refused.append(L.etp_depth_fwd_views(h, views, 1, p, p, None))
        views[5] = p + 1
        refused.append(L.etp_depth_fwd_views(h, views, 1, p, p, None))
        assert refused == [INVALID] * len(refused), refused
    finally:
        L.etp_depth_destroy(h)
    assert L.etp_depth_param_count(None) == 0 and L.etp_depth_arena_elems(None) == 0 and L.etp_depth_ws_bytes(None, 1) == 0


def test_kernel_entry_refusals_without_launching():
    L = _lib.lib()
    buf = torch.zeros(4096, dtype=torch.uint8)
    p = (buf.data_ptr() + 15) // 16 * 16
    one = (ctypes.c_void_p * 1)(p)
    twelve = (ctypes.c_void_p * 12)(*([p] * 12))
    odd = (ctypes.c_void_p * 12)(*([p] * 11 + [p + 4]))
    hole = (ctypes.c_void_p * 12)(*([p] * 11 + [None]))
    f, b = _lib.ETP_F32, _lib.ETP_BF16
    e = 1e-5
    refused = [
        L.etp_depth_stem(None, 1, 1, 64, 16, p, p, None), L.etp_depth_stem(one, 1, 1, 64, 16, None, p, None),
        L.etp_depth_stem(one, 1, 1, 64, 16, p, None, None), L.etp_depth_stem(one, 1, 1, 64, 16, p, p + 4, None),
        L.etp_depth_stem(one, 1, 1, 64, 16, p + 8, p, None), L.etp_depth_stem(one, 1, 0, 64, 16, p, p, None),
        L.etp_depth_stem(one, 1, 1, 96, 16, p, p, None), L.etp_depth_stem(one, 1, 1, 32, 16, p, p, None),
        L.etp_depth_stem(one, 1, 1, 320, 16, p, p, None), L.etp_depth_stem(one, 1, 1, 64, 24, p, p, None),
        L.etp_depth_stem(one, 2, 1, 64, 16, p, p, None), L.etp_depth_stem(odd, 12, 1, 64, 16, p, p, None),
        L.etp_depth_stem(hole, 12, 1, 64, 16, p, p, None), L.etp_depth_stem(twelve, 12, 1 << 20, 256, 32, p, p, None),
        L.etp_gn_stats(None, p, 1, 4, 16, 8, e, None), L.etp_gn_stats(p, None, 1, 4, 16, 8, e, None),
        L.etp_gn_stats(p + 4, p, 1, 4, 16, 8, e, None), L.etp_gn_stats(p, p, 0, 4, 16, 8, e, None), L.etp_gn_stats(p, p, 1, 0, 16, 8, e, None),
        L.etp_gn_stats(p, p, 1, 4, 18, 2, e, None), L.etp_gn_stats(p, p, 1, 4, 4096, 8, e, None), L.etp_gn_stats(p, p, 1, 4, 16, 3, e, None),
        L.etp_gn_stats(p, p, 1, 4, 256, 128, e, None), L.etp_gn_stats(p, p, 1 << 20, 4096, 1024, 8, e, None),
        L.etp_gn_apply(7, p, p, p, p, 0, None, None, None, None, 1, 0, p, 1, 4, 16, 8, None),
        L.etp_gn_apply(f, None, p, p, p, 0, None, None, None, None, 1, 0, p, 1, 4, 16, 8, None),
        L.etp_gn_apply(f, p, None, p, p, 0, None, None, None, None, 1, 0, p, 1, 4, 16, 8, None),
        L.etp_gn_apply(f, p, p, None, p, 0, None, None, None, None, 1, 0, p, 1, 4, 16, 8, None),
        L.etp_gn_apply(f, p, p, p, None, 0, None, None, None, None, 1, 0, p, 1, 4, 16, 8, None),
        L.etp_gn_apply(f, p, p, p, p, 0, None, None, None, None, 1, 0, None, 1, 4, 16, 8, None),
        L.etp_gn_apply(f, p, p, p, p, 3, p, None, None, None, 1, 0, p, 1, 4, 16, 8, None),
        L.etp_gn_apply(f, p, p, p, p, 1, None, None, None, None, 1, 0, p, 1, 4, 16, 8, None),
        L.etp_gn_apply(f, p, p, p, p, 2, p, None, p, p, 1, 0, p, 1, 4, 16, 8, None),
        L.etp_gn_apply(f, p, p, p, p, 2, p, p, p, None, 1, 0, p, 1, 4, 16, 8, None),
        L.etp_gn_apply(b, p, p, p, p, 1, p + 2, None, None, None, 1, 0, p, 1, 4, 16, 8, None),
        L.etp_gn_apply(b, p, p, p, p, 0, None, None, None, None, 1, 0, p + 8, 1, 4, 16, 8, None),
        L.etp_gn_apply(b, p, p, p, p, 0, None, None, None, None, 1, 0, p, 1, 4, 16, 5, None),
        L.etp_maxpool3x3s2(f, None, p, 1, 4, 4, 16, None), L.etp_maxpool3x3s2(f, p, None, 1, 4, 4, 16, None),
        L.etp_maxpool3x3s2(f, p + 4, p, 1, 4, 4, 16, None), L.etp_maxpool3x3s2(5, p, p, 1, 4, 4, 16, None),
        L.etp_maxpool3x3s2(b, p, p, 0, 4, 4, 16, None), L.etp_maxpool3x3s2(b, p, p, 1, 0, 4, 16, None),
        L.etp_maxpool3x3s2(b, p, p, 1, 4, 4, 12, None), L.etp_maxpool3x3s2(b, p, p, 1 << 16, 256, 256, 16, None),
        L.etp_conv_rows(f, None, p, 1, 4, 4, 16, 3, 1, None), L.etp_conv_rows(f, p, None, 1, 4, 4, 16, 3, 1, None),
        L.etp_conv_rows(f, p, p + 8, 1, 4, 4, 16, 3, 1, None), L.etp_conv_rows(3, p, p, 1, 4, 4, 16, 3, 1, None),
        L.etp_conv_rows(b, p, p, 1, 4, 4, 16, 2, 1, None), L.etp_conv_rows(b, p, p, 1, 4, 4, 16, 5, 1, None),
        L.etp_conv_rows(b, p, p, 1, 4, 4, 16, 3, 3, None), L.etp_conv_rows(b, p, p, 1, 4, 4, 16, 3, 0, None),
        L.etp_conv_rows(b, p, p, 1, 4, 4, 20, 3, 1, None), L.etp_conv_rows(b, p, p, 0, 4, 4, 16, 3, 1, None),
        L.etp_conv_rows(b, p, p, 1 << 12, 256, 256, 16, 3, 1, None),
    ]
    assert refused == [INVALID] * len(refused), refused
    assert L.etp_last_error()


def test_inputs_must_be_float32():
    m = dp.DepthEncoder(device="cpu", dtype=torch.float32, image_size=64, base_planes=16, blocks=(1, 1, 1, 1))
    for bad in (torch.float16, torch.float64, torch.uint8):
        with pytest.raises(TypeError):
            m({"depth": torch.zeros(1, 64, 64, 1, dtype=bad)})
        with pytest.raises(TypeError):
            m.encode_views({f"depth_{a}": torch.zeros(1, 64, 64, 1, dtype=bad) for a in range(12)})


@pytest.mark.skipif(torch.cuda.is_available(), reason="CPU-only check")
def test_compute_fails_loudly_without_gpu():
    m = dp.DepthEncoder(device="cpu", dtype=torch.float32, image_size=64, base_planes=16, blocks=(1, 1, 1, 1))
    img = torch.zeros(1, 64, 64, 1)
    with pytest.raises(_lib.EtpError):
        m({"depth": img})
    with pytest.raises(_lib.EtpError):
        m.encode_views({f"depth_{a}": img for a in range(12)})
    with pytest.raises(_lib.EtpError):
        dp.stem(img, torch.zeros(16, 1, 7, 7), torch.zeros(1, 16, 16, 16))
    with pytest.raises(_lib.EtpError):
        dp.gn_stats(torch.zeros(1, 4, 16), 8)
    with pytest.raises(_lib.EtpError):
        dp.maxpool3x3s2(torch.zeros(1, 4, 4, 16), torch.zeros(1, 2, 2, 16))
    with pytest.raises(_lib.EtpError):
        dp.conv_rows(torch.zeros(1, 4, 4, 16), torch.zeros(16, 144), 3, 1)


class _Recorder:
    """stands for an encoder: records what it is called with and returns a tensor that names the call"""

    def __init__(self, tag, with_views):
        self.tag, self.forward_calls, self.view_calls = tag, [], []
        if with_views:
            self.encode_views = self._encode_views

    def __call__(self, observations):
        self.forward_calls.append(observations)
        return torch.full((1,), self.tag)

    def _encode_views(self, observations):
        self.view_calls.append(observations)
        return torch.full((1,), self.tag + 0.5)


@pytest.mark.parametrize("depth_views", [False, True])
@pytest.mark.parametrize("rgb_views", [False, True])
def test_waypoint_mode_takes_the_depth_encoders_encode_views_when_present(monkeypatch, depth_views, rgb_views):
    """the dispatch of waypoint_mode with stand-in encoders (the GPU test runs it with the real one): an encoder with encode_views gets
    the observation dict as it is and its batch is never built; one without gets the clockwise batch; each side independently"""
    from types import SimpleNamespace
    from etpnav_amd import waypoint as wp
    B = 2
    obs = {}
    for a in range(12):
        suffix = "" if a == 0 else f"_{a * 30.0}"
        obs["rgb" + suffix] = torch.full((B, 2, 2, 3), a, dtype=torch.uint8)
        obs["depth" + suffix] = torch.full((B, 2, 2, 1), float(a))
    seen = {}

    def tail(net, predictor, rgb_embedding, depth_embedding, batch_size, in_train, generator, uniforms):
        seen.update(rgb=rgb_embedding, depth=depth_embedding, batch_size=batch_size)
        return "tail"

    def predictor_and_tail(*a, **k):
        raise AssertionError("the waypoint predictor is not part of this test")

    monkeypatch.setattr(wp, "_waypoint_tail_mode", tail)
    depth_enc, rgb_enc = _Recorder(1.0, depth_views), _Recorder(2.0, rgb_views)
    net = SimpleNamespace(depth_encoder=depth_enc, rgb_encoder=rgb_enc)
    assert wp.waypoint_mode(net, predictor_and_tail, obs, False) == "tail"
    assert seen["batch_size"] == B
    slot_of_view = torch.tensor([(12 - a) % 12 for a in range(12)])
    want = torch.empty(12 * B)
    for a in range(12):
        want[int(slot_of_view[a])::12] = a
    for enc, views, key, got in ((depth_enc, depth_views, "depth", seen["depth"]), (rgb_enc, rgb_views, "rgb", seen["rgb"])):
        if views:
            assert enc.forward_calls == [] and len(enc.view_calls) == 1 and enc.view_calls[0] is obs
            assert float(got) == enc.tag + 0.5
        else:
            assert not hasattr(enc, "encode_views") and len(enc.forward_calls) == 1
            batch = enc.forward_calls[0][key]
            assert batch.shape[0] == 12 * B and torch.equal(batch[:, 0, 0, 0].float(), want)
            assert float(got) == enc.tag
    if depth_views:                                  # depth_batch is never built: no encoder saw a "depth" batch
        assert all("depth" not in o or o is obs for o in rgb_enc.forward_calls)
