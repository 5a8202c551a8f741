"""CPU-side checks of the CLIP view encoder's boundary (in the style of tests/test_waypoint_boundary_cpu.py): the new symbols are
exported, the engine's parameter table is OpenAI CLIP's visual.* key list with its shapes (152 tensors, 87 849 216 parameters at
(224, 12)), the module's parameters are views of one arena and load strictly, every refusal of the create call and of the host-checked
entry points, and the package fails loudly without a GPU.  No kernel is launched here."""
import ctypes

import numpy as np
import pytest
import torch

from etpnav_amd import _lib
from etpnav_amd import clip as cl
from tests import clip_ref as cr

NEW = ("etp_clip_patch_rows", "etp_clip_tokens", "etp_quick_gelu", "etp_clip_cls_ln", "etp_clip_create", "etp_clip_destroy",
       "etp_clip_param_count", "etp_clip_param_info", "etp_clip_arena_elems", "etp_clip_matrix_elems", "etp_clip_bind",
       "etp_clip_refresh_weights", "etp_clip_ws_bytes", "etp_clip_fwd", "etp_clip_fwd_views", "etp_clip_set_probe")
INVALID = -1


def test_new_symbols_are_declared_and_exported():
    L = _lib.lib()
    names = _lib.declared_symbols()
    for n in NEW:
        assert n in names and hasattr(L, n), n


def test_parameter_table_is_openai_clips_visual_tower():
    for dtype in (torch.float32, torch.bfloat16):
        table = cl.param_table(dtype, 224, 12)
        assert len(table) == 152
        assert [(n, s) for n, s, _ in table] == cr.param_shapes(224, 12)
        assert sum(int(np.prod(s)) for _, s, _ in table) == 87849216
        spans = sorted((off, int(np.prod(s))) for _, s, off in table)
        assert all(a + n <= b for (a, n), (b, _) in zip(spans, spans[1:])) and all(a % 64 == 0 for a, _ in spans)
    d = dict((n, s) for n, s, _ in table)
    assert d["conv1.weight"] == (768, 3, 32, 32) and d["proj"] == (768, 512) and d["positional_embedding"] == (50, 768)
    assert d["transformer.resblocks.11.attn.in_proj_weight"] == (2304, 768)
    small = cl.param_table(torch.float32, 64, 2)
    assert [(n, s) for n, s, _ in small] == cr.param_shapes(64, 2) and len(small) == 8 + 24


def test_module_tree_loads_strictly():
    m = cl.CLIPEncoder(device="cpu", dtype=torch.float32, image_size=64, layers=2)
    assert list(m.state_dict().keys()) == [k for k, _ in cr.param_shapes(64, 2)]
    W = cr.make_weights(64, 2, 2)
    m.load_state_dict(W, strict=True)
    for k, v in m.state_dict().items():
        assert torch.equal(v, W[k]), k
    short = dict(W)
    del short["ln_post.bias"]
    with pytest.raises(RuntimeError):
        m.load_state_dict(short, strict=True)
    with pytest.raises(RuntimeError):
        m.load_state_dict(dict(W, extra=torch.zeros(1)), strict=True)
    # every parameter is a view of the one arena; the matrices lead it (the bf16 shadow region), everything fp32-only follows
    base, sd = m.arena.data_ptr(), dict(m.named_parameters())
    for k, p in sd.items():
        off = (p.data_ptr() - base) // 4
        assert 0 <= off and off + p.numel() <= m.total and off % 64 == 0, k
        is_matrix = k == "proj" or (k.endswith("weight") and p.dim() >= 2)
        assert (off < m.n_matrix) == is_matrix, k
    assert all(not p.requires_grad for p in m.parameters()) and not m.training


def test_openai_state_dict_keeps_visual_and_ignores_the_text_tower():
    m = cl.CLIPEncoder(device="cpu", dtype=torch.float32, image_size=32, layers=1)
    W = cr.make_weights(32, 1, 3)
    full = {"visual." + k: v.to(torch.float16) for k, v in W.items()}
    full.update({"token_embedding.weight": torch.zeros(4, 4), "logit_scale": torch.zeros(()), "transformer.resblocks.0.ln_1.weight": torch.ones(3)})
    m.load_openai_state_dict(full)
    for k, v in m.state_dict().items():
        assert torch.equal(v, W[k].to(torch.float16).to(torch.float32)), k
    del full["visual.proj"]
    with pytest.raises(RuntimeError):
        m.load_openai_state_dict(full)
    with pytest.raises(KeyError):
        m.load_openai_state_dict({"token_embedding.weight": torch.zeros(4, 4)})


def test_create_refusals():
    L = _lib.lib()
    for args in ((7, 224, 12), (0, 0, 12), (0, 16, 12), (0, 48, 12), (0, 256, 12), (0, 224, 0), (0, 224, 13), (0, -32, 1)):
        assert not L.etp_clip_create(*args), args
        assert b"etp_clip_create" in L.etp_last_error()
    for S in range(32, 225, 32):
        h = L.etp_clip_create(1, S, 1)
        assert h and L.etp_clip_param_count(h) == 20
        L.etp_clip_destroy(h)


def test_engine_refusals_without_launching():
    L = _lib.lib()
    h = L.etp_clip_create(_lib.ETP_BF16, 64, 2)
    try:
        assert L.etp_clip_ws_bytes(h, 0) == 0 and L.etp_clip_ws_bytes(h, -1) == 0 and L.etp_clip_ws_bytes(h, 3) > 0
        assert L.etp_clip_ws_bytes(h, 3) % 256 == 0 and L.etp_clip_ws_bytes(h, 6) > L.etp_clip_ws_bytes(h, 3)
        info = _lib.ClipTensorInfo()
        assert L.etp_clip_param_info(h, 32, ctypes.byref(info)) == INVALID and L.etp_clip_param_info(h, -1, ctypes.byref(info)) == INVALID
        assert L.etp_clip_param_info(h, 0, None) == INVALID
        buf = torch.zeros(4096, dtype=torch.uint8)
        p = (buf.data_ptr() + 255) // 256 * 256
        assert L.etp_clip_fwd(h, p, 1, p, p, None) == INVALID                      # not bound
        assert L.etp_clip_refresh_weights(h, None) == INVALID
        assert L.etp_clip_bind(h, None, p) == INVALID and L.etp_clip_bind(h, p, None) == INVALID      # bf16 needs a shadow
        assert L.etp_clip_bind(h, p + 16, p) == INVALID and L.etp_clip_bind(h, p, p + 16) == INVALID
        assert L.etp_clip_bind(h, p, p) == 0
        views = (ctypes.c_void_p * 12)(*([p] * 12))
        refused = [L.etp_clip_fwd(h, None, 1, p, p, None), L.etp_clip_fwd(h, p, 0, p, p, None), L.etp_clip_fwd(h, p, 1, None, p, None),
                   L.etp_clip_fwd(h, p, 1, p, None, None), L.etp_clip_fwd(h, p + 4, 1, p, p, None), L.etp_clip_fwd(h, p, 1, p + 4, p, None),
                   L.etp_clip_fwd(h, p, 1, p, p + 16, None), L.etp_clip_fwd_views(h, None, 1, p, p, None),
                   L.etp_clip_fwd_views(h, views, 0, p, p, None), L.etp_clip_fwd_views(h, views, 1, None, p, None),
                   L.etp_clip_set_probe(h, p + 4), L.etp_clip_set_probe(None, p)]
        views[5] = None
        refused.append(L.etp_clip_fwd_views(h, views, 1, p, p, None))
        views[5] = p + 1
        refused.append(L.etp_clip_fwd_views(h, views, 1, p, p, None))
        assert refused == [INVALID] * len(refused), refused
    finally:
        L.etp_clip_destroy(h)
    assert L.etp_clip_param_count(None) == 0 and L.etp_clip_arena_elems(None) == 0 and L.etp_clip_ws_bytes(None, 1) == 0


def test_kernel_entry_refusals_without_launching():
    L = _lib.lib()
    buf = torch.zeros(4096, dtype=torch.uint8)
    p = (buf.data_ptr() + 15) // 16 * 16
    one = (ctypes.c_void_p * 1)(p)
    twelve = (ctypes.c_void_p * 12)(*([p] * 12))
    odd = (ctypes.c_void_p * 12)(*([p] * 11 + [p + 1]))
    hole = (ctypes.c_void_p * 12)(*([p] * 11 + [None]))
    f, b = _lib.ETP_F32, _lib.ETP_BF16
    refused = [
        L.etp_clip_patch_rows(f, None, 1, 1, 32, p, None), L.etp_clip_patch_rows(f, one, 1, 1, 32, None, None),
        L.etp_clip_patch_rows(f, one, 1, 1, 32, p + 8, None), L.etp_clip_patch_rows(7, one, 1, 1, 32, p, None),
        L.etp_clip_patch_rows(f, one, 1, 0, 32, p, None), L.etp_clip_patch_rows(f, one, 1, -3, 32, p, None),
        L.etp_clip_patch_rows(b, one, 1, 1, 0, p, None), L.etp_clip_patch_rows(b, one, 1, 1, 48, p, None),
        L.etp_clip_patch_rows(b, one, 1, 1, 256, p, None), L.etp_clip_patch_rows(b, one, 2, 1, 32, p, None),
        L.etp_clip_patch_rows(b, odd, 12, 1, 32, p, None), L.etp_clip_patch_rows(b, hole, 12, 1, 32, p, None),
        L.etp_clip_tokens(None, p, p, p, p, p, 1, 32, 1e-5, None), L.etp_clip_tokens(p, None, p, p, p, p, 1, 32, 1e-5, None),
        L.etp_clip_tokens(p, p, None, p, p, p, 1, 32, 1e-5, None), L.etp_clip_tokens(p, p, p, None, p, p, 1, 32, 1e-5, None),
        L.etp_clip_tokens(p, p, p, p, None, p, 1, 32, 1e-5, None), L.etp_clip_tokens(p, p, p, p, p, None, 1, 32, 1e-5, None),
        L.etp_clip_tokens(p + 4, p, p, p, p, p, 1, 32, 1e-5, None), L.etp_clip_tokens(p, p, p, p, p, p + 8, 1, 32, 1e-5, None),
        L.etp_clip_tokens(p, p, p, p, p, p, 0, 32, 1e-5, None), L.etp_clip_tokens(p, p, p, p, p, p, 1, 33, 1e-5, None),
        L.etp_clip_tokens(p, p, p, p, p, p, 1, 288, 1e-5, None),
        L.etp_quick_gelu(f, None, 8, None), L.etp_quick_gelu(f, p + 4, 8, None), L.etp_quick_gelu(f, p, 0, None),
        L.etp_quick_gelu(f, p, 12, None), L.etp_quick_gelu(b, p, -8, None), L.etp_quick_gelu(5, p, 8, None),
        L.etp_clip_cls_ln(f, None, p, p, p, 1, 32, 1e-5, None), L.etp_clip_cls_ln(f, p, None, p, p, 1, 32, 1e-5, None),
        L.etp_clip_cls_ln(f, p, p, None, p, 1, 32, 1e-5, None), L.etp_clip_cls_ln(f, p, p, p, None, 1, 32, 1e-5, None),
        L.etp_clip_cls_ln(b, p, p, p, p + 2, 1, 32, 1e-5, None), L.etp_clip_cls_ln(b, p, p, p, p, 0, 32, 1e-5, None),
        L.etp_clip_cls_ln(b, p, p, p, p, 1, 16, 1e-5, None), L.etp_clip_cls_ln(9, p, p, p, p, 1, 32, 1e-5, None),
    ]
    assert refused == [INVALID] * len(refused), refused
    assert L.etp_last_error()


@pytest.mark.skipif(torch.cuda.is_available(), reason="CPU-only check")
def test_compute_fails_loudly_without_gpu():
    m = cl.CLIPEncoder(device="cpu", dtype=torch.float32, image_size=32, layers=1)
    img = torch.zeros(1, 32, 32, 3, dtype=torch.uint8)
    with pytest.raises(_lib.EtpError):
        m({"rgb": img})
    with pytest.raises(_lib.EtpError):
        m.encode_views({f"rgb_{a}": img for a in range(12)})
    with pytest.raises(_lib.EtpError):
        cl.quick_gelu(torch.zeros(8))
    with pytest.raises(_lib.EtpError):
        cl.patch_rows(img, torch.zeros(1, 3072))


def test_waypoint_mode_takes_encode_views_only_when_present():
    import inspect
    from etpnav_amd import waypoint as wp
    src = inspect.getsource(wp.waypoint_mode)
    assert 'hasattr(net.rgb_encoder, "encode_views")' in src
    assert hasattr(cl.CLIPEncoder, "encode_views") and not hasattr(torch.nn.Identity(), "encode_views")
