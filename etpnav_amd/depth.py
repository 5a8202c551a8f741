"""Native DD-PPO ResNet-50 depth encoder: the mirror of vlnce_baselines/models/encoders/resnet_encoders.py:13-107 (VlnResnetDepthEncoder, i.e.
habitat-lab's rl/ddppo/policy/resnet.py under resnet_policy.py::ResNetEncoder) on the HIP engine of csrc/depth_engine.hip and the kernels
of csrc/depth.hip.

    stem / gn_stats / gn_apply / maxpool3x3s2 / conv_rows     the five kernels on torch tensors (operator level, NHWC)
    param_table(dtype, image_size, base_planes, blocks)       [(state-dict name, shape, arena offset)]
    DepthEncoder(device, dtype, image_size, base_planes, blocks)
                                                              nn.Module: forward({"depth": ...}) -> [N, 128, 4, 4] fp32;
                                                              encode_views(observations) -> clockwise [12 B, 128, 4, 4] in one call

The encoder is frozen (resnet_encoders.py:52-54): forward only, parameters do not require gradients.  There is no CPU fallback: without
the built library, or without a GPU, the compute paths raise.

The real DD-PPO checkpoint (gibson-2plus-resnet50.pth) is not part of this repository and has NOT been loaded here: `from_checkpoint`
and `load_ddppo_state_dict` have seen a synthetic checkpoint of the same keys and shapes only (tests/depth_ref.py).  habitat_baselines is
not installed where this was built either: the architecture is held to a torch restatement of habitat's source (tests/depth_ref.py), not
to habitat's own classes.
"""
from __future__ import annotations

import ctypes
from functools import partial
from typing import Sequence

import torch

from . import _lib, arena
from ._lib import check, ptr
from .arena import _edt, _stream

NUM_IMGS = 12
GN_EPS = 1e-5
DEFAULT_BLOCKS = (3, 4, 6, 3)


_require_gpu = partial(arena._require_gpu, kernels="depth encoder")
_view_array = partial(arena._view_array, dtype=torch.float32, channels=1, what="depth")


# ---- operator level -----------------------------------------------------------------------------------------------------------
def stem(views, weight: torch.Tensor, out: torch.Tensor) -> torch.Tensor:
    """views: one fp32 tensor [N, S, S, 1] or a list of 12 [B, S, S, 1]; weight [bp, 1, 7, 7]; out [N, S/4, S/4, bp] fp32 (etp_depth_stem)."""
    views = [views] if isinstance(views, torch.Tensor) else list(views)
    _require_gpu(out, "stem")
    arr = _view_array(views)
    check(_lib.lib().etp_depth_stem(arr, len(views), views[0].shape[0], views[0].shape[1], weight.shape[0], ptr(weight), ptr(out),
                                    _stream()), "etp_depth_stem")
    return out


def gn_stats(x: torch.Tensor, groups: int, eps: float = GN_EPS) -> torch.Tensor:
    """x [N, HW, C] fp32 -> [N, groups, 2] = mean, 1 / sqrt(var + eps) (etp_gn_stats)."""
    _require_gpu(x, "gn_stats")
    N, HW, C = x.shape
    stats = torch.empty(N, groups, 2, dtype=torch.float32, device=x.device)
    check(_lib.lib().etp_gn_stats(ptr(x), ptr(stats), N, HW, C, groups, eps, _stream()), "etp_gn_stats")
    return stats


def gn_apply(x, stats, gamma, beta, out, relu: bool = False, nchw: bool = False, res=None, res_stats=None, res_gamma=None, res_beta=None):
    """etp_gn_apply: x [N, HW, C] fp32 pre-norm; res None, a finished tensor of out's dtype, or (with res_stats / res_gamma / res_beta) a
    second pre-norm fp32 tensor; out [N, HW, C] fp32 / bf16, or [N, C, HW] fp32 with nchw.  The operand dtype is out's (nchw: res's)."""
    _require_gpu(x, "gn_apply")
    N, HW, C = x.shape
    kind = 0 if res is None else 2 if res_stats is not None else 1
    dt = res.dtype if (nchw and kind == 1) else out.dtype
    check(_lib.lib().etp_gn_apply(_edt(dt), ptr(x), ptr(stats), ptr(gamma), ptr(beta), kind, ptr(res), ptr(res_stats), ptr(res_gamma),
                                  ptr(res_beta), int(relu), int(nchw), ptr(out), N, HW, C, stats.shape[1], _stream()), "etp_gn_apply")
    return out


def maxpool3x3s2(x: torch.Tensor, out: torch.Tensor) -> torch.Tensor:
    """x [N, H, W, C] -> out [N, (H - 1) // 2 + 1, (W - 1) // 2 + 1, C], same dtype (etp_maxpool3x3s2)."""
    _require_gpu(x, "maxpool3x3s2")
    N, H, W, C = x.shape
    check(_lib.lib().etp_maxpool3x3s2(_edt(x.dtype), ptr(x), ptr(out), N, H, W, C, _stream()), "etp_maxpool3x3s2")
    return out


def conv_rows(x: torch.Tensor, out: torch.Tensor, k: int, stride: int) -> torch.Tensor:
    """x [N, H, W, C] -> out [N Ho Wo, k k C], same dtype, columns (ky, kx, c) (etp_conv_rows)."""
    _require_gpu(x, "conv_rows")
    N, H, W, C = x.shape
    check(_lib.lib().etp_conv_rows(_edt(x.dtype), ptr(x), ptr(out), N, H, W, C, k, stride, _stream()), "etp_conv_rows")
    return out


# ---- the encoder ----------------------------------------------------------------------------------------------------------------
def _create(L, dtype, image_size, base_planes, blocks: Sequence[int]):
    if len(blocks) != 4:
        raise _lib.EtpError("etp_depth_create: four block counts are needed")
    arr = (ctypes.c_int * 4)(*[int(b) for b in blocks])
    h = L.etp_depth_create(_edt(dtype), int(image_size), int(base_planes), arr)
    if not h:
        raise _lib.EtpError("etp_depth_create: " + L.etp_last_error().decode())
    return h


def param_table(dtype: torch.dtype = torch.float32, image_size: int = 256, base_planes: int = 32, blocks: Sequence[int] = DEFAULT_BLOCKS):
    """[(state-dict name, shape, arena offset)] of the engine; needs the built library, not a GPU."""
    L = _lib.lib()
    h = _create(L, dtype, image_size, base_planes, blocks)
    try:
        return arena.read_table(L, "depth", h, _lib.DepthTensorInfo)
    finally:
        L.etp_depth_destroy(h)


class DepthEncoder(arena.FrozenArenaModule):
    """resnet_encoders.py:13-107 on the HIP engine.  Parameters are frozen views of one flat fp32 arena under the names of
    VlnResnetDepthEncoder.visual_encoder's state dict (backbone.conv1.0.weight ... compression.1.bias), so ``load_state_dict`` is strict
    under those names and ``load_ddppo_state_dict`` takes a DD-PPO checkpoint's state dict.  image_size, base_planes and blocks exist so
    that tests can be small; the shipped encoder is (256, 32, (3, 4, 6, 3))."""

    PREFIX, INFO, COPY, COPY_IN_F32 = "depth", _lib.DepthTensorInfo, "packed", True

    def __init__(self, device=None, dtype: torch.dtype = torch.bfloat16, image_size: int = 256, base_planes: int = 32,
                 blocks: Sequence[int] = DEFAULT_BLOCKS):
        super().__init__()
        assert dtype in (torch.float32, torch.bfloat16)
        self.image_size, self.base_planes, self.blocks = int(image_size), int(base_planes), tuple(blocks)
        self._init_arena(_create(_lib.lib(), dtype, image_size, base_planes, blocks), device, dtype)
        fs = self.image_size // 64
        self.output_shape = (int(self.L.etp_depth_out_channels(self.handle)), fs, fs)
        self.eval()

    def _on_move(self):
        self.set_probe(False)

    # ---- loading ----
    def load_ddppo_state_dict(self, state_dict):
        """A DD-PPO checkpoint's state dict (torch.load(path)["state_dict"]), filtered as resnet_encoders.py:40-50 does: of every key
        the parts from the third on are kept when the first of them is "visual_encoder" (actor_critic.net.visual_encoder.backbone... ->
        backbone...); strict on what is kept."""
        kept = {}
        for k, v in state_dict.items():
            parts = k.split(".")[2:]
            if len(parts) > 1 and parts[0] == "visual_encoder":
                kept[".".join(parts[1:])] = v.detach().to(torch.float32)
        if not kept:
            raise KeyError("no *.*.visual_encoder.* keys in the state dict")
        return self.load_state_dict(kept, strict=True)

    @classmethod
    def from_checkpoint(cls, path: str, device=None, dtype: torch.dtype = torch.bfloat16):
        """A DD-PPO checkpoint file (gibson-2plus-resnet50.pth).  Exercised only with a synthetic checkpoint: the file is not in the
        repository."""
        ckpt = torch.load(path, map_location="cpu")
        enc = cls(device=device, dtype=dtype)
        enc.load_ddppo_state_dict(ckpt["state_dict"])
        return enc

    # ---- compute ----
    def _prepare(self, N: int):
        _require_gpu(self.arena, "DepthEncoder")
        return self._scratch(N), torch.empty(N, *self.output_shape, dtype=torch.float32, device=self.arena.device)

    def _check_views(self, views):
        for v in views:
            assert tuple(v.shape[1:]) == (self.image_size, self.image_size, 1), (tuple(v.shape), self.image_size)
            assert v.shape[0] == views[0].shape[0]

    def probe_sizes(self, N: int):
        """element counts of the three probed activations (after the max-pool, layer1, layer4) for N images, NHWC"""
        h, bp = self.image_size // 8, self.base_planes
        return [N * h * h * bp, N * h * h * 4 * bp, N * (h // 8) ** 2 * 32 * bp]

    def set_probe(self, on: bool, N: int = 0):
        """Test aid: keep the activations after the max-pool, after layer1 and after layer4 of the following calls of N images in
        ``self._probe`` (fp32, NHWC, back to back; see probe_sizes)."""
        self._probe = torch.zeros(sum(self.probe_sizes(N)), dtype=torch.float32, device=self.arena.device) if on else None
        check(self.L.etp_depth_set_probe(self.handle, ptr(self._probe)), "etp_depth_set_probe")
        return self._probe

    def forward(self, observations) -> torch.Tensor:
        """resnet_encoders.py:77-107: observations["depth"] fp32 [N, S, S, 1] -> [N, 128, 4, 4] fp32; observations["depth_features"]
        passes through (:83-84)."""
        if "depth_features" in observations:
            return observations["depth_features"]
        depth = observations["depth"]
        if depth.dtype != torch.float32:
            raise TypeError(f"depth observations must be float32 [*, S, S, 1] (got {depth.dtype})")
        _require_gpu(self.arena, "DepthEncoder")
        depth = depth.to(self.arena.device).contiguous()
        arr = _view_array([depth])
        self._check_views([depth])
        N = depth.shape[0]
        assert self._probe is None or self._probe.numel() == sum(self.probe_sizes(N))
        ws, out = self._prepare(N)
        check(self.L.etp_depth_fwd(self.handle, arr[0], N, ptr(out), ptr(ws), _stream()), "etp_depth_fwd")
        return out

    def encode_views(self, observations) -> torch.Tensor:
        """The depth half of Policy_ViewSelection_ETP.py:176-194 in one call: the 12 depth* tensors of the rollout's observation dict (in
        the dict's order, as the reference walks it) -> [12 B, 128, 4, 4] fp32 with view a of episode b in row (12 - a) % 12 + 12 b."""
        keys = [k for k in observations if "depth" in k]
        assert len(keys) == NUM_IMGS, f"expected {NUM_IMGS} views, found {len(keys)}"
        for k in keys:
            if observations[k].dtype != torch.float32:
                raise TypeError(f"depth observations must be float32 [*, S, S, 1] (got {observations[k].dtype} for {k})")
        _require_gpu(self.arena, "DepthEncoder")
        views = [observations[k].to(self.arena.device).contiguous() for k in keys]
        arr = _view_array(views)
        self._check_views(views)
        B = views[0].shape[0]
        assert self._probe is None or self._probe.numel() == sum(self.probe_sizes(NUM_IMGS * B))
        ws, out = self._prepare(NUM_IMGS * B)
        check(self.L.etp_depth_fwd_views(self.handle, arr, B, ptr(out), ptr(ws), _stream()), "etp_depth_fwd_views")
        return out
