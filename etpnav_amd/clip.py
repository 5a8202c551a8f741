"""Native CLIP ViT-B/32 view encoder: the mirror of vlnce_baselines/models/encoders/resnet_encoders.py:244-278 (CLIPEncoder, i.e. OpenAI
clip/model.py VisionTransformer under encode_image) on the HIP engine of csrc/clip_engine.hip and the four kernels of csrc/clip.hip.

    patch_rows / tokens / quick_gelu / cls_ln      the four kernels on torch tensors (operator level)
    param_table(dtype, image_size, layers)         [(visual.*-stripped OpenAI name, shape, arena offset)]
    CLIPEncoder(device, dtype, image_size, layers) nn.Module: forward(observations) -> [N, 512] fp32;
                                                   encode_views(observations) -> clockwise [12 B, 512] fp32 in one call

The encoder is frozen and runs in eval() (resnet_encoders.py:259-261): forward only, parameters do not require gradients.
There is no CPU fallback: without the built library, or without a GPU, the compute paths raise.

`from_archive` reads OpenAI's TorchScript archive (ViT-B-32.pt).  That file is not part of this repository and its loading path has been
exercised only with a synthetic state dict of the same keys and shapes (tests/clip_ref.py), never with the real archive.
"""
from __future__ import annotations

from functools import partial

import torch

from . import _lib, arena
from ._lib import check, ptr
from .arena import _edt, _stream

NUM_IMGS, WIDTH, OUT_DIM, PATCH = 12, 768, 512, 32
MEAN = (0.48145466, 0.4578275, 0.40821073)                # resnet_encoders.py:266
STD = (0.26862954, 0.26130258, 0.27577711)
LN_EPS = 1e-5


_require_gpu = partial(arena._require_gpu, kernels="CLIP encoder")
_view_array = partial(arena._view_array, dtype=torch.uint8, channels=3, what="RGB")


# ---- operator level -----------------------------------------------------------------------------------------------------------
def patch_rows(views, out: torch.Tensor) -> torch.Tensor:
    """views: one uint8 tensor [N, S, S, 3] or a list of 12 [B, S, S, 3]; out [N (S/32)^2, 3072] fp32 / bf16 (etp_clip_patch_rows)."""
    views = [views] if isinstance(views, torch.Tensor) else list(views)
    _require_gpu(out, "patch_rows")
    arr = _view_array(views)
    check(_lib.lib().etp_clip_patch_rows(_edt(out.dtype), arr, len(views), views[0].shape[0], views[0].shape[1], ptr(out), _stream()),
          "etp_clip_patch_rows")
    return out


def tokens(prod, class_embedding, pos, gamma, beta, x, N: int, S: int, eps: float = LN_EPS) -> torch.Tensor:
    _require_gpu(x, "tokens")
    check(_lib.lib().etp_clip_tokens(ptr(prod), ptr(class_embedding), ptr(pos), ptr(gamma), ptr(beta), ptr(x), N, S, eps, _stream()),
          "etp_clip_tokens")
    return x


def quick_gelu(x: torch.Tensor) -> torch.Tensor:
    """x * sigmoid(1.702 x) in place (etp_quick_gelu)."""
    _require_gpu(x, "quick_gelu")
    check(_lib.lib().etp_quick_gelu(_edt(x.dtype), ptr(x), x.numel(), _stream()), "etp_quick_gelu")
    return x


def cls_ln(x, gamma, beta, out, N: int, S: int, eps: float = LN_EPS) -> torch.Tensor:
    _require_gpu(out, "cls_ln")
    check(_lib.lib().etp_clip_cls_ln(_edt(out.dtype), ptr(x), ptr(gamma), ptr(beta), ptr(out), N, S, eps, _stream()), "etp_clip_cls_ln")
    return out


# ---- the encoder ----------------------------------------------------------------------------------------------------------------
def _create(L, dtype, image_size, layers):
    h = L.etp_clip_create(_edt(dtype), int(image_size), int(layers))
    if not h:
        raise _lib.EtpError("etp_clip_create: " + L.etp_last_error().decode())
    return h


def param_table(dtype: torch.dtype = torch.float32, image_size: int = 224, layers: int = 12):
    """[(OpenAI state-dict name without "visual.", shape, arena offset)] of the engine; needs the built library, not a GPU."""
    L = _lib.lib()
    h = _create(L, dtype, image_size, layers)
    try:
        return arena.read_table(L, "clip", h, _lib.ClipTensorInfo)
    finally:
        L.etp_clip_destroy(h)


class CLIPEncoder(arena.FrozenArenaModule):
    """resnet_encoders.py:244-278 on the HIP engine.  Parameters are views of one flat fp32 arena under OpenAI CLIP's visual.* names
    (without the prefix), so ``load_state_dict`` is strict under those names and ``load_openai_state_dict`` takes a whole CLIP state
    dict.  image_size and layers exist so that tests can be small; the shipped encoder is (224, 12)."""

    PREFIX, INFO = "clip", _lib.ClipTensorInfo

    def __init__(self, device=None, dtype: torch.dtype = torch.bfloat16, image_size: int = 224, layers: int = 12):
        super().__init__()
        assert dtype in (torch.float32, torch.bfloat16)
        self.image_size, self.layers = int(image_size), int(layers)
        self.tokens = (self.image_size // PATCH) ** 2 + 1
        self.output_shape = (OUT_DIM,)
        self._init_arena(_create(_lib.lib(), dtype, image_size, layers), device, dtype)
        self.eval()

    def _on_move(self):
        self.set_probe(False)

    # ---- loading ----
    def load_openai_state_dict(self, state_dict):
        """A whole CLIP state dict (clip.load(...)[0].state_dict()): keeps visual.*, ignores the text tower; strict on what it keeps.
        fp16 checkpoints (OpenAI's GPU default) are widened to the fp32 arena."""
        vis = {k[len("visual."):]: v.detach().to(torch.float32) for k, v in state_dict.items() if k.startswith("visual.")}
        if not vis:
            raise KeyError("no visual.* keys in the state dict")
        return self.load_state_dict(vis, strict=True)

    @classmethod
    def from_archive(cls, path: str, device=None, dtype: torch.dtype = torch.bfloat16):
        """OpenAI's TorchScript archive (ViT-B-32.pt).  Exercised only with a synthetic state dict: the archive is not in the repository."""
        sd = torch.jit.load(path, map_location="cpu").state_dict()
        enc = cls(device=device, dtype=dtype, image_size=224, layers=12)
        enc.load_openai_state_dict(sd)
        return enc

    # ---- compute ----
    def _prepare(self, N: int):
        _require_gpu(self.arena, "CLIPEncoder")
        return self._scratch(N), torch.empty(N, OUT_DIM, dtype=torch.float32, device=self.arena.device)

    def _check_views(self, views):
        for v in views:
            assert tuple(v.shape[1:]) == (self.image_size, self.image_size, 3), (tuple(v.shape), self.image_size)
            assert v.shape[0] == views[0].shape[0]

    def set_probe(self, on: bool, N: int = 0):
        """Test aid: keep the residual stream after ln_pre, layer 0 and the last layer of the following calls of N images in
        ``self._probe`` [3, N T, 768]."""
        self._probe = torch.zeros(3, N * self.tokens, WIDTH, dtype=torch.float32, device=self.arena.device) if on else None
        check(self.L.etp_clip_set_probe(self.handle, ptr(self._probe)), "etp_clip_set_probe")
        return self._probe

    def forward(self, observations) -> torch.Tensor:
        """resnet_encoders.py:269-278: observations["rgb"] uint8 [N, S, S, 3] -> [N, 512] fp32."""
        _require_gpu(self.arena, "CLIPEncoder")
        rgb = observations["rgb"].to(self.arena.device).contiguous()
        arr = _view_array([rgb])
        self._check_views([rgb])
        N = rgb.shape[0]
        assert self._probe is None or self._probe.shape[1] == N * self.tokens
        ws, out = self._prepare(N)
        check(self.L.etp_clip_fwd(self.handle, arr[0], N, ptr(out), ptr(ws), _stream()), "etp_clip_fwd")
        return out

    def encode_views(self, observations) -> torch.Tensor:
        """The rgb half of Policy_ViewSelection_ETP.py:176-195 in one call: the 12 rgb* tensors of the rollout's observation dict (in
        the dict's order, as the reference walks it) -> [12 B, 512] fp32 with view a of episode b in row (12 - a) % 12 + 12 b."""
        _require_gpu(self.arena, "CLIPEncoder")
        keys = [k.replace("depth", "rgb") for k in observations if "depth" in k] or [k for k in observations if "rgb" in k]
        assert len(keys) == NUM_IMGS, f"expected {NUM_IMGS} views, found {len(keys)}"
        views = [observations[k].to(self.arena.device).contiguous() for k in keys]
        arr = _view_array(views)
        self._check_views(views)
        B = views[0].shape[0]
        assert self._probe is None or self._probe.shape[1] == NUM_IMGS * B * self.tokens
        ws, out = self._prepare(NUM_IMGS * B)
        check(self.L.etp_clip_fwd_views(self.handle, arr, B, ptr(out), ptr(ws), _stream()), "etp_clip_fwd_views")
        return out
