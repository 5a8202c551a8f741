"""What the planner and the three frozen engines (waypoint head, CLIP encoder, depth encoder) share on the Python side: the mirror of
csrc/arena.h.

    read_table(L, prefix, handle, info_cls)             the C parameter table -> [(state-dict name, shape, arena offset)]
    build_tree(module, arena, table, requires_grad)     nn.Parameter views of one flat arena under the reference's module tree
    FrozenArenaModule                                   base of CLIPEncoder, DepthEncoder and BinaryDistPredictorTRM

The planner is trainable (gradient arena, autograd anchor) and uses the two functions only.
"""
from __future__ import annotations

import ctypes
import math
from typing import Dict, List

import torch
import torch.nn as nn

from . import _lib
from ._lib import check, ptr


def _stream() -> int:
    return torch.cuda.current_stream().cuda_stream


def _require_gpu(t: torch.Tensor, what: str, kernels: str):
    if t.device.type != "cuda":
        raise _lib.EtpError(f"{what}: the {kernels} kernels need an MI355X (cuda/hip device); no CPU fallback exists")


def _edt(dtype: torch.dtype) -> int:
    return {torch.float32: _lib.ETP_F32, torch.bfloat16: _lib.ETP_BF16}[dtype]


def _view_array(views: List[torch.Tensor], dtype: torch.dtype, channels: int, what: str):
    """square NHWC observation tensors -> the pointer array of the *_fwd_views entry points"""
    for v in views:
        if v.dtype != dtype:
            raise TypeError(f"{what} observations must be {str(dtype).split('.')[-1]} [*, S, S, {channels}] (got {v.dtype})")
        assert v.is_contiguous() and v.dim() == 4 and v.shape[3] == channels and v.shape[1] == v.shape[2], tuple(v.shape)
    return (ctypes.c_void_p * len(views))(*[v.data_ptr() for v in views])


class _Node(nn.Module):
    """Plain container reproducing the reference's module tree (state-dict names)."""

    def forward(self, *a, **k):  # pragma: no cover
        raise RuntimeError("container module; call the forward of the module that owns the arena")


def read_table(L, prefix: str, handle, info_cls):
    """[(name, shape, offset)] from etp_<prefix>_param_count / _param_info; needs the built library, not a GPU."""
    info = info_cls()
    out = []
    for i in range(getattr(L, f"etp_{prefix}_param_count")(handle)):
        check(getattr(L, f"etp_{prefix}_param_info")(handle, i, ctypes.byref(info)), f"etp_{prefix}_param_info")
        out.append((info.name.decode(), tuple(int(info.shape[k]) for k in range(info.ndim)), int(info.offset)))
    return out


def build_tree(module: nn.Module, arena: torch.Tensor, table, requires_grad: bool) -> List[tuple]:
    """Register every table entry on `module` as an nn.Parameter that is a view of `arena`, under containers named as the
    reference's modules.  -> [(param, offset, numel, shape)]"""
    views = []
    for name, shape, off in table:
        n = math.prod(shape)
        p = nn.Parameter(arena[off:off + n].view(shape), requires_grad=requires_grad)
        *path, leaf = name.split(".")
        mod = module
        for part in path:
            if part not in mod._modules:
                mod.add_module(part, _Node())
            mod = mod._modules[part]
        mod.register_parameter(leaf, p)
        views.append((p, off, n, shape))
    return views


class FrozenArenaModule(nn.Module):
    """A forward-only engine of the library (etp_<PREFIX>_*) as an nn.Module: the handle, the fp32 arena with its parameter views,
    the operand copy of the matrix region (attribute COPY: a bf16 ``shadow`` in bf16 mode, or depth's ``packed`` weights in both
    dtypes), and the scratch cache ``_ws`` keyed by the batch count.  A subclass creates the handle and calls ``_init_arena``."""

    PREFIX = ""
    INFO = _lib.ParamInfo
    COPY = "shadow"
    COPY_IN_F32 = False
    KIND = "encoder"

    def _init_arena(self, handle, device, dtype: torch.dtype):
        self.L = _lib.lib()
        self.handle = handle
        self.compute_dtype = dtype
        self.table = read_table(self.L, self.PREFIX, handle, self.INFO)
        self.total = int(self._fn("arena_elems")(handle))
        self.n_matrix = int(self._fn("matrix_elems")(handle))
        dev = torch.device(device) if device is not None else torch.device("cuda" if torch.cuda.is_available() else "cpu")
        self.arena = torch.zeros(self.total, dtype=torch.float32, device=dev)
        setattr(self, self.COPY, None)
        self._copy_version = -1
        self._ws: Dict[int, torch.Tensor] = {}
        self._probe = None
        self._views = build_tree(self, self.arena, self.table, requires_grad=False)
        self._bind()

    def _fn(self, name: str):
        return getattr(self.L, f"etp_{self.PREFIX}_{name}")

    def __del__(self):
        try:
            if getattr(self, "handle", None):
                self._fn("destroy")(self.handle)
                self.handle = None
        except Exception:
            pass

    def _bind(self):
        if self.arena.device.type != "cuda":
            return
        if self.COPY_IN_F32 or self.compute_dtype == torch.bfloat16:
            setattr(self, self.COPY, torch.zeros(self.n_matrix, dtype=self.compute_dtype, device=self.arena.device))
        check(self._fn("bind")(self.handle, ptr(self.arena), ptr(getattr(self, self.COPY))), f"etp_{self.PREFIX}_bind")
        self._copy_version = -1

    def _on_move(self):
        """what else a subclass drops when the arena changes device (a probe buffer)"""

    def _apply(self, fn, recurse=True):
        new = fn(self.arena)
        if new.dtype != torch.float32:
            raise TypeError(f"the {self.KIND}'s master parameters stay fp32; choose the compute dtype at construction")
        if new.device != self.arena.device:
            with torch.no_grad():
                self.arena = new.contiguous()
                for p, off, n, shape in self._views:
                    p.data = self.arena[off:off + n].view(shape)
                self._ws.clear()
                self._on_move()
                self._bind()
        return self

    def load_state_dict(self, state_dict, strict: bool = True, assign: bool = False):
        r = super().load_state_dict(state_dict, strict=strict, assign=False)
        self._copy_version = -1
        return r

    def _version(self) -> int:
        """Changes whenever a parameter changes through torch.  Views created over the arena share its counter; `.to()` re-points
        them with ``p.data = ...``, which keeps each parameter's OWN counter, so those are part of the key."""
        return self.arena._version + sum(p._version for p, _, _, _ in self._views)

    def refresh_weights(self):
        """Rebuild the operand copy from the fp32 arena (done automatically when a parameter's version counter moved)."""
        check(self._fn("refresh_weights")(self.handle, _stream()), f"etp_{self.PREFIX}_refresh_weights")
        self._copy_version = self._version()

    def _scratch(self, n: int) -> torch.Tensor:
        """Before a forward of batch count n: a current operand copy, and the cached etp_<PREFIX>_ws_bytes(n) buffer."""
        if getattr(self, self.COPY) is not None and self._version() != self._copy_version:
            self.refresh_weights()
        ws = self._ws.get(n)
        if ws is None:
            ws = torch.empty(int(self._fn("ws_bytes")(self.handle, n)), dtype=torch.uint8, device=self.arena.device)
            self._ws[n] = ws
        return ws
