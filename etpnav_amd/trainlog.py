"""The pre-training log on the device (pretrain_src/pretrain_src/train_r2r.py:229-317): what the loop tells the user while it
trains, kept in small device records that launches on the step's stream update and the host reads in one copy every ``log_steps``
optimizer steps -- the training-side twin of etpnav_amd.validate.EvalCounters.

``TrainMeter`` holds one ``etp_train_task_record`` per task (the RunningMeter of utils/logger.py:68-94 fed ``loss.item()`` at
train_r2r.py:259, and the counters n_examples / n_in_units / n_loss_units of :233-234, :246) and one ``etp_train_step_record`` (the
pre-clip grad_norm of :282-290).  ``TensorReport`` is the per-tensor (sum, abs-max, L2, non-finite count) of any float arena with a
``(name, shape, offset)`` table -- the per-parameter norm loop the reference keeps commented out (:286-289), as the fingerprint of
oracle/make_golden.py:69-73 -- deterministic and in double (csrc/trainlog.hip).  ``PretrainDriver(log_steps=...)`` and
``FusedAdamW(norm_route="report")`` drive them.  There is no CPU fallback.
"""
from __future__ import annotations

import ctypes
import math
import struct
import time
from typing import Dict, Iterable, List, Optional, Sequence, Tuple

import torch

from . import _lib
from ._lib import check, ptr

TASK_RECORD_BYTES = 64      # etp_train_task_record {double run_loss, last_loss; int64 n_values, n_skipped, n_examples, n_in_units, n_loss_units, reserved}
STEP_RECORD_BYTES = 64      # etp_train_step_record {double norm_last, norm_max, norm_sum; int64 n_steps, n_nonfinite_steps, first_nonfinite_step, reserved[2]}
TENSOR_RECORD_BYTES = 32    # etp_tensor_record {double sum, sumsq; float absmax; int32 nonfinite; int64 reserved}
TASK_FMT, STEP_FMT, TENSOR_FMT = "<ddqqqqqq", "<dddqqqqq", "<ddfiq"
CHUNK = 16384               # ETP_TENSOR_REPORT_CHUNK


def _device(device, what: str) -> torch.device:
    dev = torch.device(device if device is not None else "cuda")
    if dev.type != "cuda":
        raise _lib.EtpError(f"{what} lives on an MI355X (cuda/hip device); no CPU fallback exists")
    if not torch.cuda.is_available():
        raise _lib.EtpError(f"{what} needs an MI355X (cuda/hip device) and none is visible; no CPU fallback exists")
    return dev


class TrainMeter:
    """task2loss / n_examples / n_in_units / n_loss_units / grad_norm of train_r2r.py:222-225 as one device buffer of
    ``len(task_names) + 1`` records.  ``update`` and ``optimizer_step`` enqueue one small launch each on the engine's stream and never
    synchronise; ``read`` is one device-to-host copy."""

    def __init__(self, task_names: Sequence[str], device=None, smooth: float = 0.99):
        dev = _device(device, "the training meter")
        self.names = list(task_names)
        if not self.names or len(set(self.names)) != len(self.names):
            raise ValueError("task_names: a non-empty list of distinct names")
        if not 0.0 <= float(smooth) < 1.0:
            raise ValueError("smooth must lie in [0, 1)")
        self.smooth = float(smooth)
        self.L = _lib.lib()
        n = len(self.names)
        self.rec = torch.zeros((n + 1) * 8, dtype=torch.int64, device=dev)
        self.rec[n * 8 + 5] = -1                   # first_nonfinite_step: none
        self.start_time = time.time()               # start_time of train_r2r.py:227
        self.raw = None                             # what the last read() copied: ([task tuples], step tuple)

    def ptr(self, name: Optional[str] = None) -> int:
        """address of a task's record; None: the step record's"""
        i = len(self.names) if name is None else self.names.index(name)
        return self.rec.data_ptr() + 64 * i

    def reset(self) -> None:
        self.rec.zero_()
        self.rec[len(self.names) * 8 + 5] = -1
        self.start_time = time.time()

    def update(self, name: str, step, stream=None) -> None:
        """one micro-step of task `name` on `step` (a PlannerStep / MlmStep whose run_eager has been enqueued): its device loss into
        the task's meter, B / the mask bytes / B (SAP) or Nm (MLM) into its counters (train_r2r.py:233-234, :246, :259)"""
        s = stream if stream is not None else step.eng.stream()
        n_loss = getattr(step, "Nm", None)          # loss.size(0): the masked tokens of an MLM step, the batch of a SAP step
        check(self.L.etp_train_meter_loss(ptr(step.loss), self.smooth, ptr(step.inp["txt_masks"]), step.B * step.Lt, step.B,
                                          step.B if n_loss is None else n_loss, self.ptr(name), s), "train_meter_loss")

    def optimizer_step(self, opt, stream=None) -> None:
        """behind ``opt.step()`` on the same stream: the step's pre-clip gradient norm from the optimizer's sumsq / nonfinite pair"""
        s = stream if stream is not None else opt.eng.stream()
        check(self.L.etp_train_meter_step(ptr(opt.sumsq), ptr(opt.nonfinite), self.ptr(None), s), "train_meter_step")

    def read_raw(self) -> Tuple[List[tuple], tuple]:
        """one device-to-host copy -> ([the tasks' records as tuples], the step record as a tuple), field order of the header"""
        b = self.rec.cpu().numpy().tobytes()
        n = len(self.names)
        tasks = [struct.unpack_from(TASK_FMT, b, 64 * i) for i in range(n)]
        self.raw = (tasks, struct.unpack_from(STEP_FMT, b, 64 * n))
        return self.raw

    def read(self) -> Dict[str, float]:
        """one device-to-host copy -> the reference's scalars under the reference's names: ``loss/{task}`` (RunningMeter.val: 0 while
        no value has been taken, train_r2r.py:273-275), ``grad_norm`` (:290), ``perf/{task}_ex_per_s`` / ``_in_per_s`` /
        ``_loss_per_s`` (:302-316, from the counters and the host clock), and ``skipped_losses``, ``nonfinite_steps``,
        ``first_nonfinite_step`` (-1 = none)."""
        tasks, step = self.read_raw()
        dt = max(time.time() - self.start_time, 1e-9)
        out = {}
        for name, r in zip(self.names, tasks):
            out[f"loss/{name}"] = r[0] if r[2] > 0 else 0
        out["grad_norm"] = step[0]
        for name, r in zip(self.names, tasks):
            out[f"perf/{name}_ex_per_s"] = int(r[4] / dt)
            out[f"perf/{name}_in_per_s"] = int(r[5] / dt)
            out[f"perf/{name}_loss_per_s"] = int(r[6] / dt)
        out["skipped_losses"] = sum(r[3] for r in tasks)
        out["nonfinite_steps"], out["first_nonfinite_step"] = step[4], step[5]
        return out


def table_segments(table) -> Tuple[List[str], List[int], List[int]]:
    """an engine's (name, shape, offset) table -> names, offsets, lengths in elements, in ascending offset order"""
    rows = []
    for name, shape, off in table:
        n = 1
        for s in shape:
            n *= int(s)
        rows.append((int(off), n, name))
    rows.sort()
    return [r[2] for r in rows], [r[0] for r in rows], [r[1] for r in rows]


class TensorReport:
    """Per-tensor fingerprint of a float arena laid out by `table` ((name, shape, offset) rows, an engine's ``table``): ``run`` enqueues
    etp_tensor_report, ``read`` is one copy.  `include`: the names whose records enter the totals (default: all).  The same object
    serves any arena of this layout -- gradients and parameters are two calls."""

    def __init__(self, table, arena_len: int, device=None, include: Optional[Iterable[str]] = None):
        dev = _device(device, "the tensor report")
        self.L = _lib.lib()
        self.names, off, ln = table_segments(table)          # segment order: ascending offsets
        self.table_names = [row[0] for row in table]          # the table's own order: what read() and first_nonfinite() follow
        n = len(self.names)
        inc = None if include is None else set(include)
        self.included = [True if inc is None else name in inc for name in self.names]
        plan = ctypes.c_void_p()
        check(self.L.etp_tensor_report_create((ctypes.c_int64 * n)(*off), (ctypes.c_int64 * n)(*ln),
                                              (ctypes.c_uint8 * n)(*[int(b) for b in self.included]), n, int(arena_len),
                                              ctypes.byref(plan)), "tensor_report_create")
        self.plan, self.arena_len = plan, int(arena_len)
        self.records = torch.zeros(n * 4, dtype=torch.int64, device=dev)
        self.sumsq = torch.zeros(1, dtype=torch.float32, device=dev)
        self.nonfinite = torch.zeros(1, dtype=torch.int32, device=dev)

    @property
    def chunks(self) -> int:
        return int(self.L.etp_tensor_report_chunks(self.plan))

    def run(self, arena: torch.Tensor, stream=None, sumsq: Optional[torch.Tensor] = None, nonfinite: Optional[torch.Tensor] = None):
        """enqueue the report over `arena` (fp32, contiguous, this layout's length); the totals are stored into `sumsq` / `nonfinite`
        (default: the object's own pair).  Never synchronises."""
        if arena.dtype != torch.float32 or arena.numel() != self.arena_len or arena.device != self.records.device:
            raise ValueError(f"arena: a contiguous float32 tensor of {self.arena_len} elements on {self.records.device}")
        s = stream if stream is not None else torch.cuda.current_stream().cuda_stream
        check(self.L.etp_tensor_report(self.plan, ptr(arena), ptr(self.records), ptr(self.sumsq if sumsq is None else sumsq),
                                       ptr(self.nonfinite if nonfinite is None else nonfinite), s), "tensor_report")

    def read(self) -> Dict[str, Tuple[float, float, float, int]]:
        """one device-to-host copy -> {name: (sum, absmax, l2, nonfinite)} of the last run, l2 = sqrt(sumsq), in the table's order"""
        b = self.records.cpu().numpy().tobytes()
        seg = {}
        for i, name in enumerate(self.names):
            sm, sq, amax, nf, _ = struct.unpack_from(TENSOR_FMT, b, 32 * i)
            seg[name] = (sm, amax, math.sqrt(sq), nf)
        return {name: seg[name] for name in self.table_names}

    def first_nonfinite(self) -> Optional[str]:
        """the first name of the table whose last record counts a non-finite value, or None (one copy)"""
        for name, r in self.read().items():
            if r[3]:
                return name
        return None

    def close(self) -> None:
        if getattr(self, "plan", None):
            torch.cuda.synchronize(self.records.device)
            self.L.etp_tensor_report_destroy(self.plan)
            self.plan = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass
