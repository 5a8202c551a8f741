"""Pre-training validation on the device (pretrain_src/pretrain_src/train_r2r.py:335-444): the counters validate_mlm /
validate_sap keep on the host, kept on the device across batches and read once per task.

``EvalCounters`` is the 32-byte record of csrc/eval_tail.hip (``etp_eval_record``); ``sap_eval`` is the SAP tail on a finished
``PlannerStep`` forward; ``sum_over_ranks`` replaces the three ``sum(all_gather(x))`` of the reference with one all-reduce.
``PretrainDriver.validate`` (etpnav_amd/pretrain.py) drives them.
"""
from __future__ import annotations

import struct
from typing import Sequence, Tuple

import torch

from . import _lib
from ._lib import check, ptr

RECORD_BYTES = 32          # {double loss_sum; int64 n_correct; int64 n_rows; int64 n_counted}
SAP_IGNORE = -100          # F.cross_entropy's default ignore_index (train_r2r.py:424)


class EvalCounters:
    """val_loss / n_correct / n_word of train_r2r.py:357-359 (val_gloss / n_gcorrect / n_data, :418-420) as one device record that
    ``etp_eval_accum`` adds to, batch after batch, with no host read in between."""

    def __init__(self, device=None):
        dev = torch.device(device if device is not None else "cuda")
        if dev.type != "cuda":
            raise _lib.EtpError("the validation counters live on an MI355X (cuda/hip device); no CPU fallback exists")
        self.L = _lib.lib()
        self.rec = torch.zeros(RECORD_BYTES // 8, dtype=torch.int64, device=dev)

    def ptr(self) -> int:
        return self.rec.data_ptr()

    def reset(self) -> None:
        self.rec.zero_()

    def read_all(self) -> Tuple[float, int, int, int]:
        """one device-to-host copy -> (loss_sum, n_correct, n_rows, n_counted)"""
        return struct.unpack("<dqqq", self.rec.cpu().numpy().tobytes())

    def read(self) -> Tuple[float, int, int]:
        """one device-to-host copy -> (loss_sum, n_correct, n_rows)"""
        return self.read_all()[:3]


def sap_eval(step, counters: EvalCounters, stream=None) -> None:
    """The statements of validate_sap's loop body (train_r2r.py:424-430) on a PlannerStep whose forward has been enqueued
    (``run_eager(backward=False)``): per-row nll / arg-max of ``step.logits`` against the batch's labels, added to `counters`."""
    L, s = step.L, stream if stream is not None else step.eng.stream()
    labels = step.inp["labels"]
    check(L.etp_sap_eval(ptr(step.logits), ptr(labels), step.B, step.G, SAP_IGNORE, ptr(step.row_nll), ptr(step.row_pred), s),
          "sap_eval")
    check(L.etp_eval_accum(ptr(step.row_nll), ptr(step.row_pred), ptr(labels), step.B, SAP_IGNORE, counters.ptr(), s), "eval_accum")


def sum_over_ranks(values: Sequence[float]) -> Tuple[float, ...]:
    """sum(all_gather(x)) of train_r2r.py:369-371 / :432-436 for all values at once: one all_reduce of a float64 vector when a
    process group exists, the identity otherwise.  Counts stay exact below 2^53."""
    import torch.distributed as dist
    if not (dist.is_available() and dist.is_initialized()) or dist.get_world_size() == 1:
        return tuple(values)
    dev = "cuda" if dist.get_backend() == "nccl" else "cpu"
    t = torch.tensor([float(v) for v in values], dtype=torch.float64, device=dev)
    dist.all_reduce(t)
    return tuple(t.cpu().tolist())
