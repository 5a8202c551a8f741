"""Write tests/golden/train_log_small.npz from the REAL RunningMeter class and the real torch.nn.utils.clip_grad_norm_ (needs the
reference tree: /root/reference, or $ETP_REFERENCE).

    python tools/make_golden_train_log.py

pretrain_src/pretrain_src/utils/logger.py is imported as it stands; `tensorboardX`, which it imports at module level and the meter
never touches, is replaced by an empty module when it is not installed.  The file holds data only:

  meter/task      [n] int64     which of the two interleaved tasks' meters took call i (train_r2r.py:259)
  meter/loss      [n] float32   the value handed in, as `loss.item()` of an fp32 loss (so float(loss) is what the meter saw)
  meter/val       [n] float64   that meter's _val after the call (0 where it is still None)
  meter/has       [n] int64     0 where _val is still None
  meter/reported  [n] float64   the meter's .val property after the call (logger.py:86-90)
  grads/{s}/{j}   float32       three small gradient sets; grads/{s}/norm = clip_grad_norm_'s returned total norm (fp32),
  grads/{s}/max_norm            and the max_norm it was called with

The values: ordinary losses, exact repeats, a NaN as the very first value of task 1, a NaN in mid-stream, and +inf followed by -inf
(the smoothed value of the second is inf - inf = NaN: it is skipped and the meter stays at +inf).
"""
import importlib.util
import os
import sys
import types

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
REF = os.environ.get("ETP_REFERENCE", "/root/reference")

from tests import trainlog_ref as tr      # noqa: E402


def running_meter():
    try:
        import tensorboardX  # noqa: F401
    except ImportError:
        sys.modules["tensorboardX"] = types.ModuleType("tensorboardX")
    spec = importlib.util.spec_from_file_location("etp_ref_logger", os.path.join(REF, "pretrain_src", "pretrain_src", "utils", "logger.py"))
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    return m.RunningMeter


def main():
    RunningMeter = running_meter()
    rng = np.random.RandomState(5)
    n = 44
    task = rng.randint(0, 2, n)
    task[:4] = [0, 1, 0, 1]
    loss = (2.5 + rng.standard_normal(n) * 0.7).astype(np.float32)
    loss[1] = np.nan                    # the very first value of task 1
    loss[8] = loss[6] = loss[4]         # exact repeats (task 0 takes 4, 6, 8 only if drawn so; the values repeat either way)
    loss[15] = np.nan
    t0 = [i for i in range(33, n) if task[i] == 0]
    loss[t0[0]], loss[t0[1]] = np.inf, -np.inf      # consecutive calls of task 0: inf taken, then inf - inf = NaN skipped
    loss[t0[2]] = 1.0                                # inf stays: 1*(1-sm) + inf*sm
    meters = [RunningMeter("loss/mlm"), RunningMeter("loss/sap")]
    val, has, rep = np.zeros(n), np.zeros(n, dtype=np.int64), np.zeros(n)
    for i in range(n):
        m = meters[task[i]]
        m(torch.tensor(loss[i]).item())             # loss.item() of an fp32 tensor
        has[i] = int(m._val is not None)
        val[i] = m._val if m._val is not None else 0.0
        rep[i] = m.val
    z = {"meter/task": task.astype(np.int64), "meter/loss": loss, "meter/val": val, "meter/has": has, "meter/reported": rep,
         "meter/smooth": np.float64(meters[0]._sm)}
    g = torch.Generator().manual_seed(11)
    for s, (shapes, scale, max_norm) in enumerate([([(7,), (3, 5), (64,)], 1.0, 5.0), ([(1,), (129,), (4, 4, 4)], 30.0, 5.0),
                                                   ([(33,), (2, 2)], 1e-3, 1.0)]):
        params = []
        for j, shp in enumerate(shapes):
            p = torch.nn.Parameter(torch.zeros(shp))
            p.grad = torch.randn(shp, generator=g) * scale
            z[f"grads/{s}/{j}"] = p.grad.numpy().copy()
            params.append(p)
        norm = torch.nn.utils.clip_grad_norm_(params, max_norm)
        z[f"grads/{s}/norm"] = np.float32(norm.item())
        z[f"grads/{s}/max_norm"] = np.float64(max_norm)
        print("gradient set", s, "norm", float(norm))
    np.savez_compressed(tr.GOLDEN, **z)
    print("wrote", tr.GOLDEN, os.path.getsize(tr.GOLDEN), "bytes; skipped calls:", int((np.isnan(loss)).sum()) + 1)


if __name__ == "__main__":
    main()
