"""The pre-training MLM task as one device-side step, straight through the C ABI.

Mirrors ``GlocalTextPathCMTPreTraining.forward(batch, 'mlm')`` + ``.mean()`` + ``backward()``
(pretrain_src/pretrain_src/model/pretrain_cmt.py:141-163, train_r2r.py:240-250): text encoder, panorama encoder over every
trajectory step, node aggregation, ``forward_lang2visn`` through every x-layer, tied MLM head on the masked tokens, mean
token cross-entropy, gradients of every parameter.  The model must be built with ``use_lang2visn_attn=True`` (the
pre-training config, run_pt/r2r_model_config_dep.json).  The SAP task of the same model is ``PlannerStep`` with
``batch['traj']`` (etpnav_amd/step.py).
"""
from __future__ import annotations

import ctypes
import os
import time
from typing import List, Dict, Optional

import torch

from . import _lib
from ._lib import check, ptr
from .planner import GlocalTextPathNavCMT
from .step import N_MLM_INPUTS, _Staging, _destroy_streams, _new_stream

MLM_ERR_COUNT, MLM_ERR_LABEL = 1, 2            # ETP_MLM_ERR_* of include/etpnav_hip.h


class MlmStep(_Staging):
    def __init__(self, model: GlocalTextPathNavCMT, batch: Dict[str, torch.Tensor], dropout=None, drop_seed: int = 0,
                 overlap: bool = True, traj_nodes=None, select: Optional[str] = None, capacity=None):
        """batch: etpnav_amd.synthetic.make_sap_batch layout + ``txt_labels`` [B,L] (-1 = not masked, else the token id).
        dropout: None, "config" (the model config's rates; no drop_env in this task) or (p_hidden, p_attn, p_head, p_env).
        overlap: the three-stream schedule of PlannerStep -- weight gradients on an `aux` stream, the panorama branch
        (forward and backward) on `s2` beside the text branch; False = everything on the caller's stream.
        traj_nodes: as PlannerStep's (node features from the batch's descriptor tables; check_traj()).
        select: where the masked-row gather (and its transpose for the backward) is built -- None / "device": etp_mlm_select
        (csrc/traj_batch.hip) at staging time, on the stream the step runs on, from ``batch.mlm_dev`` (a loader's int32 labels on the
        device with the host-known count) or from one int32 upload of the host ``txt_labels``; check_select() reads what it flagged.
        "host" or ETP_MLM_SELECT=0 (read once, here): torch.nonzero / cumsum on the host and six small uploads.  Same bits.
        capacity: as PlannerStep's, with Nm (the masked tokens) as a sixth key."""
        if not model._engine.cconf.use_lang2visn:
            raise _lib.EtpError("the MLM task needs a model built with use_lang2visn_attn=True (pre-training config)")
        if select not in (None, "device", "host"):
            raise ValueError(f"select: None, 'device' or 'host' (got {select!r})")
        self.select = self._planned_select = "host" if select == "host" or os.environ.get("ETP_MLM_SELECT", "1") == "0" else "device"
        self._stage(model, batch, N_MLM_INPUTS, dropout, drop_seed, 0.0, traj_nodes, capacity)
        # gradient accumulation (PretrainDriver): later micro-steps keep the arena (zero_grads False) and every micro-step's mean
        # loss is scaled by 1 / accumulation steps (train_r2r.py:250-252)
        self.zero_grads, self.loss_scale = True, 1.0
        self.aux, self.s2 = (_new_stream(self.L), _new_stream(self.L)) if overlap else (None, None)

    def _dims_of(self, batch):
        """the batch's dimensions with Nm, the host-known number of masked tokens"""
        d = super()._dims_of(batch)
        md = getattr(batch, "mlm_dev", None) if self.select == "device" else None
        d["Nm"] = int(md["n_masked"]) if md is not None else int((batch["txt_labels"] != -1).sum())
        if d["Nm"] == 0:
            raise ValueError("no masked tokens in the batch")
        return d

    def _byte_buffers(self, d):
        b = super()._byte_buffers(d)
        b.update({"st_mlm": self.L.etp_mlm_stash_bytes(self.eng.handle, d["B"], d["L"], d["G"], d["Nm"]),
                  "ws_mlm": self.L.etp_mlm_ws_bytes(self.eng.handle, d["B"], d["L"], d["G"], d["Nm"])})
        return b

    def _int_arrays(self, d):
        a = super()._int_arrays(d)
        n, Nm = d["B"] * d["L"], d["Nm"]
        a.update({"row_nll": ((Nm,), torch.float32), "row_pred": ((Nm,), torch.int32)})    # run_eval's per-row outputs
        if self.select == "device":
            a.update({"_lab": ((n,), torch.int32), "_rows": ((Nm,), torch.int32), "_ptr_t": ((n + 1,), torch.int32),
                      "labels": ((Nm,), torch.int64), "_arange": ((Nm + 1,), torch.int32), "_ones": ((Nm,), torch.float32),
                      "sel_status": ((2,), torch.int32)})
        return a

    def _bind(self, batch, d):
        """_Staging's, then the batch's selection, on the stream the step runs on"""
        if self.select != self._planned_select:            # the route was switched on a live step: its arrays are another plan's
            self._bound, self._planned_select = None, self.select
        new = super()._bind(batch, d)
        self.Nm = d["Nm"]
        self.dims = (self.B, self.Lt, self.Bp, self.V, self.G, self.eng.cconf.hidden)
        self._select(batch, new)
        return new

    def _select(self, batch, new=()):
        """the selection of `batch`: an input of the step like traj_dev, built when the batch is staged and never inside _enqueue
        (no kernel of the step takes an index from a buffer the step produces).  `new`: the arrays whose allocation is new."""
        Nm = self.Nm
        if self.select == "host":
            self._select_host(batch)
            return
        # arange and ones are written once per allocation, over all of it: the views of a later batch are prefixes
        for k, fill in (("_arange", lambda t: torch.arange(t.numel(), dtype=torch.int32, out=t)), ("_ones", lambda t: t.fill_(1.0))):
            if k in new:
                fill(self._pool[k].view(getattr(self, k).dtype))
        if "sel_status" in new:
            self.sel_status.zero_()
        md = getattr(batch, "mlm_dev", None)
        n = self.B * self.Lt
        if md is not None:
            lab = md["txt_labels"]
            if tuple(lab.shape) != (self.B, self.Lt) or lab.dtype != torch.int32 or not lab.is_contiguous() or \
                    lab.device != self._rows.device:
                raise ValueError(f"mlm_dev['txt_labels'] is a contiguous int32 tensor {(self.B, self.Lt)} on the step's device "
                                 f"(got {tuple(lab.shape)}, {lab.dtype})")
        else:
            lab = self._lab
            lab.copy_(batch["txt_labels"].reshape(-1).to(torch.int32), non_blocking=True)
        self._lab_src = lab                    # taken by reference until the next load, like traj_dev
        self.sel = (self._arange, self._rows, self._ones)
        self.selT = (self._ptr_t, self._arange[:Nm], self._ones)
        cap = self._pool["_rows"].numel() // 4
        check(self.L.etp_mlm_select(ptr(lab), n, self.eng.cconf.vocab, Nm, cap, ptr(self._rows), ptr(self._ptr_t), ptr(self.labels),
                                    ptr(self.sel_status), self.eng.stream()), "mlm_select")

    def _select_host(self, batch):
        """masked positions: row gather of the text (and its transpose for the backward), built on the host"""
        dev, Nm = self.eng.device, self.Nm
        sel = (batch["txt_labels"] != -1).reshape(-1)
        rows = torch.nonzero(sel).reshape(-1).to(torch.int32)
        i32 = lambda x: torch.as_tensor(x, dtype=torch.int32).to(dev)
        self.sel = (i32(torch.arange(Nm + 1)), rows.to(dev), torch.ones(Nm, dtype=torch.float32, device=dev))
        ptr_t = torch.zeros(self.B * self.Lt + 1, dtype=torch.int32)
        ptr_t[1:] = torch.cumsum(sel.to(torch.int32), 0)
        self.selT = (ptr_t.to(dev), i32(torch.arange(Nm)), torch.ones(Nm, dtype=torch.float32, device=dev))
        self.labels = batch["txt_labels"].reshape(-1)[sel].to(torch.int64).contiguous().to(dev)

    def check_select(self) -> None:
        """one device-to-host copy of etp_mlm_select's status words; raises EtpError naming the flags, the count the kernel found and
        the count the step was sized for.  The step itself never synchronises; a step on the host route has nothing to check."""
        if self.select != "device":
            return
        flags, count = (int(x) for x in self.sel_status.cpu().tolist())
        if flags:
            names = [n for n, bit in (("ETP_MLM_ERR_COUNT", MLM_ERR_COUNT), ("ETP_MLM_ERR_LABEL", MLM_ERR_LABEL)) if flags & bit]
            raise _lib.EtpError(f"etp_mlm_select flagged {' | '.join(names)}: {count} entries of txt_labels are masked, the step was "
                                f"sized for n_masked = {self.Nm} (vocabulary {self.eng.cconf.vocab})")

    def close(self):
        self.eng.release_aux()
        _destroy_streams(self.L, self.aux, self.s2)
        self.aux = self.s2 = None

    def run_eager(self, backward: bool = True):
        self.step_no += 1
        try:       # no lazy joins, no d_txt stream (PlannerStep re-installs its own at every enqueue)
            with self.eng.scope(aux=self.aux, aux2=None, lazy=0, drop=self._drop_state()):
                self._enqueue(self.eng.stream(), backward)
        finally:   # the aux stream is this step's own: off the handle on every exit
            self.eng.release_aux()

    def run_eval(self, counters):
        """validate_mlm's loop body (train_r2r.py:362-368) on this batch: the schedule of ``run_eager(backward=False)`` with
        etp_mlm_eval in place of etp_mlm_fwd -- per-row nll / arg-max into ``row_nll`` / ``row_pred``, their sums added to
        `counters` (etpnav_amd.validate.EvalCounters) on the device.  No loss, no dlogits, no host read."""
        self.step_no += 1
        try:
            with self.eng.scope(aux=self.aux, aux2=None, lazy=0, drop=self._drop_state()):
                self._enqueue(self.eng.stream(), False, counters)
        finally:
            self.eng.release_aux()

    def scores(self) -> torch.Tensor:
        """model(batch, task='mlm', compute_loss=False) (train_r2r.py:362): a view [Nm, vocab] of the fp32 logits the last
        run_eager / run_eval left in the stash."""
        off, ldv = ctypes.c_int64(), ctypes.c_int64()
        check(self.L.etp_mlm_stash_logits(self.eng.handle, self.B, self.Lt, self.G, self.Nm, ctypes.byref(off), ctypes.byref(ldv)),
              "mlm_stash_logits")
        n = self.Nm * ldv.value * 4
        return self.st_mlm[off.value:off.value + n].view(torch.float32).view(self.Nm, ldv.value)[:, :self.eng.cconf.vocab]

    def _enqueue(self, s: int, backward: bool, counters=None):
        L, h, i = self.L, self.eng.handle, self.inp
        s2 = self.s2 if self.s2 is not None else s
        B, Lt, G, Nm = self.B, self.Lt, self.G, self.Nm
        # text weights first on the main stream; everything else (panorama / x-layer casts, the gradient memset) rides on the
        # panorama stream, whose join precedes the MLM forward and every backward kernel
        check(L.etp_planner_refresh_part(h, 0, s), "refresh text weights")
        check(L.etp_memset_async(ptr(self.loss), 0, 4, s), "memset loss")
        check(L.etp_stream_after(s, s2), "fork")
        self._refresh_side_weights(s2)
        if backward and self.zero_grads:
            check(L.etp_memset_async(ptr(self.eng.grads), 0, self.eng.grads.numel() * 4, s2), "memset grads")
        self._txt_fwd(s)
        self._pano_fwd(s2)
        check(L.etp_stream_after(s2, s), "join")
        self._assemble(s)
        if counters is not None:
            check(L.etp_mlm_eval(h, ptr(self.txt), ptr(i["txt_masks"]), ptr(i["step_ids"]), ptr(self.gimg), ptr(i["pos"]),
                                 ptr(i["gmask"]), ptr(self.sel[0]), ptr(self.sel[1]), ptr(self.sel[2]), ptr(self.labels), B, Lt, G,
                                 Nm, ptr(self.st_mlm), ptr(self.row_nll), ptr(self.row_pred), counters.ptr(), s), "mlm_eval")
            return
        check(L.etp_mlm_fwd(h, ptr(self.txt), ptr(i["txt_masks"]), ptr(i["step_ids"]), ptr(self.gimg), ptr(i["pos"]),
                            ptr(i["gmask"]), ptr(self.sel[0]), ptr(self.sel[1]), ptr(self.sel[2]), ptr(self.labels), B, Lt, G,
                            Nm, self.loss_scale / Nm, ptr(self.loss), ptr(self.st_mlm), s), "mlm_fwd")
        if not backward:
            return
        check(L.etp_mlm_bwd(h, ptr(self.txt), ptr(i["txt_masks"]), ptr(i["step_ids"]), ptr(i["pos"]), ptr(i["gmask"]),
                            ptr(self.selT[0]), ptr(self.selT[1]), ptr(self.selT[2]), B, Lt, G, Nm, ptr(self.d_txt),
                            ptr(self.d_gimg), ptr(self.st_mlm), ptr(self.ws_mlm), s), "mlm_bwd")
        self._assemble_bwd(s)
        check(L.etp_stream_after(s, s2), "fork")                  # panorama backward beside the text backward
        self._pano_bwd(s2)
        check(L.etp_txt_bwd(h, ptr(self.d_txt), ptr(i["txt_ids"]), ptr(i["txt_masks"]), B, Lt, ptr(self.st_txt), ptr(self.ws_txt),
                            s), "txt_bwd")
        check(L.etp_stream_after(s2, s), "join")


# ---- multi-task driver pieces (what pretrain_src/pretrain_src/data/loader.py:18-75 and train_r2r.py:229-300 provide) -------------
class _TaskSource:
    """One task's stream of batches: a re-iterable (DataLoader, list of batches, ...) that is restarted when it runs dry, after
    telling the owner which epoch begins (DistributedSampler.set_epoch in the reference, loader.py:63-71)."""

    def __init__(self, name: str, batches, weight: float = 1.0, on_epoch=None):
        self.name, self.batches, self.weight, self.on_epoch = name, batches, float(weight), on_epoch
        self.epoch, self._it = 0, iter(batches)

    def take(self):
        try:
            return next(self._it)
        except StopIteration:
            self.epoch += 1
            if self.on_epoch is not None:
                self.on_epoch(self.epoch)
            self._it = iter(self.batches)
            return next(self._it)


class MetaLoader:
    """Task mixing for multi-task pre-training: yields ``(task_name, batch)`` forever; the task is held for ``accum_steps``
    consecutive draws (one gradient-accumulation window trains one task) and windows pick their task with probability
    proportional to the mixing weights -- the contract of the reference's loader (loader.py:54-63).

    Unlike the reference, which draws and (in distributed runs) broadcasts one task id per window from the training loop, the
    schedule here is PLANNED: ``horizon`` windows are drawn in one ``torch.multinomial`` call and rank 0's plan is broadcast
    once, so all ranks walk the same task sequence (the per-task gradient bucket sets of etpnav_amd.dp.task_grad_ranges rely
    on that) without a collective -- and a device round trip on the RCCL backend -- in front of every optimizer step.

    loaders: {name: batches  |  (batches, weight, on_epoch)} with ``batches`` anything ``iter()`` accepts repeatedly."""

    def __init__(self, loaders: Dict, accum_steps: int = 1, distributed: bool = False, device=None, generator=None,
                 horizon: int = 1024):
        if not isinstance(loaders, dict) or not loaders:
            raise ValueError("loaders: a non-empty {task: batches | (batches, weight, on_epoch)} mapping")
        self.sources: List[_TaskSource] = []
        for name, spec in loaders.items():
            batches, weight, on_epoch = spec if isinstance(spec, tuple) else (spec, 1.0, None)
            self.sources.append(_TaskSource(name, batches, weight, on_epoch))
        self.accum_steps, self.distributed, self.device = max(1, int(accum_steps)), bool(distributed), device
        self.generator, self.horizon = generator, int(horizon)
        self._plan: List[int] = []
        self._held, self._left = 0, 0          # task of the running window, draws left in it

    @property
    def names(self) -> List[str]:
        return [s.name for s in self.sources]

    def _extend_plan(self):
        w = torch.tensor([s.weight for s in self.sources], dtype=torch.float32)
        plan = torch.multinomial(w, self.horizon, replacement=True, generator=self.generator)
        if self.distributed:
            import torch.distributed as dist
            t = plan.to(self.device) if self.device is not None else plan
            dist.broadcast(t, 0)
            plan = t.cpu()
        self._plan = plan.tolist()[::-1]       # popped from the end

    def __iter__(self):
        while True:
            if self._left == 0:
                if not self._plan:
                    self._extend_plan()
                self._held, self._left = self._plan.pop(), self.accum_steps
            self._left -= 1
            src = self.sources[self._held]
            yield src.name, src.take()


class PretrainDriver:
    """The multi-task pre-training loop of train_r2r.py:229-300 on the MI355X planner: MetaLoader task mixing -> one
    device-side step of the drawn task (SAP = PlannerStep over trajectories, MLM = MlmStep) -> (multi-GPU) mean of exactly
    the gradient ranges that task writes (etpnav_amd.dp.task_grad_ranges: static per-task bucket sets instead of DDP's
    find_unused_parameters=True, utils/misc.py:58) -> warm-up-linear learning rate (optim/sched.py) -> fused AdamW with the
    reference's decay grouping and gradient clipping (optim/misc.py, optim/adamw.py, train_r2r.py:283-300).

    _step_for picks the step object of every batch.  Fixed SAP steps (their own stash / workspace / streams) are cached per batch
    shape, training and validation apart, and refilled in place; the MLM step is built per batch and released after it (its
    masked-token count changes the buffer plan).  With reuse_steps=True one capacity step object per task serves the whole run
    instead (and one more pair validate()): load_batch of any shape, no synchronise per batch."""

    def __init__(self, model: GlocalTextPathNavCMT, loaders: Dict, learning_rate: float = 5e-5, warmup_steps: int = 10000,
                 num_train_steps: int = 100000, grad_norm: float = 5.0, accum_steps: int = 1, dropout="config", seed: int = 0,
                 distributed: bool = False, max_cached_steps: int = 4, generator=None, max_txt_len: int = 100,
                 reuse_steps: bool = False, batch_size: Optional[int] = None, log_steps: Optional[int] = None, on_log=None):
        """accum_steps = gradient_accumulation_steps of train_r2r.py:231-300: that many consecutive (task, batch) draws (the
        MetaLoader keeps the task fixed over them, loader.py:61-63) each add the gradient of mean-loss / accum_steps to the
        arena, then ONE reduction / clipping / optimizer step follows.  max_txt_len = the dataset's truncation length
        (run_pt/r2r_pretrain_habitat.json: 100): with several ranks the row-sparse word-embedding exchange uses the
        rank-independent capacity B * max_txt_len (the collate pads to the per-batch maximum, so L differs across ranks).
        reuse_steps: one capacity PlannerStep and one capacity MlmStep serve training for the whole run and one more pair serves
        validate() (step.py _Staging: load_batch of any shape), instead of the per-shape cache and the per-batch MlmStep; the initial
        capacity is B = batch_size (default: the loaders' ``batch_size`` attribute, else the first batch) and L = max_txt_len, the rest
        grows on demand.  Nothing synchronises per batch; check_select() / check_traj() run at the validation points and in close().
        log_steps: the training log of train_r2r.py:259-317 on the device (etpnav_amd.trainlog.TrainMeter): every micro-step's loss goes
        into its task's running meter and counters instead of ``task_losses``, every optimizer step's pre-clip gradient norm into the
        step record, and after every log_steps-th optimizer step ONE read -- the only host synchronise of the training route --
        gives the reference's scalars (``loss/{task}``, ``grad_norm``, ``perf/{task}_*_per_s``, plus ``lr`` from the schedule and the
        skip / non-finite counts), appended to ``train_logs`` as (global_step, dict) and handed to on_log(global_step, dict).  None:
        no meter, ``task_losses`` grows by one device scalar per micro-step as before."""
        from .optim import FusedAdamW, WarmupLinearLR
        from . import dp
        if accum_steps < 1:
            raise ValueError("accum_steps must be >= 1")
        self.accum_steps, self.max_txt_len = int(accum_steps), int(max_txt_len)
        self._micro = 0                     # micro-steps since the last optimizer step
        self._touched = []                  # word rows touched by the SAP micro-steps of the current accumulation window
        self.model, self.dropout, self.seed = model, dropout, int(seed)
        self.meta = MetaLoader(loaders, accum_steps=accum_steps, distributed=distributed, device=model._engine.device,
                               generator=generator)
        self.opt = FusedAdamW(model, lr=learning_rate, hf_style=True, betas=(0.9, 0.98), eps=1e-6, weight_decay=0.01,
                              max_grad_norm=grad_norm, no_decay=FusedAdamW.reference_no_decay)
        self.sched = WarmupLinearLR(self.opt, learning_rate, warmup_steps, num_train_steps)
        self.global_step = 0
        self.distributed = distributed
        self._sap = {}                      # shape key -> PlannerStep
        self._sap_eval = {}                 # shape key -> PlannerStep of validate(): no dropout, apart from the training cache
        self._max = max_cached_steps
        self.reuse_steps = bool(reuse_steps)
        self._reused = {}                   # (task, training?) -> the one capacity step object of that role
        if batch_size is None:
            sizes = [getattr(spec[0] if isinstance(spec, tuple) else spec, "batch_size", None) for spec in loaders.values()]
            batch_size = max([int(b) for b in sizes if b], default=0)
        self._capacity = {"L": self.max_txt_len, **({"B": int(batch_size)} if batch_size else {})}
        self.reducers = {}
        if distributed:
            for task in ("sap", "mlm"):
                ranges, sparse = dp.task_grad_ranges(model, task)
                self.reducers[task] = dp.GradReducer(model.flat_grads, ranges, sparse_rows=sparse)
        self.task_losses = {}
        self.lr_history = []
        self.val_logs = []                  # (global_step, dict) of every validation point of run()
        if log_steps is not None and int(log_steps) < 1:
            raise ValueError("log_steps must be >= 1 (or None)")
        self.log_steps, self.on_log = (int(log_steps) if log_steps is not None else None), on_log
        self.train_logs = []                # (global_step, dict) of every log_steps-th optimizer step
        self.meter = None
        if self.log_steps is not None:
            from .trainlog import TrainMeter
            self.meter = TrainMeter(self.meta.names, model._engine.device)

    def _step_for(self, task: str, train: bool, batch):
        """The step object that runs `batch`, loaded with it.  reuse_steps: the one capacity step of (task, training / validation), built
        at the first batch and refilled ever after.  Otherwise SAP: the fixed step of the batch's shape from the training or the
        validation cache (max_cached_steps each, the oldest evicted); MLM: a step of this batch alone, which the caller _release()s."""
        from .step import PlannerStep
        kw = dict(dropout=self.dropout, drop_seed=self.seed) if train else dict(dropout=None)
        kw["capacity"] = self._capacity if self.reuse_steps else None

        def make():
            if task == "sap":
                # accumulate-mode gradients + full zeroing: the pre-training variant carries weights this task does not touch
                return PlannerStep(self.model, batch, zero_grads=train, grad_overwrite=False, **kw)
            return MlmStep(self.model, batch, **kw)

        if self.reuse_steps:
            cache, key = self._reused, (task, train)
        elif task == "sap":
            cache, key = (self._sap if train else self._sap_eval), PlannerStep.batch_shape_key(batch)
        else:
            return make()
        st = cache.get(key)
        if st is None:
            if not self.reuse_steps and len(cache) >= self._max:
                cache.pop(next(iter(cache))).close()
            st = cache[key] = make()
        else:
            st.load_batch(batch)
        return st

    def _release(self, st) -> None:
        """done with a step of one batch alone (the MLM step without reuse_steps): its buffers must be idle before they go"""
        if isinstance(st, MlmStep) and not self.reuse_steps:
            torch.cuda.current_stream().synchronize()
            st.close()

    def check_steps(self) -> None:
        """reuse_steps: what the reused steps' status words hold (check_select / check_traj): one small copy per step object"""
        for st in self._reused.values():
            st.check_traj()
            if isinstance(st, MlmStep):
                st.check_select()

    def train_step(self, name: str, batch) -> torch.Tensor:
        """One micro-step on `batch` of task `name` ('sap...' / 'mlm...': the part before '_' selects the task, as
        train_r2r.py:235); every accum_steps-th call closes the window with the gradient reduction and the optimizer step.
        Returns the device loss tensor of this micro-step, already scaled by 1 / accum_steps as the reference logs it
        (no host sync)."""
        task = name.split("_")[0]
        first = self._micro == 0
        A = self.accum_steps
        if task == "sap":
            st = self._step_for("sap", True, batch)
            st.step_no = self.global_step * A + self._micro
            st.zero_grads = first
            st.loss_scale = 1.0 / (st.B * A)
            st.run_eager()
            if st.Lt > self.max_txt_len and self.distributed:
                raise ValueError(f"instruction length {st.Lt} exceeds max_txt_len={self.max_txt_len} (the exchange capacity)")
            self._touched.append((st.inp["txt_ids"].reshape(-1).clone() if A > 1 else st.inp["txt_ids"].reshape(-1), st.B))
        elif task == "mlm":
            st = self._step_for("mlm", True, batch)
            st.step_no = self.global_step * A + self._micro
            st.zero_grads = first
            st.loss_scale = 1.0 / A
            st.run_eager()
        else:
            raise ValueError(f"unknown task {task!r}: this fork pre-trains with 'mlm' and 'sap' (pretrain_cmt.py:141-163,223-283)")
        loss = st.loss.clone()
        self._micro += 1
        if self.meter is not None:
            self.meter.update(name, st)
        else:
            self.task_losses.setdefault(name, []).append(loss)
        if self._micro < A:
            self._release(st)
            return loss
        if self.distributed:
            red = self.reducers[task]
            for i in range(len(red.ranges)):
                red.reduce_bucket(i)
            if task == "sap":
                ids = torch.cat([t for t, _ in self._touched]) if len(self._touched) > 1 else self._touched[0][0]
                red.reduce_sparse_rows(ids, capacity=sum(b for _, b in self._touched) * self.max_txt_len)
            red.finish()
        self._micro = 0
        self._touched = []
        self.global_step += 1
        self.lr_history.append(self.sched.step(self.global_step))
        self.opt.step()
        if self.meter is not None:
            self._log_point()
        self._release(st)
        return loss

    def _log_point(self) -> None:
        """behind opt.step() on its stream: the step record; at every log_steps-th optimizer step the one read (train_r2r.py:269-317)"""
        if self.opt.max_grad_norm > 0.0 or self.opt.check_finite:      # the norm pass ran (opts.grad_norm != -1, :279)
            self.meter.optimizer_step(self.opt)
        if self.global_step % self.log_steps:
            return
        log = self.meter.read()
        log["lr"] = self.lr_history[-1]
        self.train_logs.append((self.global_step, log))
        if self.on_log is not None:
            self.on_log(self.global_step, log)

    def validate(self, val_loaders: Dict, setname: str = "") -> Dict[str, float]:
        """validate() of train_r2r.py:335-444 (model.eval(): no dropout): for every task of `val_loaders` ({task: batches}) one
        pass over its batches with the loss sum, the correct rows and the row count kept on the device, read once per task
        and summed over the ranks.  -> {'val{setname}_{task}_loss' / '_acc' / '_tok_per_s'} for an MLM task,
        {'..._gloss' / '_gacc' / '_tok_per_s'} for a SAP task.  Parameters, gradients, optimizer state and the training step
        cache are left as they are."""
        from .validate import EvalCounters, sap_eval, sum_over_ranks
        out = {}
        for name in val_loaders:
            if name.split("_")[0] not in ("mlm", "sap"):
                raise ValueError(f"unknown task {name!r}: this fork validates 'mlm' and 'sap' (train_r2r.py:339-346)")
        counters = EvalCounters(self.model._engine.device)
        for name, loader in val_loaders.items():
            task = name.split("_")[0]
            counters.reset()
            t0 = time.time()
            for batch in loader:
                st = self._step_for(task, False, batch)
                if task == "sap":
                    st.run_eager(backward=False)
                    sap_eval(st, counters)
                else:
                    st.run_eval(counters)
                self._release(st)
            loss_sum, n_correct, n_rows = sum_over_ranks(counters.read())
            dt = time.time() - t0
            keys = ("loss", "acc") if task == "mlm" else ("gloss", "gacc")
            log = {keys[0]: loss_sum / n_rows, keys[1]: n_correct / n_rows, "tok_per_s": n_rows / dt}
            out.update({f"val{setname}_{name}_{k}": v for k, v in log.items()})
        self.check_steps()                  # the validation point's check of the training and validation steps' status words
        return out

    def run(self, num_steps: int, valid_steps: Optional[int] = None, val_loaders=None, val2_loaders=None, on_checkpoint=None):
        """num_steps optimizer steps.  With valid_steps, the validation points of train_r2r.py:319-332: after every valid_steps-th
        optimizer step, and once more at the end when the last step was not such a multiple, validate(val_loaders, '_seen'), then
        validate(val2_loaders, '_unseen'), then on_checkpoint(global_step) where the reference saves the model.  The dicts are
        kept in ``self.val_logs`` as (global_step, dict)."""
        it = iter(self.meta)
        out = []
        for _ in range(num_steps * self.accum_steps):       # num_steps OPTIMIZER steps
            name, batch = next(it)
            out.append((name, self.train_step(name, batch)))
            if valid_steps and self._micro == 0 and self.global_step % valid_steps == 0:
                self._validation_point(val_loaders, val2_loaders, on_checkpoint)
        if valid_steps and num_steps > 0 and self.global_step % valid_steps != 0:
            self._validation_point(val_loaders, val2_loaders, on_checkpoint)
        return out

    def _validation_point(self, val_loaders, val2_loaders, on_checkpoint):
        log = {}
        if val_loaders is not None:
            log.update(self.validate(val_loaders, setname="_seen"))
        if val2_loaders is not None:
            log.update(self.validate(val2_loaders, setname="_unseen"))
        self.val_logs.append((self.global_step, log))
        if on_checkpoint is not None:
            on_checkpoint(self.global_step)

    def close(self):
        try:
            if self._reused:
                torch.cuda.synchronize(self.model._engine.device)
                self.check_steps()
        finally:
            for st in list(self._sap.values()) + list(self._sap_eval.values()) + list(self._reused.values()):
                st.close()
            self._sap.clear()
            self._sap_eval.clear()
            self._reused.clear()
