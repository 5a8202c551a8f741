"""One whole planner training step (the unit of BASELINE.json's metric) driven straight through the C ABI.

``PlannerStep`` keeps every buffer in allocations of its own (sized by its first batch, or grow-only with ``capacity``) and runs

    weight refresh (bf16) -> zero grads -> forward_txt -> forward_panorama -> node assembly (gather-mean)
    -> forward_navigation -> cross-entropy(sum)/B -> backward of all of it into the flat gradient arena

mirroring one rollout step of ss_trainer_ETP.py:801-892 plus the backward of :504.  Nothing is
allocated or synchronised inside ``run_eager`` so the step can be captured into one hipGraph
(``capture()`` / ``replay()``) — launch-bound inner loops replay from the graph instead of being re-issued.
"""
from __future__ import annotations

import ctypes
import os
from typing import Dict, Optional

import torch

from . import _lib
from ._lib import check, ptr
from .planner import GlocalTextPathNavCMT, _cfg_get, config_dropout_rates


def build_node_csr(view_lens: torch.Tensor, V: int, G: int):
    """CSR (and its transpose) of the benchmark node assembly: node 0 = [stop] (empty), node 1 = mean of the valid
    views (ss_trainer_ETP.py:838-839), node g>=2 = view (g-2) mod view_len (one-occurrence ghost nodes,
    graph_utils.py:224-234).  Host-side index bookkeeping only (the reference does this in Python too)."""
    B = view_lens.numel()
    vl = [int(x) for x in view_lens.tolist()]
    ptr_f, idx_f, w_f = [0], [], []
    rev = [[] for _ in range(B * V)]
    for b in range(B):
        for g in range(G):
            n = b * G + g
            if g == 1:
                for v in range(vl[b]):
                    idx_f.append(b * V + v); w_f.append(1.0 / vl[b]); rev[b * V + v].append((n, 1.0 / vl[b]))
            elif g >= 2:
                v = (g - 2) % vl[b]
                idx_f.append(b * V + v); w_f.append(1.0); rev[b * V + v].append((n, 1.0))
            ptr_f.append(len(idx_f))
    ptr_b, idx_b, w_b = [0], [], []
    for r in rev:
        for n, w in r:
            idx_b.append(n); w_b.append(w)
        ptr_b.append(len(idx_b))
    i32 = lambda x: torch.tensor(x, dtype=torch.int32)
    f32 = lambda x: torch.tensor(x, dtype=torch.float32)
    return (i32(ptr_f), i32(idx_f), f32(w_f)), (i32(ptr_b), i32(idx_b), f32(w_b))


def _new_stream(L, prio: Optional[int] = None):
    """A stream at the default priority, or (`prio`) at the given level: -1 = lowest, for leaf work (weight gradients / the panorama
    branch).  (Confining these streams to a slice of the chip with hipExtStreamCreateWithCUMask was measured 1.8x SLOWER -- 7.8 ms
    per step whatever the share, profiles/r03_ab_runs.json group c4 -- and is not offered.)"""
    h = ctypes.c_void_p()
    if prio is None:
        check(L.etp_stream_create(ctypes.byref(h)), "stream_create")
    else:
        check(L.etp_stream_create_prio(ctypes.byref(h), prio), "stream_create")
    return h.value


def _destroy_streams(L, *streams):
    for st in streams:
        if st is not None:
            L.etp_stream_destroy(st)


def _node_csr(batch, V: int, G: int, dev):
    """The node aggregation's CSR and its transpose on the device: from the trajectory lists (batch['traj']: one panorama per
    trajectory step, the pre-training tasks, pretrain_cmt.py:223-283) or one panorama per episode (the fine-tuning rollout step)."""
    if "traj" in batch:
        from .graph_inputs import pack_traj_csr
        tr = batch["traj"]
        f, b = pack_traj_csr(tr["traj_vp_lens"], tr["traj_vpids"], tr["traj_cand_vpids"], tr["gmap_vpids"], V, G)
    else:
        if batch["rgb_fts"].shape[0] != batch["txt_ids"].shape[0]:
            raise ValueError("rgb_fts batch differs from txt_ids batch: pass the trajectory lists as batch['traj']")
        f, b = build_node_csr(batch["view_lens"].cpu(), V, G)
    return tuple(x.to(dev) for x in f), tuple(x.to(dev) for x in b)


# (inp key, batch key, dtype) of every device input of a step; MlmStep stages the first N_MLM_INPUTS of them
INPUTS = (("txt_ids", "txt_ids", torch.int64), ("txt_masks", "txt_masks", torch.bool), ("rgb", "rgb_fts", torch.float32),
          ("dep", "dep_fts", torch.float32), ("loc", "loc_fts", torch.float32), ("nav", "nav_types", torch.int64),
          ("view_lens", "view_lens", torch.int64), ("step_ids", "gmap_step_ids", torch.int64), ("pos", "gmap_pos_fts", torch.float32),
          ("gmask", "gmap_masks", torch.bool),
          ("visited", "gmap_visited_masks", torch.bool), ("dists", "gmap_pair_dists", torch.float32), ("labels", "labels", torch.int64))
N_MLM_INPUTS = 10
# the axes of every input in terms of a step's dimensions ('*' = a feature width, taken from the batch): what a step sizes its input
# allocations by and checks every batch against
INPUT_AXES = {"txt_ids": "BL", "txt_masks": "BL", "rgb": "RV*", "dep": "RV*", "loc": "RV*", "nav": "RV", "view_lens": "R", "step_ids": "BG",
              "pos": "BG*", "gmask": "BG", "visited": "BG", "dists": "BGG", "labels": "B"}
CAPACITY_KEYS = ("B", "L", "R", "V", "G", "Nm")


class _Staging:
    """What PlannerStep and MlmStep (pretrain.py) stage alike -- device inputs, node CSR, the API tensors and stash / workspace of the
    text and panorama branches, dropout state -- and the library calls both issue with the same arguments.  The two schedules
    themselves (which stream, which order) stay written out in each class.

    Every one of these lives in an allocation of the step's own (``_pool``: one byte buffer per name); the step's tensors are
    contiguous views of the current batch's shape at offset 0 of them.  Without ``capacity`` the step is fixed: the allocations are
    those of its first batch and ``load_batch`` refuses any other dimensions.  With ``capacity`` (a dict with any of B, L, R, V, G, Nm,
    or True = the first batch) they are sized for the capacity and ``load_batch`` accepts any shape: every entry point of the library
    recomputes its buffer plan from the dimensions it is called with, so a buffer that is large enough serves any smaller shape.
    ``regrows`` counts the loads that had to enlarge something (a fixed step's stays 0)."""

    def _dims_of(self, batch) -> Dict[str, int]:
        B, L = batch["txt_ids"].shape
        R, V = batch["rgb_fts"].shape[:2]
        return {"B": int(B), "L": int(L), "R": int(R), "V": int(V), "G": int(batch["gmap_step_ids"].shape[1])}

    def _api_tensors(self, d):
        """name -> shape of the fp32 API tensors (pmask: bool) at the dimensions d"""
        B, L, R, V, G, H = d["B"], d["L"], d["R"], d["V"], d["G"], self.eng.cconf.hidden
        return {"txt": (B, L, H), "pano": (R, V, H), "pmask": (R, V), "gimg": (B, G, H), "d_txt": (B, L, H), "d_gimg": (B, G, H),
                "d_pano": (R, V, H)}

    def _byte_buffers(self, d):
        """name -> bytes of the stash / workspace buffers at the dimensions d, as the library plans them.  Separate backward
        workspaces: the backward passes may run on parallel streams."""
        L_, h = self.L, self.eng.handle
        return {"st_txt": L_.etp_txt_stash_bytes(h, d["B"], d["L"]), "ws_txt": L_.etp_txt_ws_bytes(h, d["B"], d["L"]),
                "st_pano": L_.etp_pano_stash_bytes(h, d["R"], d["V"]), "ws_pano": L_.etp_pano_ws_bytes(h, d["R"], d["V"])}

    def _int_arrays(self, d):
        """name -> (shape, dtype) of the integer arrays the step owns"""
        return {"traj_status": ((d["B"] * d["G"] + d["R"],), torch.int32)} if self.traj_nodes else {}

    def _input_shape(self, k, t, d):
        """the shape the dimensions d give the staged input k, feature widths from the batch's tensor t"""
        return tuple(d[a] if a != "*" else int(t.shape[n]) for n, a in enumerate(INPUT_AXES[k]))

    def _plan(self, d, batch):
        """name -> (bytes, shape, dtype) of everything the step allocates at the dimensions d; shape None = a byte buffer"""
        plan = {"in:" + k: (self._input_shape(k, batch[src], d), dt) for k, src, dt in INPUTS[:self._n_inputs]}
        plan.update({k: (s, torch.bool if k == "pmask" else torch.float32) for k, s in self._api_tensors(d).items()})
        plan.update(self._int_arrays(d))
        out = {}
        for k, (shape, dt) in plan.items():
            n = 1
            for x in shape:
                n *= x
            out[k] = (n * torch.empty((), dtype=dt).element_size(), shape, dt)
        for k, nbytes in self._byte_buffers(d).items():
            if nbytes < 0:
                raise _lib.EtpError(f"{k}: the library plans no buffer for the dimensions {d}")
            out[k] = (int(nbytes), None, None)
        return out

    def _bind(self, batch, d):
        """(re)point the step's tensors at `batch`, whose dimensions are d, and copy its inputs in: views of the step's allocations,
        enlarging (never shrinking) whatever the library's byte queries for d find short -- one device synchronise per load that does
        so after the first, since the side streams of the step that last used the old allocation are not torch's.  A batch of the very
        shape that is bound only has its inputs checked and copied (tools/step_load_bench.py); a fixed step only comes here with the
        dimensions it was built for, so that is its every load.  -> the names whose allocation is new."""
        inputs = INPUTS[:self._n_inputs]
        shapes = {k: self._input_shape(k, batch[src], d) for k, src, _ in inputs}
        for k, src, _ in inputs:
            if tuple(batch[src].shape) != shapes[k]:
                raise ValueError(f"batch[{src!r}] has shape {tuple(batch[src].shape)}, the batch's dimensions {d} make it {shapes[k]}")
        short = []
        if (d, shapes) != self._bound:         # else the shape that is bound already (every load of a fixed step): plan and views stand
            need = self._plan(d, batch)
            short = [k for k, (nbytes, _, _) in need.items() if k not in self._pool or self._pool[k].numel() < nbytes]
            if short:
                self._cap = {k: max(self._cap.get(k, 0), v) for k, v in d.items()}
                at_cap = self._plan(self._cap, batch)
                if self._pool:                 # not the step's first batch
                    torch.cuda.synchronize(self.eng.device)
                    self.regrows += 1
                for k in short:
                    self._pool[k] = self.eng.buf(max(need[k][0], at_cap[k][0], 1))
            for k, (nbytes, shape, dt) in need.items():
                t = self._pool[k][:nbytes]
                if shape is not None:
                    t = t.view(dt).view(shape)
                if k.startswith("in:"):
                    self.inp[k[3:]] = t
                else:
                    setattr(self, k, t)
            self._bound, self._d = (d, shapes), d
            self.B, self.Lt, self.Bp, self.V, self.G = d["B"], d["L"], d["R"], d["V"], d["G"]
        for k, src, dt in inputs:
            self.inp[k].copy_(batch[src].to(dt), non_blocking=True)
        if self.traj_nodes:                    # forward [B*G] node rows, backward [Bp] steps; a forward-only step leaves the latter alone
            self.traj_status.zero_()
        return short

    def shape_key(self):
        return tuple(self._d.values())

    def load_batch(self, batch: Dict[str, torch.Tensor]):
        """Refill the step with another batch: the inputs are copied into the step's own allocations (the stash / workspace buffers and
        the streams are reused; only the small CSR index arrays of the node aggregation are rebuilt, or, on the table route, the new
        batch's descriptor tensors are taken by reference).  A fixed step takes the dimensions it was built for only (for MlmStep the
        masked count included); a step built with `capacity` takes any: its tensors are re-viewed at the new dimensions and whatever
        is short grows (_bind)."""
        d = self._dims_of(batch)
        if self._fixed and d != self._d:
            raise ValueError(f"batch shapes {tuple(d.values())} differ from this step's {self.shape_key()}")
        if self.graphs:
            # the CSR index tensors (the descriptor tensors) below are new allocations: kernel nodes of an existing graph would keep the old pointers
            raise RuntimeError("load_batch() on a step with captured / recorded graphs: close() the graphs (or build a new step) first")
        self._bind(batch, d)
        self._load_nodes(batch)

    def _stage(self, model: GlocalTextPathNavCMT, batch, n_inputs: int, dropout, drop_seed: int, p_env: float,
               traj_nodes: Optional[bool] = None, capacity=None):
        self.model = model
        eng = self.eng = model._engine
        eng.require_gpu()
        self.L = eng.L
        if dropout == "config":                # the model config's rates, the reference's policy.train()
            dropout = config_dropout_rates(model.config) + (float(p_env),)
        self.dropout, self.drop_seed, self.step_no = dropout, int(drop_seed) & 0xFFFFFFFF, 0
        self._n_inputs, self.regrows = n_inputs, 0
        self._fixed = capacity is None or capacity is False        # its capacity is its first batch
        cap = {} if self._fixed or capacity is True else dict(capacity)
        if any(k not in CAPACITY_KEYS for k in cap):
            raise ValueError(f"capacity: a dict with any of {CAPACITY_KEYS} or True (got {sorted(cap)})")
        self._pool, self._cap, self.inp = {}, {k: int(v) for k, v in cap.items()}, {}
        self._bound = self._d = None           # (dimensions, input shapes) the step's tensors are views of; the dimensions alone
        self.graphs = []                       # PlannerStep's captured / recorded graphs: load_batch refuses while there are any
        # node features of a trajectory batch straight from its integer tables (etp_traj_nodes_fwd / _bwd, csrc/traj_batch.hip): whenever
        # the batch carries them (TrajBatch.traj_dev of the native loaders), or forced for a string-only batch; ETP_TRAJ_NODES=0 (read
        # once, here) or traj_nodes=False keep the host-built CSR + etp_gather_sum
        self.traj_nodes = traj_nodes is not False and os.environ.get("ETP_TRAJ_NODES", "1") != "0" and \
            (getattr(batch, "traj_dev", None) is not None or bool(traj_nodes))
        self.traj_dev = self.csr_f = self.csr_b = None
        self.loss = torch.zeros(1, dtype=torch.float32, device=eng.device)
        self._bind(batch, self._dims_of(batch))
        self._load_nodes(batch)

    def _drop_state(self):
        if self.dropout is None:
            return None
        return tuple(self.dropout) + ((self.drop_seed << 32) | (self.step_no & 0xFFFFFFFF),)

    def _refresh_side_weights(self, s2: int):
        check(self.L.etp_planner_refresh_part(self.eng.handle, 1, s2), "refresh panorama weights")
        check(self.L.etp_planner_refresh_part(self.eng.handle, 2, s2), "refresh navigation weights")

    def _txt_fwd(self, s: int):
        i = self.inp
        check(self.L.etp_txt_fwd(self.eng.handle, ptr(i["txt_ids"]), ptr(i["txt_masks"]), self.B, self.Lt, ptr(self.txt),
                                 ptr(self.st_txt), s), "txt_fwd")

    def _pano_fwd(self, s2: int):
        i = self.inp
        check(self.L.etp_pano_fwd(self.eng.handle, ptr(i["rgb"]), ptr(i["dep"]), ptr(i["loc"]), ptr(i["nav"]), ptr(i["view_lens"]),
                                  self.Bp, self.V, ptr(self.pano), ptr(self.pmask), ptr(self.st_pano), s2), "pano_fwd")

    def _pano_bwd(self, s2: int):
        i = self.inp
        check(self.L.etp_pano_bwd(self.eng.handle, ptr(self.d_pano), ptr(i["rgb"]), ptr(i["dep"]), ptr(i["loc"]), ptr(i["nav"]),
                                  self.Bp, self.V, None, ptr(self.st_pano), ptr(self.ws_pano), s2), "pano_bwd")

    def _load_nodes(self, batch):
        """what the node aggregation reads for this batch: the descriptor tables, taken by reference (Kmax may differ from batch to
        batch), or the CSR and its transpose"""
        if not self.traj_nodes:
            self.csr_f, self.csr_b = _node_csr(batch, self.V, self.G, self.eng.device)
            return
        td = getattr(batch, "traj_dev", None)
        if td is None:
            if "traj" not in batch:
                raise ValueError("traj_nodes=True needs the trajectory lists (batch['traj']) or a loader's TrajBatch")
            from .graph_inputs import traj_descriptors
            td = traj_descriptors(batch["traj"], self.G, self.eng.device)
        K = int(td["Kmax"])
        want = {"step_off": (self.B + 1,), "step_vp": (self.Bp,), "cand_count": (self.Bp,), "cand_vp": (self.Bp, K),
                "gmap_id": (self.B, self.G), "gmap_len": (self.B,)}
        for k, shape in want.items():
            t = td[k]
            if tuple(t.shape) != shape or t.dtype != torch.int32 or not t.is_contiguous() or t.device != self.inp["view_lens"].device:
                raise ValueError(f"traj_dev[{k!r}] is a contiguous int32 tensor {shape} on the step's device (got {tuple(t.shape)}, {t.dtype})")
        if not 1 <= K <= 64:
            raise ValueError(f"traj_dev['Kmax'] = {K} lies outside 1 .. 64")
        self.traj_dev = td

    def check_traj(self) -> None:
        """one device-to-host copy of the status words of etp_traj_nodes_fwd / _bwd; raises EtpError naming the node rows and steps
        they flagged.  The step itself never synchronises; a step on the CSR route has nothing to check."""
        if not self.traj_nodes:
            return
        from .graph_inputs import traj_status_message
        msg = traj_status_message(self.traj_status.cpu().numpy(), self.B * self.G, self.G)
        if msg:
            raise _lib.EtpError(msg)

    def _traj_args(self):
        from .graph_inputs import traj_table_args
        return traj_table_args(self.traj_dev, self.inp["view_lens"]) + [self.B, self.Bp, self.V, int(self.traj_dev["Kmax"]), self.G,
                                                                        self.eng.cconf.hidden]

    def _assemble(self, s: int):
        """node features = gather-mean of the view embeddings (fp32 API tensors)"""
        if self.traj_nodes:
            check(self.L.etp_traj_nodes_fwd(ptr(self.pano), *self._traj_args(), ptr(self.gimg), ptr(self.traj_status), s), "node assembly")
            return
        pf, xf, wf = self.csr_f
        check(self.L.etp_gather_sum(_lib.ETP_F32, ptr(self.pano), ptr(pf), ptr(xf), ptr(wf), ptr(self.gimg), self.B * self.G,
                                    self.eng.cconf.hidden, 0, s), "node assembly")

    def _assemble_bwd(self, s: int):
        if self.traj_nodes:
            check(self.L.etp_traj_nodes_bwd(ptr(self.d_gimg), *self._traj_args(), ptr(self.d_pano),
                                            self.traj_status.data_ptr() + 4 * self.B * self.G, s), "node assembly bwd")
            return
        pb, xb, wb = self.csr_b
        check(self.L.etp_gather_sum(_lib.ETP_F32, ptr(self.d_gimg), ptr(pb), ptr(xb), ptr(wb), ptr(self.d_pano), self.Bp * self.V,
                                    self.eng.cconf.hidden, 0, s), "node assembly bwd")


class PlannerStep(_Staging):
    def __init__(self, model: GlocalTextPathNavCMT, batch: Dict[str, torch.Tensor], overlap: bool = True,
                 dropout=None, drop_seed: int = 0, refresh_weights: bool = True, zero_grads: bool = True,
                 grad_overwrite: Optional[bool] = None, share_side_streams: Optional["PlannerStep"] = None,
                 traj_nodes: Optional[bool] = None, capacity=None):
        """dropout: None (eval-mode step), "config" (the model config's rates, the reference's policy.train()), or a
        tuple (p_hidden, p_attn, p_head, p_env).  refresh_weights / zero_grads = False when etpnav_amd.optim.FusedAdamW
        closes the step: its kernel already wrote the bf16 weight shadow and zeroed the gradient arena.
        grad_overwrite: weight-gradient GEMMs store instead of accumulating (Engine.scope's grad_overwrite mode) and only the
        vector/table tail of the gradient arena is zeroed per step.  Default: on when this step owns the zeroing (fresh
        gradients every step) and every weight matrix is touched exactly once per step (not the pre-training variant, whose
        language-side x-layer weights this step does not touch).
        traj_nodes: None = the node features come from the batch's descriptor tables when it carries them (a loader's TrajBatch), else
        from the host-built CSR; True forces the tables for a string-only batch['traj'] (graph_inputs.traj_descriptors); False or
        ETP_TRAJ_NODES=0 keep the CSR.  check_traj() reads what the table route flagged.
        capacity: None = a fixed step, allocations of this batch's dimensions and a load_batch of those dimensions only; a dict with any of
        B, L, R, V, G, or True (this batch), = one step object for batches of any shape (_Staging)."""
        self.refresh_weights, self.zero_grads = refresh_weights, zero_grads
        # frozen sub-models (vlnbert_init.py:51-54 -> vilmodel_cmt.py:422-433,675-682): with fix_lang_embedding the text encoder's
        # output is detached (LanguageEncoder.forward :431-432) -- no text backward runs and no gradient reaches `embeddings.*` /
        # `lang_encoder.*`.  fix_pano_embedding alone does NOT stop the panorama backward: forward_panorama adds
        # embeddings.token_type_embeddings(1) (vilmodel_cmt.py:706-708), which stays trainable, so the gradient still crosses the
        # (frozen) panorama encoder to reach it; only with BOTH flags nothing behind the panorama branch requires a gradient
        # (the features are inputs) and autograd never enters it -- neither does this step.  Gradient slots of frozen parameters
        # in the flat arena are unspecified (their .grad is None, FusedAdamW and the data-parallel buckets leave them out).
        self.train_txt = not bool(_cfg_get(model.config, "fix_lang_embedding", False))
        self.train_pano = self.train_txt or not bool(_cfg_get(model.config, "fix_pano_embedding", False))
        if grad_overwrite is None:
            grad_overwrite = bool(zero_grads) and not model._engine.cconf.use_lang2visn and \
                os.environ.get("ETP_GRAD_OVERWRITE", "1") != "0"
        self.grad_overwrite = bool(grad_overwrite)
        self._stage(model, batch, len(INPUTS), dropout, drop_seed, model.drop_env_prob, traj_nodes, capacity)
        self.loss_scale = 1.0 / self.B                         # cross_entropy(sum) / batch_size (ss_trainer_ETP.py:892)
        eng = self.eng
        # side streams: `aux` carries the weight-gradient GEMMs, `s2` the panorama branch (independent of the text branch), `aux2`
        # the d txt_embeds chain of the navigation backward
        self.overlap = overlap
        self.aux = self.s2 = self.aux2 = None
        # leaf work (weight gradients; the panorama branch) runs at the lowest stream priority: whenever its workgroups and the
        # dependent chain's wait for the same CUs, the chain's are dispatched first (ETP_STREAM_PRIO=0: all default)
        low = -1 if os.environ.get("ETP_STREAM_PRIO", "1") != "0" else 0
        self._own_aux = share_side_streams is None
        if not self._own_aux:                  # MicroBatchedStep: one weight-gradient / d_txt stream for all micro-batches
            self.aux, self.aux2 = share_side_streams.aux, share_side_streams.aux2
        elif overlap in (True, "aux", "both"):
            self.aux = _new_stream(self.L, low)
        if overlap in (True, "s2", "both"):
            self.s2 = _new_stream(self.L, low)
        if self._own_aux and self.aux is not None and os.environ.get("ETP_DTXT_STREAM", "1") != "0":
            self.aux2 = _new_stream(self.L)
        # lazy joins: navigation / panorama weight gradients keep running on the aux stream while the text backward starts; the text
        # backward's own join (or the explicit one in enqueue_bwd_main) completes them
        self._lazy = 1 if self.aux is not None else 0
        # schedule switches are read ONCE, here (no environment lookups on the per-step path)
        self._txt_cast_split = os.environ.get("ETP_TXT_CAST_SPLIT", "1") != "0"
        self._chain_first = os.environ.get("ETP_CHAIN_FIRST", "0") == "1"
        # node assembly (gather-mean of the view embeddings) rides behind pano_fwd on the panorama stream, off the chain (round 6: -0.35 %,
        # 4.045 against 4.059 ms, three pairs, profiles/r06_ab_runs.json r6c9); ETP_ASSEMBLE_ON_S2=0 puts it back behind the join
        self._assemble_on_s2 = os.environ.get("ETP_ASSEMBLE_ON_S2", "1") != "0"
        with eng.scope(aux=self.aux, aux2=self.aux2, lazy=self._lazy):
            pass                               # the bridges' join_aux sees this step's streams from now on
        self._pano_pending = False
        self.graph = None
        self.stream = None

    def _api_tensors(self, d):
        t = super()._api_tensors(d)
        t.update({"gemb": (d["B"], d["G"], self.eng.cconf.hidden), "logits": (d["B"], d["G"]), "dlogits": (d["B"], d["G"])})
        return t

    def _byte_buffers(self, d):
        b = super()._byte_buffers(d)
        b.update({"st_nav": self.L.etp_nav_stash_bytes(self.eng.handle, d["B"], d["L"], d["G"]),
                  "ws_nav": self.L.etp_nav_ws_bytes(self.eng.handle, d["B"], d["L"], d["G"])})
        return b

    def _int_arrays(self, d):
        a = super()._int_arrays(d)
        a.update({"row_nll": ((d["B"],), torch.float32), "row_pred": ((d["B"],), torch.int32)})    # validate.sap_eval's per-row outputs
        return a

    def _scope(self, lazy: Optional[int] = None):
        """The planner handle is shared by every step object of a model (PretrainDriver alternates MlmStep and several cached
        PlannerSteps): side streams, lazy-join level, dropout state and overwrite mode are (re)installed at every enqueue, so a
        step never runs on another step's streams or silently loses its overlap schedule.  lazy = 2: a text-backward range above
        layer 0 that does not join (the next range continues the chain)."""
        return self.eng.scope(aux=self.aux, aux2=self.aux2, lazy=self._lazy if lazy is None else lazy, drop=self._drop_state(),
                              grad_overwrite=self.grad_overwrite)

    @staticmethod
    def batch_shape_key(batch):
        """shape_key() of a step built for `batch`: what PretrainDriver's per-shape cache is keyed by"""
        B, Lt = batch["txt_ids"].shape
        Bp, V = batch["rgb_fts"].shape[:2]
        return (B, Lt, Bp, V, batch["gmap_step_ids"].shape[1])

    def load_batch(self, batch: Dict[str, torch.Tensor]):
        super().load_batch(batch)
        if not self._fixed:                    # as a step built for this batch has it; a caller's own scale is set after the load
            self.loss_scale = 1.0 / self.B

    # ------------------------------------------------------------------------------------------
    def _enqueue_pano_bwd(self, s: int):
        if not self.train_pano:
            return
        with self._scope():
            self._pano_bwd(self.s2 if self.s2 is not None else s)
        self._pano_pending = True

    def enqueue_main(self, s: int, backward: bool = True, join_pano: bool = True, defer_pano: bool = False):
        """Everything except the text-encoder backward: weight refresh, zero grads, the three forwards, loss and the
        navigation + panorama backward.  The panorama branch (forward and backward) runs on a second stream beside the
        text branch; with join_pano=False its backward is left running and joined by enqueue_txt_bwd."""
        self.enqueue_fwd(s, backward)
        if backward:
            self.enqueue_bwd_main(s, join_pano, defer_pano)

    def enqueue_fwd(self, s: int, backward: bool = True, after_prologue=None):
        """weight refresh, gradient zeroing, forward_txt || forward_panorama, node assembly, forward_navigation, loss"""
        s2 = self.s2 if self.s2 is not None else s
        L, eng, h, i = self.L, self.eng, self.eng.handle, self.inp
        B, Lt, G = self.B, self.Lt, self.G
        self.step_no += 1
        with self._scope():
            L.etp_stamp_mark(s, 1)             # measurement aid: a no-op unless a stamp sink is installed (tools/chain_waits.py)
            # weight-shadow refresh and gradient zeroing ride on the stream that first needs them: the text cast on the main
            # stream, the panorama/navigation casts and the (bandwidth-bound) gradient memset on the panorama stream, whose
            # join below precedes forward_navigation and every backward kernel
            if self.refresh_weights:
                # only layer 0's cast stays in front of the first text GEMM; layers 1.. are cast on the panorama stream and
                # etp_txt_fwd waits for them after its layer 0 (ETP_TXT_CAST_SPLIT=0: the whole text cast on the main stream)
                if self.s2 is not None and self._txt_cast_split:
                    check(L.etp_planner_refresh_text_split(h, s, s2), "refresh text weights")
                else:
                    check(L.etp_planner_refresh_part(h, 0, s), "refresh text weights")
            check(L.etp_stream_after(s, s2), "fork")
            if self.refresh_weights:
                self._refresh_side_weights(s2)
            if backward and self.zero_grads:
                # overwrite mode: the matrix region [0, n_matrix) is fully rewritten by this step's weight-gradient stores
                # (round 6: navigation cast + this memset BEHIND the panorama branch instead of in front of it: no gain, r06_ab_runs.json r6c11;
                # the memset beside forward_navigation, the backward waiting for it: +0.7 %, 3.952 against 3.924 ms, four pairs, r6c16)
                lo = eng.n_matrix if self.grad_overwrite else 0
                check(L.etp_memset_async(eng.grads.data_ptr() + lo * 4, 0, (eng.grads.numel() - lo) * 4, s2), "memset grads")
            if after_prologue is not None:     # MicroBatchedStep: the other micro-batches' streams are ordered after the casts / memset
                after_prologue(s, s2)
            self._txt_fwd(s)
            self._pano_fwd(s2)
            on_s2 = self._assemble_on_s2 and s2 != s
            if on_s2:                          # the gather-mean of the view embeddings depends on the panorama branch only: behind it, off the chain
                self._assemble(s2)
            check(L.etp_stream_after(s2, s), "join")
            L.etp_stamp_mark(s, 2)
            if not on_s2:
                self._assemble(s)
            check(L.etp_nav_fwd(h, ptr(self.txt), ptr(i["txt_masks"]), ptr(i["step_ids"]), ptr(self.gimg), ptr(i["pos"]),
                                ptr(i["gmask"]), ptr(i["visited"]), ptr(i["dists"]), B, Lt, G, ptr(self.gemb), ptr(self.logits),
                                ptr(self.st_nav), s), "nav_fwd")
            check(L.etp_sap_ce(ptr(self.logits), ptr(i["labels"]), ptr(self.loss), ptr(self.dlogits) if backward else None, B, G,
                               self.loss_scale, -100, s), "sap_ce")
            L.etp_stamp_mark(s, 3)

    def enqueue_bwd_main(self, s: int, join_pano: bool = True, defer_pano: bool = False):
        """navigation backward, node assembly backward, panorama backward (on the panorama stream)"""
        s2 = self.s2 if self.s2 is not None else s
        L, h, i = self.L, self.eng.handle, self.inp
        with self._scope():
            check(L.etp_nav_bwd(h, None, ptr(self.dlogits), ptr(self.txt), ptr(i["txt_masks"]), ptr(i["step_ids"]),
                                ptr(i["pos"]), ptr(i["gmask"]), ptr(i["visited"]), ptr(i["dists"]), self.B, self.Lt, self.G,
                                ptr(self.d_txt), ptr(self.d_gimg), ptr(self.st_nav), ptr(self.ws_nav), s), "nav_bwd")
            L.etp_stamp_mark(s, 4)
            if not self.train_pano:            # frozen panorama embedding: the backward stops at the node features (d_gimg)
                if join_pano:
                    check(L.etp_planner_join_aux(h, s), "join aux")
                return
            # (round 6: this gather on the panorama stream behind the fork instead -- it feeds the panorama backward only -- measured neutral,
            # 3.971 against 3.969 ms over four pairs, r06_ab_runs.json r6c14: the text backward waits for d txt_embeds meanwhile anyway)
            self._assemble_bwd(s)
            L.etp_stamp_mark(s, 5)
            check(L.etp_stream_after(s, s2), "fork")
            if defer_pano:                     # the caller enqueues the panorama backward later (run_eager: after the first text layers);
                return                         # its stream is ordered after d_pano's producer already now
            self._pano_bwd(s2)
            if join_pano:
                check(L.etp_stream_after(s2, s), "join")
                check(L.etp_planner_join_aux(h, s), "join aux")      # callers of this mode read the non-text gradients next
            else:
                self._pano_pending = True

    def enqueue_txt_bwd(self, s: int, layer_lo: int = 0, layer_hi: Optional[int] = None, lazy: Optional[int] = None):
        """Text-encoder backward (optionally only layers [layer_lo, layer_hi), descending calls share the running gradient; `lazy`:
        the lazy-join level of this range, see _scope)."""
        L, eng, i = self.L, self.eng, self.inp
        if layer_hi is None:
            layer_hi = eng.cconf.n_l
        if not self.train_txt:     # frozen language side: only the joins this call owes its callers
            if layer_lo == 0:
                self._join_side(s)
            return
        with self._scope(lazy):
            L.etp_stamp_mark(s, 6)
            check(L.etp_txt_bwd_range(eng.handle, ptr(self.d_txt), ptr(i["txt_ids"]), ptr(i["txt_masks"]), self.B, self.Lt,
                                      ptr(self.st_txt), ptr(self.ws_txt), layer_lo, layer_hi, s), "txt_bwd")
        if layer_lo > 0:
            return
        if self._pano_pending:
            check(L.etp_stream_after(self.s2 if self.s2 is not None else s, s), "join")
            self._pano_pending = False
        L.etp_stamp_mark(s, 7)

    def _join_side(self, s: int):
        """order `s` after the weight-gradient stream and a still-running panorama backward (what the text backward's last
        range does for a trainable text encoder)"""
        check(self.L.etp_planner_join_aux(self.eng.handle, s), "join aux")
        if self._pano_pending:
            check(self.L.etp_stream_after(self.s2 if self.s2 is not None else s, s), "join")
            self._pano_pending = False
        self.L.etp_stamp_mark(s, 7)

    def run_eager(self, stream: Optional[int] = None, backward: bool = True):
        """Enqueue one step on `stream` (default: torch's current stream).  With dropout on, every call draws fresh
        masks (the step counter is part of the seed); a captured graph replays the masks it was captured with.

        ETP_CHAIN_FIRST=1 enqueues the top three text-backward layers BEFORE the panorama backward (a side branch of ~45
        launches).  Measured neutral (203.7 vs 206.1 steps/s, same box): the host issues a whole step in 1.4 ms against
        4.85 ms of GPU time (tools/host_timing.py), so issue order does not matter; the default keeps the simple order."""
        s = stream if stream is not None else self.eng.stream()
        if not backward:
            self.enqueue_main(s, False, join_pano=True)
            return
        n_l = self.eng.cconf.n_l
        head = max(0, min(3, n_l - 1)) if self._chain_first else 0
        self.enqueue_main(s, True, join_pano=False, defer_pano=head > 0)   # panorama backward overlaps the text backward
        if head > 0:
            # the top layers' weight gradients keep running while the chain continues (no join between the ranges)
            self.enqueue_txt_bwd(s, n_l - head, n_l, lazy=2 if self._lazy else 0)
            self._enqueue_pano_bwd(s)
            self.enqueue_txt_bwd(s, 0, n_l - head)
        else:
            self.enqueue_txt_bwd(s)

    def run_data_parallel(self, groups, bucket_ready, stream: Optional[int] = None, overlapped: bool = True):
        """One step issued for data-parallel training (replaces DDP's bucket hooks, ss_trainer_ETP.py:208-212): the text
        backward runs in the layer `groups` [(lo, hi), ...] (last layers first) and `bucket_ready(i, side_streams)` is called
        as soon as bucket i's gradients are ENQUEUED -- bucket 0 = everything outside the text encoder, bucket 1 + k = text
        group k (dp.planner_buckets_layered).

        overlapped=True (a reducer whose communication stream can wait for side streams: dp.GradReducer with the library
        communicator): the step keeps the free-running single-GPU schedule -- the panorama backward and all weight gradients
        stay on their side streams, nothing is joined into the dependent chain between the groups -- and `side_streams` names
        the streams that, besides `stream`, hold producers of the bucket (the reducer orders its communication stream after
        them).  Measured on one MI355X without collectives: 4.60 ms for the joined order below against 4.24 ms for the
        free-running step (bench.py --dp-schedule).
        overlapped=False (torch.distributed collectives, which only see the main stream): everything a bucket needs is joined
        into `stream` before the callback (side_streams = ())."""
        s = stream if stream is not None else self.eng.stream()
        if not overlapped or self.aux is None:
            self.enqueue_main(s, True, join_pano=True)
            bucket_ready(0, ())
            for k, (lo, hi) in enumerate(groups):
                self.enqueue_txt_bwd(s, lo, hi)
                bucket_ready(1 + k, ())
            return
        side = tuple(x for x in (self.aux, self.s2) if x is not None)
        self.enqueue_main(s, True, join_pano=False)          # the panorama backward keeps running beside the text backward
        if not groups or not self.train_txt:                 # frozen text encoder (dp.planner_buckets_layered returns no text groups)
            bucket_ready(0, side)
            self._join_side(s)
            return
        for k, (lo, hi) in enumerate(groups):
            self.enqueue_txt_bwd(s, lo, hi, lazy=2)          # no join between the layer groups; the last group (layer 0) joins
            if k == 0:
                bucket_ready(0, side)                        # issued after the first group: the panorama branch gets a head start
            bucket_ready(1 + k, (self.aux,))

    # ------------------------------------------------------------------------------------------
    def _build_graphs(self, begin, end, abort, backward: bool, split_text_bwd: bool):
        """capture() and record(): warm up eagerly (kernel attributes, lazy allocations), then build the step's graph(s) on a
        private stream between begin() and end() -> graph handle; abort() when the step raises in between.  With split_text_bwd
        the text-encoder backward is a second graph so that a gradient all-reduce of everything else can be issued between the
        two (data-parallel overlap)."""
        torch.cuda.synchronize()
        self.run_eager(backward=backward)
        torch.cuda.synchronize()
        self.stream = _new_stream(self.L)
        self.graphs, self.graph_stats = [], []
        if backward and split_text_bwd:
            fns = (lambda st: self.enqueue_main(st, True), self.enqueue_txt_bwd)
        else:
            fns = (lambda st: self.run_eager(stream=st, backward=backward),)
        for fn in fns:
            check(begin(), "graph begin")
            try:
                fn(self.stream)
            except Exception:
                abort()
                raise
            self.graphs.append(end())
        self.graph = self.graphs[0]
        return self

    def capture(self, backward: bool = True, split_text_bwd: bool = False):
        """Capture the step into hipGraph(s) by stream capture (see _build_graphs)."""
        if self.aux is not None and self.s2 is not None and not os.environ.get("ETP_GRAPH_FORCE"):
            raise _lib.EtpError("hipGraph capture with two side streams crashes hipStreamEndCapture on ROCm 7.2; "
                                "build the PlannerStep with overlap='s2', 'aux' or False for graph replay "
                                "(measured on MI355X: eager two-stream issue is the fastest mode anyway)")

        def end(checked=True):
            g = ctypes.c_void_p()
            rc = self.L.etp_graph_end(self.stream, ctypes.byref(g))
            if checked:
                check(rc, "graph_end")
            return g.value

        return self._build_graphs(lambda: self.L.etp_graph_begin(self.stream), end, lambda: end(False), backward, split_text_bwd)

    def record(self, backward: bool = True, split_text_bwd: bool = False):
        """Build the step's hipGraph EXPLICITLY (etp_rec_begin / etp_rec_end: one kernel node per launch, dependencies from
        the per-stream order and the fork/join events) instead of by stream capture -- this keeps the full three-stream
        schedule (capture() cannot: hipStreamEndCapture crashes with two side streams on ROCm 7.2) while the host issues a
        single hipGraphLaunch per step.  Like capture(), a recorded graph replays the dropout masks it was built with."""
        def end():
            g, nk, ne = ctypes.c_void_p(), ctypes.c_int64(), ctypes.c_int64()
            check(self.L.etp_rec_end(ctypes.byref(g), ctypes.byref(nk), ctypes.byref(ne)), "rec_end")
            self.graph_stats.append((int(nk.value), int(ne.value)))
            return g.value

        return self._build_graphs(self.L.etp_rec_begin, end, self.L.etp_rec_abort, backward, split_text_bwd)

    def replay(self, part: Optional[int] = None, stream: Optional[int] = None):
        """Launch the captured graph(s) on `stream` (default: torch's current stream, so torch ops order after it)."""
        s = stream if stream is not None else self.eng.stream()
        for k, g in enumerate(self.graphs):
            if part is None or part == k:
                check(self.L.etp_graph_launch(g, s), "graph_launch")

    def sync(self):
        if self.stream is not None:
            check(self.L.etp_stream_sync(self.stream), "stream_sync")
        torch.cuda.synchronize()

    def time_replays(self, iters: int) -> float:
        """HIP-event time (ms) of `iters` back-to-back replays of the single-graph step on the capture stream."""
        assert len(self.graphs) == 1
        ms = ctypes.c_float()
        check(self.L.etp_graph_time(self.graphs[0], self.stream, iters, ctypes.byref(ms)), "graph_time")
        return float(ms.value)

    def close(self):
        for g in getattr(self, "graphs", []) or []:
            self.L.etp_graph_destroy(g)
        self.graphs, self.graph = [], None
        _destroy_streams(self.L, self.stream)
        self.stream = None
        self.L.etp_planner_set_lazy_join(self.eng.handle, 0)
        self.L.etp_planner_set_aux_stream(self.eng.handle, None)
        self.L.etp_planner_set_aux2_stream(self.eng.handle, None)
        _destroy_streams(self.L, *((self.aux, self.s2, self.aux2) if self._own_aux else (self.s2,)))
        self.aux = self.s2 = self.aux2 = None


class MicroBatchedStep:
    """The same training step (one gradient of the mean loss over the whole batch, ss_trainer_ETP.py:892,1055) issued as
    `n_micro` micro-batches -- a GRADIENT-ACCUMULATION facility for a batch whose activations do not fit, not a
    performance mode.

    Measured on MI355X (profiles/r02s_bench_micro*.json): 2 micro-batches 10.8-13.7 ms, 4 micro-batches
    25.8 ms against 4.4 ms for the single chain.  The idea that one chain's kernels would fill the other's launch / drain
    gaps does not hold on this chip: a half-batch chain takes as long as the full-batch one (its kernels are bound by the
    per-launch latency, not by work), and the chains meet on the shared weight-gradient stream, where the later
    micro-batches must accumulate behind the first one's stores in issue order.
    Gradients: the first micro-batch's weight-gradient GEMMs store (first touch), the others accumulate behind it on the
    shared weight-gradient stream (in issue order, so no atomics are needed on the matrices); vector / table gradients are
    atomics as before.  The loss of every micro-batch is scaled by 1/B of the WHOLE batch, so the arena ends up with exactly
    the full-batch gradient (fp32 summation order aside; tests/test_planner_gpu.py).  Dropout draws an independent mask
    stream per micro-batch.  The pre-training loop's gradient_accumulation_steps (train_r2r.py:231-300) is implemented in
    etpnav_amd.pretrain.PretrainDriver on whole task batches instead."""

    def __init__(self, model: GlocalTextPathNavCMT, batch: Dict[str, torch.Tensor], n_micro: int = 2, dropout=None,
                 drop_seed: int = 0):
        if "traj" in batch:
            raise ValueError("MicroBatchedStep splits along the episode axis: trajectory-list batches are not supported")
        B = batch["txt_ids"].shape[0]
        if n_micro < 1 or B % n_micro != 0:
            raise ValueError(f"batch size {B} is not a multiple of n_micro={n_micro}")
        self.model, self.eng, self.L = model, model._engine, model._engine.L
        self.B, self.n = B, n_micro
        mb = B // n_micro
        self.parts = []
        for k in range(n_micro):
            sub = {key: (v[k * mb:(k + 1) * mb] if torch.is_tensor(v) and v.shape[:1] == (B,) else v) for key, v in batch.items()}
            p = PlannerStep(model, sub, overlap=True, dropout=dropout, drop_seed=drop_seed * n_micro + k,
                            refresh_weights=(k == 0), zero_grads=(k == 0), grad_overwrite=(None if k == 0 else False),
                            share_side_streams=self.parts[0] if k > 0 else None)
            p.loss_scale = 1.0 / B
            self.parts.append(p)
        # ONE weight-gradient stream and ONE d_txt stream for all micro-batches: in-order issue is what lets the later
        # micro-batches accumulate onto the first one's stores without atomics
        with self.eng.scope(aux=self.parts[0].aux, aux2=self.parts[0].aux2, lazy=1):
            pass
        self.mains = [None] + [_new_stream(self.L) for _ in range(1, n_micro)]

    @property
    def loss(self):
        return sum(p.loss for p in self.parts)

    @property
    def inp(self):
        return self.parts[0].inp

    def run_eager(self, stream: Optional[int] = None):
        s = stream if stream is not None else self.eng.stream()
        mains = [s] + self.mains[1:]
        L = self.L

        def fork_others(s_main, s_side):           # after micro-batch 0's weight casts and gradient memset are enqueued
            for m in mains[1:]:
                check(L.etp_stream_after(s_main, m), "fork")
                check(L.etp_stream_after(s_side, m), "fork")

        # issue order = order on the shared weight-gradient stream: all forwards (their text K/V projections run there), then
        # the navigation / panorama backward of every micro-batch, then the text backward of every micro-batch
        for k, (p, m) in enumerate(zip(self.parts, mains)):
            p.enqueue_fwd(m, True, after_prologue=fork_others if k == 0 else None)
        for p, m in zip(self.parts, mains):
            p.enqueue_bwd_main(m, join_pano=False)
        for p, m in zip(self.parts, mains):
            p.enqueue_txt_bwd(m)                   # joins this micro-batch's panorama branch and the weight-gradient stream
        for m in mains[1:]:
            check(L.etp_stream_after(m, s), "join")

    def close(self):
        torch.cuda.synchronize()
        for p in reversed(self.parts):
            p.close()
        _destroy_streams(self.L, *self.mains[1:])
        self.mains = [None]
