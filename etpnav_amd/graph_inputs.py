"""Graph inputs of forward_navigation assembled on the device.

The reference rebuilds, at every rollout step and on the host, everything forward_navigation needs besides the node
embeddings: ``RLTrainer._nav_gmap_variable`` (ss_trainer_ETP.py:344-417) walks Python dicts of every episode's
``GraphMap``, which itself re-runs networkx all-pairs Dijkstra after every update (graph_utils.py:256-257), fills the
pairwise distance matrix in an O(G^2) Python loop and copies six tensors to the GPU.  Here the host only keeps COMPACT
arrays per episode (positions, edge lengths, ghost fronts) and one kernel launch (``etp_gmap_assemble``) produces the padded
device tensors.

* ``pack_episode(gmap, cur_vp, cur_pos, cur_heading)`` reads any object with the reference GraphMap's attributes
  (``node_pos, node_stepId, ghost_aug_pos, ghost_fronts`` and either ``graph_nx`` or ``edges``) — so the reference's own
  GraphMap can be used unchanged;
* ``GraphMapLite`` is a numpy-only GraphMap with the same update rules (graph_utils.py:118-257) that simply skips the
  per-step Dijkstra (the device does the shortest paths);
* ``nav_gmap_variable(gmaps, cur_vp, cur_pos, cur_heading, device)`` returns the same dict as the reference method
  (without ``gmap_img_fts``; see the next item);
* ``gmap_img_fts``: the reference stacks per-node tensors in Python (``get_node_embeds``, ss_trainer_ETP.py:360-365).  In
  **device-store mode** GraphMapLite is given ROW INDICES into one embedding store tensor instead of tensors
  (``update_graph(..., cur_embeds=row, cand_embeds=[rows])``); ``pack_img_csr`` turns the graphs into a CSR and
  ``gather_rows`` (autograd wrapper of ``etp_gather_sum``) produces the padded ``[B,G,H]`` tensor in one launch, with
  the gradient flowing back into the store through the transposed CSR;
* ``DeviceGraphMaps`` keeps the maps themselves on the device (``etp_gmap_update``, csrc/gmap_update.hip): one launch per rollout
  step maintains them in place and emits the compact arrays, ``etp_gmap_embed_csr`` builds the CSR there, and the host keeps a
  ``GraphMapView`` of names and positions from a small record.  A route beside ``GraphMapLite`` + ``nav_gmap_variable``.

* ``EmbedStore`` builds the embedding store those rows live in (``etp_pano_store_fwd``, csrc/pano_store.hip): ``append`` turns the
  panorama encoder's output of one rollout step into the step's rows (the masked panorama mean and the candidate views,
  ss_trainer_ETP.py:838-839, 864-865) in one launch and hands back the row numbers ``update`` / ``update_graph`` take; the backward of
  every later ``img_fts`` / ``gather_rows`` reaches the panorama encoder of the step that wrote a row.

* ``traj_descriptors`` / ``aggregate_gmap_features(..., traj_dev=)``: the pre-training node features (``_aggregate_gmap_features``,
  pretrain vilmodel.py:585-619) from integer tables on the device (``etp_traj_nodes_fwd`` / ``_bwd``, csrc/traj_batch.hip) instead of
  ``pack_traj_csr``'s host-built CSR; the same bits.

``cur_heading`` is the scalar heading (radians) that the reference obtains with ``heading_from_quaternion(cur_ori)``
(graph_utils.py:54-59); quaternion handling belongs to the simulator side and is out of scope.
"""
from __future__ import annotations

from typing import Dict, List, Optional, Sequence

import numpy as np
import torch

from . import _lib
from ._lib import check, ptr

MAX_NODES, MAX_GHOSTS = 64, 192      # limits of etp_gmap_assemble (csrc/graph.hip)


def _is_row(x) -> bool:
    return isinstance(x, (int, np.integer))


def _dist(a, b) -> float:
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return float(np.sqrt(((b - a) ** 2).sum()))          # calc_position_distance graph_utils.py:13-19


class GraphMapLite:
    """GraphMap (graph_utils.py:118-257) without networkx: same node / ghost bookkeeping, edges kept as a dict; shortest
    paths are left to the device.  Embeddings are stored as given (tensors), exactly like the reference."""

    def __init__(self, has_real_pos: bool, loc_noise: float, merge_ghost: bool, ghost_aug: float, rng=None):
        self.node_pos: Dict[str, np.ndarray] = {}
        self.node_embeds: Dict[str, object] = {}
        self.node_stepId: Dict[str, int] = {}
        self.edges: Dict[tuple, float] = {}
        self.ghost_cnt = 0
        self.ghost_pos: Dict[str, list] = {}
        self.ghost_mean_pos: Dict[str, np.ndarray] = {}
        self.ghost_aug_pos: Dict[str, np.ndarray] = {}
        self.ghost_embeds: Dict[str, list] = {}
        self.ghost_fronts: Dict[str, list] = {}
        self.ghost_real_pos: Dict[str, list] = {}
        self.node_stop_scores: Dict[str, float] = {}         # viewpoint -> stop probability (graph_utils.py:161); decide.py fills it
        self.has_real_pos, self.merge_ghost, self.ghost_aug, self.loc_noise = has_real_pos, merge_ghost, ghost_aug, loc_noise
        self.rng = rng if rng is not None else np.random

    def _nearest(self, queries: np.ndarray, keys: Dict[str, np.ndarray]) -> List[Optional[str]]:
        """For every query position the key within ``loc_noise`` of it that is nearest (first in insertion order among equals), or
        None -- the rule of GraphMap._localize (graph_utils.py:146-158) for ALL queries against all keys in one distance matrix
        instead of a Python loop per pair."""
        if not len(keys) or not len(queries):
            return [None] * len(queries)
        names = list(keys.keys())
        K = np.asarray([keys[k] for k in names], dtype=np.float64).reshape(len(names), 3)
        Q = np.asarray(queries, dtype=np.float64).reshape(-1, 3)
        d2 = ((Q[:, None, :] - K[None, :, :]) ** 2).sum(-1)
        j = d2.argmin(1)                                     # argmin returns the FIRST minimum, as the reference's strict `<` does
        best = d2[np.arange(len(Q)), j] ** 0.5
        return [names[jj] if dd <= self.loc_noise and dd < 10000 else None for jj, dd in zip(j.tolist(), best.tolist())]

    def _localize(self, qpos, kpos_dict):                   # single-query form (kept: the trainer side calls it, graph_utils.py:146)
        return self._nearest(np.asarray(qpos, dtype=np.float64).reshape(1, 3), kpos_dict)[0]

    def identify_node(self, cur_pos, cur_heading, cand_ang, cand_dis):      # :160-166 + estimate_cand_pos :61-71
        cur_vp = str(len(self.node_pos))
        cand_vp = [f"{cur_vp}_{i}" for i in range(len(cand_ang))]
        ang = (float(cur_heading) + np.asarray(cand_ang, dtype=np.float64)) % (2 * np.pi)
        dis = np.asarray(cand_dis, dtype=np.float64)
        cand_pos = np.zeros((len(cand_vp), 3))
        cand_pos[:, 0] = cur_pos[0] - dis * np.sin(ang)
        cand_pos[:, 1] = cur_pos[1]
        cand_pos[:, 2] = cur_pos[2] - dis * np.cos(ang)
        return cur_vp, cand_vp, [p for p in cand_pos]

    def _add_edge(self, u, v, w):
        self.edges[(u, v) if u <= v else (v, u)] = float(w)

    def delete_ghost(self, vp):                              # :168-175
        for d in (self.ghost_pos, self.ghost_mean_pos, self.ghost_embeds, self.ghost_fronts):
            d.pop(vp)
        self.ghost_aug_pos.pop(vp, None)
        if self.has_real_pos:
            self.ghost_real_pos.pop(vp)

    def update_graph(self, prev_vp, step_id, cur_vp, cur_pos, cur_embeds, cand_vp, cand_pos, cand_embeds, cand_real_pos):
        """The bookkeeping of GraphMap.update_graph (graph_utils.py:177-257) without its two networkx all-pairs calls (the device
        computes the shortest paths, csrc/graph.hip), organised around what depends on what:
          1. the visited node and its edge to the previous one;
          2. every candidate against the VISITED nodes at once (their positions do not change during the call): a match is an edge;
          3. the remaining candidates, in order, against the ghosts (sequential by nature: each may create or move a ghost);
          4. the position jitter of the ghosts."""
        cur_pos = np.asarray(cur_pos, dtype=np.float64)
        if prev_vp is not None:
            self._add_edge(prev_vp, cur_vp, _dist(self.node_pos[prev_vp], cur_pos))
        self.node_pos[cur_vp], self.node_embeds[cur_vp], self.node_stepId[cur_vp] = cur_pos, cur_embeds, step_id
        n = min(len(cand_vp), len(cand_pos), len(cand_embeds))
        cand_xyz = np.asarray([np.asarray(p, dtype=np.float64) for p in cand_pos[:n]], dtype=np.float64).reshape(n, 3)
        on_node = self._nearest(cand_xyz, self.node_pos)
        for i in range(n):
            if on_node[i] is not None:
                self._add_edge(cur_vp, on_node[i], _dist(cur_pos, self.node_pos[on_node[i]]))
            else:
                self._absorb(cur_vp, cand_xyz[i], cand_embeds[i], cand_real_pos[i] if self.has_real_pos else None)
        self._jitter_ghosts()

    def _absorb(self, front_vp, pos, embeds, real_pos):
        """One candidate that is no visited node: it joins the ghost it localises to (merge_ghost) or becomes a new ghost."""
        gvp = self._localize(pos, self.ghost_mean_pos) if self.merge_ghost else None
        if gvp is None:
            gvp = f"g{self.ghost_cnt}"
            self.ghost_cnt += 1
            self.ghost_pos[gvp], self.ghost_mean_pos[gvp], self.ghost_fronts[gvp] = [pos], pos, [front_vp]
            # device-store mode keeps the ROWS of the embedding store (summed on the device later); tensor mode the running sum
            self.ghost_embeds[gvp] = [[int(embeds)] if _is_row(embeds) else embeds, 1]
            if self.has_real_pos:
                self.ghost_real_pos[gvp] = [real_pos]
            return
        self.ghost_pos[gvp].append(pos)
        self.ghost_mean_pos[gvp] = np.mean(self.ghost_pos[gvp], axis=0)
        acc = self.ghost_embeds[gvp]
        if _is_row(embeds):
            acc[0].append(int(embeds))
        else:
            acc[0] = acc[0] + embeds
        acc[1] += 1
        self.ghost_fronts[gvp].append(front_vp)
        if self.has_real_pos:
            self.ghost_real_pos[gvp].append(real_pos)

    def _jitter_ghosts(self):                                # graph_utils.py:245-252
        self.ghost_aug_pos = {k: np.array(v, dtype=np.float64) for k, v in self.ghost_mean_pos.items()}
        if self.ghost_aug != 0:
            for gvp, gpos in self.ghost_aug_pos.items():
                noise = self.rng.normal(loc=(0, 0, 0), scale=(self.ghost_aug, 0, self.ghost_aug), size=(3,))
                self.ghost_aug_pos[gvp] = gpos + np.clip(noise, -self.ghost_aug, self.ghost_aug)

    def get_node_embeds(self, vp):                           # :272-276 (tensor mode only)
        if not vp.startswith("g"):
            return self.node_embeds[vp]
        return self.ghost_embeds[vp][0] / self.ghost_embeds[vp][1]

    def embed_rows(self, vp):
        """Device-store mode: (rows of the embedding store, weight) whose weighted sum is get_node_embeds(vp)."""
        if not vp.startswith("g"):
            return [int(self.node_embeds[vp])], 1.0
        rows, cnt = self.ghost_embeds[vp]
        return list(rows), 1.0 / cnt


def pack_episode(gmap, cur_vp: str, cur_pos, cur_heading: float) -> dict:
    """Compact arrays of one episode from a GraphMap-like object (reference GraphMap or GraphMapLite)."""
    nodes = list(gmap.node_pos.keys())
    ghosts = list(gmap.ghost_pos.keys())
    idx = {vp: i for i, vp in enumerate(nodes)}
    n, m = len(nodes), len(ghosts)
    adj = np.full((n, n), -1.0, dtype=np.float64)
    if hasattr(gmap, "graph_nx"):
        edge_iter = ((u, v, w) for u, v, w in gmap.graph_nx.edges(data="weight"))
    else:
        edge_iter = ((u, v, w) for (u, v), w in gmap.edges.items())
    for u, v, w in edge_iter:
        adj[idx[u], idx[v]] = adj[idx[v], idx[u]] = w
    return {
        "n_nodes": n, "n_ghost": m,
        "node_pos": np.array([gmap.node_pos[vp] for vp in nodes], dtype=np.float64).reshape(n, 3),
        "node_step": np.array([gmap.node_stepId[vp] for vp in nodes], dtype=np.int64),
        "adj": adj,
        "ghost_pos": np.array([gmap.ghost_aug_pos[vp] for vp in ghosts], dtype=np.float64).reshape(m, 3),
        "ghost_fronts": [[idx[f] for f in gmap.ghost_fronts[vp]] for vp in ghosts],
        "cur_node": idx[cur_vp], "cur_pos": np.asarray(cur_pos, dtype=np.float64), "cur_heading": float(cur_heading),
    }


def pack_batch(episodes: Sequence[dict]) -> Dict[str, np.ndarray]:
    """Pad the per-episode arrays to batch maxima (host side, O(total nodes + edges))."""
    B = len(episodes)
    Nmax = max(1, max(e["n_nodes"] for e in episodes))
    Mmax = max(e["n_ghost"] for e in episodes)
    Fmax = max(1, max(sum(len(f) for f in e["ghost_fronts"]) for e in episodes))
    if Nmax > MAX_NODES or Mmax > MAX_GHOSTS:
        raise ValueError(f"etp_gmap_assemble handles <= {MAX_NODES} visited nodes and <= {MAX_GHOSTS} ghosts per episode")
    out = {
        "node_pos": np.zeros((B, Nmax, 3), np.float32), "node_step": np.zeros((B, Nmax), np.int32),
        "n_nodes": np.zeros(B, np.int32), "adj": np.full((B, Nmax, Nmax), -1.0, np.float32),
        "ghost_pos": np.zeros((B, max(Mmax, 1), 3), np.float32), "n_ghost": np.zeros(B, np.int32),
        "front_ptr": np.zeros((B, Mmax + 1), np.int32), "front_idx": np.zeros((B, Fmax), np.int32),
        "cur_node": np.zeros(B, np.int32), "cur_pos": np.zeros((B, 3), np.float32), "cur_heading": np.zeros(B, np.float32),
    }
    for b, e in enumerate(episodes):
        n, m = e["n_nodes"], e["n_ghost"]
        out["n_nodes"][b], out["n_ghost"][b] = n, m
        out["node_pos"][b, :n] = e["node_pos"]
        out["node_step"][b, :n] = e["node_step"]
        out["adj"][b, :n, :n] = e["adj"]
        if m:
            out["ghost_pos"][b, :m] = e["ghost_pos"]
        q = 0
        for g, fr in enumerate(e["ghost_fronts"]):
            out["front_idx"][b, q:q + len(fr)] = fr
            q += len(fr)
            out["front_ptr"][b, g + 1] = q
        out["front_ptr"][b, m + 1:] = q
        out["cur_node"][b], out["cur_pos"][b], out["cur_heading"][b] = e["cur_node"], e["cur_pos"], e["cur_heading"]
    out["_dims"] = (B, Nmax, Mmax, Fmax)
    return out


def assemble_on_device(batch: Dict[str, np.ndarray], device, G: Optional[int] = None,
                       keep_compact: bool = False) -> Dict[str, torch.Tensor]:
    """One H2D copy per compact array + one kernel.  Raises without the HIP library / a GPU (no CPU fallback).
    ``keep_compact``: also return the uploaded compact tensors (plus ``_dims``) under ``"compact"``, for ``decide.RolloutDecider``."""
    dev = torch.device(device)
    if dev.type != "cuda":
        raise _lib.EtpError("etp_gmap_assemble needs an MI355X (cuda/hip device); no CPU fallback exists")
    L = _lib.lib()
    B, Nmax, Mmax, Fmax = batch["_dims"]
    need = int((1 + batch["n_nodes"] + batch["n_ghost"]).max())
    G = need if G is None else G
    if G < need:
        raise ValueError(f"G={G} < 1 + nodes + ghosts = {need}")
    t = {k: torch.from_numpy(v).to(dev) for k, v in batch.items() if k != "_dims"}
    out = {
        "gmap_step_ids": torch.empty(B, G, dtype=torch.int64, device=dev),
        "gmap_masks": torch.empty(B, G, dtype=torch.bool, device=dev),
        "gmap_visited_masks": torch.empty(B, G, dtype=torch.bool, device=dev),
        "gmap_pos_fts": torch.empty(B, G, 7, dtype=torch.float32, device=dev),
        "gmap_pair_dists": torch.empty(B, G, G, dtype=torch.float32, device=dev),
    }
    check(L.etp_gmap_assemble(ptr(t["node_pos"]), ptr(t["node_step"]), ptr(t["n_nodes"]), ptr(t["adj"]), ptr(t["ghost_pos"]),
                              ptr(t["n_ghost"]), ptr(t["front_ptr"]), ptr(t["front_idx"]), ptr(t["cur_node"]), ptr(t["cur_pos"]),
                              ptr(t["cur_heading"]), B, Nmax, Mmax, Fmax, G, ptr(out["gmap_step_ids"]), ptr(out["gmap_masks"]),
                              ptr(out["gmap_visited_masks"]), ptr(out["gmap_pos_fts"]), ptr(out["gmap_pair_dists"]),
                              torch.cuda.current_stream(dev).cuda_stream), "etp_gmap_assemble")
    if keep_compact:
        out["compact"] = dict(t, _dims=batch["_dims"])
    return out


def nav_gmap_variable(gmaps: Sequence, cur_vp: Sequence[str], cur_pos, cur_heading: Sequence[float], device,
                      keep_compact: bool = False) -> dict:
    """Drop-in for RLTrainer._nav_gmap_variable (ss_trainer_ETP.py:344-417) minus ``gmap_img_fts`` (see module docstring);
    ``cur_heading[i]`` replaces ``cur_ori[i]`` (= heading_from_quaternion(cur_ori[i])).  ``keep_compact``: the uploaded compact
    tensors come back under ``"compact"`` (pop it before the dict goes to the policy) for ``decide.RolloutDecider.decide``."""
    eps = [pack_episode(g, cur_vp[i], cur_pos[i], cur_heading[i]) for i, g in enumerate(gmaps)]
    out = assemble_on_device(pack_batch(eps), device, keep_compact=keep_compact)
    out["gmap_vp_ids"] = [[None] + list(g.node_pos.keys()) + list(g.ghost_pos.keys()) for g in gmaps]
    out["no_vp_left"] = [len(g.ghost_pos) == 0 for g in gmaps]
    return out


# ---- node embeddings from a device-resident store (device-store mode) ---------------------------------------------------
def pack_img_csr(gmaps: Sequence, row_offsets: Sequence[int], G: int, n_store_rows: int):
    """CSR over the embedding store for the padded [B*G] node list ([stop] and padding: empty rows -> zeros), plus its
    transpose for the backward.  row_offsets[b] shifts episode b's row ids into the concatenated store."""
    ptr_f, idx_f, w_f = [0], [], []
    rev: List[list] = [[] for _ in range(n_store_rows)]
    for b, g in enumerate(gmaps):
        vps = [None] + list(g.node_pos.keys()) + list(g.ghost_pos.keys())
        if len(vps) > G:
            raise ValueError(f"G={G} < {len(vps)} graph entries")
        for t in range(G):
            if 1 <= t < len(vps):
                rows, w = g.embed_rows(vps[t])
                for r in rows:
                    idx_f.append(row_offsets[b] + r); w_f.append(w); rev[row_offsets[b] + r].append((b * G + t, w))
            ptr_f.append(len(idx_f))
    ptr_b, idx_b, w_b = [0], [], []
    for r in rev:
        for n, w in r:
            idx_b.append(n); w_b.append(w)
        ptr_b.append(len(idx_b))
    i32 = lambda x: torch.tensor(x, dtype=torch.int32)
    f32 = lambda x: torch.tensor(x, dtype=torch.float32)
    return (i32(ptr_f), i32(idx_f), f32(w_f)), (i32(ptr_b), i32(idx_b), f32(w_b))


class _GatherRows(torch.autograd.Function):
    @staticmethod
    def forward(ctx, store, n_out, fwd, bwd):
        L = _lib.lib()
        R, H = store.shape
        out = torch.empty(n_out, H, dtype=torch.float32, device=store.device)
        s = torch.cuda.current_stream(store.device).cuda_stream
        check(L.etp_gather_sum(_lib.ETP_F32, ptr(store), ptr(fwd[0]), ptr(fwd[1]), ptr(fwd[2]), ptr(out), n_out, H, 0, s),
              "etp_gather_sum")
        ctx.bwd, ctx.R = bwd, R
        return out

    @staticmethod
    def backward(ctx, d_out):
        L = _lib.lib()
        d_out = d_out.float().contiguous()
        H = d_out.shape[1]
        d_store = torch.empty(ctx.R, H, dtype=torch.float32, device=d_out.device)
        s = torch.cuda.current_stream(d_out.device).cuda_stream
        b = ctx.bwd
        check(L.etp_gather_sum(_lib.ETP_F32, ptr(d_out), ptr(b[0]), ptr(b[1]), ptr(b[2]), ptr(d_store), ctx.R, H, 0, s),
              "etp_gather_sum (transposed)")
        return d_store, None, None, None


def gather_rows(store: torch.Tensor, gmaps: Sequence, row_offsets: Sequence[int], G: int) -> torch.Tensor:
    """gmap_img_fts [B,G,H] (fp32) from the embedding store [R,H] on the device; differentiable w.r.t. the store.  ``store``: a tensor,
    or an ``EmbedStore`` (its rows used so far, differentiable w.r.t. the pano_embeds of every ``append``)."""
    if isinstance(store, EmbedStore):
        store = store.rows()
    if store.device.type != "cuda":
        raise _lib.EtpError("etp_gather_sum needs an MI355X (cuda/hip device); no CPU fallback exists")
    fwd, bwd = pack_img_csr(gmaps, row_offsets, G, store.shape[0])
    dev = store.device
    fwd = tuple(x.to(dev) for x in fwd)
    bwd = tuple(x.to(dev) for x in bwd)
    out = _GatherRows.apply(store.float().contiguous(), len(gmaps) * G, fwd, bwd)
    return out.view(len(gmaps), G, store.shape[1])


# ---- the map itself on the device (csrc/gmap_update.hip): update_graph in one launch, nothing re-serialised --------------------
GMAP_FMAX, GMAP_HDR, GMAP_KMAX = 512, 8, 16                   # ETP_GMAP_FMAX, ETP_GMAP_HDR, the kernel's candidate limit
GMAP_ERR_CAPACITY, GMAP_ERR_INPUT, GMAP_ERR_ROW = 1, 2, 4     # ETP_GMAP_ERR_*
GMAP_EDGE, GMAP_NEW, GMAP_MERGED = 1, 2, 3                    # ETP_GMAP_*: what became of a candidate (record, bits 24 ..)
_NO_GPU = "the device-resident map (etp_gmap_update) needs an MI355X (cuda/hip device); no CPU fallback exists"


# ---- the embedding store itself (csrc/pano_store.hip): panorama outputs to rows, one launch per step and direction ------------------
PSTORE_ERR_EMPTY, PSTORE_ERR_MASKED, PSTORE_ERR_COUNT, PSTORE_ERR_ROW = 1, 2, 4, 8     # ETP_PSTORE_ERR_*
PSTORE_VMAX = 64                                              # views per panorama the kernels take (one lane per view)


def _alias_rows(buf: torch.Tensor, r0: int, n: int) -> torch.Tensor:
    """rows r0 .. r0+n-1 of ``buf`` as a tensor of its own over the same memory: no view of ``buf`` in autograd's eyes, so the
    kernels' writes into the buffer and ``reset`` never meet autograd's in-place bookkeeping"""
    H = buf.shape[1]
    return torch.empty(0, dtype=buf.dtype, device=buf.device).set_(buf.untyped_storage(), buf.storage_offset() + r0 * H, (n, H), (H, 1))


class _PanoStoreFn(torch.autograd.Function):
    """pano_embeds [B,V,H] -> the call's block of store rows (etp_pano_store_fwd writes them into the store's buffer); the backward is
    etp_pano_store_bwd on the block's gradient with block-relative rows.  meta [3,B] int32: absolute base, n_cand, block-relative base."""

    @staticmethod
    def forward(ctx, pano_embeds, store, masks, nav_types, meta, status, r0, n_rows):
        B, V, H = pano_embeds.shape
        check(_lib.lib().etp_pano_store_fwd(ptr(pano_embeds), ptr(masks), ptr(nav_types), ptr(meta[0]), ptr(meta[1]), B, V, H, ptr(store.buf),
                                            store.capacity, ptr(status), torch.cuda.current_stream(pano_embeds.device).cuda_stream),
              "etp_pano_store_fwd")
        ctx.save_for_backward(masks, nav_types, meta)
        ctx.dims = (B, V, H, n_rows)
        return _alias_rows(store.buf, r0, n_rows)

    @staticmethod
    def backward(ctx, d_block):
        masks, nav_types, meta = ctx.saved_tensors
        B, V, H, n_rows = ctx.dims
        d_block = d_block.float().contiguous()
        if d_block.data_ptr() % 16:
            d_block = d_block.clone()
        d_pano = torch.empty(B, V, H, dtype=torch.float32, device=d_block.device)
        check(_lib.lib().etp_pano_store_bwd(ptr(d_block), ptr(masks), ptr(nav_types), ptr(meta[2]), ptr(meta[1]), B, V, H, n_rows, ptr(d_pano),
                                            0, torch.cuda.current_stream(d_block.device).cuda_stream), "etp_pano_store_bwd")
        return d_pano, None, None, None, None, None, None, None


class _JoinBlocks(torch.autograd.Function):
    """the blocks of every ``append`` so far -> the store's rows [R,H] as ONE tensor (they already lie behind one another in the
    buffer: nothing is copied); the backward hands each block its slice of d_store, and autograd sums what every later step sent to
    a block before that block's _PanoStoreFn.backward runs."""

    @staticmethod
    def forward(ctx, store, R, *blocks):
        ctx.spans = store._spans[:len(blocks)]
        return _alias_rows(store.buf, 0, R)

    @staticmethod
    def backward(ctx, d_store):
        return (None, None) + tuple(d_store[r0:r0 + n] if need else None for (r0, n), need in zip(ctx.spans, ctx.needs_input_grad[2:]))


class EmbedStore:
    """The embedding store of one rollout: one fp32 [capacity_rows, hidden] buffer on the device whose rows ``DeviceGraphMaps.update``,
    ``GraphMapLite.update_graph`` (device-store mode), ``DeviceGraphMaps.img_fts`` and ``gather_rows`` index.

        store = EmbedStore(capacity_rows, hidden, device); store.reset()                     # once per rollout
        cur_rows, cand_rows = store.append(pano_embeds, pano_masks, nav_types, n_cand)      # per step: ss_trainer_ETP.py:838-839, 864-865
        maps.update(..., cur_rows, cand_rows); gmap_img_fts = maps.img_fts(store, G)
        ... loss.backward(); store.check()

    ``append`` gives episode b of the call ``1 + n_cand[b]`` consecutive rows behind the rows used so far, in episode order: the masked
    panorama mean, then the views with ``nav_types == 1`` in view order.  It never synchronises: what the kernel flags (no unmasked view,
    a candidate at a masked-out view, a candidate count other than ``n_cand[b]``) stays on the device until ``check()`` copies the
    status vectors of all calls in one transfer and raises.  With autograd on, the gradient of every later ``img_fts`` / ``gather_rows``
    flows through the rows into the ``pano_embeds`` of the call that wrote them; under ``torch.no_grad()`` no graph is built."""

    def __init__(self, capacity_rows: int, hidden: int, device):
        if hidden not in (256, 512, 768) or capacity_rows < 1:
            raise ValueError(f"hidden is 256, 512 or 768 and capacity_rows positive (got {hidden}, {capacity_rows})")
        self.capacity, self.hidden, self.device = int(capacity_rows), int(hidden), torch.device(device)
        self.buf = torch.empty(self.capacity, self.hidden, dtype=torch.float32, device=self.device)
        self.reset()

    def reset(self) -> None:
        self.buf.zero_()
        self.rows_used = 0
        self._blocks: List[torch.Tensor] = []                 # one per append, in row order
        self._spans: List[tuple] = []                         # (first row, rows) of each
        self._status: List[torch.Tensor] = []
        self._checked = 0                                     # calls whose status check() has already seen

    def append(self, pano_embeds: torch.Tensor, pano_masks: torch.Tensor, nav_types: torch.Tensor, n_cand: Sequence[int]):
        """-> (cur_rows [B], cand_rows [B][n_cand[b]]) as Python ints.  ``pano_embeds`` [B,V,H] fp32, ``pano_masks`` [B,V] bool or uint8,
        ``nav_types`` [B,V] int64, ``n_cand``: host list (``len(wp_outputs['cand_angles'][i])``).  ValueError before anything is launched,
        the store unchanged: rows beyond the capacity, n_cand[b] outside 0 .. 16, V outside 1 .. 64, wrong shapes or dtypes."""
        if not (torch.is_tensor(pano_embeds) and pano_embeds.dim() == 3 and pano_embeds.dtype == torch.float32 and pano_embeds.shape[2] == self.hidden):
            raise ValueError(f"pano_embeds is a float32 tensor [B, V, {self.hidden}]")
        B, V, H = pano_embeds.shape
        if not (1 <= V <= PSTORE_VMAX and B >= 1):
            raise ValueError(f"B >= 1 and 1 <= V <= {PSTORE_VMAX} views (got B={B}, V={V})")
        if not (torch.is_tensor(pano_masks) and tuple(pano_masks.shape) == (B, V) and pano_masks.dtype in (torch.bool, torch.uint8)):
            raise ValueError(f"pano_masks is a bool or uint8 tensor [{B}, {V}]")
        if not (torch.is_tensor(nav_types) and tuple(nav_types.shape) == (B, V) and nav_types.dtype == torch.int64):
            raise ValueError(f"nav_types is an int64 tensor [{B}, {V}]")
        if any(t.device != self.buf.device for t in (pano_embeds, pano_masks, nav_types)):
            raise ValueError(f"the store lives on {self.device}; so must pano_embeds, pano_masks and nav_types")
        ks = [int(k) for k in n_cand]
        if len(ks) != B or any(k < 0 or k > GMAP_KMAX for k in ks):
            raise ValueError(f"n_cand holds one count in 0 .. {GMAP_KMAX} per episode (got {ks} for B={B})")
        n_rows = B + sum(ks)
        if self.rows_used + n_rows > self.capacity:
            raise ValueError(f"{self.rows_used} rows used + {n_rows} new > capacity {self.capacity}")
        if self.device.type != "cuda":
            raise _lib.EtpError("the embedding store (etp_pano_store_fwd) needs an MI355X (cuda/hip device); no CPU fallback exists")
        r0 = self.rows_used
        rel = np.concatenate([[0], np.cumsum([1 + k for k in ks])[:-1]]).astype(np.int32)
        meta = torch.from_numpy(np.stack([rel + r0, np.asarray(ks, dtype=np.int32), rel]).astype(np.int32)).pin_memory().to(self.device, non_blocking=True)
        status = torch.empty(B, dtype=torch.int32, device=self.device)
        masks = pano_masks.contiguous()
        masks = masks.view(torch.uint8) if masks.dtype == torch.bool else masks
        block = _PanoStoreFn.apply(pano_embeds.contiguous(), self, masks, nav_types.contiguous(), meta, status, r0, n_rows)
        self._blocks.append(block); self._spans.append((r0, n_rows)); self._status.append(status)
        self.rows_used = r0 + n_rows
        base = (rel + r0).tolist()
        return base, [[base[b] + 1 + j for j in range(ks[b])] for b in range(B)]

    def rows(self) -> torch.Tensor:
        """the rows used so far, [rows_used, H], over the buffer's memory; with autograd on, differentiable with respect to the
        pano_embeds of every append"""
        R = self.rows_used
        if torch.is_grad_enabled() and any(b.requires_grad for b in self._blocks):
            return _JoinBlocks.apply(self, R, *self._blocks)
        return self.buf[:R]

    def check(self) -> None:
        """one device-to-host copy of the status vectors of every append since the last check; raises naming call and episode"""
        new = self._status[self._checked:]
        if not new:
            return
        flags = torch.cat(new).cpu().numpy()
        first, self._checked = self._checked, len(self._status)
        if flags.any():
            bad, o = [], 0
            for c, s in enumerate(new):
                bad += [f"call {first + c} episode {b}: flags {int(f)}" for b, f in enumerate(flags[o:o + len(s)]) if f]
                o += len(s)
            raise _lib.EtpError("etp_pano_store_fwd flagged (ETP_PSTORE_ERR_*: 1 no unmasked view, 2 candidate at a masked-out view, "
                                "4 candidate count != n_cand, 8 rows outside the store): " + "; ".join(bad))


class GraphMapView:
    """What the host keeps of one environment's device-resident map: names and positions under the reference's attribute names
    (graph_utils.py:143-161), filled from the kernel's record -- no distance is computed here.  ``RolloutDecider``,
    ``env_actions_from_record`` and the trainer's ``_teacher_action_new`` read it like a GraphMapLite."""

    def __init__(self, has_real_pos: bool):
        self.has_real_pos = has_real_pos
        self.node_pos: Dict[str, np.ndarray] = {}
        self.node_stepId: Dict[str, int] = {}
        self.ghost_cnt = 0
        self.ghost_pos: Dict[str, list] = {}
        self.ghost_mean_pos: Dict[str, np.ndarray] = {}
        self.ghost_aug_pos: Dict[str, np.ndarray] = {}
        self.ghost_fronts: Dict[str, list] = {}
        self.ghost_real_pos: Dict[str, list] = {}
        self.node_stop_scores: Dict[str, float] = {}
        self._sum: Dict[str, np.ndarray] = {}
        self.max_row = -1                                     # the largest row of the embedding store this map was ever given
        self.pending_delete = -1                              # index, in the DEVICE's order, of the ghost the next update removes

    def delete_ghost(self, vp: str) -> None:
        """graph_utils.py:185-191 on the view; the device drops the ghost at the start of the next update (nothing reads the map
        in between, ss_trainer_ETP.py:976-977)."""
        if self.pending_delete >= 0:
            raise ValueError("one ghost can be deleted between two updates (consume_ghost); a second delete_ghost is pending")
        self.pending_delete = list(self.ghost_pos.keys()).index(vp)
        for d in (self.ghost_pos, self.ghost_mean_pos, self.ghost_fronts, self._sum):
            d.pop(vp)
        self.ghost_aug_pos.pop(vp, None)
        if self.has_real_pos:
            self.ghost_real_pos.pop(vp)


class DeviceGraphMaps:
    """The maps of ``num_envs`` environments resident on the device, one state record per ORIGINAL environment, and a
    ``GraphMapView`` of each on the host.

        maps = DeviceGraphMaps(num_envs, device, has_real_pos, loc_noise, merge_ghost, ghost_aug)
        cur_vp, cand_vp, cand_pos = maps.identify_node(cur_pos, cur_heading, cand_angles, cand_distances)
        maps.update(prev_vp, step_ids, cur_vp, cur_pos, cur_heading, cand_pos, cur_rows, cand_rows, cand_real_pos)
        nav_inputs = maps.nav_inputs()                        # the dict of nav_gmap_variable(..., keep_compact=True)
        nav_inputs["gmap_img_fts"] = maps.img_fts(store, nav_inputs["gmap_masks"].shape[1])
        ... decider.decide(nav_logits, maps.gmaps, cur_vp, ..., compact=nav_inputs.pop("compact")); maps.pause(i) beside decider.pause(i)

    ``update`` is one host-to-device copy (every argument in one buffer), one launch of ``etp_gmap_update`` and ONE device-to-host
    copy (the record).  What the kernel would flag (a full map, a ``prev_vp`` that is no node) is refused on the host before the launch,
    so a ``ValueError`` leaves views and device records as they were."""

    def __init__(self, num_envs: int, device, has_real_pos: bool, loc_noise: float, merge_ghost: bool, ghost_aug: float):
        self.num_envs, self.device = int(num_envs), torch.device(device)
        self.has_real_pos, self.loc_noise, self.merge_ghost, self.ghost_aug = bool(has_real_pos), float(loc_noise), bool(merge_ghost), float(ghost_aug)
        self.state = None
        self.out: Dict[str, torch.Tensor] = {}
        if self.device.type == "cuda":
            S, dev = self.num_envs, self.device
            self.slot_bytes = int(_lib.lib().etp_gmap_slot_bytes())
            self.state = torch.empty(S * self.slot_bytes, dtype=torch.uint8, device=dev)
            f32, i32 = (lambda *s: torch.empty(*s, dtype=torch.float32, device=dev)), (lambda *s: torch.empty(*s, dtype=torch.int32, device=dev))
            self.out = {"node_pos": f32(S, MAX_NODES, 3), "node_step": i32(S, MAX_NODES), "n_nodes": i32(S), "adj": f32(S, MAX_NODES, MAX_NODES),
                        "ghost_pos": f32(S, MAX_GHOSTS, 3), "n_ghost": i32(S), "front_ptr": i32(S, MAX_GHOSTS + 1), "front_idx": i32(S, GMAP_FMAX),
                        "cur_node": i32(S), "cur_pos": f32(S, 3), "cur_heading": f32(S), "record": i32(S, GMAP_HDR + GMAP_KMAX)}
        self.reset()

    # ---- bookkeeping (RolloutDecider's) ----
    def reset(self) -> None:
        self.active = list(range(self.num_envs))
        self.views = [GraphMapView(self.has_real_pos) for _ in range(self.num_envs)]
        self.B = 0
        self._slot_dev = None
        if self.state is not None:
            slots = torch.arange(self.num_envs, dtype=torch.int32).to(self.device)
            check(_lib.lib().etp_gmap_reset(ptr(self.state), self.num_envs, ptr(slots), self.num_envs,
                                            torch.cuda.current_stream(self.device).cuda_stream), "etp_gmap_reset")

    def pause(self, i: int) -> None:
        """``not_done_index.pop(i)`` (ss_trainer_ETP.py:1036-1044): the environment's record stays behind, untouched"""
        self.active.pop(i)

    @property
    def gmaps(self) -> List[GraphMapView]:
        return [self.views[s] for s in self.active]

    def identify_node(self, cur_pos, cur_heading, cand_angles, cand_distances):
        """GraphMap.identify_node (graph_utils.py:177-183, estimate_cand_pos :61-71) for every active environment -> (cur_vp [B],
        cand_vp [B][K_b], cand_pos [B][K_b] arrays of 3).  A Python loop over the environments (K_b differs) with GraphMapLite's numpy
        expressions on each, so the positions are its bits; it is not one vectorised call."""
        cur_vp, cand_vp, cand_pos = [], [], []
        for i, v in enumerate(self.gmaps):
            vp = str(len(v.node_pos))
            ang = (float(cur_heading[i]) + np.asarray(cand_angles[i], dtype=np.float64)) % (2 * np.pi)
            dis = np.asarray(cand_distances[i], dtype=np.float64)
            p = np.zeros((len(ang), 3))
            p[:, 0] = cur_pos[i][0] - dis * np.sin(ang)
            p[:, 1] = cur_pos[i][1]
            p[:, 2] = cur_pos[i][2] - dis * np.cos(ang)
            cur_vp.append(vp); cand_vp.append([f"{vp}_{k}" for k in range(len(ang))]); cand_pos.append([x for x in p])
        return cur_vp, cand_vp, cand_pos

    # ---- the update ----
    def update(self, prev_vp, step_ids, cur_vp, cur_pos, cur_heading, cand_pos, cur_rows, cand_rows, cand_real_pos=None,
               generator=None, noise=None) -> np.ndarray:
        """GraphMap.update_graph for every active environment -> the record [B, 8 + 16] (include/etpnav_hip.h).  ``prev_vp[i]``: a
        node's name or None; ``step_ids``: one int or [B]; ``cand_pos[i]`` / ``cand_rows[i]``: the K_i <= 16 candidates and their rows
        of the embedding store; ``noise`` [B,192,3]: standard normals for ghost_aug (drawn from ``generator``, a numpy Generator,
        when absent)."""
        views, B, K = self.gmaps, len(self.active), GMAP_KMAX
        if not (B and B == len(cur_vp) == len(prev_vp) == len(cand_pos) == len(cand_rows) == len(cur_rows)):
            raise ValueError(f"{len(self.active)} active environments, {len(cur_vp)} viewpoints, {len(cand_pos)} candidate lists")
        ks = [len(c) for c in cand_pos]
        if max(ks) > K or any(len(r) != k for r, k in zip(cand_rows, ks)):
            raise ValueError(f"at most {K} candidates per step, each with its row of the embedding store")
        for v, vp in zip(views, cur_vp):
            if vp != str(len(v.node_pos)):
                raise ValueError(f"viewpoint {vp!r}: the next node of this map is {str(len(v.node_pos))!r} (identify_node)")
        # what the kernel would flag is refused here, before the launch: a flagged episode would leave the other episodes' records
        # advanced and no view mirrored.  The views hold the counts after the pending deletion.
        for i, v in enumerate(views):
            n, m, f = len(v.node_pos), len(v.ghost_pos), sum(len(x) for x in v.ghost_fronts.values())
            if n + 1 > MAX_NODES or m + ks[i] > MAX_GHOSTS or f + ks[i] > GMAP_FMAX:
                raise ValueError(f"episode {i}: the map is full (<= {MAX_NODES} visited nodes, {MAX_GHOSTS} ghosts, {GMAP_FMAX} absorbed candidates)")
            if prev_vp[i] is not None and not (str(prev_vp[i]).isdigit() and int(prev_vp[i]) < n):
                raise ValueError(f"episode {i}: prev_vp {prev_vp[i]!r} is no visited node of this map")
            rows = [int(cur_rows[i])] + [int(r) for r in cand_rows[i]]
            if min(rows) < 0:
                raise ValueError(f"episode {i}: rows of the embedding store are >= 0")
        if self.state is None:
            raise _lib.EtpError(_NO_GPU)
        for i, v in enumerate(views):
            v.max_row = max([v.max_row, int(cur_rows[i])] + [int(r) for r in cand_rows[i]])
        use_noise = self.ghost_aug != 0
        if use_noise:
            noise = (generator if generator is not None else np.random.default_rng()).standard_normal((B, MAX_GHOSTS, 3)) if noise is None \
                else np.ascontiguousarray(noise, dtype=np.float64).reshape(B, MAX_GHOSTS, 3)
        # one buffer, one copy: the doubles first, then the 4-byte operands
        f64 = np.zeros(B * 3 + B * K * 3 + (B * MAX_GHOSTS * 3 if use_noise else 0))
        i32 = np.zeros(B * (6 + K) + B, dtype=np.int32)
        cp = f64[:B * 3].reshape(B, 3)
        cq = f64[B * 3:B * 3 + B * K * 3].reshape(B, K, 3)
        cp[:] = np.asarray(cur_pos, dtype=np.float64).reshape(B, 3)
        if use_noise:
            f64[B * 3 + B * K * 3:] = noise.ravel()
        cols = i32[:B * 6].reshape(6, B)                      # slot, prev_node, step_id, n_cand, cur_row, del_ghost
        crow = i32[B * 6:B * (6 + K)].reshape(B, K)
        crow[:] = -1
        cols[0], cols[2], cols[3], cols[4] = self.active, step_ids, ks, cur_rows
        for i, v in enumerate(views):
            cols[1, i] = -1 if prev_vp[i] is None else int(prev_vp[i])
            cols[5, i] = v.pending_delete
            if ks[i]:
                cq[i, :ks[i]] = np.asarray(cand_pos[i], dtype=np.float64).reshape(ks[i], 3)
                crow[i, :ks[i]] = cand_rows[i]
        i32[B * (6 + K):].view(np.float32)[:] = np.asarray(cur_heading, dtype=np.float32).reshape(B)
        host = np.concatenate([f64.view(np.uint8), i32.view(np.uint8)])
        dev_buf = torch.from_numpy(host).to(self.device)
        base = dev_buf.data_ptr()
        o8, o4 = (lambda n: base + 8 * n), (lambda n: base + f64.nbytes + 4 * n)
        o = self.out
        check(_lib.lib().etp_gmap_update(
            ptr(self.state), self.num_envs, o4(0), o4(B), o4(2 * B), o8(0), o4(B * (6 + K)), o8(B * 3), o4(3 * B), o4(4 * B), o4(6 * B), o4(5 * B),
            o8(B * 3 + B * K * 3) if use_noise else None, self.loc_noise, int(self.merge_ghost), self.ghost_aug, B, K,
            ptr(o["node_pos"]), ptr(o["node_step"]), ptr(o["n_nodes"]), ptr(o["adj"]), ptr(o["ghost_pos"]), ptr(o["n_ghost"]),
            ptr(o["front_ptr"]), ptr(o["front_idx"]), ptr(o["cur_node"]), ptr(o["cur_pos"]), ptr(o["cur_heading"]), ptr(o["record"]),
            torch.cuda.current_stream(self.device).cuda_stream), "etp_gmap_update")
        self._slot_dev = dev_buf[f64.nbytes:f64.nbytes + 4 * B].view(torch.int32)
        rec = o["record"][:B].cpu().numpy()                   # the one host synchronisation of the update
        self.B = B
        if rec[:, 2].any():                                  # refused above on the host; a flag here means view and record disagree
            raise _lib.EtpError(f"etp_gmap_update flagged episodes {np.nonzero(rec[:, 2])[0].tolist()} (flags {rec[:, 2].tolist()}): "
                                f"the views no longer describe the device records; reset()")
        self._mirror(rec, views, cur_vp, cp, step_ids, cq, cand_real_pos, noise if use_noise else None)
        return rec

    def _mirror(self, rec, views, cur_vp, cur_pos, step_ids, cand_pos, cand_real_pos, noise) -> None:
        """the views after the update, from the record alone: O(candidates) dictionary work per episode, no distances"""
        steps = np.broadcast_to(np.asarray(step_ids), (len(views),))
        scale = np.array([self.ghost_aug, 0.0, self.ghost_aug])
        for i, v in enumerate(views):
            v.pending_delete = -1
            vp = cur_vp[i]
            v.node_pos[vp], v.node_stepId[vp] = cur_pos[i].copy(), int(steps[i])
            for k, c in enumerate(rec[i, GMAP_HDR:].tolist()):
                if c < 0:
                    break
                kind, tgt = c >> 24, c & 0xFFFFFF
                if kind == GMAP_EDGE:
                    continue
                gvp, pos = f"g{tgt}", cand_pos[i, k].copy()
                real = cand_real_pos[i][k] if self.has_real_pos else None
                if kind == GMAP_NEW:
                    v.ghost_pos[gvp], v.ghost_mean_pos[gvp], v._sum[gvp], v.ghost_fronts[gvp] = [pos], pos, pos.copy(), [vp]
                    if self.has_real_pos:
                        v.ghost_real_pos[gvp] = [real]
                else:
                    v.ghost_pos[gvp].append(pos)
                    v._sum[gvp] = v._sum[gvp] + pos
                    v.ghost_mean_pos[gvp] = v._sum[gvp] / np.float64(len(v.ghost_pos[gvp]))
                    v.ghost_fronts[gvp].append(vp)
                    if self.has_real_pos:
                        v.ghost_real_pos[gvp].append(real)
            v.ghost_cnt = int(rec[i, 4])
            if int(rec[i, 0]) != len(v.node_pos) or int(rec[i, 1]) != len(v.ghost_pos):
                raise _lib.EtpError(f"episode {i}: the view holds {len(v.node_pos)} nodes / {len(v.ghost_pos)} ghosts, the device {rec[i, :2].tolist()}")
            if noise is None or not v.ghost_mean_pos:
                v.ghost_aug_pos = {k: np.array(p, dtype=np.float64) for k, p in v.ghost_mean_pos.items()}
            else:
                m = len(v.ghost_mean_pos)
                aug = np.asarray(list(v.ghost_mean_pos.values())) + np.clip(noise[i, :m] * scale, -self.ghost_aug, self.ghost_aug)
                v.ghost_aug_pos = dict(zip(v.ghost_mean_pos.keys(), aug))

    # ---- the consumers' inputs ----
    def compact(self) -> dict:
        """the arrays the last update emitted, as ``assemble_on_device(..., keep_compact=True)`` returns them"""
        if self.state is None or not self.B:
            raise _lib.EtpError(_NO_GPU if self.state is None else "no update has run yet")
        c = {k: v[:self.B] for k, v in self.out.items() if k != "record"}
        c["_dims"] = (self.B, MAX_NODES, MAX_GHOSTS, GMAP_FMAX)
        return c

    def nav_inputs(self, G: Optional[int] = None) -> dict:
        """the dict of ``nav_gmap_variable(..., keep_compact=True)`` (without gmap_img_fts: ``img_fts``) from the emitted arrays:
        one launch of etp_gmap_assemble, nothing uploaded"""
        t = self.compact()
        views, B, dev = self.gmaps, self.B, self.device
        need = max(1 + len(v.node_pos) + len(v.ghost_pos) for v in views)
        G = need if G is None else G
        if G < need:
            raise ValueError(f"G={G} < 1 + nodes + ghosts = {need}")
        out = {
            "gmap_step_ids": torch.empty(B, G, dtype=torch.int64, device=dev),
            "gmap_masks": torch.empty(B, G, dtype=torch.bool, device=dev),
            "gmap_visited_masks": torch.empty(B, G, dtype=torch.bool, device=dev),
            "gmap_pos_fts": torch.empty(B, G, 7, dtype=torch.float32, device=dev),
            "gmap_pair_dists": torch.empty(B, G, G, dtype=torch.float32, device=dev),
        }
        check(_lib.lib().etp_gmap_assemble(ptr(t["node_pos"]), ptr(t["node_step"]), ptr(t["n_nodes"]), ptr(t["adj"]), ptr(t["ghost_pos"]),
                                           ptr(t["n_ghost"]), ptr(t["front_ptr"]), ptr(t["front_idx"]), ptr(t["cur_node"]), ptr(t["cur_pos"]),
                                           ptr(t["cur_heading"]), B, MAX_NODES, MAX_GHOSTS, GMAP_FMAX, G, ptr(out["gmap_step_ids"]),
                                           ptr(out["gmap_masks"]), ptr(out["gmap_visited_masks"]), ptr(out["gmap_pos_fts"]),
                                           ptr(out["gmap_pair_dists"]), torch.cuda.current_stream(dev).cuda_stream), "etp_gmap_assemble")
        out["compact"] = t
        out["gmap_vp_ids"] = [[None] + list(v.node_pos.keys()) + list(v.ghost_pos.keys()) for v in views]
        out["no_vp_left"] = [len(v.ghost_pos) == 0 for v in views]
        return out

    def embed_csr(self, G: int, R: int):
        """-> (ptr_f, idx_f, w_f), (ptr_b, idx_b, w_b), status on the device: ``pack_img_csr`` from the states (etp_gmap_embed_csr)"""
        if self.state is None or not self.B:
            raise _lib.EtpError(_NO_GPU if self.state is None else "no update has run yet")
        views, B, dev = self.gmaps, self.B, self.device
        need = max(1 + len(v.node_pos) + len(v.ghost_pos) for v in views)
        if G < need:
            raise ValueError(f"G={G} < 1 + nodes + ghosts = {need}")
        nnz = max(1, sum(len(v.node_pos) + sum(len(f) for f in v.ghost_fronts.values()) for v in views))
        i32, f32 = (lambda n: torch.empty(n, dtype=torch.int32, device=dev)), (lambda n: torch.empty(n, dtype=torch.float32, device=dev))
        fwd, bwd, status = (i32(B * G + 1), i32(nnz), f32(nnz)), (i32(R + 1), i32(R), f32(R)), i32(B)
        check(_lib.lib().etp_gmap_embed_csr(ptr(self.state), self.num_envs, ptr(self._slot_dev), B, G, R, ptr(fwd[0]), ptr(fwd[1]), ptr(fwd[2]),
                                            ptr(bwd[0]), ptr(bwd[1]), ptr(bwd[2]), ptr(status), torch.cuda.current_stream(dev).cuda_stream),
              "etp_gmap_embed_csr")
        return fwd, bwd, status

    def img_fts(self, store: torch.Tensor, G: int) -> torch.Tensor:
        """gmap_img_fts [B,G,H] (fp32) from the embedding store [R,H]: ``gather_rows`` without the host-side CSR; differentiable
        with respect to the store.  ``store``: a tensor, or an ``EmbedStore`` (its rows used so far, differentiable with respect to the
        pano_embeds of every ``append``)"""
        if isinstance(store, EmbedStore):
            store = store.rows()
        if store.device.type != "cuda" or self.state is None:
            raise _lib.EtpError(_NO_GPU)
        top = max(v.max_row for v in self.gmaps)
        if top >= store.shape[0]:                             # the kernel would flag it (ETP_GMAP_ERR_ROW) and gather row 0 with weight 0
            raise ValueError(f"the maps hold row {top} of the embedding store, which has {store.shape[0]} rows")
        fwd, bwd, _ = self.embed_csr(G, int(store.shape[0]))   # rows and G were checked on the host: the status is all zero
        out = _GatherRows.apply(store.float().contiguous(), self.B * G, fwd, bwd)
        return out.view(self.B, G, store.shape[1])


# ---- panorama inputs: candidate views first, then the remaining panorama views (row a13, first half) -------------------
def vp_feature_variable(obs: dict, device) -> dict:
    """Drop-in for RLTrainer._vp_feature_variable (ss_trainer_ETP.py:308-342) on the device: three gathers
    (etp_vp_gather) instead of per-episode torch.cat / pad loops.  `obs` keys as in the reference: cand_img_idxes,
    cand_rgb, cand_depth, cand_angle_fts (lists of per-episode tensors), pano_rgb [B,12,F], pano_depth [B,12,Fd],
    pano_angle_fts [12,4].  (Forward only: these are detached perception features in the reference as well.)
    An `obs` from ETP.forward(mode='waypoint') with fuse_pano_inputs carries the five tensors already (waypoint.panorama_inputs built
    them in one launch, csrc/pano_inputs.hip): they are handed on as they are."""
    if "pano_inputs" in obs:
        return {k: obs["pano_inputs"][k] for k in ("rgb_fts", "dep_fts", "loc_fts", "nav_types", "view_lens")}
    dev = torch.device(device)
    if dev.type != "cuda":
        raise _lib.EtpError("etp_vp_gather needs an MI355X (cuda/hip device); no CPU fallback exists")
    L = _lib.lib()
    B = len(obs["cand_rgb"])
    P = obs["pano_rgb"].shape[1]
    ks = [int(x.shape[0]) for x in obs["cand_rgb"]]
    cand_ptr = torch.tensor(np.concatenate([[0], np.cumsum(ks)]), dtype=torch.int32, device=dev)
    mask = torch.zeros(B, P, dtype=torch.uint8)
    for i in range(B):
        mask[i, torch.as_tensor(np.asarray(obs["cand_img_idxes"][i], dtype=np.int64))] = 1
    V = max(k + P - int(mask[i].sum()) for i, k in enumerate(ks))
    mask = mask.to(dev)
    s = torch.cuda.current_stream(dev).cuda_stream
    nav_types = torch.empty(B, V, dtype=torch.int64, device=dev)
    view_lens = torch.empty(B, dtype=torch.int64, device=dev)
    out = {}
    for name, cand_key, pano_key in (("rgb_fts", "cand_rgb", "pano_rgb"), ("dep_fts", "cand_depth", "pano_depth"),
                                     ("loc_fts", "cand_angle_fts", "pano_angle_fts")):
        cand = torch.cat([torch.as_tensor(x, dtype=torch.float32) for x in obs[cand_key]], 0).to(dev).contiguous()
        pano = torch.as_tensor(obs[pano_key], dtype=torch.float32).to(dev).contiguous()
        F = pano.shape[-1]
        stride = 0 if pano.dim() == 2 else P * F
        o = torch.empty(B, V, F, dtype=torch.float32, device=dev)
        first = name == "rgb_fts"
        check(L.etp_vp_gather(ptr(cand), ptr(cand_ptr), ptr(pano), stride, ptr(mask), B, P, F, V, ptr(o),
                              ptr(nav_types) if first else None, ptr(view_lens) if first else None, s), "etp_vp_gather")
        out[name] = o
    out["nav_types"], out["view_lens"] = nav_types, view_lens
    return out


# ---- pre-training: GlobalMapEncoder._aggregate_gmap_features (pretrain_src/pretrain_src/model/vilmodel.py:585-619) ------
def pack_traj_csr(traj_vp_lens: Sequence[Sequence[int]], traj_vpids: Sequence[Sequence[str]],
                  traj_cand_vpids: Sequence[Sequence[Sequence[str]]], gmap_vpids: Sequence[Sequence], V: int, G: int):
    """CSR (+ transpose) that turns the flat panorama embeddings [sum_i T_i, V, H] of a batch of trajectories into the
    padded node features [B, G, H]: a visited node = mean of the valid views of the step that visited it (a later visit
    overwrites an earlier one); an unvisited node = mean of the candidate-view embeddings (view j of step t) over the
    steps at which it was seen while not yet visited; entry 0 ([stop]) and padding are zero rows."""
    ptr_f, idx_f, w_f = [0], [], []
    n_rows = sum(len(x) for x in traj_vp_lens) * V
    rev: List[list] = [[] for _ in range(n_rows)]
    base = 0
    for i in range(len(traj_vp_lens)):
        visited, unvisited = {}, {}
        for t, vp in enumerate(traj_vpids[i]):
            n = int(traj_vp_lens[i][t])
            visited[vp] = ([(base + t) * V + j for j in range(n)], 1.0 / n)
            for j, cvp in enumerate(traj_cand_vpids[i][t]):
                if cvp not in visited:
                    # a candidate slot beyond the step's valid views is a zero row in the reference (embeds * vp_masks,
                    # :599-600) that still counts in the mean: keep the slot, drop the row
                    unvisited.setdefault(cvp, []).append((base + t) * V + j if j < n else None)
        if len(gmap_vpids[i]) > G:
            raise ValueError(f"G={G} < {len(gmap_vpids[i])} graph entries")
        for g in range(G):
            if 1 <= g < len(gmap_vpids[i]):
                vp = gmap_vpids[i][g]
                rows, w = visited[vp] if vp in visited else (unvisited[vp], 1.0 / len(unvisited[vp]))
                for r in rows:
                    if r is None:
                        continue
                    idx_f.append(r); w_f.append(w); rev[r].append((i * G + g, w))
            ptr_f.append(len(idx_f))
        base += len(traj_vp_lens[i])
    ptr_b, idx_b, w_b = [0], [], []
    for r in rev:
        for n, w in r:
            idx_b.append(n); w_b.append(w)
        ptr_b.append(len(idx_b))
    i32 = lambda x: torch.tensor(x, dtype=torch.int32)
    f32 = lambda x: torch.tensor(x, dtype=torch.float32)
    return (i32(ptr_f), i32(idx_f), f32(w_f)), (i32(ptr_b), i32(idx_b), f32(w_b))


TRAJ_KMAX = 64                                                # etp_traj_nodes_*: candidate slots per step (one lane per slot)
TRAJ_ERR_COUNT_OR_LEN, TRAJ_ERR_VIEWS, TRAJ_ERR_STEPS, TRAJ_ERR_NODE = 1, 8, 16, 32     # ETP_TRAJ_ERR_* of etp_traj_nodes_fwd / _bwd
TRAJ_TABLES = ("step_off", "step_vp", "cand_count", "cand_vp", "gmap_id", "gmap_len")


def traj_descriptors(traj: dict, G: int, device) -> dict:
    """The integer tables etp_traj_nodes_fwd / _bwd read (include/etpnav_hip.h), from the string lists of any trajectory batch
    (``traj_vpids``, ``traj_cand_vpids``, ``gmap_vpids``): -> {step_off [B+1], step_vp [R], cand_count [R], cand_vp [R, Kmax], gmap_id [B, G],
    gmap_len [B]} int32 on ``device`` plus ``Kmax``.  Ids number a sample's viewpoints in the order they first appear; -1 is [stop] and
    padding.  One buffer (pinned when the device is a GPU), one copy.  The native loaders (pretrain_data.py) stage the same tables from
    their cached records instead."""
    vpids, cands, gvps = traj["traj_vpids"], traj["traj_cand_vpids"], traj["gmap_vpids"]
    B = len(vpids)
    steps = np.asarray([len(p) for p in vpids], dtype=np.int64)
    R = int(steps.sum())
    counts = np.asarray([len(c) for s in cands for c in s], dtype=np.int32)
    if len(cands) != B or len(gvps) != B or counts.size != R or any(len(s) != len(p) for s, p in zip(cands, vpids)):
        raise ValueError("traj_vpids, traj_cand_vpids and gmap_vpids describe different batches")
    Kmax = max(1, int(counts.max()) if R else 0)
    if Kmax > TRAJ_KMAX:
        raise ValueError(f"{Kmax} candidates at one step (at most {TRAJ_KMAX})")
    if max(len(g) for g in gvps) > G:
        raise ValueError(f"G={G} < {max(len(g) for g in gvps)} graph entries")
    shapes = {"step_off": (B + 1,), "step_vp": (R,), "cand_count": (R,), "cand_vp": (R, Kmax), "gmap_id": (B, G), "gmap_len": (B,)}
    offs, total = {}, 0
    for k in TRAJ_TABLES:
        offs[k] = total
        total += (int(np.prod(shapes[k])) + 3) // 4 * 4       # 16-byte pieces
    dev = torch.device(device)
    stage = torch.empty(total, dtype=torch.int32, pin_memory=dev.type == "cuda")
    host = stage.numpy()
    h = {k: host[offs[k]:offs[k] + int(np.prod(shapes[k]))].reshape(shapes[k]) for k in TRAJ_TABLES}
    host[:] = -1
    h["step_off"][0] = 0
    np.cumsum(steps, out=h["step_off"][1:])
    h["cand_count"][:] = counts
    h["gmap_len"][:] = [len(g) for g in gvps]
    r = 0
    for i in range(B):
        ids: Dict[str, int] = {}
        num = lambda vp: ids.setdefault(vp, len(ids))
        for t, vp in enumerate(vpids[i]):
            h["step_vp"][r] = num(vp)
            c = cands[i][t]
            if c:
                h["cand_vp"][r, :len(c)] = [num(x) for x in c]
            r += 1
        h["gmap_id"][i, :len(gvps[i])] = [-1 if vp is None else num(vp) for vp in gvps[i]]
    d = stage.to(dev, non_blocking=True)
    out = {k: d[offs[k]:offs[k] + int(np.prod(shapes[k]))].view(shapes[k]) for k in TRAJ_TABLES}
    out["Kmax"] = Kmax
    return out


def traj_status_message(status: np.ndarray, n_nodes: int, G: int) -> Optional[str]:
    """what the status words of etp_traj_nodes_fwd (the first ``n_nodes`` = B*G) and etp_traj_nodes_bwd (one per step) report, or None"""
    status = np.asarray(status)
    if not status.any():
        return None
    f, b = status[:n_nodes], status[n_nodes:]
    rows = [f"(sample {i // G}, node {i % G}): {int(f[i])}" for i in np.nonzero(f)[0].tolist()]
    steps = [f"step {i}: {int(b[i])}" for i in np.nonzero(b)[0].tolist()]
    return ("etp_traj_nodes flagged (ETP_TRAJ_ERR_*: 1 cand_count outside 0 .. Kmax or gmap_len outside 1 .. G, 8 view_lens outside "
            "1 .. V, 16 malformed step range, 32 a listed node neither visited nor named) -- forward rows " + (", ".join(rows) or "none") +
            "; backward " + (", ".join(steps) or "none"))


def traj_table_args(td: dict, view_lens: torch.Tensor) -> list:
    """the seven table pointers of etp_traj_nodes_fwd / _bwd, in the entry points' order"""
    return [ptr(td["step_off"]), ptr(td["step_vp"]), ptr(view_lens), ptr(td["cand_count"]), ptr(td["cand_vp"]), ptr(td["gmap_id"]),
            ptr(td["gmap_len"])]


class _TrajNodes(torch.autograd.Function):
    @staticmethod
    def forward(ctx, pano, view_lens, td, dims, status):
        B, R, V, G, H = dims
        out = torch.empty(B * G, H, dtype=torch.float32, device=pano.device)
        s = torch.cuda.current_stream(pano.device).cuda_stream
        check(_lib.lib().etp_traj_nodes_fwd(ptr(pano), *traj_table_args(td, view_lens), B, R, V,
                                            td["Kmax"], G, H, ptr(out), ptr(status), s), "etp_traj_nodes_fwd")
        ctx.td, ctx.view_lens, ctx.dims, ctx.status = td, view_lens, dims, status
        return out

    @staticmethod
    def backward(ctx, d_out):
        B, R, V, G, H = ctx.dims
        d_out = d_out.float().contiguous()
        if d_out.data_ptr() % 16:
            d_out = d_out.clone()
        d_pano = torch.empty(R * V, H, dtype=torch.float32, device=d_out.device)
        s = torch.cuda.current_stream(d_out.device).cuda_stream
        td = ctx.td
        check(_lib.lib().etp_traj_nodes_bwd(ptr(d_out), *traj_table_args(td, ctx.view_lens), B, R,
                                            V, td["Kmax"], G, H, ptr(d_pano), ctx.status.data_ptr() + 4 * B * G, s), "etp_traj_nodes_bwd")
        return d_pano, None, None, None, None


def aggregate_gmap_features(traj_embeds: torch.Tensor, traj_vp_lens, traj_vpids, traj_cand_vpids, gmap_vpids, G: int,
                            traj_dev: Optional[dict] = None):
    """Device version of GlobalMapEncoder._aggregate_gmap_features: traj_embeds [sum T, V, H] (output of the panorama
    encoder for every trajectory step) -> gmap_img_fts [B, G, H] incl. the zero [stop] row; differentiable.
    ``traj_dev`` (``traj_descriptors`` or a loader's ``TrajBatch.traj_dev``): no CSR is built, etp_traj_nodes_fwd / _bwd read the tables;
    ``traj_vp_lens`` may then be the device tensor ``view_lens`` [sum T] int64 and the three string lists are not read.  The kernels'
    status words land in ``traj_dev['status']`` [B*G + sum T]: ``traj_status_message`` reads them (nothing synchronises here)."""
    if traj_embeds.device.type != "cuda":
        raise _lib.EtpError("etp_gather_sum / etp_traj_nodes_fwd need an MI355X (cuda/hip device); no CPU fallback exists")
    R, V, H = traj_embeds.shape
    if traj_dev is not None:
        dev, B = traj_embeds.device, int(traj_dev["gmap_len"].numel())
        if tuple(traj_dev["gmap_id"].shape) != (B, G) or traj_dev["step_vp"].numel() != R:
            raise ValueError(f"the descriptors hold {traj_dev['step_vp'].numel()} steps and nodes {tuple(traj_dev['gmap_id'].shape)}; "
                             f"the call has {R} steps and G={G}")
        if torch.is_tensor(traj_vp_lens):
            vl = traj_vp_lens.to(dev, torch.int64).reshape(-1).contiguous()
        else:
            vl = torch.tensor([int(n) for s in traj_vp_lens for n in s], dtype=torch.int64).to(dev)
        if vl.numel() != R:
            raise ValueError(f"{vl.numel()} view lengths for {R} steps")
        traj_dev["status"] = status = torch.zeros(B * G + R, dtype=torch.int32, device=dev)
        out = _TrajNodes.apply(traj_embeds.float().contiguous().view(R * V, H), vl, traj_dev, (B, R, V, G, H), status)
        return out.view(B, G, H)
    fwd, bwd = pack_traj_csr(traj_vp_lens, traj_vpids, traj_cand_vpids, gmap_vpids, V, G)
    dev = traj_embeds.device
    fwd, bwd = tuple(x.to(dev) for x in fwd), tuple(x.to(dev) for x in bwd)
    out = _GatherRows.apply(traj_embeds.float().contiguous().view(R * V, H), len(traj_vp_lens) * G, fwd, bwd)
    return out.view(len(traj_vp_lens), G, H)
