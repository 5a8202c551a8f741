"""Pre-training batches on the device: annotations + the resident view-feature store -> the SAP / MLM batch dict.

Replaces the reference's ``R2RTextPathData`` / ``SapDataset`` / ``MlmDataset`` / ``sap_collate`` / ``mlm_collate``
(pretrain_src/pretrain_src/data/dataset.py:360-526, tasks.py:12-130, 271-364, common.py:9-128) without h5py, jsonlines or networkx:

  * ``NavGraphs.load(connectivity_dir)``   load_nav_graphs (common.py:71-103): positions, directional all-pairs Dijkstra distances and
    the hop counts of the minimum-distance paths; distances are summed from the source in path order, as networkx's Dijkstra does.
  * ``R2RTextPathIndex``                   R2RTextPathData.get_input (dataset.py:408-481) as a compact record per (item, end index):
    store rows, candidate tables, graph-map ids / step ids / masks / position features, the action label -- no feature row.
  * ``SapBatches`` / ``MlmBatches``        iterables for MetaLoader / PretrainDriver: per batch ONE pinned staging buffer with everything
    the host built, ONE host-to-device copy, then etp_traj_views and etp_traj_pair_dists (csrc/traj_batch.hip).  No synchronisation.
    The batch is a ``TrajBatch``: the dict, plus the trajectory's integer tables on the device (``traj_dev``) from which the steps
    compute the node features (etp_traj_nodes_fwd / _bwd) without building a CSR from the string lists.

Candidate angles are pinned to float32: ``np.float32(base) + np.float32(offset)`` (dataset.py:502-503).  That is what the reference's
expression ``view_angle[0] + v[2]`` (a float32 scalar plus a Python float) gives under numpy 2; under the reference's own numpy 1.x the
same expression promotes to float64 before the sine, so its last bit can differ there.

Deviations from the reference, both on purpose: the random draws come from the numpy ``Generator`` given, not from the global
``random`` / ``np.random`` streams (same distributions); a path of one viewpoint has no negative end, so it is always a 'pos' sample
(the reference raises in np.random.randint(0)).
"""
from __future__ import annotations

import heapq
import json
import math
import os
from typing import Dict, List, Optional, Sequence, Tuple

import numpy as np
import torch

from . import _lib
from ._lib import check, ptr

MAX_DIST = 30            # dataset.py:16-18
MAX_STEP = 10
TRAIN_MAX_STEP = 20
MAX_CANDS = 64           # ETP ABI: Kmax <= 64
VOCAB_RANGE = (1996, 29611)      # tasks.py:60
MASK_TOKEN_ID = 103
TRAJ_ERR_COUNT, TRAJ_ERR_VIEW, TRAJ_ERR_ROW, TRAJ_ERR_VIEWS = 1, 2, 4, 8     # ETP_TRAJ_ERR_* of etp_traj_views
TRAJ_ERR_LEN, TRAJ_ERR_SCAN, TRAJ_ERR_INDEX = 1, 2, 4                        # ... of etp_traj_pair_dists


# ---- common.py:43-68 ---------------------------------------------------------------------------------------------------------------
def angle_fts(headings, elevations) -> np.ndarray:
    """get_angle_fts with angle_feat_size 4: [sin h, cos h, sin e, cos e] in the dtype the angles come in, then float32"""
    fts = np.vstack([np.sin(headings), np.cos(headings), np.sin(elevations), np.cos(elevations)]).transpose().astype(np.float32)
    return np.ascontiguousarray(fts)


def view_rel_angles(base_view: int = 0) -> np.ndarray:
    """get_view_rel_angles: [36, 2] float32 (heading, elevation) of the 12 x 3 panorama grid relative to `base_view`"""
    out = np.zeros((36, 2), dtype=np.float32)
    base_h = (base_view % 12) * math.radians(30)
    base_e = (base_view // 12 - 1) * math.radians(30)
    heading, elevation = 0, math.radians(-30)
    for ix in range(36):
        if ix == 0:
            heading, elevation = 0, math.radians(-30)
        elif ix % 12 == 0:
            heading = 0
            elevation += math.radians(30)
        else:
            heading += math.radians(30)
        out[ix, 0] = heading - base_h
        out[ix, 1] = elevation - base_e
    return out


def mask_tokens(tokens, u, vocab_range=VOCAB_RANGE, mask_id: int = MASK_TOKEN_ID, u2=None):
    """The deterministic part of random_word (tasks.py:12-53): ``u[i]`` is token i's uniform, ``u2[i]`` the uniform that picks its random
    word as ``vocab_range[0] + int(u2[i] * span)`` (random.choice over range(*vocab_range)).  -> (ids, labels) int64, label -1 = not
    masked.  With no token drawn, token 0 is masked ("at least mask 1")."""
    tok = np.asarray(tokens, dtype=np.int64)
    u = np.asarray(u, dtype=np.float64)
    u2 = np.zeros_like(u) if u2 is None else np.asarray(u2, dtype=np.float64)
    if tok.ndim != 1 or u.shape != tok.shape or u2.shape != tok.shape:
        raise ValueError("tokens, u and u2 are 1-D of one length")
    sel = u < 0.15
    p = u / 0.15
    span = int(vocab_range[1]) - int(vocab_range[0])
    word = int(vocab_range[0]) + (u2 * span).astype(np.int64)
    ids = np.where(sel & (p < 0.8), mask_id, np.where(sel & (p < 0.9), word, tok)).astype(np.int64)
    labels = np.where(sel, tok, -1).astype(np.int64)
    if tok.size and not sel.any():
        labels[0], ids[0] = tok[0], mask_id
    return ids, labels


# ---- common.py:71-103 --------------------------------------------------------------------------------------------------------------
class NavGraphs:
    """Per scan: ``vps`` (node order of the reference's graph), ``index`` {vp: local index}, ``pos`` [n, 3] float64, ``dist`` [n, n]
    float64 with dist[a, b] the Dijkstra distance FROM a TO b (the two directions differ in the last bits: each is summed from its own
    source in path order), ``hops`` [n, n] int32 = len(shortest path) - 1, -1 where unreachable."""

    def __init__(self, scans: Dict[str, dict]):
        self.scans = scans
        self.offset, off = {}, 0
        for s, g in scans.items():
            self.offset[s] = off
            off += len(g["vps"]) ** 2
        self.dist_len = off
        self.dist_tab: Optional[torch.Tensor] = None

    @staticmethod
    def _dijkstra(adj: Dict[str, Dict[str, float]], source: str):
        """networkx _dijkstra_multisource: (distance, insertion counter, node) heap, dist[v] + weight summed from the source"""
        dist, seen, paths = {}, {source: 0}, {source: [source]}
        fringe, c = [(0, 0, source)], 1
        while fringe:
            d, _, v = heapq.heappop(fringe)
            if v in dist:
                continue
            dist[v] = d
            for w, cost in adj[v].items():
                vw = dist[v] + cost
                if w in dist:
                    continue
                if w not in seen or vw < seen[w]:
                    seen[w] = vw
                    heapq.heappush(fringe, (vw, c, w))
                    c += 1
                    paths[w] = paths[v] + [w]
        return dist, paths

    @classmethod
    def from_connectivity(cls, data_by_scan: Dict[str, list]) -> "NavGraphs":
        scans = {}
        for scan, data in data_by_scan.items():
            adj: Dict[str, Dict[str, float]] = {}
            positions = {}
            for i, item in enumerate(data):
                if not item["included"]:
                    continue
                for j, conn in enumerate(item["unobstructed"]):
                    if conn and data[j]["included"]:
                        positions[item["image_id"]] = np.array([item["pose"][3], item["pose"][7], item["pose"][11]])
                        if not data[j]["unobstructed"][i]:
                            raise ValueError(f"{scan}: graph should be undirected")
                        a, b = item["pose"], data[j]["pose"]
                        w = ((a[3] - b[3]) ** 2 + (a[7] - b[7]) ** 2 + (a[11] - b[11]) ** 2) ** 0.5
                        u, v = item["image_id"], data[j]["image_id"]
                        adj.setdefault(u, {})
                        adj.setdefault(v, {})
                        adj[u][v] = w
                        adj[v][u] = w
            vps = list(adj)
            index = {v: k for k, v in enumerate(vps)}
            n = len(vps)
            dist = np.full((n, n), np.inf, dtype=np.float64)
            hops = np.full((n, n), -1, dtype=np.int32)
            for a in vps:
                d, paths = cls._dijkstra(adj, a)
                for b, x in d.items():
                    dist[index[a], index[b]] = x
                    hops[index[a], index[b]] = len(paths[b]) - 1
            scans[scan] = {"vps": vps, "index": index, "pos": np.stack([positions[v] for v in vps]) if n else np.zeros((0, 3)),
                           "dist": dist, "hops": hops}
        return cls(scans)

    @classmethod
    def load(cls, connectivity_dir: str) -> "NavGraphs":
        with open(os.path.join(connectivity_dir, "scans.txt")) as f:
            names = [x.strip() for x in f.readlines()]
        data = {}
        for scan in names:
            with open(os.path.join(connectivity_dir, "%s_connectivity.json" % scan)) as f:
                data[scan] = json.load(f)
        return cls.from_connectivity(data)

    def to_device(self, device) -> "NavGraphs":
        flat = np.concatenate([g["dist"].reshape(-1) for g in self.scans.values()]) if self.scans else np.zeros(0)
        self.dist_tab = torch.from_numpy(np.ascontiguousarray(flat, dtype=np.float64)).to(device)
        return self


# ---- dataset.py:408-526 ------------------------------------------------------------------------------------------------------------
def read_json_lines(path: str) -> List[dict]:
    with open(path) as f:
        return [json.loads(line) for line in f if line.strip()]


class R2RTextPathIndex:
    """R2RTextPathData over a FeatureStore: ``record(idx, end_idx)`` is get_input(idx, ..., return_act_label=True) with the end
    viewpoint ``item['path'][end_idx]``, as indices and scalars.  Two ordering rules of the reference hold: get_cur_angle is taken
    BEFORE the TRAIN_MAX_STEP truncation (dataset.py:431-436), and end_idx -- hence the label -- comes from the untruncated path."""

    def __init__(self, anno_files: Sequence, store, scanvp_cands, graphs: NavGraphs, image_feat_size: int = 768,
                 depth_feat_size: int = 128, max_txt_len: int = 100, act_visited_node: bool = False):
        self.data: List[dict] = []
        for a in anno_files:
            self.data.extend(read_json_lines(a) if isinstance(a, (str, os.PathLike)) else list(a))
        if isinstance(scanvp_cands, (str, os.PathLike)):
            with open(scanvp_cands) as f:
                scanvp_cands = json.load(f)
        self.store, self.graphs = store, graphs
        self.image_feat_size, self.depth_feat_size = int(image_feat_size), int(depth_feat_size)
        self.max_txt_len, self.act_visited_node = int(max_txt_len), bool(act_visited_node)
        self.base_angles = view_rel_angles(12)                                   # all_point_rel_angles[12]
        self.view_loc_tab = angle_fts(self.base_angles[:, 0], self.base_angles[:, 1])
        keys = list(store.img.keys)
        self.row_of = {k: i for i, k in enumerate(keys)}
        # candidate tables per "{scan}_{vp}": names, view indices and angle features, in the file's order (dataset.py:495-504)
        self.cands: Dict[str, tuple] = {}
        for key, nav in scanvp_cands.items():
            if len(nav) > MAX_CANDS:
                raise ValueError(f"{key}: {len(nav)} candidates at one viewpoint (at most {MAX_CANDS})")
            names = list(nav.keys())
            view = np.array([nav[k][0] for k in names], dtype=np.int32).reshape(-1)
            if view.size and (view.min() < 0 or view.max() > 35):
                raise ValueError(f"{key}: candidate view index outside 0 .. 35")
            base = self.base_angles[view]
            h = base[:, 0] + np.array([nav[k][2] for k in names], dtype=np.float32).reshape(-1)
            e = base[:, 1] + np.array([nav[k][3] for k in names], dtype=np.float32).reshape(-1)
            loc = angle_fts(h, e) if names else np.zeros((0, 4), dtype=np.float32)
            self.cands[key] = (names, view, loc, {k: int(nav[k][0]) for k in names})
        self._records: Dict[Tuple[int, int], dict] = {}

    def __len__(self):
        return len(self.data)

    def _cand(self, scan: str, vp: str):
        key = "%s_%s" % (scan, vp)
        if key not in self.cands:
            raise ValueError(f"unknown key {key!r} in the candidate file")
        return self.cands[key]

    def cur_angle(self, scan: str, path: List[str], start_heading):
        if len(path) < 2:
            return start_heading, 0
        viewidx = self._cand(scan, path[-2])[3][path[-1]]
        return (viewidx % 12) * math.radians(30), (viewidx // 12 - 1) * math.radians(30)

    def gmap_pos_fts(self, scan: str, cur_vp: str, vpids: List[Optional[str]], cur_heading, cur_elevation) -> np.ndarray:
        """get_gmap_pos_fts / calculate_vp_rel_pos_fts (dataset.py:324-346, common.py:111-128), operation for operation in float64"""
        g = self.graphs.scans[scan]
        ci = g["index"][cur_vp]
        a = g["pos"][ci]
        rel_angles, rel_dists = [], []
        for vp in vpids:
            if vp is None:
                rel_angles.append([0, 0])
                rel_dists.append([0, 0, 0])
                continue
            vi = g["index"][vp]
            b = g["pos"][vi]
            dx, dy, dz = b[0] - a[0], b[1] - a[1], b[2] - a[2]
            xy = max(np.sqrt(dx ** 2 + dy ** 2), 1e-8)
            xyz = max(np.sqrt(dx ** 2 + dy ** 2 + dz ** 2), 1e-8)
            heading = np.arcsin(dx / xy)
            if b[1] < a[1]:
                heading = np.pi - heading
            heading -= cur_heading
            elevation = np.arcsin(dz / xyz)
            elevation -= cur_elevation
            rel_angles.append([heading, elevation])
            rel_dists.append([xyz / MAX_DIST, g["dist"][ci, vi] / MAX_DIST, int(g["hops"][ci, vi]) / MAX_STEP])
        rel_angles = np.array(rel_angles).astype(np.float32)
        rel_dists = np.array(rel_dists).astype(np.float32)
        return np.concatenate([angle_fts(rel_angles[:, 0], rel_angles[:, 1]), rel_dists], 1)

    def record(self, idx: int, end_idx: Optional[int] = None) -> dict:
        item = self.data[idx]
        full = item["path"]
        end_idx = len(full) - 1 if end_idx is None else int(end_idx)
        if not 0 <= end_idx < len(full):
            raise ValueError(f"end index {end_idx} outside the path of item {idx}")
        key = (idx, end_idx)
        if key in self._records:
            return self._records[key]
        scan, end_vp = item["scan"], full[end_idx]
        if scan not in self.graphs.scans:
            raise ValueError(f"unknown key {scan!r} in the connectivity graphs")
        path = full[:end_idx + 1]
        cur_heading, cur_elevation = self.cur_angle(scan, path, item["heading"])      # before the truncation
        if len(path) > TRAIN_MAX_STEP:
            path = path[:TRAIN_MAX_STEP] + [end_vp]
        rows, tables, cand_vpids = [], [], []
        for vp in path:
            skey = "%s_%s" % (scan, vp)
            if skey not in self.row_of:
                raise ValueError(f"unknown key {skey!r} in the feature store")
            names, view, loc, _ = self._cand(scan, vp)
            rows.append(self.row_of[skey])
            tables.append((view, loc))
            cand_vpids.append(list(names))
        # get_gmap_inputs (dataset.py:288-322)
        visited, unvisited = {}, {}
        for t, vp in enumerate(path):
            visited[vp] = t + 1
            unvisited.pop(vp, None)
            for nxt in self._cand(scan, vp)[0]:
                if nxt not in visited:
                    unvisited[nxt] = 0
        gmap_vpids = [None] + list(visited) + list(unvisited)
        step_ids = [0] + list(visited.values()) + list(unvisited.values())
        if self.act_visited_node:
            vmask = [0] + [1 if vp == path[-1] else 0 for vp in gmap_vpids[1:]]
        else:
            vmask = [0] + [1] * len(visited) + [0] * len(unvisited)
        g = self.graphs.scans[scan]
        for vp in gmap_vpids[1:]:
            if vp not in g["index"]:
                raise ValueError(f"unknown key {vp!r} in the connectivity graph of {scan}")
        # get_act_labels (dataset.py:390-406): end_idx of the untruncated path
        if end_vp == full[-1]:
            glabel = llabel = 0
        else:
            glabel = llabel = -100
            nxt = full[end_idx + 1]
            if nxt in gmap_vpids:
                glabel = gmap_vpids.index(nxt)
            if nxt in cand_vpids[-1]:
                llabel = cand_vpids[-1].index(nxt) + 1
        # the trajectory as graph indices (the index space of gmap_idx): what etp_traj_nodes_fwd / _bwd read instead of the names
        kmax = max(1, max(len(c) for c in cand_vpids))
        cand_vp = np.full((len(path), kmax), -1, dtype=np.int32)
        for t, c in enumerate(cand_vpids):
            cand_vp[t, :len(c)] = [g["index"][vp] for vp in c]
        rec = {
            "step_vp": np.asarray([g["index"][vp] for vp in path], dtype=np.int32), "cand_vp": cand_vp,
            "instr_id": item["instr_id"], "scan": scan,
            "txt": np.asarray(item["instr_encoding"][:self.max_txt_len], dtype=np.int64),
            "rows": np.asarray(rows, dtype=np.int32), "tables": tables,
            "view_lens": [len(v) + 36 - len(set(v.tolist())) for v, _ in tables],
            "traj_vpids": list(path), "traj_cand_vpids": cand_vpids, "gmap_vpids": gmap_vpids,
            "gmap_idx": np.asarray([-1] + [g["index"][vp] for vp in gmap_vpids[1:]], dtype=np.int32),
            "gmap_step_ids": np.asarray(step_ids, dtype=np.int64), "gmap_visited_masks": np.asarray(vmask, dtype=np.bool_),
            "gmap_pos_fts": self.gmap_pos_fts(scan, path[-1], gmap_vpids, cur_heading, cur_elevation),
            "global_act_label": glabel, "local_act_label": llabel,
        }
        self._records[key] = rec
        return rec


# ---- tasks.py:55-138, 271-364 ------------------------------------------------------------------------------------------------------
def _align(n: int, a: int = 16) -> int:
    return (n + a - 1) // a * a


class TrajBatch(dict):
    """The batch dict of the native loaders -- keys and values as before -- with the trajectory's integer tables on the device beside it:
    ``traj_dev`` = {step_off [B+1], step_vp [R], cand_count [R], cand_vp [R, Kmax], gmap_id [B, G], gmap_len [B]} int32 views of the
    batch's one staging buffer, plus ``Kmax``.  PlannerStep / MlmStep compute the node features from them (etp_traj_nodes_fwd / _bwd)
    and build no CSR from ``traj``'s string lists.  An MLM batch also carries ``mlm_dev`` = {txt_labels: int32 [B, L] on the device (-1 =
    not masked), n_masked: the host-known count}, a view of the same buffer: MlmStep builds its row gather from it (etp_mlm_select)."""
    traj_dev: Optional[dict] = None
    mlm_dev: Optional[dict] = None


class _Batches:
    task = ""

    def __init__(self, index: R2RTextPathIndex, batch_size: int, generator: np.random.Generator, device, shuffle: bool = True):
        if batch_size < 1:
            raise ValueError("batch_size must be >= 1")
        self.index, self.batch_size, self.gen, self.shuffle = index, int(batch_size), generator, shuffle
        self.device = torch.device(device)
        dev = getattr(index.store, "_dev", None)
        if self.device.type != "cuda":
            raise ValueError(f"the native loaders assemble on the GPU; device {device!r} is none (no CPU fallback exists)")
        if dev is None or dev[0].device.type != "cuda":
            raise ValueError("the feature store is not on the device: call FeatureStore.to_device(device) first")
        if index.graphs.dist_tab is None or index.graphs.dist_tab.device.type != "cuda":
            raise ValueError("the distance table is not on the device: call NavGraphs.to_device(device) first")
        self.img, self.dep, _ = dev
        if self.img.shape[1] != 36 or index.image_feat_size > self.img.shape[2] or index.image_feat_size % 4 or self.img.shape[2] % 4:
            raise ValueError("the image store must be [N, 36, ld] with image_feat_size <= ld, both multiples of 4")
        if self.dep is not None and (index.depth_feat_size > self.dep.shape[2] or index.depth_feat_size % 4 or self.dep.shape[2] % 4):
            raise ValueError("the depth store must be [N, 36, ld] with depth_feat_size <= ld, both multiples of 4")
        self.view_loc_tab = torch.from_numpy(index.view_loc_tab).to(self.device).contiguous()
        self.status: Optional[torch.Tensor] = None
        self._status_split = 0

    def __len__(self):
        return (len(self.index) + self.batch_size - 1) // self.batch_size

    def check(self) -> None:
        """read the status words of the last batch in one copy; raises EtpError naming the flagged steps / samples"""
        if self.status is None:
            return
        st = self.status.cpu().numpy()
        R = self._status_split
        if st.any():
            raise _lib.EtpError(f"{self.task} batch flagged: etp_traj_views steps {np.nonzero(st[:R])[0].tolist()} "
                                f"(status {st[:R][st[:R] != 0].tolist()}), etp_traj_pair_dists samples {np.nonzero(st[R:])[0].tolist()} "
                                f"(status {st[R:][st[R:] != 0].tolist()})")

    def assemble(self, recs: List[dict], txt: List[np.ndarray], labels: np.ndarray, txt_labels: Optional[List[np.ndarray]] = None) -> dict:
        """records -> the batch dict of synthetic.make_sap_batch on the device (a TrajBatch): one staging buffer, one copy, two launches"""
        idx = self.index
        B = len(recs)
        R = sum(len(r["rows"]) for r in recs)
        Kmax = max(1, max(len(v) for r in recs for v, _ in r["tables"]))
        V = max(n for r in recs for n in r["view_lens"])
        G = max(len(r["gmap_vpids"]) for r in recs)
        L = max(len(t) for t in txt)
        segs = [("pano_row", np.int32, (R,)), ("cand_count", np.int32, (R,)), ("cand_view", np.int32, (R, Kmax)),
                ("cand_loc", np.float32, (R, Kmax, 4)), ("scan_off", np.int64, (B,)), ("scan_n", np.int32, (B,)),
                ("gmap_idx", np.int32, (B, G)), ("gmap_len", np.int32, (B,)), ("step_off", np.int32, (B + 1,)), ("step_vp", np.int32, (R,)),
                ("cand_vp", np.int32, (R, Kmax)), ("txt_ids", np.int64, (B, L)),
                ("txt_masks", np.bool_, (B, L)), ("gmap_step_ids", np.int64, (B, G)), ("gmap_pos_fts", np.float32, (B, G, 7)),
                ("gmap_visited_masks", np.bool_, (B, G)), ("labels", np.int64, (B,))]
        if txt_labels is not None:                                               # what etp_mlm_select reads: rides in the same copy
            segs.append(("mlm_labels", np.int32, (B, L)))
        offs, total = {}, 0
        for name, dt, shape in segs:
            offs[name] = total
            total += _align(int(np.prod(shape)) * np.dtype(dt).itemsize)
        stage = torch.zeros(total, dtype=torch.uint8, pin_memory=self.device.type == "cuda")    # pad_sequence / pad_tensors: zero padding
        host = stage.numpy()
        h = {name: host[offs[name]:offs[name] + int(np.prod(shape)) * np.dtype(dt).itemsize].view(dt).reshape(shape)
             for name, dt, shape in segs}
        r0 = 0
        h["cand_vp"][:] = -1
        for b, rec in enumerate(recs):
            n = len(rec["rows"])
            h["pano_row"][r0:r0 + n] = rec["rows"]
            h["step_off"][b + 1] = r0 + n
            h["step_vp"][r0:r0 + n] = rec["step_vp"]
            h["cand_vp"][r0:r0 + n, :rec["cand_vp"].shape[1]] = rec["cand_vp"]
            for t, (view, loc) in enumerate(rec["tables"]):
                k = len(view)
                h["cand_count"][r0 + t] = k
                h["cand_view"][r0 + t, :k] = view
                h["cand_loc"][r0 + t, :k] = loc
            r0 += n
            g = len(rec["gmap_vpids"])
            h["scan_off"][b] = idx.graphs.offset[rec["scan"]]
            h["scan_n"][b] = len(idx.graphs.scans[rec["scan"]]["vps"])
            h["gmap_idx"][b, :g] = rec["gmap_idx"]
            h["gmap_len"][b] = g
            h["txt_ids"][b, :len(txt[b])] = txt[b]
            h["txt_masks"][b, :len(txt[b])] = True
            h["gmap_step_ids"][b, :g] = rec["gmap_step_ids"]
            h["gmap_pos_fts"][b, :g] = rec["gmap_pos_fts"]
            h["gmap_visited_masks"][b, :g] = rec["gmap_visited_masks"]
        h["labels"][:] = labels
        if txt_labels is not None:
            h["mlm_labels"][:] = -1
            for b, t in enumerate(txt_labels):
                h["mlm_labels"][b, :len(t)] = t
        dev = stage.to(self.device, non_blocking=True)                           # the ONE host-to-device copy
        torch_dt = {np.int32: torch.int32, np.int64: torch.int64, np.float32: torch.float32, np.bool_: torch.bool}
        d = {name: dev[offs[name]:offs[name] + int(np.prod(shape)) * np.dtype(dt).itemsize].view(torch_dt[dt]).view(shape)
             for name, dt, shape in segs}
        Fi, Fd = idx.image_feat_size, idx.depth_feat_size
        new = lambda shape, dt: torch.empty(shape, dtype=dt, device=self.device)
        out = {"rgb_fts": new((R, V, Fi), torch.float32), "dep_fts": new((R, V, Fd), torch.float32) if self.dep is not None else None,
               "loc_fts": new((R, V, 4), torch.float32), "nav_types": new((R, V), torch.int64), "view_lens": new((R,), torch.int64)}
        pair, gmask = new((B, G, G), torch.float32), new((B, G), torch.uint8)
        self.status, self._status_split = new((R + B,), torch.int32), R
        s = torch.cuda.current_stream(self.device).cuda_stream
        L_ = _lib.lib()
        check(L_.etp_traj_views(ptr(self.img), ptr(self.dep), ptr(d["pano_row"]), ptr(d["cand_count"]), ptr(d["cand_view"]),
                                ptr(d["cand_loc"]), ptr(self.view_loc_tab), R, V, Kmax, 36, Fi, self.img.shape[2], Fd,
                                self.dep.shape[2] if self.dep is not None else 0, self.img.shape[0], ptr(out["rgb_fts"]),
                                ptr(out["dep_fts"]), ptr(out["loc_fts"]), ptr(out["nav_types"]), ptr(out["view_lens"]),
                                self.status.data_ptr(), s), "etp_traj_views")
        check(L_.etp_traj_pair_dists(ptr(idx.graphs.dist_tab), idx.graphs.dist_len, ptr(d["scan_off"]), ptr(d["scan_n"]),
                                     ptr(d["gmap_idx"]), ptr(d["gmap_len"]), B, G, ptr(pair), ptr(gmask),
                                     self.status.data_ptr() + 4 * R, s), "etp_traj_pair_dists")
        if out["dep_fts"] is None:
            del out["dep_fts"]
        out.update({k: d[k] for k in ("txt_ids", "txt_masks", "gmap_step_ids", "gmap_pos_fts", "gmap_visited_masks", "labels")})
        out.update({"gmap_masks": gmask.view(torch.bool), "gmap_pair_dists": pair,
                    "traj": {"traj_step_lens": [len(r["rows"]) for r in recs], "traj_vp_lens": [list(r["view_lens"]) for r in recs],
                             "traj_vpids": [r["traj_vpids"] for r in recs], "traj_cand_vpids": [r["traj_cand_vpids"] for r in recs],
                             "gmap_vpids": [r["gmap_vpids"] for r in recs]}})
        if txt_labels is not None:                                               # host: the fallback route of MlmStep (select="host")
            tl = torch.full((B, L), -1, dtype=torch.int64)
            for b, t in enumerate(txt_labels):
                tl[b, :len(t)] = torch.from_numpy(t)
            out["txt_labels"] = tl
        out = TrajBatch(out)
        if txt_labels is not None:                                               # mask_tokens ran on the host: the count is known here
            out.mlm_dev = {"txt_labels": d["mlm_labels"], "n_masked": int((h["mlm_labels"] != -1).sum())}
        out.traj_dev = {"step_off": d["step_off"], "step_vp": d["step_vp"], "cand_count": d["cand_count"], "cand_vp": d["cand_vp"],
                        "gmap_id": d["gmap_idx"], "gmap_len": d["gmap_len"], "Kmax": Kmax}
        return out

    def _order(self):
        n = len(self.index)
        order = self.gen.permutation(n) if self.shuffle else np.arange(n)
        for i in range(0, n, self.batch_size):
            yield [int(x) for x in order[i:i + self.batch_size]]


class SapBatches(_Batches):
    """SapDataset + sap_collate (tasks.py:271-364).  Per sample one uniform picks the end type ('pos' below end_vp_pos_ratio; the two
    negative types are the same draw for R2R, dataset.py:422-426), a negative end index is ``generator.integers(len(path) - 1)``."""
    task = "sap"

    def __init__(self, index, batch_size, generator, device, end_vp_pos_ratio: float = 0.2, shuffle: bool = True):
        super().__init__(index, batch_size, generator, device, shuffle)
        self.end_vp_pos_ratio = float(end_vp_pos_ratio)

    def batch(self, samples: Sequence[Tuple[int, Optional[int]]]) -> dict:
        """samples: (item index, end index or None = the last viewpoint)"""
        recs = [self.index.record(i, e) for i, e in samples]
        return self.assemble(recs, [r["txt"] for r in recs], np.asarray([r["global_act_label"] for r in recs], dtype=np.int64))

    def __iter__(self):
        for ids in self._order():
            samples = []
            for i in ids:
                n = len(self.index.data[i]["path"])
                r = self.gen.random()
                samples.append((i, None) if r < self.end_vp_pos_ratio or n < 2 else (i, int(self.gen.integers(n - 1))))
            yield self.batch(samples)


class MlmBatches(_Batches):
    """MlmDataset + mlm_collate (tasks.py:55-138): always the 'pos' end; per token two uniforms of the generator drive mask_tokens.
    ``labels`` (the SAP label of the same record) rides along so that the dict has one layout for both tasks."""
    task = "mlm"

    def __init__(self, index, batch_size, generator, device, vocab_range=VOCAB_RANGE, mask_id: int = MASK_TOKEN_ID, shuffle: bool = True):
        super().__init__(index, batch_size, generator, device, shuffle)
        self.vocab_range, self.mask_id = tuple(vocab_range), int(mask_id)

    def batch(self, items: Sequence[int], uniforms: Optional[Sequence] = None) -> dict:
        """uniforms: per item (u, u2) for mask_tokens; None = drawn from the generator"""
        recs = [self.index.record(i, None) for i in items]
        ids, labels = [], []
        for b, r in enumerate(recs):
            n = len(r["txt"])
            u, u2 = uniforms[b] if uniforms is not None else (self.gen.random(n), self.gen.random(n))
            a, l = mask_tokens(r["txt"], u, self.vocab_range, self.mask_id, u2)
            ids.append(a)
            labels.append(l)
        return self.assemble(recs, ids, np.asarray([r["global_act_label"] for r in recs], dtype=np.int64), labels)

    def __iter__(self):
        for ids in self._order():
            yield self.batch(ids)
