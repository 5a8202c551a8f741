"""Native waypoint head: the mirror of vlnce_baselines/waypoint_pred/TRM_net.py (BinaryDistPredictor_TRM) and of the heat-map tail of
vlnce_baselines/models/Policy_ViewSelection_ETP.py:220-318, on the HIP engine of csrc/waypoint_engine.hip and the two kernels of
csrc/waypoint.hip.

    ring_attn(q, k, v, ctx, B, neighbor, alpha)      etp_ring_attn_fwd on torch tensors (operator level)
    waypoint_tail(logits, max_pred, sigma, uniforms) etp_waypoint_tail -> CandidateTable (device)
    BinaryDistPredictorTRM                            nn.Module with the reference's state-dict names; forward -> logits [B,120,12];
                                                      candidates(logits, in_train, generator) -> CandidateTable
    waypoint_mode(net, predictor, observations, in_train)   the body of ETP.forward(mode='waypoint')
    panorama_inputs(rgb_embedding, depth_embedding, cand, in_train, V)   etp_pano_inputs: the candidate table and the two embeddings ->
                                                      the panorama encoder's inputs in one launch (net.fuse_pano_inputs routes
                                                      waypoint_mode through it)

The predictor is frozen and runs in eval() (ss_trainer_ETP.py:201-202): forward only, parameters do not require gradients.
There is no CPU fallback: without the built library, or without a GPU, the compute paths raise.
"""
from __future__ import annotations

import math
from copy import deepcopy
from functools import partial
from typing import NamedTuple, Optional

import numpy as np
import torch

from . import _lib, arena
from ._lib import check, ptr
from .arena import _edt, _stream

NUM_ANGLES, NUM_IMGS, NUM_CLASSES = 120, 12, 12           # Policy_ViewSelection_ETP.py:176-178
MAX_PREDICTIONS, NMS_SIGMA = 5, (7.0, 5.0)                # :233-236
HEATMAP_OFFSET = 5                                        # TRM_net.py:20


_require_gpu = partial(arena._require_gpu, kernels="waypoint")


# ---- operator level -----------------------------------------------------------------------------------------------------------
def ring_attn(q: torch.Tensor, k: torch.Tensor, v: torch.Tensor, ctx: torch.Tensor, B: int, neighbor: int = 1,
              alpha: float = 0.125) -> torch.Tensor:
    """ctx[B*12, :768] = neighbourhood attention of q / k / v (rows [B*12, ld], 2-D tensors or column slices of one packed
    [B*12, 2304] buffer; stride(1) == 1).  Writes into `ctx` (same dtype, bf16 or fp32) and returns it."""
    _require_gpu(q, "ring_attn")
    dt = _edt(q.dtype)
    for t in (q, k, v, ctx):
        assert t.dim() == 2 and t.stride(1) == 1 and t.dtype == q.dtype and t.device == q.device
    check(_lib.lib().etp_ring_attn_fwd(dt, q.data_ptr(), q.stride(0), k.data_ptr(), k.stride(0), v.data_ptr(), v.stride(0),
                                       ctx.data_ptr(), ctx.stride(0), B, neighbor, alpha, _stream()), "etp_ring_attn_fwd")
    return ctx


class CandidateTable(NamedTuple):
    """Device-side result of the tail.  `table` is ONE int32 tensor [7, B, max_pred] whose rows are count (column 0), angle, dist,
    img_cw, img_ccw, samp_angle, samp_dist: a single copy brings everything the host loops need."""
    heat: torch.Tensor
    nms_map: torch.Tensor
    table: torch.Tensor
    sampled: bool

    @property
    def count(self): return self.table[0, :, 0]
    @property
    def angle(self): return self.table[1]
    @property
    def dist(self): return self.table[2]
    @property
    def img_cw(self): return self.table[3]
    @property
    def img_ccw(self): return self.table[4]
    @property
    def samp_angle(self): return self.table[5]
    @property
    def samp_dist(self): return self.table[6]


def waypoint_tail(logits: torch.Tensor, max_pred: int = MAX_PREDICTIONS, sigma=NMS_SIGMA,
                  uniforms: Optional[torch.Tensor] = None) -> CandidateTable:
    """logits [B,120,12] fp32 (rolled) -> heat, nms map and the candidate table (etp_waypoint_tail)."""
    _require_gpu(logits, "waypoint_tail")
    assert logits.dtype == torch.float32 and logits.shape[1:] == (NUM_ANGLES, NUM_CLASSES)
    logits = logits.contiguous()
    B = logits.shape[0]
    heat = torch.empty_like(logits)
    nms_map = torch.empty_like(logits)
    table = torch.full((7, B, max(max_pred, 1)), -1, dtype=torch.int32, device=logits.device)
    if uniforms is not None:
        uniforms = uniforms.to(device=logits.device, dtype=torch.float32).contiguous()
        assert tuple(uniforms.shape) == (B, max_pred)
    cnt = torch.empty(max(B, 1), dtype=torch.int32, device=logits.device)
    check(_lib.lib().etp_waypoint_tail(ptr(logits), B, max_pred, float(sigma[0]), float(sigma[1]), ptr(uniforms), ptr(heat),
                                       ptr(nms_map), ptr(cnt), table[1].data_ptr(), table[2].data_ptr(), table[3].data_ptr(),
                                       table[4].data_ptr(), table[5].data_ptr() if uniforms is not None else None,
                                       table[6].data_ptr() if uniforms is not None else None, _stream()), "etp_waypoint_tail")
    table[0, :, 0] = cnt[:B]
    return CandidateTable(heat, nms_map, table, uniforms is not None)


# ---- the predictor --------------------------------------------------------------------------------------------------------------
def _create(L, dtype):
    h = L.etp_waypoint_create(_lib.ETP_BF16 if dtype == torch.bfloat16 else _lib.ETP_F32)
    if not h:
        raise _lib.EtpError("etp_waypoint_create: " + L.etp_last_error().decode())
    return h


def param_table(dtype: torch.dtype = torch.float32):
    """[(reference state-dict name, shape, arena offset)] of the engine; needs the built library, not a GPU."""
    L = _lib.lib()
    h = _create(L, dtype)
    try:
        return arena.read_table(L, "waypoint", h, _lib.ParamInfo)
    finally:
        L.etp_waypoint_destroy(h)


class BinaryDistPredictorTRM(arena.FrozenArenaModule):
    """TRM_net.py:9-88 on the HIP engine.  Parameters are views of one flat fp32 arena under the reference's names (the unused
    visual_merge / mergefeats_LayerNorm included), so ``load_state_dict(torch.load(cwp_fn)['predictor']['state_dict'])`` is strict."""

    PREFIX, KIND = "waypoint", "predictor"

    def __init__(self, hidden_dim: int = 768, n_classes: int = 12, device=None, dtype: torch.dtype = torch.bfloat16):
        super().__init__()
        assert hidden_dim == 768 and n_classes == 12, "the shipped predictor: hidden 768, 12 distance classes"
        assert dtype in (torch.float32, torch.bfloat16)
        self.num_angles, self.num_imgs, self.n_classes = NUM_ANGLES, NUM_IMGS, NUM_CLASSES
        self.TRM_LAYER, self.TRM_NEIGHBOR, self.HEATMAP_OFFSET = 2, 1, HEATMAP_OFFSET
        self._init_arena(_create(_lib.lib(), dtype), device, dtype)

    def forward(self, rgb_feats, depth_feats) -> torch.Tensor:
        """TRM_net.py:62-88.  depth_feats [12*B,128,4,4] (or [12*B,2048]); rgb_feats is ignored, as in the reference (only its
        batch size was read there).  -> logits [B,120,12] fp32, the angle axis already rolled by HEATMAP_OFFSET."""
        _require_gpu(self.arena, "BinaryDistPredictorTRM")
        x = depth_feats.reshape(depth_feats.shape[0], -1).to(device=self.arena.device, dtype=torch.float32).contiguous()
        assert x.shape[1] == 2048 and x.shape[0] % NUM_IMGS == 0, tuple(x.shape)
        B = x.shape[0] // NUM_IMGS
        ws = self._scratch(B)
        logits = torch.empty(B, NUM_ANGLES, NUM_CLASSES, dtype=torch.float32, device=self.arena.device)
        check(self.L.etp_waypoint_fwd(self.handle, ptr(x), B, ptr(logits), ptr(ws), _stream()), "etp_waypoint_fwd")
        return logits

    def candidates(self, logits: torch.Tensor, in_train: bool, generator: Optional[torch.Generator] = None,
                   uniforms: Optional[torch.Tensor] = None) -> CandidateTable:
        """Policy_ViewSelection_ETP.py:220-282 on the device.  in_train draws one uniform per candidate slot with torch.rand on the
        device (`generator`), or takes `uniforms` [B,5]; torch's Categorical stream is not reproduced."""
        if in_train and uniforms is None:
            uniforms = torch.rand(logits.shape[0], MAX_PREDICTIONS, device=logits.device, generator=generator)
        return waypoint_tail(logits, MAX_PREDICTIONS, NMS_SIGMA, uniforms if in_train else None)


# ---- ETP.forward(mode='waypoint') -----------------------------------------------------------------------------------------------
def angle_feature_torch(headings: torch.Tensor) -> torch.Tensor:
    """vlnce_baselines/models/utils.py:49-57"""
    z = torch.zeros_like(headings)
    return torch.stack([torch.sin(headings), torch.cos(headings), torch.sin(z), torch.cos(z)]).float().T


def pano_constants():
    """Policy_ViewSelection_ETP.py:141-143"""
    idx = np.arange(0, 12, dtype=np.int64)
    return idx, angle_feature_torch(torch.from_numpy((1 - idx / 12) * 2 * math.pi))


def waypoint_mode(net, waypoint_predictor, observations, in_train: bool, generator=None, uniforms=None):
    """Policy_ViewSelection_ETP.py:172-342 with the predictor and the heat-map tail on the device and ONE device-to-host copy (the
    candidate table) in place of the per-episode .nonzero() / .cpu() / .tolist() calls.  `net` supplies depth_encoder,
    rgb_encoder, space_pool_rgb, space_pool_depth, pano_angle_fts and pano_img_idxes."""
    if hasattr(net.rgb_encoder, "encode_views") or hasattr(net.depth_encoder, "encode_views"):
        return _waypoint_mode_views(net, waypoint_predictor, observations, in_train, generator, uniforms)
    batch_size = observations["rgb"].shape[0]
    depth_batch = torch.zeros_like(observations["depth"]).repeat(NUM_IMGS, 1, 1, 1)
    rgb_batch = torch.zeros_like(observations["rgb"]).repeat(NUM_IMGS, 1, 1, 1)
    # reverse the order of the input images to clockwise (:182-190): view a_count of every episode goes to slot (12 - a_count) % 12
    a_count = 0
    for k, v in observations.items():
        if "depth" in k:
            ra_count = (NUM_IMGS - a_count) % NUM_IMGS
            depth_batch[ra_count::NUM_IMGS] = v
            rgb_batch[ra_count::NUM_IMGS] = observations[k.replace("depth", "rgb")]
            a_count += 1
    obs_view12 = {"depth": depth_batch, "rgb": rgb_batch}
    depth_embedding = net.depth_encoder(obs_view12)       # [12B, 128, 4, 4]
    rgb_embedding = net.rgb_encoder(obs_view12)           # [12B, 512]
    return _waypoint_tail_mode(net, waypoint_predictor, rgb_embedding, depth_embedding, batch_size, in_train, generator, uniforms)


def _waypoint_mode_views(net, waypoint_predictor, observations, in_train, generator, uniforms):
    """waypoint_mode with a native view encoder on either side (etpnav_amd.clip.CLIPEncoder, etpnav_amd.depth.DepthEncoder): such an
    encoder takes the 12 view tensors as they are -- its first kernel writes the clockwise order -- so only the other half of the reorder
    (:182-190), if any, is built here.  The two sides are independent of each other."""
    batch_size = observations["rgb"].shape[0]
    if hasattr(net.depth_encoder, "encode_views"):
        depth_embedding = net.depth_encoder.encode_views(observations)  # [12B, 128, 4, 4], clockwise; no depth_batch
    else:
        depth_batch = torch.zeros_like(observations["depth"]).repeat(NUM_IMGS, 1, 1, 1)
        a_count = 0
        for k, v in observations.items():
            if "depth" in k:
                depth_batch[(NUM_IMGS - a_count) % NUM_IMGS::NUM_IMGS] = v
                a_count += 1
        depth_embedding = net.depth_encoder({"depth": depth_batch})     # [12B, 128, 4, 4]
    if hasattr(net.rgb_encoder, "encode_views"):
        rgb_embedding = net.rgb_encoder.encode_views(observations)      # [12B, 512], clockwise
    else:
        rgb_batch = torch.zeros_like(observations["rgb"]).repeat(NUM_IMGS, 1, 1, 1)
        a_count = 0
        for k in observations:
            if "depth" in k:
                rgb_batch[(NUM_IMGS - a_count) % NUM_IMGS::NUM_IMGS] = observations[k.replace("depth", "rgb")]
                a_count += 1
        rgb_embedding = net.rgb_encoder({"rgb": rgb_batch})             # [12B, 512]
    return _waypoint_tail_mode(net, waypoint_predictor, rgb_embedding, depth_embedding, batch_size, in_train, generator, uniforms)


# ---- panorama inputs in one launch (csrc/pano_inputs.hip) -----------------------------------------------------------------------
PINPUTS_ERR_COUNT, PINPUTS_ERR_ANGLE, PINPUTS_ERR_VIEWS = 1, 2, 4     # ETP_PINPUTS_ERR_*
PANO_INPUT_KEYS = ("rgb_fts", "dep_fts", "loc_fts", "nav_types", "view_lens")   # what forward_panorama takes
_POPCOUNT12 = np.array([bin(m).count("1") for m in range(1 << NUM_IMGS)], dtype=np.int64)
_angle_tabs = {}


def cand_angle_table() -> torch.Tensor:
    """[120, 4] fp32 on the host: angle_feature_torch of every heat-map angle, clockwise (Policy_ViewSelection_ETP.py:307, 309); row a
    holds the bits the per-episode call gives for angle index a"""
    return angle_feature_torch(torch.arange(NUM_ANGLES).float() / 120 * 2 * math.pi)


def _host_cand_tables():
    """what the fused route hands the simulator side, per heat-map index and built once with the existing route's expressions:
    cand_angle_fts rows [120,4], counter-clockwise angles (:308) and distances (:310) as Python floats"""
    if "host" not in _angle_tabs:
        a120 = torch.arange(NUM_ANGLES)
        _angle_tabs["host"] = (cand_angle_table(), (2 * math.pi - a120.float() / 120 * 2 * math.pi).tolist(),
                               ((torch.arange(NUM_CLASSES) + 1) * 0.25).tolist())
    return _angle_tabs["host"]


def _device_angle_tabs(device):
    key = str(device)
    if key not in _angle_tabs:
        _angle_tabs[key] = (cand_angle_table().contiguous().to(device), pano_constants()[1].contiguous().to(device))
    return _angle_tabs[key]


def host_img_idxes(angle: np.ndarray) -> np.ndarray:
    """counter-clockwise view of every heat-map angle index (:313-314)"""
    img = 12 - (angle.astype(np.int64) + 5) // 10
    img[img == 12] = 0
    return img


def host_view_lens(host: np.ndarray, in_train: bool) -> np.ndarray:
    """view_len of every episode from the host copy of the candidate table [7, B, max_pred]: K + 12 - the distinct candidate views.
    Vectorised; an episode the kernel would flag (count or angle out of range) gives -1."""
    count = host[0, :, 0].astype(np.int64)
    angle = host[5 if in_train else 1].astype(np.int64)
    B, mp = angle.shape
    live = np.arange(mp)[None, :] < count[:, None]
    ok = (count >= 0) & (count <= mp) & ~(live & ((angle < 0) | (angle >= NUM_ANGLES))).any(1)
    bits = np.where(live & ok[:, None], np.left_shift(1, host_img_idxes(np.clip(angle, 0, NUM_ANGLES - 1))), 0)
    mask = np.bitwise_or.reduce(bits, axis=1) if mp else np.zeros(B, np.int64)
    return np.where(ok, count + NUM_IMGS - _POPCOUNT12[mask], -1)


def panorama_inputs(rgb_embedding: torch.Tensor, depth_embedding: torch.Tensor, cand: CandidateTable, in_train: bool,
                    V: Optional[int] = None, host: Optional[np.ndarray] = None) -> dict:
    """Policy_ViewSelection_ETP.py:289-342 followed by ss_trainer_ETP.py:308-342 (_vp_feature_variable) in one launch of
    etp_pano_inputs: rgb_embedding [12B, Frgb] and depth_embedding [12B, C, H, W] (clockwise, fp32) and the candidate table ->
    {rgb_fts [B,V,Frgb], dep_fts [B,V,C], loc_fts [B,V,4], nav_types [B,V] int64, view_lens [B] int64, status [B] int32,
    cand_img [B,max_pred] int32}, all on the device.  `in_train` picks the sampled angle row of the table, as waypoint_mode does.
    V=None: the reference's padded length, from `host` (the host copy of cand.table; copied here when absent) -- the outputs have the
    reference's shapes.  V=int: a capacity (16 always suffices for max_pred = 5); the launch does not depend on a host copy, padding
    rows are zero and masked by view_lens.  status is left on the device (ETP_PINPUTS_ERR_*): a flagged episode's rows are unwritten."""
    _require_gpu(rgb_embedding, "panorama_inputs")
    rgb = rgb_embedding.to(torch.float32).contiguous()
    dep = depth_embedding.to(device=rgb.device, dtype=torch.float32).contiguous()
    assert rgb.dim() == 2 and rgb.shape[0] % NUM_IMGS == 0 and dep.dim() >= 2 and dep.shape[0] == rgb.shape[0], (tuple(rgb.shape), tuple(dep.shape))
    B, Frgb, C = rgb.shape[0] // NUM_IMGS, rgb.shape[1], dep.shape[1]
    HW = dep[0, 0].numel()
    table = cand.table
    assert table.dtype == torch.int32 and table.is_contiguous() and table.shape[:2] == (7, B) and table.device == rgb.device, tuple(table.shape)
    assert not in_train or cand.sampled, "in_train reads the sampled rows of the table: build it with uniforms"
    mp = table.shape[2]
    if V is None:
        host = table.cpu().numpy() if host is None else host
        V = max(NUM_IMGS, int(host_view_lens(host, in_train).max()))
    dev = rgb.device
    cand_tab, pano_tab = _device_angle_tabs(dev)
    out = {"rgb_fts": torch.empty(B, V, Frgb, dtype=torch.float32, device=dev), "dep_fts": torch.empty(B, V, C, dtype=torch.float32, device=dev),
           "loc_fts": torch.empty(B, V, 4, dtype=torch.float32, device=dev), "nav_types": torch.empty(B, V, dtype=torch.int64, device=dev),
           "view_lens": torch.empty(B, dtype=torch.int64, device=dev), "status": torch.empty(B, dtype=torch.int32, device=dev),
           "cand_img": torch.empty(B, mp, dtype=torch.int32, device=dev)}
    check(_lib.lib().etp_pano_inputs(ptr(rgb), ptr(dep), table[0].data_ptr(), table[5 if in_train else 1].data_ptr(), ptr(cand_tab),
                                     ptr(pano_tab), B, V, mp, Frgb, C, HW, ptr(out["rgb_fts"]), ptr(out["dep_fts"]), ptr(out["loc_fts"]),
                                     ptr(out["nav_types"]), ptr(out["view_lens"]), ptr(out["cand_img"]), ptr(out["status"]), _stream()),
          "etp_pano_inputs")
    return out


def _fused_tail_outputs(net, rgb_embedding, depth_embedding, cand, host, in_train):
    """the output dict of mode='waypoint' with ETP.fuse_pano_inputs: the simulator side's host values from the table copy, and the
    planner's inputs from one launch; cand_rgb / cand_depth / pano_rgb / pano_depth are not built"""
    count = host[0, :, 0]
    angle, dist = host[5 if in_train else 1].astype(np.int64), host[6 if in_train else 2].astype(np.int64)
    lens = host_view_lens(host, in_train)
    if (lens < 0).any():
        raise _lib.EtpError(f"the candidate table of episodes {np.nonzero(lens < 0)[0].tolist()} is malformed (count outside 0 .. "
                            f"{angle.shape[1]} or an angle outside 0 .. 119)")
    V = getattr(net, "pano_inputs_capacity", None)
    if V is not None and int(lens.max()) > V:
        raise ValueError(f"pano_inputs_capacity={V} < the longest view list {int(lens.max())}")
    V = max(NUM_IMGS, int(lens.max())) if V is None else V   # None: the reference's padded length
    # launched first: the device works while the host builds the lists below (the embeddings in the shapes the existing route reads
    # them in, its two reshapes before the pools)
    pano = panorama_inputs(rgb_embedding.reshape(-1, 512), depth_embedding.reshape(-1, 128, 4, 4), cand, in_train, V=V)
    angle_fts, angles_cc, dists = _host_cand_tables()
    img = host_img_idxes(angle)
    ks = count.tolist()
    return {
        "cand_angle_fts": [angle_fts[angle[j, :n]] for j, n in enumerate(ks)],
        "cand_img_idxes": [img[j, :n].copy() for j, n in enumerate(ks)],
        "cand_angles": [[angles_cc[a] for a in angle[j, :n].tolist()] for j, n in enumerate(ks)],
        "cand_distances": [[dists[d] for d in dist[j, :n].tolist()] for j, n in enumerate(ks)],
        "pano_angle_fts": deepcopy(net.pano_angle_fts), "pano_img_idxes": deepcopy(net.pano_img_idxes),
        "pano_inputs": pano,
    }


def _waypoint_tail_mode(net, waypoint_predictor, rgb_embedding, depth_embedding, batch_size, in_train, generator, uniforms):
    logits = waypoint_predictor(rgb_embedding, depth_embedding)
    cand = waypoint_predictor.candidates(logits, in_train, generator=generator, uniforms=uniforms)
    host = cand.table.cpu().numpy()                       # the one device-to-host copy of the call
    if getattr(net, "fuse_pano_inputs", False):
        return _fused_tail_outputs(net, rgb_embedding, depth_embedding, cand, host, in_train)

    # back to counter-clockwise (:201-213) and the two average pools (:289-290)
    rgb_r = rgb_embedding.reshape(batch_size, NUM_IMGS, 512, 1, 1)
    dep_r = depth_embedding.reshape(batch_size, NUM_IMGS, 128, 4, 4)
    rgb_feats = net.space_pool_rgb(torch.cat((rgb_r[:, 0:1, :], torch.flip(rgb_r[:, 1:, :], [1])), dim=1))
    depth_feats = net.space_pool_depth(torch.cat((dep_r[:, 0:1, :], torch.flip(dep_r[:, 1:, :], [1])), dim=1))

    cand_rgb, cand_depth, cand_angle_fts, cand_img_idxes, cand_angles, cand_distances = [], [], [], [], [], []
    for j in range(batch_size):
        n = int(host[0, j, 0])
        angle_idxes = torch.from_numpy(host[5 if in_train else 1, j, :n].astype(np.int64))
        distance_idxes = torch.from_numpy(host[6 if in_train else 2, j, :n].astype(np.int64))
        angle_rad_c = angle_idxes.float() / 120 * 2 * math.pi                   # clockwise (:307)
        angle_rad_cc = 2 * math.pi - angle_idxes.float() / 120 * 2 * math.pi    # counter-clockwise (:308)
        cand_angle_fts.append(angle_feature_torch(angle_rad_c))
        cand_angles.append(angle_rad_cc.tolist())
        cand_distances.append(((distance_idxes + 1) * 0.25).tolist())
        img_idxes = 12 - (angle_idxes.numpy() + 5) // 10                        # counter-clockwise (:313-314)
        img_idxes[img_idxes == 12] = 0
        cand_img_idxes.append(img_idxes)
        cand_rgb.append(rgb_feats[j, img_idxes, ...])
        cand_depth.append(depth_feats[j, img_idxes, ...])
    return {
        "cand_rgb": cand_rgb, "cand_depth": cand_depth, "cand_angle_fts": cand_angle_fts, "cand_img_idxes": cand_img_idxes,
        "cand_angles": cand_angles, "cand_distances": cand_distances,
        "pano_rgb": rgb_feats, "pano_depth": depth_feats,
        "pano_angle_fts": deepcopy(net.pano_angle_fts), "pano_img_idxes": deepcopy(net.pano_img_idxes),
    }
