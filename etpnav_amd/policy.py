"""Habitat-free mirror of the planner-facing part of vlnce_baselines/models/Policy_ViewSelection_ETP.py.

``ETP.forward(mode=...)`` keeps the reference's keyword names and dispatch (Policy_ViewSelection_ETP.py:157-170,
:344-358) for the three planner modes.  ``mode='waypoint'`` (:172-342) runs the native waypoint head (etpnav_amd/waypoint.py)
once the two perception encoders are attached as ``net.depth_encoder`` / ``net.rgb_encoder``: the native ones
(etpnav_amd.depth.DepthEncoder, the DD-PPO ResNet-50; etpnav_amd.clip.CLIPEncoder, the ViT-B/32), with which a rollout step
needs neither habitat_baselines nor torch's convolution library, or the reference's own modules; without them it raises
NotImplementedError (habitat's simulator itself stays out of scope).
``PolicyViewSelectionETP`` mirrors ILPolicy (models/policy.py:12-19): it just holds ``.net``.
"""
from __future__ import annotations

import torch
import torch.nn as nn

from .vlnbert_init import get_vlnbert_models
from .waypoint import pano_constants, waypoint_mode


class ETP(nn.Module):
    def __init__(self, model_config=None, dtype: torch.dtype = torch.bfloat16, device=None, fuse_drop_env: bool = True):
        super().__init__()
        self.vln_bert = get_vlnbert_models(config=model_config, dtype=dtype, device=device)
        self.drop_env = nn.Dropout(p=0.4)          # Policy_ViewSelection_ETP.py:102
        # fused: the p=0.4 feature dropout rides in forward_panorama's operand cast (and its mask is recomputed for the
        # img_linear weight gradient and d rgb_fts) instead of a separate elementwise pass over [B,V,F] + a saved mask
        self.fuse_drop_env = fuse_drop_env
        # mode='waypoint': VlnResnetDepthEncoder / CLIPEncoder (:118-138), supplied by the user: the native etpnav_amd.depth.DepthEncoder
        # and etpnav_amd.clip.CLIPEncoder, or the reference's modules; None = not attached
        self.depth_encoder = None
        self.rgb_encoder = None
        self.space_pool_depth = nn.Sequential(nn.AdaptiveAvgPool2d((1, 1)), nn.Flatten(start_dim=2))   # :125
        self.space_pool_rgb = nn.Sequential(nn.AdaptiveAvgPool2d((1, 1)), nn.Flatten(start_dim=2))     # :139
        self.pano_img_idxes, self.pano_angle_fts = pano_constants()                                    # :141-143
        # mode='waypoint' with fuse_pano_inputs: the planner's panorama inputs (rgb_fts .. view_lens) come out of one launch
        # (waypoint.panorama_inputs) under 'pano_inputs', and cand_rgb / cand_depth / pano_rgb / pano_depth are not built;
        # graph_inputs.vp_feature_variable hands them on.  pano_inputs_capacity: None = the reference's padded length, or a fixed
        # number of view rows (16 suffices for five candidates).  Off: the reference's ten keys, as before.
        self.fuse_pano_inputs = False
        self.pano_inputs_capacity = None

    def forward(self, mode=None, txt_ids=None, txt_masks=None, txt_embeds=None, waypoint_predictor=None,
                observations=None, in_train=True, rgb_fts=None, dep_fts=None, loc_fts=None, nav_types=None,
                view_lens=None, gmap_vp_ids=None, gmap_step_ids=None, gmap_img_fts=None, gmap_pos_fts=None,
                gmap_masks=None, gmap_visited_masks=None, gmap_pair_dists=None):
        if mode == "language":
            return self.vln_bert.forward_txt(txt_ids, txt_masks)
        if mode == "panorama":
            if self.fuse_drop_env:
                self.vln_bert.drop_env_prob = self.drop_env.p if self.training else 0.0
            else:
                self.vln_bert.drop_env_prob = 0.0
                rgb_fts = self.drop_env(rgb_fts)   # :345 (identity in eval())
            return self.vln_bert.forward_panorama(rgb_fts, dep_fts, loc_fts, nav_types, view_lens)
        if mode == "navigation":
            return self.vln_bert.forward_navigation(txt_embeds, txt_masks, gmap_vp_ids, gmap_step_ids, gmap_img_fts,
                                                    gmap_pos_fts, gmap_masks, gmap_visited_masks, gmap_pair_dists)
        if mode == "waypoint":
            if self.depth_encoder is None or self.rgb_encoder is None:
                raise NotImplementedError("mode='waypoint' needs the CLIP + DD-PPO encoders: attach them as "
                                          "net.depth_encoder / net.rgb_encoder (etpnav_amd.depth.DepthEncoder, "
                                          "etpnav_amd.clip.CLIPEncoder or the reference's modules; INTEGRATION.md)")
            return waypoint_mode(self, waypoint_predictor, observations, in_train)
        raise NotImplementedError(mode)


class PolicyViewSelectionETP(nn.Module):
    """Holds ``.net`` like ILPolicy; ``from_config`` keeps the reference signature (observation/action spaces unused)."""

    def __init__(self, observation_space=None, action_space=None, model_config=None, dtype=torch.bfloat16, device=None):
        super().__init__()
        self.net = ETP(model_config=model_config, dtype=dtype, device=device)

    @classmethod
    def from_config(cls, config, observation_space=None, action_space=None, **kw):
        model_config = getattr(config, "MODEL", config)
        return cls(observation_space=observation_space, action_space=action_space, model_config=model_config, **kw)
