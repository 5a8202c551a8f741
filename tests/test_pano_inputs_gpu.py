"""etp_pano_inputs (csrc/pano_inputs.hip) on the MI355X against tests/pano_inputs_ref.py, and the fused route of
ETP.forward(mode='waypoint') against the existing one.

Operator: pano_inputs_ref.cases() (B in {1, 3, 8, 33} x (Frgb, C, HW) in {(512, 128, 16), (16, 8, 16), (260, 6, 1)}), each at V = the
reference length, 16 and 20 and in both table modes.  Outputs start as payload NaNs (0xFF bytes for the integers) inside guarded buffers
whose guards must come back intact; pano_inputs_ref.check holds rgb_fts, loc_fts, nav_types, view_lens, cand_img and status bit for bit
and every element of dep_fts to |got - ref| <= gam(HW) mean|x| + u |ref| (float64 reference, no multiplier; padding rows exact zeros, the
constant channel exact); inputs unchanged; a second run bit-identical.  Malformed episodes (count 6, count -1, angle 120, V too small for
one episode) are flagged, their rows keep the fill and the other episodes are correct.  Refusals leave the fill intact.

End to end: small native encoders (etpnav_amd.clip.CLIPEncoder at 64 x 64 with 2 layers, etpnav_amd.depth.DepthEncoder at 64 x 64) and
the predictor; ETP.forward(mode='waypoint') with fuse_pano_inputs, then graph_inputs.vp_feature_variable, against the flag-off route on
the same observations and uniforms: the four exact outputs bit-equal, dep_fts of both routes within the bound of the float64 mean.  The
recordings of tests/golden/waypoint_small.npz are replayed the same way, and forward_panorama takes the result.

ETP_PANO_INPUTS_BOUNDS_OUT=<path> writes the worst ratios there (profiles/pano_inputs_op_bounds.txt is such a file).
"""
import os
from types import SimpleNamespace

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from etpnav_amd import _lib, graph_inputs  # noqa: E402
from etpnav_amd import waypoint as wp  # noqa: E402
from tests import move_ref as mr  # noqa: E402
from tests import pano_inputs_ref as pir  # noqa: E402

DEV = "cuda"
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "waypoint_small.npz")
NAN_BITS = 0x7FC12345
SEEN = {}


@pytest.fixture(scope="module", autouse=True)
def report_worst():
    yield
    lines = ["# tests/test_pano_inputs_gpu.py: worst |got - fp64| / bound of dep_fts per case (bound: tests/pano_inputs_ref.py, no multiplier);",
             "# every other output is compared bit for bit"]
    lines += [f"{k:44s} {v:.4f}" for k, v in sorted(SEEN.items())]
    print("\n" + "\n".join(lines))
    out = os.environ.get("ETP_PANO_INPUTS_BOUNDS_OUT")
    if out:
        with open(out, "w") as f:
            f.write("\n".join(lines) + "\n")


def checked(name, got, ref, cc=None):
    SEEN[name] = max(SEEN.get(name, 0.0), pir.check(name, got, ref, cc))


class Outputs:
    """the seven outputs as payload NaNs / 0xFF bytes inside guarded buffers"""

    def __init__(self, B, V, mp, F, C):
        self.f = {"rgb_fts": mr.guarded((B, V, F)), "dep_fts": mr.guarded((B, V, C)), "loc_fts": mr.guarded((B, V, 4))}
        self.g_nav, self.nav = mr.guarded_i64((B, V))
        self.g_len, self.lens = mr.guarded_i64((B,))
        self.g_img, self.g_st = mr.guarded((B * mp * 4,), torch.uint8), mr.guarded((B * 4,), torch.uint8)
        self.img, self.st = self.g_img.t.view(torch.int32).view(B, mp), self.g_st.t.view(torch.int32)

    def guards(self):
        return list(self.f.values()) + [self.g_nav, self.g_len, self.g_img, self.g_st]

    def ptrs(self):
        return [self.f["rgb_fts"].t.data_ptr(), self.f["dep_fts"].t.data_ptr(), self.f["loc_fts"].t.data_ptr(), self.nav.data_ptr(),
                self.lens.data_ptr(), self.img.data_ptr(), self.st.data_ptr()]

    def numpy(self):
        out = {k: g.t.cpu().numpy() for k, g in self.f.items()}
        out.update(nav_types=self.nav.cpu().numpy(), view_lens=self.lens.cpu().numpy(), cand_img=self.img.cpu().numpy(), status=self.st.cpu().numpy())
        return out


def launch(rgb, dep, table, in_train, V, out, override=None):
    """rgb / dep / table on the device -> rc of etp_pano_inputs"""
    cand_tab, pano_tab = wp._device_angle_tabs(rgb.device)
    B, mp = table.shape[1], table.shape[2]
    a = dict(B=B, V=V, max_pred=mp, Frgb=rgb.shape[1], C=dep.shape[1], HW=dep.shape[2])
    a.update(override or {})
    rc = _lib.lib().etp_pano_inputs(rgb.data_ptr(), dep.data_ptr(), table[0].data_ptr(), table[5 if in_train else 1].data_ptr(),
                                    cand_tab.data_ptr(), pano_tab.data_ptr(), a["B"], a["V"], a["max_pred"], a["Frgb"], a["C"], a["HW"],
                                    *out.ptrs(), torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    return rc


def on_device(rgb, dep, table):
    return torch.from_numpy(rgb).to(DEV), torch.from_numpy(dep).to(DEV), torch.from_numpy(table).to(DEV)


@pytest.mark.parametrize("B,dims,shift", pir.cases(), ids=[f"B{B}-F{d[0]}-C{d[1]}-HW{d[2]}" for B, d, _ in pir.cases()])
def test_operator_against_the_restatement(B, dims, shift):
    table = pir.crafted_table(B, shift)
    rgb, dep, cc = pir.make_inputs(B, dims)
    d_rgb, d_dep, d_tab = on_device(rgb, dep, table)
    keep = [t.clone() for t in (d_rgb, d_dep, d_tab)]
    for in_train in (False, True):
        for vm in pir.V_MODES:
            V = pir.ref_length(table, in_train) if vm == "ref" else vm
            name = f"B{B} F{dims[0]} C{dims[1]} HW{dims[2]} V{vm} {'train' if in_train else 'eval'}"
            ref = pir.pano_inputs(rgb, dep, table, in_train, V)
            assert ref["written"].all()
            out = Outputs(B, V, table.shape[2], dims[0], dims[1])
            assert launch(d_rgb, d_dep, d_tab, in_train, V, out) == 0, _lib.lib().etp_last_error()
            for g in out.guards():
                g.check(name)
            got = out.numpy()
            checked(name, got, ref, cc)
            for t, k in zip((d_rgb, d_dep, d_tab), keep):
                mr.exact(name + " inputs unchanged", t.cpu(), k.cpu())
            again = Outputs(B, V, table.shape[2], dims[0], dims[1])
            assert launch(d_rgb, d_dep, d_tab, in_train, V, again) == 0
            for k, v in again.numpy().items():
                assert v.tobytes() == got[k].tobytes(), f"{name}: second run differs in {k}"


def test_high_level_call_gives_the_operators_bits_at_both_forms_of_V():
    B, dims = 8, (512, 128, 16)
    table = pir.crafted_table(B, 0)
    rgb, dep, cc = pir.make_inputs(B, dims)
    d_rgb, d_dep, d_tab = on_device(rgb, dep, table)
    cand = wp.CandidateTable(None, None, d_tab, True)
    for in_train in (False, True):
        for V in (None, 16):
            out = wp.panorama_inputs(d_rgb, d_dep.reshape(12 * B, 128, 4, 4), cand, in_train, V=V)
            assert list(out) == ["rgb_fts", "dep_fts", "loc_fts", "nav_types", "view_lens", "status", "cand_img"]
            Vr = pir.ref_length(table, in_train) if V is None else V
            assert out["rgb_fts"].shape[1] == Vr
            checked(f"panorama_inputs V={V} train={in_train}", {k: v.cpu().numpy() for k, v in out.items()},
                    pir.pano_inputs(rgb, dep, table, in_train, Vr), cc)


def test_malformed_episodes_are_flagged_keep_the_fill_and_leave_the_others_correct():
    B, dims, V = 8, (16, 8, 16), 15
    table = pir.crafted_table(B, 0)
    table[0, 1, 0], table[0, 2, 0], table[1, 4, 2] = 6, -1, 120           # count 6, count -1, angle 120; episode 3 needs 16 > V rows
    rgb, dep, cc = pir.make_inputs(B, dims)
    ref = pir.pano_inputs(rgb, dep, table, False, V)
    assert ref["status"].tolist() == [0, pir.ERR_COUNT, pir.ERR_COUNT, pir.ERR_VIEWS, pir.ERR_ANGLE, 0, 0, 0]
    out = Outputs(B, V, 5, dims[0], dims[1])
    assert launch(*on_device(rgb, dep, table), False, V, out) == 0
    for g in out.guards():
        g.check("malformed")
    got = out.numpy()
    checked("malformed episodes", got, ref, cc)
    bad = ~ref["written"]
    assert bad.sum() == 4
    for k in ("rgb_fts", "dep_fts", "loc_fts"):
        assert (got[k][bad].view(np.int32) == NAN_BITS).all(), f"a flagged episode wrote {k}"
    for k in ("nav_types", "view_lens", "cand_img"):
        assert (got[k][bad] == -1).all(), f"a flagged episode wrote {k}"


REFUSED = {"Frgb 510": dict(Frgb=510), "HW 0": dict(HW=0), "V 11": dict(V=11), "max_pred 0": dict(max_pred=0), "B 0": dict(B=0)}


@pytest.mark.parametrize("name", list(REFUSED))
def test_refusals_leave_the_fill_intact(name):
    B, dims, V = 3, (512, 128, 16), 16
    rgb, dep, _ = pir.make_inputs(B, dims)
    out = Outputs(B, V, 5, dims[0], dims[1])
    assert launch(*on_device(rgb, dep, pir.crafted_table(B, 0)), False, V, out, REFUSED[name]) == -1
    for g in out.guards():
        g.intact(name)


# ---- end to end --------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def net():
    from etpnav_amd.policy import ETP
    return ETP(model_config=SimpleNamespace(task_type="r2r"), dtype=torch.float32, device=DEV).eval()


def both_routes(net, pred, obs, in_train, uniforms):
    """-> (flag-off output, its vp_feature_variable, flag-on output, its vp_feature_variable)"""
    net.fuse_pano_inputs = False
    old = wp.waypoint_mode(net, pred, obs, in_train, uniforms=uniforms)
    vp_old = graph_inputs.vp_feature_variable(old, DEV)
    net.fuse_pano_inputs = True
    try:
        new = net(mode="waypoint", waypoint_predictor=pred, observations=obs, in_train=False) if not in_train else \
            wp.waypoint_mode(net, pred, obs, True, uniforms=uniforms)
        vp_new = graph_inputs.vp_feature_variable(new, DEV)
    finally:
        net.fuse_pano_inputs = False
    return old, vp_old, new, vp_new


def compare_routes(name, old, vp_old, new, vp_new, ref):
    assert list(new) == ["cand_angle_fts", "cand_img_idxes", "cand_angles", "cand_distances", "pano_angle_fts", "pano_img_idxes", "pano_inputs"]
    assert list(vp_new) == list(vp_old) == ["rgb_fts", "dep_fts", "loc_fts", "nav_types", "view_lens"]
    for k in ("rgb_fts", "loc_fts", "nav_types", "view_lens"):
        mr.exact(f"{name} {k}: fused route against the existing one", vp_new[k].cpu(), vp_old[k].cpu())
    assert new["cand_angles"] == old["cand_angles"] and new["cand_distances"] == old["cand_distances"]
    for a, b in zip(new["cand_img_idxes"], old["cand_img_idxes"]):
        assert a.tolist() == b.tolist()
    for a, b in zip(new["cand_angle_fts"], old["cand_angle_fts"]):
        mr.exact(f"{name} cand_angle_fts", a.contiguous(), b.contiguous())
    assert not new["pano_inputs"]["status"].any()
    checked(f"e2e {name} fused", {k: v.cpu().numpy() for k, v in new["pano_inputs"].items()}, ref)
    d_old = vp_old["dep_fts"].cpu().numpy().astype(np.float64)
    assert (np.abs(d_old - ref["dep_fts"]) <= ref["dep_bound"]).all(), f"{name}: the existing route's dep_fts leaves the bound"


def test_fused_route_is_the_existing_route_with_native_encoders(net):
    from etpnav_amd import clip as cl
    from etpnav_amd import depth as dp
    from tests import clip_ref as cr
    from tests import depth_ref as dr
    from tests import waypoint_ref as wr
    B, S = 3, 64
    _, bp, blocks = dr.ALL_CASES[0]
    rgb_enc = cl.CLIPEncoder(device=DEV, dtype=torch.bfloat16, image_size=S, layers=2)
    rgb_enc.load_state_dict(cr.make_weights(S, 2, 3), strict=True)
    dep_enc = dp.DepthEncoder(device=DEV, dtype=torch.bfloat16, image_size=S, base_planes=bp, blocks=blocks)
    dep_enc.load_state_dict(dr.make_weights(S, bp, blocks, 3), strict=True)
    images, depth = cr.make_images(12 * B, S, 3), dr.make_depth(0, 12 * B, S)
    obs = {}
    for a in range(12):                          # the rollout's key order: rgb, depth, rgb_30.0, depth_30.0, ...
        suffix = "" if a == 0 else f"_{a * 30.0}"
        obs["rgb" + suffix] = images[(12 - a) % 12::12].contiguous().to(DEV)
        obs["depth" + suffix] = depth[(12 - a) % 12::12].contiguous().to(DEV)
    pred = wp.BinaryDistPredictorTRM(device=DEV, dtype=torch.float32)
    pred.load_state_dict(wr.make_weights(2), strict=True)
    net.rgb_encoder, net.depth_encoder = rgb_enc, dep_enc
    try:
        rgb_e = rgb_enc.encode_views(obs).float().cpu().numpy()
        dep_e = dep_enc.encode_views(obs).float().reshape(12 * B, 128, 16).cpu().numpy()
        assert np.abs(dep_e).max() > 0 and np.abs(rgb_e).max() > 0
        uniforms = torch.rand(B, 5, generator=torch.Generator().manual_seed(4)).to(DEV)
        for in_train in (False, True):
            old, vp_old, new, vp_new = both_routes(net, pred, obs, in_train, uniforms)
            table = pred.candidates(pred(None, torch.from_numpy(dep_e).to(DEV).reshape(12 * B, 128, 4, 4)), in_train, uniforms=uniforms).table.cpu().numpy()
            V = pir.ref_length(table, in_train)
            assert V == vp_new["rgb_fts"].shape[1] == vp_old["rgb_fts"].shape[1]
            compare_routes(f"native encoders train={in_train}", old, vp_old, new, vp_new, pir.pano_inputs(rgb_e, dep_e, table, in_train, V))
        # a fixed capacity: the same rows, zero rows behind them, and forward_panorama takes it
        net.fuse_pano_inputs, net.pano_inputs_capacity = True, 16
        cap = graph_inputs.vp_feature_variable(net(mode="waypoint", waypoint_predictor=pred, observations=obs, in_train=False), DEV)
        net.fuse_pano_inputs, net.pano_inputs_capacity = False, None
        _, vp_old, _, vp_new = both_routes(net, pred, obs, False, uniforms)
        Vr = vp_new["rgb_fts"].shape[1]
        assert cap["rgb_fts"].shape[1] == 16
        for k in ("rgb_fts", "dep_fts", "loc_fts", "nav_types"):
            mr.exact(f"capacity 16 {k}", cap[k][:, :Vr].contiguous().cpu(), vp_new[k].cpu())
            assert not cap[k][:, Vr:].any()
        mr.exact("capacity 16 view_lens", cap["view_lens"].cpu(), vp_new["view_lens"].cpu())
        with torch.no_grad():
            for vp in (vp_new, cap):
                embeds, masks = net(mode="panorama", **vp)
                assert tuple(embeds.shape[:2]) == tuple(vp["rgb_fts"].shape[:2]) and bool(torch.isfinite(embeds.float()).all())
                assert masks.sum(1).tolist() == vp["view_lens"].tolist()
    finally:
        net.rgb_encoder = net.depth_encoder = None
        net.fuse_pano_inputs, net.pano_inputs_capacity = False, None


class _Lookup(torch.nn.Module):
    """a stand-in as a module (the fixture's net has held module encoders: torch then takes modules only under those names)"""

    def __init__(self, fn):
        super().__init__()
        self.fn = fn

    def forward(self, o):
        return self.fn(o)


class _Encoders:
    """stand-ins for the perception encoders: look the stored embedding up by the view id painted into the observation"""

    def __init__(self, golden):
        self.depth_table = torch.from_numpy(golden["depth_table"].astype(np.float32)).to(DEV)
        self.rgb_table = torch.from_numpy(golden["rgb_table"].astype(np.float32)).to(DEV)

    def depth(self, o):
        return self.depth_table[o["depth"][:, 0, 0, 0].long()].reshape(-1, 128, 4, 4)

    def rgb(self, o):
        return self.rgb_table[o["rgb"][:, 0, 0, 0].long()]


def test_fused_route_replays_the_recorded_branch(net):
    from tests import waypoint_ref as wr
    z = dict(np.load(GOLDEN))
    pred = wp.BinaryDistPredictorTRM(device=DEV, dtype=torch.float32)
    pred.load_state_dict(wr.make_weights(int(z["seed"]), float(z["cls_scale"])), strict=True)
    obs = {}
    for a in range(12):
        suffix = "" if a == 0 else f"_{a * 30.0}"
        ids = (torch.arange(3) * 12 + a).float().reshape(3, 1, 1, 1)
        obs["rgb" + suffix], obs["depth" + suffix] = ids.expand(3, 2, 2, 3).clone().to(DEV), ids.expand(3, 2, 2, 1).clone().to(DEV)
    enc = _Encoders(z)
    net.depth_encoder, net.rgb_encoder = _Lookup(enc.depth), _Lookup(enc.rgb)
    rgb, dep = pir.golden_tables(z)
    table = pir.golden_table(z)
    try:
        for in_train in (False, True):
            prefix = "train_" if in_train else "eval_"
            old, vp_old, new, vp_new = both_routes(net, pred, obs, in_train, torch.from_numpy(z["uniforms"]).to(DEV))
            V = pir.ref_length(table, in_train)
            ref = pir.pano_inputs(rgb, dep, table, in_train, V)
            compare_routes(f"recording {prefix}", old, vp_old, new, vp_new, ref)
            for j in range(3):                               # the recording itself: the candidates the real branch picked
                assert new["cand_img_idxes"][j].tolist() == z[f"{prefix}cand_img_idxes_{j}"].tolist()
                np.testing.assert_allclose(new["cand_angles"][j], z[f"{prefix}cand_angles_{j}"], rtol=0, atol=1e-5)
                np.testing.assert_allclose(new["cand_distances"][j], z[f"{prefix}cand_distances_{j}"], rtol=0, atol=1e-5)
                k = len(new["cand_angles"][j])
                got = new["pano_inputs"]["rgb_fts"][j, :k].cpu().numpy()
                assert got.tobytes() == z[f"{prefix}cand_rgb_{j}"].tobytes()
    finally:
        net.depth_encoder = net.rgb_encoder = None
