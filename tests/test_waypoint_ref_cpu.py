"""tests/waypoint_ref.py (the fp64 restatement the GPU tests of the waypoint head compare against) pinned down on the CPU:

  * where the reference tree is present (/root/reference, or $ETP_REFERENCE), it equals the REAL classes at 1e-10 on random inputs:
    head against BinaryDistPredictor_TRM in fp64, tail against the real nms on the wrapped map, window mask against
    get_attention_mask for n = 0 .. 5;
  * everywhere, it equals tests/golden/waypoint_small.npz (recorded from the real classes by tools/make_golden_waypoint.py);
  * every deliberate error of waypoint_ref.MUTATIONS is rejected by those recordings;
  * the input conditions the GPU comparison rests on hold for every shared case.
"""
import importlib
import os
import sys
import types

import numpy as np
import pytest
import torch

from tests import waypoint_ref as wr

REF = os.environ.get("ETP_REFERENCE", "/root/reference")
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "waypoint_small.npz")
needs_ref = pytest.mark.skipif(not os.path.isdir(os.path.join(REF, "vlnce_baselines", "waypoint_pred")),
                               reason="the reference tree is not on this machine")


@pytest.fixture(scope="module")
def golden():
    g = dict(np.load(GOLDEN))
    g["W"] = wr.make_weights(int(g["seed"]), float(g["cls_scale"]))
    return g


@pytest.fixture(scope="module")
def ref():
    """(TRM_net, utils) of the reference, imported with stand-ins for boto3 / botocore (never called) and a pytorch_transformers
    whose BertConfig is the vendored one"""
    for n in ("boto3", "botocore", "botocore.exceptions"):
        sys.modules.setdefault(n, types.ModuleType(n))
    sys.modules["botocore.exceptions"].ClientError = Exception
    for pk in ("vlnce_baselines", "vlnce_baselines.waypoint_pred", "vlnce_baselines.waypoint_pred.transformer",
               "vlnce_baselines.waypoint_pred.transformer.pytorch_transformer"):
        if pk not in sys.modules:
            m = types.ModuleType(pk)
            m.__path__ = [os.path.join(REF, *pk.split("."))]
            sys.modules[pk] = m
    mb = importlib.import_module("vlnce_baselines.waypoint_pred.transformer.pytorch_transformer.modeling_bert")
    if "pytorch_transformers" not in sys.modules:
        pt = types.ModuleType("pytorch_transformers")
        pt.BertConfig = mb.BertConfig
        sys.modules["pytorch_transformers"] = pt
    return (importlib.import_module("vlnce_baselines.waypoint_pred.TRM_net"),
            importlib.import_module("vlnce_baselines.waypoint_pred.utils"))


def real_tail(ut, logits, max_pred):
    L = torch.as_tensor(logits).double()
    B = L.shape[0]
    p = torch.softmax(L.reshape(B, -1), 1).reshape(B, 120, 12)
    wrap = torch.cat((p[:, -1:], p, p[:, :1]), 1)
    return p.numpy(), ut.nms(wrap.unsqueeze(1), max_predictions=max_pred, sigma=(7.0, 5.0)).squeeze(1)[:, 1:-1].numpy()


def all_tail_cases():
    return ([(f"random B={B} max_pred={mp}", wr.tail_random(B, mp), mp) for B, mp in wr.TAIL_RANDOM]
            + [(f"{k} max_pred={mp}", wr.tail_crafted(k), mp) for k in wr.CRAFTED for mp in (5, 8)])


# ---- against the real classes ------------------------------------------------------------------------------------------------------
@needs_ref
def test_head_equals_the_real_predictor_in_fp64(ref):
    trm, _ = ref
    W = wr.make_weights(7)
    m = trm.BinaryDistPredictor_TRM(device="cpu").double().eval()
    assert list(m.state_dict().keys()) == [k for k, _ in wr.param_shapes()]
    assert [tuple(v.shape) for v in m.state_dict().values()] == [s for _, s in wr.param_shapes()]
    m.load_state_dict({k: v.double() for k, v in W.items()}, strict=True)
    d = torch.from_numpy(np.abs(np.random.default_rng(1).standard_normal((24, 2048))))
    with torch.no_grad():
        want = m(torch.zeros(24, 1), d.reshape(24, 128, 4, 4))
    got = wr.head_ref(W, d)
    assert tuple(got.shape) == (2, 120, 12)
    assert float((got - want).abs().max()) <= 1e-10
    for mut in ("roll", "window"):
        assert float((wr.head_ref(W, d, mut=mut) - want).abs().max()) > 1e-3, mut


@needs_ref
def test_tail_equals_the_real_nms(ref):
    _, ut = ref
    for name, logits, mp in all_tail_cases():
        p, o = real_tail(ut, logits, mp)
        t = wr.tail_ref(logits, mp)
        assert np.abs(p - t["heat"]).max() <= 1e-10, name
        assert np.abs(o - t["nms_map"]).max() <= 1e-10, name
        assert ((o != 0) == (t["nms_map"] != 0)).all(), name
        a, d = np.nonzero(o[0])
        assert t["angle"][0, :len(a)].tolist() == a.tolist() and t["dist"][0, :len(a)].tolist() == d.tolist(), name


@needs_ref
def test_window_mask_equals_get_attention_mask(ref):
    _, ut = ref
    for n in range(6):
        assert (ut.get_attention_mask(12, n).reshape(12, 12).numpy() == wr.ring_mask(n)).all(), n


# ---- against the committed recordings ----------------------------------------------------------------------------------------------
def test_fixture_weights_are_the_generated_ones(golden):
    fp = wr.fingerprint(golden["W"])
    assert [str(k) for k in golden["keys"]] == [k for k, _ in wr.param_shapes()]
    assert len(golden["keys"]) == 42 and sum(int(np.prod(s)) for _, s in wr.param_shapes()) == 17614200
    np.testing.assert_allclose(np.array([fp[k] for k, _ in wr.param_shapes()]), golden["fingerprint"], rtol=1e-12, atol=0)
    assert tuple(golden["depth_cw"].shape) == (36, 2048) and golden["depth_cw"].dtype == np.float16


def test_head_equals_the_fixture(golden):
    d = torch.from_numpy(golden["depth_cw"].astype(np.float32))
    got = wr.head_ref(golden["W"], d)
    # the recording is the reference's fp32 run: its own rounding is what separates the two
    assert float((got - torch.from_numpy(golden["logits"]).double()).abs().max()) <= 2e-5
    for mut in ("roll", "window"):
        assert float((wr.head_ref(golden["W"], d, mut=mut) - torch.from_numpy(golden["logits"]).double()).abs().max()) > 1e-2, mut


def test_tail_equals_the_fixture(golden):
    t = wr.tail_ref(golden["logits"], 5, uniforms=golden["uniforms"])
    assert np.abs(t["heat"] - golden["heat"]).max() <= 1e-6
    assert ((t["nms_map"] != 0) == (golden["nms_map"] != 0)).all()
    assert np.abs(t["nms_map"] - golden["nms_map"]).max() <= 1e-6
    for j in range(3):
        n = int(t["count"][j])
        # eval: the candidates are the non-zero cells; train: the recorded samples of the real branch
        np.testing.assert_allclose(golden[f"eval_cand_angles_{j}"], 2 * np.pi - t["angle"][j, :n] / 120 * 2 * np.pi, atol=1e-5)
        np.testing.assert_allclose(golden[f"eval_cand_distances_{j}"], (t["dist"][j, :n] + 1) * 0.25, atol=1e-6)
        assert golden[f"eval_cand_img_idxes_{j}"].tolist() == t["img_ccw"][j, :n].tolist()
        np.testing.assert_allclose(golden[f"train_cand_angles_{j}"], 2 * np.pi - t["samp_angle"][j, :n] / 120 * 2 * np.pi, atol=1e-5)
        np.testing.assert_allclose(golden[f"train_cand_distances_{j}"], (t["samp_dist"][j, :n] + 1) * 0.25, atol=1e-6)
    for kind in wr.CRAFTED:
        tc = wr.tail_ref(wr.tail_crafted(kind), 5)
        n = int(tc["count"][0])
        assert np.stack((tc["angle"][0, :n], tc["dist"][0, :n]), 1).tolist() == golden["crafted_" + kind].tolist(), kind


def _train_cells(golden, t):
    return [(np.round((2 * np.pi - golden[f"train_cand_angles_{j}"]) / (2 * np.pi) * 120).astype(int).tolist()
             == t["samp_angle"][j, :int(t["count"][j])].tolist()) for j in range(3)]


@pytest.mark.parametrize("mut", [m for m in wr.MUTATIONS if m not in ("roll", "window")])
def test_tail_mutations_are_rejected_by_the_recordings(golden, mut):
    """each deliberate error changes the candidate cells of at least one recorded map (the crafted maps under the real nms, the
    fixture's sampled cells under the real waypoint branch)"""
    seen = []
    for kind in wr.CRAFTED:
        tc = wr.tail_ref(wr.tail_crafted(kind), 5, mut=mut)
        n = int(tc["count"][0])
        if np.stack((tc["angle"][0, :n], tc["dist"][0, :n]), 1).tolist() != golden["crafted_" + kind].tolist():
            seen.append(kind)
    t = wr.tail_ref(golden["logits"], 5, uniforms=golden["uniforms"], mut=mut)
    if not all(_train_cells(golden, t)):
        seen.append("fixture samples")
    assert seen, f"mutation {mut} passes every recording"
    expect = {"intdiv": "five_apart_d2", "noncircular": "dist_ends", "nowrap": "angle0", "last": "tie", "pointer": "fixture samples"}[mut]
    assert expect in seen, (mut, seen)


def test_input_conditions_hold_for_every_shared_case(golden):
    for name, logits, mp in all_tail_cases():
        wr.check_conditions(logits, mp, wr.make_uniforms(logits, mp, 1), name=name)
    t = wr.check_conditions(golden["logits"], 5, golden["uniforms"], name="fixture")
    gap = float(golden["bf16_autocast_gap"])
    assert all(min(ms) >= 4 * gap for ms in t["margins"]), ([min(ms) for ms in t["margins"]], gap)
    assert t["count"].tolist() == [5, 5, 5]


def test_bounds_reject_small_errors():
    """the comparator fails on an error of two bounds, in an element of ctx and in a heat cell"""
    q, k, v = wr.attn_case(2, 1, True)
    ctx, E = wr.ring_attn_ref(q, k, v, 1, 0.125, True)
    wr.record("cpu/ctx", ctx.numpy(), ctx.numpy(), E.numpy(), "exact")
    bad = ctx.clone()
    bad[1, 3, 5, 7] += 2 * E[1, 3, 5, 7]
    with pytest.raises(AssertionError):
        wr.record("cpu/ctx", bad.numpy(), ctx.numpy(), E.numpy(), "two bounds off")
    # fp32 emulation of the documented schedule stays inside the bound
    s = 0.125 * (q[:, :, :, None, :] * k[:, :, [[(i + o) % 12 for o in (-1, 0, 1)] for i in range(12)]]).sum(-1)
    P = torch.softmax(s, -1)
    emu = (P[..., None] * v[:, :, [[(i + o) % 12 for o in (-1, 0, 1)] for i in range(12)]]).sum(-2).bfloat16().double()
    assert wr.record("cpu/ctx", emu.numpy(), ctx.numpy(), E.numpy(), "fp32 emulation, bf16 store") <= 1.0
    logits = wr.tail_random(1, 5)
    ref = wr.tail_ref(logits, 5)
    Eh = wr.heat_bound(logits)
    h32 = torch.softmax(torch.from_numpy(logits).reshape(1, -1), 1).reshape(1, 120, 12).double().numpy()
    assert wr.record("cpu/heat", h32, ref["heat"], Eh, "torch fp32 softmax") <= 1.0
    badh = ref["heat"].copy()
    badh[0, 7, 7] *= 1.0 + 1e-5
    with pytest.raises(AssertionError):
        wr.record("cpu/heat", badh, ref["heat"], Eh, "1e-5 relative")
    for key in [k for k in wr.WORST if k.startswith("cpu/")]:
        del wr.WORST[key]
