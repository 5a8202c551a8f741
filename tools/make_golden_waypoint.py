"""Write tests/golden/waypoint_small.npz from the REAL reference code (build container only; needs the reference tree).

    python tools/make_golden_waypoint.py [--reference /root/reference]

Runs, on the CPU:
  * the real BinaryDistPredictor_TRM (vlnce_baselines/waypoint_pred/TRM_net.py) loaded from tests/waypoint_ref.make_weights(seed) --
    imported with stand-in modules for boto3 / botocore (imported by the vendored file_utils.py, never called) and a
    `pytorch_transformers` whose BertConfig is the vendored one (waypoint_pred/transformer/pytorch_transformer/modeling_bert.py);
  * the real nms (waypoint_pred/utils.py);
  * the real `mode == 'waypoint'` branch of ETP.forward (models/Policy_ViewSelection_ETP.py:172-342), cut out of the source with
    `ast` and executed unchanged against a stand-in `self` whose encoders look stored embeddings up by the view id painted into the
    observation (the way oracle/ref_trainer_fns.py runs the trainer's method bodies).  While it runs, torch.distributions.Categorical
    is a recording stand-in that draws by inverse CDF from stored uniforms.

No program text of the reference and no weights go into the file: inputs (fp16-exact embeddings, uniforms), recorded outputs, the
weight seed and a (sum, abs-max, L2) fingerprint per tensor.  The input conditions the GPU tests rest on are asserted here.
"""
import argparse
import ast
import importlib
import math
import os
import sys
import types
from copy import deepcopy

import numpy as np
import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from tests import waypoint_ref as wr  # noqa: E402

OUT = os.path.join(ROOT, "tests", "golden", "waypoint_small.npz")


def load_reference(ref):
    for n in ("boto3", "botocore", "botocore.exceptions"):
        sys.modules.setdefault(n, types.ModuleType(n))
    sys.modules["botocore.exceptions"].ClientError = Exception
    for pk in ("vlnce_baselines", "vlnce_baselines.waypoint_pred", "vlnce_baselines.waypoint_pred.transformer",
               "vlnce_baselines.waypoint_pred.transformer.pytorch_transformer"):
        m = types.ModuleType(pk)
        m.__path__ = [os.path.join(ref, *pk.split("."))]
        sys.modules[pk] = m
    mb = importlib.import_module("vlnce_baselines.waypoint_pred.transformer.pytorch_transformer.modeling_bert")
    pt = types.ModuleType("pytorch_transformers")
    pt.BertConfig = mb.BertConfig
    sys.modules["pytorch_transformers"] = pt
    return (importlib.import_module("vlnce_baselines.waypoint_pred.TRM_net"),
            importlib.import_module("vlnce_baselines.waypoint_pred.utils"))


def cut_function(path, name):
    tree = ast.parse(open(path).read())
    for node in ast.walk(tree):
        if isinstance(node, ast.FunctionDef) and node.name == name:
            return node
    raise KeyError(name)


def waypoint_branch(ref, nms):
    """the statements under `elif mode == 'waypoint':` of ETP.forward as a function (self, waypoint_predictor, observations, in_train)"""
    path = os.path.join(ref, "vlnce_baselines", "models", "Policy_ViewSelection_ETP.py")
    tree = ast.parse(open(path).read())
    etp = next(n for n in tree.body if isinstance(n, ast.ClassDef) and n.name == "ETP")
    fwd = next(n for n in etp.body if isinstance(n, ast.FunctionDef) and n.name == "forward")
    body = None
    for node in ast.walk(fwd):
        if (isinstance(node, ast.If) and isinstance(node.test, ast.Compare) and isinstance(node.test.left, ast.Name)
                and node.test.left.id == "mode" and isinstance(node.test.comparators[0], ast.Constant)
                and node.test.comparators[0].value == "waypoint"):
            body = node.body
    assert body is not None
    args = ast.arguments(posonlyargs=[], args=[ast.arg(arg=a) for a in ("self", "waypoint_predictor", "observations", "in_train")],
                         kwonlyargs=[], kw_defaults=[], defaults=[])
    fn = ast.FunctionDef(name="waypoint_branch", args=args, body=body, decorator_list=[], returns=None, **({"type_params": []} if sys.version_info >= (3, 12) else {}))
    mod = ast.fix_missing_locations(ast.Module(body=[fn], type_ignores=[]))
    ns = {"torch": torch, "F": F, "math": math, "np": np, "nms": nms, "deepcopy": deepcopy}
    utils_path = os.path.join(ref, "vlnce_baselines", "models", "utils.py")
    aft = ast.fix_missing_locations(ast.Module(body=[cut_function(utils_path, "angle_feature_torch")], type_ignores=[]))
    exec(compile(aft, utils_path, "exec"), ns)
    exec(compile(mod, path, "exec"), ns)
    return ns["waypoint_branch"], ns["angle_feature_torch"]


class RecordingCategorical:
    """stand-in for torch.distributions.Categorical: sample() is the inverse CDF at the stored uniforms of the next episode"""
    uniforms = None
    calls = 0
    probs_seen = []

    def __init__(self, probs):
        self.probs = probs

    def sample(self):
        j = RecordingCategorical.calls
        RecordingCategorical.calls += 1
        p = self.probs.double().numpy()
        RecordingCategorical.probs_seen.append(p)
        act = []
        for c in range(p.shape[0]):
            cdf = np.cumsum(p[c])
            act.append(min(int(np.searchsorted(cdf, float(RecordingCategorical.uniforms[j, c]) * cdf[-1], side="right")), p.shape[1] - 1))
        return torch.tensor(act, dtype=torch.long)


def observations_of(B):
    """12 counter-clockwise views per episode; every pixel of view a of episode b holds the id b*12 + a"""
    obs = {}
    for a in range(12):
        suffix = "" if a == 0 else f"_{a * 30.0}"
        ids = (torch.arange(B) * 12 + a).float().reshape(B, 1, 1, 1)
        obs["rgb" + suffix] = ids.expand(B, 2, 2, 3).clone()
        obs["depth" + suffix] = ids.expand(B, 2, 2, 1).clone()
    return obs


def stand_in_self(depth_table, rgb_table, angle_feature_torch):
    s = types.SimpleNamespace()
    s.depth_encoder = lambda o: depth_table[o["depth"][:, 0, 0, 0].long()].reshape(-1, 128, 4, 4)
    s.rgb_encoder = lambda o: rgb_table[o["rgb"][:, 0, 0, 0].long()]
    s.space_pool_depth = torch.nn.Sequential(torch.nn.AdaptiveAvgPool2d((1, 1)), torch.nn.Flatten(start_dim=2))
    s.space_pool_rgb = torch.nn.Sequential(torch.nn.AdaptiveAvgPool2d((1, 1)), torch.nn.Flatten(start_dim=2))
    s.pano_img_idxes = np.arange(0, 12, dtype=np.int64)
    s.pano_angle_fts = angle_feature_torch(torch.from_numpy((1 - s.pano_img_idxes / 12) * 2 * math.pi))
    return s


def pack_outputs(prefix, out, store):
    B = len(out["cand_rgb"])
    for k in ("cand_rgb", "cand_depth", "cand_angle_fts"):
        for j in range(B):
            store[f"{prefix}{k}_{j}"] = out[k][j].numpy()
    for j in range(B):
        store[f"{prefix}cand_img_idxes_{j}"] = np.asarray(out["cand_img_idxes"][j])
        store[f"{prefix}cand_angles_{j}"] = np.asarray(out["cand_angles"][j], dtype=np.float64)
        store[f"{prefix}cand_distances_{j}"] = np.asarray(out["cand_distances"][j], dtype=np.float64)
    store[prefix + "pano_rgb"] = out["pano_rgb"].numpy()
    store[prefix + "pano_depth"] = out["pano_depth"].numpy()
    store[prefix + "pano_angle_fts"] = out["pano_angle_fts"].numpy()
    store[prefix + "pano_img_idxes"] = np.asarray(out["pano_img_idxes"])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reference", default="/root/reference")
    a = ap.parse_args()
    trm, ut = load_reference(a.reference)
    branch, angle_feature_torch = waypoint_branch(a.reference, ut.nms)
    B, seed = wr.GOLDEN_B, wr.GOLDEN_SEED
    W = wr.make_weights(seed)
    model = trm.BinaryDistPredictor_TRM(device="cpu").eval()
    model.load_state_dict(W, strict=True)
    rng = np.random.default_rng(900 + seed)
    # golden_depth is in the clockwise order the predictor sees; the id-indexed table holds view a of episode b (counter-clockwise)
    # at row b*12 + a, i.e. clockwise slot (12 - a) % 12
    cw = wr.golden_depth(seed).reshape(B, 12, 2048)
    depth_table = cw[:, [(12 - a) % 12 for a in range(12)]].reshape(12 * B, 2048).contiguous()
    rgb_table = torch.from_numpy(rng.standard_normal((12 * B, 512)).astype(np.float16).astype(np.float32))
    obs = observations_of(B)
    me = stand_in_self(depth_table, rgb_table, angle_feature_torch)
    store = {"seed": np.int64(seed), "cls_scale": np.float64(wr.CLS_SCALE), "depth_table": depth_table.numpy().astype(np.float16),
             "rgb_table": rgb_table.numpy().astype(np.float16), "keys": np.array([k for k, _ in wr.param_shapes()]),
             "note": np.array(f"vis_classifier.2.weight of make_weights is scaled by {wr.CLS_SCALE}; that scale moves the pick margins and "
                              f"the bf16 autocast gap alike, so the three episodes are numbers {wr.GOLDEN_EPISODES} of a seeded pool of "
                              f"{wr.GOLDEN_POOL}, the ones whose every pick leads by 4 x the gap")}
    fp = wr.fingerprint(W)
    store["fingerprint"] = np.array([fp[k] for k, _ in wr.param_shapes()], dtype=np.float64)
    assert [k for k, _ in wr.param_shapes()] == list(model.state_dict().keys())

    # in_train False, and the clockwise depth embeddings / logits the branch saw
    seen = {}
    real_forward = model.forward
    def spy(rgb, depth):
        seen["depth_cw"] = depth.detach().clone()
        seen["logits"] = real_forward(rgb, depth)
        return seen["logits"]
    with torch.no_grad():
        out_eval = branch(me, spy, obs, False)
    logits = seen["logits"].detach()
    assert torch.equal(seen["depth_cw"].reshape(12 * B, 2048), wr.golden_depth(seed))
    store["depth_cw"] = seen["depth_cw"].reshape(12 * B, 2048).numpy().astype(np.float16)
    store["logits"] = logits.numpy()
    pack_outputs("eval_", out_eval, store)

    # heat and nms map from the real nms
    p = torch.softmax(logits.reshape(B, -1), 1).reshape(B, 120, 12)
    wrap = torch.cat((p[:, -1:], p, p[:, :1]), 1)
    store["heat"] = p.numpy()
    store["nms_map"] = ut.nms(wrap.unsqueeze(1), max_predictions=5, sigma=(7.0, 5.0)).squeeze(1)[:, 1:-1].numpy()

    # in_train True with stored uniforms through the recording Categorical
    uniforms = wr.make_uniforms(logits, 5, seed)
    store["uniforms"] = uniforms
    RecordingCategorical.uniforms, RecordingCategorical.calls = uniforms, 0
    real_cat = torch.distributions.Categorical
    torch.distributions.Categorical = RecordingCategorical
    try:
        with torch.no_grad():
            out_train = branch(me, spy, obs, True)
    finally:
        torch.distributions.Categorical = real_cat
    pack_outputs("train_", out_train, store)

    # the reference's own bf16 gap: autocast(bfloat16) on the CPU against its fp32
    with torch.no_grad(), torch.autocast("cpu", dtype=torch.bfloat16):
        lg_bf16 = real_forward(torch.zeros(12 * B, 1), seen["depth_cw"]).float()
    gap = float((lg_bf16 - logits).abs().max())
    store["bf16_autocast_gap"] = np.float64(gap)

    # the real nms on the crafted maps of tests/waypoint_ref.py (max_predictions 5): the candidate cells, row-major
    for kind in wr.CRAFTED:
        L = torch.from_numpy(wr.tail_crafted(kind))
        pc = torch.softmax(L.reshape(1, -1), 1).reshape(1, 120, 12)
        o = ut.nms(torch.cat((pc[:, -1:], pc, pc[:, :1]), 1).unsqueeze(1), max_predictions=5, sigma=(7.0, 5.0)).squeeze(1)[0, 1:-1]
        store["crafted_" + kind] = o.nonzero().numpy()

    # ---- input conditions (fp64 restatement alone) ----
    t = wr.check_conditions(logits, 5, uniforms, name="fixture")
    margins = [min(ms) for ms in t["margins"]]
    store["pick_margins"] = np.asarray(margins, dtype=np.float64)
    assert all(m >= 4 * gap for m in margins), (
        f"pick margins {margins} against 4 x the bf16 autocast gap {gap}: raise tests/waypoint_ref.CLS_SCALE")
    ref64 = wr.head_ref(W, seen["depth_cw"].reshape(12 * B, 2048))
    err = float((ref64 - logits.double()).abs().max())
    assert err < 2e-4, err
    assert (t["nms_map"] != 0).tolist() == (store["nms_map"] != 0).tolist()
    np.savez_compressed(OUT, **store)
    print(f"{OUT}: {os.path.getsize(OUT)} bytes; logits |max| {float(logits.abs().max()):.3f}, fp64 restatement within {err:.2e}, "
          f"bf16 autocast gap {gap:.4f}, pick margins {['%.3f' % m for m in margins]}, counts {t['count'].tolist()}, "
          f"episodes {wr.GOLDEN_EPISODES} of a pool of {wr.GOLDEN_POOL} (vis_classifier.2.weight x {wr.CLS_SCALE}): every pick leads by 4 x the gap")


if __name__ == "__main__":
    main()
