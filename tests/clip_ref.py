"""float64 restatement of OpenAI CLIP's visual tower (clip/model.py VisionTransformer under encode_image, behind the reference's
CLIPEncoder, vlnce_baselines/models/encoders/resnet_encoders.py:244-278) under its own state-dict names, the counter-based weights and
images every CLIP test uses, and the derived bounds of the four kernels of etpnav_amd/csrc/clip.hip.

Weights and images.  No library RNG: element i of a tensor is splitmix64(i XOR key(tensor name, seed)); the top 53 bits give
u in [-1, 1).  Matrices are u * fan_in^-1/2, LayerNorm gains 1 + 0.1 u, biases and embeddings 0.02 u; image bytes are the top 8 bits.
Everything is rounded to fp32 once (the engine's arena is fp32) and the float64 restatement reads those fp32 values.  No weight file is
committed: ViT-B/32 is 350 MB.

The restatement (forward) is pinned to transformers.CLIPVisionModelWithProjection in float64 by tests/test_clip_ref_cpu.py and to
tests/golden/clip_small.npz (tools/make_golden_clip.py).  `mut` plants one deliberate mistake; the CPU test shows each is rejected.

Bounds.  u = 2^-24, gam(k) = k u / (1 - k u) (tests/reduce_ref.py).
  patch rows   exact: (float(x) / 255 - mean) / std in torch's fp32, then round-to-nearest-even for bf16.
  tokens       the row is prod + pos (one rounding: e_x = u |sum|) followed by the row schedule of ln_fwd_s_kernel, so the bound is
               reduce_ref.ln_fwd_bounds with that input error (4 NCH lane-sequential adds and the 6 butterfly levels).
  cls LN       the same with e_x = 0 (+ one bf16 ulp of the reference for a bf16 output, as reduce_ref does for every bf16 store).
  QuickGELU    (qgelu_bound) the kernel's instruction forms: t = fl(1.702f v); a = fl(t * -log2e); e = v_exp_f32(a) (one ulp);
               d = fl(1 + e); r = v_rcp_f32(d) (one ulp); y = fl(v r).  Constants: 1.702f and log2e in fp32 are each within u of the
               real number.  Relative error of a: 4 u (two constants, two products), i.e. |a| 4 u absolute, which is a relative error
               ln2 |a| 4 u = 4 u |1.702 v| of e; plus 2 u for the instruction.  That error reaches d scaled by e / (1 + e); d adds u,
               the reciprocal 2 u, the last product u.  Where e overflows or 1 / d falls below the smallest normal number the hardware
               returns 0 for a true value below |v| 2^-126: an absolute floor of (|v| + 1) 2^-126.  bf16 storage adds half a bf16 ulp of
               the reference (round to nearest).
"""
import zlib

import numpy as np
import torch

from tests import reduce_ref as rr
from tests.row_ref import ulp_bf16

F64 = torch.float64
U = rr.U
WIDTH, HEADS, INTER, PATCH, OUT = 768, 12, 3072, 32, 512
MEAN = (0.48145466, 0.4578275, 0.40821073)
STD = (0.26862954, 0.26130258, 0.27577711)
EPS = 1e-5
M64 = (1 << 64) - 1


# ---- counter-based values -------------------------------------------------------------------------------------------------------
def _splitmix64(z):
    with np.errstate(over="ignore"):
        z = z + np.uint64(0x9E3779B97F4A7C15)
        z = (z ^ (z >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
        z = (z ^ (z >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
        return z ^ (z >> np.uint64(31))


def tensor_key(name, seed):
    return int(_splitmix64(np.array([(zlib.crc32(name.encode()) | (int(seed) << 32)) & M64], dtype=np.uint64))[0])


def hash_bits(name, seed, n):
    idx = np.arange(n, dtype=np.uint64)
    return _splitmix64(idx ^ np.uint64(tensor_key(name, seed)))


def hash_uniform(name, seed, shape):
    """float64 tensor of `shape`, element i = top 53 bits of the hash as u in [-1, 1)"""
    n = int(np.prod(shape))
    u = (hash_bits(name, seed, n) >> np.uint64(11)).astype(np.float64) * (2.0 ** -52) - 1.0
    return torch.from_numpy(u).reshape(*shape)


def hash_bytes(name, seed, shape):
    n = int(np.prod(shape))
    return torch.from_numpy((hash_bits(name, seed, n) >> np.uint64(56)).astype(np.uint8)).reshape(*shape)


def param_shapes(image_size=224, layers=12):
    """OpenAI CLIP's visual.* keys (prefix stripped) in state-dict order, with their shapes"""
    T = (image_size // PATCH) ** 2 + 1
    out = [("class_embedding", (WIDTH,)), ("positional_embedding", (T, WIDTH)), ("proj", (WIDTH, OUT)),
           ("conv1.weight", (WIDTH, 3, PATCH, PATCH)), ("ln_pre.weight", (WIDTH,)), ("ln_pre.bias", (WIDTH,))]
    for i in range(layers):
        p = f"transformer.resblocks.{i}."
        out += [(p + "attn.in_proj_weight", (3 * WIDTH, WIDTH)), (p + "attn.in_proj_bias", (3 * WIDTH,)),
                (p + "attn.out_proj.weight", (WIDTH, WIDTH)), (p + "attn.out_proj.bias", (WIDTH,)),
                (p + "ln_1.weight", (WIDTH,)), (p + "ln_1.bias", (WIDTH,)),
                (p + "mlp.c_fc.weight", (INTER, WIDTH)), (p + "mlp.c_fc.bias", (INTER,)),
                (p + "mlp.c_proj.weight", (WIDTH, INTER)), (p + "mlp.c_proj.bias", (WIDTH,)),
                (p + "ln_2.weight", (WIDTH,)), (p + "ln_2.bias", (WIDTH,))]
    return out + [("ln_post.weight", (WIDTH,)), ("ln_post.bias", (WIDTH,))]


def make_weights(image_size=224, layers=12, seed=1):
    """{name: fp32 tensor}: matrices u fan_in^-1/2, LayerNorm gains 1 + 0.1 u, biases and embeddings 0.02 u"""
    W = {}
    for name, shape in param_shapes(image_size, layers):
        u = hash_uniform(name, seed, shape)
        if name.startswith("ln_") and name.endswith("weight") or ".ln_" in name and name.endswith("weight"):
            v = 1.0 + 0.1 * u
        elif name == "proj":
            v = u * shape[0] ** -0.5                       # x @ proj: fan_in is the first axis
        elif name.endswith("weight") and len(shape) >= 2:
            v = u * float(np.prod(shape[1:])) ** -0.5
        else:
            v = 0.02 * u
        W[name] = v.to(torch.float32)
    return W


def make_images(n, image_size, seed=1, name="images"):
    return hash_bytes(name, seed, (n, image_size, image_size, 3))


# ---- the restatement -------------------------------------------------------------------------------------------------------------
def normalise(images, mut=None):
    """resnet_encoders.py:264-267,274-275 in torch's own fp32: [N, S, S, 3] uint8 -> [N, 3, S, S] fp32"""
    x = images.permute(0, 3, 1, 2).to(torch.float32) / 255
    mean = torch.tensor(MEAN, dtype=torch.float32, device=images.device)
    std = torch.tensor(STD, dtype=torch.float32, device=images.device)
    if mut == "mean_std_swapped":
        mean, std = std, mean
    if mut == "bgr":
        x = x.flip(1)
    return (x - mean.view(1, 3, 1, 1)) / std.view(1, 3, 1, 1)


def patch_rows(images, mut=None):
    """[N, S, S, 3] uint8 -> [N (S/32)^2, 3072] fp32, columns in conv1.weight's (c, ky, kx) order"""
    x = normalise(images, mut)
    N, _, S, _ = x.shape
    G = S // PATCH
    x = x.reshape(N, 3, G, PATCH, G, PATCH)
    if mut == "columns_kykxc":
        return x.permute(0, 2, 4, 3, 5, 1).reshape(N * G * G, 3 * PATCH * PATCH)
    return x.permute(0, 2, 4, 1, 3, 5).reshape(N * G * G, 3 * PATCH * PATCH)


def clockwise_slots(views):
    """the reference loop (Policy_ViewSelection_ETP.py:176-190) on a list of 12 [B, ...] tensors -> [12 B, ...]"""
    batch = torch.zeros_like(views[0]).repeat(12, *([1] * (views[0].dim() - 1)))
    for a_count, v in enumerate(views):
        batch[(12 - a_count) % 12::12] = v
    return batch


def layer_norm(x, g, b, eps=EPS):
    mu = x.mean(-1, keepdim=True)
    var = ((x - mu) ** 2).mean(-1, keepdim=True)
    return (x - mu) / torch.sqrt(var + eps) * g + b


def quick_gelu(x):
    return x * torch.sigmoid(1.702 * x)


def forward(W, images, layers, mut=None, dtype=F64):
    """-> (embeddings [N, 512], probes [3, N T, 768]: the residual stream after ln_pre, after layer 0, after the last layer)"""
    W = {k: v.to(dtype) for k, v in W.items()}
    N, S = images.shape[0], images.shape[1]
    P = (S // PATCH) ** 2
    rows = patch_rows(images, mut).to(dtype)
    prod = (rows @ W["conv1.weight"].reshape(WIDTH, -1).T).reshape(N, P, WIDTH)
    cls = W["class_embedding"].expand(N, 1, WIDTH)
    x = torch.cat([prod, cls], 1) if mut == "class_last" else torch.cat([cls, prod], 1)
    pos = W["positional_embedding"]
    x = x + (pos.roll(1, 0) if mut == "pos_shift" else pos)
    if mut != "no_ln_pre":
        x = layer_norm(x, W["ln_pre.weight"], W["ln_pre.bias"])
    probes = [x.reshape(-1, WIDTH).clone()]
    T = P + 1
    act = (lambda v: torch.nn.functional.gelu(v)) if mut == "erf_gelu" else quick_gelu
    for i in range(layers):
        p = f"transformer.resblocks.{i}."
        ln1 = lambda v: layer_norm(v, W[p + "ln_1.weight"], W[p + "ln_1.bias"])
        ln2 = lambda v: layer_norm(v, W[p + "ln_2.weight"], W[p + "ln_2.bias"])

        def attn(v):
            qkv = v @ W[p + "attn.in_proj_weight"].T + W[p + "attn.in_proj_bias"]
            q, k, val = (t.reshape(N, T, HEADS, 64).transpose(1, 2) for t in qkv.split(WIDTH, -1))
            s = q @ k.transpose(-1, -2) * (1.0 if mut == "no_scale" else 0.125)
            ctx = (torch.softmax(s, -1) @ val).transpose(1, 2).reshape(N, T, WIDTH)
            return ctx @ W[p + "attn.out_proj.weight"].T + W[p + "attn.out_proj.bias"]

        def mlp(v):
            return act(v @ W[p + "mlp.c_fc.weight"].T + W[p + "mlp.c_fc.bias"]) @ W[p + "mlp.c_proj.weight"].T + W[p + "mlp.c_proj.bias"]

        if mut == "post_norm":
            x = ln1(x + attn(x))
            x = ln2(x + mlp(x))
        else:
            x = x + attn(ln1(x))
            x = x + mlp(ln2(x))
        if i == 0:
            probes.append(x.reshape(-1, WIDTH).clone())
    probes.append(x.reshape(-1, WIDTH).clone())
    cls_row = x[:, -1] if mut == "class_last" else x[:, 0]
    y = layer_norm(cls_row, W["ln_post.weight"], W["ln_post.bias"]) @ W["proj"]
    return y, torch.stack(probes)


MUTATIONS = ("erf_gelu", "post_norm", "no_ln_pre", "class_last", "pos_shift", "no_scale", "bgr", "columns_kykxc", "mean_std_swapped")


# ---- transformers.CLIPVisionModelWithProjection with the same weights ------------------------------------------------------------
def hf_model(W, image_size, layers, dtype=F64):
    from transformers import CLIPVisionConfig, CLIPVisionModelWithProjection
    cfg = CLIPVisionConfig(hidden_size=WIDTH, intermediate_size=INTER, projection_dim=OUT, num_hidden_layers=layers,
                           num_attention_heads=HEADS, image_size=image_size, patch_size=PATCH, hidden_act="quick_gelu",
                           layer_norm_eps=EPS, attention_dropout=0.0)
    cfg._attn_implementation = "sdpa"
    m = CLIPVisionModelWithProjection(cfg).eval()
    sd = {"vision_model.embeddings.class_embedding": W["class_embedding"],
          "vision_model.embeddings.patch_embedding.weight": W["conv1.weight"],
          "vision_model.embeddings.position_embedding.weight": W["positional_embedding"],
          "vision_model.pre_layrnorm.weight": W["ln_pre.weight"], "vision_model.pre_layrnorm.bias": W["ln_pre.bias"],
          "vision_model.post_layernorm.weight": W["ln_post.weight"], "vision_model.post_layernorm.bias": W["ln_post.bias"],
          "visual_projection.weight": W["proj"].T.contiguous()}
    for i in range(layers):
        p, h = f"transformer.resblocks.{i}.", f"vision_model.encoder.layers.{i}."
        for j, n in enumerate(("q_proj", "k_proj", "v_proj")):            # in_proj is split into q / k / v
            sd[h + f"self_attn.{n}.weight"] = W[p + "attn.in_proj_weight"][j * WIDTH:(j + 1) * WIDTH]
            sd[h + f"self_attn.{n}.bias"] = W[p + "attn.in_proj_bias"][j * WIDTH:(j + 1) * WIDTH]
        for a, b in (("self_attn.out_proj", "attn.out_proj"), ("layer_norm1", "ln_1"), ("layer_norm2", "ln_2"), ("mlp.fc1", "mlp.c_fc"),
                     ("mlp.fc2", "mlp.c_proj")):
            sd[h + a + ".weight"], sd[h + a + ".bias"] = W[p + b + ".weight"], W[p + b + ".bias"]
    missing, unexpected = m.load_state_dict({k: v.clone() for k, v in sd.items()}, strict=False)
    assert not unexpected and all("position_ids" in k for k in missing), (missing, unexpected)
    return m.to(dtype)


def hf_forward(W, images, layers, dtype=F64, autocast=False):
    m = hf_model(W, images.shape[1], layers, dtype)
    px = normalise(images).to(dtype)
    with torch.no_grad():
        if autocast:
            with torch.autocast("cpu", dtype=torch.bfloat16):
                o = m(pixel_values=px, output_hidden_states=True)
        else:
            o = m(pixel_values=px, output_hidden_states=True)
    hs = o.hidden_states
    return o.image_embeds.to(F64), torch.stack([hs[0], hs[1], hs[-1]]).reshape(3, -1, WIDTH).to(F64)


def rel_l2(got, ref):
    return float((got.to(F64) - ref.to(F64)).norm() / ref.to(F64).norm())


# ---- the cases of the fixture and of the engine tests -----------------------------------------------------------------------------
GOLDEN_CASES = {"s64_l2_n3": (64, 2, 3), "s224_l12_n2": (224, 12, 2)}             # name -> (image size, layers, images)
ENGINE_CASES = {"s32_l1": (32, 1), "s64_l2": (64, 2), "s96_l2": (96, 2), "s224_l1": (224, 1), "s224_l12": (224, 12)}
CASE_SEED = 1


# ---- kernel bounds ----------------------------------------------------------------------------------------------------------------
def tokens_reference(prod, cls, pos, gamma, beta, N, T):
    """-> (fp64 reference [N T, 768], elementwise bound) of clip_tokens_kernel"""
    p64 = prod.to(F64).reshape(N, T - 1, WIDTH)
    x = torch.cat([cls.to(F64).expand(N, 1, WIDTH), p64], 1) + pos.to(F64)
    x = x.reshape(N * T, WIDTH)
    ref = layer_norm(x, gamma.to(F64), beta.to(F64))
    st = rr.ln_stats(x, EPS)
    bound, _ = rr.ln_fwd_bounds(x, gamma, beta, EPS, ref, st, False, e_x=U * x.abs())
    return ref, bound


def cls_ln_reference(x, gamma, beta, N, T, bf16_out):
    rows = x.to(F64).reshape(N, T, WIDTH)[:, 0]
    ref = layer_norm(rows, gamma.to(F64), beta.to(F64))
    bound, _ = rr.ln_fwd_bounds(rows, gamma, beta, EPS, ref, rr.ln_stats(rows, EPS), bf16_out)
    return ref, bound


def qgelu_reference(v):
    """fp64 v * sigmoid(1.702 v) of the fp32 / bf16 input values (NaN at -inf, +inf at +inf)"""
    v = v.to(F64)
    return v * torch.sigmoid(1.702 * v)


def qgelu_bound(v, ref, bf16_out):
    v = v.to(F64)
    fin = torch.isfinite(v)
    vv = torch.where(fin, v, torch.zeros_like(v))
    t = (1.702 * vv).abs()
    frac = torch.sigmoid(-1.702 * vv)                                     # e / (1 + e)
    rel = frac * (4 * U * t + 2 * U) + U + 2 * U + U
    rel = rel / (1 - rel)
    rf = torch.where(fin, ref, torch.zeros_like(ref))
    b = rel * rf.abs() + (vv.abs() + 1) * 2.0 ** -126
    if bf16_out:
        b = b + 0.5 * ulp_bf16(rf)
    return b


def qgelu_values(n, seed=3):
    """n fp32 values: hashed u * 30, with 0, +-88, +-inf and the function's minimum near -0.7 planted at the front"""
    v = (hash_uniform("qgelu", seed, (n,)) * 30).to(torch.float32)
    xmin = -0.7517915                                                     # argmin of v sigmoid(1.702 v): 1.702 v = -1.27846...
    special = torch.tensor([0.0, -0.0, 88.0, -88.0, float("inf"), float("-inf"), xmin, xmin + 1e-3], dtype=torch.float32)
    v[:special.numel()] = special
    return v
