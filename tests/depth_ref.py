"""The DD-PPO ResNet depth encoder in plain torch and in float64 NHWC, the counter-based weights and depth images every depth test uses,
the case lists and the derived bounds of the kernels of etpnav_amd/csrc/depth.hip.

Architecture.  habitat_baselines is not installed here, so `ResNetEncoder` below restates habitat-lab's rl/ddppo/policy/resnet.py
(ResNet, Bottleneck) and resnet_policy.py::ResNetEncoder from their source, with habitat's attribute names (backbone.conv1,
backbone.layer1..4[i].convs / .downsample, compression), as VlnResnetDepthEncoder builds them
(vlnce_baselines/models/encoders/resnet_encoders.py:26-32: baseplanes 32, ngroups baseplanes // 2, resnet50, no input normalisation).
Its state_dict() is the key contract: 162 tensors, 7 069 408 parameters.  `forward64` restates every operator in float64 on NHWC
tensors; tests/test_depth_ref_cpu.py pins it to the module in float64 and to tests/golden/depth_small.npz (tools/make_golden_depth.py).
`mut` plants one deliberate mistake; the CPU test shows each is rejected.

Weights and images.  No library RNG: element i of a tensor is a hash of (tensor name, seed, i) (tests/clip_ref.py), u in [-1, 1).
Convolutions are 0.05 u (2 / fan_in)^1/2 -- small on purpose: the pre-norm variances are then ~1e-3, where GroupNorm's eps = 1e-5 is a
visible part of var + eps, so a wrong eps is a visible mistake --, GroupNorm gains 1 + 0.3 u, biases 0.2 u, depth pixels (u + 1) / 2.
Everything is rounded to fp32 once and the float64 restatement reads those fp32 values.

Bounds.  u = 2^-24, gam(k) = k u / (1 - k u).
  stem        pooled = ((a + b) + (c + d)) * 0.25: three roundings (the scaling is exact); 49 fused multiply-adds in tap order: the
              classical bound of a length-49 recursive sum of products with a relative error gam(3) already in one factor, i.e.
              |err| <= gam(52) sum_taps |w| |pooled|, elementwise, no multiplier.
  gn_stats    schedule of gn_stats_kernel: d = x - pivot (one rounding); per channel R partial sums of ceil(HW / R) terms each, then R
              terms, then the group's channels lane-strided (ceil(cg / 64) terms) and 6 butterfly levels: every term passes through at
              most k = ceil(HW / R) + R + ceil(cg / 64) + 6 additions (stats_depth).  With D = mean |x - pivot|:
              |mean err| <= gam(k + 2) D + u |mean|                       (d, the k additions, the division; the final addition)
              q = sum fl(fl(x - m)^2) / n: |var err| <= gam(k + 4) (var + dm^2) + 2 dm sqrt(var) + dm^2 =: dv   (dm = the line above)
              rstd = 1 / sqrt(var + eps): |f(v') - f(v)| <= dv / (2 (v + eps - dv)^(3/2)) (f' is monotone), + 3 u rstd (add, sqrt, div).
  gn_apply    y = fl(fl(fl(x - m) r) g) + b: relative 3 u on the product, u on each sum, with the statistics it was GIVEN (the test
              feeds the kernel's own statistics to the reference): |err| <= gam(4) (|x - m| r |g| + |b|); every residual adds its own
              such term and one more rounding u |y|; bf16 storage is checked bitwise against the fp32 run instead.
"""

import numpy as np
import torch
import torch.nn as nn
import torch.nn.functional as F

from tests import reduce_ref as rr
from tests.clip_ref import hash_uniform

F64 = torch.float64
U = rr.U
EPS = 1e-5
NUM_IMGS = 12
FULL = (256, 32, (3, 4, 6, 3))
N_TENSORS, N_PARAMS = 162, 7069408


# ---- the torch module (habitat's names) -------------------------------------------------------------------------------------------
def conv3x3(i, o, stride=1):
    return nn.Conv2d(i, o, 3, stride, 1, bias=False)


def conv1x1(i, o, stride=1):
    return nn.Conv2d(i, o, 1, stride, bias=False)


class Bottleneck(nn.Module):
    expansion = 4

    def __init__(self, inplanes, planes, ngroups, stride=1, downsample=None):
        super().__init__()
        self.convs = nn.Sequential(conv1x1(inplanes, planes), nn.GroupNorm(ngroups, planes), nn.ReLU(True),
                                   conv3x3(planes, planes, stride), nn.GroupNorm(ngroups, planes), nn.ReLU(True),
                                   conv1x1(planes, planes * 4), nn.GroupNorm(ngroups, planes * 4))
        self.relu = nn.ReLU(True)
        self.downsample = downsample

    def forward(self, x):
        identity = x
        out = self.convs(x)
        if self.downsample is not None:
            identity = self.downsample(x)
        return self.relu(out + identity)


class ResNet(nn.Module):
    def __init__(self, in_channels, base_planes, ngroups, layers):
        super().__init__()
        self.conv1 = nn.Sequential(nn.Conv2d(in_channels, base_planes, 7, 2, 3, bias=False), nn.GroupNorm(ngroups, base_planes),
                                   nn.ReLU(True))
        self.maxpool = nn.MaxPool2d(3, 2, 1)
        self.inplanes = base_planes
        self.layer1 = self._make_layer(ngroups, base_planes, layers[0])
        self.layer2 = self._make_layer(ngroups, base_planes * 2, layers[1], 2)
        self.layer3 = self._make_layer(ngroups, base_planes * 4, layers[2], 2)
        self.layer4 = self._make_layer(ngroups, base_planes * 8, layers[3], 2)
        self.final_channels = self.inplanes
        self.final_spatial_compress = 1.0 / 32

    def _make_layer(self, ngroups, planes, blocks, stride=1):
        downsample = None
        if stride != 1 or self.inplanes != planes * 4:
            downsample = nn.Sequential(conv1x1(self.inplanes, planes * 4, stride), nn.GroupNorm(ngroups, planes * 4))
        layers = [Bottleneck(self.inplanes, planes, ngroups, stride, downsample)]
        self.inplanes = planes * 4
        for _ in range(1, blocks):
            layers.append(Bottleneck(self.inplanes, planes, ngroups))
        return nn.Sequential(*layers)

    def forward(self, x):
        x = self.maxpool(self.conv1(x))
        return self.layer4(self.layer3(self.layer2(self.layer1(x))))


class ResNetEncoder(nn.Module):
    """resnet_policy.py::ResNetEncoder for one depth channel, normalize_visual_inputs False"""

    def __init__(self, image_size=256, base_planes=32, blocks=(3, 4, 6, 3)):
        super().__init__()
        self.backbone = ResNet(1, base_planes, base_planes // 2, blocks)
        fs = int((image_size // 2) * self.backbone.final_spatial_compress)
        cc = int(round(2048 / (fs ** 2)))
        self.compression = nn.Sequential(nn.Conv2d(self.backbone.final_channels, cc, 3, padding=1, bias=False), nn.GroupNorm(1, cc),
                                         nn.ReLU(True))
        self.output_shape = (cc, fs, fs)

    def forward(self, observations):
        x = observations["depth"].permute(0, 3, 1, 2)
        x = F.avg_pool2d(x, 2)
        return self.compression(self.backbone(x))


# ---- counter-based weights and images ----------------------------------------------------------------------------------------------
def param_shapes(image_size=256, base_planes=32, blocks=(3, 4, 6, 3)):
    """the state dict's keys in its order, with their shapes (from the module itself, on the meta device)"""
    with torch.device("meta"):
        m = ResNetEncoder(image_size, base_planes, blocks)
    return [(k, tuple(v.shape)) for k, v in m.state_dict().items()]


def make_weights(image_size=256, base_planes=32, blocks=(3, 4, 6, 3), seed=1):
    W = {}
    for name, shape in param_shapes(image_size, base_planes, blocks):
        u = hash_uniform(name, seed, shape)
        if len(shape) == 4:
            v = 0.05 * u * (2.0 / float(np.prod(shape[1:]))) ** 0.5
        elif name.endswith("weight"):
            v = 1.0 + 0.3 * u
        else:
            v = 0.2 * u
        W[name] = v.to(torch.float32)
    return W


def make_depth(case_index, n, image_size, first=0):
    """n depth images [n, S, S, 1] fp32 in [0, 1): image i is a function of (case_index, first + i) alone"""
    return torch.stack([((hash_uniform(f"depth.{case_index}.{first + i}", 7, (image_size, image_size, 1)) + 1.0) * 0.5).to(torch.float32)
                        for i in range(n)])


def ddppo_checkpoint(W):
    """a synthetic DD-PPO checkpoint: the encoder under actor_critic.net.visual_encoder.*, beside keys the filter must drop"""
    sd = {"actor_critic.net.visual_encoder." + k: v.clone() for k, v in W.items()}
    sd["actor_critic.net.visual_fc.1.weight"] = torch.zeros(4, 4)
    sd["actor_critic.net.state_encoder.rnn.weight_ih_l0"] = torch.zeros(4, 4)
    sd["actor_critic.action_distribution.linear.weight"] = torch.zeros(4, 4)
    sd["actor_critic.critic.fc.bias"] = torch.zeros(1)
    return {"state_dict": sd, "extra_state": {"step": 0}}


# ---- float64 operators, NHWC -------------------------------------------------------------------------------------------------------
def pool2(depth):
    """[N, S, S, 1] -> [N, S/2, S/2, 1]: the 2x2 average"""
    x = depth[..., 0]
    return ((x[:, 0::2, 0::2] + x[:, 0::2, 1::2] + x[:, 1::2, 0::2] + x[:, 1::2, 1::2]) / 4.0)[..., None]


def rows(x, k, stride):
    """im2col: [N, H, W, C] -> ([N Ho Wo, k k C] with columns (ky, kx, c), Ho, Wo); pad (k - 1) / 2 with zeros"""
    N, H, W, C = x.shape
    pad = (k - 1) // 2
    Ho, Wo = (H + 2 * pad - k) // stride + 1, (W + 2 * pad - k) // stride + 1
    xp = F.pad(x, (0, 0, pad, pad, pad, pad))
    cols = [xp[:, ky:ky + stride * (Ho - 1) + 1:stride, kx:kx + stride * (Wo - 1) + 1:stride, :] for ky in range(k) for kx in range(k)]
    return torch.cat(cols, dim=-1).reshape(N * Ho * Wo, k * k * C), Ho, Wo


def conv(x, w, stride):
    """x [N, H, W, Cin], w [Cout, Cin, k, k] (torch's layout) -> [N, Ho, Wo, Cout]"""
    r, Ho, Wo = rows(x, w.shape[2], stride)
    return (r @ w.permute(0, 2, 3, 1).reshape(w.shape[0], -1).T).reshape(x.shape[0], Ho, Wo, w.shape[0])


def group_of(C, G, interleaved=False):
    c = torch.arange(C)
    return c % G if interleaved else c // (C // G)


def gn_stats(x, G, eps=EPS, unbiased=False, interleaved=False):
    """x [N, HW, C] -> (mean [N, G], rstd [N, G]); groups of consecutive channels, biased variance"""
    N, HW, C = x.shape
    gi = group_of(C, G, interleaved)
    mean, rstd = torch.zeros(N, G, dtype=x.dtype), torch.zeros(N, G, dtype=x.dtype)
    for g in range(G):
        v = x[:, :, gi == g].reshape(N, -1)
        mean[:, g] = v.mean(1)
        rstd[:, g] = 1.0 / torch.sqrt(v.var(1, unbiased=unbiased and v.shape[1] > 1) + eps)
    return mean, rstd


def gn_apply(x, mean, rstd, gamma, beta, interleaved=False):
    gi = group_of(x.shape[2], mean.shape[1], interleaved)
    return (x - mean[:, gi][:, None, :]) * rstd[:, gi][:, None, :] * gamma + beta


def gn(x4, gamma, beta, G, mut=None, eps=EPS):
    N, H, W, C = x4.shape
    x = x4.reshape(N, H * W, C)
    il = mut == "groups_interleaved"
    mean, rstd = gn_stats(x, G, 1e-12 if mut == "eps_1e-12" else eps, mut == "unbiased_variance", il)
    return gn_apply(x, mean, rstd, gamma, beta, il).reshape(N, H, W, C)


def maxpool(x):
    """MaxPool2d(3, 2, 1) on [N, H, W, C]; -inf padding"""
    N, H, W, C = x.shape
    Ho, Wo = (H - 1) // 2 + 1, (W - 1) // 2 + 1
    xp = F.pad(x, (0, 0, 1, 1, 1, 1), value=float("-inf"))
    out = None
    for ky in range(3):
        for kx in range(3):
            v = xp[:, ky:ky + 2 * (Ho - 1) + 1:2, kx:kx + 2 * (Wo - 1) + 1:2, :]
            out = v if out is None else torch.maximum(out, v)
    return out


MUTATIONS = ("stride_on_first_1x1", "unbiased_variance", "eps_1e-12", "compression_16_groups", "no_relu_after_residual", "no_avg_pool",
             "groups_interleaved", "nhwc_as_nchw", "views_counter_clockwise")


def forward64(W, depth, base_planes, blocks, mut=None, probes=None):
    """W {name: tensor}, depth [N, S, S, 1] -> [N, Cc, fs, fs] float64 (NCHW, as the module returns it).  probes: a list that receives the
    NHWC activations after the max-pool, after layer1 and after layer4."""
    P = {k: v.to(F64) for k, v in W.items()}
    ng = base_planes // 2
    x = depth.to(F64)
    if mut != "no_avg_pool":
        x = pool2(x)
    x = torch.relu(gn(conv(x, P["backbone.conv1.0.weight"], 2), P["backbone.conv1.1.weight"], P["backbone.conv1.1.bias"], ng, mut))
    x = maxpool(x)
    if probes is not None:
        probes.append(x)
    for l in range(4):
        for i in range(blocks[l]):
            p = f"backbone.layer{l + 1}.{i}."
            stride = 2 if (l > 0 and i == 0) else 1
            s0, s1 = (stride, 1) if mut == "stride_on_first_1x1" else (1, stride)
            a = torch.relu(gn(conv(x, P[p + "convs.0.weight"], s0), P[p + "convs.1.weight"], P[p + "convs.1.bias"], ng, mut))
            b = torch.relu(gn(conv(a, P[p + "convs.3.weight"], s1), P[p + "convs.4.weight"], P[p + "convs.4.bias"], ng, mut))
            c = gn(conv(b, P[p + "convs.6.weight"], 1), P[p + "convs.7.weight"], P[p + "convs.7.bias"], ng, mut)
            idt = x
            if i == 0:
                idt = gn(conv(x, P[p + "downsample.0.weight"], stride), P[p + "downsample.1.weight"], P[p + "downsample.1.bias"], ng, mut)
            x = c + idt
            if mut != "no_relu_after_residual":
                x = torch.relu(x)
        if probes is not None and l in (0, 3):
            probes.append(x)
    y = torch.relu(gn(conv(x, P["compression.0.weight"], 1), P["compression.1.weight"], P["compression.1.bias"],
                      16 if mut == "compression_16_groups" else 1, mut))
    if mut == "nhwc_as_nchw":
        return y.reshape(y.shape[0], y.shape[3], y.shape[1], y.shape[2])
    return y.permute(0, 3, 1, 2).contiguous()


def clockwise(views, mut=None):
    """12 view tensors [B, ...] -> [12 B, ...]: view a of episode b in slot (12 - a) % 12 + 12 b (Policy_ViewSelection_ETP.py:182-190)"""
    B = views[0].shape[0]
    out = torch.zeros(NUM_IMGS * B, *views[0].shape[1:], dtype=views[0].dtype)
    for a, v in enumerate(views):
        out[(a if mut == "views_counter_clockwise" else (NUM_IMGS - a) % NUM_IMGS)::NUM_IMGS] = v
    return out


def module_with(W, image_size, base_planes, blocks, dtype=torch.float32):
    m = ResNetEncoder(image_size, base_planes, blocks).to(dtype).eval()
    m.load_state_dict({k: v.to(dtype) for k, v in W.items()}, strict=True)
    return m


# ---- cases ------------------------------------------------------------------------------------------------------------------------
ENGINE_CASES = ((64, 16, (1, 1, 1, 1)), (64, 32, (2, 1, 1, 1)), (128, 16, (1, 2, 1, 1)))     # the second has a block without downsample
ENGINE_NS = (1, 3, 13)
ENGINE_N_MAX = 13
# image size 192: 3 x 3 output maps, Cc = round(2048 / 9) = 228 (no multiple of 8: the GEMM's scalar epilogue), 6 x 6 stem tiles
CASE_192, CASE_192_N = (192, 16, (1, 1, 1, 1)), 3
FULL_N = 2                      # the full network once at N = 2 (images 0, 1) and at N = 12 through encode_views (images 0 .. 11 as views)
ALL_CASES = ENGINE_CASES + (FULL, CASE_192)       # fixture order: case_0 .. case_4
ALL_CASE_N = (ENGINE_N_MAX,) * 3 + (NUM_IMGS, CASE_192_N)
STEM_S, STEM_BP, STEM_N, STEM_B = (64, 128, 192), (16, 32), (1, 3, 13), (1, 3)
ROWS_HW, ROWS_C, ROWS_KS, ROWS_N = (1, 2, 4, 7, 32), (16, 32, 64, 256), ((1, 1), (1, 2), (3, 1), (3, 2)), (1, 3)
GN_HW, GN_C, GN_G, GN_N = (1, 16, 49, 1024, 4096), (16, 32, 128, 1024), (1, 8, 16), (1, 3, 13)


def gn_cases():
    """the full cross product (HW, C, G, N) of GN_HW x GN_C x GN_G x GN_N; where HW C >= 2^20 (a float64 reference of 13 such images is
    large) N = 13 is left out, so those tensors run at N = 1 and 3: 174 of the 180 cases"""
    return [(HW, C, G, N) for HW in GN_HW for C in GN_C for G in GN_G for N in GN_N if not (HW * C >= 1 << 20 and N == 13)]


# ---- schedules and bounds ------------------------------------------------------------------------------------------------------------
def gam(k):
    return rr.gam(k)


def stem_bound(depth64, w64):
    """elementwise bound of the stem's pre-norm output [N, S/4, S/4, bp]"""
    return gam(52) * conv(pool2(depth64).abs(), w64.abs(), 2)


def f32(v):
    return np.asarray(v, dtype=np.float32)


def emulate_stem(depth, w):
    """depth_stem_kernel in fp32 numpy: pooled = ((a + b) + (c + d)) * 0.25, then the 49 taps in (ky, kx) order, acc = fma(x, w, acc)
    (the product is exact in float64; the sum is rounded to fp32)."""
    x = depth[..., 0].numpy().astype(np.float32)
    pooled = f32(f32(f32(x[:, 0::2, 0::2] + x[:, 0::2, 1::2]) + f32(x[:, 1::2, 0::2] + x[:, 1::2, 1::2])) * np.float32(0.25))
    N, P, _ = pooled.shape
    Ho = P // 2
    xp = np.zeros((N, P + 6, P + 6), np.float32)
    xp[:, 3:3 + P, 3:3 + P] = pooled
    wn = w.numpy().astype(np.float32)
    acc = np.zeros((N, Ho, Ho, wn.shape[0]), np.float32)
    for ky in range(7):
        for kx in range(7):
            v = xp[:, ky:ky + 2 * (Ho - 1) + 1:2, kx:kx + 2 * (Ho - 1) + 1:2]
            acc = f32(v[..., None].astype(np.float64) * wn[:, 0, ky, kx].astype(np.float64) + acc.astype(np.float64))
    return torch.from_numpy(acc)


GN_THREADS = 1024              # depth.hip GN_NT


def stats_schedule(HW, C, G):
    """[(q0, Qc, R)] of gn_stats_kernel's channel chunks"""
    Q = C // 4
    return [(q0, min(GN_THREADS, Q - q0), GN_THREADS // min(GN_THREADS, Q - q0)) for q0 in range(0, Q, GN_THREADS)]


def stats_depth(HW, C, G):
    cg = C // G
    return max(-(-HW // R) + R for _, _, R in stats_schedule(HW, C, G)) + -(-cg // 64) + 6


def _group_sums(v, HW, C, G):
    """v [HW, C] fp32 -> [G] fp32 on gn_stats_kernel's schedule"""
    cg = C // G
    chs = np.zeros(C, np.float32)
    for q0, Qc, R in stats_schedule(HW, C, G):
        c0, c1 = q0 * 4, (q0 + Qc) * 4
        part = np.zeros((R, c1 - c0), np.float32)
        for j in range(-(-HW // R)):
            blk = v[j * R:(j + 1) * R, c0:c1]
            part[:blk.shape[0]] = f32(part[:blk.shape[0]] + blk)
        s = np.zeros(c1 - c0, np.float32)
        for r in range(R):
            s = f32(s + part[r])
        chs[c0:c1] = s
    out = np.zeros(G, np.float32)
    for g in range(G):
        lanes = np.zeros(64, np.float32)
        for j in range(-(-cg // 64)):
            blk = chs[g * cg + j * 64:min(g * cg + (j + 1) * 64, (g + 1) * cg)]
            lanes[:blk.shape[0]] = f32(lanes[:blk.shape[0]] + blk)
        for o in (32, 16, 8, 4, 2, 1):
            lanes = f32(lanes + lanes[np.arange(64) ^ o])
        out[g] = lanes[0]
    return out


def emulate_stats(x, G, eps=EPS, one_pass=False):
    """gn_stats_kernel in fp32 numpy -> [N, G, 2].  one_pass: the rejected E[x^2] - E[x]^2 form on the same summation schedule."""
    N, HW, C = x.shape
    cg = C // G
    n = np.float32(HW * cg)
    xn = x.numpy().astype(np.float32)
    gi = np.arange(C) // cg
    out = np.zeros((N, G, 2), np.float32)
    for i in range(N):
        if one_pass:
            m = f32(_group_sums(xn[i], HW, C, G) / n)
            var = f32(f32(_group_sums(f32(xn[i] * xn[i]), HW, C, G) / n) - f32(m * m))
        else:
            piv = xn[i, 0, np.arange(G) * cg]
            m = f32(piv + f32(_group_sums(f32(xn[i] - piv[gi]), HW, C, G) / n))
            d = f32(xn[i] - m[gi])
            var = f32(_group_sums(f32(d * d), HW, C, G) / n)
        out[i, :, 0] = m
        with np.errstate(invalid="ignore", divide="ignore"):
            out[i, :, 1] = f32(np.float32(1.0) / np.sqrt(f32(var + np.float32(eps))))
    return torch.from_numpy(out)


def stats_bounds(x64, G, eps=EPS):
    """-> (mean [N, G], rstd [N, G], mean bound, rstd bound) in float64 for x [N, HW, C]"""
    N, HW, C = x64.shape
    cg = C // G
    k = stats_depth(HW, C, G)
    mean, rstd = gn_stats(x64, G, eps)
    xg = x64.reshape(N, HW, G, cg)
    D = (xg - xg[:, :1, :, :1]).abs().mean(dim=(1, 3))
    var = xg.var(dim=(1, 3), unbiased=False)
    dm = gam(k + 2) * D + U * mean.abs()
    dv = gam(k + 4) * (var + dm ** 2) + 2 * dm * var.sqrt() + dm ** 2
    lo = (var + eps - dv).clamp_min(1e-300)
    dr = dv / (2.0 * lo ** 1.5) + 3 * U * rstd
    return mean, rstd, dm, dr


def apply_ref(x64, stats64, gamma64, beta64):
    """-> (y, bound): GroupNorm of x [N, HW, C] with GIVEN statistics [N, G, 2], and gam(4) (|x - m| r |g| + |b|)"""
    gi = group_of(x64.shape[2], stats64.shape[1])
    m, r = stats64[:, gi, 0][:, None, :], stats64[:, gi, 1][:, None, :]
    y = (x64 - m) * r * gamma64 + beta64
    return y, gam(4) * ((x64 - m).abs() * r * gamma64.abs() + beta64.abs())
