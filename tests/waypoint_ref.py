"""fp64 restatement of the waypoint head (etpnav_amd/waypoint.py, csrc/waypoint.hip, csrc/waypoint_engine.hip) with derived error
bounds, the weight generator, and the cases the CPU and GPU tests share.

Written from the description of what the reference computes (vlnce_baselines/waypoint_pred/TRM_net.py:62-88,
waypoint_pred/transformer/waypoint_bert.py, waypoint_pred/utils.py:8-64,90-102, models/Policy_ViewSelection_ETP.py:172-342);
tests/test_waypoint_ref_cpu.py pins it to the real classes where the reference tree is present and to tests/golden/waypoint_small.npz
everywhere.

  head_ref(W, depth)                 logits [B,120,12], rolled by HEATMAP_OFFSET
  ring_attn_ref(q, k, v, n, alpha)   (ctx, bound) of etp_ring_attn_fwd
  tail_ref(logits, max_pred, ...)    heat, nms map, candidate table, samples, pick margins of etp_waypoint_tail
  heat_bound(logits)                 elementwise bound of heat / the non-zero nms values

`mut=` switches ONE deliberate error on (MUTATIONS); the CPU test shows that each is rejected.

Bounds (first-order propagation of the kernels' documented rounding points, u = 2^-24; no fitted multiplier):

 ring attention (waypoint.hip ring_attn_fwd_kernel; operands are exact bf16 / fp32 values, products are FMAs)
   E_s  = alpha 18 u sum_d |q_d k_d| + u |s|       16 chained FMAs + 2 butterfly additions, then the multiply by alpha
   E_t  = E_s(j) + max_k E_s(k) + u |s_j - m|      the subtraction of the row maximum
   r_j  = E_t + EXPF_REL                           expf: within one ulp = 2u relative (the HIP math API's table for expf; the same
                                                   figure reduce_ref.py uses)
   E_l / l = sum_j P_j r_j + 2n u                  l: 2n serial additions
   E_acc / l = sum_j P_j |v_jd| (r_j + (2n+1) u)   2n+1 chained FMAs
   E_ctx = E_acc / l + |ctx| (E_l / l + u) + U |ctx| + 2^-126     the division; the store (U = 2^-8 in bf16 mode, the project's
                                                   unit for a bf16 store, 0 in fp32 mode); the flush-to-zero floor
 heat map (waypoint_tail_kernel)
   r_k  = u |l_k - m| + EXPF_REL                   e_k = expf(l_k - m)
   E_heat = heat_k (r_k + sum_j heat_j r_j + 14 u + u) + 2^-126
                                                   the 1 440-term sum's longest addition chain is 14 (5 per thread + 6 butterfly
                                                   steps + 3 across the four waves); the division
"""
import numpy as np
import torch

F64 = torch.float64
U32 = 2.0 ** -24
U_BF16 = 2.0 ** -8
EXPF_REL = 2.0 * U32          # expf: <= 1 ulp
SUM_CHAIN = 14
FTZ = 2.0 ** -126
H, I, HEADS, TOK, ANG, DST = 768, 3072, 12, 12, 120, 12
OFFSET = 5
MUTATIONS = ("intdiv", "noncircular", "nowrap", "roll", "last", "pointer", "window")

# worst |got - ref| / bound per key (the GPU test writes them to profiles/waypoint_op_bounds.txt)
WORST = {}


# ---- parameters ------------------------------------------------------------------------------------------------------------------
def param_shapes():
    """[(state-dict key, shape)] in the reference module's order (TRM_net.py:27-60): 42 tensors, 17 614 200 parameters."""
    out = [("visual_fc_depth.1.weight", (H, 2048)), ("visual_fc_depth.1.bias", (H,)),
           ("visual_merge.0.weight", (H, 2 * H)), ("visual_merge.0.bias", (H,))]
    for l in range(2):
        p = f"waypoint_TRM.bert.encoder.layer.{l}."
        for n in ("query", "key", "value"):
            out += [(p + f"attention.self.{n}.weight", (H, H)), (p + f"attention.self.{n}.bias", (H,))]
        out += [(p + "attention.output.dense.weight", (H, H)), (p + "attention.output.dense.bias", (H,)),
                (p + "attention.output.LayerNorm.weight", (H,)), (p + "attention.output.LayerNorm.bias", (H,)),
                (p + "intermediate.dense.weight", (I, H)), (p + "intermediate.dense.bias", (I,)),
                (p + "output.dense.weight", (H, I)), (p + "output.dense.bias", (H,)),
                (p + "output.LayerNorm.weight", (H,)), (p + "output.LayerNorm.bias", (H,))]
    out += [("mergefeats_LayerNorm.weight", (H,)), ("mergefeats_LayerNorm.bias", (H,)),
            ("vis_classifier.0.weight", (H, H)), ("vis_classifier.0.bias", (H,)),
            ("vis_classifier.2.weight", (ANG * DST // TOK, H)), ("vis_classifier.2.bias", (ANG * DST // TOK,))]
    return out


CLS_SCALE = 2.0      # scale of vis_classifier.2.weight: random weights give a nearly flat heat map (logit std 0.77); this gives 1.5


def make_weights(seed, cls_scale=CLS_SCALE):
    """{key: fp32 tensor}: a numpy default_rng fill.  Matrices N(0, 1) * row_scale / sqrt(fan_in), row scales uniform in [0.5, 1.5];
    biases N(0, 0.1); LayerNorm weights 1 + N(0, 0.1), biases N(0, 0.1)."""
    rng = np.random.default_rng(seed)
    W = {}
    for name, shape in param_shapes():
        if len(shape) == 2:
            w = rng.standard_normal(shape) * (rng.uniform(0.5, 1.5, (shape[0], 1)) / np.sqrt(shape[1]))
            if name == "vis_classifier.2.weight":
                w = w * cls_scale
        elif "LayerNorm.weight" in name:
            w = 1.0 + 0.1 * rng.standard_normal(shape)
        else:
            w = 0.1 * rng.standard_normal(shape)
        W[name] = torch.from_numpy(w.astype(np.float32))
    return W


def fingerprint(W):
    """{key: (sum, abs-max, L2)} in fp64: the golden file stores this instead of the weights"""
    return {k: (float(v.double().sum()), float(v.double().abs().max()), float(v.double().norm())) for k, v in W.items()}


# ---- head ----------------------------------------------------------------------------------------------------------------------------
def ring_mask(n):
    """[12,12] 0/1: token i sees i-n .. i+n (mod 12)"""
    m = np.zeros((TOK, TOK), dtype=np.int64)
    for i in range(TOK):
        for o in range(-n, n + 1):
            m[i, (i + o) % TOK] = 1
    return m


def ring_attn_vals(q, k, v, n, alpha):
    """q / k / v [B, heads, 12, 64] fp64 -> (ctx, P [.., 12, 2n+1], s, gathered k, gathered v)"""
    idx = torch.tensor([[(i + o) % TOK for o in range(-n, n + 1)] for i in range(TOK)], device=q.device)   # [12, 2n+1]
    kg, vg = k[:, :, idx], v[:, :, idx]                                  # [B, h, 12, 2n+1, 64]
    s = alpha * (q[:, :, :, None, :] * kg).sum(-1)
    P = torch.softmax(s, -1)
    return (P[..., None] * vg).sum(-2), P, s, kg, vg


def ring_attn_ref(q, k, v, n, alpha, bf16):
    """-> (ctx, E_ctx) per the module docstring; q / k / v hold the STORED operand values"""
    q, k, v = (t.detach().to(F64) for t in (q, k, v))
    ctx, P, s, kg, vg = ring_attn_vals(q, k, v, n, alpha)
    E_s = alpha * 18 * U32 * (q[:, :, :, None, :].abs() * kg.abs()).sum(-1) + U32 * s.abs()
    t = s - s.amax(-1, keepdim=True)
    r = E_s + E_s.amax(-1, keepdim=True) + U32 * t.abs() + EXPF_REL
    El = (P * r).sum(-1, keepdim=True) + 2 * n * U32
    Eacc = ((P * (r + (2 * n + 1) * U32))[..., None] * vg.abs()).sum(-2)
    E = Eacc + ctx.abs() * (El + U32) + (U_BF16 if bf16 else 0.0) * ctx.abs() + FTZ
    return ctx, E


def _ln(x, g, b):
    u = x.mean(-1, keepdim=True)
    s = ((x - u) ** 2).mean(-1, keepdim=True)
    return g * ((x - u) / torch.sqrt(s + 1e-12)) + b


def _gelu(x):
    return x * 0.5 * (1.0 + torch.erf(x / np.sqrt(2.0)))


def head_ref(W, depth, neighbor=1, mut=None, return_raw=False, dtype=F64):
    """W {key: tensor}, depth [12B, 2048] (or [12B,128,4,4]) -> logits [B,120,12] fp64, rolled.  (dtype=torch.float32 on tensors that
    already live on a GPU: the eager baseline of tools/waypoint_bench.py.)"""
    W = {k: v.detach().to(dtype) for k, v in W.items()}
    lin = lambda x, n: x @ W[n + ".weight"].T + W[n + ".bias"]
    d = depth.detach().to(dtype).reshape(depth.shape[0], -1)
    B = d.shape[0] // TOK
    x = torch.relu(lin(d, "visual_fc_depth.1"))
    n = neighbor + (1 if mut == "window" else 0)
    for l in range(2):
        p = f"waypoint_TRM.bert.encoder.layer.{l}."
        sp = lambda t: t.reshape(B, TOK, HEADS, 64).permute(0, 2, 1, 3)
        q, k, v = (sp(lin(x, p + f"attention.self.{nm}")) for nm in ("query", "key", "value"))
        ctx = ring_attn_vals(q, k, v, n, 0.125)[0].permute(0, 2, 1, 3).reshape(B * TOK, H)
        a = _ln(lin(ctx, p + "attention.output.dense") + x, W[p + "attention.output.LayerNorm.weight"],
                W[p + "attention.output.LayerNorm.bias"])
        x = _ln(lin(_gelu(lin(a, p + "intermediate.dense")), p + "output.dense") + a, W[p + "output.LayerNorm.weight"],
                W[p + "output.LayerNorm.bias"])
    raw = lin(torch.relu(lin(x, "vis_classifier.0")), "vis_classifier.2").reshape(B, ANG, DST)
    if return_raw:
        return raw
    if mut == "roll":
        return torch.cat((raw[:, -OFFSET:], raw[:, :-OFFSET]), 1)
    return torch.cat((raw[:, OFFSET:], raw[:, :OFFSET]), 1)


# ---- tail ----------------------------------------------------------------------------------------------------------------------------
def _softmax64(x):
    e = np.exp(x - x.max())
    return e / e.sum()


def regional_probs(logits_ep, sector):
    """softmax over the 10 x 12 logits of image sector `sector`, taken from the logits rolled back by 5"""
    back = np.concatenate((logits_ep[-OFFSET:], logits_ep[:-OFFSET]), 0).reshape(12, 10 * DST)
    return _softmax64(back[sector])


def tail_ref(logits, max_pred=5, sigma=(7.0, 5.0), uniforms=None, mut=None):
    """logits [B,120,12] -> dict of numpy arrays: heat, nms_map [B,120,12] fp64; count [B]; angle, dist, img_cw, img_ccw, samp_angle,
    samp_dist [B,max_pred] int (-1 beyond the count; samp_* only with uniforms); margins: per episode the list of
    log(pick) - log(best other cell) of the picks with a positive value (cells exactly equal to the pick -- its wrap copy, a cell with
    the same logit -- do not count: they are equal bit for bit in every precision and the lower index wins)."""
    L = np.asarray(torch.as_tensor(logits).detach().to(F64).cpu().numpy(), dtype=np.float64)
    B = L.shape[0]
    out = dict(heat=np.zeros((B, ANG, DST)), nms_map=np.zeros((B, ANG, DST)), count=np.zeros(B, dtype=np.int64), margins=[])
    for nm in ("angle", "dist", "img_cw", "img_ccw", "samp_angle", "samp_dist"):
        out[nm] = np.full((B, max_pred), -1, dtype=np.int64)
    for b in range(B):
        p = _softmax64(L[b].ravel()).reshape(ANG, DST)
        out["heat"][b] = p
        wrap = p.copy() if mut == "nowrap" else np.concatenate((p[-1:], p, p[:1]), 0)
        rows = wrap.shape[0]
        supp, res = wrap.copy(), np.zeros_like(wrap)
        margins = []
        ys, xs = np.arange(rows, dtype=np.float64)[:, None], np.arange(DST, dtype=np.float64)[None, :]
        for _ in range(max_pred):
            flat = supp.ravel()
            ix = int(np.argmax(flat)) if mut != "last" else int(len(flat) - 1 - np.argmax(flat[::-1]))
            res.flat[ix] = wrap.flat[ix]
            if flat[ix] > 0:
                other = supp.copy()
                other[other == flat[ix]] = 0.0          # exact ties (wrap copies, equal logits): the index decides in any precision
                second = other.max()
                margins.append(np.log(flat[ix]) - np.log(second) if second > 0 else np.inf)
            y_mu = (ix // DST) if mut == "intdiv" else ix / DST
            x_mu = ix % DST
            xd = xs - x_mu
            xd = np.abs(xd) if mut == "noncircular" else np.minimum(np.abs(xd), np.abs(xd + DST))
            g = (np.abs(xd) <= sigma[0]) & (np.abs(ys - y_mu) <= sigma[1])
            supp = supp * (1.0 - g)
        res[res < 0] = 0
        res = res if mut == "nowrap" else res[1:-1]
        out["nms_map"][b] = res
        out["margins"].append(margins)
        a, d = np.nonzero(res)
        n = len(a)
        out["count"][b] = n
        out["angle"][b, :n], out["dist"][b, :n] = a, d
        out["img_cw"][b, :n] = ((a + 5) // 10) % 12
        out["img_ccw"][b, :n] = (12 - (a + 5) // 10) % 12
        if uniforms is not None:
            for c in range(n):
                sec = int(out["img_cw"][b, c])
                cdf = np.cumsum(regional_probs(L[b], sec))
                act = min(int(np.searchsorted(cdf, float(uniforms[b][c]) * cdf[-1], side="right")), 10 * DST - 1)
                pointer = ((sec - 1) * 10 + (0 if mut == "pointer" else 5)) if sec != 0 else 0
                out["samp_angle"][b, c] = act // DST + pointer
                out["samp_dist"][b, c] = act % DST
    return out


def heat_bound(logits):
    """elementwise bound of heat (module docstring) -> numpy [B,120,12]"""
    L = np.asarray(torch.as_tensor(logits).detach().to(F64).cpu().numpy(), dtype=np.float64)
    B = L.shape[0]
    E = np.zeros_like(L)
    for b in range(B):
        l = L[b].ravel()
        heat = _softmax64(l)
        t = np.where(np.isfinite(l), np.abs(l - l.max()), 0.0)       # a -inf logit gives an exact 0
        r = U32 * t + EXPF_REL
        E[b] = (heat * (r + (heat * r).sum() + (SUM_CHAIN + 1) * U32) + FTZ).reshape(ANG, DST)
    return E


def make_uniforms(logits, max_pred, seed):
    """[B,max_pred] fp32: for every candidate of tail_ref(logits) the MIDPOINT of the CDF interval of a regional cell with probability
    >= 1e-3, drawn with default_rng(seed); 0.5 in the unused slots."""
    rng = np.random.default_rng(seed)
    t = tail_ref(logits, max_pred)
    L = np.asarray(torch.as_tensor(logits).detach().to(F64).cpu().numpy())
    u = np.full((L.shape[0], max_pred), 0.5, dtype=np.float32)
    for b in range(L.shape[0]):
        for c in range(int(t["count"][b])):
            pr = regional_probs(L[b], int(t["img_cw"][b, c]))
            k = int(rng.choice(np.nonzero(pr >= 1e-3)[0]))
            cdf = np.concatenate(([0.0], np.cumsum(pr)))
            u[b, c] = 0.5 * (cdf[k] + cdf[k + 1]) / cdf[-1]
    return u


def check_conditions(logits, max_pred, uniforms=None, margin=1e-4, name=""):
    """The conditions the GPU comparison rests on, asserted on the fp64 reference alone: every pick with a positive value exceeds the
    best other cell by `margin` in logit; every uniform sits within its cell's CDF interval at least 5e-4 from both edges (the midpoint
    of a cell with regional probability >= 1e-3)."""
    t = tail_ref(logits, max_pred, uniforms=uniforms)
    worst = min([m for ms in t["margins"] for m in ms] + [np.inf])
    assert worst >= margin, f"{name}: a pick leads the next cell by only {worst:.3g} in logit"
    if uniforms is not None:
        L = np.asarray(torch.as_tensor(logits).detach().to(F64).cpu().numpy())
        for b in range(L.shape[0]):
            for c in range(int(t["count"][b])):
                cdf = np.concatenate(([0.0], np.cumsum(regional_probs(L[b], int(t["img_cw"][b, c])))))
                uu = float(uniforms[b][c]) * cdf[-1]
                k = int(np.searchsorted(cdf[1:], uu, side="right"))
                assert min(uu - cdf[k], cdf[k + 1] - uu) >= 5e-4 - 1e-7, f"{name}: uniform [{b},{c}] sits {min(uu - cdf[k], cdf[k + 1] - uu):.3g} from a CDF edge"
    return t


# ---- cases the CPU and GPU tests share ---------------------------------------------------------------------------------------------
ATTN_B = (1, 2, 5, 33)          # 12, 24, 60 and 396 rows
ATTN_N = (0, 1, 5)
TAIL_RANDOM = [(B, mp) for B in (1, 3, 17) for mp in (1, 5, 8)]
TAIL_SEED = 11
CRAFTED = ("angle0", "angle119", "dist_ends", "five_apart_d0", "five_apart_d2", "few_survive", "inf_column", "tie")
GOLDEN_SEED, GOLDEN_B = 3, 3
# The fixture's episodes, chosen on the CPU out of a pool of 2048 random ones: scaling vis_classifier.2.weight scales the pick margins
# and the bf16 gap of the reference alike, so no scale makes random episodes pass "every pick leads by 4 x the bf16 autocast gap";
# about one episode in 400 does (tools/make_golden_waypoint.py asserts it for these three).
GOLDEN_POOL, GOLDEN_EPISODES = 2048, (1064, 1243, 707)


def attn_case(B, n, bf16, seed=0):
    """q, k, v [B, heads, 12, 64] fp32 holding the stored values: standard normal; the last query of the last episode scaled by 8
    (|s| ~ 60), in episode 0 the key of token 3 equal to 3 x query 2 (a row maximum far above the rest)."""
    g = torch.Generator().manual_seed(100 * seed + 7 * B + n)
    q, k, v = (torch.randn(B, HEADS, TOK, 64, generator=g) for _ in range(3))
    k[0, :, 3] = 3.0 * q[0, :, 2]
    q[B - 1, :, TOK - 1] *= 8.0
    if bf16:
        q, k, v = (t.bfloat16().float() for t in (q, k, v))
    return q, k, v


def tail_random(B, max_pred, seed=TAIL_SEED):
    """random logits scaled so that the softmax has clear peaks: N(0, 3)"""
    rng = np.random.default_rng(1000 * seed + 10 * B + max_pred)
    return (3.0 * rng.standard_normal((B, ANG, DST))).astype(np.float32)


def tail_crafted(kind, seed=TAIL_SEED):
    """one episode [1,120,12] fp32: a low random background (N(0, 0.3) - 6) with peaks set by hand"""
    rng = np.random.default_rng(seed + 17 * CRAFTED.index(kind))
    L = (0.3 * rng.standard_normal((ANG, DST)) - 6.0)
    if kind == "angle0":            # the global peak at angle 0: wrapped rows 1 and 121 hold it, the second pick is lost with row 121
        L[0, 3] = 4.0; L[40, 5] = 3.0; L[80, 9] = 2.0
    elif kind == "angle119":        # rows 120 and 0
        L[119, 6] = 4.0; L[30, 2] = 3.0; L[75, 10] = 2.0
    elif kind == "dist_ends":       # the two ends of the circular distance rule
        L[20, 0] = 4.0; L[20, 8] = 3.5; L[20, 7] = 3.0; L[60, 11] = 2.5; L[60, 3] = 2.0; L[62, 0] = 1.5
    elif kind == "five_apart_d0":   # d = 0: rows a-5 .. a+5 go, the second peak with them
        L[50, 0] = 4.0; L[45, 1] = 3.0
    elif kind == "five_apart_d2":   # d > 0: rows a-4 .. a+5 go, the second peak five rows up survives
        L[50, 2] = 4.0; L[45, 1] = 3.0
    elif kind == "few_survive":     # three finite cells: the later rounds find an all-zero map and pick wrap cell 0
        L[:] = -np.inf
        L[10, 2] = 1.0; L[55, 6] = 0.5; L[100, 9] = 0.0
    elif kind == "inf_column":
        L = 3.0 * rng.standard_normal((ANG, DST))
        L[:, 5] = -np.inf
    elif kind == "tie":             # two exactly equal logits two rows apart: the lower flat index is picked and suppresses the other
        L[70, 3] = 4.0; L[72, 3] = 4.0; L[20, 9] = 2.0
    return L[None].astype(np.float32)


def golden_depth(seed=GOLDEN_SEED, episodes=GOLDEN_EPISODES):
    """depth embeddings [12B, 2048] of the fixture, clockwise view order: |N(0,1)| values exact in fp16 (the depth encoder ends in a
    ReLU), the episodes `episodes` of a pool of GOLDEN_POOL"""
    rng = np.random.default_rng(500 + seed)
    pool = np.abs(rng.standard_normal((TOK * GOLDEN_POOL, 2048))).astype(np.float16).astype(np.float32).reshape(GOLDEN_POOL, TOK, 2048)
    return torch.from_numpy(np.ascontiguousarray(pool[list(episodes)]).reshape(-1, 2048))


def record(key, got, ref, E, name=""):
    """every element finite and |got - ref| <= E; the worst ratio goes to WORST[key]"""
    got, ref, E = (np.asarray(t, dtype=np.float64) for t in (got, ref, E))
    assert got.shape == ref.shape, (name, got.shape, ref.shape)
    assert np.isfinite(got).all(), f"{name}: non-finite elements"
    ratio = np.abs(got - ref) / E
    worst = float(ratio.max()) if ratio.size else 0.0
    if worst > WORST.get(key, (0.0, ""))[0]:
        WORST[key] = (worst, name)
    if worst > 1.0:
        i = int(ratio.argmax())
        raise AssertionError(f"{name}: |got - ref| = {worst:.3g} x the bound at {np.unravel_index(i, ratio.shape)} "
                             f"(got {got.ravel()[i]:.8g}, ref {ref.ravel()[i]:.8g}, bound {E.ravel()[i]:.3g}); "
                             f"{int((ratio > 1).sum())} of {ratio.size} elements beyond it")
    return worst
