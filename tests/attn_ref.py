"""fp64 restatement of the attention operator (etp_attn_fwd / etp_attn_bwd, include/etpnav_hip.h) with a propagated error bound,
the comparator and the case generator of its op-level tests (tests/test_attn_kernels_gpu.py).

tests/test_attn_ref_cpu.py pins the values to oracle/planner_oracle.py's `bert_attention_core`; tests/test_attn_bounds_cpu.py shows
that CPU emulations of every kernel family's rounding schedule stay inside the bound and that the comparator can fail.

  attn_ref(q, k, v, keymask, mask_mode, dist, sp_w, sp_b, alpha, dctx, bf16=, gemm=) -> (values, bounds)
      q [B, heads, Lq, 64], k / v [B, heads, Lk, 64], dctx like q: the STORED operands (bf16 or fp32 values, converted exactly);
      keymask [B, Lk] bool or None; dist [B, Lq, Lk] or None.  values / bounds: dicts over ctx, dQ, dK, dV, d_sp_w, d_sp_b.

      s = alpha q.k^T + (keymask term + (sp_w dist + sp_b))    keymask term: mode 0 (1 - m) * -10000, mode 1 -inf where !m
      P = softmax(s)   ctx = P V   dP = dO V^T   D = rowsum(P dP)   dS = P (dP - D)
      dQ = alpha dS K   dK = alpha dS^T Q   dV = P^T dO   d_sp_w = sum dS dist   d_sp_b = sum dS

The bound is not a measured number: it is the first-order propagation of the rounding points the kernels document, with
u = 2^-8 (unit roundoff of bf16) in bf16 mode and u = 0 in fp32 mode.  Each line names what it models:

  E_ctx = u (P |V| + |ctx|) + E_P |V|        P rounded to bf16 before P.V (attn_rows.hip rows_fwd_kernel: the P strip; attn.hip
                                             attn_fwd_kernel: the stored P tile; flash_fwd_kernel: exp(s - m_run) per tile;
                                             norm.hip softmax_fwd_kernel's store), ctx rounded at its store
  E_dV  = u (P^T |dO| + |dV|) + E_P^T |dO|   the same rounded P (recomputed from lse in attn_rows.hip rows_bwd_kernel and
                                             attn.hip flash_bwd_dkv_kernel), dV rounded at its store
  E_D   = sum_d |dO| E_ctx                   D = rowsum(dO * O) from the ROUNDED ctx (attn.hip flash_bwd_dq_kernel); the other
                                             families form D = rowsum(P dP), whose error is smaller
  E_dS  = u |dS| + P E_D + E_P |dP - D|      dS rounded to bf16 before dS.K / dS^T.Q (every backward kernel; norm.hip
         + P (E_dP + sum_j P_j E_dP_j)       softmax_bwd_kernel's store); E_dP: see below
  E_dQ  = alpha E_dS |K| + u |dQ|            dQ rounded at its store
  E_dK  = alpha E_dS^T |Q| + u |dK|          dK rounded at its store
  E_dw  = sum E_dS |dist|,  E_db = sum E_dS  the bias gradients are sums of the same dS (fp32 atomics, one per workgroup)
  ctx, dQ, dK, dV: + FP32_REL max(1, max|ref|)   accumulation order, __expf, v_rcp (row_ref.py's fp32 class)
  d_sp_w: + FP32_REL max(1, sum |dS| |dist|)    the two scalars are fp32 running sums over ALL B * heads * Lq * Lk elements of dS
  d_sp_b: + FP32_REL max(1, sum |dS|)           (norm.hip softmax_bwd_kernel `aw += ds * d[k]; ab += ds`, attn.hip attn_bwd_kernel and
                                             attn_rows.hip rows_bwd_kernel likewise) followed by one atomicAdd per workgroup.  Every
                                             row of dS sums to zero, so d_sp_b is 0 in exact arithmetic and max|ref| says nothing about
                                             what was accumulated: the fp32 class is taken relative to the sum of the magnitudes
                                             instead.  FP32_REL = 335 * 2^-24 covers addition chains of up to 335 roundings, each
                                             at most 2^-24 of the magnitudes summed so far.  (Found on the MI355X: with max|ref| the
                                             fp32 batched-GEMM path at 97 x 64, B = 23 x 12 -- 1.7 M terms -- ended 1.2e-4 from a
                                             reference of -4e-5 and a bound of 2e-5; sum |dS| there is about 5e4.)

E_P = 2 max_k E_s[q, k] P is the effect of a score error E_s (dP / P <= 2 max E_s).  E_s is zero except
  * gemm=True, bf16 (the batched-GEMM path): alpha Q.K^T is stored in bf16 before softmax_fwd adds mask and bias in fp32
    (planner.hip attn_fwd_impl, "S = alpha * Q K^T") -> E_s = u |alpha q.k|, and dP = dO V^T is stored in bf16 before softmax_bwd reads
    it (attn_bwd_impl, "dP = dctx V^T") -> E_dP = u |dP|.  With a query scaled to |s| ~ 60 the bound of that family is loose on that row:
    that is what the family computes;
  * a row whose keys are ALL invalid under mask_mode 0: every kernel adds -10000 in fp32, whose ulp there is 2^-10 -> E_s = 2^-11 per
    fp32 addition at that magnitude (attn_rows.hip key_term + the score; a second one with the distance bias).  Both dtypes.
"""
import torch

F64 = torch.float64
U_BF16 = 2.0 ** -8
FP32_REL = 2e-5           # tests/row_ref.py FP32_REL
NAMES = ("ctx", "dQ", "dK", "dV", "d_sp_w", "d_sp_b")

# worst |got - ref| / E seen per key (the GPU tests use "<family cell>/<tensor>")
WORST = {}


def attn_ref(q, k, v, keymask, mask_mode, dist, sp_w, sp_b, alpha, dctx, bf16=True, gemm=False):
    q, k, v, do = (t.detach().to(F64) for t in (q, k, v, dctx))
    B, nh, Lq, _ = q.shape
    u = U_BF16 if bf16 else 0.0
    s0 = alpha * (q @ k.transpose(-1, -2))
    add = torch.zeros(B, 1, 1, k.shape[2], dtype=F64, device=q.device)
    if keymask is not None:
        neg = float("-inf") if mask_mode else -10000.0
        add = torch.where(keymask, 0.0, neg).to(F64)[:, None, None, :]
    n_add = 1
    if dist is not None:
        dist = dist.detach().to(F64)
        add = add + (dist * float(sp_w) + float(sp_b))[:, None]
        n_add = 2
    P = torch.softmax(s0 + add, -1)
    ctx = P @ v
    dP = do @ v.transpose(-1, -2)
    D = (P * dP).sum(-1, keepdim=True)
    dS = P * (dP - D)
    dQ = alpha * (dS @ k)
    dK = alpha * (dS.transpose(-1, -2) @ q)
    dV = P.transpose(-1, -2) @ do
    val = {"ctx": ctx, "dQ": dQ, "dK": dK, "dV": dV}
    if dist is not None:
        val["d_sp_w"] = (dS.sum(1) * dist).sum()
        val["d_sp_b"] = dS.sum()

    # score error: zero except in the two situations of the docstring
    Es = torch.zeros(B, nh, Lq, 1, dtype=F64, device=q.device)
    E_dP = torch.zeros_like(dP)
    if gemm and bf16:
        Es = Es + u * s0.abs().amax(-1, keepdim=True)
        E_dP = u * dP.abs()
    if keymask is not None and not mask_mode:
        none_valid = ~keymask.any(-1)
        Es = Es + n_add * 2.0 ** -11 * none_valid.to(F64)[:, None, None, None]
    E_P = 2.0 * Es * P
    E_ctx = u * (P @ v.abs() + ctx.abs()) + E_P @ v.abs()
    E_dV = u * (P.transpose(-1, -2) @ do.abs() + dV.abs()) + E_P.transpose(-1, -2) @ do.abs()
    E_D = (do.abs() * E_ctx).sum(-1, keepdim=True)
    E_dS = u * dS.abs() + P * E_D + E_P * (dP - D).abs() + P * (E_dP + (P * E_dP).sum(-1, keepdim=True))
    E_dQ = alpha * (E_dS @ k.abs()) + u * dQ.abs()
    E_dK = alpha * (E_dS.transpose(-1, -2) @ q.abs()) + u * dK.abs()
    E = {"ctx": E_ctx, "dQ": E_dQ, "dK": E_dK, "dV": E_dV}
    if dist is not None:
        E["d_sp_w"] = (E_dS.sum(1) * dist.abs()).sum()
        E["d_sp_b"] = E_dS.sum()
    for n in ("ctx", "dQ", "dK", "dV"):
        E[n] = E[n] + FP32_REL * max(1.0, float(val[n].abs().max()))
    if dist is not None:       # fp32 running sums and atomics over ALL of dS: relative to what they accumulate (docstring)
        E["d_sp_w"] = E["d_sp_w"] + FP32_REL * max(1.0, float((dS.abs().sum(1) * dist.abs()).sum()))
        E["d_sp_b"] = E["d_sp_b"] + FP32_REL * max(1.0, float(dS.abs().sum()))
    return val, E


def close(got, ref, E, name, key=None):
    """every element of `got` finite and |got - ref| <= E elementwise; the worst ratio goes to WORST[key or name]."""
    got, ref, E = got.detach().to(F64), ref.detach().to(F64), torch.as_tensor(E, dtype=F64, device=ref.device)
    assert got.shape == ref.shape, (name, tuple(got.shape), tuple(ref.shape))
    bad = ~torch.isfinite(got)
    assert not bool(bad.any()), f"{name}: {int(bad.sum())} non-finite elements"
    ratio = (got - ref).abs() / E
    worst = float(ratio.max()) if ratio.numel() else 0.0
    key = key or name
    if worst > WORST.get(key, (0.0, ""))[0]:
        WORST[key] = (worst, name)
    if worst > 1.0:
        i = int(ratio.reshape(-1).argmax())
        idx = tuple(int(x) for x in torch.unravel_index(torch.tensor(i), ratio.shape)) if ratio.dim() else ()
        raise AssertionError(f"{name}: |got - ref| = {worst:.3g} x the bound at {idx} (got {float(got.reshape(-1)[i]):.6g}, "
                             f"ref {float(ref.reshape(-1)[i]):.6g}, bound {float(E.reshape(-1)[i] if E.dim() else E):.3g}); "
                             f"{int((ratio > 1).sum())} of {ratio.numel()} elements beyond it")
    return worst


def same_bits(name, got, want):
    assert got.dtype == want.dtype and got.shape == want.shape, (name, got.dtype, want.dtype, tuple(got.shape), tuple(want.shape))
    iv = {torch.float32: torch.int32, torch.bfloat16: torch.int16}[got.dtype]
    diff = got.contiguous().view(iv) != want.contiguous().view(iv)
    assert not bool(diff.any()), f"{name}: {int(diff.sum())} elements differ bitwise"


def check_all(got, val, E, name, key, d_init=None):
    """got: dict over NAMES (d_sp_* only with the distance bias); d_init: the (d_sp_w, d_sp_b) the buffers held before the call (the
    kernels accumulate: expected = initial + reference)."""
    for n in ("ctx", "dV", "dQ", "dK"):
        close(got[n], val[n], E[n], f"{name} {n}", f"{key}/{n}")
    if "d_sp_w" in val:
        for j, n in enumerate(("d_sp_w", "d_sp_b")):
            init = 0.0 if d_init is None else float(d_init[j])
            close(got[n].reshape(()), val[n] + init, E[n], f"{name} {n}", f"{key}/{n}")


# ---- layouts ---------------------------------------------------------------------------------------------------------------
def split_heads(x, B, nh):
    """[B*L, heads*64] rows (head h at column h*64) -> [B, heads, L, 64]"""
    return x.reshape(B, -1, nh, 64).permute(0, 2, 1, 3)


def merge_heads(x):
    """[B, heads, L, 64] -> [B*L, heads*64]"""
    B, nh, L, d = x.shape
    return x.permute(0, 2, 1, 3).reshape(B * L, nh * d)


# ---- cases -----------------------------------------------------------------------------------------------------------------
# every 16-row tile count of the register-resident kernels and the 64 / 96 / 128 tile edges of the LDS-tile kernels on both axes
SHORT = [(1, 128), (128, 1), (80, 80), (36, 36), (16, 80), (97, 64), (64, 97), (1, 1), (15, 17), (17, 15), (16, 16), (33, 48),
         (48, 33), (63, 65), (65, 63), (64, 64), (80, 16), (95, 96), (96, 95), (96, 96), (97, 113), (113, 97), (127, 128), (128, 127),
         (128, 128), (15, 33), (33, 127), (127, 63), (63, 1), (113, 16)]
SHORT_F32_TILE = [s for s in SHORT if max(s) <= 64]
SHORT_Q96 = [s for s in SHORT if 64 < s[0] <= 96 and 64 < s[1] <= 96]
# the 128-key tiles of the streaming kernels: one key / one query past a tile, ragged last tiles, a single query row
LONG = [(16, 512), (512, 512), (130, 300), (64, 129), (129, 64), (300, 70), (257, 255), (1, 640)]
BATCHES = [(1, 12), (3, 4), (23, 12)]        # 23 x 12 = 276 workgroups of the one-per-(batch, head) kernels: more than the CUs
MASKS = ["all", "first", "last", "not0", "tail", "lead", "none"]


def key_mask(kind, Lk, mask_mode, tile, gen):
    """one batch entry's key mask [Lk] (True = valid).  Under mask_mode 1 at least one key stays valid."""
    m = torch.ones(Lk, dtype=torch.bool)
    nt = (Lk + tile - 1) // tile
    if kind == "first":
        m[1:] = False
    elif kind == "last":
        m[:-1] = False
    elif kind == "not0":                       # key 0 invalid, random others
        m = torch.rand(Lk, generator=gen) > 0.3
        m[0] = False
        if Lk > 1:
            m[Lk - 1 - int(torch.randint(0, Lk - 1, (1,), generator=gen))] = True
    elif kind == "tail":                       # whole trailing tiles invalid (half of them; within one tile: its second half)
        m[(tile * (nt // 2) if nt > 1 else max(1, Lk // 2)):] = False
    elif kind == "lead":                       # the whole leading tile invalid (flash_fwd_kernel's m_new == -inf prefix)
        if Lk > tile:
            m[:tile] = False
        else:
            m[: Lk // 2] = False
    elif kind == "none":                       # mask_mode 0 only: every key invalid (-10000 on the whole row)
        m[:] = False
    if mask_mode and not bool(m.any()):
        m[:] = True
    return m


def make_case(Lq, Lk, B, nh, bf16, mask_mode, with_dist, alpha, sp_w, seed, rot=0, null_mask=False):
    """CPU tensors of one case: q / k / v / dctx [B, heads, L, 64] fp32 holding the stored values (rounded to bf16 in bf16 mode),
    km [B, Lk] bool or None, dist [B, Lq, Lk] fp32 or None, sp_w / sp_b.  Standard normal operands; in batch entry 0 a key equal to
    3 x query 0 (row maximum far above the rest, in the last tile), in the last batch entry the last query scaled by 8 (|s| ~ 60)."""
    gen = torch.Generator().manual_seed(1000 * seed + 7 * Lq + Lk + 131 * B)
    rnd = lambda *s: torch.randn(*s, generator=gen)
    q, k, v, do = rnd(B, nh, Lq, 64), rnd(B, nh, Lk, 64), rnd(B, nh, Lk, 64), rnd(B, nh, Lq, 64)
    k[0, :, Lk - 3 if Lk > 3 else Lk - 1] = 3.0 * q[0, :, 0]
    q[B - 1, :, Lq - 1] *= 8.0
    if bf16:
        q, k, v, do = (t.bfloat16().float() for t in (q, k, v, do))
    tile = 128 if max(Lq, Lk) > 128 else 16
    kinds = [MASKS[(rot + b) % len(MASKS)] for b in range(B)]
    kinds = [("all" if (kd == "none" and mask_mode) else kd) for kd in kinds]
    if mask_mode and Lk > 128 and rot % 4 == 1:        # the streaming forward's fully excluded prefix needs -inf on a whole leading tile
        kinds[B // 2] = "lead"
    km = None if null_mask else torch.stack([key_mask(kd, Lk, mask_mode, tile, gen) for kd in kinds])
    dist = torch.rand(B, Lq, Lk, generator=gen) * 3.0 if with_dist else None
    f32 = lambda x: float(torch.tensor(x, dtype=torch.float32))      # the kernels read alpha, sp_w and sp_b as fp32
    return dict(q=q, k=k, v=v, dctx=do, km=km, kinds=None if null_mask else kinds, dist=dist, sp_w=f32(sp_w), sp_b=f32(0.1), alpha=f32(alpha),
                mask_mode=mask_mode, bf16=bf16, Lq=Lq, Lk=Lk, B=B, nh=nh)


def case_grid(shapes, seeds=(0, 1), dist_ok=True):
    """(Lq, Lk, B, heads, mask_mode, with_dist, alpha, sp_w, seed, rot, null_mask) over `shapes` x `seeds`: batch size, mask rotation,
    alpha, the distance bias and its weight cycle with the case index instead of multiplying the list; a shape sees mask_mode 0 under
    one seed and 1 under the other."""
    out = []
    for sd in seeds:
        for j, (Lq, Lk) in enumerate(shapes):
            i = j + 3 * sd
            B, nh = BATCHES[i % 3]
            with_dist = dist_ok and (i // 2) % 2 == 0
            out.append((Lq, Lk, B, nh, (j + sd) % 2, with_dist, 0.2 if i % 5 == 3 else 0.125, -1.7 if i % 4 == 1 else 0.3, sd, i,
                        i % 7 == 5))
    return out


def ref_of(c, gemm=False, device=None):
    """attn_ref of a make_case dict (optionally on `device`)"""
    t = lambda x: None if x is None else (x.to(device) if device else x)
    return attn_ref(t(c["q"]), t(c["k"]), t(c["v"]), t(c["km"]), c["mask_mode"], t(c["dist"]), c["sp_w"], c["sp_b"], c["alpha"],
                    t(c["dctx"]), bf16=c["bf16"], gemm=gemm)
