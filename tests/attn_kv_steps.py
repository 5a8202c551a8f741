"""Cases, reference and CPU emulation for the per-episode K/V indirection of the attention operator (etp_attn_fwd_kv /
etp_attn_bwd_kv, include/etpnav_hip.h), shared by tests/test_attn_kv_steps_cpu.py and tests/test_attn_kv_steps_gpu.py.

The batched rollout stacks T steps along the batch axis: B = T * kv_mod episodes, episode e = t * kv_mod + b reads the keys / values /
key mask of instruction b = e % kv_mod.  A case holds q / dctx per stacked episode and k / v / km per INSTRUCTION; `replicated` lays
them out as the T-fold copy the plain operator takes, which is also what tests/attn_ref.py's fp64 reference is evaluated on.

Summed gradient (sum_steps = 1): the kernel keeps dK / dV of instruction b in fp32 accumulators over the T episodes that read it and
stores once.  Reference: sum_t dK_t, sum_t dV_t of attn_ref.  Bound: sum_t E_dK_t, sum_t E_dV_t, with no multiplier:
  * E_t already bounds what episode t's products can be off by (bf16 P and dS, the rounded D: attn_ref's docstring);
  * attn_ref's E_t ends with u |dK_t|, the store rounding of a per-episode output.  The summed kernel rounds only the total, once:
    u |sum_t dK_t| <= sum_t u |dK_t|, so the T per-episode store terms cover it;
  * the fp32 term FP32_REL max(1, max|ref_t|) per episode covers accumulation order; T episodes, T terms.
"""
import torch

from tests import attn_ref as ar

F64 = torch.float64
rb = lambda x: x.to(torch.bfloat16).to(F64)
rf = lambda x: x.to(torch.float32).to(F64)
Tr = lambda x: x.transpose(-1, -2)

# instruction mask patterns (attn_ref.key_mask kinds): a fully excluded LEADING key tile and the last key only valid are always present
KINDS = {1: ("lead", "last", "not0", "tail", "all"), 0: ("last", "none", "not0", "lead", "first")}


def make_steps_case(Lq, Lk, kv_mod, T, nh, mask_mode, seed, rot=0, alpha=0.125, null_mask=False):
    """CPU tensors: q / dctx [T*kv_mod, heads, Lq, 64], k / v [kv_mod, heads, Lk, 64] (bf16 values in fp32), km [kv_mod, Lk] bool.
    Standard normal operands as attn_ref.make_case: instruction 0 holds a key equal to 3 x query 0 of episode 0 in its last tile, the
    last episode's last query is scaled by 8."""
    B = kv_mod * T
    gen = torch.Generator().manual_seed(7919 * seed + 13 * Lq + Lk + 101 * kv_mod + 17 * T)
    rnd = lambda *s: torch.randn(*s, generator=gen)
    q, do = rnd(B, nh, Lq, 64), rnd(B, nh, Lq, 64)
    k, v = rnd(kv_mod, nh, Lk, 64), rnd(kv_mod, nh, Lk, 64)
    k[0, :, Lk - 3 if Lk > 3 else Lk - 1] = 3.0 * q[0, :, 0]
    q[B - 1, :, Lq - 1] *= 8.0
    q, k, v, do = (t.bfloat16().float() for t in (q, k, v, do))
    tile = 128 if max(Lq, Lk) > 128 else 16
    kinds = [KINDS[mask_mode][(rot + b) % len(KINDS[mask_mode])] for b in range(kv_mod)]
    km = None if null_mask else torch.stack([ar.key_mask(kd, Lk, mask_mode, tile, gen) for kd in kinds])
    f32 = lambda x: float(torch.tensor(x, dtype=torch.float32))
    return dict(q=q, k=k, v=v, dctx=do, km=km, kinds=kinds, alpha=f32(alpha), mask_mode=mask_mode, Lq=Lq, Lk=Lk, kv_mod=kv_mod, T=T,
                B=B, nh=nh)


def replicated(c):
    """the attn_ref.make_case-shaped dict of the same problem with K, V and masks replicated T times (episode e at index e)"""
    T = c["T"]
    return dict(q=c["q"], k=c["k"].repeat(T, 1, 1, 1), v=c["v"].repeat(T, 1, 1, 1), dctx=c["dctx"],
                km=None if c["km"] is None else c["km"].repeat(T, 1), kinds=None, dist=None, sp_w=0.0, sp_b=0.0, alpha=c["alpha"],
                mask_mode=c["mask_mode"], bf16=True, Lq=c["Lq"], Lk=c["Lk"], B=c["B"], nh=c["nh"])


def sum_steps(x, c):
    """[T*kv_mod, ...] per stacked episode -> [kv_mod, ...] summed over the T episodes of each instruction"""
    return x.reshape(c["T"], c["kv_mod"], *x.shape[1:]).sum(0)


def summed_ref(c, device=None):
    """-> (values, bounds) of the replicated problem (attn_ref, all tensors per stacked episode) plus dK_sum / dV_sum [kv_mod, ...]"""
    val, E = ar.ref_of(replicated(c), device=device)
    for n in ("dK", "dV"):
        val[n + "_sum"], E[n + "_sum"] = sum_steps(val[n], c), sum_steps(E[n], c)
    return val, E


def emulate_summed(c, mut=None):
    """The summed kernel's schedule on the CPU (attn.hip flash_fwd_kernel, flash_bwd_dq_kernel, flash_bwd_dkv_kernel<., true>): every
    product in float64, rounded where the kernels hold fp32 / store bf16.  Forward: online softmax over 128-key tiles, exp(s - m_run)
    rounded to bf16 per tile; backward: P recomputed from lse, D = rowsum(dO * O) from the rounded O, P and dS rounded to bf16 before
    their products, dK / dV accumulated in fp32 over the query tiles of ALL T episodes of an instruction and rounded to bf16 once.
    -> dict dK_sum, dV_sum [kv_mod, heads, Lk, 64].

    mut: 'drop_episode'  the last step's episodes never reach the accumulators (a loop that ends one step early)
         'no_modulo'     episode e reads instruction min(e, kv_mod - 1): b in place of b % kv_mod, clamped to the cache's last instruction
         'wrong_mask'    keys / values of the right instruction under the key mask of the next one"""
    T, M = c["T"], c["kv_mod"]
    alpha = c["alpha"]
    acc = {"dK_sum": torch.zeros(M, c["nh"], c["Lk"], 64, dtype=F64), "dV_sum": torch.zeros(M, c["nh"], c["Lk"], 64, dtype=F64)}
    for e in range(c["B"]):
        t, b = divmod(e, M)
        if mut == "drop_episode" and t == T - 1:
            continue
        bk = min(e, M - 1) if mut == "no_modulo" else b
        bm = (b + 1) % M if mut == "wrong_mask" else bk
        q, do = c["q"][e].to(F64), c["dctx"][e].to(F64)
        k, v = c["k"][bk].to(F64), c["v"][bk].to(F64)
        s = rf(alpha * (q @ Tr(k)))
        if c["km"] is not None:
            neg = float("-inf") if c["mask_mode"] else -10000.0
            s = rf(s + torch.where(c["km"][bm], 0.0, neg).to(F64)[None, None, :])
        m_run = torch.full(s.shape[:-1] + (1,), float("-inf"), dtype=F64)
        l_run = torch.zeros_like(m_run)
        o = torch.zeros(s.shape[:-1] + (64,), dtype=F64)
        for k0 in range(0, c["Lk"], 128):
            st = s[..., k0:k0 + 128]
            m_new = torch.maximum(m_run, st.amax(-1, keepdim=True))
            mref = torch.where(torch.isinf(m_new), torch.zeros_like(m_new), m_new)
            ex = rf(torch.exp(st - mref))
            scale = rf(torch.exp(m_run - mref))
            l_run = rf(l_run * scale + ex.sum(-1, keepdim=True))
            o = rf(o * scale + rb(ex) @ v[..., k0:k0 + 128, :])
            m_run = m_new
        ctx = rb(o / l_run)
        lse = rf(m_run + torch.log(l_run))
        p = rf(torch.exp(s - lse))
        dp = rf(do @ Tr(v))
        D = rf((do * ctx).sum(-1, keepdim=True))
        ds = rb(p * (dp - D))
        acc["dV_sum"][b] = rf(acc["dV_sum"][b] + Tr(rb(p)) @ do)         # fp32 accumulators, carried from episode to episode
        acc["dK_sum"][b] = rf(acc["dK_sum"][b] + Tr(ds) @ q)
    return {"dK_sum": rb(rf(alpha * acc["dK_sum"])), "dV_sum": rb(acc["dV_sum"])}
