"""The comparator of the GEMM op tests (tests/gemm_ref.py `close`, `Guarded` and the bounds of `gemm_ref`) can pass and can fail.

Pass: CPU emulations of the kernels' summation and rounding schedules -- products and block sums in float64, rounded to fp32 / bf16 /
half exactly where the kernels hold fp32 or store -- stay within ratio 1 of the bound on EVERY element of EVERY shape of the GPU
matrix (gemm_ref.shape_matrix):

  chain   fp32 accumulation in chained 32-wide blocks (one bf16 MFMA k-step, one fp32 slab), the epilogue's fp32 steps one by one
  k2      the reduction's 64-wide slabs dealt to two chains whose partial sums are added in the epilogue (mm32 `k2` classes)
  split   ksplit partial sums, each scaled (the first with the bias), added to C in every order (fp32 atomics)
  stores  bf16 C, bf16 Z of ACT_GELU, half Z of ACT_GELU_SAVEGRAD, one rounding after the fp32 sum under out_mode 1

Fail: every mutation of MUTATIONS raises -- an AssertionError of `close` or of a guard."""
import itertools

import pytest
import torch

from tests import gemm_ref as gr

F64 = torch.float64
rf = lambda x: x.to(torch.float32).to(F64)
rb = lambda x: x.to(torch.float32).to(torch.bfloat16).to(F64)
rh = lambda x: x.to(torch.float32).to(torch.float16).to(F64)


def chain(A, B, lo, hi, starts=None, mut=None):
    """fp32 chain over 32-wide blocks of [lo, hi): acc = fl(acc + fl(A_blk . B_blk^T)).  mutations act on 64-wide slabs"""
    acc = torch.zeros(A.shape[0], B.shape[0], dtype=F64)
    starts = range(lo, hi, 32) if starts is None else starts
    last = (hi - lo - 1) // 64 if hi > lo else 0
    for k0 in starts:
        k1 = min(k0 + 32, hi)
        slab = (k0 - lo) // 64
        a0, a1 = k0, k1
        if mut == "drop_slab" and slab == 1:
            continue
        if mut == "stale_last_slab" and slab == last and slab > 0:          # the ring's last slot still holds the slab before
            a0, a1 = k0 - 64, k1 - 64
        p = rf(A[:, a0:a1] @ B[:, a0:a1].t())
        acc = rf(acc + p)
        if mut == "double_slab" and slab == 1:
            acc = rf(acc + p)
    return acc


def emulate(A, B, ep, alpha=1.0, act=gr.ACT_NONE, out_mode=0, ksplit=1, bk=64, bf16=True, c_bf16=None, sched="chain", order=None,
            mut=None, colsum_old=None):
    c_bf16 = bf16 if c_bf16 is None else c_bf16
    A, B = A.to(F64), B.to(F64)
    K = A.shape[1]
    bias, R, C0, Z = (None if ep.get(k) is None else ep[k].to(F64) for k in ("bias", "R", "C0", "Z"))
    if mut == "bias_shifted" and bias is not None:
        bias = torch.roll(bias, 1)
    vs = []
    for s, (lo, hi) in enumerate(gr.split_ranges(K, ksplit, bk)):
        if sched == "k2":
            st = list(range(lo, hi, 32))
            acc = rf(chain(A, B, lo, hi, [k for k in st if (k // 64) % 2 == 0]) + chain(A, B, lo, hi, [k for k in st if (k // 64) % 2 == 1]))
        else:
            acc = chain(A, B, lo, hi, mut=mut)
        b = bias if (bias is not None and (s == 0 or mut == "bias_every_split")) else None
        if mut == "alpha_after_bias" and b is not None:
            v = rf(alpha * rf(acc + b))
        else:
            v = rf(alpha * acc)
            v = v if b is None else rf(v + b)
        vs.append(v)
    out = {}
    if ksplit == 1:
        v = vs[0]
        if act == gr.ACT_GELU:
            out["Z"] = (rb if bf16 else rf)(gr.gelu(v) if mut == "z_after_activation" else v)
            y = rf(gr.gelu(v))
        elif act == gr.ACT_GELU_SAVEGRAD:
            d = rf(gr.gelu_grad(v))
            out["Z"] = ((rb if mut == "grad_as_bf16" else rh) if bf16 else rf)(d)
            y = rf(gr.gelu(v))
        elif act == gr.ACT_RELU:
            y = torch.relu(v)
        elif act == gr.ACT_GELU_BWD:
            y = rf(v * rf(gr.gelu_grad(Z)))
        elif act == gr.ACT_MUL_Z:
            y = rf(v * Z)
        elif act == gr.ACT_RELU_BWD:
            y = torch.where(Z > 0, v, torch.zeros_like(v))
        else:
            y = v
        if R is not None:
            y = rf(y + R)
        if out_mode:
            y = rf(y + C0)
        out["C"] = (rb if c_bf16 else rf)(y)
    else:
        C = C0
        for j, s in enumerate(order if order is not None else range(ksplit)):
            t = vs[s]
            if R is not None and (s == 0 or mut == "r_every_split"):
                t = rf(t + R)
            C = rf(C + t)
        out["C"] = C
    if colsum_old is not None:
        X = B[torch.arange(A.shape[0]) % B.shape[0]] if mut == "colsum_over_b" else A
        acc = torch.zeros(A.shape[0], dtype=F64)
        for k0 in range(0, K, 32):
            acc = rf(acc + rf(X[:, k0:k0 + 32].sum(1)))
        out["a_colsum"] = rf(colsum_old.to(F64) + acc)
    return out


def case(M, N, K, bf16, i, act=None, c_bf16=None, bias=True, R=True, out_mode=None, alpha=None):
    act = gr.ACTS[i % 7] if act is None else act
    c_bf16 = (bf16 and i % 2 == 0) if c_bf16 is None else c_bf16
    out_mode = (i // 2) % 2 if out_mode is None else out_mode
    alpha = gr.f32((1.0, 0.5, -1.7)[i % 3] if alpha is None else alpha)
    A, B, sa, sb = gr.make_operands(M, N, K, bf16, 0)
    ep = gr.make_epilogue(M, N, act, bf16, c_bf16, i, with_bias=bias, with_r=R)
    return dict(A=A, B=B, sa=sa, sb=sb, ep=ep, kw=dict(alpha=alpha, act=act, out_mode=out_mode, bk=64 if bf16 else 32, bf16=bf16, c_bf16=c_bf16))


def ref_of(c, **over):
    kw = dict(c["kw"], **over)
    ep = c["ep"]
    return gr.gemm_ref(c["A"], c["B"], bias=ep["bias"], R=ep["R"], C0=ep["C0"], Z=ep["Z"], **kw)


SHAPES = gr.shape_matrix()
CHUNKS = 16


@pytest.mark.parametrize("chunk", range(CHUNKS))
def test_schedule_emulations_stay_inside_the_bound(chunk):
    worst = 0.0
    for i, (M, N, K, bf16) in list(enumerate(SHAPES))[chunk::CHUNKS]:
        # the whole epilogue, activation / C dtype / out_mode / alpha cycling with the shape; k2 where the mm32 k2 classes run
        c = case(M, N, K, bf16, i)
        val, E = ref_of(c)
        sched = "k2" if (bf16 and K % 128 == 0 and K >= 256 and i % 2) else "chain"
        got = emulate(c["A"], c["B"], c["ep"], sched=sched, **c["kw"])
        for n in val:
            worst = max(worst, gr.close(got[n], val[n], E[n], f"{sched} {M}x{N}x{K} act {c['kw']['act']} {n}", "cpu/" + n))
        # split-K with the fused bias gradient, every order of the atomic additions
        ks = (2, 4)[i % 2]
        c = case(M, N, K, bf16, i, act=gr.ACT_NONE, c_bf16=False, R=False, out_mode=2)
        old = torch.randn(M, generator=torch.Generator().manual_seed(i))
        val, E = ref_of(c, ksplit=ks, colsum_old=old)
        for order in itertools.permutations(range(ks)):
            got = emulate(c["A"], c["B"], c["ep"], ksplit=ks, order=order, colsum_old=old, **c["kw"])
            for n in val:
                worst = max(worst, gr.close(got[n], val[n], E[n], f"split {ks} {order} {M}x{N}x{K} {n}", "cpu/split/" + n))
    assert worst <= 1.0


def must_pass(fn, *a):
    """a precondition inside a mutation case: its failure must not count as the mutation being caught"""
    try:
        return fn(*a)
    except AssertionError as e:
        raise RuntimeError(f"precondition of a mutation case failed: {e}")


def small_row(c):
    """a row of A of scale 2^-10 that is not the zero row"""
    rows = [int(r) for r in (c["sa"] == 2.0 ** -10).nonzero().flatten() if int(r) != c["A"].shape[0] // 3]
    return rows[0]


def swap_tiles(C, bm=64, bn=64):
    C = C.clone()
    C[:bm, :bn], C[bm:2 * bm, :bn] = C[bm:2 * bm, :bn].clone(), C[:bm, :bn].clone()
    return C


def remap_other_axis(C, bm=64, bn=64):
    """2 x 3 tiles (tiles_m < tiles_n: tn = id / tiles_m, tm = id % tiles_m): every workgroup computes the tile of the map's other branch
    (tm = id / tiles_n, tn = id % tiles_n) and stores it where the right branch points"""
    out = C.clone()
    for i in range(6):
        tm, tn, wm, wn = i % 2, i // 2, i // 3, i % 3
        out[tm * bm:(tm + 1) * bm, tn * bn:(tn + 1) * bn] = C[wm * bm:(wm + 1) * bm, wn * bn:(wn + 1) * bn]
    return out


def mut_drop_k(K):
    def run():
        c = case(128, 192, K, True, 0, act=gr.ACT_NONE, c_bf16=False, R=False, out_mode=0, alpha=1.0)
        val, E = ref_of(c)
        r = small_row(c)
        A = c["A"].clone()
        A[r, int(A[r].abs().argmax())] = 0.0                          # one product a_k b_k missing from every element of the row
        got = emulate(A, c["B"], c["ep"], **c["kw"])
        gr.close(got["C"][r], val["C"][r], E["C"][r], f"dropped k, row of scale 2^-10, K {K}")
    return run


def mut_chain(mut, **kw):
    def run():
        c = case(128, 192, 256, True, 1, **kw)
        val, E = ref_of(c)
        got = emulate(c["A"], c["B"], c["ep"], mut=mut, **c["kw"])
        for n in val:
            gr.close(got[n], val[n], E[n], f"{mut} {n}")
    return run


def mut_output(fn):
    def run():
        c = case(128, 192, 128, True, 0, act=gr.ACT_NONE, R=False, out_mode=0)
        val, E = ref_of(c)
        gr.close(fn(emulate(c["A"], c["B"], c["ep"], **c["kw"])["C"]), val["C"], E["C"], fn.__name__)
    return run


def mut_split(mut):
    def run():
        c = case(72, 136, 512, True, 0, act=gr.ACT_NONE, c_bf16=False, out_mode=2)
        val, E = ref_of(c, ksplit=4)
        got = emulate(c["A"], c["B"], c["ep"], ksplit=4, mut=mut, **c["kw"])
        gr.close(got["C"], val["C"], E["C"], mut)
    return run


def mut_colsum():
    c = case(72, 136, 256, True, 0, act=gr.ACT_NONE, c_bf16=False, R=False, out_mode=1)
    old = torch.randn(72, generator=torch.Generator().manual_seed(2))
    val, E = ref_of(c, colsum_old=old)
    got = emulate(c["A"], c["B"], c["ep"], mut="colsum_over_b", colsum_old=old, **c["kw"])
    must_pass(gr.close, got["C"], val["C"], E["C"], "C beside the wrong column sums")          # the product itself is right
    gr.close(got["a_colsum"], val["a_colsum"], E["a_colsum"], "a_colsum summed over B")


def mut_group_order():
    """three problems of one shape with K = 128, 512, 256: the launcher sorts them to 512, 256, 128; C pointers taken from the caller's
    order put the K = 512 result into the first problem's buffer"""
    Ks = (128, 512, 256)
    cs = [case(64, 72, K, True, 0, act=gr.ACT_NONE, c_bf16=False, R=False, out_mode=0) for K in Ks]
    outs = [emulate(c["A"], c["B"], c["ep"], **c["kw"])["C"] for c in cs]
    order = sorted(range(3), key=lambda i: -Ks[i])
    for i, c in enumerate(cs):
        val, E = ref_of(c)
        gr.close(outs[order[i]], val["C"], E["C"], f"group member {i} holds the result of member {order[i]}")


def mut_pad_columns():
    g = gr.guarded_2d(65, 20, 88, torch.float32, col0=8)
    g.view.fill_(1.0)
    must_pass(g.intact, "untouched")
    g.flat.view(69, 88)[2:67, 8:32] = 1.0                             # the 8-column chunk that holds columns 16 .. 23
    g.intact("pad columns 20 .. 23 written")


def mut_batch_swapped():
    gen = torch.Generator().manual_seed(4)
    A = torch.randn(2, 3, 70, 64, generator=gen).bfloat16().float()
    B = (torch.randn(2, 3, 40, 64, generator=gen) * 0.1 + 0.01).bfloat16().float()
    val, E = gr.gemm_ref(A, B, alpha=0.125)
    got = torch.stack([torch.stack([emulate(A[zo, zi], B[zo, zi], {}, alpha=0.125)["C"] for zi in range(3)]) for zo in range(2)])
    must_pass(gr.close, got, val["C"], E["C"], "batched, right")
    z = torch.arange(6)
    swapped = got.reshape(6, 70, 40)[(z % 2) * 3 + z // 2].reshape(2, 3, 70, 40)     # (zo, zi) = (z % outer, z / outer)
    gr.close(swapped, val["C"], E["C"], "batch index zo / zi swapped")


MUTATIONS = {
    "one dropped k-product in a row of scale 2^-10, K = 64": mut_drop_k(64),
    "one dropped k-product in a row of scale 2^-10, K = 128": mut_drop_k(128),
    "one dropped k-product in a row of scale 2^-10, K = 768": mut_drop_k(768),
    "a dropped slab": mut_chain("drop_slab"),
    "a doubled slab": mut_chain("double_slab"),
    "the last slab of the ring read one slab stale": mut_chain("stale_last_slab"),
    "two output tiles swapped": mut_output(swap_tiles),
    "a row of the remap applied to the other axis": mut_output(remap_other_axis),
    "bias shifted by one column": mut_chain("bias_shifted", act=gr.ACT_NONE),
    "bias added by every split": mut_split("bias_every_split"),
    "R added by every split": mut_split("r_every_split"),
    "alpha applied after the bias": mut_chain("alpha_after_bias", act=gr.ACT_NONE, alpha=0.5),
    "the GELU derivative stored as bf16 instead of half": mut_chain("grad_as_bf16", act=gr.ACT_GELU_SAVEGRAD),
    "Z stored after the activation": mut_chain("z_after_activation", act=gr.ACT_GELU),
    "a_colsum summed over B instead of A": mut_colsum,
    "a group problem's C pointer from the caller's order": mut_group_order,
    "pad columns written": mut_pad_columns,
    "batch index zo / zi swapped": mut_batch_swapped,
}


@pytest.mark.parametrize("name", list(MUTATIONS))
def test_the_comparator_fails_for(name):
    with pytest.raises(AssertionError):
        MUTATIONS[name]()


def test_the_unmutated_emulations_of_the_mutation_cases_pass():
    """the mutation cases raise because of the mutation: the same cases without it stay inside the bound"""
    for kw in (dict(), dict(act=gr.ACT_NONE), dict(act=gr.ACT_NONE, alpha=0.5), dict(act=gr.ACT_GELU_SAVEGRAD), dict(act=gr.ACT_GELU)):
        c = case(128, 192, 256, True, 1, **kw)
        val, E = ref_of(c)
        got = emulate(c["A"], c["B"], c["ep"], **c["kw"])
        for n in val:
            gr.close(got[n], val[n], E[n], f"unmutated {kw} {n}")
    c = case(72, 136, 512, True, 0, act=gr.ACT_NONE, c_bf16=False, out_mode=2)
    val, E = ref_of(c, ksplit=4)
    gr.close(emulate(c["A"], c["B"], c["ep"], ksplit=4, **c["kw"])["C"], val["C"], E["C"], "unmutated split with R on the first split")
    Ks = (128, 512, 256)
    for K in Ks:
        c = case(64, 72, K, True, 0, act=gr.ACT_NONE, c_bf16=False, R=False, out_mode=0)
        val, E = ref_of(c)
        gr.close(emulate(c["A"], c["B"], c["ep"], **c["kw"])["C"], val["C"], E["C"], f"unmutated group member K {K}")
