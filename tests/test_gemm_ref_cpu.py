"""tests/gemm_ref.py restates what oracle/planner_oracle.py computes: its `linear`, its `gelu_erf` and their autograd, in float64 to
1e-12 -- the forward with bias + GELU (both Z forms), the data gradient with the GELU backward (both forms), the weight gradient with
the fused bias gradient -- plus the algebra of alpha, residual, accumulate and split ranges that the oracle has no name for."""
import pytest
import torch

from oracle import planner_oracle as po
from tests import gemm_ref as gr

F64 = torch.float64
TOL = 1e-12


def same(got, want, name):
    err = float((got - want).abs().max())
    assert err <= TOL * max(1.0, float(want.abs().max())), (name, err)


@pytest.fixture(scope="module")
def ffn():
    """one FFN block through the oracle in float64 with autograd: h = linear(x, w1, b1), y = gelu_erf(h), o = linear(y, w2, b2)"""
    gen = torch.Generator().manual_seed(5)
    M, H, I = 37, 24, 52
    x, w1, b1, w2, b2 = (torch.randn(*s, generator=gen, dtype=F64).requires_grad_() for s in ((M, H), (I, H), (I,), (H, I), (H,)))
    h = po.linear(x, w1, b1)
    h.retain_grad()
    y = po.gelu_erf(h)
    y.retain_grad()
    o = po.linear(y, w2, b2)
    do = torch.randn(M, H, generator=gen, dtype=F64)
    (o * do).sum().backward()
    return dict(x=x, w1=w1, b1=b1, w2=w2, b2=b2, h=h, y=y, o=o, do=do)


def test_forward_bias_gelu_and_both_saved_tensors(ffn):
    f = {k: v.detach() for k, v in ffn.items()}
    val, _ = gr.gemm_ref(f["x"], f["w1"], bias=f["b1"], act=gr.ACT_GELU, bf16=False)
    same(val["C"], f["y"], "gelu(linear)")
    same(val["Z"], f["h"], "saved pre-activation")
    val, _ = gr.gemm_ref(f["x"], f["w1"], bias=f["b1"], act=gr.ACT_GELU_SAVEGRAD, bf16=False)
    same(val["C"], f["y"], "gelu(linear), derivative saved")
    h = f["h"].clone().requires_grad_()
    po.gelu_erf(h).sum().backward()
    same(val["Z"], h.grad, "saved derivative = autograd of the oracle's gelu_erf")
    val, _ = gr.gemm_ref(f["y"], f["w2"], bias=f["b2"], bf16=False)
    same(val["C"], f["o"], "linear")
    val, _ = gr.gemm_ref(f["x"], f["w1"], bias=f["b1"], act=gr.ACT_RELU, bf16=False)
    same(val["C"], torch.relu(f["h"]), "relu(linear)")


def test_data_gradient_with_gelu_backward(ffn):
    """dh = (do . w2) * gelu'(h): B operand = w2 stored [N (reduction)][K], i.e. logical [I, H] = w2^T"""
    f = {k: v.detach() for k, v in ffn.items()}
    val, _ = gr.gemm_ref(f["do"], f["w2"].t(), Z=f["h"], act=gr.ACT_GELU_BWD, bf16=False)
    same(val["C"], ffn["h"].grad, "dgrad x gelu'(Z)")
    d = gr.gemm_ref(f["x"], f["w1"], bias=f["b1"], act=gr.ACT_GELU_SAVEGRAD, bf16=False)[0]["Z"]
    val, _ = gr.gemm_ref(f["do"], f["w2"].t(), Z=d, act=gr.ACT_MUL_Z, bf16=False)
    same(val["C"], ffn["h"].grad, "dgrad x saved derivative")
    val, _ = gr.gemm_ref(f["do"], f["w2"].t(), bf16=False)
    same(val["C"], ffn["y"].grad, "plain dgrad")
    # relu backward against autograd
    x = f["x"].clone().requires_grad_()
    hr = po.linear(x, f["w1"], f["b1"])
    hr.retain_grad()
    (po.linear(torch.relu(hr), f["w2"], f["b2"]) * f["do"]).sum().backward()
    val, _ = gr.gemm_ref(f["do"], f["w2"].t(), Z=hr.detach(), act=gr.ACT_RELU_BWD, bf16=False)
    same(val["C"], hr.grad, "dgrad x (Z > 0)")
    # the input gradient of the first linear with the gradient already in its buffer as a residual
    val, _ = gr.gemm_ref(hr.grad, f["w1"].t(), R=f["do"], bf16=False)
    same(val["C"], x.grad + f["do"], "dgrad + R")


def test_weight_gradient_with_bias_gradient(ffn):
    """dW[n, k] = sum_m dY[m, n] X[m, k] (TN storage: A = dY^T, B = X^T logically), db = colsum(dY) fused as a_colsum; accumulating"""
    f = {k: v.detach() for k, v in ffn.items()}
    dh = ffn["h"].grad
    w0, b0 = torch.full_like(f["w1"], 0.25), torch.full_like(f["b1"], -0.5)
    for ksplit, out_mode in ((1, 1), (1, 0), (4, 2), (2, 2)):
        val, _ = gr.gemm_ref(dh.t(), f["x"].t(), C0=w0, out_mode=out_mode, ksplit=ksplit, bk=8, bf16=False, colsum_old=b0)
        same(val["C"], ffn["w1"].grad + (w0 if out_mode else 0.0), f"wgrad ksplit {ksplit} out_mode {out_mode}")
        same(val["a_colsum"], ffn["b1"].grad + b0, "bias gradient")


def test_alpha_before_bias_residual_after_activation_and_accumulate():
    gen = torch.Generator().manual_seed(1)
    A, B = torch.randn(9, 16, generator=gen, dtype=F64), torch.randn(7, 16, generator=gen, dtype=F64)
    bias, R, C0 = torch.randn(7, generator=gen, dtype=F64), torch.randn(9, 7, generator=gen, dtype=F64), torch.randn(9, 7, generator=gen, dtype=F64)
    v = -1.7 * (A @ B.t()) + bias
    val, _ = gr.gemm_ref(A, B, alpha=-1.7, bias=bias, R=R, C0=C0, act=gr.ACT_GELU, out_mode=1, bf16=False)
    same(val["C"], po.gelu_erf(v) + R + C0, "C0 + gelu(alpha acc + bias) + R")
    same(val["Z"], v, "Z = alpha acc + bias")
    val, _ = gr.gemm_ref(A[:, :0], B[:, :0], alpha=0.5, bias=bias, bf16=False)
    same(val["C"], bias.expand(9, 7), "K = 0: epi(0)")


def test_split_ranges_follow_the_kernels():
    assert gr.split_ranges(130, 4, 64) == [(0, 64), (64, 128), (128, 130), (130, 130)]        # an empty last split
    assert gr.split_ranges(1000, 4, 64) == [(0, 256), (256, 512), (512, 768), (768, 1000)]
    assert gr.split_ranges(1024, 4, 64) == [(0, 256), (256, 512), (512, 768), (768, 1024)]
    assert gr.split_ranges(1000, 2, 32) == [(0, 512), (512, 1000)]
    assert gr.split_ranges(200, 1, 64) == [(0, 200)]


def test_operands_carry_every_scale_and_the_zero_rows():
    A, B, sa, sb = gr.make_operands(70, 40, 64, True, 0)
    assert set(sa.tolist()) == {2.0 ** e for e in gr.SCALE_EXPS} and set(sb.tolist()) == set(sa.tolist())
    assert not bool(A[70 // 3].any()) and not bool(B[20].any())
    assert torch.equal(A, A.bfloat16().float()) and torch.equal(B, B.bfloat16().float())
    val, E = gr.gemm_ref(A, B, alpha=0.5, bias=torch.ones(40), bf16=True, c_bf16=False)
    assert bool((E["C"][70 // 3] == 0).all()) and bool((E["C"][:, 20] == 0).all())            # exactly epi(0) there
    assert bool((val["C"][70 // 3] == 1.0).all())
