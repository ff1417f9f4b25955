"""fused_gelu(x, bias=b): the GeLU backward that also sums the dx it writes
down the columns into the gradient of the bias in front of it (csrc/gelu.hip
gelu_bwd_bias, folded by csrc/colsum.hip).

dx is fused_gelu's without the bias, bit for bit. The bias gradient is held
to an fp64 column sum of that bf16 dx: one bf16 rounding of the result (2^-8
relative) plus the worst case of fp32 accumulation in any order
(rows * 2^-24 * sum_i |dx_ij|); torch's own dx.sum(0) is held to the same
bound to show the inputs allow it. Width 200 is not built: there the bias is
ignored and stays with whoever attached it."""

import pytest
import torch

pytestmark = pytest.mark.gpu

ROWS = [1, 4, 5, 1023]
COLS = [128, 3072, 4096]
DT = torch.bfloat16


def _data(rows, cols):
    g = torch.Generator(device="cuda").manual_seed(rows * 8191 + cols)
    x = torch.randn(rows, cols, device="cuda", generator=g).to(DT)
    dy = torch.randn(rows, cols, device="cuda", generator=g).to(DT)
    return x, dy


def _run(x, dy, bias):
    from adapcc_amd.ops.fused import fused_gelu

    xr = x.detach().clone().requires_grad_(True)
    y = fused_gelu(xr, bias=bias) if bias is not None else fused_gelu(xr)
    y.backward(dy)
    return y.detach(), xr.grad


def _within_bound(got, dx, rows):
    exact = dx.double().sum(0)
    bound = 2.0 ** -8 * exact.abs() + rows * 2.0 ** -24 * dx.double().abs(
    ).sum(0)
    err = (got.double() - exact).abs()
    worst = (err - bound).max().item()
    print(f"rows {rows} cols {dx.shape[1]}: max err {err.max().item():.3e}, "
          f"max (err - bound) {worst:.3e}")
    return bool((err <= bound).all())


@pytest.mark.parametrize("cols", COLS)
@pytest.mark.parametrize("rows", ROWS)
def test_dx_bits_and_bias_gradient(rows, cols):
    from adapcc_amd.ops.fused import gelu_bias_grad_fusable

    x, dy = _data(rows, cols)
    bias = torch.zeros(cols, device="cuda", dtype=DT, requires_grad=True)
    assert gelu_bias_grad_fusable(x.device, x.dtype, rows, cols, bias)
    y0, dx0 = _run(x, dy, None)
    y1, dx1 = _run(x, dy, bias)
    assert torch.equal(y1, y0)
    assert torch.equal(dx1, dx0)
    assert bias.grad is not None and bias.grad.dtype == DT
    assert bias.grad.shape == (cols,)
    assert _within_bound(bias.grad, dx0, rows), "kernel column sum"
    assert _within_bound(dx0.sum(0), dx0, rows), "torch column sum"


@pytest.mark.parametrize("dtype", [torch.float32, torch.float16],
                         ids=["f32", "f16"])
def test_other_dtypes_keep_the_plain_backward(dtype):
    """The kernel pins dx's bits for bf16 only; f32 and f16 are not fusable
    and ignore the bias."""
    from adapcc_amd.ops.fused import gelu_bias_grad_fusable

    x, dy = (t.to(dtype) for t in _data(5, 128))
    bias = torch.zeros(128, device="cuda", dtype=dtype, requires_grad=True)
    assert not gelu_bias_grad_fusable(x.device, dtype, 5, 128, bias)
    _, dx0 = _run(x, dy, None)
    _, dx1 = _run(x, dy, bias)
    assert torch.equal(dx1, dx0)
    assert bias.grad is None


def test_3d_input_sums_over_all_leading_dims():
    x, dy = _data(12, 128)
    bias = torch.zeros(128, device="cuda", dtype=DT, requires_grad=True)
    _, dx = _run(x.view(3, 4, 128), dy.view(3, 4, 128), bias)
    assert _within_bound(bias.grad, dx.view(12, 128), 12)


@pytest.mark.parametrize("rows", ROWS)
def test_unsupported_width_ignores_the_bias(rows):
    from adapcc_amd.ops.fused import gelu_bias_grad_fusable

    x, dy = _data(rows, 200)
    bias = torch.zeros(200, device="cuda", dtype=DT, requires_grad=True)
    assert not gelu_bias_grad_fusable(x.device, x.dtype, rows, 200, bias)
    y0, dx0 = _run(x, dy, None)
    y1, dx1 = _run(x, dy, bias)
    assert torch.equal(y1, y0) and torch.equal(dx1, dx0)
    assert bias.grad is None


def test_switch_off_and_no_grad_leave_the_bias_alone(monkeypatch):
    from adapcc_amd.ops import fused

    x, dy = _data(5, 128)
    bias = torch.zeros(128, device="cuda", dtype=DT, requires_grad=True)
    with torch.no_grad():
        assert not fused.gelu_bias_grad_fusable(x.device, DT, 5, 128, bias)
    assert not fused.gelu_bias_grad_fusable(x.device, DT, 5, 128, bias.detach())
    monkeypatch.setattr(fused, "FUSE_GELU_BIAS_GRAD", False)
    assert not fused.gelu_bias_grad_fusable(x.device, DT, 5, 128, bias)
    _run(x, dy, bias)
    assert bias.grad is None


def test_mlp_bias_gradient_reaches_c_fc(monkeypatch):
    """GPT-2's MLP hands c_fc its bias detached and still fills c_fc.bias.grad;
    everything else keeps its bits."""
    from adapcc_amd.models.gpt2 import MLP, GPT2Config
    from adapcc_amd.ops import fused

    torch.manual_seed(7)
    mlp = MLP(GPT2Config(n_embd=768)).to("cuda", DT)
    torch.nn.init.normal_(mlp.c_fc.bias, std=0.02)
    x, _ = _data(37, 768)
    dy = _data(37, 768)[1]

    def step():
        mlp.zero_grad(set_to_none=True)
        xr = x.clone().requires_grad_(True)
        y = mlp(xr)
        y.backward(dy)
        return y.detach(), xr.grad, {n: p.grad.clone()
                                     for n, p in mlp.named_parameters()}

    y1, dx1, g1 = step()
    monkeypatch.setattr(fused, "FUSE_GELU_BIAS_GRAD", False)
    y0, dx0, g0 = step()
    assert torch.equal(y1, y0) and torch.equal(dx1, dx0)
    for n in g0:
        if n != "c_fc.bias":
            assert torch.equal(g1[n], g0[n]), n
    # each is one bf16 rounding (2^-8) of an fp32 sum of the same 37 values
    # per column; the sums differ by at most rows * 2^-24 * sum |dx|, with
    # |dx| under 4 here
    torch.testing.assert_close(g1["c_fc.bias"].float(),
                               g0["c_fc.bias"].float(), rtol=2.0 ** -6,
                               atol=37 * 2.0 ** -24 * 37 * 4)


def test_empty_batch_leaves_the_bias_with_the_linear():
    """No rows: nothing to launch, so the bias stays attached to c_fc and
    still gets a (zero) gradient."""
    from adapcc_amd.models.gpt2 import MLP, GPT2Config
    from adapcc_amd.ops import fused

    mlp = MLP(GPT2Config(n_embd=128)).to("cuda", DT)
    x = torch.zeros(0, 128, device="cuda", dtype=DT)
    assert not fused.gelu_bias_grad_fusable(x.device, DT, 0, 512,
                                            mlp.c_fc.bias)
    mlp(x).sum().backward()
    g = mlp.c_fc.bias.grad
    assert g is not None and g.shape == (512,) and not g.any()
