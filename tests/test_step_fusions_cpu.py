"""On the CPU the pass fusions of ops/fused.py all fall back: fused_gelu
ignores a bias it is handed, which stays attached to the linear in front, and
GPT-2's MLP gives the gradients of the plain composition."""

import torch
import torch.nn.functional as F


def test_fused_gelu_with_bias_is_the_plain_composition():
    from adapcc_amd.ops.fused import fused_gelu, gelu_bias_grad_fusable

    torch.manual_seed(0)
    lin = torch.nn.Linear(16, 128)
    x = torch.randn(5, 16, requires_grad=True)
    dy = torch.randn(5, 128)
    assert not gelu_bias_grad_fusable(x.device, x.dtype, 5, 128, lin.bias)

    y = fused_gelu(lin(x), bias=lin.bias)
    y.backward(dy)
    got = (y.detach(), x.grad.clone(), lin.weight.grad.clone(),
           lin.bias.grad.clone())

    x.grad = None
    lin.zero_grad(set_to_none=True)
    y = F.gelu(F.linear(x, lin.weight, lin.bias), approximate="tanh")
    y.backward(dy)
    want = (y.detach(), x.grad, lin.weight.grad, lin.bias.grad)
    for g, w in zip(got, want):
        assert torch.equal(g, w)


def test_mlp_gradients_are_the_plain_composition():
    from adapcc_amd.models.gpt2 import MLP, GPT2Config

    torch.manual_seed(1)
    mlp = MLP(GPT2Config(n_embd=32))
    torch.nn.init.normal_(mlp.c_fc.bias, std=0.02)
    torch.nn.init.normal_(mlp.c_proj.bias, std=0.02)
    x = torch.randn(3, 7, 32, requires_grad=True)
    dy = torch.randn(3, 7, 32)

    mlp(x).backward(dy)
    got = [x.grad.clone()] + [p.grad.clone() for p in mlp.parameters()]

    x.grad = None
    mlp.zero_grad(set_to_none=True)
    h = F.gelu(F.linear(x, mlp.c_fc.weight, mlp.c_fc.bias),
               approximate="tanh")
    F.linear(h, mlp.c_proj.weight, mlp.c_proj.bias).backward(dy)
    want = [x.grad] + [p.grad for p in mlp.parameters()]
    assert all(g is not None for g in want)
    for g, w in zip(got, want):
        assert torch.equal(g, w)
