"""Packed-QKV flash attention (ops/attention.py: flash_attention_qkv) and
the in-kernel delta of the backward (csrc/attn.hip): the packed path must
equal the unpacked one bitwise, match the fp32 reference, write every
element of its single [B,T,3C] gradient, take strided upstream gradients,
fall back where it does not qualify, and stay hipGraph-capturable."""

import math

import pytest
import torch

from attn_util import heads, ref_attention_f32, unheads

pytestmark = pytest.mark.gpu

D = 64
SHAPES = [(1, 1, 128), (2, 3, 256)]


def make_qkv(B, H, S, seed=0):
    torch.manual_seed(seed)
    return torch.randn(B, S, 3 * H * D, device="cuda", dtype=torch.bfloat16)


def ref_packed_f32(qkv, H, g):
    """y [B,T,C] and d(qkv) [B,T,3C] of the fp32 reference for upstream g."""
    C = H * D
    x = qkv.detach().float().requires_grad_(True)
    q, k, v = (heads(t, H) for t in x.split(C, dim=2))
    y = unheads(ref_attention_f32(q, k, v, 1.0 / math.sqrt(D), True))
    y.backward(g.float())
    return y.detach(), x.grad


def assert_grads_close(got, want, C):
    # the three gradients separately, as the unpacked test does
    for part_got, part_want in zip(got.float().split(C, dim=2),
                                   want.split(C, dim=2)):
        torch.testing.assert_close(part_got, part_want, rtol=5e-2, atol=5e-2)


@pytest.mark.parametrize("B,H,S", SHAPES)
def test_packed_equals_unpacked_bitwise(B, H, S):
    from adapcc_amd.ops.attention import (_FlashAttnFn, fa_qkv_supported,
                                          flash_attention_qkv)

    C = H * D
    qkv = make_qkv(B, H, S).requires_grad_(True)
    g = torch.randn(B, S, C, device="cuda", dtype=torch.bfloat16)
    assert fa_qkv_supported(qkv, H, 0.0)

    # unpacked: _FlashAttnFn on the split views
    q, k, v = (heads(t, H).requires_grad_(True)
               for t in qkv.detach().split(C, dim=2))
    o = _FlashAttnFn.apply(q, k, v, 1.0 / math.sqrt(D), True)
    o.backward(heads(g, H))
    want_y = unheads(o.detach())
    want_grad = torch.cat([unheads(t.grad) for t in (q, k, v)], dim=2)

    y = flash_attention_qkv(qkv, H)
    assert y.shape == (B, S, C) and y.is_contiguous()
    torch.testing.assert_close(y.detach(), want_y, rtol=0, atol=0)

    # poison the block torch.empty hands to the packed gradient next
    poison = torch.full((B, S, 3 * C), float("nan"), device="cuda",
                        dtype=torch.bfloat16)
    del poison
    y.backward(g)
    assert torch.isfinite(qkv.grad).all()
    torch.testing.assert_close(qkv.grad, want_grad, rtol=0, atol=0)


@pytest.mark.parametrize("B,H,S", SHAPES)
def test_packed_matches_fp32_reference(B, H, S):
    from adapcc_amd.ops.attention import flash_attention_qkv

    C = H * D
    qkv = make_qkv(B, H, S, seed=1).requires_grad_(True)
    g = torch.randn(B, S, C, device="cuda", dtype=torch.bfloat16)
    y = flash_attention_qkv(qkv, H)
    y.backward(g)
    ref_y, ref_grad = ref_packed_f32(qkv, H, g)
    torch.testing.assert_close(y.detach().float(), ref_y, rtol=2e-2,
                               atol=2e-2)
    assert_grads_close(qkv.grad, ref_grad, C)


def test_bwd_writes_delta():
    """fa_bwd fills its delta workspace with rowsum(dO*O). The bf16
    products are exact in fp32, so at most the summation order differs from
    torch's: per row |err| <= 64 * 2^-24 * sum|dO_i*O_i|. The kernel's own
    order is a fixed tree over adjacent elements, restated here with
    elementwise fp32 adds, which it must match bitwise."""
    from adapcc_amd.ops.fused import _core

    c = _core()
    B, H, S = 2, 3, 256
    torch.manual_seed(2)
    shape = (B, H, S, D)
    q, k, v, o, do = (torch.randn(shape, device="cuda", dtype=torch.bfloat16)
                      for _ in range(5))
    stream = torch.cuda.current_stream().cuda_stream
    scale = 1.0 / math.sqrt(D)
    s3 = [H * S * D, S * D, D]

    # a real logsumexp keeps the (unchecked) dq/dk/dv finite; O and dO are
    # the known random tensors above
    lse = torch.empty(B, H, S, device="cuda", dtype=torch.float32)
    o_fwd = torch.empty_like(q)
    c.fa_fwd(q.data_ptr(), k.data_ptr(), v.data_ptr(), o_fwd.data_ptr(),
             lse.data_ptr(), B, H, S, s3 * 4, scale, stream)

    delta = torch.full((B, H, S), float("nan"), device="cuda",
                       dtype=torch.float32)
    dq, dk, dv = (torch.empty_like(q) for _ in range(3))
    c.fa_bwd(q.data_ptr(), k.data_ptr(), v.data_ptr(), o.data_ptr(),
             do.data_ptr(), lse.data_ptr(), delta.data_ptr(), dq.data_ptr(),
             dk.data_ptr(), dv.data_ptr(), B, H, S, s3 * 8, scale, stream)
    torch.cuda.synchronize()

    prod = do.float() * o.float()
    want = prod.sum(-1)
    bound = 64 * 2.0 ** -24 * prod.abs().sum(-1)
    err = (delta - want).abs()
    print("delta max err", err.max().item(), "min bound", bound.min().item(),
          "max err/bound", (err / bound).max().item())
    assert torch.isfinite(delta).all()
    assert (err <= bound).all()

    tree = prod + 0.0
    while tree.shape[-1] > 1:
        tree = tree[..., 0::2] + tree[..., 1::2]
    torch.testing.assert_close(delta, tree.squeeze(-1), rtol=0, atol=0)


def test_expanded_dout():
    """y.sum().backward(): the upstream gradient is an expanded scalar."""
    from adapcc_amd.ops.attention import flash_attention_qkv

    B, H, S = 2, 3, 256
    C = H * D
    qkv = make_qkv(B, H, S, seed=3).requires_grad_(True)
    flash_attention_qkv(qkv, H).sum().backward()
    g = torch.ones(B, S, C, device="cuda", dtype=torch.bfloat16)
    _, ref_grad = ref_packed_f32(qkv, H, g)
    assert_grads_close(qkv.grad, ref_grad, C)


def test_transposed_slice_dout():
    """Upstream gradient that is a transposed slice of a larger tensor:
    rows contiguous and 16-B aligned, batch/row strides unrelated to
    [B,T,C], so the kernels read it in place."""
    from adapcc_amd.ops.attention import flash_attention_qkv

    B, H, S = 2, 3, 256
    C = H * D
    qkv = make_qkv(B, H, S, seed=4).requires_grad_(True)
    big = torch.randn(S + 3, B, 2 * C, device="cuda", dtype=torch.bfloat16)
    g = big[1:S + 1, :, 8:8 + C].transpose(0, 1)
    assert g.shape == (B, S, C) and not g.is_contiguous()
    flash_attention_qkv(qkv, H).backward(g)
    _, ref_grad = ref_packed_f32(qkv, H, g)
    assert_grads_close(qkv.grad, ref_grad, C)


def _sdpa_packed(qkv, H):
    C = qkv.shape[2] // 3
    q, k, v = (heads(t, H) for t in qkv.split(C, dim=2))
    return unheads(torch.nn.functional.scaled_dot_product_attention(
        q, k, v, is_causal=True))


@pytest.mark.parametrize("case", ["fp32", "T192", "offset4"])
def test_fallbacks(case, monkeypatch):
    from adapcc_amd.ops import attention

    B, H = 2, 3
    C = H * D
    torch.manual_seed(5)
    if case == "fp32":
        qkv = torch.randn(B, 128, 3 * C, device="cuda")
    elif case == "T192":
        qkv = torch.randn(B, 192, 3 * C, device="cuda", dtype=torch.bfloat16)
    else:
        base = torch.randn(B * 128 * 3 * C + 4, device="cuda",
                           dtype=torch.bfloat16)
        qkv = base[4:].view(B, 128, 3 * C)
        assert qkv.storage_offset() == 4 and qkv.is_contiguous()
    assert not attention.fa_qkv_supported(qkv, H, 0.0)

    def no_kernel(*a, **kw):
        raise AssertionError("fast path taken")

    monkeypatch.setattr(attention, "_launch_fwd", no_kernel)
    out = attention.flash_attention_qkv(qkv, H)
    assert out.shape == (B, qkv.shape[1], C)
    torch.testing.assert_close(out, _sdpa_packed(qkv, H), rtol=1e-2,
                               atol=1e-2)


def test_graph_capture_replays_bitwise():
    from adapcc_amd.ops.attention import flash_attention_qkv

    B, H, S = 2, 3, 256
    C = H * D
    qkv = make_qkv(B, H, S, seed=6).requires_grad_(True)
    g = torch.randn(B, S, C, device="cuda", dtype=torch.bfloat16)

    def fwd_bwd(x, gy):
        y = flash_attention_qkv(x, H)
        (gx,) = torch.autograd.grad(y, x, gy)
        return y, gx

    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        for _ in range(2):
            fwd_bwd(qkv, g)
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()

    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        y, gx = fwd_bwd(qkv, g)

    for seed in (7, 8):
        new_qkv = make_qkv(B, H, S, seed=seed)
        new_g = torch.randn(B, S, C, device="cuda", dtype=torch.bfloat16)
        with torch.no_grad():
            qkv.copy_(new_qkv)
            g.copy_(new_g)
        graph.replay()
        torch.cuda.synchronize()
        want_y, want_gx = fwd_bwd(new_qkv.requires_grad_(True), new_g)
        torch.testing.assert_close(y.detach(), want_y.detach(), rtol=0,
                                   atol=0)
        torch.testing.assert_close(gx, want_gx, rtol=0, atol=0)


def _two_layer_d64():
    from adapcc_amd.models.gpt2 import GPT2Config

    return GPT2Config(vocab_size=2048, n_positions=256, n_embd=128,
                      n_layer=2, n_head=2)


def _tiny():
    from adapcc_amd.models.gpt2 import GPT2Config

    return GPT2Config.tiny()


@pytest.mark.parametrize("make_cfg,fast", [(_tiny, False),
                                           (_two_layer_d64, True)])
def test_model_matches_old_composition(make_cfg, fast, monkeypatch):
    """One fwd+bwd of GPT-2 in bf16 against the same model with
    flash_attention_qkv replaced by split/views/flash_attention/contiguous.
    The forward is arithmetically identical; in the backward only delta's
    summation order differs."""
    from adapcc_amd.models.gpt2 import GPT2
    from adapcc_amd.ops import attention

    cfg = make_cfg()
    torch.manual_seed(9)
    model = GPT2(cfg).to("cuda").to(torch.bfloat16)
    T = cfg.n_positions
    data = torch.randint(0, cfg.vocab_size, (2, T + 1), device="cuda")
    x, t = data[:, :-1], data[:, 1:].contiguous()

    packed_calls = []
    real_apply = attention._FlashAttnQkvFn.apply

    def counting_apply(*a):
        packed_calls.append(1)
        return real_apply(*a)

    monkeypatch.setattr(attention._FlashAttnQkvFn, "apply", counting_apply)

    def run():
        for p in model.parameters():
            p.grad = None
        _, loss = model(x, t)
        loss.backward()
        return loss.detach().clone(), [p.grad.clone()
                                       for p in model.parameters()]

    loss_new, grads_new = run()
    assert len(packed_calls) == (cfg.n_layer if fast else 0)
    monkeypatch.setattr(attention, "flash_attention_qkv",
                        attention._attention_qkv_composed)
    loss_old, grads_old = run()
    assert len(packed_calls) == (cfg.n_layer if fast else 0)

    torch.testing.assert_close(loss_new, loss_old, rtol=0, atol=0)
    for (name, _), a, b in zip(model.named_parameters(), grads_new,
                               grads_old):
        torch.testing.assert_close(a, b, msg=lambda m: f"{name}: {m}")
