"""flash_attention_qkv on the CPU: always the composed fallback."""

import torch


def test_flash_attention_qkv_cpu_fallback():
    from adapcc_amd.ops.attention import fa_qkv_supported, flash_attention_qkv

    B, T, H, D = 2, 128, 3, 64
    C = H * D
    torch.manual_seed(0)
    qkv = torch.randn(B, T, 3 * C, requires_grad=True)
    assert not fa_qkv_supported(qkv, H, 0.0)
    y = flash_attention_qkv(qkv, H)
    assert y.shape == (B, T, C)

    q, k, v = (t.view(B, T, H, D).transpose(1, 2)
               for t in qkv.detach().split(C, dim=2))
    ref = torch.nn.functional.scaled_dot_product_attention(
        q, k, v, is_causal=True).transpose(1, 2).reshape(B, T, C)
    torch.testing.assert_close(y.detach(), ref, rtol=1e-2, atol=1e-2)

    y.sum().backward()
    assert qkv.grad.shape == qkv.shape
    assert torch.isfinite(qkv.grad).all()
