"""The non-causal attention interface on the CPU: never the kernels, always
the SDPA composition, and the ViT that is built on it."""

import torch
import torch.nn.functional as F


def _heads(t, H):
    B, T, C = t.shape
    return t.view(B, T, H, C // H).transpose(1, 2)


def test_fa_supported_noncausal_false_on_cpu():
    from adapcc_amd.ops.attention import fa_qkv_supported, fa_supported

    q = torch.randn(2, 3, 197, 64, dtype=torch.bfloat16)
    assert not fa_supported(q, q.clone(), q.clone(), False, 0.0)
    qkv = torch.randn(2, 197, 3 * 3 * 64, dtype=torch.bfloat16)
    assert not fa_qkv_supported(qkv, 3, 0.0, causal=False)


def test_flash_attention_qkv_noncausal_cpu_is_sdpa():
    from adapcc_amd.ops.attention import flash_attention_qkv

    torch.manual_seed(0)
    B, T, H, D = 2, 37, 3, 16
    C = H * D
    qkv = torch.randn(B, T, 3 * C, requires_grad=True)
    y = flash_attention_qkv(qkv, H, causal=False)
    assert y.shape == (B, T, C)
    q, k, v = (_heads(t, H) for t in qkv.split(C, dim=2))
    ref = F.scaled_dot_product_attention(q, k, v)
    ref = ref.transpose(1, 2).reshape(B, T, C)
    torch.testing.assert_close(y, ref)
    # and it differs from the causal result, which stays the default
    y_causal = flash_attention_qkv(qkv, H)
    assert not torch.allclose(y, y_causal)
    y.sum().backward()
    assert torch.isfinite(qkv.grad).all()


def test_vit_tiny_cpu_matches_explicit_sdpa():
    from adapcc_amd.models.vit import ViT, ViTConfig

    torch.manual_seed(1)
    cfg = ViTConfig.tiny()
    model = ViT(cfg)
    images = torch.randn(2, 3, cfg.image_size, cfg.image_size)

    def block(blk, x):
        B, T, C = x.shape
        h = blk.ln1(x)
        q, k, v = (_heads(t, blk.heads) for t in blk.qkv(h).split(C, dim=2))
        a = F.scaled_dot_product_attention(q, k, v)
        a = a.transpose(1, 2).contiguous().view(B, T, C)
        x = x + blk.proj(a)
        return x + blk.mlp(blk.ln2(x))

    with torch.no_grad():
        got = model(images)
        x = model.patch(images).flatten(2).transpose(1, 2)
        cls = model.cls_token.expand(x.shape[0], -1, -1)
        x = torch.cat([cls, x], dim=1) + model.pos
        for blk in model.blocks:
            x = block(blk, x)
        want = model.head(model.ln(x[:, 0]))
    assert got.shape == (2, cfg.num_classes)
    torch.testing.assert_close(got, want)
