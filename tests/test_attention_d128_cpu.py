"""Head dimension 128 of the flash attention, the parts that need no GPU:
the gate (ops/attention.py: _kernel_ok) takes 64 and 128 and nothing else,
the four public predicates are false off the GPU, the fallbacks compute
attention at that width, and MoETransformerBlock(fused_attention=True) is the
default block computed another way."""

import math

import pytest
import torch

from attn_util import heads, ref_attention_f32, unheads

D = 128
SCALE = 1.0 / math.sqrt(D)


class FakeBf16Cuda:
    is_cuda = True
    dtype = torch.bfloat16


def test_gate_takes_head_dim_64_and_128(monkeypatch):
    from adapcc_amd.ops import attention

    monkeypatch.setattr(attention, "_core", lambda: True)
    ok = attention._kernel_ok
    assert ok(FakeBf16Cuda(), 128, 128, True, 0.0)
    assert ok(FakeBf16Cuda(), 128, 197, False, 0.0)
    assert ok(FakeBf16Cuda(), 128, 128, True, 0.1)
    assert ok(FakeBf16Cuda(), 128, 197, False, 0.1)
    assert ok(FakeBf16Cuda(), 64, 128, True, 0.1)
    for d in (32, 96, 256):
        assert not ok(FakeBf16Cuda(), d, 128, True, 0.0), d
        assert not ok(FakeBf16Cuda(), d, 197, False, 0.0), d
    assert not ok(FakeBf16Cuda(), 128, 192, True, 0.0)
    assert not ok(FakeBf16Cuda(), 128, 128, True, 1.0)
    # and still needs the extension
    monkeypatch.setattr(attention, "_core", lambda: None)
    assert not ok(FakeBf16Cuda(), 128, 128, True, 0.0)


def test_predicates_false_on_cpu():
    from adapcc_amd.ops.attention import (fa_qkv_supported,
                                          fa_qkv_varlen_supported,
                                          fa_supported, fa_varlen_supported)

    H, S = 2, 128
    q = torch.randn(1, H, S, D, dtype=torch.bfloat16)
    assert not fa_supported(q, q, q, True, 0.0)
    qkv = torch.randn(1, S, 3 * H * D, dtype=torch.bfloat16)
    assert not fa_qkv_supported(qkv, H, 0.0)
    cu = torch.tensor([0, 65, S], dtype=torch.int32)
    t = torch.randn(S, H, D, dtype=torch.bfloat16)
    assert not fa_varlen_supported(t, t, t, cu, True, 0.0)
    assert not fa_qkv_varlen_supported(qkv[0], H, cu, 0.0)


@pytest.mark.parametrize("causal", [True, False])
def test_qkv_fallback_matches_reference(causal):
    from adapcc_amd.ops.attention import flash_attention_qkv

    torch.manual_seed(0)
    B, H, T = 2, 2, 65
    C = H * D
    qkv = torch.randn(B, T, 3 * C)
    y = flash_attention_qkv(qkv, H, causal=causal)
    q, k, v = (heads(t, H) for t in qkv.split(C, dim=2))
    want = unheads(ref_attention_f32(q, k, v, SCALE, causal))
    assert y.shape == (B, T, C)
    torch.testing.assert_close(y, want, rtol=1e-5, atol=1e-5)


@pytest.mark.parametrize("causal", [True, False])
def test_qkv_varlen_fallback_matches_reference_per_sequence(causal):
    from adapcc_amd.ops.attention import flash_attention_qkv_varlen

    torch.manual_seed(1)
    H = 2
    C = H * D
    lens = [1, 65, 0, 33]
    cu = [0]
    for n in lens:
        cu.append(cu[-1] + n)
    total = cu[-1]
    qkv = torch.randn(total, 3 * C)
    y = flash_attention_qkv_varlen(qkv, H, torch.tensor(cu, dtype=torch.int32),
                                   causal=causal)
    assert y.shape == (total, C)
    for a, b in zip(cu[:-1], cu[1:]):
        if b == a:
            continue
        q, k, v = (heads(t[None], H) for t in qkv[a:b].split(C, dim=1))
        want = unheads(ref_attention_f32(q, k, v, SCALE, causal))[0]
        torch.testing.assert_close(y[a:b], want, rtol=1e-5, atol=1e-5)


def _blocks(seed=3):
    """The default block and the fused one, constructed from one seed."""
    from adapcc_amd.models.moe import MoETransformerBlock

    kw = dict(d_model=256, n_head=2, d_hidden=512, num_local_experts=2)
    torch.manual_seed(seed)
    plain = MoETransformerBlock(**kw)
    torch.manual_seed(seed)
    explicit = MoETransformerBlock(fused_attention=False, **kw)
    torch.manual_seed(seed)
    fused = MoETransformerBlock(fused_attention=True, **kw)
    return plain, explicit, fused


def test_moe_block_fused_attention_matches_default():
    plain, _, fused = _blocks()
    assert list(fused.state_dict().keys()) == list(plain.state_dict().keys())
    fused.load_state_dict(plain.state_dict())
    plain.eval()
    fused.eval()
    torch.manual_seed(4)
    x = torch.randn(2, 65, 256)
    with torch.no_grad():
        want = plain(x)
        got = fused(x)
    torch.testing.assert_close(got, want, rtol=1e-5, atol=1e-5)


def test_moe_block_default_unchanged():
    """Without the argument and with fused_attention=False the block is one
    and the same: same parameters from the same seed, same output bits."""
    plain, explicit, _ = _blocks()
    for (na, a), (nb, b) in zip(plain.state_dict().items(),
                                explicit.state_dict().items()):
        assert na == nb and torch.equal(a, b), na
    plain.eval()
    explicit.eval()
    torch.manual_seed(5)
    x = torch.randn(2, 65, 256)
    with torch.no_grad():
        torch.testing.assert_close(explicit(x), plain(x), rtol=0, atol=0)
    # what the default block computes: nn.MultiheadAttention itself
    with torch.no_grad():
        h = plain.ln1(x)
        a, _ = plain.attn(h, h, h, need_weights=False)
        y = x + a
        y = y + plain.moe(plain.ln2(y))
        torch.testing.assert_close(plain(x), y, rtol=0, atol=0)
