"""Attention dropout, the parts that need no GPU: the torch replica of the
kernels' keep(seed, bh, q, k) mask (ops/attention.py, csrc/attn_drop.h) is
statistically a Bernoulli(1-p) field with no visible structure along keys,
queries, planes or seeds, has the exact properties the kernels rely on, and
the CPU fallback and the ViT config behave.

Every count below is compared with its binomial expectation n*pi at
6 * sqrt(n*pi*(1-pi)). Overlapping pairs and blocks are not independent
trials, which moves the true deviation by a factor close to 1; six standard
deviations of a correct generator fail about once in 5e8 counts, and the
test takes ~4e3 of them."""

import math

import pytest
import torch

SEED = 1234
B, H = 2, 3          # B*H = 6 planes, not a power of two
SIGMAS = 6.0


def _mask(seed, S, p):
    from adapcc_amd.ops.attention import dropout_keep_mask_reference

    return dropout_keep_mask_reference(seed, B, H, S, p)


def _check(name, count, n, pi):
    """count: tensor of counts, each out of n trials of probability pi."""
    mean = n * pi
    sd = math.sqrt(n * pi * (1.0 - pi))
    dev = ((count.double() - mean).abs() / sd).max().item()
    print(f"{name}: n={n} worst {dev:.2f} sigma")
    assert dev <= SIGMAS, f"{name}: {dev:.2f} sigma"


@pytest.mark.parametrize("p", [0.1, 0.5])
@pytest.mark.parametrize("S", [197, 256])
def test_replica_statistics(S, p):
    m = _mask(SEED, S, p)
    assert m.shape == (B, H, S, S) and m.dtype == torch.bool
    m = m.view(B * H, S, S)
    k = 1.0 - p
    _check("total", m.sum(), m.numel(), k)
    _check("rows", m.sum(dim=2), S, k)
    _check("columns", m.sum(dim=1), S, k)
    _check("planes", m.sum(dim=(1, 2)), S * S, k)
    along_k = m[:, :, 1:] & m[:, :, :-1]
    _check("pairs along k", along_k.sum(), along_k.numel(), k ** 2)
    along_q = m[:, 1:, :] & m[:, :-1, :]
    _check("pairs along q", along_q.sum(), along_q.numel(), k ** 2)
    across = m[1:] & m[:-1]
    _check("pairs across planes", across.sum(), across.numel(), k ** 2)
    blocks = along_k[:, 1:, :] & along_k[:, :-1, :]
    _check("2x2 blocks", blocks.sum(), blocks.numel(), k ** 4)
    both = m & _mask(SEED + 1, S, p).view(B * H, S, S)
    _check("kept under both seeds", both.sum(), both.numel(), k ** 2)


def test_replica_exact_properties():
    S = 197
    m1 = _mask(SEED, S, 0.1)
    assert torch.equal(m1, _mask(SEED, S, 0.1))
    # one word, two thresholds: what p = 0.5 keeps, p = 0.1 keeps
    m5 = _mask(SEED, S, 0.5)
    assert (m1 | ~m5).all()
    assert (m1 & ~m5).any()
    # planes draw different masks, across heads and across batch entries
    planes = m1.view(B * H, S, S)
    for i in range(B * H):
        for j in range(i + 1, B * H):
            assert not torch.equal(planes[i], planes[j])
    # a tensor seed is the same seed, and the high word matters
    assert torch.equal(m1, _mask(torch.tensor([SEED]), S, 0.1))
    assert not torch.equal(m1, _mask(SEED + (1 << 32), S, 0.1))
    # the plane index is b*H + h, whatever the split
    from adapcc_amd.ops.attention import dropout_keep_mask_reference

    other = dropout_keep_mask_reference(SEED, 3, 2, S, 0.1)
    assert torch.equal(other.view(6, S, S), planes)


def test_threshold():
    from adapcc_amd.ops.attention import _drop_threshold

    assert _drop_threshold(0.5) == 1 << 31
    assert _drop_threshold(0.1) == round(0.1 * 2 ** 32)
    assert _drop_threshold(0.0) == 1
    assert _drop_threshold(1.0 - 2.0 ** -40) == 2 ** 32 - 1


def test_public_mask_on_cpu_is_replica():
    from adapcc_amd.ops.attention import fa_dropout_mask

    got = fa_dropout_mask(torch.tensor([SEED]), B, H, 65, 0.1)
    assert got.dtype == torch.bool
    assert torch.equal(got, _mask(SEED, 65, 0.1))
    with pytest.raises(ValueError):
        fa_dropout_mask(SEED, B, H, 65, 1.0)


def test_cpu_fallback_runs_with_dropout():
    from adapcc_amd.ops.attention import (fa_qkv_supported, fa_supported,
                                          flash_attention,
                                          flash_attention_qkv)

    torch.manual_seed(0)
    q, k, v = (torch.randn(1, 2, 16, 64, requires_grad=True)
               for _ in range(3))
    assert not fa_supported(q, k, v, True, 0.1)
    o = flash_attention(q, k, v, causal=True, dropout_p=0.1)
    assert o.shape == q.shape and torch.isfinite(o).all()
    o.sum().backward()
    assert torch.isfinite(q.grad).all()

    qkv = torch.randn(1, 16, 3 * 128)
    assert not fa_qkv_supported(qkv, 2, 0.1)
    y = flash_attention_qkv(qkv, 2, dropout_p=0.1, causal=False)
    assert y.shape == (1, 16, 128) and torch.isfinite(y).all()


def test_gate_takes_dropout_below_one(monkeypatch):
    """Device and extension aside, the gate's dropout rule: 0 <= p < 1."""
    from adapcc_amd.ops import attention

    class FakeBf16Cuda:
        is_cuda = True
        dtype = torch.bfloat16

    monkeypatch.setattr(attention, "_core", lambda: True)
    ok = attention._kernel_ok
    assert ok(FakeBf16Cuda(), 64, 128, True, 0.0)
    assert ok(FakeBf16Cuda(), 64, 128, True, 0.1)
    assert ok(FakeBf16Cuda(), 64, 197, False, 0.5)
    assert not ok(FakeBf16Cuda(), 64, 128, True, 1.0)
    assert not ok(FakeBf16Cuda(), 64, 128, True, -0.1)


def test_vit_config_attn_dropout():
    from adapcc_amd.models.vit import ViT, ViTConfig

    assert ViTConfig().attn_dropout == 0
    cfgs = [ViTConfig(image_size=16, patch_size=8, num_classes=5, dim=32,
                      depth=1, heads=2, mlp_dim=64, attn_dropout=p)
            for p in (0.0, 0.5)]
    outs = []
    x = torch.randn(2, 3, 16, 16)
    for cfg in cfgs:
        torch.manual_seed(1)
        model = ViT(cfg).eval()
        assert model.blocks[0].attn_dropout == cfg.attn_dropout
        with torch.no_grad():
            outs.append(model(x))
    torch.testing.assert_close(outs[0], outs[1], rtol=0, atol=0)
    # and in training it is passed on: the output moves
    torch.manual_seed(1)
    model = ViT(cfgs[1]).train()
    with torch.no_grad():
        assert not torch.equal(model(x), outs[1])
