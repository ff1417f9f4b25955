"""Grouped-query / multi-query attention (k, v with Hk < H heads, H % Hk ==
0), the parts that need no GPU: the torch fallbacks of the four entry
points against the fp32 reference on K/V repeated to H heads (whose
autograd makes the reference dk, dv the group sums), the packed
(H + 2*Hk)*D layout, the argument checks, and GPT-2 with n_kv_head."""

import dataclasses
import math

import pytest
import torch

from attn_util import ref_attention_f32

D = 64
SCALE = 1.0 / math.sqrt(D)
TOL = dict(rtol=1e-5, atol=1e-5)  # that of the other CPU fallback tests


def gqa_reference(q, k, v, causal):
    """[B,H,S,D] q, [B,Hk,S,D] k, v -> fp32 o; differentiable."""
    G = q.shape[1] // k.shape[1]
    return ref_attention_f32(q, k.repeat_interleave(G, dim=1),
                             v.repeat_interleave(G, dim=1), SCALE, causal)


def leaves(*ts):
    return [t.detach().clone().requires_grad_(True) for t in ts]


def assert_grads(got, want, **tol):
    for name, a, b in zip(("dq", "dk", "dv"), got, want):
        assert a.grad.shape == a.shape
        torch.testing.assert_close(a.grad, b.grad,
                                   msg=lambda m, n=name: f"{n}: {m}", **tol)


# ---------------------------------------------------------------------------
# 1. fixed-length fallback
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("causal", [True, False])
@pytest.mark.parametrize("Hk", [2, 1])
def test_fixed_fallback(Hk, causal):
    from adapcc_amd.ops.attention import flash_attention

    torch.manual_seed(0)
    q = torch.randn(2, 4, 65, D)
    k, v = torch.randn(2, Hk, 65, D), torch.randn(2, Hk, 65, D)
    g = torch.randn(2, 4, 65, D)
    a, b = leaves(q, k, v), leaves(q, k, v)
    o = flash_attention(*a, causal=causal)
    assert o.shape == q.shape
    o.backward(g)
    ref = gqa_reference(*b, causal)
    ref.backward(g)
    torch.testing.assert_close(o.detach(), ref.detach(), **TOL)
    assert a[1].grad.shape == k.shape and a[2].grad.shape == v.shape
    assert_grads(a, b, **TOL)


# ---------------------------------------------------------------------------
# 2. packed fallback
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("causal", [True, False])
def test_packed_fallback(causal):
    from adapcc_amd.ops.attention import flash_attention, flash_attention_qkv

    H, Hk = 4, 2
    torch.manual_seed(1)
    qkv = torch.randn(2, 65, (H + 2 * Hk) * D)
    g = torch.randn(2, 65, H * D)

    x0 = qkv.clone().requires_grad_(True)
    y = flash_attention_qkv(x0, H, causal=causal, n_kv_head=Hk)
    assert y.shape == (2, 65, 256)
    y.backward(g)
    assert x0.grad.shape == qkv.shape

    x1 = qkv.clone().requires_grad_(True)
    q = x1[..., :H * D].view(2, 65, H, D).transpose(1, 2)
    k = x1[..., H * D:(H + Hk) * D].view(2, 65, Hk, D).transpose(1, 2)
    v = x1[..., (H + Hk) * D:].view(2, 65, Hk, D).transpose(1, 2)
    want = flash_attention(q, k, v, causal=causal)
    want = want.transpose(1, 2).reshape(2, 65, H * D)
    want.backward(g)
    torch.testing.assert_close(y.detach(), want.detach(), rtol=0, atol=0)
    torch.testing.assert_close(x0.grad, x1.grad, rtol=0, atol=0)


# ---------------------------------------------------------------------------
# 3. variable-length fallback
# ---------------------------------------------------------------------------
LENS = [1, 33, 64, 65, 0, 129]
TOTAL = sum(LENS)


def cu_of(lens):
    cu = [0]
    for n in lens:
        cu.append(cu[-1] + n)
    return torch.tensor(cu, dtype=torch.int32)


def per_sequence_reference(q, k, v, lens, causal):
    """gqa_reference on each sequence by itself; [total,H,D] q, out."""
    out = []
    cu = cu_of(lens).tolist()
    for a, b in zip(cu[:-1], cu[1:]):
        if b > a:
            qs, ks, vs = (t[a:b].transpose(0, 1)[None] for t in (q, k, v))
            out.append(gqa_reference(qs, ks, vs, causal)[0].transpose(0, 1))
    return torch.cat(out)


@pytest.mark.parametrize("causal", [True, False])
def test_varlen_fallback(causal):
    from adapcc_amd.ops.attention import flash_attention_varlen

    H, Hk = 4, 2
    torch.manual_seed(2)
    q = torch.randn(TOTAL, H, D)
    k, v = torch.randn(TOTAL, Hk, D), torch.randn(TOTAL, Hk, D)
    g = torch.randn(TOTAL, H, D)
    a, b = leaves(q, k, v), leaves(q, k, v)
    o = flash_attention_varlen(*a, cu_of(LENS), causal=causal)
    assert o.shape == (TOTAL, H, D)
    o.backward(g)
    ref = per_sequence_reference(*b, LENS, causal)
    ref.backward(g)
    torch.testing.assert_close(o.detach(), ref.detach(), **TOL)
    assert_grads(a, b, **TOL)


@pytest.mark.parametrize("causal", [True, False])
def test_varlen_packed_fallback(causal):
    from adapcc_amd.ops.attention import flash_attention_qkv_varlen

    H, Hk = 4, 2
    torch.manual_seed(3)
    qkv = torch.randn(TOTAL, (H + 2 * Hk) * D)
    g = torch.randn(TOTAL, H * D)
    x0 = qkv.clone().requires_grad_(True)
    y = flash_attention_qkv_varlen(x0, H, cu_of(LENS), causal=causal,
                                   n_kv_head=Hk)
    assert y.shape == (TOTAL, H * D)
    y.backward(g)
    assert x0.grad.shape == qkv.shape

    x1 = qkv.clone().requires_grad_(True)
    q = x1[:, :H * D].view(TOTAL, H, D)
    k = x1[:, H * D:(H + Hk) * D].view(TOTAL, Hk, D)
    v = x1[:, (H + Hk) * D:].view(TOTAL, Hk, D)
    ref = per_sequence_reference(q, k, v, LENS, causal).reshape(TOTAL, H * D)
    ref.backward(g)
    torch.testing.assert_close(y.detach(), ref.detach(), **TOL)
    torch.testing.assert_close(x0.grad, x1.grad, **TOL)


# ---------------------------------------------------------------------------
# 4. errors
# ---------------------------------------------------------------------------
def test_heads_that_do_not_divide():
    from adapcc_amd.ops.attention import (flash_attention,
                                          flash_attention_qkv,
                                          flash_attention_qkv_varlen,
                                          flash_attention_varlen)

    H, Hk = 4, 3
    q, k = torch.randn(2, H, 65, D), torch.randn(2, Hk, 65, D)
    with pytest.raises(ValueError):
        flash_attention(q, k, k)
    with pytest.raises(ValueError):
        flash_attention_qkv(torch.randn(2, 65, (H + 2 * Hk) * D), H,
                            n_kv_head=Hk)
    cu = cu_of(LENS)
    q, k = torch.randn(TOTAL, H, D), torch.randn(TOTAL, Hk, D)
    with pytest.raises(ValueError):
        flash_attention_varlen(q, k, k, cu)
    with pytest.raises(ValueError):
        flash_attention_qkv_varlen(torch.randn(TOTAL, (H + 2 * Hk) * D), H,
                                   cu, n_kv_head=Hk)


def test_k_and_v_of_different_head_counts():
    from adapcc_amd.ops.attention import (flash_attention,
                                          flash_attention_varlen)

    q, k, v = (torch.randn(2, h, 65, D) for h in (4, 2, 1))
    with pytest.raises(ValueError):
        flash_attention(q, k, v)
    with pytest.raises(ValueError):
        flash_attention(q, q, k)
    q, k, v = (torch.randn(TOTAL, h, D) for h in (4, 2, 1))
    with pytest.raises(ValueError):
        flash_attention_varlen(q, k, v, cu_of(LENS))
    with pytest.raises(ValueError):
        flash_attention_varlen(q, q, k, cu_of(LENS))


def test_not_supported_on_cpu():
    from adapcc_amd.ops.attention import (fa_qkv_supported,
                                          fa_qkv_varlen_supported,
                                          fa_supported, fa_varlen_supported)

    q = torch.randn(2, 4, 128, D, dtype=torch.bfloat16)
    k = torch.randn(2, 2, 128, D, dtype=torch.bfloat16)
    assert not fa_supported(q, k, k, True, 0.0)
    assert not fa_varlen_supported(q[0].transpose(0, 1), k[0].transpose(0, 1),
                                   k[0].transpose(0, 1), cu_of([128]), True,
                                   0.0)
    qkv = torch.randn(2, 128, 8 * D, dtype=torch.bfloat16)
    assert not fa_qkv_supported(qkv, 4, 0.0, n_kv_head=2)
    assert not fa_qkv_varlen_supported(qkv[0], 4, cu_of([128]), 0.0,
                                       n_kv_head=2)


# ---------------------------------------------------------------------------
# 5, 6. GPT-2
# ---------------------------------------------------------------------------
def tiny_model(n_kv_head, seed=4):
    from adapcc_amd.models.gpt2 import GPT2, GPT2Config

    cfg = dataclasses.replace(GPT2Config.tiny(), n_kv_head=n_kv_head)
    torch.manual_seed(seed)
    return GPT2(cfg).eval()


def expand_kv_state(sd, H, Hk, hd):
    """The state_dict of the n_kv_head = H model that computes what the
    n_kv_head = Hk model with `sd` computes: the K and V row blocks of each
    K/V head of c_attn repeated G times."""
    G = H // Hk
    out = {}
    for name, t in sd.items():
        if ".c_attn." in name:
            q, k, v = t.split([H * hd, Hk * hd, Hk * hd], dim=0)
            k, v = (x.view(Hk, hd, *x.shape[1:]).repeat_interleave(G, dim=0)
                    .reshape(H * hd, *x.shape[1:]) for x in (k, v))
            t = torch.cat([q, k, v], dim=0)
        out[name] = t.clone()
    return out


def test_gpt2_default_config_unchanged():
    a, b = tiny_model(None), tiny_model(4, seed=5)
    sa, sb = a.state_dict(), b.state_dict()
    assert list(sa) == list(sb)
    assert all(sa[n].shape == sb[n].shape for n in sa)
    assert sa["h.0.attn.c_attn.weight"].shape == (3 * 128, 128)
    b.load_state_dict(sa)
    idx = torch.randint(0, a.cfg.vocab_size, (2, 65))
    with torch.no_grad():
        la, lb = a(idx)[0], b(idx)[0]
    torch.testing.assert_close(la, lb, rtol=0, atol=0)


def test_gpt2_grouped_config():
    g = tiny_model(2)
    w = [t for n, t in g.state_dict().items() if n.endswith("c_attn.weight")]
    assert w and all(t.shape == ((4 + 4) * 32, 128) for t in w)
    full = tiny_model(4, seed=6)
    full.load_state_dict(expand_kv_state(g.state_dict(), 4, 2, 32))
    idx = torch.randint(0, g.cfg.vocab_size, (2, 65))
    lg = g(idx)[0]
    with torch.no_grad():
        lf = full(idx)[0]
    torch.testing.assert_close(lg.detach(), lf, **TOL)
    lg.float().square().mean().backward()
    grads = [p.grad for n, p in g.named_parameters() if "c_attn" in n]
    assert grads and all(x is not None and torch.isfinite(x).all()
                         for x in grads)
