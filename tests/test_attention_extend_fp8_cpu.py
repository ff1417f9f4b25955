"""``flash_attention_extend`` over e4m3 caches off the kernel path (CPU, fp32
q): the composed route against ``extend_reference`` on the dequantised
caches, and the argument errors of the scales."""

import pytest
import torch

from attn_extend_ref import extend_reference

from adapcc_amd.ops.attention import (fa_extend_supported,
                                      flash_attention_extend,
                                      kv_quantize_reference)

F8 = torch.float8_e4m3fn


def make(B, H, Hk, Sq, Smax, D, seed=0):
    torch.manual_seed(seed)
    q = torch.randn(B, H, Sq, D)
    kf, vf = torch.randn(2, B, Hk, Smax, D)
    vf = vf * torch.arange(1, Hk + 1).view(1, Hk, 1, 1)
    ks, vs = (x.abs().amax(dim=(0, 2, 3)) / 448 for x in (kf, vf))
    return q, kv_quantize_reference(kf, ks), kv_quantize_reference(vf, vs), ks, vs


def deq(c, s):
    return c.float() * s.view(1, -1, 1, 1)


@pytest.mark.parametrize("append,ql,causal", [
    (False, None, True), (False, None, False), (True, None, True),
    (True, [5, 3, 0], True)])
def test_composed_route(append, ql, causal):
    B, H, Hk, Sq, Smax, D = 3, 4, 2, 5, 40, 16
    past = [0, 17, Smax - 2]
    q, k, v, ks, vs = make(B, H, Hk, Sq, Smax, D)
    lens = torch.tensor(past, dtype=torch.int32)
    qlt = None if ql is None else torch.tensor(ql, dtype=torch.int32)
    new = {}
    if append:
        new = dict(k_new=torch.randn(B, Hk, Sq, D), v_new=torch.randn(B, Hk, Sq, D))
    k0 = k.clone()
    assert not fa_extend_supported(q, k, v, lens, qlt, k_scale=ks, v_scale=vs)
    out, lse = flash_attention_extend(q, k, v, lens, q_lens=qlt, causal=causal,
                                      return_lse=True, k_scale=ks, v_scale=vs,
                                      **new)
    n = [Sq] * B if ql is None else ql
    total = [min(p + x, Smax) if append else p for p, x in zip(past, n)]
    if append:      # the stored rows are q8 of the new ones, nothing else moved
        want = k0.clone().view(torch.uint8)
        code = kv_quantize_reference(new["k_new"], ks).view(torch.uint8)
        for b in range(B):
            want[b, :, past[b]:total[b]] = code[b, :, :total[b] - past[b]]
        assert torch.equal(k.view(torch.uint8), want)
    ref, ref_lse, _, _ = extend_reference(q, deq(k, ks), deq(v, vs), total,
                                          q_lens=ql, causal=causal)
    torch.testing.assert_close(out, ref, rtol=1e-4, atol=1e-4)
    torch.testing.assert_close(lse, ref_lse, rtol=1e-4, atol=1e-4)


def test_scale_argument_errors():
    q, k, v, ks, vs = make(2, 4, 2, 3, 24, 16)
    lens = torch.tensor([3, 9], dtype=torch.int32)
    kb, vb = deq(k, ks), deq(v, vs)
    bad = [
        dict(k_cache=kb, v_cache=vb, k_scale=ks, v_scale=vs),  # not e4m3
        dict(k_cache=k, v_cache=v),                            # no scales
        dict(k_cache=k, v_cache=v, k_scale=ks),                # one only
        dict(k_cache=k, v_cache=v, k_scale=ks, v_scale=vs[:1]),
        dict(k_cache=k, v_cache=v, k_scale=ks.double(), v_scale=vs),
    ]
    for kw in bad:
        with pytest.raises(ValueError):
            flash_attention_extend(q, cache_seqlens=lens, **kw)
        assert not fa_extend_supported(q, kw["k_cache"], kw["v_cache"], lens,
                                       k_scale=kw.get("k_scale"),
                                       v_scale=kw.get("v_scale"))
