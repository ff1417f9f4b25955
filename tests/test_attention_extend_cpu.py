"""flash_attention_extend off the kernel path (fp32 on the CPU): the composed
route against the per-sequence reference, the cache after the append, the
argument errors, and Sq == 1 against ``flash_attention_decode``."""

import pytest
import torch

from attn_decode_ref import decode_reference
from attn_extend_ref import extend_reference

from adapcc_amd.ops.attention import (fa_extend_supported,
                                      flash_attention_decode,
                                      flash_attention_extend)

TOL = dict(rtol=1e-5, atol=1e-5)
B, H, HK, SQ, SMAX, D = 5, 4, 2, 6, 16, 8
# past 0, mid-cache, a cache too full for the chunk (twice), an empty one
PAST = [0, 5, 13, 16, 0]
Q_LENS = [6, 3, 6, 2, 0]          # n_b = 0 in the last sequence


def make(seed=0):
    torch.manual_seed(seed)
    q = torch.randn(B, H, SQ, D)
    k, v = torch.randn(2, B, HK, SMAX, D)
    kn, vn = torch.randn(2, B, HK, SQ, D)
    return q, k, v, kn, vn


def lens_t(x):
    return torch.tensor(x, dtype=torch.int32)


@pytest.mark.parametrize("causal", [True, False])
@pytest.mark.parametrize("new", [True, False])
@pytest.mark.parametrize("ragged", [True, False])
def test_composed_matches_reference(causal, new, ragged):
    """Without new rows and causal, total_b < n_b in sequences 0 and 4: rows
    there see no key and come out zero with lse -inf."""
    q, k, v, kn, vn = make()
    ql = Q_LENS if ragged else None
    kw = dict(k_new=kn, v_new=vn) if new else {}
    ref, ref_lse, ke, ve = extend_reference(q, k, v, PAST, q_lens=ql,
                                            causal=causal, **kw)
    past_t = lens_t(PAST)
    out, lse = flash_attention_extend(
        q, k, v, past_t, q_lens=None if ql is None else lens_t(ql),
        causal=causal, return_lse=True, **kw)
    torch.testing.assert_close(out, ref, **TOL)
    torch.testing.assert_close(lse, ref_lse, **TOL)
    assert torch.equal(k, ke) and torch.equal(v, ve)     # the append, exact
    assert past_t.tolist() == PAST
    assert out.transpose(1, 2).is_contiguous()
    if ragged:
        assert not out[4].any() and (lse[4] == float("-inf")).all()
        assert not out[1, :, 3:].any()
    if causal and not new:
        assert not out[0].any() and (lse[0] == float("-inf")).all()


def test_nan_in_padding_does_not_leak():
    q, k, v, kn, vn = make(1)
    past = [0, 5, 9, 2, 0]
    for b, (p, n) in enumerate(zip(past, Q_LENS)):
        k[b, :, p + n:] = v[b, :, p + n:] = float("nan")
        q[b, :, n:] = kn[b, :, n:] = vn[b, :, n:] = float("nan")
    ref = extend_reference(q, k, v, past, kn, vn, Q_LENS)[0]
    out = flash_attention_extend(q, k, v, lens_t(past), kn, vn,
                                 lens_t(Q_LENS))
    assert torch.isfinite(out).all()
    torch.testing.assert_close(out, ref, **TOL)


def test_one_row_is_decode():
    q, k, v, kn, vn = make(2)
    q, kn, vn = q[:, :, :1], kn[:, :, :1], vn[:, :, :1]
    k2, v2 = k.clone(), v.clone()
    out, lse = flash_attention_extend(q, k, v, lens_t(PAST), kn, vn,
                                      return_lse=True)
    k0, v0 = k2.clone(), v2.clone()
    dec, dec_lse = flash_attention_decode(
        q[:, :, 0], k2, v2, lens_t(PAST), kn[:, :, 0], vn[:, :, 0],
        return_lse=True)
    # the two public calls, bit for bit: output, lse and both caches
    assert dec.shape == (B, H, D) and dec.is_contiguous()
    assert torch.equal(out[:, :, 0], dec)
    assert torch.equal(lse[:, :, 0], dec_lse)
    assert torch.equal(k, k2) and torch.equal(v, v2)
    # both leave a full cache (sequence 3) alone
    assert torch.equal(k[3], k0[3]) and torch.equal(v[3], v0[3])
    # and decode is right: the reference over the appended caches
    ref, ref_lse = decode_reference(q[:, :, 0], k2, v2,
                                    [min(p + 1, SMAX) for p in PAST])
    torch.testing.assert_close(dec, ref, **TOL)
    torch.testing.assert_close(dec_lse, ref_lse, **TOL)


def test_argument_errors():
    q, k, v, kn, vn = make(3)
    lt = lens_t(PAST)
    assert not fa_extend_supported(q, k, v, lt)          # fp32 on the CPU
    bad = [
        dict(q=q[:, :, 0]), dict(k_cache=k[:, :, :, :4]),
        dict(q=q[:, :3]), dict(v_cache=v.double()),
        dict(cache_seqlens=lt.long()), dict(cache_seqlens=lt[:2]),
        dict(q_lens=lt.long()), dict(q_lens=lt[:2]), dict(q_lens=[1] * B),
        dict(k_new=kn), dict(k_new=kn, v_new=vn[:, :, :2]),
        dict(k_new=kn.double(), v_new=vn),
    ]
    for change in bad:
        args = dict(q=q, k_cache=k, v_cache=v, cache_seqlens=lt)
        args.update(change)
        with pytest.raises(ValueError, match="flash_attention_extend"):
            flash_attention_extend(**args)
    with pytest.raises(RuntimeError, match="forward only"):
        flash_attention_extend(q.clone().requires_grad_(), k, v, lt)
