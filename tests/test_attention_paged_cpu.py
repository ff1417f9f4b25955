"""``block_table`` off the kernel path (fp32 on the CPU): the composed paged
route of flash_attention_extend and flash_attention_decode against the
per-sequence reference on the contiguous cache, the pools after the append,
and the argument errors."""

import pytest
import torch

from attn_extend_ref import extend_reference
from attn_paged_ref import repage, to_pages

from adapcc_amd.ops.attention import (fa_decode_supported,
                                      fa_extend_supported,
                                      flash_attention_decode,
                                      flash_attention_extend)

TOL = dict(rtol=1e-5, atol=1e-5)
B, H, HK, SQ, SMAX, D = 5, 4, 2, 6, 128, 8
# an empty cache, mid-page, across a page edge, too full for the chunk, full
PAST = [0, 5, 60, 125, 128]
Q_LENS = [6, 3, 6, 6, 0]


def make(seed=0):
    torch.manual_seed(seed)
    q = torch.randn(B, H, SQ, D)
    k, v = torch.randn(2, B, HK, SMAX, D)
    kn, vn = torch.randn(2, B, HK, SQ, D)
    return q, k, v, kn, vn


def lens_t(x):
    return torch.tensor(x, dtype=torch.int32)


def same_bits(a, b):    # NaN pages included
    return torch.equal(a.view(torch.int32), b.view(torch.int32))


@pytest.mark.parametrize("P", [16, 64])
@pytest.mark.parametrize("causal", [True, False])
@pytest.mark.parametrize("new", [True, False])
@pytest.mark.parametrize("decode", [False, True])
def test_composed_matches_reference(decode, new, causal, P):
    """decode: the first row of the block through flash_attention_decode
    (causal only)."""
    q, k, v, kn, vn = make(P)
    ql = Q_LENS
    if decode:
        q, kn, vn, ql, causal = q[:, :, :1], kn[:, :, :1], vn[:, :, :1], None, True
    kw = dict(k_new=kn, v_new=vn) if new else {}
    n = ql or [1] * B
    totals = [min(p + x, SMAX) if new else p for p, x in zip(PAST, n)]
    kp, vp, table = to_pages(k, v, P, seed=P, totals=totals)
    ref, ref_lse, ke, ve = extend_reference(q, k, v, PAST, q_lens=ql,
                                            causal=causal, **kw)
    past_t, table0 = lens_t(PAST), table.clone()
    if decode:
        assert not fa_decode_supported(q[:, :, 0], kp, vp, past_t,
                                       block_table=table)
        out, lse = flash_attention_decode(
            q[:, :, 0], kp, vp, past_t, return_lse=True, block_table=table,
            **{name: t[:, :, 0] for name, t in kw.items()})
        assert out.shape == (B, H, D) and out.is_contiguous()
        out, lse = out.unsqueeze(2), lse.unsqueeze(2)
    else:
        ql_t = lens_t(ql)
        assert not fa_extend_supported(q, kp, vp, past_t, ql_t,
                                       block_table=table)
        out, lse = flash_attention_extend(q, kp, vp, past_t, q_lens=ql_t,
                                          causal=causal, return_lse=True,
                                          block_table=table, **kw)
        assert ql_t.tolist() == Q_LENS
    torch.testing.assert_close(out, ref, **TOL)
    torch.testing.assert_close(lse, ref_lse, **TOL)
    # the appended rows in their pages, every other page (NaN) untouched
    assert same_bits(kp, repage(ke, table, P, totals))
    assert same_bits(vp, repage(ve, table, P, totals))
    assert past_t.tolist() == PAST and torch.equal(table, table0)


def test_argument_errors():
    q, k, v, kn, vn = make(3)
    kp, vp, table = to_pages(k, v, 16)
    lt = lens_t(PAST)
    bad = [
        dict(block_table=table.long()), dict(block_table=table[:2]),
        dict(block_table=table[0]), dict(block_table=table.tolist()),
        dict(k_cache=kp[:, :, :, :4]), dict(v_cache=vp.double()),
        dict(k_cache=kp[0], v_cache=vp[0]), dict(q=q[:, :3]),
        dict(cache_seqlens=lt[:2]), dict(k_new=kn[:, :1], v_new=vn[:, :1]),
        dict(block_table=table[:, :1].expand(B, 1 << 27)),   # Smax 2^31
    ]
    for change in bad:
        args = dict(q=q, k_cache=kp, v_cache=vp, cache_seqlens=lt,
                    block_table=table)
        args.update(change)
        with pytest.raises(ValueError, match="flash_attention_extend"):
            flash_attention_extend(**args)
        args = {n: t[:, :, 0] if n in ("q", "k_new", "v_new") else t
                for n, t in args.items()}
        with pytest.raises(ValueError, match="flash_attention_decode"):
            flash_attention_decode(**args)
