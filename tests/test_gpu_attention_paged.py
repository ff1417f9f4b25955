"""Paged KV cache (``block_table``) in the kernels of csrc/attn_extend.hip and
csrc/attn_decode.hip: against the fp32 per-sequence reference on the
contiguous cache (rtol = atol = 2e-2, lse 1e-3: the arithmetic is the unpaged
kernels'), and bit for bit against the unpaged call on the gathered slab of
the same Smax and split count. Pages no sequence needs hold NaN, and table
entries past a sequence's length name one of them."""

import functools

import pytest
import torch

from attn_extend_ref import extend_reference
from attn_paged_ref import bits, from_pages, repage, to_pages

from adapcc_amd.ops.attention import (fa_decode_supported,
                                      fa_extend_supported,
                                      flash_attention_decode,
                                      flash_attention_extend)

pytestmark = pytest.mark.gpu

O_TOL = dict(rtol=2e-2, atol=2e-2)
LSE_TOL = dict(rtol=1e-3, atol=1e-3)
PASTS = [0, 1, 63, 127, 128, 200]


@functools.lru_cache(maxsize=None)
def case(B, H, Hk, Sq, D, Smax, seed, past, q_lens=None, causal=True,
         new=True, dtype=torch.bfloat16):
    """Inputs on the CPU and the reference for them, made once per shape."""
    torch.manual_seed(seed)
    q = torch.randn(B, H, Sq, D).to(dtype)
    k, v = torch.randn(2, B, Hk, Smax, D).to(dtype)
    kn, vn = torch.randn(2, B, Hk, Sq, D).to(dtype)
    if q_lens is not None:      # padding rows may hold anything
        for b, n in enumerate(q_lens):
            q[b, :, n:] = kn[b, :, n:] = vn[b, :, n:] = float("nan")
    new_kw = dict(k_new=kn, v_new=vn) if new else {}
    ref = extend_reference(q, k, v, past, q_lens=q_lens, causal=causal,
                           **new_kw)
    n = q_lens or [Sq] * B
    totals = [min(p + x, Smax) if new else p for p, x in zip(past, n)]
    return (q, k, v, kn, vn), ref, totals


def rand(B, Sq, Smax, seed, H=8, Hk=2, D=64):
    torch.manual_seed(seed)
    bf = dict(device="cuda", dtype=torch.bfloat16)
    return (torch.randn(B, H, Sq, D, **bf), *torch.randn(2, B, Hk, Smax, D, **bf),
            *torch.randn(2, B, Hk, Sq, D, **bf))


def lens_t(lens):
    return None if lens is None else torch.tensor(lens, dtype=torch.int32,
                                                  device="cuda")


def check(P, B, H, Hk, Sq, D, seed, past, q_lens=None, causal=True, new=True,
          num_splits=None, decode=False, kernels=True,
          dtype=torch.bfloat16):
    """One paged call against the reference, the unpaged call on the
    gathered slab (bits), the re-paged reference cache (bits), itself."""
    Smax = P * -(-400 // P)
    data, (ref, ref_lse, ke, ve), totals = case(
        B, H, Hk, Sq, D, Smax, seed, tuple(past),
        None if q_lens is None else tuple(q_lens), causal, new, dtype)
    q, k, v, kn, vn = (t.cuda() for t in data)
    kp, vp, table = to_pages(k, v, P, seed, totals)
    pt, qt, table0 = lens_t(past), lens_t(q_lens), table.clone()

    def call(kc, vc, **kw):
        if new:
            kw.update(k_new=kn, v_new=vn)
        if decode:
            kw = {n: t[:, :, 0] if n.endswith("new") else t
                  for n, t in kw.items()}
            out, lse = flash_attention_decode(
                q[:, :, 0], kc, vc, pt, return_lse=True,
                num_splits=num_splits, **kw)
            return out.unsqueeze(2), lse.unsqueeze(2)
        return flash_attention_extend(q, kc, vc, pt, q_lens=qt, causal=causal,
                                      return_lse=True, num_splits=num_splits,
                                      **kw)

    supported = fa_decode_supported(q[:, :, 0], kp, vp, pt, block_table=table) \
        if decode else fa_extend_supported(q, kp, vp, pt, qt,
                                           block_table=table)
    assert supported == kernels
    slabs = from_pages(kp, table), from_pages(vp, table)
    kp2, vp2 = kp.clone(), vp.clone()
    out, lse = call(kp, vp, block_table=table)
    live = ref_lse > float("-inf")
    torch.testing.assert_close(out.float().cpu()[live], ref[live], **O_TOL)
    torch.testing.assert_close(lse.cpu(), ref_lse, **LSE_TOL)
    assert not out.cpu()[~live].any() and torch.isfinite(out).all()
    assert torch.equal(bits(kp), bits(repage(ke, table.cpu(), P, totals)))
    assert torch.equal(bits(vp), bits(repage(ve, table.cpu(), P, totals)))
    assert pt.tolist() == list(past) and torch.equal(table, table0)
    if kernels:
        flat, flat_lse = call(*slabs)
        assert torch.equal(out, flat) and torch.equal(lse, flat_lse)
        again, again_lse = call(kp2, vp2, block_table=table)
        assert torch.equal(out, again) and torch.equal(lse, again_lse)
    return out


@pytest.mark.parametrize("Sq", [1, 5, 33, 130])
@pytest.mark.parametrize("P", [16, 64, 256])
@pytest.mark.parametrize("ragged", [False, True])
@pytest.mark.parametrize("num_splits", [1, 3])
def test_extend_tile_and_page_edges(num_splits, ragged, P, Sq):
    """G = 4, D = 64. P = 16: four pages to a 64-key tile; 256: four tiles to
    a page; ragged, n_b runs from Sq down to 0."""
    B = len(PASTS)
    q_lens = [Sq * (B - 1 - b) // (B - 1) for b in range(B)] if ragged else None
    check(P, B, 8, 2, Sq, 64, Sq, PASTS, q_lens, num_splits=num_splits)


@pytest.mark.parametrize("D", [64, 128])
@pytest.mark.parametrize("H,Hk", [(4, 4), (6, 2), (32, 1)])
@pytest.mark.parametrize("causal", [True, False])
def test_extend_heads(H, Hk, D, causal):
    check(16, 2, H, Hk, 45, D, H + D, [70, 257], causal=causal, num_splits=3)


@pytest.mark.parametrize("H,Hk,D", [(8, 2, 64), (16, 16, 128)])
@pytest.mark.parametrize("P", [16, 32, 128])
@pytest.mark.parametrize("num_splits", [None, 2])
@pytest.mark.parametrize("new", [True, False])
def test_decode(new, num_splits, P, H, Hk, D):
    """A 32-key sub-tile lies in two pages at P = 16, in one from 32 on."""
    check(P, 4, H, Hk, 1, D, P + H, [0, 1, 129, 399], new=new,
          num_splits=num_splits, decode=True)


@pytest.mark.parametrize("causal", [True, False])
def test_unallocated_pages_are_never_read(causal):
    """NaN in every unused page and in q, k_new, v_new past q_lens: check()
    asserts a finite output."""
    check(16, 4, 12, 1, 45, 64, 9, [0, 33, 129, 256], [45, 1, 17, 0],
          causal=causal, num_splits=3)


def test_shared_prefix():
    """Two tables name the same two pages; the new rows land in private
    pages."""
    P, past = 16, [40, 50]
    q, k, v, kn, vn = rand(2, 5, 400, 21)
    k[1, :, :2 * P], v[1, :, :2 * P] = k[0, :, :2 * P], v[0, :, :2 * P]
    kp, vp, table = to_pages(k, v, P, 21)
    table[1, :2] = table[0, :2]
    shared = table[0, :2].long()
    k0, v0 = kp[shared].clone(), vp[shared].clone()
    ref, ref_lse, ke, ve = extend_reference(q, k, v, past, kn, vn)
    out, lse = flash_attention_extend(q, kp, vp, lens_t(past), kn, vn,
                                      return_lse=True, block_table=table)
    torch.testing.assert_close(out.float().cpu(), ref, **O_TOL)
    torch.testing.assert_close(lse.cpu(), ref_lse, **LSE_TOL)
    assert torch.equal(kp[shared], k0) and torch.equal(vp[shared], v0)
    assert torch.equal(bits(from_pages(kp, table)), bits(ke))
    assert torch.equal(bits(from_pages(vp, table)), bits(ve))


def test_graph_replay_with_refilled_lengths_and_table():
    """Replayed twice after lengths, table and pools changed in place."""
    P = 64
    q, k, v, kn, vn = rand(3, 33, 448, 11)
    kp, vp, table = to_pages(k, v, P, 0)
    pt, qt = lens_t([5, 200, 64]), lens_t([33, 1, 20])
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        flash_attention_extend(q, kp, vp, pt, kn, vn, qt, return_lse=True,
                               num_splits=2, block_table=table)   # warm-up
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=side):
        out, lse = flash_attention_extend(q, kp, vp, pt, kn, vn, qt,
                                          return_lse=True, num_splits=2,
                                          block_table=table)
    for seed, past, q_lens in ((1, [130, 1, 367], [7, 33, 33]),
                               (2, [0, 257, 33], [33, 0, 12])):
        kp1, vp1, table1 = to_pages(k, v, P, seed)
        kp.copy_(kp1), vp.copy_(vp1), table.copy_(table1)
        pt.copy_(lens_t(past)), qt.copy_(lens_t(q_lens))
        graph.replay()
        torch.cuda.synchronize()
        ref, ref_lse, ke, _ = extend_reference(q, k, v, past, kn, vn, q_lens)
        torch.testing.assert_close(out.float().cpu(), ref, **O_TOL)
        torch.testing.assert_close(lse.cpu(), ref_lse, **LSE_TOL)
        assert torch.equal(bits(from_pages(kp, table)), bits(ke))


@pytest.mark.parametrize("P,dtype", [(24, torch.bfloat16),
                                     (8, torch.bfloat16),
                                     (16, torch.float16)])
@pytest.mark.parametrize("decode", [False, True])
def test_unsupported_pages_answer_through_the_composed_route(P, dtype, decode):
    check(P, 4, 8, 2, 1 if decode else 9, 64, 13, [0, 1, 129, 380],
          decode=decode, kernels=False, dtype=dtype)
