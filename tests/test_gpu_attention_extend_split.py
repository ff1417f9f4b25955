"""Split-KV launches of the multi-row attention over a KV cache
(csrc/attn_extend.hip: fa_extend_kernel<., true> and the combine kernel)
against the fp32 per-sequence reference. Outputs at the project's attention
tolerance rtol = atol = 2e-2, lse at 1e-3: the merge of the splits is fp32
and gets no looser bound. At Smax = 400 forced counts of 2 to 4 give splits
of 256 or 128 keys."""

import pytest
import torch

from attn_extend_ref import extend_reference

import adapcc_amd._core as core
from adapcc_amd.ops.attention import (fa_extend_supported,
                                      flash_attention_extend)

pytestmark = pytest.mark.gpu

O_TOL = dict(rtol=2e-2, atol=2e-2)
LSE_TOL = dict(rtol=1e-3, atol=1e-3)
SMAX = 400
PASTS = [0, 1, 63, 127, 128, 200]


def make(B, H, Hk, Sq, D, seed=0, Smax=SMAX):
    torch.manual_seed(seed)
    bf = dict(device="cuda", dtype=torch.bfloat16)
    q = torch.randn(B, H, Sq, D, **bf)
    k, v = torch.randn(2, B, Hk, Smax, D, **bf)
    kn, vn = torch.randn(2, B, Hk, Sq, D, **bf)
    return q, k, v, kn, vn


def lens_t(lens):
    return None if lens is None else torch.tensor(lens, dtype=torch.int32,
                                                  device="cuda")


def check(q, k, v, past, kn=None, vn=None, q_lens=None, causal=True,
          num_splits=None):
    """One call against the reference: output, lse, exact zeros and -inf
    where a row is padding or sees no key, the caches bit for bit, the
    length tensors untouched."""
    pt, qt = lens_t(past), lens_t(q_lens)
    assert fa_extend_supported(q, k, v, pt, qt)
    ref, ref_lse, ke, ve = extend_reference(q, k, v, past, kn, vn, q_lens,
                                            causal)
    out, lse = flash_attention_extend(q, k, v, pt, kn, vn, qt, causal=causal,
                                      return_lse=True, num_splits=num_splits)
    assert out.shape == q.shape and out.transpose(1, 2).is_contiguous()
    live = ref_lse > float("-inf")
    torch.testing.assert_close(out.float().cpu()[live], ref[live], **O_TOL)
    torch.testing.assert_close(lse.cpu(), ref_lse, **LSE_TOL)
    assert not out.cpu()[~live].any()
    for got, want in ((k, ke), (v, ve)):    # bits: padding may hold NaN
        assert torch.equal(got.cpu().view(torch.int16),
                           want.view(torch.int16))
    assert pt.tolist() == list(past)
    assert q_lens is None or qt.tolist() == list(q_lens)
    return out, lse


@pytest.mark.parametrize("Sq", [1, 5, 33, 130])
@pytest.mark.parametrize("ragged", [False, True])
@pytest.mark.parametrize("num_splits", [2, 4])
def test_tile_edges(num_splits, Sq, ragged):
    """G = 4. Sequences shorter than a split leave whole splits empty; with
    past 127 and 128 the causal band straddles key 128, so rows of a live
    workgroup have their limit under the split's start; ragged, n_b runs
    from Sq down to 0 and the last tile of the last split is ragged."""
    B = len(PASTS)
    q, k, v, kn, vn = make(B, 8, 2, Sq, 64, seed=Sq)
    q_lens = [Sq * (B - 1 - b) // (B - 1) for b in range(B)] if ragged else None
    k0, v0 = k.clone(), v.clone()
    out, lse = check(q, k, v, PASTS, kn, vn, q_lens, num_splits=num_splits)
    if ragged:
        assert not out[-1].any() and (lse[-1] == float("-inf")).all()
    again = flash_attention_extend(q, k0, v0, lens_t(PASTS), kn, vn,
                                   lens_t(q_lens), num_splits=num_splits)
    assert torch.equal(out, again)      # deterministic


@pytest.mark.parametrize("D", [64, 128])
@pytest.mark.parametrize("H,Hk", [(4, 4), (8, 2), (6, 2), (32, 1)])
@pytest.mark.parametrize("causal", [True, False])
def test_heads(H, Hk, D, causal):
    q, k, v, kn, vn = make(2, H, Hk, 45, D, seed=H + D)
    check(q, k, v, [70, 257], kn, vn, causal=causal, num_splits=3)


def test_one_split_is_the_unsplit_kernel():
    q, k, v, kn, vn = make(2, 8, 2, 45, 64, seed=5)
    past = lens_t([70, 257])
    res = [flash_attention_extend(q, k.clone(), v.clone(), past, kn, vn,
                                  return_lse=True, num_splits=ns)
           for ns in (1, None)]
    assert torch.equal(res[0][0], res[1][0])
    assert torch.equal(res[0][1], res[1][1])


@pytest.mark.parametrize("causal", [True, False])
def test_padding_is_never_read(causal):
    past, q_lens, Sq = [0, 33, 129, 256], [45, 1, 17, 0], 45
    q, k, v, kn, vn = make(len(past), 12, 1, Sq, 64, seed=9)
    for b, (p, n) in enumerate(zip(past, q_lens)):
        k[b, :, p + n:] = v[b, :, p + n:] = float("nan")
        q[b, :, n:] = kn[b, :, n:] = vn[b, :, n:] = float("nan")
    out, _ = check(q, k, v, past, kn, vn, q_lens, causal=causal,
                   num_splits=4)
    assert torch.isfinite(out).all()


def test_graph_replay_with_refilled_lengths():
    """The split plan reads no length: captured once with four splits,
    replayed twice after both length tensors changed in place."""
    q, k, v, kn, vn = make(3, 8, 2, 33, 64, seed=11)
    k0, v0 = k.clone(), v.clone()
    pt, qt = lens_t([5, 200, 64]), lens_t([33, 1, 20])
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        flash_attention_extend(q, k, v, pt, kn, vn, qt, return_lse=True,
                               num_splits=4)                   # warm-up
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=side):
        out, lse = flash_attention_extend(q, k, v, pt, kn, vn, qt,
                                          return_lse=True, num_splits=4)
    for past, q_lens in (([130, 1, 367], [7, 33, 33]),
                         ([0, 257, 33], [33, 0, 12])):
        k.copy_(k0), v.copy_(v0)
        pt.copy_(lens_t(past)), qt.copy_(lens_t(q_lens))
        graph.replay()
        torch.cuda.synchronize()
        ref, ref_lse, ke, _ = extend_reference(q, k0, v0, past, kn, vn,
                                               q_lens)
        torch.testing.assert_close(out.float().cpu(), ref, **O_TOL)
        torch.testing.assert_close(lse.cpu(), ref_lse, **LSE_TOL)
        assert torch.equal(k.cpu().view(torch.int16), ke.view(torch.int16))


@pytest.mark.parametrize("B,Hk,Sq,G,Smax", [
    (1, 2, 8, 4, 4096), (1, 1, 8, 16, 16384), (32, 16, 8, 1, 16384),
    (8, 4, 512, 4, 4096), (1, 1, 1, 1, 2047), (6, 2, 130, 4, 400)])
def test_policy(B, Hk, Sq, G, Smax):
    n = core.fa_extend_splits(B, Hk, Sq, G, Smax, 0, 0)
    assert n >= 1 and (n == 1 or Smax >= 2048)
    # the split length: the capacity over n, rounded up to 128 keys
    per = -(-Smax // n)
    L = -(-per // 128) * 128
    assert (n - 1) * L < Smax <= n * L


def test_policy_splits_a_short_chunk_over_a_long_cache():
    B, H, Hk, Sq, D, Smax = 1, 8, 2, 8, 64, 4096
    assert core.fa_extend_splits(B, Hk, Sq, H // Hk, Smax, 0, 0) > 1
    q, k, v, kn, vn = make(B, H, Hk, Sq, D, seed=17, Smax=Smax)
    check(q, k, v, [4000], kn, vn)


def test_arguments():
    q, k, v, kn, vn = make(2, 8, 2, 9, 64, seed=13)
    with pytest.raises(ValueError):
        flash_attention_extend(q, k, v, lens_t([70, 257]), num_splits=0)
    q, k, v, kn, vn = make(2, 4, 2, 9, 32, seed=13)     # D = 32: composed
    assert not fa_extend_supported(q, k, v, lens_t([70, 257]))
    ref = extend_reference(q, k, v, [70, 257], kn, vn)[0]
    out = flash_attention_extend(q, k, v, lens_t([70, 257]), kn, vn,
                                 num_splits=2)
    torch.testing.assert_close(out.float().cpu(), ref, **O_TOL)
