"""Multi-row attention over a KV cache (csrc/attn_extend.hip) against the
fp32 per-sequence reference computed from the bf16 inputs. Outputs at the
project's attention tolerance rtol = atol = 2e-2, lse at 1e-3. Every test
asserts ``fa_extend_supported`` first, so where extend is not a kernel path
it fails there."""

import pytest
import torch

from attn_extend_ref import extend_reference

from adapcc_amd.ops.attention import (fa_extend_supported,
                                      flash_attention_extend)

pytestmark = pytest.mark.gpu

O_TOL = dict(rtol=2e-2, atol=2e-2)
LSE_TOL = dict(rtol=1e-3, atol=1e-3)
SMAX = 400
PASTS = [0, 1, 63, 64, 65, 200]


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


def bits(t):
    return t.cpu().contiguous().view(torch.int16)


def check(q, k, v, past, kn=None, vn=None, q_lens=None, causal=True):
    """One call against the reference: output, lse, exact zeros and -inf
    where a row is padding or sees no key, the caches bit for bit (so every
    row but the appended ones is untouched), the length tensors untouched."""
    pt, qt = lens_t(past), lens_t(q_lens)
    assert fa_extend_supported(q, k, v, pt, qt)
    ref, ref_lse, ke, ve = extend_reference(q, k, v, past, kn, vn, q_lens,
                                            causal)
    out, lse = flash_attention_extend(q, k, v, pt, kn, vn, qt, causal=causal,
                                      return_lse=True)
    assert out.shape == q.shape and out.transpose(1, 2).is_contiguous()
    live = ref_lse > float("-inf")
    # padding rows of q may hold NaN: compare the live rows, pin the others
    torch.testing.assert_close(out.float().cpu()[live], ref[live], **O_TOL)
    torch.testing.assert_close(lse.cpu(), ref_lse, **LSE_TOL)
    assert not out.cpu()[~live].any()
    assert torch.equal(bits(k), bits(ke)) and torch.equal(bits(v), bits(ve))
    assert pt.tolist() == list(past)
    assert q_lens is None or qt.tolist() == list(q_lens)
    return out, lse


@pytest.mark.parametrize("Sq", [1, 5, 32, 33, 130])
@pytest.mark.parametrize("ragged", [False, True])
def test_tile_edges(Sq, ragged):
    """G = 4: 130 positions are 520 group rows, five workgroups with a ragged
    last one. Ragged: n_b runs from Sq down to 0."""
    B = len(PASTS)
    q, k, v, kn, vn = make(B, 8, 2, Sq, 64, seed=Sq)
    q_lens = [Sq * (B - 1 - b) // (B - 1) for b in range(B)] if ragged else None
    k0, v0 = k.clone(), v.clone()
    out, lse = check(q, k, v, PASTS, kn, vn, q_lens)
    if ragged:
        assert not out[-1].any() and (lse[-1] == float("-inf")).all()
    again = flash_attention_extend(q, k0, v0, lens_t(PASTS), kn, vn,
                                   lens_t(q_lens))
    assert torch.equal(out, again)      # deterministic


@pytest.mark.parametrize("D", [64, 128])
@pytest.mark.parametrize("H,Hk", [(4, 4), (8, 2), (6, 2), (12, 1), (32, 1)])
@pytest.mark.parametrize("causal", [True, False])
def test_heads(H, Hk, D, causal):
    """Sq = 45: at G = 3, 135 group rows straddle a workgroup boundary in
    the middle of a position's heads."""
    q, k, v, kn, vn = make(2, H, Hk, 45, D, seed=H + D)
    check(q, k, v, [70, 257], kn, vn, causal=causal)


def test_append_stays_inside_the_cache():
    """Chunks that overrun Smax: the dropped rows go nowhere. The caches are
    views with guard rows before and after every (batch, head) plane."""
    B, H, Hk, Sq, D, Smax, pad = 4, 8, 2, 40, 128, 100, 48
    q, _, _, kn, vn = make(B, H, Hk, Sq, D, seed=7, Smax=8)
    torch.manual_seed(8)
    kbuf, vbuf = torch.randn(2, B, Hk, Smax + 2 * pad, D, device="cuda",
                             dtype=torch.bfloat16)
    k, v = kbuf[:, :, pad:-pad], vbuf[:, :, pad:-pad]
    kb0, vb0 = kbuf.clone(), vbuf.clone()
    check(q, k, v, [0, 59, 61, 95], kn, vn, q_lens=[40, 40, 40, 7])
    for buf, buf0 in ((kbuf, kb0), (vbuf, vb0)):
        assert torch.equal(buf[:, :, :pad], buf0[:, :, :pad])
        assert torch.equal(buf[:, :, -pad:], buf0[:, :, -pad:])


@pytest.mark.parametrize("causal", [True, False])
def test_padding_is_never_read(causal):
    past, q_lens, Sq = [0, 33, 129, 256], [45, 1, 17, 0], 45
    q, k, v, kn, vn = make(len(past), 12, 1, Sq, 64, seed=9)
    for b, (p, n) in enumerate(zip(past, q_lens)):
        k[b, :, p + n:] = v[b, :, p + n:] = float("nan")
        q[b, :, n:] = kn[b, :, n:] = vn[b, :, n:] = float("nan")
    out, _ = check(q, k, v, past, kn, vn, q_lens, causal=causal)
    assert torch.isfinite(out).all()


def test_layouts_match_contiguous_bit_for_bit():
    B, H, Hk, Sq, D = 2, 8, 2, 45, 64
    q, k, v, kn, vn = make(B, H, Hk, Sq, D, seed=5)
    past = lens_t([70, 257])
    kt = k.transpose(1, 2).contiguous().transpose(1, 2)   # [B,Smax,Hk,D]
    vt = v.transpose(1, 2).contiguous().transpose(1, 2)
    packed = torch.cat([t.transpose(1, 2).reshape(B, Sq, -1)
                        for t in (q, kn, vn)], dim=-1)    # [B,Sq,(H+2Hk)D]
    qs, ks, vs = (t.view(B, Sq, -1, D).transpose(1, 2) for t in
                  packed.split([H * D, Hk * D, Hk * D], dim=-1))
    assert not kt.is_contiguous() and not ks.is_contiguous()
    assert fa_extend_supported(qs, kt, vt, past)
    want = flash_attention_extend(q, k, v, past, kn, vn)
    got = flash_attention_extend(qs, kt, vt, past, ks, vs)
    assert torch.equal(got, want)
    assert torch.equal(kt, k) and torch.equal(vt, v)


def test_cross_attention():
    """Non-causal, no new rows, Sq != total; an empty cache gives zeros."""
    q, k, v, _, _ = make(3, 8, 2, 45, 128, seed=3)
    out, _ = check(q, k, v, [100, 333, 0], causal=False)
    assert not out[2].any()


def test_graph_replay_with_refilled_lengths():
    """No host sync: the call (append and attention kernels) is captured
    once and replayed after both length tensors changed in place; two
    replays, each against the reference from the same starting caches."""
    q, k, v, kn, vn = make(3, 8, 2, 33, 64, seed=11)
    k0, v0 = k.clone(), v.clone()
    pt, qt = lens_t([5, 200, 64]), lens_t([33, 1, 20])
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        flash_attention_extend(q, k, v, pt, kn, vn, qt,
                               return_lse=True)                # warm-up
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=side):
        out, lse = flash_attention_extend(q, k, v, pt, kn, vn, qt,
                                          return_lse=True)
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
        assert torch.equal(bits(k), bits(ke))


def test_side_stream():
    """The launcher makes the tensors' device current itself and launches on
    the stream that is current for it: one call under a side stream."""
    q, k, v, kn, vn = make(2, 8, 2, 5, 64, seed=15)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        check(q, k, v, [0, 63], kn, vn)
    torch.cuda.current_stream().wait_stream(side)


@pytest.mark.parametrize("H,Hk,D", [(64, 1, 64), (4, 2, 32)])
def test_fallbacks_answer_instead_of_throwing(H, Hk, D):
    q, k, v, kn, vn = make(2, H, Hk, 9, D, seed=13)
    past = [70, 257]
    assert not fa_extend_supported(q, k, v, lens_t(past))
    ref = extend_reference(q, k, v, past, kn, vn)[0]
    out = flash_attention_extend(q, k, v, lens_t(past), kn, vn)
    torch.testing.assert_close(out.float().cpu(), ref, **O_TOL)
