"""Split-KV decode attention (csrc/attn_decode.hip) against the fp32
reference softmax(q·K^T·scale over keys < len)·V computed from the bf16
inputs. Outputs at the project's attention tolerance rtol = atol = 2e-2, lse
at 1e-3. Every test asserts ``fa_decode_supported`` first, so where decode is
not a kernel path it fails there."""

import pytest
import torch

from attn_decode_ref import decode_reference

from adapcc_amd.ops.attention import (fa_decode_supported,
                                      flash_attention_decode)

pytestmark = pytest.mark.gpu

O_TOL = dict(rtol=2e-2, atol=2e-2)
LSE_TOL = dict(rtol=1e-3, atol=1e-3)
SMAX = 300
LENS = [1, 31, 32, 33, 127, 128, 129, SMAX, 0]


def make(B, H, Hk, Smax, D, seed=0):
    torch.manual_seed(seed)
    q = torch.randn(B, H, D, device="cuda", dtype=torch.bfloat16)
    k = torch.randn(B, Hk, Smax, D, device="cuda", dtype=torch.bfloat16)
    v = torch.randn(B, Hk, Smax, D, device="cuda", dtype=torch.bfloat16)
    return q, k, v


def lens_t(lens):
    return torch.tensor(lens, dtype=torch.int32, device="cuda")


def check(q, k, v, lens, ref_lens=None, **kw):
    assert fa_decode_supported(q, k, v, lens)
    out, lse = flash_attention_decode(q, k, v, lens, return_lse=True, **kw)
    ref, ref_lse = decode_reference(
        q, k, v, lens.tolist() if ref_lens is None else ref_lens)
    torch.testing.assert_close(out.float().cpu(), ref, **O_TOL)
    torch.testing.assert_close(lse.cpu(), ref_lse, **LSE_TOL)
    return out, lse


@pytest.mark.parametrize("num_splits", [1, 2, 3, None])
def test_split_and_ragged_edges(num_splits):
    """At 3 splits of 128 keys the short sequences have empty splits and 129
    straddles an edge; length 0 gives a zero row and lse -inf."""
    q, k, v = make(len(LENS), 8, 2, SMAX, 64)
    out, lse = check(q, k, v, lens_t(LENS), num_splits=num_splits)
    assert not out[-1].any() and (lse[-1] == float("-inf")).all()
    again = flash_attention_decode(q, k, v, lens_t(LENS),
                                   num_splits=num_splits)
    assert torch.equal(out, again)      # deterministic


@pytest.mark.parametrize("D", [64, 128])
@pytest.mark.parametrize("H,Hk", [(4, 4), (8, 2), (12, 1), (32, 1)])
@pytest.mark.parametrize("num_splits", [1, 3])
def test_heads(H, Hk, D, num_splits):
    q, k, v = make(2, H, Hk, SMAX, D, seed=H + D)
    check(q, k, v, lens_t([70, 257]), num_splits=num_splits)


@pytest.mark.parametrize("num_splits", [1, 3])
def test_layouts_match_contiguous_bit_for_bit(num_splits):
    B, H, Hk, D = 2, 8, 2, 64
    q, k, v = make(B, H, Hk, SMAX, D, seed=5)
    lens = lens_t([70, 257])
    want = flash_attention_decode(q, k, v, lens, num_splits=num_splits)
    kt = k.transpose(1, 2).contiguous().transpose(1, 2)   # [B,Smax,Hk,D]
    vt = v.transpose(1, 2).contiguous().transpose(1, 2)
    packed = torch.zeros(B, (H + 2 * Hk) * D, device="cuda",
                         dtype=torch.bfloat16)
    packed[:, :H * D] = q.reshape(B, H * D)
    qs = packed[:, :H * D].view(B, H, D)
    assert not kt.is_contiguous() and qs.stride(0) != H * D
    assert fa_decode_supported(qs, kt, vt, lens)
    got = flash_attention_decode(qs, kt, vt, lens, num_splits=num_splits)
    assert torch.equal(got, want)


@pytest.mark.parametrize("packed", [False, True])
@pytest.mark.parametrize("D", [64, 128])
@pytest.mark.parametrize("num_splits", [1, 3])
def test_append(num_splits, D, packed):
    """The shared append kernel at Sq = 1. ``packed``: the new rows are
    strided views cut from one [B, (H + 2 Hk) D] projection, as
    ``GPT2.generate`` passes them."""
    B, H, Hk = 4, 8, 2
    q, k, v = make(B, H, Hk, SMAX, D, seed=7)
    kn, vn = torch.randn(2, B, Hk, D, device="cuda", dtype=torch.bfloat16)
    if packed:
        qkv = torch.cat([t.reshape(B, -1) for t in (q, kn, vn)], dim=1)
        q, kn, vn = (t.view(B, -1, D) for t in
                     qkv.split([H * D, Hk * D, Hk * D], dim=1))
        assert kn.stride(0) == (H + 2 * Hk) * D and not vn.is_contiguous()
    lens = [0, 127, 128, SMAX]                    # the last one is full
    lt = lens_t(lens)
    k0, v0 = k.clone(), v.clone()
    ke, ve = k.clone(), v.clone()
    for b, n in enumerate(lens[:-1]):
        ke[b, :, n], ve[b, :, n] = kn[b], vn[b]
    check(q, k, v, lt, ref_lens=[1, 128, 129, SMAX], num_splits=num_splits,
          k_new=kn, v_new=vn)
    # the new rows exactly, every other element untouched, lengths too
    assert torch.equal(k, ke) and torch.equal(v, ve)
    assert torch.equal(k[-1], k0[-1]) and torch.equal(v[-1], v0[-1])
    assert lt.tolist() == lens


@pytest.mark.parametrize("num_splits", [1, 3])
def test_padding_is_never_read(num_splits):
    lens = [1, 33, 129, 256]
    q, k, v = make(len(lens), 12, 1, SMAX, 64, seed=9)
    for b, n in enumerate(lens):
        k[b, :, n:] = float("nan")
        v[b, :, n:] = float("nan")
    out, _ = check(q, k, v, lens_t(lens), num_splits=num_splits)
    assert torch.isfinite(out).all()


def test_graph_replay_with_refilled_lengths():
    """No host sync: the call (decode and combine kernels) is captured once
    and replayed after the lengths changed in place; two replays, each
    against the reference."""
    q, k, v = make(3, 8, 2, SMAX, 64, seed=11)
    lt = lens_t([5, 200, 64])
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        flash_attention_decode(q, k, v, lt, return_lse=True,
                               num_splits=3)                   # warm-up
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=side):
        out, lse = flash_attention_decode(q, k, v, lt, return_lse=True,
                                          num_splits=3)
    for lens in ([130, 1, SMAX], [0, 257, 33]):
        lt.copy_(lens_t(lens))
        graph.replay()
        torch.cuda.synchronize()
        ref, ref_lse = decode_reference(q, k, v, lens)
        torch.testing.assert_close(out.float().cpu(), ref, **O_TOL)
        torch.testing.assert_close(lse.cpu(), ref_lse, **LSE_TOL)


@pytest.mark.parametrize("H,Hk,D", [(64, 1, 64), (4, 2, 32)])
def test_fallbacks_answer_instead_of_throwing(H, Hk, D):
    q, k, v = make(2, H, Hk, SMAX, D, seed=13)
    lens = lens_t([70, 257])
    assert not fa_decode_supported(q, k, v, lens)
    out = flash_attention_decode(q, k, v, lens)
    ref, _ = decode_reference(q, k, v, lens.tolist())
    torch.testing.assert_close(out.float().cpu(), ref, **O_TOL)
