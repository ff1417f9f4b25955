"""Extend attention over FP8 (e4m3) KV caches (csrc/attn_extend_fp8.hip)
against ``extend_reference`` on the dequantised fp32 caches
``cache.float() * scale``. e4m3 -> bf16 is exact, so the kernel's roundings
are the bf16 kernel's and so are the tolerances: rtol = atol = 2e-2 on the
output, 1e-3 on the lse. Every call asserts ``fa_extend_supported`` with the
scales first, so where this is not a kernel path it fails there. A call that
appends is held to the caches as read back afterwards (the chunk attends over
its own stored codes), and its written bytes to ``kv_quantize_reference``."""

import pytest
import torch

from attn_extend_ref import extend_reference
from test_gpu_attention_decode_fp8 import (F8, LSE_TOL, O_TOL, U8,
                                           assert_appended, deq, hard_rows,
                                           lens_t, to_pool)

from adapcc_amd.ops.attention import (fa_extend_supported,
                                      flash_attention_extend,
                                      kv_quantize_reference)

pytestmark = pytest.mark.gpu

SMAX = 400
PASTS = [0, 1, 63, 64, 65, 200]


def make(B, H, Hk, Sq, Smax, D, seed=0):
    """q bf16, caches quantised from randn with scale = amax / 448 per head
    (distinct, not powers of two); V grows with the head, so a swapped or
    dropped v_scale shows."""
    torch.manual_seed(seed)
    q = torch.randn(B, H, Sq, D, device="cuda", dtype=torch.bfloat16)
    kf, vf = torch.randn(2, B, Hk, Smax, D, device="cuda")
    vf = vf * torch.arange(1, Hk + 1, device="cuda").view(1, Hk, 1, 1)
    ks, vs = (x.abs().amax(dim=(0, 2, 3)) / 448 for x in (kf, vf))
    return q, kv_quantize_reference(kf, ks), kv_quantize_reference(vf, vs), ks, vs


def run(q, k, v, ks, vs, past, ql=None, **kw):
    lens, qlt = lens_t(past), None if ql is None else lens_t(ql)
    assert fa_extend_supported(q, k, v, lens, qlt, kw.get("block_table"),
                               k_scale=ks, v_scale=vs)
    return flash_attention_extend(q, k, v, lens, q_lens=qlt, return_lse=True,
                                  k_scale=ks, v_scale=vs, **kw)


def check(got, q, k, v, ks, vs, past, ql=None, causal=True):
    """got = (out, lse) against the reference over caches k, v holding
    past[b] keys, the chunk's among them."""
    ref, ref_lse, _, _ = extend_reference(q, deq(k, ks), deq(v, vs), past,
                                          q_lens=ql, causal=causal)
    torch.testing.assert_close(got[0].float().cpu(), ref, **O_TOL)
    torch.testing.assert_close(got[1].cpu(), ref_lse, **LSE_TOL)


def ragged_lens(Sq, B):
    return [max(Sq - b * -(-Sq // (B - 1)), 0) for b in range(B)]  # Sq .. 0


@pytest.mark.parametrize("D", [64, 128])
@pytest.mark.parametrize("ragged", [False, True])
@pytest.mark.parametrize("Sq", [1, 5, 33, 130])
def test_rows_pasts_and_splits(Sq, ragged, D):
    """Past 0 and 1 leave rows that see no key: zeros and lse -inf there."""
    B = len(PASTS)
    q, k, v, ks, vs = make(B, 8, 2, Sq, SMAX, D, seed=Sq + D)
    ql = ragged_lens(Sq, B) if ragged else None
    ref = extend_reference(q, deq(k, ks), deq(v, vs), PASTS, q_lens=ql)
    for ns in (1, 2, 4):
        out, lse = run(q, k, v, ks, vs, PASTS, ql, num_splits=ns)
        torch.testing.assert_close(out.float().cpu(), ref[0], **O_TOL)
        torch.testing.assert_close(lse.cpu(), ref[1], **LSE_TOL)
        dead = lse == float("-inf")
        assert dead[0].all() and not out[dead].any()
        again = run(q, k, v, ks, vs, PASTS, ql, num_splits=ns)
        assert torch.equal(out, again[0]) and torch.equal(lse, again[1])


@pytest.mark.parametrize("D", [64, 128])
@pytest.mark.parametrize("causal", [True, False])
@pytest.mark.parametrize("H,Hk", [(4, 4), (6, 2), (32, 1)])
def test_heads(H, Hk, causal, D):
    past = [45, 70, 257]
    q, k, v, ks, vs = make(3, H, Hk, 45, SMAX, D, seed=H + D)
    for ns in (1, 2):
        check(run(q, k, v, ks, vs, past, causal=causal, num_splits=ns), q, k,
              v, ks, vs, past, causal=causal)


@pytest.mark.parametrize("D", [64, 128])
@pytest.mark.parametrize("num_splits", [1, 4])
def test_padding_is_never_read(num_splits, D):
    Sq, past, ql = 33, [33, 64, 129, 300], [33, 20, 1, 0]
    q, k, v, ks, vs = make(4, 8, 2, Sq, SMAX, D, seed=9)
    for b, n in enumerate(past):
        k.view(U8)[b, :, n:] = 0x7F     # the e4m3 NaN code
        v.view(U8)[b, :, n:] = 0x7F
        q[b, :, ql[b]:] = float("nan")
    out, lse = run(q, k, v, ks, vs, past, ql, num_splits=num_splits)
    assert torch.isfinite(out).all()
    for b, n in enumerate(ql):
        assert not out[b, :, n:].any()
        assert (lse[b, :, n:] == float("-inf")).all()
    check((out, lse), q, k, v, ks, vs, past, ql)    # reads live rows only


def pools(k, v, P, B):
    mp = k.shape[2] // P
    N = B * mp + 5
    table = torch.randperm(N, device="cuda")[:B * mp].view(B, mp).int()
    return to_pool(k, P, table, N), to_pool(v, P, table, N), table


@pytest.mark.parametrize("D", [64, 128])
@pytest.mark.parametrize("P", [16, 64])
def test_paged_matches_gathered_slab(P, D):
    B, Sq, Smax, past = 3, 45, 448, [45, 150, 439]
    q, k, v, ks, vs = make(B, 8, 2, Sq, Smax, D, seed=P + D)
    kp, vp, table = pools(k, v, P, B)
    for b, n in enumerate(past):
        table[b, -(-n // P):] = table.max() + 7   # unused, out of range
    for ns in (1, 2):
        got = run(q, kp, vp, ks, vs, past, block_table=table, num_splits=ns)
        check(got, q, k, v, ks, vs, past)
        slab = run(q, k, v, ks, vs, past, num_splits=ns)
        assert torch.equal(got[0], slab[0]) and torch.equal(got[1], slab[1])


def test_strided_cache_matches_contiguous():
    past = [70, 257]
    q, k, v, ks, vs = make(2, 8, 2, 45, SMAX, 64, seed=5)
    want = run(q, k, v, ks, vs, past)
    kt, vt = (c.transpose(1, 2).contiguous().transpose(1, 2) for c in (k, v))
    assert not kt.is_contiguous()
    assert torch.equal(run(q, kt, vt, ks, vs, past)[0], want[0])


@pytest.mark.parametrize("D", [64, 128])
@pytest.mark.parametrize("P", [None, 16, 64])
@pytest.mark.parametrize("num_splits", [1, 4])
def test_append_quantises_then_attends_over_stored(num_splits, P, D):
    """Sequence 2 reaches Smax (its last rows are dropped), 3 is full. First
    rows like the cache's own under its scales: the output against the
    caches as read back. Then rows with every rounding case under
    power-of-two scales, where the kernel's division and the reference's
    agree exactly: the written bytes (their outputs cancel values of
    hundreds, which the output tolerance is not made for)."""
    B, H, Hk, Sq, Smax = 4, 8, 2, 5, 448
    q, k, v, ks, vs = make(B, H, Hk, Sq, Smax, D, seed=7)
    past, ql = [0, 63, Smax - 2, Smax], [Sq, Sq - 1, Sq, Sq]
    kw, table = {}, None
    if P is not None:
        k, v, table = pools(k, v, P, B)
        kw = dict(block_table=table)
    slab = (lambda c: c) if P is None else (
        lambda c: c.view(U8)[table.long()].transpose(1, 2)
        .reshape(B, Hk, Smax, D).view(F8))
    total = [min(p + n, Smax) for p, n in zip(past, ql)]
    kn, vn = torch.randn(2, B, Hk, Sq, D, device="cuda").bfloat16()
    vn = vn * torch.arange(1, Hk + 1, device="cuda").view(1, Hk, 1, 1)
    ps = (torch.tensor([2.0 ** -3, 2.0], device="cuda"),
          torch.tensor([2.0, 2.0 ** -3], device="cuda"))
    for (s_k, s_v), (kn, vn) in (((ks, vs), (kn, vn)),
                                 (ps, hard_rows((B, Hk, Sq, D), *ps, D + Sq))):
        k0, v0 = k.clone(), v.clone()
        got = run(q, k, v, s_k, s_v, past, ql, k_new=kn, v_new=vn,
                  num_splits=num_splits, **kw)
        if s_k is ks:
            check(got, q, slab(k), slab(v), ks, vs, total, ql)
            continue
        assert_appended(k, k0, kn, s_k, past, ql, table)
        assert_appended(v, v0, vn, s_v, past, ql, table)
