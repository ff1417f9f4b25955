"""Decode attention over FP8 (e4m3) KV caches (csrc/attn_decode_fp8.hip)
against ``decode_reference`` on the dequantised fp32 caches
``cache.float() * scale``. e4m3 -> bf16 is exact, so the kernel's roundings
are the bf16 kernel's and so are the tolerances: rtol = atol = 2e-2 on the
output, 1e-3 on the lse. Every test asserts ``fa_decode_supported`` with the
scales first, so where this is not a kernel path it fails there."""

import pytest
import torch

from attn_decode_ref import decode_reference

from adapcc_amd.ops.attention import (fa_decode_supported,
                                      flash_attention_decode, kv_cache_append,
                                      kv_quantize_reference)

pytestmark = pytest.mark.gpu

O_TOL = dict(rtol=2e-2, atol=2e-2)
LSE_TOL = dict(rtol=1e-3, atol=1e-3)
F8, U8 = torch.float8_e4m3fn, torch.uint8
SMAX = 300
LENS = [1, 31, 32, 33, 127, 128, 129, SMAX, 0]


def make(B, H, Hk, Smax, D, seed=0):
    """q bf16, caches quantised from randn with scale = amax / 448 per head
    (distinct, not powers of two)."""
    torch.manual_seed(seed)
    q = torch.randn(B, H, D, device="cuda", dtype=torch.bfloat16)
    kf, vf = torch.randn(2, B, Hk, Smax, D, device="cuda")
    vf = vf * torch.arange(1, Hk + 1, device="cuda").view(1, Hk, 1, 1)
    ks, vs = (x.abs().amax(dim=(0, 2, 3)) / 448 for x in (kf, vf))
    return q, kv_quantize_reference(kf, ks), kv_quantize_reference(vf, vs), ks, vs


def lens_t(lens):
    return torch.tensor(lens, dtype=torch.int32, device="cuda")


def deq(c, s):
    return c.float() * s.view(1, -1, 1, 1)


def check(q, k, v, ks, vs, lens, ref_kv=None, ref_lens=None, **kw):
    assert fa_decode_supported(q, k, v, lens, kw.get("block_table"),
                               k_scale=ks, v_scale=vs)
    out, lse = flash_attention_decode(q, k, v, lens, return_lse=True,
                                      k_scale=ks, v_scale=vs, **kw)
    rk, rv = (k, v) if ref_kv is None else ref_kv
    ref, ref_lse = decode_reference(
        q, deq(rk, ks), deq(rv, vs),
        lens.tolist() if ref_lens is None else ref_lens)
    torch.testing.assert_close(out.float().cpu(), ref, **O_TOL)
    torch.testing.assert_close(lse.cpu(), ref_lse, **LSE_TOL)
    return out, lse


def to_pool(c, P, table, n_pages):
    """The pool [n_pages,Hk,P,D] holding slab c under table; other pages hold
    the e4m3 NaN code."""
    B, Hk, Smax, D = c.shape
    pool = torch.full((n_pages, Hk, P, D), 0x7F, dtype=U8, device=c.device)
    pages = c.view(U8).view(B, Hk, Smax // P, P, D).transpose(1, 2)
    pool[table.long()] = pages
    return pool.view(F8)


@pytest.mark.parametrize("num_splits", [1, 3, None])
def test_split_and_ragged_edges(num_splits):
    q, k, v, ks, vs = make(len(LENS), 8, 2, SMAX, 64)
    out, lse = check(q, k, v, ks, vs, lens_t(LENS), num_splits=num_splits)
    assert not out[-1].any() and (lse[-1] == float("-inf")).all()
    again = flash_attention_decode(q, k, v, lens_t(LENS), k_scale=ks,
                                   v_scale=vs, num_splits=num_splits)
    assert torch.equal(out, again)      # deterministic


@pytest.mark.parametrize("D", [64, 128])
@pytest.mark.parametrize("H,Hk", [(4, 4), (8, 2), (32, 1)])
@pytest.mark.parametrize("num_splits", [1, 3])
def test_heads(H, Hk, D, num_splits):
    q, k, v, ks, vs = make(2, H, Hk, SMAX, D, seed=H + D)
    check(q, k, v, ks, vs, lens_t([70, 257]), num_splits=num_splits)


@pytest.mark.parametrize("D", [64, 128])
@pytest.mark.parametrize("num_splits", [1, 3])
def test_padding_is_never_read(num_splits, D):
    lens = [1, 33, 129, 256]
    q, k, v, ks, vs = make(len(lens), 8, 2, SMAX, D, seed=9)
    for b, n in enumerate(lens):
        k.view(U8)[b, :, n:] = 0x7F     # the e4m3 NaN code
        v.view(U8)[b, :, n:] = 0x7F
    out, _ = check(q, k, v, ks, vs, lens_t(lens), num_splits=num_splits)
    assert torch.isfinite(out).all()


@pytest.mark.parametrize("D", [64, 128])
@pytest.mark.parametrize("P", [16, 64])
def test_paged_matches_gathered_slab(P, D):
    B, H, Hk, Smax, lens = 3, 8, 2, 320, [1, 150, 311]
    q, k, v, ks, vs = make(B, H, Hk, Smax, D, seed=P + D)
    mp, N = Smax // P, B * (Smax // P) + 5
    table = torch.randperm(N, device="cuda")[:B * mp].view(B, mp).int()
    kp, vp = to_pool(k, P, table, N), to_pool(v, P, table, N)
    for b, n in enumerate(lens):
        table[b, -(-n // P):] = N + 7   # unused entries, out of range
    for ns in (1, 3):
        out, _ = check(q, kp, vp, ks, vs, lens_t(lens), ref_kv=(k, v),
                       block_table=table, num_splits=ns)
        slab = flash_attention_decode(q, k, v, lens_t(lens), k_scale=ks,
                                      v_scale=vs, num_splits=ns)
        assert torch.equal(out, slab)


def test_strided_cache_matches_contiguous():
    q, k, v, ks, vs = make(2, 8, 2, SMAX, 64, seed=5)
    lens = lens_t([70, 257])
    want = flash_attention_decode(q, k, v, lens, k_scale=ks, v_scale=vs)
    kt, vt = (c.transpose(1, 2).contiguous().transpose(1, 2) for c in (k, v))
    assert not kt.is_contiguous()
    assert fa_decode_supported(q, kt, vt, lens, k_scale=ks, v_scale=vs)
    got = flash_attention_decode(q, kt, vt, lens, k_scale=ks, v_scale=vs)
    assert torch.equal(got, want)


def hard_rows(shape, ks, vs, seed):
    """bf16 rows whose quotients by the (power-of-two) scales hit values past
    +-448, e4m3 subnormals (multiples of 2^-10 under 2^-6), exact ties at
    both granularities, and ordinary values."""
    g = torch.Generator(device="cuda").manual_seed(seed)
    codes = torch.tensor([500.0, -3000.0, 448.0, 464.0, -480.0, 2.0 ** -10,
                          3 * 2.0 ** -10, -5 * 2.0 ** -10, 2.0 ** -11,
                          9 * 2.0 ** -9, 1.0625, 1.1875, 17.0, -19.0, 0.0],
                         device="cuda")
    pick = torch.randint(0, 2 * len(codes), shape, device="cuda", generator=g)
    x = torch.where(pick < len(codes), codes[pick % len(codes)],
                    torch.randn(shape, device="cuda", generator=g) * 40)
    return ((x * ks.view(1, -1, 1, 1)).bfloat16(),
            (x.flip(-1) * vs.view(1, -1, 1, 1)).bfloat16())


def paged(k, v, P, B, Smax):
    """(k, v, {}, None) as they are for P None, else their pools under a
    shuffled table, the keyword and the table."""
    if P is None:
        return k, v, {}, None
    mp = Smax // P
    N = B * mp + 2
    table = torch.randperm(N, device="cuda")[:B * mp].view(B, mp).int()
    return (to_pool(k, P, table, N), to_pool(v, P, table, N),
            dict(block_table=table), table)


def assert_appended(c, c0, new, s, past, n, table):
    """Cache c is c0 with rows i < n[b] of q8(new, s) at logical rows
    past[b] + i < Smax: those rows equal as floats (+-0 are one value),
    every other byte and nothing else changed."""
    P = c.shape[2]
    Smax = P if table is None else P * table.shape[1]
    want = c0.clone()
    wrote = torch.zeros(c.shape[:3], dtype=torch.bool, device=c.device)
    code = kv_quantize_reference(new, s).view(U8)
    for b in range(len(past)):
        for i in range(min(n[b], Smax - past[b])):
            r = past[b] + i
            at = (b, slice(None), r) if table is None else (
                int(table[b, r // P]), slice(None), r % P)
            want.view(U8)[at] = code[b, :, i]
            wrote[at] = True
    assert torch.equal(c.float()[wrote], want.float()[wrote])
    assert torch.equal(c.view(U8)[~wrote], c0.view(U8)[~wrote])


@pytest.mark.parametrize("D", [64, 128])
@pytest.mark.parametrize("P", [None, 16, 64])
@pytest.mark.parametrize("Sq", [1, 5])
def test_kv_cache_append_quantises_exactly(Sq, P, D):
    """Power-of-two scales: the kernel's division and the reference's agree
    exactly. Sequence 2 reaches Smax (at Sq 5 its last rows are dropped),
    sequence 3 is full."""
    B, Hk, Smax = 4, 2, 320
    _, k, v, _, _ = make(B, 2, Hk, Smax, D, seed=Sq)
    ks = torch.tensor([2.0 ** -3, 2.0], device="cuda")
    vs = torch.tensor([2.0, 2.0 ** -3], device="cuda")
    kn, vn = hard_rows((B, Hk, Sq, D), ks, vs, seed=D + Sq)
    past, ql = [0, 127, Smax - 2, Smax], [Sq, Sq - 1, Sq, Sq]
    k, v, kw, table = paged(k, v, P, B, Smax)
    k0, v0, lt = k.clone(), v.clone(), lens_t(past)
    kv_cache_append(k, v, lt, kn, vn, q_lens=lens_t(ql), k_scale=ks,
                    v_scale=vs, **kw)
    assert_appended(k, k0, kn, ks, past, ql, table)
    assert_appended(v, v0, vn, vs, past, ql, table)
    assert lt.tolist() == past


@pytest.mark.parametrize("P", [None, 16])
@pytest.mark.parametrize("num_splits", [1, 3])
def test_decode_appends_quantised_row(num_splits, P):
    B, H, Hk, D, Smax = 4, 8, 2, 64, 320
    q, k, v, _, _ = make(B, H, Hk, Smax, D, seed=7)
    ks = torch.tensor([2.0 ** -3, 2.0], device="cuda")
    vs = torch.tensor([2.0, 2.0 ** -3], device="cuda")
    kn, vn = (t[:, :, 0] for t in hard_rows((B, Hk, 1, D), ks, vs, seed=3))
    lens = [0, 127, 128, Smax]                    # the last one is full
    k, v, kw, table = paged(k, v, P, B, Smax)
    k0, v0, lt = k.clone(), v.clone(), lens_t(lens)
    assert fa_decode_supported(q, k, v, lt, table, k_scale=ks, v_scale=vs)
    out, lse = flash_attention_decode(q, k, v, lt, k_new=kn, v_new=vn,
                                      return_lse=True, num_splits=num_splits,
                                      k_scale=ks, v_scale=vs, **kw)
    assert_appended(k, k0, kn.unsqueeze(2), ks, lens, [1] * B, table)
    assert_appended(v, v0, vn.unsqueeze(2), vs, lens, [1] * B, table)
    assert lt.tolist() == lens
    # attention over len + 1 keys of the cache as read back
    slab = (lambda c: c) if P is None else (
        lambda c: c.view(U8)[table.long()].transpose(1, 2)
        .reshape(B, Hk, Smax, D).view(F8))
    ref, ref_lse = decode_reference(q, deq(slab(k), ks), deq(slab(v), vs),
                                    [1, 128, 129, Smax])
    torch.testing.assert_close(out.float().cpu(), ref, **O_TOL)
    torch.testing.assert_close(lse.cpu(), ref_lse, **LSE_TOL)
