"""FP8 (e4m3) KV caches off the kernel path, on the CPU: the composed decode
against ``decode_reference`` on the dequantised caches at decode's tolerances,
the quantisation function, and the argument errors. q is fp32: the route
dequantises to q's dtype, which is exact in fp32, while bf16 would round
code * scale by up to 2^-9, more than the lse tolerance at a one-key
sequence."""

import pytest
import torch

from attn_decode_ref import decode_reference

from adapcc_amd.ops.attention import (flash_attention_decode,
                                      flash_attention_extend, kv_cache_append,
                                      kv_quantize_reference)

O_TOL = dict(rtol=2e-2, atol=2e-2)
LSE_TOL = dict(rtol=1e-3, atol=1e-3)
F8 = torch.float8_e4m3fn
B, H, HK, SMAX, D = 4, 4, 2, 64, 16
LENS = [0, 1, 37, 63]


def lens_t(x):
    return torch.tensor(x, dtype=torch.int32)


def make(seed=0):
    torch.manual_seed(seed)
    q = torch.randn(B, H, D)
    kf, vf = torch.randn(2, B, HK, SMAX, D)
    ks, vs = (x.abs().amax(dim=(0, 2, 3)) / 448 for x in (kf, vf))
    return q, kv_quantize_reference(kf, ks), kv_quantize_reference(vf, vs), ks, vs


def deq(c, s):
    return c.float() * s.view(1, -1, 1, 1)


@pytest.mark.parametrize("P", [None, 16])
@pytest.mark.parametrize("new", [False, True])
def test_composed_matches_reference(new, P):
    q, k, v, ks, vs = make()
    kn, vn = torch.randn(2, B, HK, D)
    ke, ve = k.clone(), v.clone()
    kw, n_keys = {}, LENS
    if new:
        kw, n_keys = dict(k_new=kn, v_new=vn), [n + 1 for n in LENS]
        for b, n in enumerate(LENS):
            ke[b, :, n] = kv_quantize_reference(kn, ks)[b]
            ve[b, :, n] = kv_quantize_reference(vn, vs)[b]
    if P is not None:           # pages in reverse order, one spare NaN page
        mp = SMAX // P
        table = (B * mp - 1 - torch.arange(B * mp)).view(B, mp).int()
        pool = lambda c: torch.cat([
            c.view(torch.uint8).view(B, HK, mp, P, D).transpose(1, 2)
            .reshape(B * mp, HK, P, D).flip(0),
            torch.full((1, HK, P, D), 0x7F, dtype=torch.uint8)]).view(F8)
        k, v, kw["block_table"] = pool(k), pool(v), table
    out, lse = flash_attention_decode(q, k, v, lens_t(LENS), return_lse=True,
                                      k_scale=ks, v_scale=vs, **kw)
    ref, ref_lse = decode_reference(q, deq(ke, ks), deq(ve, vs), n_keys)
    torch.testing.assert_close(out.float(), ref, **O_TOL)
    torch.testing.assert_close(lse, ref_lse, **LSE_TOL)
    if P is None:               # the new rows quantised, nothing else touched
        assert torch.equal(k.view(torch.uint8), ke.view(torch.uint8))
        assert torch.equal(v.view(torch.uint8), ve.view(torch.uint8))


def test_quantize_saturates_and_is_never_nan():
    x = torch.tensor([[[500.0, -1e30, 448.0, 464.0, 1e-9, -0.0, 3e38]]])
    got = kv_quantize_reference(x, torch.tensor([1.0]))
    assert got.dtype == F8
    assert got.float().tolist() == [[[448.0, -448.0, 448.0, 448.0, 0.0, 0.0,
                                      448.0]]]
    big = kv_quantize_reference(torch.randn(2, 3, 50) * 1e4,
                                torch.tensor([1.0, 7.0, 1e-3]))
    assert (big.view(torch.uint8) & 0x7F != 0x7F).all()


def test_append_alone_quantises_and_drops_overflow():
    _, k, v, ks, vs = make(1)
    kn, vn = torch.randn(2, B, HK, 5, D, dtype=torch.bfloat16) * 3
    past, ql = [0, 10, 61, 64], [5, 0, 5, 5]
    ke, ve = k.clone(), v.clone()
    for c, new, s in ((ke, kn, ks), (ve, vn, vs)):
        for b in range(B):
            n = min(ql[b], SMAX - past[b])
            c[b, :, past[b]:past[b] + n] = kv_quantize_reference(new, s)[b, :, :n]
    kv_cache_append(k, v, lens_t(past), kn, vn, q_lens=lens_t(ql), k_scale=ks,
                    v_scale=vs)
    assert torch.equal(k.view(torch.uint8), ke.view(torch.uint8))
    assert torch.equal(v.view(torch.uint8), ve.view(torch.uint8))


def test_argument_errors():
    q, k, v, ks, vs = make()
    lens = lens_t(LENS)
    bad = [dict(), dict(k_scale=ks), dict(k_scale=ks, v_scale=vs[:1]),
           dict(k_scale=ks, v_scale=vs.double()),
           dict(k_scale=torch.stack([ks, ks], 1)[:, 0], v_scale=vs),
           dict(k_scale=ks, v_scale=vs.to("meta"))]
    for kw in bad:
        with pytest.raises(ValueError):
            flash_attention_decode(q, k, v, lens, **kw)
    kb, vb = k.to(torch.bfloat16), v.to(torch.bfloat16)
    with pytest.raises(ValueError):     # scales without an fp8 cache
        flash_attention_decode(q, kb, vb, lens, k_scale=ks, v_scale=vs)
    with pytest.raises(ValueError):     # as before this mode existed
        flash_attention_decode(q, kb, vb, lens)
    with pytest.raises(ValueError):     # extend does not take e4m3 caches
        flash_attention_extend(q.unsqueeze(2), k, v, lens)
