"""flash_attention_decode off the kernel path (CPU): the composed route
against an fp32 reference, and the argument errors."""

import pytest
import torch

from attn_decode_ref import decode_reference

from adapcc_amd.ops.attention import (fa_decode_supported,
                                      flash_attention_decode)

O_TOL = dict(rtol=2e-2, atol=2e-2)
LENS = [1, 31, 32, 33, 127, 128, 129, 300]


def make(B, H, Hk, Smax, D, dtype=torch.bfloat16, seed=0):
    g = torch.Generator().manual_seed(seed)
    q = torch.randn(B, H, D, generator=g).to(dtype)
    k = torch.randn(B, Hk, Smax, D, generator=g).to(dtype)
    v = torch.randn(B, Hk, Smax, D, generator=g).to(dtype)
    return q, k, v


@pytest.mark.parametrize("H,Hk", [(4, 4), (12, 1)])
def test_composed_matches_reference(H, Hk):
    q, k, v = make(len(LENS) + 1, H, Hk, 300, 64)
    lens = torch.tensor(LENS + [0], dtype=torch.int32)
    assert not fa_decode_supported(q, k, v, lens)
    out, lse = flash_attention_decode(q, k, v, lens, return_lse=True)
    ref, ref_lse = decode_reference(q, k, v, lens)
    torch.testing.assert_close(out.float(), ref, **O_TOL)
    # bf16 q·K^T inside SDPA does not enter lse: it is formed in fp32
    torch.testing.assert_close(lse, ref_lse, rtol=1e-3, atol=1e-3)
    assert lens.tolist() == LENS + [0]


def test_composed_append():
    q, k, v = make(3, 8, 2, 40, 64, seed=1)
    lens = torch.tensor([0, 17, 40], dtype=torch.int32)
    kn, vn = torch.randn(2, 3, 2, 64).to(torch.bfloat16)
    k0, v0 = k.clone(), v.clone()
    out = flash_attention_decode(q, k, v, lens, k_new=kn, v_new=vn)
    ke, ve = k0.clone(), v0.clone()
    for b, n in enumerate([0, 17]):      # the full sequence writes nothing
        ke[b, :, n], ve[b, :, n] = kn[b], vn[b]
    assert torch.equal(k, ke) and torch.equal(v, ve)
    ref, _ = decode_reference(q, ke, ve, [1, 18, 40])
    torch.testing.assert_close(out.float(), ref, **O_TOL)


@pytest.mark.parametrize("bad", [
    lambda q, k, v, n: (q[0], k, v, n),                    # q not 3-D
    lambda q, k, v, n: (q, k, v[:, :, :5], n),             # cache shapes
    lambda q, k, v, n: (q[:, :3], k, v, n),                # H % Hk
    lambda q, k, v, n: (q.float(), k, v, n),               # dtypes
    lambda q, k, v, n: (q, k, v, n.long()),                # lengths dtype
    lambda q, k, v, n: (q, k, v, n[:1]),                   # lengths shape
])
def test_value_errors(bad):
    q, k, v = make(2, 4, 2, 16, 64)
    n = torch.tensor([3, 16], dtype=torch.int32)
    with pytest.raises(ValueError, match="flash_attention_decode"):
        flash_attention_decode(*bad(q, k, v, n))


def test_new_rows_and_splits_errors():
    q, k, v = make(2, 4, 2, 16, 64)
    n = torch.tensor([3, 16], dtype=torch.int32)
    kn = torch.zeros(2, 2, 64, dtype=torch.bfloat16)
    with pytest.raises(ValueError, match="k_new and v_new together"):
        flash_attention_decode(q, k, v, n, k_new=kn)
    with pytest.raises(ValueError, match="v_new must be"):
        flash_attention_decode(q, k, v, n, k_new=kn, v_new=kn[:, :1])
    with pytest.raises(ValueError, match="num_splits"):
        flash_attention_decode(q, k, v, n, num_splits=0)


def test_requires_grad_is_an_error():
    q, k, v = make(2, 4, 2, 16, 64)
    n = torch.tensor([3, 16], dtype=torch.int32)
    with pytest.raises(RuntimeError, match="forward only"):
        flash_attention_decode(q.requires_grad_(), k, v, n)
    with torch.no_grad():
        flash_attention_decode(q, k, v, n)
