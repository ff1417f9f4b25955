"""The fixed-length causal dK/dV kernel starts its q-tile loop at the diagonal
(csrc/attn.hip fa_bwd_dkv_kernel, t0), as the variable-length one always did.
At B1 H2 S1024 D64 (8 key tiles, up to 14 skipped q tiles each) its dk and dv
are the bits of the variable-length kernels on the same single sequence."""

import pytest
import torch

pytestmark = pytest.mark.gpu


def test_fixed_length_causal_dkv_equals_varlen():
    from adapcc_amd.ops.attention import (flash_attention,
                                          flash_attention_varlen)

    H, S, D = 2, 1024, 64
    g = torch.Generator(device="cuda").manual_seed(5)
    q, k, v, do = (torch.randn(S, H, D, device="cuda", generator=g)
                   .to(torch.bfloat16) for _ in range(4))

    def batch4(t):  # [S,H,D] -> [1,H,S,D]
        return t.transpose(0, 1)[None]

    qf, kf, vf = (batch4(t).contiguous().requires_grad_(True)
                  for t in (q, k, v))
    of = flash_attention(qf, kf, vf, causal=True)
    of.backward(batch4(do).contiguous())

    cu = torch.tensor([0, S], dtype=torch.int32, device="cuda")
    qv, kv, vv = (t.clone().requires_grad_(True) for t in (q, k, v))
    ov = flash_attention_varlen(qv, kv, vv, cu, causal=True)
    ov.backward(do)

    assert torch.isfinite(kf.grad).all() and kf.grad.abs().sum() > 0
    assert torch.equal(batch4(ov.detach()), of.detach())
    assert torch.equal(batch4(kv.grad), kf.grad), "dk"
    assert torch.equal(batch4(vv.grad), vf.grad), "dv"
    assert torch.equal(batch4(qv.grad), qf.grad), "dq"
