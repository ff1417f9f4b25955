"""Non-causal, any-length mode of the hand-written CDNA4 flash attention
(csrc/attn.hip, ops/attention.py): numerics against a plain fp32 reference
at the sequence lengths where the ragged tail takes another path, the key
count through lse, the edge keys, padding neither read nor written, the
packed path, the rescale path, and the ViT block that uses it."""

import math

import pytest
import torch
from torch.utils._python_dispatch import TorchDispatchMode

from attn_util import record_launches, ref_attention_f32

pytestmark = pytest.mark.gpu

B, H, D = 2, 3, 64
SCALE = 1.0 / math.sqrt(D)
# 1: one valid key; 33: second 32-key half partly valid; 64: a whole 64-tile
# in a partial q-tile; 65: the prefetch stages a tile with one valid row;
# 128: aligned; 129: second workgroup has one row, dkv sums over two
# q-tiles; 197: ViT
SEQS = [1, 33, 64, 65, 128, 129, 197]


def rand(S, seed, b=B, h=H):
    torch.manual_seed(seed)
    return torch.randn(b, h, S, D, device="cuda", dtype=torch.bfloat16)


@pytest.mark.parametrize("S", SEQS)
def test_fwd_bwd_matches_reference(S):
    from adapcc_amd.ops.attention import fa_supported, flash_attention

    q = rand(S, 0).requires_grad_(True)
    k = rand(S, 1).requires_grad_(True)
    v = rand(S, 2).requires_grad_(True)
    assert fa_supported(q, k, v, False, 0.0)

    o = flash_attention(q, k, v, causal=False)
    ref = ref_attention_f32(q, k, v, SCALE, False)
    torch.testing.assert_close(o.float(), ref, rtol=2e-2, atol=2e-2)

    g = rand(S, 3)
    o.backward(g)
    qr = q.detach().float().requires_grad_(True)
    kr = k.detach().float().requires_grad_(True)
    vr = v.detach().float().requires_grad_(True)
    ref_attention_f32(qr, kr, vr, SCALE, False).backward(g.float())
    torch.testing.assert_close(q.grad.float(), qr.grad, rtol=5e-2, atol=5e-2)
    torch.testing.assert_close(k.grad.float(), kr.grad, rtol=5e-2, atol=5e-2)
    torch.testing.assert_close(v.grad.float(), vr.grad, rtol=5e-2, atol=5e-2)


@pytest.mark.parametrize("S", SEQS)
def test_lse_counts_keys(S):
    """q = 0 makes every score exactly 0, so lse = log(S): one key more or
    less moves it by >= 1/(S+1) >= 5e-3, fp32 log error is ~1e-6."""
    from adapcc_amd.ops.attention import _fa_forward_lse

    q = torch.zeros(B, H, S, D, device="cuda", dtype=torch.bfloat16)
    k, v = rand(S, 4), rand(S, 5)
    _, lse = _fa_forward_lse(q, k, v, SCALE, False)
    assert lse.shape == (B, H, S)
    want = torch.full_like(lse, math.log(S))
    torch.testing.assert_close(lse, want, rtol=0, atol=1e-4)


@pytest.mark.parametrize("S", [197, 65])
@pytest.mark.parametrize("which", ["last", "first"])
def test_edge_keys_counted(S, which):
    """One key takes essentially all the softmax weight: score 16 against 0
    for the others (weight of the rest <= 196 * e^-16 ~ 2e-5)."""
    from adapcc_amd.ops.attention import flash_attention

    e = S - 1 if which == "last" else 0
    q = torch.full((B, H, S, D), 0.5, device="cuda", dtype=torch.bfloat16)
    k = torch.zeros_like(q)
    k[:, :, e] = 4.0
    v = rand(S, 6)
    q.requires_grad_(True)
    k.requires_grad_(True)
    v.requires_grad_(True)
    o = flash_attention(q, k, v, causal=False)
    want = v.detach()[:, :, e:e + 1].float().expand(B, H, S, D)
    torch.testing.assert_close(o.float(), want, rtol=2e-2, atol=2e-2)

    g = torch.ones_like(o)
    o.backward(g)  # dv[e] = sum_q P[q,e] g[q]: the column sum of g, = S
    want_dv = g.float().sum(dim=2)
    torch.testing.assert_close(v.grad[:, :, e].float(), want_dv, rtol=5e-2,
                               atol=5e-2)


def _padded(S, seed, fill):
    """[B,H,S,D] slice of a [B,H,Sp,D] buffer whose rows >= S hold fill."""
    Sp = (S + 127) // 128 * 128
    buf = torch.full((B, H, Sp, D), fill, device="cuda",
                     dtype=torch.bfloat16)
    buf[:, :, :S] = rand(S, seed)
    return buf, buf[:, :, :S]


def _run_raw(q, k, v, do, o, lse, dq, dk, dv, delta):
    from adapcc_amd.ops.attention import _launch_bwd, _launch_fwd

    _launch_fwd(q, k, v, o, lse, SCALE, causal=False)
    _launch_bwd(q, k, v, o, do, lse, dq, dk, dv, SCALE, causal=False,
                delta=delta)
    torch.cuda.synchronize()


@pytest.mark.parametrize("S", [197, 65])
def test_padding_never_read(S):
    """NaN in rows >= S of every input buffer changes no bit of any result."""
    results = []
    for fill in (float("nan"), 0.0):
        _, q = _padded(S, 10, fill)
        _, k = _padded(S, 11, fill)
        _, v = _padded(S, 12, fill)
        _, do = _padded(S, 13, fill)
        # o is read back by the backward: its padding is an input too
        _, o = _padded(S, 14, fill)
        _, dq = _padded(S, 15, 0.0)
        _, dk = _padded(S, 16, 0.0)
        _, dv = _padded(S, 17, 0.0)
        lse = torch.empty(B, H, S, device="cuda", dtype=torch.float32)
        delta = torch.empty_like(lse)
        _run_raw(q, k, v, do, o, lse, dq, dk, dv, delta)
        results.append([t.clone() for t in (o, lse, delta, dq, dk, dv)])
    for got, want in zip(*results):
        assert torch.isfinite(got).all()
        torch.testing.assert_close(got, want, rtol=0, atol=0)


@pytest.mark.parametrize("S", [197, 1])
def test_padding_never_written(S):
    """Rows >= S of o, dq, dk, dv and the entries after lse and delta keep
    their sentinel, bit for bit."""
    sent = 1234.0  # exact in bf16 and fp32
    _, q = _padded(S, 20, 0.0)
    _, k = _padded(S, 21, 0.0)
    _, v = _padded(S, 22, 0.0)
    _, do = _padded(S, 23, 0.0)
    outs = [_padded(S, 24 + i, sent) for i in range(4)]  # o, dq, dk, dv
    n = B * H * S
    flat = [torch.full((n + 256,), sent, device="cuda", dtype=torch.float32)
            for _ in range(2)]
    lse, delta = (f[:n].view(B, H, S) for f in flat)
    _run_raw(q, k, v, do, outs[0][1], lse, outs[1][1], outs[2][1],
             outs[3][1], delta)
    for buf, view in outs:
        assert torch.isfinite(view.float()).all()
        guard = buf[:, :, S:]
        assert guard.numel() > 0
        assert (guard == sent).all()
    for f in flat:
        assert torch.isfinite(f[:n]).all()
        assert (f[n:] == sent).all()
    # and the rows that are written are right
    ref = ref_attention_f32(q, k, v, SCALE, False)
    torch.testing.assert_close(outs[0][1].float(), ref, rtol=2e-2, atol=2e-2)


class _RecordOps(TorchDispatchMode):
    def __init__(self):
        super().__init__()
        self.names = []

    def __torch_dispatch__(self, func, types, args=(), kwargs=None):
        self.names.append(str(func))
        return func(*args, **(kwargs or {}))


def test_packed_equals_composed_bitwise_no_copies():
    from adapcc_amd.ops.attention import (_attention_qkv_composed,
                                          fa_qkv_supported,
                                          flash_attention_qkv)

    T, C = 197, H * D
    torch.manual_seed(30)
    qkv = torch.randn(B, T, 3 * C, device="cuda", dtype=torch.bfloat16)
    g = torch.randn(B, T, C, device="cuda", dtype=torch.bfloat16)
    assert fa_qkv_supported(qkv, H, 0.0, causal=False)
    assert not fa_qkv_supported(qkv, H, 0.0)  # causal: T % 128 != 0

    x0 = qkv.clone().requires_grad_(True)
    want = _attention_qkv_composed(x0, H, causal=False)
    want.backward(g)

    x1 = qkv.clone().requires_grad_(True)
    with _RecordOps() as rec:
        y = flash_attention_qkv(x1, H, causal=False)
        (gx,) = torch.autograd.grad(y, x1, g)
    assert y.shape == (B, T, C) and y.is_contiguous()
    torch.testing.assert_close(y.detach(), want.detach(), rtol=0, atol=0)
    assert torch.isfinite(gx).all()
    torch.testing.assert_close(gx, x0.grad, rtol=0, atol=0)

    # no pass over the activations besides the kernels: nothing that
    # copies, concatenates or makes contiguous
    assert rec.names, "dispatch mode saw nothing"
    copies = [n for n in rec.names
              if any(w in n for w in ("cat", "clone", "copy", "contiguous"))]
    assert not copies, copies


def test_extreme_values_stable():
    """The spiked key of test_fa_extreme_values_stable, at S = 197: a later
    tile forces a max jump past the defer-max threshold."""
    from adapcc_amd.ops.attention import flash_attention

    torch.manual_seed(2)
    S = 197
    q = (torch.randn(1, 2, S, D, device="cuda") * 4).to(torch.bfloat16)
    k = (torch.randn(1, 2, S, D, device="cuda") * 4).to(torch.bfloat16)
    k[:, :, 150, :] *= 8
    v = torch.randn(1, 2, S, D, device="cuda").to(torch.bfloat16)
    o = flash_attention(q, k, v, causal=False)
    assert torch.isfinite(o.float()).all()
    ref = ref_attention_f32(q, k, v, SCALE, False)
    torch.testing.assert_close(o.float(), ref, rtol=3e-2, atol=3e-2)


def test_vit_block_takes_fast_path(monkeypatch):
    """One ViT-base encoder block in bf16 against the same weights run
    through the split / SDPA / contiguous formula it replaced."""
    import torch.nn.functional as F

    from adapcc_amd.models.vit import EncoderBlock

    torch.manual_seed(40)
    dim, heads, T = 768, 12, 197
    blk = EncoderBlock(dim, heads, 3072).to("cuda").to(torch.bfloat16)
    x = torch.randn(2, T, dim, device="cuda", dtype=torch.bfloat16)
    g = torch.randn_like(x)

    def old_forward(x):
        Bx, Tx, C = x.shape
        h = blk.ln1(x)
        q, k, v = blk.qkv(h).split(C, dim=2)
        hd = C // heads
        q = q.view(Bx, Tx, heads, hd).transpose(1, 2)
        k = k.view(Bx, Tx, heads, hd).transpose(1, 2)
        v = v.view(Bx, Tx, heads, hd).transpose(1, 2)
        a = F.scaled_dot_product_attention(q, k, v)
        a = a.transpose(1, 2).contiguous().view(Bx, Tx, C)
        x = x + blk.proj(a)
        return x + blk.mlp(blk.ln2(x))

    calls = record_launches(monkeypatch)

    x_new = x.clone().requires_grad_(True)
    y_new = blk(x_new)
    y_new.backward(g)
    assert calls == [("fwd", False, 0.0, False), ("bwd", False, 0.0, False)]

    x_old = x.clone().requires_grad_(True)
    y_old = old_forward(x_old)
    y_old.backward(g)
    assert len(calls) == 2

    torch.testing.assert_close(y_new.detach().float(), y_old.detach().float(),
                               rtol=2e-2, atol=2e-2)
    torch.testing.assert_close(x_new.grad.float(), x_old.grad.float(),
                               rtol=5e-2, atol=5e-2)
