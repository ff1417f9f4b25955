"""Hand-written CDNA4 flash attention (csrc/attn.hip) with autograd.

Supported fast paths, both bf16, head_dim 64, self-attention (q, k, v of one
shape), no dropout: causal with seq len a multiple of 128 (GPT-2), and
non-causal with any seq len >= 1 (ViT: 197). Anything else falls back to
torch SDPA. Tensors are [B, H, S, D] with any batch/head/row strides (rows
must be contiguous and 16-B aligned), so the usual
``.view(B,T,H,hd).transpose(1,2)`` projection views work without a copy.
``flash_attention_qkv`` takes the packed [B,T,3C] projection and returns
[B,T,C], reading and writing both layouts in place, in either mode.
"""

from __future__ import annotations

import math

import torch

from .fused import _core

__all__ = ["flash_attention", "flash_attention_qkv", "fa_supported",
           "fa_qkv_supported"]


def _strides3(t: torch.Tensor):
    return [t.stride(0), t.stride(1), t.stride(2)]


def _row_ok(t: torch.Tensor) -> bool:
    if t.stride(3) != 1:
        return False
    if t.data_ptr() % 16 != 0:
        return False
    # every row/plane base must stay 16-B aligned (bf16: 8 elements)
    return all(s % 8 == 0 for s in _strides3(t))


def _kernel_ok(t: torch.Tensor, D: int, S: int, causal: bool,
               dropout_p: float) -> bool:
    """What the kernels take, layout aside: bf16 on the GPU, head_dim 64,
    S >= 1 (a multiple of 128 when causal), no dropout, extension built."""
    if dropout_p != 0.0 or not (t.is_cuda and t.dtype == torch.bfloat16):
        return False
    if D != 64 or S < 1 or (causal and S % 128 != 0):
        return False
    return bool(_core())


def fa_supported(q: torch.Tensor, k: torch.Tensor, v: torch.Tensor,
                 causal: bool, dropout_p: float) -> bool:
    if q.dim() != 4 or q.shape != k.shape or q.shape != v.shape:
        return False
    if not (_row_ok(q) and _row_ok(k) and _row_ok(v)):
        return False
    return _kernel_ok(q, q.shape[3], q.shape[2], causal, dropout_p)


def _launch_fwd(q, k, v, o, lse, scale, causal=True):
    B, H, S, _ = q.shape
    strides = _strides3(q) + _strides3(k) + _strides3(v) + _strides3(o)
    stream = torch.cuda.current_stream(q.device).cuda_stream
    _core().fa_fwd(q.data_ptr(), k.data_ptr(), v.data_ptr(), o.data_ptr(),
                   lse.data_ptr(), B, H, S, strides, scale, stream, causal)


def _launch_bwd(q, k, v, o, dout, lse, dq, dk, dv, scale, causal=True,
                delta=None):
    """dq/dk/dv are written in place; delta = rowsum(dO*O) is computed by
    the dq kernel into a workspace (``delta``: contiguous [B,H,S] fp32, made
    here when not given) the dkv kernel then reads."""
    B, H, S, _ = q.shape
    # e.g. y.sum().backward() hands down an expanded, zero-stride dout
    do = dout if _row_ok(dout) else dout.contiguous()
    if delta is None:
        delta = torch.empty((B, H, S), dtype=torch.float32, device=q.device)
    strides = (_strides3(q) + _strides3(k) + _strides3(v) + _strides3(o) +
               _strides3(do) + _strides3(dq) + _strides3(dk) +
               _strides3(dv))
    stream = torch.cuda.current_stream(q.device).cuda_stream
    _core().fa_bwd(q.data_ptr(), k.data_ptr(), v.data_ptr(), o.data_ptr(),
                   do.data_ptr(), lse.data_ptr(), delta.data_ptr(),
                   dq.data_ptr(), dk.data_ptr(), dv.data_ptr(), B, H, S,
                   strides, scale, stream, causal)


def _fa_forward_lse(q, k, v, scale, causal):
    """Forward only: (o, lse), lse the [B,H,S] fp32 natural-log logsumexp
    of the scaled scores."""
    B, H, S, D = q.shape
    # O lives in [B,S,H,D] memory so the caller's
    # transpose(1,2).view(B,T,C) is free; returned as its [B,H,S,D] view
    o = torch.empty((B, S, H, D), dtype=q.dtype,
                    device=q.device).transpose(1, 2)
    lse = torch.empty((B, H, S), dtype=torch.float32, device=q.device)
    _launch_fwd(q, k, v, o, lse, scale, causal=causal)
    return o, lse


def _heads(t: torch.Tensor, n_head: int) -> torch.Tensor:
    """[B,T,C] (any row stride) -> its [B,H,T,C/H] view."""
    B, T, C = t.shape
    return t.view(B, T, n_head, C // n_head).transpose(1, 2)


class _FlashAttnFn(torch.autograd.Function):
    """[B,H,S,D] q, k, v; causal needs S % 128 == 0."""

    @staticmethod
    def forward(ctx, q, k, v, scale, causal):
        o, lse = _fa_forward_lse(q, k, v, scale, causal)
        ctx.save_for_backward(q, k, v, o, lse)
        ctx.scale, ctx.causal = scale, causal
        return o

    @staticmethod
    def backward(ctx, dout):
        q, k, v, o, lse = ctx.saved_tensors
        dq = torch.empty(q.shape, dtype=q.dtype, device=q.device)
        dk = torch.empty_like(dq)
        dv = torch.empty_like(dq)
        _launch_bwd(q, k, v, o, dout, lse, dq, dk, dv, ctx.scale,
                    causal=ctx.causal)
        return dq, dk, dv, None, None


class _FlashAttnQkvFn(torch.autograd.Function):
    """Attention straight off the packed projection: q, k, v are strided
    views of qkv [B,T,3C], O is written as [B,T,C], and the backward writes
    dq, dk, dv into the three thirds of one [B,T,3C] gradient."""

    @staticmethod
    def forward(ctx, qkv, n_head, scale, causal):
        B, T, C3 = qkv.shape
        C = C3 // 3
        q, k, v = (_heads(t, n_head) for t in qkv.split(C, dim=2))
        y = torch.empty((B, T, C), dtype=qkv.dtype, device=qkv.device)
        lse = torch.empty((B, n_head, T), dtype=torch.float32,
                          device=qkv.device)
        _launch_fwd(q, k, v, _heads(y, n_head), lse, scale, causal=causal)
        ctx.save_for_backward(qkv, y, lse)
        ctx.n_head, ctx.scale, ctx.causal = n_head, scale, causal
        return y

    @staticmethod
    def backward(ctx, dy):
        qkv, y, lse = ctx.saved_tensors
        H = ctx.n_head
        C = y.shape[2]
        q, k, v = (_heads(t, H) for t in qkv.split(C, dim=2))
        dqkv = torch.empty_like(qkv)
        dq, dk, dv = (_heads(t, H) for t in dqkv.split(C, dim=2))
        _launch_bwd(q, k, v, _heads(y, H), _heads(dy, H), lse, dq, dk, dv,
                    ctx.scale, causal=ctx.causal)
        return dqkv, None, None, None


def flash_attention(q: torch.Tensor, k: torch.Tensor, v: torch.Tensor,
                    causal: bool = True, dropout_p: float = 0.0,
                    scale: float = None) -> torch.Tensor:
    """SDPA drop-in for [B,H,S,D] inputs; runs the hand-written CDNA4
    kernels when the shape qualifies, torch SDPA otherwise."""
    if fa_supported(q, k, v, causal, dropout_p):
        s = scale if scale is not None else 1.0 / math.sqrt(q.shape[-1])
        return _FlashAttnFn.apply(q, k, v, s, causal)
    return torch.nn.functional.scaled_dot_product_attention(
        q, k, v, is_causal=causal, dropout_p=dropout_p, scale=scale)


def _attention_qkv_composed(qkv: torch.Tensor, n_head: int,
                            dropout_p: float = 0.0,
                            causal: bool = True) -> torch.Tensor:
    """split -> head views -> flash_attention -> [B,T,C]."""
    B, T, C3 = qkv.shape
    C = C3 // 3
    q, k, v = (_heads(t, n_head) for t in qkv.split(C, dim=2))
    y = flash_attention(q, k, v, causal=causal, dropout_p=dropout_p)
    return y.transpose(1, 2).contiguous().view(B, T, C)


def fa_qkv_supported(qkv: torch.Tensor, n_head: int,
                     dropout_p: float, causal: bool = True) -> bool:
    if qkv.dim() != 3 or qkv.shape[0] < 1 or qkv.shape[2] % (3 * n_head):
        return False
    if not qkv.is_contiguous() or qkv.data_ptr() % 16 != 0:
        return False
    return _kernel_ok(qkv, qkv.shape[2] // (3 * n_head), qkv.shape[1],
                      causal, dropout_p)


def flash_attention_qkv(qkv: torch.Tensor, n_head: int,
                        dropout_p: float = 0.0,
                        causal: bool = True) -> torch.Tensor:
    """Self-attention on the packed projection qkv [B,T,3C] (q, k, v
    thirds, heads contiguous within each); returns [B,T,C]. The qualifying
    case (bf16, head_dim 64, contiguous, no dropout; T a multiple of 128 when
    causal, any T >= 1 when not) runs the CDNA4 kernels directly on the
    packed layout with no copies; anything else composes
    ``flash_attention`` from views."""
    if fa_qkv_supported(qkv, n_head, dropout_p, causal):
        scale = 1.0 / math.sqrt(qkv.shape[2] // (3 * n_head))
        return _FlashAttnQkvFn.apply(qkv, n_head, scale, causal)
    return _attention_qkv_composed(qkv, n_head, dropout_p, causal)
