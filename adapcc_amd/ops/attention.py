"""Hand-written CDNA4 flash attention (csrc/attn.hip) with autograd.

Supported fast paths, both bf16, head_dim 64 or 128, self-attention (q, k, v
of one length), attention dropout 0 <= p < 1: causal with seq len a multiple
of 128 (GPT-2), and non-causal with any seq len >= 1 (ViT: 197). Anything else
falls back to torch SDPA. k and v may have fewer heads than q (grouped-query
attention, multi-query with one): q is [B,H,S,D], k and v [B,Hk,S,D] with
H % Hk == 0, and query head h reads K/V head h // (H // Hk). The kernels
index K/V that way themselves, and the backward sums dk and dv over each
group in its fp32 accumulators, so nothing is expanded or reduced outside
them and dk, dv have k's shape. Tensors are [B, H, S, D] with any
batch/head/row strides (rows must be contiguous and 16-B aligned), so the usual
``.view(B,T,H,hd).transpose(1,2)`` projection views work without a copy.
``flash_attention_qkv`` takes the packed [B,T,3C] projection and returns
[B,T,C], reading and writing both layouts in place, in either mode; with
``n_kv_head`` the projection is [B,T,(H + 2*Hk)*D], q columns, then k, then v.

Dropout acts on the attention probabilities inside the kernels. The mask is
a pure function keep(seed, b*H+h, q, k) (csrc/attn_drop.h) that the backward
regenerates, never a stored tensor (H and h are the query heads, also with
fewer K/V heads); kept probabilities are multiplied by
1/(1-p). The 64-bit seed is one int64 on the device, read when the kernels
run: drawn from torch's generator per call (so ``torch.manual_seed``
reproduces a run, without a host sync, and a captured graph that refills it
sees a fresh mask on every replay), or passed as ``dropout_seed``. It is
this project's own stream, not the Philox one of torch SDPA.
``dropout_keep_mask_reference`` is the same function in torch integer ops,
``fa_dropout_mask`` the kernels' own answer.

A third mode takes sequences of any lengths packed back to back:
``flash_attention_varlen`` on [total,H,D] tensors and
``flash_attention_qkv_varlen`` on the packed [total,3C] projection, both
with ``cu_seqlens`` (int32 [n_seqs + 1] row offsets on the device), causal
or not, with the same dropout. Attention is block-diagonal: a row sees only
its own sequence. No padding, no length condition and no host sync: a small
plan kernel turns ``cu_seqlens`` into the map from workgroup to (sequence,
tile) on the device (``varlen_tile_map_reference`` is its definition), so
the call can sit in a captured graph whose ``cu_seqlens`` is refilled
between replays. The dropout mask of sequence i, head h is plane i * H + h
of the same function, q and k counted from the sequence start. Off the
kernel path the same function is composed from torch SDPA under a
block-diagonal mask. To everything between the entry points and the kernels
this mode is the fixed-length call with B = 1, S = total and the map
(``tmap``) as one more argument.
"""

from __future__ import annotations

import math
from typing import Optional

import torch

from .fused import _core

__all__ = ["flash_attention", "flash_attention_qkv", "fa_supported",
           "fa_qkv_supported", "fa_dropout_mask",
           "dropout_keep_mask_reference", "flash_attention_varlen",
           "flash_attention_qkv_varlen", "fa_varlen_supported",
           "fa_qkv_varlen_supported", "varlen_tile_map_reference"]


_QT = 128  # rows per workgroup tile, csrc/attn.hip's kQT


def _strides3(t: torch.Tensor):
    return [t.stride(0), t.stride(1), t.stride(2)]


def _rows4(t: torch.Tensor) -> torch.Tensor:
    """[total,H,D] -> its [1,H,total,D] view, the kernels' tensor form."""
    return t.unsqueeze(0).transpose(1, 2)


def _bhsd(t: torch.Tensor) -> torch.Tensor:
    """The kernels' form of either layout: [B,H,S,D] as it is, packed
    sequences [total,H,D] as their [1,H,total,D] view."""
    return t if t.dim() == 4 else _rows4(t)


def _row_ok(t: torch.Tensor) -> bool:
    if t.stride(3) != 1:
        return False
    if t.data_ptr() % 16 != 0:
        return False
    # every row/plane base must stay 16-B aligned (bf16: 8 elements)
    return all(s % 8 == 0 for s in _strides3(t))


def _kernel_ok(t: torch.Tensor, D: int, S: int, causal: bool,
               dropout_p: float) -> bool:
    """What the kernels take, layout aside: bf16 on the GPU, head_dim 64
    or 128, S >= 1 (a multiple of 128 when causal), 0 <= dropout_p < 1,
    extension built."""
    if not 0.0 <= dropout_p < 1.0:
        return False
    if not (t.is_cuda and t.dtype == torch.bfloat16):
        return False
    if D not in (64, 128) or S < 1 or (causal and S % 128 != 0):
        return False
    return bool(_core())


def _gqa_shapes_ok(q: torch.Tensor, k: torch.Tensor, v: torch.Tensor,
                   heads_at: int) -> bool:
    """k and v of one shape that is q's in every dimension but the heads'
    (``heads_at``), where their size divides q's."""
    if q.dim() != k.dim() or k.shape != v.shape:
        return False
    H, Hk = q.shape[heads_at], k.shape[heads_at]
    if Hk < 1 or H % Hk != 0:
        return False
    return all(a == b for i, (a, b) in enumerate(zip(q.shape, k.shape))
               if i != heads_at)


def _qkv_ok(q: torch.Tensor, k: torch.Tensor, v: torch.Tensor, dim: int,
            causal: bool, dropout_p: float) -> bool:
    """Separate q, k, v of ``dim`` dimensions, heads in dimension 1."""
    if q.dim() != dim or not _gqa_shapes_ok(q, k, v, 1):
        return False
    q, k, v = _bhsd(q), _bhsd(k), _bhsd(v)
    if not (_row_ok(q) and _row_ok(k) and _row_ok(v)):
        return False
    return _kernel_ok(q, q.shape[3], q.shape[2], causal, dropout_p)


def fa_supported(q: torch.Tensor, k: torch.Tensor, v: torch.Tensor,
                 causal: bool, dropout_p: float) -> bool:
    """q [B,H,S,D]; k, v [B,Hk,S,D] of one shape with H % Hk == 0."""
    return _qkv_ok(q, k, v, 4, causal, dropout_p)


# ---------------------------------------------------------------------------
# Dropout mask
# ---------------------------------------------------------------------------
_M32 = 0xFFFFFFFF


def _drop_threshold(p: float) -> int:
    """keep iff word >= thr; round() ties to even, as the launcher does."""
    return min(max(round(p * 2 ** 32), 1), 2 ** 32 - 1)


def _fmix(x: torch.Tensor) -> torch.Tensor:
    # 32-bit values carried in int64: a product wraps mod 2^64, which keeps
    # its low 32 bits right; every shift sees a masked, non-negative value
    x = x ^ (x >> 16)
    x = (x * 0x85EBCA6B) & _M32
    x = x ^ (x >> 13)
    x = (x * 0xC2B2AE35) & _M32
    return x ^ (x >> 16)


def dropout_keep_mask_reference(seed, B: int, H: int, S: int,
                                p: float) -> torch.Tensor:
    """The kernels' keep(seed, bh, q, k) as a [B,H,S,S] bool tensor on the
    CPU, in torch integer ops (csrc/attn_drop.h is the definition). seed:
    int or one-element int64 tensor."""
    seed = int(seed) & 0xFFFFFFFFFFFFFFFF
    seed_lo, seed_hi = seed & _M32, seed >> 32
    bh = torch.arange(B * H, dtype=torch.int64).view(-1, 1)
    r = torch.arange(S, dtype=torch.int64).view(1, -1)
    a = _fmix((seed_lo + bh * 0x9E3779B1 + r * 0x85EBCA77) & _M32)
    b = _fmix(((seed_hi ^ ((bh * 0xC2B2AE3D) & _M32))
               + r * 0x27D4EB2F) & _M32)
    x = (a.view(B * H, S, 1) + b.view(B * H, 1, S)) & _M32
    x = (x * 0x2C1B3C6D) & _M32
    x = x ^ (x >> 15)
    x = (x * 0x297A2D39) & _M32
    x = x ^ (x >> 15)
    return (x >= _drop_threshold(p)).view(B, H, S, S)


def fa_dropout_mask(seed, B: int, H: int, S: int, p: float) -> torch.Tensor:
    """[B,H,S,S] bool, True where attention dropout at rate p keeps the
    probability. seed: one-element int64 tensor (or an int). A seed tensor
    on the GPU is answered by the kernels' own device function, anything
    else by the replica."""
    if not 0.0 <= p < 1.0:
        raise ValueError("fa_dropout_mask: need 0 <= p < 1")
    if isinstance(seed, torch.Tensor) and seed.is_cuda:
        core = _core()
        if not core:
            raise RuntimeError("fa_dropout_mask: native extension missing")
        s = _seed_tensor(seed, seed.device)
        out = torch.empty((B, H, S, S), dtype=torch.uint8, device=s.device)
        stream = torch.cuda.current_stream(s.device).cuda_stream
        core.fa_dropout_mask(out.data_ptr(), s.data_ptr(), B, H, S, p,
                             stream)
        return out.bool()
    return dropout_keep_mask_reference(seed, B, H, S, p)


def _seed_tensor(seed: Optional[torch.Tensor],
                 device: torch.device) -> torch.Tensor:
    """The one-element int64 device tensor the kernels read the seed from;
    drawn from torch's generator on the device when none is given."""
    if seed is None:
        return torch.randint(0, 2 ** 63 - 1, (1,), dtype=torch.int64,
                             device=device)
    if (seed.dtype != torch.int64 or seed.numel() != 1
            or seed.device != device):
        raise ValueError("dropout_seed: need a one-element int64 tensor on "
                         "the inputs' device")
    return seed.view(1)


def _tmap_kw(tmap: Optional[torch.Tensor], total: int):
    """The bindings' keywords for a tile map; none means fixed length. The
    map has total // 128 + n_seqs rows, which gives the sequence count."""
    if tmap is None:
        return {}
    return {"tmap": tmap.data_ptr(), "n_seqs": tmap.shape[0] - total // _QT}


def _launch_fwd(q, k, v, o, lse, scale, causal=True, dropout_p=0.0,
                seed=None, tmap=None):
    """q, k, v, o: [B,H,S,D]; lse: [B,H,S] fp32. With ``tmap``, the tile
    map of ``_varlen_plan``, they hold packed sequences: [1,H,total,D]
    views and [1,H,total]."""
    B, H, S, _ = q.shape
    strides = _strides3(q) + _strides3(k) + _strides3(v) + _strides3(o)
    stream = torch.cuda.current_stream(q.device).cuda_stream
    _core().fa_fwd(q.data_ptr(), k.data_ptr(), v.data_ptr(), o.data_ptr(),
                   lse.data_ptr(), B, H, S, strides, scale, stream, causal,
                   dropout_p, seed.data_ptr() if dropout_p > 0.0 else 0,
                   head_dim=q.shape[3], n_kv_head=k.shape[1],
                   **_tmap_kw(tmap, S))


def _launch_bwd(q, k, v, o, dout, lse, dq, dk, dv, scale, causal=True,
                delta=None, dropout_p=0.0, seed=None, tmap=None):
    """dq/dk/dv are written in place; delta = rowsum(dO*O) is computed by
    the dq kernel into a workspace (``delta``: contiguous [B,H,S] fp32, made
    here when not given) the dkv kernel then reads. With dropout, ``seed``
    is the forward's seed tensor. k, v, dk, dv may have fewer heads than q
    (H % Hk == 0); dk, dv are then the sums over each group. ``tmap`` as in
    ``_launch_fwd``."""
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
                   strides, scale, stream, causal, dropout_p,
                   seed.data_ptr() if dropout_p > 0.0 else 0,
                   head_dim=q.shape[3], n_kv_head=k.shape[1],
                   **_tmap_kw(tmap, S))


def _fa_forward_lse(q, k, v, scale, causal, dropout_p=0.0, seed=None,
                    tmap=None):
    """Forward only: (o, lse), lse the [B,H,S] fp32 natural-log logsumexp
    of the scaled scores (dropout does not enter it). With ``tmap`` q, k, v
    hold packed sequences, [total,H,D] or their [1,H,total,D] views, o comes
    back in q's form and lse is [1,H,total]."""
    B, H, S, D = _bhsd(q).shape
    if q.dim() == 4:
        # O lives in [B,S,H,D] memory so the caller's
        # transpose(1,2).view(B,T,C) is free; returned as its [B,H,S,D] view
        o = torch.empty((B, S, H, D), dtype=q.dtype,
                        device=q.device).transpose(1, 2)
    else:
        o = torch.empty((S, H, D), dtype=q.dtype, device=q.device)
    lse = torch.empty((B, H, S), dtype=torch.float32, device=q.device)
    _launch_fwd(_bhsd(q), _bhsd(k), _bhsd(v), _bhsd(o), lse, scale,
                causal=causal, dropout_p=dropout_p, seed=seed, tmap=tmap)
    return o, lse


def _heads(t: torch.Tensor, n_head: int) -> torch.Tensor:
    """[B,T,C] (any row stride) -> its [B,H,T,C/H] view; packed sequences
    [total,C] -> [1,H,total,C/H]."""
    if t.dim() == 2:
        t = t.unsqueeze(0)
    B, T, C = t.shape
    return t.view(B, T, n_head, C // n_head).transpose(1, 2)


def _kv_heads(name: str, n_head: int, n_kv_head: Optional[int]) -> int:
    """The K/V head count of a packed projection: n_head when not given."""
    Hk = n_head if n_kv_head is None else int(n_kv_head)
    if n_head < 1 or Hk < 1 or n_head % Hk != 0:
        raise ValueError(f"{name}: n_kv_head must divide n_head, got "
                         f"n_head {n_head}, n_kv_head {n_kv_head}")
    return Hk


def _qkv_parts(t: torch.Tensor, n_head: int, Hk: int):
    """The q, k, v column ranges of a packed [.., (H + 2*Hk)*D] tensor:
    H*D q columns, then Hk*D of k, then Hk*D of v (thirds when Hk == H)."""
    D = t.shape[-1] // (n_head + 2 * Hk)
    return t.split([n_head * D, Hk * D, Hk * D], dim=-1)


def _qkv_heads(t: torch.Tensor, n_head: int, Hk: int):
    """The three parts of t as [B,H,T,D], [B,Hk,T,D], [B,Hk,T,D] views."""
    q, k, v = _qkv_parts(t, n_head, Hk)
    return _heads(q, n_head), _heads(k, Hk), _heads(v, Hk)


def _drop_kw(ctx, seed):
    """Keyword arguments of the launch helpers for ctx's dropout; none at
    p = 0, so that path calls them exactly as before."""
    if ctx.dropout_p > 0.0:
        return {"dropout_p": ctx.dropout_p, "seed": seed}
    return {}


def _plan_of(cu_seqlens: Optional[torch.Tensor], total: int):
    """The tile map of a packed-sequence call; None at fixed length."""
    return None if cu_seqlens is None else _varlen_plan(cu_seqlens, total)


class _FlashAttnFn(torch.autograd.Function):
    """[B,H,S,D] q, k, v; causal needs S % 128 == 0. With cu_seqlens, the
    int32 row offsets of sequences held back to back, [total,H,D] q, k, v
    of any lengths. seed: the one-element int64 device tensor of the
    dropout mask, None at dropout_p = 0."""

    @staticmethod
    def forward(ctx, q, k, v, scale, causal, dropout_p=0.0, seed=None,
                cu_seqlens=None):
        ctx.scale, ctx.causal, ctx.dropout_p = scale, causal, dropout_p
        tmap = _plan_of(cu_seqlens, q.shape[0])
        o, lse = _fa_forward_lse(q, k, v, scale, causal, tmap=tmap,
                                 **_drop_kw(ctx, seed))
        # tmap and seed are None where the mode has none
        ctx.save_for_backward(q, k, v, o, lse, tmap, seed)
        return o

    @staticmethod
    def backward(ctx, dout):
        q, k, v, o, lse, tmap, seed = ctx.saved_tensors
        dq = torch.empty(q.shape, dtype=q.dtype, device=q.device)
        dk = torch.empty(k.shape, dtype=q.dtype, device=q.device)
        dv = torch.empty_like(dk)
        _launch_bwd(_bhsd(q), _bhsd(k), _bhsd(v), _bhsd(o), _bhsd(dout), lse,
                    _bhsd(dq), _bhsd(dk), _bhsd(dv), ctx.scale,
                    causal=ctx.causal, tmap=tmap, **_drop_kw(ctx, seed))
        return dq, dk, dv, None, None, None, None, None


class _FlashAttnQkvFn(torch.autograd.Function):
    """Attention straight off the packed projection: q, k, v are strided
    views of qkv [B,T,(H+2*Hk)*D] (n_kv_head None: Hk = H, [B,T,3C]), O is
    written as [B,T,H*D], and the backward writes dq, dk, dv into the three
    parts of one gradient of qkv's shape. With cu_seqlens, qkv is
    [total,(H+2*Hk)*D] and O [total,H*D], sequences back to back."""

    @staticmethod
    def forward(ctx, qkv, n_head, scale, causal, dropout_p=0.0, seed=None,
                n_kv_head=None, cu_seqlens=None):
        Hk = n_head if n_kv_head is None else n_kv_head
        C = qkv.shape[-1] // (n_head + 2 * Hk) * n_head
        q, k, v = _qkv_heads(qkv, n_head, Hk)
        B, _, T, _ = q.shape
        tmap = _plan_of(cu_seqlens, T)
        y = torch.empty((*qkv.shape[:-1], C), dtype=qkv.dtype,
                        device=qkv.device)
        lse = torch.empty((B, n_head, T), dtype=torch.float32,
                          device=qkv.device)
        ctx.n_head, ctx.scale, ctx.causal = n_head, scale, causal
        ctx.dropout_p, ctx.n_kv_head = dropout_p, Hk
        _launch_fwd(q, k, v, _heads(y, n_head), lse, scale, causal=causal,
                    tmap=tmap, **_drop_kw(ctx, seed))
        # tmap and seed are None where the mode has none
        ctx.save_for_backward(qkv, y, lse, tmap, seed)
        return y

    @staticmethod
    def backward(ctx, dy):
        qkv, y, lse, tmap, seed = ctx.saved_tensors
        H = ctx.n_head
        q, k, v = _qkv_heads(qkv, H, ctx.n_kv_head)
        dqkv = torch.empty_like(qkv)
        dq, dk, dv = _qkv_heads(dqkv, H, ctx.n_kv_head)
        _launch_bwd(q, k, v, _heads(y, H), _heads(dy, H), lse, dq, dk, dv,
                    ctx.scale, causal=ctx.causal, tmap=tmap,
                    **_drop_kw(ctx, seed))
        return dqkv, None, None, None, None, None, None, None


def flash_attention(q: torch.Tensor, k: torch.Tensor, v: torch.Tensor,
                    causal: bool = True, dropout_p: float = 0.0,
                    scale: float = None,
                    dropout_seed: Optional[torch.Tensor] = None
                    ) -> torch.Tensor:
    """SDPA drop-in for [B,H,S,D] inputs; runs the hand-written CDNA4
    kernels when the shape qualifies, torch SDPA otherwise. k and v may be
    [B,Hk,S,D] with H % Hk == 0 (grouped-query attention): query head h
    reads K/V head h // (H // Hk), and dk, dv come back in k's shape.
    dropout_seed
    (kernels only): one-element int64 tensor on the device that fixes the
    dropout mask; drawn from torch's generator when absent."""
    if fa_supported(q, k, v, causal, dropout_p):
        s = scale if scale is not None else 1.0 / math.sqrt(q.shape[-1])
        seed = (_seed_tensor(dropout_seed, q.device) if dropout_p > 0.0
                else None)
        return _FlashAttnFn.apply(q, k, v, s, causal, dropout_p, seed)
    gqa = False
    if q.dim() == 4 and k.dim() == 4 and v.dim() == 4:
        H, Hk = q.shape[1], k.shape[1]
        if v.shape[1] != Hk:
            raise ValueError("flash_attention: k and v must have one head "
                             f"count, got {Hk} and {v.shape[1]}")
        if Hk != H and (Hk < 1 or H % Hk != 0):
            raise ValueError("flash_attention: the K/V head count must "
                             f"divide q's, got {H} and {Hk}")
        gqa = Hk != H
    return torch.nn.functional.scaled_dot_product_attention(
        q, k, v, is_causal=causal, dropout_p=dropout_p, scale=scale,
        enable_gqa=gqa)


def _attention_qkv_composed(qkv: torch.Tensor, n_head: int,
                            dropout_p: float = 0.0,
                            causal: bool = True,
                            dropout_seed: Optional[torch.Tensor] = None,
                            n_kv_head: Optional[int] = None
                            ) -> torch.Tensor:
    """split -> head views -> flash_attention -> [B,T,C]."""
    B, T, C3 = qkv.shape
    Hk = _kv_heads("flash_attention_qkv", n_head, n_kv_head)
    q, k, v = _qkv_heads(qkv, n_head, Hk)
    y = flash_attention(q, k, v, causal=causal, dropout_p=dropout_p,
                        dropout_seed=dropout_seed)
    return y.transpose(1, 2).contiguous().view(B, T, n_head * q.shape[3])


def _packed_ok(qkv: torch.Tensor, dim: int, n_head: int,
               n_kv_head: Optional[int], causal: bool,
               dropout_p: float) -> bool:
    """A packed projection [.., S, (H + 2*Hk)*D] of ``dim`` dimensions."""
    try:
        W = n_head + 2 * _kv_heads("", n_head, n_kv_head)
    except ValueError:
        return False
    if qkv.dim() != dim or qkv.shape[0] < 1 or qkv.shape[-1] % W:
        return False
    if not qkv.is_contiguous() or qkv.data_ptr() % 16 != 0:
        return False
    return _kernel_ok(qkv, qkv.shape[-1] // W, qkv.shape[-2], causal,
                      dropout_p)


def fa_qkv_supported(qkv: torch.Tensor, n_head: int,
                     dropout_p: float, causal: bool = True,
                     n_kv_head: Optional[int] = None) -> bool:
    return _packed_ok(qkv, 3, n_head, n_kv_head, causal, dropout_p)


def flash_attention_qkv(qkv: torch.Tensor, n_head: int,
                        dropout_p: float = 0.0,
                        causal: bool = True,
                        dropout_seed: Optional[torch.Tensor] = None,
                        n_kv_head: Optional[int] = None
                        ) -> torch.Tensor:
    """Self-attention on the packed projection qkv [B,T,3C] (q, k, v
    thirds, heads contiguous within each); returns [B,T,C]. With n_kv_head
    = Hk < n_head (it must divide n_head) the projection is
    [B,T,(H + 2*Hk)*D]: H*D q columns, then Hk*D of k, then Hk*D of v, and
    the result [B,T,H*D]. The qualifying
    case (bf16, head_dim 64 or 128, contiguous, dropout_p < 1; T a multiple
    of 128 when causal, any T >= 1 when not) runs the CDNA4 kernels directly
    on the packed layout with no copies; anything else composes
    ``flash_attention`` from views. dropout_seed as in ``flash_attention``."""
    Hk = _kv_heads("flash_attention_qkv", n_head, n_kv_head)
    if fa_qkv_supported(qkv, n_head, dropout_p, causal, Hk):
        scale = 1.0 / math.sqrt(qkv.shape[2] // (n_head + 2 * Hk))
        seed = (_seed_tensor(dropout_seed, qkv.device) if dropout_p > 0.0
                else None)
        return _FlashAttnQkvFn.apply(qkv, n_head, scale, causal, dropout_p,
                                     seed, Hk)
    return _attention_qkv_composed(qkv, n_head, dropout_p, causal,
                                   dropout_seed, Hk)


# ---------------------------------------------------------------------------
# Variable-length (packed sequences) attention
# ---------------------------------------------------------------------------
def _check_cu_seqlens(name: str, cu_seqlens, device: torch.device) -> None:
    """Shape, dtype and device of cu_seqlens; its contents are never read
    on the host."""
    if not isinstance(cu_seqlens, torch.Tensor):
        raise ValueError(f"{name}: cu_seqlens must be a tensor")
    if cu_seqlens.dtype != torch.int32:
        raise ValueError(f"{name}: cu_seqlens must be int32, got "
                         f"{cu_seqlens.dtype}")
    if cu_seqlens.dim() != 1 or cu_seqlens.numel() < 2:
        raise ValueError(f"{name}: cu_seqlens must be 1-D with n_seqs + 1 "
                         f">= 2 elements, got shape "
                         f"{tuple(cu_seqlens.shape)}")
    if cu_seqlens.device != device:
        raise ValueError(f"{name}: cu_seqlens is on {cu_seqlens.device}, "
                         f"the inputs on {device}")


def _cu_ok(cu_seqlens, device: torch.device) -> bool:
    try:
        _check_cu_seqlens("", cu_seqlens, device)
    except ValueError:
        return False
    return cu_seqlens.is_contiguous() and cu_seqlens.data_ptr() % 4 == 0


def fa_varlen_supported(q: torch.Tensor, k: torch.Tensor, v: torch.Tensor,
                        cu_seqlens: torch.Tensor, causal: bool,
                        dropout_p: float) -> bool:
    """q [total,H,D]; k, v [total,Hk,D] of one shape with H % Hk == 0. No
    length condition, causal or not: any total >= 1."""
    return (_cu_ok(cu_seqlens, q.device)
            and _qkv_ok(q, k, v, 3, False, dropout_p))


def fa_qkv_varlen_supported(qkv: torch.Tensor, n_head: int,
                            cu_seqlens: torch.Tensor, dropout_p: float,
                            causal: bool = True,
                            n_kv_head: Optional[int] = None) -> bool:
    return (_cu_ok(cu_seqlens, qkv.device)
            and _packed_ok(qkv, 2, n_head, n_kv_head, False, dropout_p))


def varlen_tile_map_reference(cu_seqlens, total: int) -> torch.Tensor:
    """The plan of the variable-length kernels in plain Python: the int32
    [total // 128 + n_seqs, 4] map whose rows are (seq, tile, start, len),
    one per 128-row tile in sequence order, then -1 rows. This is the
    definition ``_core.fa_varlen_plan`` is held to.

    Sequence i is rows [e_i, e_i+1) with e_i = clamp(max(cu[0..i]), 0,
    total). On a well-formed vector that is cu_seqlens itself; on any other
    the sequences are still disjoint and inside [0, total), so their tiles
    fit the map and no kernel that follows it leaves the buffers. A sequence
    that comes out empty has no tile."""
    cu = [int(x) for x in torch.as_tensor(cu_seqlens).tolist()]
    total = int(total)
    n_seqs = len(cu) - 1
    if n_seqs < 1 or total < 1:
        raise ValueError("varlen_tile_map_reference: need n_seqs >= 1 and "
                         "total >= 1")

    def clamp(x):
        return min(max(x, 0), total)

    rows = []
    m = cu[0]
    for i in range(n_seqs):
        e = clamp(m)
        m = max(m, cu[i + 1])
        length = clamp(m) - e
        rows += [(i, j, e, length) for j in range(-(-length // _QT))]
    max_tiles = total // _QT + n_seqs
    assert len(rows) <= max_tiles
    rows += [(-1, -1, -1, -1)] * (max_tiles - len(rows))
    return torch.tensor(rows, dtype=torch.int32).view(max_tiles, 4)


def _varlen_plan(cu_seqlens: torch.Tensor, total: int) -> torch.Tensor:
    """Runs the plan kernel on the current stream; no host sync."""
    n_seqs = cu_seqlens.numel() - 1
    tmap = torch.empty((total // _QT + n_seqs, 4), dtype=torch.int32,
                       device=cu_seqlens.device)
    stream = torch.cuda.current_stream(cu_seqlens.device).cuda_stream
    _core().fa_varlen_plan(cu_seqlens.data_ptr(), n_seqs, total,
                           tmap.data_ptr(), stream)
    return tmap


def _varlen_mask(cu_seqlens: torch.Tensor, total: int,
                 causal: bool) -> torch.Tensor:
    """[total,total] bool, True where q row (dim 0) may see k row (dim 1):
    same sequence, and k <= q when causal. Built on cu_seqlens' device with
    no host sync."""
    rows = torch.arange(total, dtype=torch.int32, device=cu_seqlens.device)
    # sequence id of a row = number of sequence ends <= row
    sid = torch.bucketize(rows, cu_seqlens[1:].contiguous(), right=True)
    mask = sid.view(-1, 1) == sid.view(1, -1)
    if causal:
        mask = mask & (rows.view(1, -1) <= rows.view(-1, 1))
    return mask


def flash_attention_varlen(q: torch.Tensor, k: torch.Tensor, v: torch.Tensor,
                           cu_seqlens: torch.Tensor, causal: bool = True,
                           dropout_p: float = 0.0, scale: float = None,
                           dropout_seed: Optional[torch.Tensor] = None
                           ) -> torch.Tensor:
    """Self-attention over sequences packed back to back. q: [total,H,D],
    k, v: [total,Hk,D] with H % Hk == 0, query head h reading K/V head
    h // (H // Hk) (any row and head strides); cu_seqlens: int32 [n_seqs + 1]
    on the same device, sequence i owning rows cu_seqlens[i] ..
    cu_seqlens[i+1]-1. A row attends only inside its own sequence (and to
    keys at or before itself when causal). Returns [total,H,D].

    Contract for cu_seqlens, which is never read on the host and so not
    checked: non-decreasing, first entry 0, last entry total. Zero-length
    sequences are fine anywhere. A vector that breaks the contract gives
    unspecified values but no access outside the tensors.

    bf16 on the GPU with D = 64 or 128 runs the CDNA4 kernels (any lengths, no
    padding, no host sync; dropout mask plane seq * H + h with q and k
    counted from the sequence start); anything else runs torch SDPA under
    the block-diagonal mask, with torch's dropout."""
    if q.dim() != 3 or not _gqa_shapes_ok(q, k, v, 1):
        raise ValueError("flash_attention_varlen: need q [total,H,D] and "
                         "k, v [total,Hk,D] of one shape with H % Hk == 0, "
                         f"got {tuple(q.shape)}, {tuple(k.shape)}, "
                         f"{tuple(v.shape)}")
    _check_cu_seqlens("flash_attention_varlen", cu_seqlens, q.device)
    if fa_varlen_supported(q, k, v, cu_seqlens, causal, dropout_p):
        s = scale if scale is not None else 1.0 / math.sqrt(q.shape[-1])
        seed = (_seed_tensor(dropout_seed, q.device) if dropout_p > 0.0
                else None)
        return _FlashAttnFn.apply(q, k, v, s, causal, dropout_p, seed,
                                  cu_seqlens)
    mask = _varlen_mask(cu_seqlens, q.shape[0], causal)
    gqa = {"enable_gqa": True} if k.shape[1] != q.shape[1] else {}
    y = torch.nn.functional.scaled_dot_product_attention(
        _rows4(q), _rows4(k), _rows4(v), attn_mask=mask,
        dropout_p=dropout_p, scale=scale, **gqa)
    return y.squeeze(0).transpose(0, 1)


def flash_attention_qkv_varlen(qkv: torch.Tensor, n_head: int,
                               cu_seqlens: torch.Tensor,
                               dropout_p: float = 0.0, causal: bool = True,
                               dropout_seed: Optional[torch.Tensor] = None,
                               n_kv_head: Optional[int] = None
                               ) -> torch.Tensor:
    """``flash_attention_varlen`` on the packed projection qkv [total,3C]
    (q, k, v thirds, heads contiguous within each); returns [total,C]. With
    n_kv_head = Hk the row is (H + 2*Hk)*D wide, as in
    ``flash_attention_qkv``, and the result [total,H*D]. The
    qualifying case (bf16, head_dim 64 or 128, contiguous, dropout_p < 1)
    runs the kernels directly on the packed layout with no copies; anything else
    composes ``flash_attention_varlen`` from views. cu_seqlens: see there."""
    Hk = _kv_heads("flash_attention_qkv_varlen", n_head, n_kv_head)
    W = n_head + 2 * Hk
    if qkv.dim() != 2 or qkv.shape[1] % W:
        raise ValueError("flash_attention_qkv_varlen: qkv must be "
                         "[total, (n_head + 2 * n_kv_head) * D], got "
                         f"{tuple(qkv.shape)}")
    _check_cu_seqlens("flash_attention_qkv_varlen", cu_seqlens, qkv.device)
    total, C3 = qkv.shape
    D = C3 // W
    if fa_qkv_varlen_supported(qkv, n_head, cu_seqlens, dropout_p, causal,
                               Hk):
        scale = 1.0 / math.sqrt(D)
        seed = (_seed_tensor(dropout_seed, qkv.device) if dropout_p > 0.0
                else None)
        return _FlashAttnQkvFn.apply(qkv, n_head, scale, causal, dropout_p,
                                     seed, Hk, cu_seqlens)
    q, k, v = (t.view(total, -1, D) for t in _qkv_parts(qkv, n_head, Hk))
    y = flash_attention_varlen(q, k, v, cu_seqlens, causal=causal,
                               dropout_p=dropout_p,
                               dropout_seed=dropout_seed)
    return y.contiguous().view(total, n_head * D)
