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

``flash_attention_decode`` is the generation step: one new query row per
sequence, q [B,H,D], against a KV cache [B,Hk,Smax,D] of which
``cache_seqlens`` (int32 [B] on the device) says how many keys count, with
the same head grouping. Its kernels (csrc/attn_decode.hip) split the keys,
not the query rows, over workgroups, read every K/V byte once per K/V head
for all H // Hk query heads, and merge the splits deterministically. The
split count depends on the shapes alone, so there is no host sync either and
a captured graph whose lengths are refilled stays valid. With ``k_new`` and
``v_new`` the new token's rows are first written into the cache in place.
Forward only.

``flash_attention_extend`` is the same over a block of rows: q [B,H,Sq,D]
against the cache, optionally appending the block's own k and v rows
([B,Hk,Sq,D]) first, with ``q_lens`` for a ragged block. Causal, row i sees
keys up to total_b - n_b + i (bottom-right aligned: chunked prefill, a
further turn on a kept cache, drafted tokens); non-causal it is
cross-attention over the cached keys. Its kernel (csrc/attn_extend.hip)
gives a workgroup one K/V head and 128 rows of the flattened (position, query
head) axis, so a K/V tile is staged once for all H // Hk heads and a short
chunk under GQA still fills its MFMA columns. A short chunk over a long
cache is also split over the keys, as decode is: the split count comes from
the shapes alone, the splits leave fp32 partials and a second kernel merges
them deterministically. No host sync; forward only.

Decode is extend at Sq = 1 with new rows and no ``q_lens``, so the two share
their host path: ``_check_cached``, ``_cached_kernel_ok``, the launch preamble
``_cached_launch_args``, one append kernel (csrc/attn_cache.h) and, off the
kernel path, ``_extend_composed`` (a masked rewrite of the caches, then torch
SDPA under the explicit mask), which decode calls on ``unsqueeze(2)`` views.

Both calls also take a paged cache: with ``block_table`` (int32
[B,max_pages] on the device) k_cache and v_cache are pools [N,Hk,P,D] of N
pages of P key rows, logical row j of sequence b lives in row j % P of page
block_table[b, j // P], and max_pages * P stands where Smax did. The kernels
look the page up themselves (csrc/attn_cache.h's ``paged_offset``; entries
clamped to [0, N-1] on the device), so nothing is gathered, the table is
never read on the host, and memory grows with the tokens held, sequences of
any lengths share one pool and a common prefix is stored once. P must be a
power of two >= 16 there; ``_paged_composed`` (gather, compose, write the
appended rows back) is the route for everything else and the definition.

Decode also takes an FP8 cache: k_cache and v_cache (slabs or pools) of
``torch.float8_e4m3fn`` with per-head ``k_scale``, ``v_scale`` (fp32 [Hk] on
the device), a stored byte c of head hk standing for float(c) * scale[hk].
Half the memory per key and half the bytes a step reads, which is what
bounds decode. The kernels (csrc/attn_decode_fp8.hip) load the bytes in a
layout of their own, dequantise in registers (e4m3 -> bf16 is exact) into
the bf16 MFMA path, and fold the scales into the softmax scale and the final
normalisation; q, the new rows and the output stay bf16. Rows are quantised
when they are written, by one function, ``kv_quantize_reference``
(divide, clamp to +-448, round to nearest even): by decode's own append and
by ``kv_cache_append``, the append step alone, which is one way a prompt
enters such a cache. ``flash_attention_extend`` takes the same caches and
scales (csrc/attn_extend_fp8.hip: the bytes are converted once per workgroup
on their way into LDS, and the bf16 kernel's tiles, MFMAs and split merge do
the rest): chunked prefill, a further turn and drafted tokens run on the e4m3
cache itself. It quantises a chunk's rows first and attends over them as
stored, so a prompt sees the same keys however it is chunked.
"""

from __future__ import annotations

import math
from typing import NamedTuple, Optional

import torch

from .fused import _core

__all__ = ["flash_attention", "flash_attention_qkv", "fa_supported",
           "fa_qkv_supported", "fa_dropout_mask",
           "dropout_keep_mask_reference", "flash_attention_varlen",
           "flash_attention_qkv_varlen", "fa_varlen_supported",
           "fa_qkv_varlen_supported", "varlen_tile_map_reference",
           "flash_attention_decode", "fa_decode_supported",
           "flash_attention_extend", "fa_extend_supported",
           "kv_cache_append", "kv_quantize_reference"]


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
    """Rows (the last dimension) contiguous and 16-B aligned, whatever the
    number of leading dimensions."""
    if t.stride(-1) != 1:
        return False
    if t.data_ptr() % 16 != 0:
        return False
    # every row/plane base must stay 16-B aligned (bf16: 8 elements; one-byte
    # elements, the e4m3 caches: 16)
    step = 16 if t.element_size() == 1 else 8
    return all(s % step == 0 for s in t.stride()[:-1])


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


# ---------------------------------------------------------------------------
# Attention over a KV cache: what decode (one query row per sequence) and
# extend (a block of rows) share
# ---------------------------------------------------------------------------
_DECODE_MAX_GROUP = 32  # csrc/attn_decode_plan.h's kDecodeMaxGroup
_PAGED_MAX_KEYS = 1 << 30   # its bound on Smax, for max_pages * P


def _is_fp8(k_cache, v_cache) -> bool:
    return k_cache.dtype == v_cache.dtype == torch.float8_e4m3fn


def _check_cached(name, q, k_cache, v_cache, cache_seqlens, k_new, v_new,
                  q_lens=None, block_table=None, k_scale=None, v_scale=None,
                  fp8_ok=False) -> None:
    """The argument checks of the calls over a KV cache. q is [B,H,D]
    (decode) or [B,H,Sq,D] (extend), new rows then [B,Hk,D] or [B,Hk,Sq,D];
    q_lens (extend) like cache_seqlens. With block_table (int32
    [B,max_pages]) the caches are page pools [N,Hk,P,D]. fp8_ok (decode, extend
    and ``kv_cache_append``): e4m3 caches under a q of another float dtype are
    taken, with k_scale and v_scale, fp32 [Hk]."""
    rows = "" if name.endswith("decode") else "Sq,"
    paged = block_table is not None
    form = "[N,Hk,P,D]" if paged else "[B,Hk,Smax,D]"
    if (q.dim() != (4 if rows else 3) or k_cache.dim() != 4
            or k_cache.shape != v_cache.shape):
        raise ValueError(f"{name}: need q [B,H,{rows}D] and k_cache, v_cache "
                         f"{form} of one shape, got {tuple(q.shape)}, "
                         f"{tuple(k_cache.shape)}, {tuple(v_cache.shape)}")
    B, H, D = q.shape[0], q.shape[1], q.shape[-1]
    Bk, Hk, Smax, Dk = k_cache.shape
    if paged:
        if not isinstance(block_table, torch.Tensor):
            raise ValueError(f"{name}: block_table must be a tensor")
        if block_table.dtype != torch.int32:
            raise ValueError(f"{name}: block_table must be int32, got "
                             f"{block_table.dtype}")
        if (block_table.dim() != 2 or block_table.shape[0] != B
                or block_table.shape[1] < 1):
            raise ValueError(f"{name}: block_table must be [B,max_pages] = "
                             f"[{B},>=1], got {tuple(block_table.shape)}")
        if block_table.device != q.device:
            raise ValueError(f"{name}: block_table is on "
                             f"{block_table.device}, the inputs on {q.device}")
        if block_table.shape[1] * Smax > _PAGED_MAX_KEYS:
            raise ValueError(f"{name}: max_pages * P = "
                             f"{block_table.shape[1]} * {Smax} keys is over "
                             f"2^30")
        Bk = B      # the pool's first dimension counts pages, not sequences
    if Bk != B or Dk != D or min(*q.shape, Hk, Smax) < 1:
        raise ValueError(f"{name}: q {tuple(q.shape)} and the caches "
                         f"{tuple(k_cache.shape)} do not agree in batch and "
                         "head_dim (or a dimension is empty)")
    if H % Hk != 0:
        raise ValueError(f"{name}: the K/V head count must divide q's, got "
                         f"{H} and {Hk}")
    if (fp8_ok and _is_fp8(k_cache, v_cache) and q.is_floating_point()
            and q.element_size() > 1):
        for n, t in (("k_scale", k_scale), ("v_scale", v_scale)):
            if (not isinstance(t, torch.Tensor) or t.dtype != torch.float32
                    or t.shape != (Hk,) or not t.is_contiguous()
                    or t.device != q.device):
                raise ValueError(f"{name}: an e4m3 cache needs {n}, fp32 "
                                 f"[Hk] = [{Hk}], contiguous, on {q.device}")
    elif not (q.dtype == k_cache.dtype == v_cache.dtype):
        raise ValueError(f"{name}: q and the caches must have one dtype, got "
                         f"{q.dtype}, {k_cache.dtype}, {v_cache.dtype}")
    elif k_scale is not None or v_scale is not None:
        raise ValueError(f"{name}: k_scale and v_scale go with e4m3 "
                         f"(torch.float8_e4m3fn) caches, got {k_cache.dtype}")
    if not (q.device == k_cache.device == v_cache.device):
        raise ValueError(f"{name}: q and the caches must be on one device")
    for n, t in (("cache_seqlens", cache_seqlens), ("q_lens", q_lens)):
        if t is None and n == "q_lens":
            continue
        if not isinstance(t, torch.Tensor):
            raise ValueError(f"{name}: {n} must be a tensor")
        if t.dtype != torch.int32:
            raise ValueError(f"{name}: {n} must be int32, got {t.dtype}")
        if t.shape != (B,):
            raise ValueError(f"{name}: {n} must be [B] = [{B}], got "
                             f"{tuple(t.shape)}")
        if t.device != q.device:
            raise ValueError(f"{name}: {n} is on {t.device}, the inputs on "
                             f"{q.device}")
    if (k_new is None) != (v_new is None):
        raise ValueError(f"{name}: pass k_new and v_new together or neither")
    want = (B, Hk) + tuple(q.shape[2:])
    for n, t in (("k_new", k_new), ("v_new", v_new)):
        if t is None:
            continue
        if t.shape != want or t.dtype != q.dtype or t.device != q.device:
            raise ValueError(f"{name}: {n} must be [B,Hk,{rows}D] = "
                             f"{list(want)} of q's dtype and device, got "
                             f"{tuple(t.shape)} {t.dtype} on {t.device}")


def _check_no_grad(name, *tensors) -> None:
    if torch.is_grad_enabled() and any(
            t is not None and t.requires_grad for t in tensors):
        raise RuntimeError(f"{name}: forward only, but an input requires "
                           "grad; call it under torch.no_grad()")


def _cached_kernel_ok(q, k_cache, v_cache, cache_seqlens,
                      q_lens=None, block_table=None) -> bool:
    """Where the cached calls run their kernels, for arguments that
    ``_check_cached`` has passed."""
    if block_table is not None:
        P = k_cache.shape[2]
        # the kernels split a row index with a shift and a mask
        if P < 16 or P & (P - 1) or not block_table.is_contiguous():
            return False
    if not (q.is_cuda and q.dtype == torch.bfloat16):
        return False
    if q.shape[-1] not in (64, 128):
        return False
    if q.shape[1] // k_cache.shape[1] > _DECODE_MAX_GROUP:
        return False
    if not (_row_ok(q) and _row_ok(k_cache) and _row_ok(v_cache)):
        return False
    if not cache_seqlens.is_contiguous():
        return False
    if q_lens is not None and not q_lens.is_contiguous():
        return False
    return bool(_core())


class _CachedLaunch(NamedTuple):
    """What both kernel launches over a cache build the same way."""
    kw: dict            # pointers: k_new, v_new (with new rows), lse (asked for)
    new_strides: list   # of the new rows, k's then v's; zeros without them
    lse: Optional[torch.Tensor]     # fp32, q's shape without D, or None
    device: int         # q's index: the launchers make it current
    stream: int         # that device's current stream
    Smax: int           # the cache's capacity: max_pages * P when paged
    # the tensors kw's k_new, v_new point into (contiguous copies of rows not
    # 16-B aligned): alive while the launcher holds this result
    new_rows: Optional[tuple]


def _cached_launch_args(q, k_cache, k_new, v_new, return_lse,
                        block_table=None) -> _CachedLaunch:
    kw = {}
    Smax = k_cache.shape[2]
    if block_table is not None:
        N, P, max_pages = k_cache.shape[0], Smax, block_table.shape[1]
        kw.update(block_table=block_table.data_ptr(), n_pages=N, page_size=P,
                  max_pages=max_pages)
        Smax = max_pages * P
    new_rows = None
    new_strides = [0] * (2 * (q.dim() - 1))
    if k_new is not None:
        new_rows = tuple(t if _row_ok(t) else t.contiguous()
                         for t in (k_new, v_new))
        kw.update(k_new=new_rows[0].data_ptr(), v_new=new_rows[1].data_ptr())
        new_strides = list(new_rows[0].stride()[:-1]
                           + new_rows[1].stride()[:-1])
    lse = None
    if return_lse:
        lse = torch.empty(q.shape[:-1], dtype=torch.float32, device=q.device)
        kw.update(lse=lse.data_ptr())
    return _CachedLaunch(kw, new_strides, lse, q.get_device(),
                         torch.cuda.current_stream(q.device).cuda_stream,
                         Smax, new_rows)


# ---------------------------------------------------------------------------
# Decode: one query row per sequence against a KV cache
# ---------------------------------------------------------------------------
def fa_decode_supported(q: torch.Tensor, k_cache: torch.Tensor,
                        v_cache: torch.Tensor,
                        cache_seqlens: torch.Tensor,
                        block_table: Optional[torch.Tensor] = None,
                        k_scale: Optional[torch.Tensor] = None,
                        v_scale: Optional[torch.Tensor] = None) -> bool:
    """True where ``flash_attention_decode`` runs its kernels: bf16 q on the
    GPU, head_dim 64 or 128, at most 32 query heads per K/V head, rows
    contiguous and 16-B aligned, extension built; with ``block_table`` also
    a page size that is a power of two >= 16 and a contiguous table. The
    caches are bf16, or e4m3 with ``k_scale`` and ``v_scale``."""
    try:
        _check_cached("flash_attention_decode", q, k_cache, v_cache,
                      cache_seqlens, None, None, None, block_table, k_scale,
                      v_scale, fp8_ok=True)
    except ValueError:
        return False
    return _cached_kernel_ok(q, k_cache, v_cache, cache_seqlens, None,
                             block_table)


def _launch_decode(q, k_cache, v_cache, cache_seqlens, k_new, v_new, scale,
                   num_splits, return_lse, block_table=None, k_scale=None,
                   v_scale=None):
    """The kernel path, for arguments that passed ``_check_cached`` and
    ``_cached_kernel_ok``. With the scales: e4m3 caches and the kernels of
    csrc/attn_decode_fp8.hip."""
    core = _core()
    B, H, D = q.shape
    Hk = k_cache.shape[1]
    a = _cached_launch_args(q, k_cache, k_new, v_new, return_lse, block_table)
    Smax = a.Smax
    ns = core.fa_decode_splits(B, Hk, Smax,
                               0 if num_splits is None else int(num_splits),
                               a.device)
    out = torch.empty((B, H, D), dtype=q.dtype, device=q.device)
    if ns > 1:
        o_part = torch.empty((B, H, ns, D), dtype=torch.float32,
                             device=q.device)
        lse_part = torch.empty((B, H, ns), dtype=torch.float32,
                               device=q.device)
        a.kw.update(o_part=o_part.data_ptr(), lse_part=lse_part.data_ptr())
    strides = ([q.stride(0), q.stride(1)] + _strides3(k_cache)
               + _strides3(v_cache) + a.new_strides)
    if k_scale is not None:
        core.fa_decode_fp8(q.data_ptr(), k_cache.data_ptr(),
                           v_cache.data_ptr(), cache_seqlens.data_ptr(),
                           k_scale.data_ptr(), v_scale.data_ptr(),
                           out.data_ptr(), B, H, Hk, Smax, D, strides, scale,
                           ns, a.device, a.stream, **a.kw)
    else:
        core.fa_decode(q.data_ptr(), k_cache.data_ptr(), v_cache.data_ptr(),
                       cache_seqlens.data_ptr(), out.data_ptr(), B, H, Hk,
                       Smax, D, strides, scale, ns, a.device, a.stream,
                       **a.kw)
    return (out, a.lse) if return_lse else out


# ---------------------------------------------------------------------------
# FP8 (e4m3) caches: the quantisation function, the append step alone, and
# decode off the kernel path
# ---------------------------------------------------------------------------
def kv_quantize_reference(x: torch.Tensor, scale: torch.Tensor) -> torch.Tensor:
    """The one quantisation function of the e4m3 caches, in torch:
    q8(x, s) = rne_e4m3(clamp(float(x) / s, -448, 448)) as
    ``torch.float8_e4m3fn``. x has the K/V heads in dim 1, scale is [Hk]
    (> 0). The clamp is part of the definition: without it a value past 448
    becomes NaN. The append kernel (csrc/attn_decode_fp8.hip) computes the
    same with an fp32 division."""
    s = scale.float().view((1, -1) + (1,) * (x.dim() - 2))
    return (x.float() / s).clamp(-448.0, 448.0).to(torch.float8_e4m3fn)


def _append_composed(k_cache, v_cache, cache_seqlens, k_new, v_new, q_lens,
                     block_table) -> None:
    """The append step off the kernel path: ``_paged_composed``'s write-back
    (a masked rewrite through an inverse index, no host sync), a slab being
    the pool of B pages of Smax rows under the table arange(B). One-byte
    caches move as uint8: k_new, v_new are quantised already."""
    B, Hk, Sq, D = k_new.shape
    N, P = k_cache.shape[0], k_cache.shape[2]
    dev = k_new.device
    if block_table is None:
        table = torch.arange(B, device=dev).view(B, 1)
    else:
        table = block_table.clamp(0, N - 1).long()
    Smax = table.shape[1] * P
    past = cache_seqlens.clamp(0, Smax).view(B, 1).long()
    n = (torch.full_like(cache_seqlens, Sq) if q_lens is None
         else q_lens.clamp(0, Sq)).view(B, 1)
    i = torch.arange(Sq, device=dev).view(1, Sq)
    row = past + i                                        # [B,Sq]
    kept = (i < n) & (row < Smax)
    row = row.clamp(max=Smax - 1)
    slot = torch.where(kept, table.gather(1, row // P) * P + row % P, N * P)
    inv = torch.full((N * P + 1,), -1, dtype=torch.long, device=dev)
    inv.scatter_(0, slot.reshape(-1), torch.arange(B * Sq, device=dev))
    inv = inv[:N * P].view(N, P)
    hit = (inv >= 0).view(N, 1, P, 1)
    for pool, new in ((k_cache, k_new), (v_cache, v_new)):
        if pool.element_size() == 1:
            pool, new = pool.view(torch.uint8), new.view(torch.uint8)
        src = new.transpose(1, 2).reshape(B * Sq, Hk, D)
        pool.copy_(torch.where(hit, src[inv.clamp(min=0)].transpose(1, 2),
                               pool))


def kv_cache_append(k_cache: torch.Tensor, v_cache: torch.Tensor,
                    cache_seqlens: torch.Tensor, k_new: torch.Tensor,
                    v_new: torch.Tensor,
                    q_lens: Optional[torch.Tensor] = None,
                    block_table: Optional[torch.Tensor] = None,
                    k_scale: Optional[torch.Tensor] = None,
                    v_scale: Optional[torch.Tensor] = None) -> None:
    """The append step of ``flash_attention_extend`` alone, in place: rows
    i < n_b of k_new, v_new [B,Hk,Sq,D] go to logical cache rows past_b + i
    (through ``block_table`` when the caches are pools), rows at or past
    Smax are dropped, no other byte is written, the lengths are neither
    modified nor read on the host. Caches of k_new's dtype take the rows as
    they are; e4m3 caches (``torch.float8_e4m3fn``) need ``k_scale`` and
    ``v_scale`` (fp32 [Hk]) and take ``kv_quantize_reference`` of them, so a
    stored byte c of head hk stands for float(c) * scale[hk]. This is one way
    a prompt enters an e4m3 cache: prefill attention runs in bf16, its k and
    v are appended here, and ``flash_attention_decode`` then steps over e4m3
    (``flash_attention_extend`` with the scales is the other: it appends
    first and attends over the stored rows).
    bf16 rows on the GPU run the append kernels (csrc/attn_extend.hip,
    csrc/attn_decode_fp8.hip); anything else is composed in torch."""
    name = "kv_cache_append"
    if not isinstance(k_new, torch.Tensor) or k_new.dim() != 4:
        raise ValueError(f"{name}: need k_new and v_new [B,Hk,Sq,D]")
    _check_cached(name, k_new, k_cache, v_cache, cache_seqlens, k_new, v_new,
                  q_lens, block_table, k_scale, v_scale, fp8_ok=True)
    if k_new.shape[1] != k_cache.shape[1]:
        raise ValueError(f"{name}: k_new has {k_new.shape[1]} heads, the "
                         f"caches {k_cache.shape[1]}")
    _check_no_grad(name, k_cache, v_cache, k_new, v_new)
    if _cached_kernel_ok(k_new, k_cache, v_cache, cache_seqlens, q_lens,
                         block_table) and _row_ok(v_new):
        B, Hk, Sq, D = k_new.shape
        a = _cached_launch_args(k_new, k_cache, None, None, False,
                                block_table)
        if k_scale is not None:
            a.kw.update(k_scale=k_scale.data_ptr(),
                        v_scale=v_scale.data_ptr())
        if q_lens is not None:
            a.kw.update(q_lens=q_lens.data_ptr())
        _core().fa_kv_append(
            k_cache.data_ptr(), v_cache.data_ptr(), k_new.data_ptr(),
            v_new.data_ptr(), cache_seqlens.data_ptr(), B, Hk, Sq, a.Smax, D,
            _strides3(k_cache) + _strides3(v_cache),
            _strides3(k_new) + _strides3(v_new), a.device, a.stream, **a.kw)
        return
    if k_scale is not None:
        k_new = kv_quantize_reference(k_new, k_scale)
        v_new = kv_quantize_reference(v_new, v_scale)
    _append_composed(k_cache, v_cache, cache_seqlens, k_new, v_new, q_lens,
                     block_table)


def _fp8_extend_composed(q, k_cache, v_cache, cache_seqlens, k_new, v_new,
                         q_lens, causal, scale, return_lse, block_table,
                         k_scale, v_scale):
    """Extend over e4m3 caches off the kernel path, and its definition: the
    new rows quantised and written, the caches dequantised to q's dtype,
    then the composed route on those with no new rows and the lengths
    advanced on the device."""
    lens = cache_seqlens
    if k_new is not None:
        _append_composed(k_cache, v_cache, cache_seqlens,
                         kv_quantize_reference(k_new, k_scale),
                         kv_quantize_reference(v_new, v_scale), q_lens,
                         block_table)
        n = q.shape[2] if q_lens is None else q_lens.clamp(0, q.shape[2])
        lens = cache_seqlens.clamp(min=0) + n     # clamped to Smax below
    kd, vd = ((c.float() * s.view(1, -1, 1, 1)).to(q.dtype)
              for c, s in ((k_cache, k_scale), (v_cache, v_scale)))
    return _extend_composed(q, kd, vd, lens, None, None, q_lens, causal,
                            scale, return_lse, block_table)


def _fp8_decode_composed(q, k_cache, v_cache, cache_seqlens, k_new, v_new,
                         scale, return_lse, block_table, k_scale, v_scale):
    """Decode over e4m3 caches off the kernel path: a block of one row."""
    one = [None if t is None else t.unsqueeze(2) for t in (q, k_new, v_new)]
    res = _fp8_extend_composed(one[0], k_cache, v_cache, cache_seqlens,
                               one[1], one[2], None, True, scale, return_lse,
                               block_table, k_scale, v_scale)
    return (res[0][:, :, 0], res[1][:, :, 0]) if return_lse else res[:, :, 0]


def flash_attention_decode(q: torch.Tensor, k_cache: torch.Tensor,
                           v_cache: torch.Tensor,
                           cache_seqlens: torch.Tensor,
                           k_new: Optional[torch.Tensor] = None,
                           v_new: Optional[torch.Tensor] = None,
                           scale: float = None,
                           num_splits: Optional[int] = None,
                           return_lse: bool = False,
                           block_table: Optional[torch.Tensor] = None,
                           k_scale: Optional[torch.Tensor] = None,
                           v_scale: Optional[torch.Tensor] = None):
    """Attention of one new token per sequence over a KV cache. q: [B,H,D];
    k_cache, v_cache: [B,Hk,Smax,D] with H % Hk == 0 and any batch, head and
    row strides (a [B,Smax,Hk,D] cache goes in as its transposed view), query
    head h reading K/V head h // (H // Hk); cache_seqlens: int32 [B] on the
    same device, the number of keys of each sequence that count. Returns
    [B,H,D], with ``return_lse`` also the fp32 [B,H] natural-log logsumexp
    of the scaled scores. A sequence of length 0 gives a zero row and lse
    -inf.

    With k_new and v_new ([B,Hk,D], both or neither) the new token's rows
    are first written into cache row cache_seqlens[b], in place, and the
    attention covers cache_seqlens[b] + 1 keys. cache_seqlens itself is
    never modified, and never read on the host: the caller advances it.
    Lengths are clamped to [0, Smax]; appending to a full cache is the
    caller's error and gives unspecified values, but no access outside the
    tensors.

    bf16 on the GPU with D = 64 or 128 and H // Hk <= 32 runs the CDNA4
    split-KV kernels; num_splits None lets the shapes decide the number of
    key splits, an integer asks for that many (the kernels only). Anything
    else is composed as ``flash_attention_extend`` composes a block of one
    row. Forward only.

    With ``block_table`` (int32 [B,max_pages]) the cache is paged: k_cache
    and v_cache are pools [N,Hk,P,D] and Smax = max_pages * P, as
    ``flash_attention_extend`` describes.

    FP8 cache: k_cache and v_cache of dtype ``torch.float8_e4m3fn`` (slabs
    or pools, rows 16-B aligned: leading strides multiples of 16) with
    ``k_scale`` and ``v_scale``, fp32 [Hk] on the same device, positive: a
    stored byte c of K/V head hk stands for float(c) * scale[hk]. q, k_new,
    v_new and the output keep q's dtype; new rows are stored as
    ``kv_quantize_reference`` of them, and lse is the logsumexp of the
    scaled scores of the dequantised keys. The scales are read on the device
    only. bf16 q runs the kernels of csrc/attn_decode_fp8.hip, which read
    half the bytes and dequantise in registers (e4m3 -> bf16 is exact);
    anything else quantises and writes the new rows, dequantises the caches
    to q's dtype and composes as above. ``kv_cache_append`` fills such a
    cache from a bf16 prefill."""
    _check_cached("flash_attention_decode", q, k_cache, v_cache,
                  cache_seqlens, k_new, v_new, None, block_table, k_scale,
                  v_scale, fp8_ok=True)
    _check_no_grad("flash_attention_decode", q, k_cache, v_cache, k_new,
                   v_new)
    if num_splits is not None and int(num_splits) < 1:
        raise ValueError("flash_attention_decode: num_splits must be None or "
                         f">= 1, got {num_splits}")
    if _cached_kernel_ok(q, k_cache, v_cache, cache_seqlens, None,
                         block_table):
        s = scale if scale is not None else 1.0 / math.sqrt(q.shape[-1])
        return _launch_decode(q, k_cache, v_cache, cache_seqlens, k_new,
                              v_new, s, num_splits, return_lse, block_table,
                              k_scale, v_scale)
    if k_scale is not None:
        return _fp8_decode_composed(q, k_cache, v_cache, cache_seqlens, k_new,
                                    v_new, scale, return_lse, block_table,
                                    k_scale, v_scale)
    # a block of one row; [B,1,H,D] memory, so the [B,H,D] result is contiguous
    one = [None if t is None else t.unsqueeze(2) for t in (q, k_new, v_new)]
    res = _extend_composed(one[0], k_cache, v_cache, cache_seqlens, one[1],
                           one[2], None, True, scale, return_lse, block_table)
    return (res[0][:, :, 0], res[1][:, :, 0]) if return_lse else res[:, :, 0]


# ---------------------------------------------------------------------------
# Extend: a block of query rows per sequence against a KV cache
# ---------------------------------------------------------------------------
def fa_extend_supported(q: torch.Tensor, k_cache: torch.Tensor,
                        v_cache: torch.Tensor, cache_seqlens: torch.Tensor,
                        q_lens: Optional[torch.Tensor] = None,
                        block_table: Optional[torch.Tensor] = None,
                        k_scale: Optional[torch.Tensor] = None,
                        v_scale: Optional[torch.Tensor] = None) -> bool:
    """True where ``flash_attention_extend`` runs its kernels: bf16 q on the
    GPU, head_dim 64 or 128, at most 32 query heads per K/V head, rows
    contiguous and 16-B aligned, extension built; with ``block_table`` also
    a page size that is a power of two >= 16 and a contiguous table. The
    caches are bf16, or e4m3 with ``k_scale`` and ``v_scale``."""
    try:
        _check_cached("flash_attention_extend", q, k_cache, v_cache,
                      cache_seqlens, None, None, q_lens, block_table, k_scale,
                      v_scale, fp8_ok=True)
    except ValueError:
        return False
    return _cached_kernel_ok(q, k_cache, v_cache, cache_seqlens, q_lens,
                             block_table)


def _launch_extend(q, k_cache, v_cache, cache_seqlens, k_new, v_new, q_lens,
                   causal, scale, return_lse, num_splits=None,
                   block_table=None, k_scale=None, v_scale=None):
    """The kernel path, for arguments that passed ``_check_cached`` and
    ``_cached_kernel_ok``. With the scales: e4m3 caches and the kernels of
    csrc/attn_extend_fp8.hip."""
    core = _core()
    B, H, Sq, D = q.shape
    Hk = k_cache.shape[1]
    a = _cached_launch_args(q, k_cache, k_new, v_new, return_lse, block_table)
    Smax = a.Smax
    ns = core.fa_extend_splits(B, Hk, Sq, H // Hk, Smax,
                               0 if num_splits is None else int(num_splits),
                               a.device)
    if ns > 1:
        o_part = torch.empty((B, H, Sq, ns, D), dtype=torch.float32,
                             device=q.device)
        lse_part = torch.empty((B, H, Sq, ns), dtype=torch.float32,
                               device=q.device)
        a.kw.update(n_splits=ns, o_part=o_part.data_ptr(),
                    lse_part=lse_part.data_ptr())
    # [B,Sq,H,D] memory, as the forward's: transpose(1,2).view(B,Sq,C) is free
    out = torch.empty((B, Sq, H, D), dtype=q.dtype,
                      device=q.device).transpose(1, 2)
    if q_lens is not None:
        a.kw.update(q_lens=q_lens.data_ptr())
    strides = (_strides3(q) + _strides3(k_cache) + _strides3(v_cache)
               + _strides3(out) + a.new_strides)
    if k_scale is not None:
        core.fa_extend_fp8(q.data_ptr(), k_cache.data_ptr(),
                           v_cache.data_ptr(), cache_seqlens.data_ptr(),
                           k_scale.data_ptr(), v_scale.data_ptr(),
                           out.data_ptr(), B, H, Hk, Sq, Smax, D, strides,
                           scale, bool(causal), a.device, a.stream, **a.kw)
    else:
        core.fa_extend(q.data_ptr(), k_cache.data_ptr(), v_cache.data_ptr(),
                       cache_seqlens.data_ptr(), out.data_ptr(), B, H, Hk,
                       Sq, Smax, D, strides, scale, bool(causal), a.device,
                       a.stream, **a.kw)
    return (out, a.lse) if return_lse else out


def _paged_composed(q, k_pool, v_pool, block_table, cache_seqlens, k_new,
                    v_new, q_lens, causal, scale, return_lse):
    """The paged calls off the kernel path, and their definition: the
    table's pages gathered into [B,Hk,Smax,D] slabs (entries clamped to
    [0, N-1], as the kernels clamp them), ``_extend_composed`` on the slabs,
    then the appended rows alone written back into the pools; no host sync.
    The write-back is a masked rewrite through an inverse index: pool row
    (page, r) takes new row inv[page * P + r] where that is >= 0. A dropped
    row scatters its index into one dummy slot past the pool, so there is
    neither a ``nonzero`` nor a duplicate target among the real slots."""
    B, Sq = q.shape[0], q.shape[2]
    N, Hk, P, D = k_pool.shape
    max_pages = block_table.shape[1]
    Smax = max_pages * P
    table = block_table.clamp(0, N - 1).long()            # [B,max_pages]

    def slab(pool):     # [B,max_pages,Hk,P,D] -> [B,Hk,Smax,D]
        return pool[table].transpose(1, 2).reshape(B, Hk, Smax, D)

    k_slab, v_slab = slab(k_pool), slab(v_pool)
    res = _extend_composed(q, k_slab, v_slab, cache_seqlens, k_new, v_new,
                           q_lens, causal, scale, return_lse)
    if k_new is None:
        return res
    past = cache_seqlens.clamp(0, Smax).view(B, 1).long()
    n = (torch.full_like(cache_seqlens, Sq) if q_lens is None
         else q_lens.clamp(0, Sq)).view(B, 1)
    i = torch.arange(Sq, device=q.device).view(1, Sq)
    row = past + i                                        # [B,Sq]
    kept = (i < n) & (row < Smax)
    row = row.clamp(max=Smax - 1)
    slot = table.gather(1, row // P) * P + row % P
    slot = torch.where(kept, slot, N * P)
    inv = torch.full((N * P + 1,), -1, dtype=torch.long, device=q.device)
    inv.scatter_(0, slot.reshape(-1), torch.arange(B * Sq, device=q.device))
    inv = inv[:N * P].view(N, P)
    hit = (inv >= 0).view(N, 1, P, 1)
    for pool, new in ((k_pool, k_new), (v_pool, v_new)):
        src = new.transpose(1, 2).reshape(B * Sq, Hk, D)
        pool.copy_(torch.where(hit, src[inv.clamp(min=0)].transpose(1, 2),
                               pool))
    return res


def _extend_composed(q, k_cache, v_cache, cache_seqlens, k_new, v_new, q_lens,
                     causal, scale, return_lse, block_table=None):
    """The append as one gathered, masked rewrite of the caches in place (an
    index_put without duplicate targets), then SDPA under the explicit
    [B,1,Sq,Smax] mask; no host sync. With a block_table: ``_paged_composed``
    around this."""
    if block_table is not None:
        return _paged_composed(q, k_cache, v_cache, block_table,
                               cache_seqlens, k_new, v_new, q_lens, causal,
                               scale, return_lse)
    B, H, Sq, D = q.shape
    Hk, Smax = k_cache.shape[1], k_cache.shape[2]
    dev = q.device
    past = cache_seqlens.clamp(0, Smax).view(B, 1, 1, 1)
    n = (torch.full_like(cache_seqlens, Sq) if q_lens is None
         else q_lens.clamp(0, Sq)).view(B, 1, 1, 1)
    keys = torch.arange(Smax, device=dev).view(1, 1, 1, Smax)
    total = past
    if k_new is not None:
        # cache row j takes new row j - past_b where that is one of the n_b
        src = keys.view(1, 1, Smax, 1) - past
        hit = (src >= 0) & (src < n)
        at = src.clamp(0, Sq - 1).long().expand(B, Hk, Smax, D)
        k_cache.copy_(torch.where(hit, k_new.gather(2, at), k_cache))
        v_cache.copy_(torch.where(hit, v_new.gather(2, at), v_cache))
        total = (past + n).clamp(max=Smax)
    rows = torch.arange(Sq, device=dev).view(1, 1, Sq, 1)
    limit = total - n + rows if causal else (total - 1).expand(B, 1, Sq, 1)
    mask = (rows < n) & (keys <= limit)                   # [B,1,Sq,Smax]
    some = mask.any(-1, keepdim=True)                     # [B,1,Sq,1]
    # rows past a sequence's length may hold anything, NaN included
    live = (keys < total).view(B, 1, Smax, 1)
    kz = torch.where(live, k_cache, 0)
    vz = torch.where(live, v_cache, 0)
    qz = torch.where(rows < n, q, 0)
    gqa = {"enable_gqa": True} if Hk != H else {}
    # an all-masked row would be NaN: let it see all keys, zero it afterwards
    y = torch.nn.functional.scaled_dot_product_attention(
        qz, kz, vz, attn_mask=mask | ~some, scale=scale, **gqa)
    y = torch.where(some, y, 0)
    y = y.transpose(1, 2).contiguous().transpose(1, 2)    # [B,Sq,H,D] memory
    if not return_lse:
        return y
    s = scale if scale is not None else 1.0 / math.sqrt(D)
    G = H // Hk
    sc = torch.einsum("bhgqd,bhkd->bhgqk",
                      qz.float().view(B, Hk, G, Sq, D), kz.float()) * s
    sc = sc.masked_fill(~mask.unsqueeze(2), float("-inf"))
    return y, torch.logsumexp(sc, dim=-1).view(B, H, Sq)


def flash_attention_extend(q: torch.Tensor, k_cache: torch.Tensor,
                           v_cache: torch.Tensor,
                           cache_seqlens: torch.Tensor,
                           k_new: Optional[torch.Tensor] = None,
                           v_new: Optional[torch.Tensor] = None,
                           q_lens: Optional[torch.Tensor] = None,
                           causal: bool = True, scale: float = None,
                           return_lse: bool = False,
                           num_splits: Optional[int] = None,
                           block_table: Optional[torch.Tensor] = None,
                           k_scale: Optional[torch.Tensor] = None,
                           v_scale: Optional[torch.Tensor] = None):
    """Attention of a block of Sq query rows per sequence over a KV cache:
    chunked prefill, a further turn on a kept cache, a few drafted tokens,
    or (non-causal, no new rows) cross-attention. q: [B,H,Sq,D]; k_cache,
    v_cache: [B,Hk,Smax,D] with H % Hk == 0 and any batch, head and row
    strides (a [B,Smax,Hk,D] cache goes in as its transposed view), query
    head h reading K/V head h // (H // Hk); cache_seqlens: int32 [B] on the
    same device; q_lens: optional int32 [B], the number of leading query
    rows of each sequence that are real. Returns [B,H,Sq,D] in [B,Sq,H,D]
    memory, with ``return_lse`` also the fp32 [B,H,Sq] natural-log logsumexp
    of the scaled scores.

    past_b = clamp(cache_seqlens[b], 0, Smax); n_b = Sq, or clamp(q_lens[b],
    0, Sq). With k_new and v_new ([B,Hk,Sq,D], both or neither, strided views
    allowed) rows i < n_b are first written into cache rows past_b + i, in
    place; rows that would land at or past Smax are dropped (the caller's
    error: unspecified values, but no access outside the tensors), and
    total_b = min(past_b + n_b, Smax). Without them total_b = past_b: the
    caller has written and counted the chunk's keys already. With off_b =
    total_b - n_b, query row i < n_b sees keys 0 .. off_b + i when causal
    (bottom-right aligned) and keys < total_b when not. A row i >= n_b, or
    one that sees no key, gives a zero row and lse -inf. Neither length
    tensor is modified or read on the host, and no other cache row is
    written. With Sq == 1, new rows and no q_lens this is
    ``flash_attention_decode``.

    bf16 on the GPU with D = 64 or 128 and H // Hk <= 32 runs the CDNA4
    kernels of csrc/attn_extend.hip; num_splits None lets the shapes decide
    the number of key splits (one wherever Smax < 2048, and wherever the row
    tiles alone fill the chip); an integer asks for that many, and since a
    split is a multiple of 128 keys fewer may be used. Anything else is
    composed from a masked cache rewrite and torch SDPA under the explicit
    mask, which ignores num_splits. Forward only.

    With ``block_table`` the cache is paged. k_cache and v_cache are then
    page pools [N,Hk,P,D], N pages of P key rows, with any page, head and
    row strides (a [N,P,Hk,D] pool goes in as its transposed view), and
    block_table is int32 [B,max_pages] on the same device: logical key row
    j of sequence b is row j % P of page block_table[b, j // P]. Smax =
    max_pages * P takes the slab's capacity everywhere above: the clamps of
    cache_seqlens, the drop of appended rows, the split plan. New rows are
    written in place at logical rows past_b + i, through the table. The
    table promises, unchecked: entries 0 .. ceil(total_b / P) - 1 of row b
    name the sequence's pages; later entries may hold anything and are not
    read; two rows may name one page (a shared prefix) as long as no call
    appends into it. Every entry that is read is clamped to [0, N-1] first,
    so a malformed table gives unspecified values but no access outside the
    pools. The table is never read on the host: a captured graph stays
    valid when lengths and entries are refilled. The kernels take P a power
    of two >= 16 and a contiguous table, and give the output bits of the
    unpaged call on the gathered slab of the same Smax and split count;
    anything else gathers the pages, composes as above and writes the
    appended rows back.

    FP8 cache: k_cache and v_cache of dtype ``torch.float8_e4m3fn`` (slabs
    or pools, rows 16-B aligned: leading strides multiples of 16) with
    ``k_scale`` and ``v_scale``, fp32 [Hk] on the same device, positive: a
    stored byte c of K/V head hk stands for float(c) * scale[hk]. q, k_new,
    v_new and the output keep q's dtype, and lse is the logsumexp of the
    scaled scores of the dequantised keys. The scales are read on the device
    only. New rows are stored as ``kv_quantize_reference`` of them before
    the attention, which reads them back as stored: the chunk attends over
    its own quantised keys, so a prompt gives the same attention inputs
    however it is cut into chunks. That differs from a bf16 prefill followed
    by ``kv_cache_append``, where the prompt attends over the unquantised
    keys and only later tokens see the stored ones. bf16 q runs the kernels
    of csrc/attn_extend_fp8.hip, which read half the bytes, convert them
    once per workgroup on the way into LDS (e4m3 -> bf16 is exact) and fold
    the scales into the softmax scale and the final normalisation; anything
    else quantises and writes the new rows, dequantises the caches to q's
    dtype and composes as above."""
    _check_cached("flash_attention_extend", q, k_cache, v_cache,
                  cache_seqlens, k_new, v_new, q_lens, block_table, k_scale,
                  v_scale, fp8_ok=True)
    _check_no_grad("flash_attention_extend", q, k_cache, v_cache, k_new,
                   v_new)
    if num_splits is not None and int(num_splits) < 1:
        raise ValueError("flash_attention_extend: num_splits must be None or "
                         f">= 1, got {num_splits}")
    if _cached_kernel_ok(q, k_cache, v_cache, cache_seqlens, q_lens,
                         block_table):
        s = scale if scale is not None else 1.0 / math.sqrt(q.shape[-1])
        return _launch_extend(q, k_cache, v_cache, cache_seqlens, k_new,
                              v_new, q_lens, causal, s, return_lse,
                              num_splits, block_table, k_scale, v_scale)
    if k_scale is not None:
        return _fp8_extend_composed(q, k_cache, v_cache, cache_seqlens, k_new,
                                    v_new, q_lens, causal, scale, return_lse,
                                    block_table, k_scale, v_scale)
    return _extend_composed(q, k_cache, v_cache, cache_seqlens, k_new, v_new,
                            q_lens, causal, scale, return_lse, block_table)
