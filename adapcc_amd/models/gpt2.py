"""Minimal GPT-2 for the DDP training workload (reference:
models/gpt2/train_gpt2_ddp.py used transformers' GPT2DoubleHeadsModel on
PersonaChat; here a self-contained implementation sized identically to GPT-2
small, trained on synthetic tokens — no network access for datasets).

Attention runs through torch SDPA (rocm flash/mem-efficient backends);
everything else is plain PyTorch so autograd works with DDP buckets the
adapcc hook consumes. ``GPT2.generate`` samples greedily with a KV cache on
the decode attention kernels.
"""

from __future__ import annotations

import math
from dataclasses import dataclass

import torch
import torch.nn as nn
import torch.nn.functional as F

from ..ops.fused import FusedLayerNorm


@dataclass
class GPT2Config:
    vocab_size: int = 50257
    n_positions: int = 1024
    n_embd: int = 768
    n_layer: int = 12
    n_head: int = 12
    dropout: float = 0.0
    # dropout on each sublayer's output before it joins the residual stream
    # (transformers' resid_pdrop), fused with the add and the next LayerNorm
    resid_dropout: float = 0.0
    # K/V heads (grouped-query attention; 1: multi-query). None: n_head.
    # Must divide n_head; query head h reads K/V head h // (n_head //
    # n_kv_head), and c_attn is (n_head + 2*n_kv_head) * head_dim wide
    n_kv_head: int = None

    @classmethod
    def small(cls) -> "GPT2Config":
        return cls()

    @classmethod
    def tiny(cls) -> "GPT2Config":
        return cls(vocab_size=2048, n_positions=256, n_embd=128, n_layer=2,
                   n_head=4)

    @classmethod
    def medium(cls) -> "GPT2Config":
        return cls(n_embd=1024, n_layer=24, n_head=16)


class CausalSelfAttention(nn.Module):
    def __init__(self, cfg: GPT2Config):
        super().__init__()
        assert cfg.n_embd % cfg.n_head == 0
        self.n_head = cfg.n_head
        self.n_kv_head = (cfg.n_head if cfg.n_kv_head is None
                          else cfg.n_kv_head)
        assert self.n_kv_head >= 1 and cfg.n_head % self.n_kv_head == 0
        head_dim = cfg.n_embd // cfg.n_head
        self.c_attn = nn.Linear(
            cfg.n_embd, (cfg.n_head + 2 * self.n_kv_head) * head_dim)
        self.c_proj = nn.Linear(cfg.n_embd, cfg.n_embd)
        self.dropout = cfg.dropout

    def _forward_cached(self, x: torch.Tensor, cache: dict) -> torch.Tensor:
        """Generation (no dropout). cache: this layer's dict, ``Smax`` set;
        ``k``, ``v`` [B,Smax,Hk,D] are made on the first call, uninitialised:
        no row is read before it is written. ``lens`` (int32 [B] on the
        device, absent: zeros) counts the keys each sequence holds. x
        [B,T,C] is a block of T new positions, of which the first
        ``q_lens[b]`` (int32 [B], absent: all) are real: one
        ``flash_attention_extend`` call appends their k and v at row
        lens[b] and attends row i over lens[b] + i + 1 keys, straight off
        the projection. One token onto an existing cache with no ``q_lens``
        is the decode step, ``flash_attention_decode``. With ``table``
        (int32 [B,max_pages]) and ``page`` the cache is paged: ``k``, ``v``
        are pools [B * max_pages, page, Hk, D] and both calls get the table
        as ``block_table``. With ``dtype`` (``torch.float8_e4m3fn``) the
        cache is made of that dtype and both calls get ``k_scale`` and
        ``v_scale`` (fp32 [Hk]) from the dict."""
        from ..ops import attention

        H, Hk = self.n_head, self.n_kv_head
        qkv = self.c_attn(x)
        B, T, W = qkv.shape
        D = W // (H + 2 * Hk)
        q, k, v = qkv.split([H * D, Hk * D, Hk * D], dim=-1)
        table = cache.get("table")
        scales = {n: cache[n] for n in ("k_scale", "v_scale") if n in cache}
        if T == 1 and "k" in cache and cache.get("q_lens") is None:
            y = attention.flash_attention_decode(
                q.view(B, H, D), cache["k"].transpose(1, 2),
                cache["v"].transpose(1, 2), cache["lens"],
                k_new=k.view(B, Hk, D), v_new=v.view(B, Hk, D),
                block_table=table, **scales)
            return self.c_proj(y.view(B, 1, H * D))
        if "k" not in cache:
            shape = ((B, cache["Smax"]) if table is None
                     else (table.numel(), cache["page"]))
            dtype = cache.get("dtype", qkv.dtype)
            cache["k"] = qkv.new_empty(*shape, Hk, D, dtype=dtype)
            cache["v"] = qkv.new_empty(*shape, Hk, D, dtype=dtype)
        lens = cache.get("lens")
        if lens is None:
            lens = torch.zeros(B, dtype=torch.int32, device=x.device)
        y = attention.flash_attention_extend(
            q.view(B, T, H, D).transpose(1, 2), cache["k"].transpose(1, 2),
            cache["v"].transpose(1, 2), lens,
            k_new=k.view(B, T, Hk, D).transpose(1, 2),
            v_new=v.view(B, T, Hk, D).transpose(1, 2),
            q_lens=cache.get("q_lens"), block_table=table, **scales)
        return self.c_proj(y.transpose(1, 2).view(B, T, H * D))

    def forward(self, x: torch.Tensor,
                cu_seqlens: torch.Tensor = None,
                cache: dict = None) -> torch.Tensor:
        from ..ops import attention

        if cache is not None:
            return self._forward_cached(x, cache)
        p = self.dropout if self.training else 0.0
        if cu_seqlens is not None:
            # x is [1,total,C], documents back to back: attention stays
            # inside each document, on the [total,3C] view
            qkv = self.c_attn(x)
            y = attention.flash_attention_qkv_varlen(
                qkv.view(qkv.shape[1], qkv.shape[2]), self.n_head,
                cu_seqlens, dropout_p=p, n_kv_head=self.n_kv_head)
            return self.c_proj(y.view(1, y.shape[0], y.shape[1]))
        # packed [B,T,3C] in, [B,T,C] out: no split/transpose copies
        return self.c_proj(attention.flash_attention_qkv(
            self.c_attn(x), self.n_head,
            dropout_p=self.dropout if self.training else 0.0,
            n_kv_head=self.n_kv_head,
        ))


class MLP(nn.Module):
    def __init__(self, cfg: GPT2Config):
        super().__init__()
        self.c_fc = nn.Linear(cfg.n_embd, 4 * cfg.n_embd)
        self.c_proj = nn.Linear(4 * cfg.n_embd, cfg.n_embd)

    def forward(self, x: torch.Tensor) -> torch.Tensor:
        from ..ops.fused import fused_gelu, gelu_bias_grad_fusable

        w, b = self.c_fc.weight, self.c_fc.bias
        rows = x.numel() // max(x.shape[-1], 1)
        if gelu_bias_grad_fusable(x.device, x.dtype, rows, w.shape[0], b):
            # the GeLU backward sums the dx it writes into c_fc.bias' gradient
            # (no reduce pass over dx); the GEMM still adds the bias
            return self.c_proj(fused_gelu(F.linear(x, w, b.detach()), bias=b))
        return self.c_proj(fused_gelu(self.c_fc(x)))


class Block(nn.Module):
    def __init__(self, cfg: GPT2Config):
        super().__init__()
        self.ln_1 = FusedLayerNorm(cfg.n_embd)
        self.attn = CausalSelfAttention(cfg)
        self.ln_2 = FusedLayerNorm(cfg.n_embd)
        self.mlp = MLP(cfg)

    def forward(self, x: torch.Tensor,
                cu_seqlens: torch.Tensor = None,
                cache: dict = None) -> torch.Tensor:
        if cache is not None:
            x = x + self.attn(self.ln_1(x), cache=cache)
        elif cu_seqlens is None:
            x = x + self.attn(self.ln_1(x))
        else:
            x = x + self.attn(self.ln_1(x), cu_seqlens)
        x = x + self.mlp(self.ln_2(x))
        return x

    def forward_resid_dropout(self, x: torch.Tensor, y: torch.Tensor,
                              next_ln: nn.LayerNorm, p: float, site: int,
                              cu_seqlens: torch.Tensor = None):
        """The block with residual dropout p. x: the residual stream, y =
        ln_1(x), already computed where x was. Each sublayer output goes
        through one fused dropout + add + LayerNorm: the attention's with
        ln_2, the MLP's with next_ln (the next block's ln_1, or ln_f).
        Returns the new stream and next_ln of it; uses mask sites site and
        site + 1. cu_seqlens: as in forward."""
        from ..ops.fused import fused_dropout_add_layer_norm

        a = self.attn(y) if cu_seqlens is None else self.attn(y, cu_seqlens)
        x, y = fused_dropout_add_layer_norm(
            a, x, self.ln_2.weight, self.ln_2.bias, self.ln_2.eps,
            dropout_p=p, site=site)
        return fused_dropout_add_layer_norm(
            self.mlp(y), x, next_ln.weight, next_ln.bias, next_ln.eps,
            dropout_p=p, site=site + 1)


class GPT2(nn.Module):
    def __init__(self, cfg: GPT2Config):
        super().__init__()
        self.cfg = cfg
        self.wte = nn.Embedding(cfg.vocab_size, cfg.n_embd)
        self.wpe = nn.Embedding(cfg.n_positions, cfg.n_embd)
        self.drop = nn.Dropout(cfg.dropout)
        self.h = nn.ModuleList(Block(cfg) for _ in range(cfg.n_layer))
        self.ln_f = FusedLayerNorm(cfg.n_embd)
        self.lm_head = nn.Linear(cfg.n_embd, cfg.vocab_size, bias=False)
        self.lm_head.weight = self.wte.weight  # weight tying (as GPT-2)
        self.apply(self._init)
        for name, p in self.named_parameters():
            if name.endswith("c_proj.weight"):
                nn.init.normal_(p, mean=0.0,
                                std=0.02 / math.sqrt(2 * cfg.n_layer))

    @staticmethod
    def _init(m: nn.Module) -> None:
        if isinstance(m, nn.Linear):
            nn.init.normal_(m.weight, mean=0.0, std=0.02)
            if m.bias is not None:
                nn.init.zeros_(m.bias)
        elif isinstance(m, nn.Embedding):
            nn.init.normal_(m.weight, mean=0.0, std=0.02)

    def num_params(self, non_embedding: bool = True) -> int:
        n = sum(p.numel() for p in self.parameters())
        if non_embedding:
            n -= self.wpe.weight.numel()
        return n

    def _packed_positions(self, cu_seqlens: torch.Tensor,
                          total: int) -> torch.Tensor:
        """Position ids that restart at every document start, from
        cu_seqlens on the device (no host sync). Clamped into the position
        table, so a malformed cu_seqlens cannot index outside it."""
        rows = torch.arange(total, dtype=torch.int32,
                            device=cu_seqlens.device)
        ends = cu_seqlens[1:].contiguous()
        doc = torch.bucketize(rows, ends, right=True)
        doc = doc.clamp_(max=ends.numel() - 1)
        pos = rows - cu_seqlens[:-1][doc]
        return pos.clamp_(0, self.cfg.n_positions - 1).long()

    def forward(self, idx: torch.Tensor, targets: torch.Tensor = None,
                cu_seqlens: torch.Tensor = None):
        """cu_seqlens (int32 [n_docs + 1] on idx's device, non-decreasing
        from 0 to total): idx is [1,total] and holds documents back to back,
        each at most n_positions long; total may exceed n_positions.
        Position ids restart at each document and attention stays inside
        it. The caller masks the targets that cross a document boundary
        with the loss' ignore_index (-100)."""
        B, T = idx.shape
        if cu_seqlens is None:
            pos = torch.arange(T, device=idx.device)
            kw = {}
        else:
            if B != 1:
                raise ValueError("GPT2.forward: with cu_seqlens idx must be "
                                 f"[1, total], got {tuple(idx.shape)}")
            pos = self._packed_positions(cu_seqlens, T)
            kw = {"cu_seqlens": cu_seqlens}
        x = self.drop(self.wte(idx) + self.wpe(pos))
        if self.training and self.cfg.resid_dropout > 0.0:
            # every LayerNorm but the first runs fused with the add (and
            # dropout) in front of it: 2 * n_layer calls, one site each
            lns = [b.ln_1 for b in self.h[1:]] + [self.ln_f]
            y = self.h[0].ln_1(x)
            for i, block in enumerate(self.h):
                x, y = block.forward_resid_dropout(
                    x, y, lns[i], self.cfg.resid_dropout, site=2 * i, **kw)
            x = y
        else:
            for block in self.h:
                x = block(x, **kw)
            x = self.ln_f(x)
        logits = self.lm_head(x)
        loss = None
        if targets is not None:
            # Fused CE (csrc/ce.hip) on GPU: one read pass fwd, one
            # read+write pass bwd; no 6.6 GB log-softmax intermediate.
            from ..ops.fused import fused_cross_entropy

            loss = fused_cross_entropy(
                logits.view(-1, logits.size(-1)), targets.view(-1)
            )
        return logits, loss

    @torch.no_grad()
    def generate(self, idx: torch.Tensor, max_new_tokens: int,
                 return_logits: bool = False,
                 prompt_lens: torch.Tensor = None,
                 prefill_chunk: int = None,
                 kv_page_size: int = None,
                 kv_cache_dtype: torch.dtype = None,
                 kv_scales=None):
        """Greedy continuation of the prompts idx [B,T], T + max_new_tokens
        <= n_positions: returns [B, T + max_new_tokens], and with
        ``return_logits`` also the [B, max_new_tokens, vocab] logits each
        new token was the argmax of.

        ``prompt_lens`` (int32 [B] on idx's device, each in 1..T) makes the
        batch ragged: idx is right-padded with any valid token id, sequence
        b's prompt is its first prompt_lens[b] tokens, its first new token
        comes from the logits at position prompt_lens[b] - 1 and it
        continues from there. The return value is then the
        [B, max_new_tokens] new tokens alone (a ragged batch has no
        rectangular concatenation). ``prefill_chunk`` sends the prompt
        through the layers that many positions at a time.

        Each attention layer keeps its k and v in a cache
        [B, T + max_new_tokens, Hk, D]. The prompt's attention is
        ``flash_attention_extend``, which appends a chunk's k and v rows and
        attends in one pass at any length; every further token is one pass
        over [B,1,C] through ``flash_attention_decode``. Lengths and
        position ids stay on the device: neither the prefill nor the loop
        has a host sync. No dropout, whatever the module's mode.

        ``kv_page_size`` P pages the caches: each layer holds pools
        [B * max_pages, P, Hk, D], max_pages = ceil((T + max_new_tokens) /
        P), and all layers share one int32 block table [B, max_pages] that
        hands the pages out interleaved across the sequences (page j of
        sequence b is pool page j * B + b), which every prefill chunk and
        decode step passes as ``block_table``. The tokens are the unpaged
        run's.

        ``kv_cache_dtype=torch.float8_e4m3fn`` stores every layer's caches
        (or pools) as e4m3, half the bytes: rows are quantised as they are
        appended and every chunk and step attends over the stored codes, so
        chunking, raggedness and paging change nothing about what is
        attended. ``kv_scales`` is an optional pair (k, v) of fp32
        [n_layer, Hk] tensors on idx's device, a stored byte c of layer l,
        head hk standing for float(c) * scale[l, hk]; the default is ones.
        None keeps the caches in the model's dtype; any other dtype
        raises."""
        B, T = idx.shape
        total = T + max_new_tokens
        if T < 1 or max_new_tokens < 1 or total > self.cfg.n_positions:
            raise ValueError("GPT2.generate: need a prompt, max_new_tokens "
                             f">= 1 and T + max_new_tokens <= n_positions, "
                             f"got T {T}, max_new_tokens {max_new_tokens}, "
                             f"n_positions {self.cfg.n_positions}")
        chunk = T if prefill_chunk is None else int(prefill_chunk)
        if chunk < 1:
            raise ValueError("GPT2.generate: prefill_chunk must be >= 1, got "
                             f"{prefill_chunk}")
        ragged = prompt_lens is not None
        if ragged:
            if (prompt_lens.dtype != torch.int32 or prompt_lens.shape != (B,)
                    or prompt_lens.device != idx.device):
                raise ValueError("GPT2.generate: prompt_lens must be int32 "
                                 f"[{B}] on idx's device")
            plens = prompt_lens.clamp(1, T)
        else:
            plens = torch.full((B,), T, dtype=torch.int32, device=idx.device)
        batch = torch.arange(B, device=idx.device)
        caches = [{"Smax": total} for _ in self.h]
        if kv_cache_dtype is not None:
            if kv_cache_dtype != torch.float8_e4m3fn:
                raise ValueError("GPT2.generate: kv_cache_dtype must be None "
                                 "or torch.float8_e4m3fn, got "
                                 f"{kv_cache_dtype}")
            Hk = self.h[0].attn.n_kv_head
            if kv_scales is None:
                kv_scales = (torch.ones(len(self.h), Hk, device=idx.device),
                             ) * 2
            ks, vs = kv_scales
            for s in (ks, vs):
                if (s.dtype != torch.float32 or s.shape != (len(self.h), Hk)
                        or s.device != idx.device):
                    raise ValueError("GPT2.generate: kv_scales must be two "
                                     f"fp32 [{len(self.h)},{Hk}] tensors on "
                                     "idx's device")
            for i, cache in enumerate(caches):
                cache.update(dtype=kv_cache_dtype,
                             k_scale=ks[i].contiguous(),
                             v_scale=vs[i].contiguous())
        elif kv_scales is not None:
            raise ValueError("GPT2.generate: kv_scales goes with "
                             "kv_cache_dtype=torch.float8_e4m3fn")
        if kv_page_size is not None:
            P = int(kv_page_size)
            if P < 1:
                raise ValueError("GPT2.generate: kv_page_size must be >= 1, "
                                 f"got {kv_page_size}")
            max_pages = -(-total // P)
            table = (torch.arange(max_pages, device=idx.device).view(1, -1)
                     * B + batch.view(B, 1)).to(torch.int32)
            for cache in caches:
                cache.update(page=P, table=table)

        def hidden(x):
            for block, cache in zip(self.h, caches):
                x = block(x, cache=cache)
            return x

        def head(x):      # x [B,C]
            return self.lm_head(self.ln_f(x.unsqueeze(1)))[:, 0]

        # prefill: last[b] is the hidden state at position plens[b] - 1
        last = None
        for c0 in range(0, T, chunk):
            n = min(chunk, T - c0)
            for cache in caches:
                cache["lens"] = plens.clamp(max=c0)
                cache["q_lens"] = (plens - c0).clamp(0, n) if ragged else None
            pos = torch.arange(c0, c0 + n, device=idx.device)
            x = hidden(self.wte(idx[:, c0:c0 + n]) + self.wpe(pos))
            if not ragged:
                last = x[:, -1]
                continue
            at = plens - 1 - c0
            here = ((at >= 0) & (at < n)).view(B, 1)
            xa = x[batch, at.clamp(0, n - 1).long()]
            last = xa if last is None else torch.where(here, xa, last)
        logits = [head(last)]
        tokens = [logits[0].argmax(-1, keepdim=True)]
        lens = plens.clone()
        for cache in caches:
            cache["lens"] = lens
            cache["q_lens"] = None
        for _ in range(max_new_tokens - 1):
            x = self.wte(tokens[-1]) + self.wpe(lens.long()).unsqueeze(1)
            logits.append(head(hidden(x)[:, 0]))
            tokens.append(logits[-1].argmax(-1, keepdim=True))
            lens += 1      # every layer has appended this token's k and v
        out = torch.cat(tokens if ragged else [idx] + tokens, dim=1)
        if return_logits:
            return out, torch.stack(logits, dim=1)
        return out
