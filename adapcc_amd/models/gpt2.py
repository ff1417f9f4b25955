"""Minimal GPT-2 for the DDP training workload (reference:
models/gpt2/train_gpt2_ddp.py used transformers' GPT2DoubleHeadsModel on
PersonaChat; here a self-contained implementation sized identically to GPT-2
small, trained on synthetic tokens — no network access for datasets).

Attention runs through torch SDPA (rocm flash/mem-efficient backends);
everything else is plain PyTorch so autograd works with DDP buckets the
adapcc hook consumes.
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

    def forward(self, x: torch.Tensor,
                cu_seqlens: torch.Tensor = None) -> torch.Tensor:
        from ..ops import attention

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
                cu_seqlens: torch.Tensor = None) -> torch.Tensor:
        if cu_seqlens is None:
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
