"""Shared by the flash-attention GPU tests: the fp32 reference and the
[B,T,C] <-> [B,H,T,C/H] head views."""

import torch


def ref_attention_f32(q, k, v, scale, causal):
    """fp32 attention reference (explicit, no SDPA)."""
    qf, kf, vf = q.float(), k.float(), v.float()
    s = torch.matmul(qf, kf.transpose(-1, -2)) * scale
    if causal:
        S = q.shape[-2]
        mask = torch.ones(S, S, dtype=torch.bool, device=q.device).triu(1)
        s = s.masked_fill(mask, float("-inf"))
    p = torch.softmax(s, dim=-1)
    return torch.matmul(p, vf)


def heads(t, H):
    B, T, C = t.shape
    return t.view(B, T, H, C // H).transpose(1, 2)


def unheads(t):
    B, H, T, d = t.shape
    return t.transpose(1, 2).reshape(B, T, H * d)
