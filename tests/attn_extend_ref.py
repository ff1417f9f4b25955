"""The extend attention tests' reference (not a test module)."""

import torch


def extend_reference(q, k_cache, v_cache, past, k_new=None, v_new=None,
                     q_lens=None, causal=True, scale=None):
    """``flash_attention_extend``'s contract in fp32 on the CPU from the
    given inputs, one sequence at a time. past, q_lens: lists of ints.
    Returns (out [B,H,Sq,D], lse [B,H,Sq], k_cache_after, v_cache_after);
    the caches keep their dtype."""
    B, H, Sq, D = q.shape
    Hk, Smax = k_cache.shape[1], k_cache.shape[2]
    G = H // Hk
    scale = D ** -0.5 if scale is None else scale
    kc, vc = k_cache.detach().cpu().clone(), v_cache.detach().cpu().clone()
    out = torch.zeros(B, H, Sq, D)
    lse = torch.full((B, H, Sq), float("-inf"))
    for b in range(B):
        p = min(max(int(past[b]), 0), Smax)
        n = Sq if q_lens is None else min(max(int(q_lens[b]), 0), Sq)
        total = p
        if k_new is not None:
            total = min(p + n, Smax)
            kc[b, :, p:total] = k_new[b, :, :total - p].cpu()
            vc[b, :, p:total] = v_new[b, :, :total - p].cpu()
        off = total - n
        for i in range(n):
            seen = min(off + i + 1, total) if causal else total
            if seen <= 0:
                continue
            k = kc[b, :, :seen].float().repeat_interleave(G, 0)
            v = vc[b, :, :seen].float().repeat_interleave(G, 0)
            s = torch.einsum("hd,hkd->hk", q[b, :, i].float().cpu(), k)
            s = s * scale
            lse[b, :, i] = torch.logsumexp(s, -1)
            out[b, :, i] = torch.einsum("hk,hkd->hd", torch.softmax(s, -1), v)
    return out, lse, kc, vc
