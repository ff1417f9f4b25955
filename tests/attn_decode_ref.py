"""The decode attention tests' reference (not a test module)."""

import torch


def decode_reference(q, k_cache, v_cache, lens, scale=None):
    """softmax(q·K^T·scale over keys < len)·V in fp32 from the bf16 inputs;
    (out [B,H,D], lse [B,H]). A length 0 gives a zero row and lse -inf."""
    B, H, D = q.shape
    G = H // k_cache.shape[1]
    scale = D ** -0.5 if scale is None else scale
    out = torch.zeros(B, H, D)
    lse = torch.full((B, H), float("-inf"))
    for b, n in enumerate(int(x) for x in lens):
        if n == 0:
            continue
        k = k_cache[b, :, :n].float().cpu().repeat_interleave(G, 0)
        v = v_cache[b, :, :n].float().cpu().repeat_interleave(G, 0)
        s = torch.einsum("hd,hkd->hk", q[b].float().cpu(), k) * scale
        lse[b] = torch.logsumexp(s, -1)
        out[b] = torch.einsum("hk,hkd->hd", torch.softmax(s, -1), v)
    return out, lse
