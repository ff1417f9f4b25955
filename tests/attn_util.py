"""Shared by the flash-attention GPU tests: the fp32 reference, the
[B,T,C] <-> [B,H,T,C/H] head views and the recorder of kernel launches."""

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


def record_launches(monkeypatch, extra=None):
    """Wraps the launch helpers of adapcc_amd.ops.attention for the test and
    returns the list that collects one (direction, causal, dropout_p,
    varlen) per launch, varlen saying whether a tile map was passed.
    ``extra(*args)``, given the helper's positional arguments, returns a
    tuple that is appended to the entry."""
    from adapcc_amd.ops import attention

    calls = []

    def wrap(direction, real):
        def launch(*a, **kw):
            calls.append((direction, kw.get("causal", True),
                          kw.get("dropout_p", 0.0),
                          kw.get("tmap") is not None)
                         + (extra(*a) if extra else ()))
            return real(*a, **kw)
        return launch

    monkeypatch.setattr(attention, "_launch_fwd",
                        wrap("fwd", attention._launch_fwd))
    monkeypatch.setattr(attention, "_launch_bwd",
                        wrap("bwd", attention._launch_bwd))
    return calls
