"""Top-1 MoE routing, dispatch and combine (csrc/moe.hip) with autograd.

``moe_route_top1`` turns gate logits into a :class:`Routing`: per token the
winning expert (argmax of the logits, lowest index on a tie), its softmax
probability in fp32, and a slot ``expert*capacity + pos`` where ``pos`` is the
token's stable rank among the tokens of that expert, or -1 when the expert is
over capacity; plus the inverse map ``src`` (token per slot, -1 when empty).
``moe_dispatch`` gathers token rows into the ``[E*capacity, d]`` buffer and
``moe_combine`` brings expert outputs back, scaled by the gate probability.

On the GPU, in fp32/fp16/bf16 with rows that are a multiple of 16 bytes, each
step is a hand-written kernel; anything else runs a plain-torch fallback with
the same semantics. Neither path indexes with a boolean mask, so neither
synchronises with the host and both can be captured into a graph.
"""

from __future__ import annotations

from typing import NamedTuple

import torch

from .fused import _DT, _core

__all__ = ["Routing", "moe_route_top1", "moe_dispatch", "moe_combine",
           "moe_fusable"]

_MAX_EXPERTS = 256
_TOK_BLOCK = 256  # tokens per routing workgroup (kTokBlock in moe.hip)


class Routing(NamedTuple):
    gate_p: torch.Tensor   # [T] fp32, differentiable w.r.t. the logits
    expert: torch.Tensor   # [T] int32
    slot: torch.Tensor     # [T] int32, -1 = dropped
    src: torch.Tensor      # [E*capacity] int32, -1 = empty
    capacity: int
    num_experts: int


def _kernels_on(t: torch.Tensor) -> bool:
    return bool(t.is_cuda and _core() and t.dtype in _DT
                and not torch.is_autocast_enabled())


def _route_fusable(logits: torch.Tensor, capacity: int) -> bool:
    if logits.dim() != 2 or not _kernels_on(logits):
        return False
    T, E = logits.shape
    return (T >= 1 and 1 <= E <= _MAX_EXPERTS and capacity >= 1
            and E * capacity < 2 ** 31 and T < 2 ** 31)


def _rows_fusable(x: torch.Tensor) -> bool:
    if x.dim() != 2 or not _kernels_on(x):
        return False
    T, d = x.shape
    return (T >= 1 and d >= 1 and (d * x.element_size()) % 16 == 0
            and x.is_contiguous() and x.data_ptr() % 16 == 0)


def moe_fusable(x: torch.Tensor, logits: torch.Tensor,
                capacity: int = 1) -> bool:
    """True when route, dispatch and combine all run the HIP kernels for
    tokens ``x [T, d]`` and gate logits ``logits [T, E]``."""
    return (x.dim() == 2 and logits.dim() == 2
            and x.shape[0] == logits.shape[0]
            and _rows_fusable(x) and _route_fusable(logits, capacity))


def _stream(t: torch.Tensor) -> int:
    return torch.cuda.current_stream(t.device).cuda_stream


def _rows(t: torch.Tensor) -> torch.Tensor:
    """Contiguous and 16-B aligned (e.g. an expanded grad is neither)."""
    t = t.contiguous()
    return t if t.data_ptr() % 16 == 0 else t.clone()


# ---------------------------------------------------------------- launches
# Outputs are caller-provided; the kernels write every byte of them.

def _launch_route(logits, capacity, gate_p, expert, slot, src):
    T, E = logits.shape
    nb = (T + _TOK_BLOCK - 1) // _TOK_BLOCK
    ws = torch.empty(2 * nb * E + E, dtype=torch.int32, device=logits.device)
    counts, offs, totals = ws[:nb * E], ws[nb * E:2 * nb * E], ws[2 * nb * E:]
    _core().moe_route(_DT[logits.dtype], logits.data_ptr(), gate_p.data_ptr(),
                      expert.data_ptr(), slot.data_ptr(), src.data_ptr(),
                      counts.data_ptr(), offs.data_ptr(), totals.data_ptr(),
                      T, E, capacity, _stream(logits))


def _launch_route_bwd(logits, gate_p, expert, slot, dgate, dlogits):
    T, E = logits.shape
    _core().moe_route_bwd(_DT[logits.dtype], logits.data_ptr(),
                          gate_p.data_ptr(), expert.data_ptr(),
                          slot.data_ptr(), dgate.data_ptr(),
                          dlogits.data_ptr(), T, E, _stream(logits))


def _launch_gather(inp, index, out, scale=None, scale_by_src=False):
    """out[r] = inp[index[r]] (* scale[r], or scale[index[r]] when
    ``scale_by_src``); zero rows where index[r] is -1."""
    _core().moe_gather(_DT[inp.dtype], inp.data_ptr(), inp.shape[0],
                       index.data_ptr(),
                       0 if scale is None else scale.data_ptr(),
                       scale_by_src, out.data_ptr(), out.shape[0],
                       inp.shape[1], _stream(inp))


def _launch_rowdot(a, b, index, out):
    """out[r] = dot(a[r], b[index[r]]) in fp32; 0 where index[r] is -1."""
    _core().moe_rowdot(_DT[a.dtype], a.data_ptr(), b.data_ptr(), b.shape[0],
                       index.data_ptr(), out.data_ptr(), a.shape[0],
                       a.shape[1], _stream(a))


# ---------------------------------------------------------------- autograd

class _RouteFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, logits, capacity):
        lc = logits.contiguous()
        T, E = lc.shape
        dev = lc.device
        gate_p = torch.empty(T, dtype=torch.float32, device=dev)
        expert = torch.empty(T, dtype=torch.int32, device=dev)
        slot = torch.empty(T, dtype=torch.int32, device=dev)
        src = torch.empty(E * capacity, dtype=torch.int32, device=dev)
        _launch_route(lc, capacity, gate_p, expert, slot, src)
        ctx.save_for_backward(lc, gate_p, expert, slot)
        ctx.mark_non_differentiable(expert, slot, src)
        return gate_p, expert, slot, src

    @staticmethod
    def backward(ctx, dgate, *_):
        lc, gate_p, expert, slot = ctx.saved_tensors
        dlogits = torch.empty_like(lc)
        _launch_route_bwd(lc, gate_p, expert, slot,
                          dgate.to(torch.float32).contiguous(), dlogits)
        return dlogits, None


class _DispatchFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, slot, src):
        ctx.save_for_backward(slot)
        out = torch.empty((src.shape[0], x.shape[1]), dtype=x.dtype,
                          device=x.device)
        _launch_gather(x, src, out)
        return out

    @staticmethod
    def backward(ctx, dout):
        (slot,) = ctx.saved_tensors
        dout = _rows(dout)
        dx = torch.empty((slot.shape[0], dout.shape[1]), dtype=dout.dtype,
                         device=dout.device)
        _launch_gather(dout, slot, dx)
        return dx, None, None


class _CombineFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, back, gate_p, slot, src):
        ctx.save_for_backward(back, gate_p, slot, src)
        y = torch.empty((slot.shape[0], back.shape[1]), dtype=back.dtype,
                        device=back.device)
        _launch_gather(back, slot, y, scale=gate_p)
        return y

    @staticmethod
    def backward(ctx, dy):
        back, gate_p, slot, src = ctx.saved_tensors
        dy = _rows(dy)
        dback = dgate = None
        if ctx.needs_input_grad[0]:
            dback = torch.empty_like(back)
            _launch_gather(dy, src, dback, scale=gate_p, scale_by_src=True)
        if ctx.needs_input_grad[1]:
            dgate = torch.empty_like(gate_p)
            _launch_rowdot(dy, back, slot, dgate)
        return dback, dgate, None, None


# ---------------------------------------------------------------- fallback

def _route_torch(logits: torch.Tensor, capacity: int):
    T, E = logits.shape
    lf = logits.float()
    expert = lf.argmax(dim=-1)  # first occurrence wins a tie
    onehot = torch.nn.functional.one_hot(expert, E)
    pos = (onehot.cumsum(dim=0) - 1).gather(1, expert[:, None]).squeeze(1)
    keep = pos < capacity
    slot = torch.where(keep, expert * capacity + pos, -1)
    # dropped tokens all land in one spare entry past the end
    n = E * capacity
    src = torch.full((n + 1,), -1, dtype=torch.int64, device=logits.device)
    src.scatter_(0, torch.where(keep, slot, n),
                 torch.arange(T, device=logits.device))
    gate_p = lf.softmax(dim=-1).gather(1, expert[:, None]).squeeze(1)
    # a dropped token's logits get no gradient, as in the kernel
    gate_p = torch.where(keep, gate_p, gate_p.detach())
    return (gate_p, expert.to(torch.int32), slot.to(torch.int32),
            src[:n].to(torch.int32))


def _gather_torch(inp, index, scale=None):
    """inp[index] with zero rows where index is -1, optionally times the
    fp32 per-row ``scale`` with a single rounding."""
    valid = (index >= 0)[:, None]
    rows = inp.index_select(0, index.clamp(min=0).long())
    if scale is not None:
        rows = (rows.float() * scale[:, None]).to(inp.dtype)
    return torch.where(valid, rows, torch.zeros((), dtype=inp.dtype,
                                                device=inp.device))


# ------------------------------------------------------------------ public

def moe_route_top1(logits: torch.Tensor, capacity: int) -> Routing:
    """Top-1 routing of ``logits [T, E]`` with ``capacity`` slots per
    expert."""
    if logits.dim() != 2:
        raise ValueError("moe_route_top1: logits must be [tokens, experts]")
    capacity = int(capacity)
    if capacity < 1:
        raise ValueError("moe_route_top1: capacity must be >= 1")
    if _route_fusable(logits, capacity):
        gate_p, expert, slot, src = _RouteFn.apply(logits, capacity)
    else:
        gate_p, expert, slot, src = _route_torch(logits, capacity)
    return Routing(gate_p, expert, slot, src, capacity, logits.shape[1])


def moe_dispatch(x: torch.Tensor, routing: Routing) -> torch.Tensor:
    """``out[s] = x[src[s]]``, zero rows for empty slots: ``[E*cap, d]``."""
    if x.dim() != 2 or x.shape[0] != routing.slot.shape[0]:
        raise ValueError("moe_dispatch: x must be [tokens, d]")
    if _rows_fusable(x) and routing.src.is_cuda:
        return _DispatchFn.apply(x, routing.slot, routing.src)
    return _gather_torch(x, routing.src)


def moe_combine(back: torch.Tensor, routing: Routing) -> torch.Tensor:
    """``y[t] = back[slot[t]] * gate_p[t]``, zero rows for dropped tokens:
    ``[T, d]``."""
    if back.dim() != 2 or back.shape[0] != routing.src.shape[0]:
        raise ValueError("moe_combine: back must be [E*capacity, d]")
    if _rows_fusable(back) and routing.slot.is_cuda:
        return _CombineFn.apply(back, routing.gate_p, routing.slot,
                                routing.src)
    return _gather_torch(back, routing.slot, scale=routing.gate_p)
