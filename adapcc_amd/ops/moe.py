"""Top-1 and top-2 MoE routing, dispatch and combine (csrc/moe.hip) with
autograd.

``moe_route_top1`` turns gate logits into a :class:`Routing`: per token the
winning expert (argmax of the logits, lowest index on a tie), its softmax
probability in fp32, and a slot ``expert*capacity + pos`` where ``pos`` is the
token's stable rank among the tokens of that expert, or -1 when the expert is
over capacity; plus the inverse map ``src`` (token per slot, -1 when empty).
``moe_dispatch`` gathers token rows into the ``[E*capacity, d]`` buffer and
``moe_combine`` brings expert outputs back, scaled by the gate probability.

``moe_route_topk`` (``k`` in {1, 2}) gives a :class:`RoutingTopK`:

* ``expert[t,0]`` is the argmax of the logits and ``expert[t,1]`` the argmax
  over the remaining experts, the lowest index winning a tie in both.
* ``gate[T,k]`` (fp32): for ``k=2, normalize=True`` the softmax over the two
  chosen logits (fastmoe NaiveGate / Mixtral), otherwise the full-softmax
  probabilities of the chosen experts. ``k=1`` reproduces ``moe_route_top1``
  bit for bit.
* GShard capacity priority: every first choice is placed before any second
  choice. ``pos`` of a first choice is its stable rank among the first
  choices of its expert; ``pos`` of a second choice is the number of first
  choices of that expert (kept or not) plus its stable rank among the second
  choices. ``slot[t,k] = expert*capacity + pos`` or -1; ``src`` and
  ``src_choice`` give the token and the choice held by each slot, or -1.
* ``load[E]`` counts first choices before capacity, and ``aux_loss`` is the
  Switch/GShard balance loss ``E * sum_e (load[e]/T) * mean_t p[t,e]``: 1 for
  a uniform gate, differentiable through the mean probabilities only.

``moe_dispatch`` and ``moe_combine`` take either routing; with two choices
``y[t] = sum_k gate[t,k] * back[slot[t,k]]`` over the kept ones, summed in
fp32 and rounded once.

On the GPU, in fp32/fp16/bf16 with rows that are a multiple of 16 bytes, each
step is a hand-written kernel; anything else runs a plain-torch fallback with
the same semantics. Neither path indexes with a boolean mask, so neither
synchronises with the host and both can be captured into a graph.
"""

from __future__ import annotations

from typing import NamedTuple

import torch

from .fused import _DT, _core

__all__ = ["Routing", "RoutingTopK", "moe_route_top1", "moe_route_topk",
           "moe_dispatch", "moe_combine", "moe_fusable"]

_MAX_EXPERTS = 256
_TOK_BLOCK = 256  # tokens per routing workgroup (kTokBlock in moe.hip)


class Routing(NamedTuple):
    gate_p: torch.Tensor   # [T] fp32, differentiable w.r.t. the logits
    expert: torch.Tensor   # [T] int32
    slot: torch.Tensor     # [T] int32, -1 = dropped
    src: torch.Tensor      # [E*capacity] int32, -1 = empty
    capacity: int
    num_experts: int


class RoutingTopK(NamedTuple):
    gate: torch.Tensor        # [T, k] fp32, differentiable w.r.t. the logits
    expert: torch.Tensor      # [T, k] int32
    slot: torch.Tensor        # [T, k] int32, -1 = dropped
    src: torch.Tensor         # [E*capacity] int32 token, -1 = empty
    src_choice: torch.Tensor  # [E*capacity] int32 choice, -1 = empty
    load: torch.Tensor        # [E] int32 first choices, before capacity
    aux_loss: torch.Tensor    # 0-dim fp32 balance loss
    capacity: int
    num_experts: int
    k: int


def _kernels_on(t: torch.Tensor) -> bool:
    return bool(t.is_cuda and _core() and t.dtype in _DT
                and not torch.is_autocast_enabled())


def _route_fusable(logits: torch.Tensor, capacity: int, k: int = 1) -> bool:
    if logits.dim() != 2 or not _kernels_on(logits):
        return False
    T, E = logits.shape
    return (T >= 1 and k in (1, 2) and k <= E <= _MAX_EXPERTS
            and capacity >= 1 and E * capacity < 2 ** 31
            and k * T < 2 ** 31)


def _rows_fusable(x: torch.Tensor) -> bool:
    if x.dim() != 2 or not _kernels_on(x):
        return False
    T, d = x.shape
    return (T >= 1 and d >= 1 and (d * x.element_size()) % 16 == 0
            and x.is_contiguous() and x.data_ptr() % 16 == 0)


def moe_fusable(x: torch.Tensor, logits: torch.Tensor,
                capacity: int = 1, k: int = 1) -> bool:
    """True when top-``k`` route, dispatch and combine all run the HIP
    kernels for tokens ``x [T, d]`` and gate logits ``logits [T, E]``."""
    return (x.dim() == 2 and logits.dim() == 2
            and x.shape[0] == logits.shape[0]
            and _rows_fusable(x) and _route_fusable(logits, capacity, k))


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


def _launch_route_topk(logits, k, capacity, normalize, gate, pmax, expert,
                       slot, src, src_choice, load, aux):
    """gate/expert/slot are [T, k], pmax (the first choice's full-softmax
    probability, kept for the backward pass) is [T]."""
    T, E = logits.shape
    nb = (T + _TOK_BLOCK - 1) // _TOK_BLOCK
    n = k * nb * E
    ws = torch.empty(2 * n + E, dtype=torch.int32, device=logits.device)
    psum = torch.empty(nb * E, dtype=torch.float32, device=logits.device)
    counts, offs, totals = ws[:n], ws[n:2 * n], ws[2 * n:]
    _core().moe_route_topk(_DT[logits.dtype], logits.data_ptr(), k, normalize,
                           gate.data_ptr(), pmax.data_ptr(),
                           expert.data_ptr(), slot.data_ptr(), src.data_ptr(),
                           src_choice.data_ptr(), load.data_ptr(),
                           aux.data_ptr(), counts.data_ptr(), offs.data_ptr(),
                           totals.data_ptr(), psum.data_ptr(), T, E, capacity,
                           _stream(logits))


def _launch_route_topk_bwd(logits, k, normalize, pmax, gate, expert, slot,
                           dgate, load, daux, dlogits):
    """``daux`` is a one-element fp32 tensor, or None when the balance loss
    received no gradient."""
    T, E = logits.shape
    _core().moe_route_topk_bwd(_DT[logits.dtype], logits.data_ptr(), k,
                               normalize, pmax.data_ptr(), gate.data_ptr(),
                               expert.data_ptr(), slot.data_ptr(),
                               dgate.data_ptr(), load.data_ptr(),
                               0 if daux is None else daux.data_ptr(),
                               dlogits.data_ptr(), T, E, _stream(logits))


def _launch_gather(inp, index, out, scale=None, scale_by_src=False,
                   choice=None):
    """out[r] = inp[index[r]] (* scale[r], or scale[index[r]] when
    ``scale_by_src``, or scale[index[r], choice[r]] with ``choice``); zero
    rows where index[r] is -1."""
    _core().moe_gather(_DT[inp.dtype], inp.data_ptr(), inp.shape[0],
                       index.data_ptr(),
                       0 if scale is None else scale.data_ptr(),
                       scale_by_src,
                       0 if choice is None else choice.data_ptr(),
                       1 if choice is None else scale.shape[1],
                       out.data_ptr(), out.shape[0], inp.shape[1],
                       _stream(inp))


def _launch_gather2(inp, index, out, scale=None):
    """out[r] = sum_c inp[index[r, c]] (* scale[r, c]) over the entries of
    ``index [rows, 2]`` that are not -1, summed in fp32 and rounded once."""
    _core().moe_gather2(_DT[inp.dtype], inp.data_ptr(), inp.shape[0],
                        index.data_ptr(),
                        0 if scale is None else scale.data_ptr(),
                        out.data_ptr(), out.shape[0], inp.shape[1],
                        _stream(inp))


def _launch_rowdot(a, b, index, out):
    """out[r] = dot(a[r], b[index[r]]) in fp32; 0 where index[r] is -1.
    ``index [rows, 2]`` gives ``out [rows, 2]``."""
    _core().moe_rowdot(_DT[a.dtype], a.data_ptr(), b.data_ptr(), b.shape[0],
                       index.data_ptr(), out.data_ptr(), index.numel(),
                       a.shape[1], index.dim() - 1, _stream(a))


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


class _RouteTopKFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, logits, k, capacity, normalize):
        lc = logits.contiguous()
        T, E = lc.shape
        dev = lc.device
        gate = torch.empty((T, k), dtype=torch.float32, device=dev)
        pmax = torch.empty(T, dtype=torch.float32, device=dev)
        expert = torch.empty((T, k), dtype=torch.int32, device=dev)
        slot = torch.empty((T, k), dtype=torch.int32, device=dev)
        src = torch.empty(E * capacity, dtype=torch.int32, device=dev)
        src_choice = torch.empty(E * capacity, dtype=torch.int32, device=dev)
        load = torch.empty(E, dtype=torch.int32, device=dev)
        aux = torch.empty((), dtype=torch.float32, device=dev)
        _launch_route_topk(lc, k, capacity, normalize, gate, pmax, expert,
                           slot, src, src_choice, load, aux)
        ctx.save_for_backward(lc, pmax, gate, expert, slot, load)
        ctx.k, ctx.normalize = k, normalize
        ctx.mark_non_differentiable(expert, slot, src, src_choice, load)
        # an output nobody differentiates arrives as None, not as zeros
        ctx.set_materialize_grads(False)
        return gate, expert, slot, src, src_choice, load, aux

    @staticmethod
    def backward(ctx, dgate, d1, d2, d3, d4, d5, daux):
        lc, pmax, gate, expert, slot, load = ctx.saved_tensors
        if dgate is None:
            dgate = torch.zeros_like(gate)
        if daux is not None:
            daux = daux.to(torch.float32).reshape(1).contiguous()
        dlogits = torch.empty_like(lc)
        _launch_route_topk_bwd(lc, ctx.k, ctx.normalize, pmax, gate, expert,
                               slot, dgate.to(torch.float32).contiguous(),
                               load, daux, dlogits)
        return dlogits, None, None, None


class _Dispatch2Fn(torch.autograd.Function):
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
        _launch_gather2(dout, slot, dx)
        return dx, None, None


class _Combine2Fn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, back, gate, slot, src, src_choice):
        gate = gate.contiguous()
        ctx.save_for_backward(back, gate, slot, src, src_choice)
        y = torch.empty((slot.shape[0], back.shape[1]), dtype=back.dtype,
                        device=back.device)
        _launch_gather2(back, slot, y, scale=gate)
        return y

    @staticmethod
    def backward(ctx, dy):
        back, gate, slot, src, src_choice = ctx.saved_tensors
        dy = _rows(dy)
        dback = dgate = None
        if ctx.needs_input_grad[0]:
            dback = torch.empty_like(back)
            _launch_gather(dy, src, dback, scale=gate, scale_by_src=True,
                           choice=src_choice)
        if ctx.needs_input_grad[1]:
            dgate = torch.empty_like(gate)
            _launch_rowdot(dy, back, slot, dgate)
        return dback, dgate, None, None, None


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


def _route_topk_torch(logits: torch.Tensor, k: int, capacity: int,
                      normalize: bool):
    T, E = logits.shape
    dev = logits.device
    lf = logits.float()
    probs = lf.softmax(dim=-1)
    e0 = lf.argmax(dim=-1)  # first occurrence wins a tie
    if k == 2:
        first = torch.nn.functional.one_hot(e0, E).bool()
        e1 = lf.masked_fill(first, float("-inf")).argmax(dim=-1)
        expert = torch.stack([e0, e1], dim=1)
    else:
        expert = e0[:, None]
    # rank the k*T (choice, token) pairs choice-major: every first choice is
    # placed before any second choice
    flat = expert.t().reshape(-1)
    onehot = torch.nn.functional.one_hot(flat, E)
    pos = (onehot.cumsum(dim=0) - 1).gather(1, flat[:, None]).squeeze(1)
    keep = pos < capacity
    slot_flat = torch.where(keep, flat * capacity + pos, -1)
    # dropped pairs all land in one spare entry past the end
    n = E * capacity
    target = torch.where(keep, slot_flat, n)
    src = torch.full((n + 1,), -1, dtype=torch.int64, device=dev)
    src.scatter_(0, target, torch.arange(T, device=dev).repeat(k))
    src_choice = torch.full((n + 1,), -1, dtype=torch.int64, device=dev)
    src_choice.scatter_(0, target,
                        torch.arange(k, device=dev).repeat_interleave(T))
    slot = slot_flat.view(k, T).t()
    if k == 2 and normalize:
        x = lf.gather(1, expert)
        r = (x[:, 1] - x[:, 0]).exp()
        g0 = 1.0 / (1.0 + r)
        gate = torch.stack([g0, r * g0], dim=1)
    else:
        gate = probs.gather(1, expert)
    # a dropped choice's gate gets no gradient, as in the kernel
    gate = torch.where(slot >= 0, gate, gate.detach())
    load = onehot[:T].sum(dim=0)
    aux = E * ((load.float() / T) * probs.mean(dim=0)).sum()
    return (gate, expert.to(torch.int32), slot.to(torch.int32).contiguous(),
            src[:n].to(torch.int32), src_choice[:n].to(torch.int32),
            load.to(torch.int32), aux)


def _combine_topk_torch(back, gate, slot):
    """sum_k gate[t,k] * back[slot[t,k]] over kept choices: fp32 sum, one
    rounding, exact zero rows where every choice is dropped."""
    T, k = slot.shape
    rows = back.index_select(0, slot.clamp(min=0).reshape(-1).long())
    rows = rows.view(T, k, -1).float() * gate[:, :, None]
    rows = torch.where((slot >= 0)[:, :, None], rows,
                       torch.zeros((), device=back.device))
    return rows.sum(dim=1).to(back.dtype)


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


def moe_route_topk(logits: torch.Tensor, k: int, capacity: int,
                   normalize: bool = True, *,
                   use_kernels: bool = True) -> RoutingTopK:
    """Top-``k`` routing (``k`` in {1, 2}) of ``logits [T, E]`` with
    ``capacity`` slots per expert, GShard priority and the Switch/GShard
    load-balancing loss; see the module docstring. ``use_kernels=False``
    takes the plain-torch path even where the kernels apply."""
    if logits.dim() != 2:
        raise ValueError("moe_route_topk: logits must be [tokens, experts]")
    if k not in (1, 2):
        raise ValueError("moe_route_topk: k must be 1 or 2")
    if logits.shape[1] < k:
        raise ValueError("moe_route_topk: need at least k experts")
    capacity = int(capacity)
    if capacity < 1:
        raise ValueError("moe_route_topk: capacity must be >= 1")
    normalize = bool(normalize)
    if use_kernels and _route_fusable(logits, capacity, k):
        out = _RouteTopKFn.apply(logits, k, capacity, normalize)
    else:
        out = _route_topk_torch(logits, k, capacity, normalize)
    return RoutingTopK(*out, capacity, logits.shape[1], k)


def moe_dispatch(x: torch.Tensor, routing, *,
                 use_kernels: bool = True) -> torch.Tensor:
    """``out[s] = x[src[s]]``, zero rows for empty slots: ``[E*cap, d]``.
    ``routing`` is a :class:`Routing` or a :class:`RoutingTopK`."""
    if x.dim() != 2 or x.shape[0] != routing.slot.shape[0]:
        raise ValueError("moe_dispatch: x must be [tokens, d]")
    if use_kernels and _rows_fusable(x) and routing.src.is_cuda:
        if isinstance(routing, RoutingTopK) and routing.k == 2:
            return _Dispatch2Fn.apply(x, routing.slot, routing.src)
        return _DispatchFn.apply(x, routing.slot.reshape(-1), routing.src)
    return _gather_torch(x, routing.src)


def moe_combine(back: torch.Tensor, routing, *,
                use_kernels: bool = True) -> torch.Tensor:
    """``y[t] = back[slot[t]] * gate_p[t]`` for a :class:`Routing`,
    ``y[t] = sum_k gate[t,k] * back[slot[t,k]]`` (fp32 sum, one rounding) for
    a :class:`RoutingTopK`; dropped choices are skipped and a token with
    nothing kept gets a zero row: ``[T, d]``."""
    if back.dim() != 2 or back.shape[0] != routing.src.shape[0]:
        raise ValueError("moe_combine: back must be [E*capacity, d]")
    fused = use_kernels and _rows_fusable(back) and routing.slot.is_cuda
    if not isinstance(routing, RoutingTopK):
        if fused:
            return _CombineFn.apply(back, routing.gate_p, routing.slot,
                                    routing.src)
        return _gather_torch(back, routing.slot, scale=routing.gate_p)
    if not fused:
        return _combine_topk_torch(back, routing.gate, routing.slot)
    if routing.k == 2:
        return _Combine2Fn.apply(back, routing.gate, routing.slot,
                                 routing.src, routing.src_choice)
    return _CombineFn.apply(back, routing.gate.reshape(-1),
                            routing.slot.reshape(-1), routing.src)
