"""Fused CDNA4 op wrappers (autograd integration for the hand-written HIP
kernels in csrc/lnorm.hip, csrc/ce.hip and csrc/gelu.hip).

``fused_dropout_add_layer_norm`` is the pre-norm residual step
``x_new = residual + dropout(h); y = LayerNorm(x_new)`` in one kernel each
way. Its mask is the attention kernels' keep(seed, site, row, col)
(csrc/attn_drop.h) over the flattened rows, regenerated in the backward and
never stored; the seed is attention's too: one int64 on the device, drawn
from torch's generator per call or passed as ``dropout_seed``.
``dropout_add_keep_mask_reference`` is that mask in torch integer ops.

Three fusions drop passes over memory that the training step does not need;
each has a module-level switch, so one process can run both paths:

``FUSE_CE_GRAD``: when the logits need a gradient, the cross-entropy forward
keeps each row in registers and writes loss, lse and dlogits (for an
upstream gradient of 1) after one read (csrc/ce.hip, ``ce_fwd_grad``). The
backward launches ``ce_bwd`` with the upstream gradient on the device: at
exactly 1.0 it returns at once and the saved dlogits are the result, any
other value recomputes them as before. Bits are those of the two-kernel path.

``FUSE_GELU_BIAS_GRAD``: ``fused_gelu(x, bias=b)`` takes the gradient of the
bias that the linear in front added from the GeLU backward, which sums the dx
it writes down the columns (csrc/gelu.hip, ``gelu_bwd_bias``): torch's reduce
kernel over dx goes. ``gelu_bias_grad_fusable`` says when; the caller then
hands the linear ``b.detach()``.

``FUSE_COLSUM_FOLD``: the per-wave dgamma/dbeta partials of the LayerNorm
backwards, and the GeLU's, are summed by one ``colsum_fold`` launch
(csrc/colsum.hip) that writes the parameter dtype, where torch took a reduce
and a cast kernel per array."""

from __future__ import annotations

from typing import Optional

import torch
import torch.nn as nn

_CORE = None
_DT = {}

# see the module docstring; tests flip these to compare the paths
FUSE_CE_GRAD = True
FUSE_GELU_BIAS_GRAD = True
FUSE_COLSUM_FOLD = True


def _core():
    global _CORE
    if _CORE is None:
        try:
            from adapcc_amd import _core as c

            _CORE = c
            _DT.update({torch.float32: c.DTYPE_F32, torch.float16: c.DTYPE_F16,
                        torch.bfloat16: c.DTYPE_BF16})
        except ImportError:
            _CORE = False
    return _CORE


def ln_fusable(cols: int, dtype: torch.dtype) -> bool:
    c = _core()
    if not c or dtype not in _DT:
        return False
    return bool(c.ln_supported(cols, _DT[dtype]))


def _fold_partials(parts, nslots: int, cols: int, dtype: torch.dtype):
    """Column sums of up to three [nslots * cols] fp32 partial arrays, each
    as a [cols] tensor of dtype: one colsum_fold launch, or torch's reduce
    and cast per array with the switch off."""
    if not (FUSE_COLSUM_FOLD and cols % 4 == 0 and dtype in _DT):
        return [p.view(nslots, cols).sum(0).to(dtype) for p in parts]
    dev = parts[0].device
    outs = [torch.empty(cols, dtype=dtype, device=dev) for _ in parts]
    pad = [0] * (3 - len(parts))
    _core().colsum_fold(
        _DT[dtype], *([p.data_ptr() for p in parts] + pad),
        *([o.data_ptr() for o in outs] + pad), nslots, cols,
        torch.cuda.current_stream(dev).cuda_stream)
    return outs


class _FusedLayerNormFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x: torch.Tensor, weight: torch.Tensor,
                bias: torch.Tensor, eps: float) -> torch.Tensor:
        c = _core()
        xc = x.contiguous()
        cols = xc.shape[-1]
        rows = xc.numel() // cols
        y = torch.empty_like(xc)
        mean = torch.empty(rows, dtype=torch.float32, device=xc.device)
        rstd = torch.empty_like(mean)
        stream = torch.cuda.current_stream(xc.device).cuda_stream
        c.ln_fwd(_DT[xc.dtype], xc.data_ptr(), weight.data_ptr(),
                 bias.data_ptr(), y.data_ptr(), mean.data_ptr(),
                 rstd.data_ptr(), rows, cols, eps, stream)
        ctx.save_for_backward(xc, weight, mean, rstd)
        return y

    @staticmethod
    def backward(ctx, dy: torch.Tensor):
        c = _core()
        x, weight, mean, rstd = ctx.saved_tensors
        cols = x.shape[-1]
        rows = x.numel() // cols
        dyc = dy.contiguous()
        dx = torch.empty_like(x)
        nblocks = max(1, min(1024, (rows + 3) // 4))
        nslots = nblocks * 4  # one partial per wave
        ws = torch.empty(2 * nslots * cols, dtype=torch.float32,
                         device=x.device)
        wsg = ws[: nslots * cols]
        wsb = ws[nslots * cols:]
        stream = torch.cuda.current_stream(x.device).cuda_stream
        c.ln_bwd(_DT[x.dtype], dyc.data_ptr(), x.data_ptr(),
                 weight.data_ptr(), mean.data_ptr(), rstd.data_ptr(),
                 dx.data_ptr(), wsg.data_ptr(), wsb.data_ptr(),
                 rows, cols, nblocks, stream)
        dgamma, dbeta = _fold_partials([wsg, wsb], nslots, cols, weight.dtype)
        return dx, dgamma, dbeta, None


class _FusedCrossEntropyFn(torch.autograd.Function):
    """Mean cross-entropy over rows without materializing log-softmax
    (csrc/ce.hip). Saves ~2x the logits tensor of HBM traffic plus the
    6.6 GB log-softmax intermediate on the GPT-2 flagship path.

    First-order only: the backward launches kernels on raw pointers, and on
    the fused path the gradient it returns is a tensor saved by the forward,
    which a recompute overwrites in place. Double backward through this
    Function is not supported."""

    @staticmethod
    def forward(ctx, logits: torch.Tensor, targets: torch.Tensor,
                ignore_index: int, want_grad: bool = False) -> torch.Tensor:
        c = _core()
        lc = logits.contiguous()
        rows, cols = lc.shape
        tc = targets.contiguous().to(torch.int64)
        loss = torch.empty(rows, dtype=torch.float32, device=lc.device)
        lse = torch.empty_like(loss)
        stream = torch.cuda.current_stream(lc.device).cuda_stream
        n_valid = (tc != ignore_index).sum().to(torch.float32).clamp(min=1)
        ctx.ignore_index = ignore_index
        # training: dlogits leave the forward's one read of the logits
        # (want_grad: a backward will come; the caller knows, in here grad
        # mode is off and needs_input_grad ignores no_grad)
        ctx.fused = bool(FUSE_CE_GRAD and want_grad
                         and cols <= c.ce_fused_max_cols(_DT[lc.dtype]))
        if ctx.fused:
            # the backward's gscale for an upstream gradient of 1
            g0 = (torch.ones_like(n_valid) / n_valid).reshape(1)
            dlogits = torch.empty_like(lc)
            c.ce_fwd_grad(_DT[lc.dtype], lc.data_ptr(), tc.data_ptr(),
                          g0.data_ptr(), loss.data_ptr(), lse.data_ptr(),
                          dlogits.data_ptr(), rows, cols, ignore_index, stream)
            ctx.save_for_backward(lc, tc, lse, n_valid, dlogits)
            ctx.dlogits_fresh = True
        else:
            c.ce_fwd(_DT[lc.dtype], lc.data_ptr(), tc.data_ptr(),
                     loss.data_ptr(), lse.data_ptr(), rows, cols,
                     ignore_index, stream)
            ctx.save_for_backward(lc, tc, lse, n_valid)
        return loss.sum() / n_valid

    @staticmethod
    def backward(ctx, grad_out: torch.Tensor):
        c = _core()
        logits, targets, lse, n_valid, *saved = ctx.saved_tensors
        rows, cols = logits.shape
        up = grad_out.to(torch.float32).reshape(1).contiguous()
        gscale = up / n_valid
        if ctx.fused and ctx.dlogits_fresh:
            # the kernel reads the upstream gradient itself (no host sync):
            # at 1.0 the saved dlogits stand, else it recomputes over them.
            # Only once: what this returns may end up as a leaf's .grad.
            ctx.dlogits_fresh = False
            dlogits, up_ptr = saved[0], up.data_ptr()
        else:
            dlogits, up_ptr = torch.empty_like(logits), 0
        stream = torch.cuda.current_stream(logits.device).cuda_stream
        c.ce_bwd(_DT[logits.dtype], logits.data_ptr(), targets.data_ptr(),
                 lse.data_ptr(), gscale.data_ptr(), up_ptr,
                 dlogits.data_ptr(), rows, cols, ctx.ignore_index, stream)
        return dlogits, None, None, None


def fused_cross_entropy(logits: torch.Tensor, targets: torch.Tensor,
                        ignore_index: int = -100) -> torch.Tensor:
    """F.cross_entropy(reduction='mean') drop-in for 2D logits; runs the
    fused HIP kernel on GPU, falls back to torch elsewhere."""
    if (
        logits.is_cuda
        and logits.dim() == 2
        and logits.shape[0] > 0
        and logits.shape[1] > 0
        and _core()
        and logits.dtype in _DT
        and not torch.is_autocast_enabled()
    ):
        return _FusedCrossEntropyFn.apply(
            logits, targets, ignore_index,
            torch.is_grad_enabled() and logits.requires_grad)
    return torch.nn.functional.cross_entropy(
        logits.float(), targets, ignore_index=ignore_index)


class _FusedGeluFn(torch.autograd.Function):
    """tanh-GeLU with a one-exp tanh (csrc/gelu.hip). Measured ~10%
    faster than torch's tanh-GeLU at the flagship MLP shape (both are
    near memory-bound; the win is the shorter VALU chain)."""

    @staticmethod
    def forward(ctx, x: torch.Tensor) -> torch.Tensor:
        c = _core()
        xc = x.contiguous()
        y = torch.empty_like(xc)
        stream = torch.cuda.current_stream(xc.device).cuda_stream
        c.gelu_fwd(_DT[xc.dtype], xc.data_ptr(), y.data_ptr(), xc.numel(),
                   stream)
        ctx.save_for_backward(xc)
        return y

    @staticmethod
    def backward(ctx, dy: torch.Tensor):
        c = _core()
        (x,) = ctx.saved_tensors
        dyc = dy.contiguous()
        dx = torch.empty_like(x)
        stream = torch.cuda.current_stream(x.device).cuda_stream
        c.gelu_bwd(_DT[x.dtype], x.data_ptr(), dyc.data_ptr(), dx.data_ptr(),
                   x.numel(), stream)
        return dx


class _FusedGeluBiasFn(torch.autograd.Function):
    """_FusedGeluFn over [..., cols] whose backward also returns the column
    sum of dx as the gradient of ``bias``: the bias a linear added to x,
    handed to that linear detached."""

    @staticmethod
    def forward(ctx, x: torch.Tensor, bias: torch.Tensor) -> torch.Tensor:
        c = _core()
        xc = x.contiguous()
        y = torch.empty_like(xc)
        stream = torch.cuda.current_stream(xc.device).cuda_stream
        c.gelu_fwd(_DT[xc.dtype], xc.data_ptr(), y.data_ptr(), xc.numel(),
                   stream)
        ctx.save_for_backward(xc)
        ctx.bias_dtype = bias.dtype
        return y

    @staticmethod
    def backward(ctx, dy: torch.Tensor):
        c = _core()
        (x,) = ctx.saved_tensors
        cols = x.shape[-1]
        rows = x.numel() // cols
        dyc = dy.contiguous()
        dx = torch.empty_like(x)
        # one partial row per block: 1024 blocks fill the chip, and the
        # workspace stays a small fraction of dx
        nblocks = max(1, min(1024, (rows + 3) // 4))
        ws = torch.empty(nblocks * cols, dtype=torch.float32, device=x.device)
        stream = torch.cuda.current_stream(x.device).cuda_stream
        c.gelu_bwd_bias(_DT[x.dtype], x.data_ptr(), dyc.data_ptr(),
                        dx.data_ptr(), ws.data_ptr(), rows, cols, nblocks,
                        stream)
        (dbias,) = _fold_partials([ws], nblocks, cols, ctx.bias_dtype)
        return dx, dbias


def _gelu_kernel_path(device: torch.device, dtype: torch.dtype) -> bool:
    return bool(device.type == "cuda" and _core() and dtype in _DT
                and not torch.is_autocast_enabled())


def gelu_bias_grad_fusable(device: torch.device, dtype: torch.dtype,
                           rows: int, cols: int,
                           bias: Optional[torch.Tensor]) -> bool:
    """Whether ``fused_gelu(x, bias=bias)`` on an x of this device and dtype
    with ``rows`` rows of ``cols`` elements takes bias' gradient from the
    GeLU backward: the kernel path, bf16 at a width it is built for, at
    least one row, a [cols] bias of a kernel dtype that wants a gradient.
    The caller asks before the linear and, on True, gives the linear
    ``bias.detach()``; ``fused_gelu`` decides by this function alone, so the
    two cannot disagree."""
    if not (FUSE_GELU_BIAS_GRAD and bias is not None and rows >= 1
            and cols >= 1 and _gelu_kernel_path(device, dtype)):
        return False
    if not (torch.is_grad_enabled() and bias.requires_grad):
        return False
    if bias.device != device or bias.dtype not in _DT \
            or bias.shape != (cols,):
        return False
    return bool(_core().gelu_bias_supported(cols, _DT[dtype]))


def fused_gelu(x: torch.Tensor,
               bias: Optional[torch.Tensor] = None) -> torch.Tensor:
    """F.gelu(x, approximate='tanh') drop-in; HIP kernel on GPU, torch
    fallback elsewhere.

    bias: the bias that the linear which produced x added. Where
    ``gelu_bias_grad_fusable`` holds for x and bias, the caller has given
    that linear ``bias.detach()`` and bias gets its gradient here: dx summed
    over the rows, rounded to bias' dtype. Everywhere else (CPU, autocast,
    other widths, the switch off) bias is ignored: it stayed attached to the
    linear and gets its gradient there."""
    if _gelu_kernel_path(x.device, x.dtype):
        cols = x.shape[-1] if x.dim() >= 1 else 0
        if gelu_bias_grad_fusable(x.device, x.dtype,
                                  x.numel() // max(cols, 1), cols, bias):
            return _FusedGeluBiasFn.apply(x, bias)
        return _FusedGeluFn.apply(x)
    return torch.nn.functional.gelu(x, approximate="tanh")


class FusedLayerNorm(nn.LayerNorm):
    """Drop-in nn.LayerNorm that runs the hand-written CDNA4 kernels when
    the shape/dtype qualify (GPU, matching weight dtype, supported width);
    falls back to the stock implementation otherwise (CPU, autocast-mixed
    dtypes, odd widths)."""

    def forward(self, x: torch.Tensor) -> torch.Tensor:
        if (
            x.is_cuda
            and not torch.is_autocast_enabled()
            and len(self.normalized_shape) == 1
            and self.weight is not None
            and self.bias is not None
            and self.weight.dtype == x.dtype
            and ln_fusable(x.shape[-1], x.dtype)
        ):
            return _FusedLayerNormFn.apply(x, self.weight, self.bias,
                                           self.eps)
        return super().forward(x)


# ---------------------------------------------------------------------------
# Residual dropout + add + LayerNorm
# ---------------------------------------------------------------------------
def dropout_add_keep_mask_reference(seed, rows: int, cols: int, p: float,
                                    site: int = 0) -> torch.Tensor:
    """The ln_dropadd kernels' keep(seed, site, row, col) as a [rows, cols]
    bool tensor on the CPU, in torch integer ops: the rectangular form of
    ``attention.dropout_keep_mask_reference`` with the plane index as the
    call site (csrc/attn_drop.h is the definition). seed: int or one-element
    int64 tensor."""
    from .attention import _M32, _drop_threshold, _fmix

    seed = int(seed) & 0xFFFFFFFFFFFFFFFF
    seed_lo, seed_hi = seed & _M32, seed >> 32
    site = int(site) & _M32
    r = torch.arange(rows, dtype=torch.int64).view(-1, 1)
    c = torch.arange(cols, dtype=torch.int64).view(1, -1)
    a = _fmix((seed_lo + site * 0x9E3779B1 + r * 0x85EBCA77) & _M32)
    b = _fmix(((seed_hi ^ ((site * 0xC2B2AE3D) & _M32))
               + c * 0x27D4EB2F) & _M32)
    x = (a + b) & _M32
    x = (x * 0x2C1B3C6D) & _M32
    x = x ^ (x >> 15)
    x = (x * 0x297A2D39) & _M32
    x = x ^ (x >> 15)
    return x >= _drop_threshold(p)


def _dropadd_fusable(h: torch.Tensor, residual: torch.Tensor,
                     weight: torch.Tensor, bias: torch.Tensor) -> bool:
    """What the ln_dropadd kernels take: GPU, no autocast, one dtype for
    all four, a supported width, 1 <= rows < 2^32 (the mask's row word)."""
    if not h.is_cuda or torch.is_autocast_enabled():
        return False
    if weight is None or bias is None or h.dim() < 1:
        return False
    if not (h.dtype == residual.dtype == weight.dtype == bias.dtype):
        return False
    if not (h.device == residual.device == weight.device == bias.device):
        return False
    cols = h.shape[-1]
    if weight.shape != (cols,) or bias.shape != (cols,) or cols == 0:
        return False
    if not 1 <= h.numel() // cols < 2 ** 32:
        return False
    return ln_fusable(cols, h.dtype)


def _launch_dropadd_fwd(h, residual, weight, bias, x_new, y, mean, rstd,
                        eps, dropout_p, seed, site):
    cols = h.shape[-1]
    stream = torch.cuda.current_stream(h.device).cuda_stream
    _core().ln_dropadd_fwd(
        _DT[h.dtype], h.data_ptr(), residual.data_ptr(), weight.data_ptr(),
        bias.data_ptr(), x_new.data_ptr(), y.data_ptr(), mean.data_ptr(),
        rstd.data_ptr(), h.numel() // cols, cols, eps, stream, dropout_p,
        seed.data_ptr() if dropout_p > 0.0 else 0, site)


def _launch_dropadd_bwd(dy, dx_new, x_new, weight, mean, rstd, dres, dh,
                        wsg, wsb, nblocks, dropout_p, seed, site):
    """dx_new: None when no gradient reaches x_new directly; dh: None at
    dropout_p = 0, where it equals dres."""
    cols = x_new.shape[-1]
    stream = torch.cuda.current_stream(x_new.device).cuda_stream
    _core().ln_dropadd_bwd(
        _DT[x_new.dtype], dy.data_ptr(),
        dx_new.data_ptr() if dx_new is not None else 0, x_new.data_ptr(),
        weight.data_ptr(), mean.data_ptr(), rstd.data_ptr(), dres.data_ptr(),
        dh.data_ptr() if dh is not None else 0, wsg.data_ptr(),
        wsb.data_ptr(), x_new.numel() // cols, cols, nblocks, stream,
        dropout_p, seed.data_ptr() if dropout_p > 0.0 else 0, site)


class _DropoutAddLayerNormFn(torch.autograd.Function):
    """(x_new, y) of the fused step. Saves x_new, weight, the row
    statistics and, with dropout, the seed: neither h nor a mask."""

    @staticmethod
    def forward(ctx, h, residual, weight, bias, eps, dropout_p, seed, site):
        hc, rc = h.contiguous(), residual.contiguous()
        cols = rc.shape[-1]
        rows = rc.numel() // cols
        x_new = torch.empty_like(rc)
        y = torch.empty_like(rc)
        mean = torch.empty(rows, dtype=torch.float32, device=rc.device)
        rstd = torch.empty_like(mean)
        _launch_dropadd_fwd(hc, rc, weight, bias, x_new, y, mean, rstd, eps,
                            dropout_p, seed, site)
        ctx.dropout_p, ctx.site = dropout_p, site
        if dropout_p > 0.0:
            ctx.save_for_backward(x_new, weight, mean, rstd, seed)
        else:
            ctx.save_for_backward(x_new, weight, mean, rstd)
        # an output nobody differentiates arrives as None, not as zeros
        ctx.set_materialize_grads(False)
        return x_new, y

    @staticmethod
    def backward(ctx, dx_new, dy):
        x_new, weight, mean, rstd, *seed = ctx.saved_tensors
        if dx_new is None and dy is None:
            return (None,) * 8
        cols = x_new.shape[-1]
        rows = x_new.numel() // cols
        # only x_new is used: the LN branch contributes exact zeros
        dyc = dy.contiguous() if dy is not None else torch.zeros_like(x_new)
        dxc = dx_new.contiguous() if dx_new is not None else None
        dres = torch.empty_like(x_new)
        dh = torch.empty_like(x_new) if ctx.dropout_p > 0.0 else None
        nblocks = max(1, min(1024, (rows + 3) // 4))
        nslots = nblocks * 4  # one partial per wave, as in ln_bwd
        ws = torch.empty(2 * nslots * cols, dtype=torch.float32,
                         device=x_new.device)
        wsg = ws[: nslots * cols]
        wsb = ws[nslots * cols:]
        _launch_dropadd_bwd(dyc, dxc, x_new, weight, mean, rstd, dres, dh,
                            wsg, wsb, nblocks, ctx.dropout_p,
                            seed[0] if seed else None, ctx.site)
        dgamma, dbeta = _fold_partials([wsg, wsb], nslots, cols, weight.dtype)
        return (dh if dh is not None else dres, dres, dgamma, dbeta,
                None, None, None, None)


def _dropout_add_layer_norm_composed(h, residual, weight, bias, eps,
                                     dropout_p, dropout_seed, site):
    """The same step in plain torch. With dropout it applies the replica
    mask in fp32 with one rounding, like the kernel, so an explicit seed
    drops the same elements on every path (reading the seed for the replica
    is a host sync on the GPU)."""
    from .attention import _seed_tensor

    cols = h.shape[-1]
    if dropout_p > 0.0:
        seed = _seed_tensor(dropout_seed, h.device)
        keep = dropout_add_keep_mask_reference(
            seed, h.numel() // max(cols, 1), cols, dropout_p, site)
        keep = keep.view(h.shape).to(h.device)
        rf = residual.float()
        x_new = torch.where(keep, rf + h.float() * (1.0 / (1.0 - dropout_p)),
                            rf).to(torch.result_type(h, residual))
    else:
        x_new = residual + h
    y = torch.nn.functional.layer_norm(x_new, (cols,), weight, bias, eps)
    return x_new, y


def fused_dropout_add_layer_norm(h: torch.Tensor, residual: torch.Tensor,
                                 weight: torch.Tensor, bias: torch.Tensor,
                                 eps: float = 1e-5, dropout_p: float = 0.0,
                                 dropout_seed: Optional[torch.Tensor] = None,
                                 site: int = 0):
    """x_new = residual + dropout(h, dropout_p); y = LayerNorm(x_new) over
    the last dimension. Returns (x_new, y), both differentiable. In fp32 per
    element, x_new = round(residual + h / (1 - p)) where kept and residual
    itself where dropped; y is exactly ``FusedLayerNorm`` of x_new.

    GPU tensors of one dtype (f32, f16, bf16) at a width ``ln_fusable``
    takes run the HIP kernels; anything else (CPU, autocast, mixed dtypes,
    other widths) composes the same step in torch. dropout_seed: one-element
    int64 tensor on the inputs' device fixing the mask, drawn from torch's
    generator when absent (not at dropout_p = 0). site: a uint32 naming the
    call site, so calls sharing one seed get independent masks."""
    if not 0.0 <= dropout_p < 1.0:
        raise ValueError("fused_dropout_add_layer_norm: need 0 <= dropout_p "
                         "< 1")
    if not 0 <= site < 2 ** 32:
        raise ValueError("fused_dropout_add_layer_norm: site is a uint32")
    if h.shape != residual.shape:
        raise ValueError("fused_dropout_add_layer_norm: h and residual "
                         "differ in shape")
    if _dropadd_fusable(h, residual, weight, bias):
        from .attention import _seed_tensor

        seed = (_seed_tensor(dropout_seed, h.device) if dropout_p > 0.0
                else None)
        return _DropoutAddLayerNormFn.apply(h, residual, weight, bias, eps,
                                            dropout_p, seed, site)
    return _dropout_add_layer_norm_composed(h, residual, weight, bias, eps,
                                            dropout_p, dropout_seed, site)
