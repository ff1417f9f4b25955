"""MoE routing + dispatch + combine, forward and backward, on one GPU:
the fused kernels (adapcc_amd/ops/moe.py) against the stock-torch op chain
of MoEMLP's non-fused path. world_size=1, expert MLPs excluded (the
dispatch buffer goes straight back into combine).

Run on a GPU box:  python benchmarks/moe_route_bench.py [--csv out.csv]
                                                       [--top-k 2]

d=1024, E=16, capacity_factor=1.25, T in {2048, 16384, 65536}, fp32 and
bf16. The two paths alternate in one process; every figure is the median
over --rounds windows of --iters steps timed with device events after a
warm-up, with the fastest and slowest window beside it. For the fused path
and for its two forward gather kernels on their own, the bytes the
algorithm has to move over the time taken are printed as GB/s.

--top-k 2 times top-2 routing with the balance loss in the backward pass
(capacity doubles): the fused kernels against the plain-torch fallback chain
of ops/moe.py (``use_kernels=False``), same columns; the two forward row
kernels are then the dispatch gather and the two-source scaled gather-sum.
"""
import argparse
import math
import os
import statistics
import sys

import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

D_MODEL = 1024
EXPERTS = 16
CAPACITY_FACTOR = 1.25
TOKENS = (2048, 16384, 65536)
DTYPES = (torch.float32, torch.bfloat16)


def torch_step(x, logits, cap):
    """MoEMLP.forward's non-fused body around an identity expert stage."""
    T, d = x.shape
    E = logits.shape[1]
    probs = logits.softmax(dim=-1)
    gate_p, expert_idx = probs.max(dim=-1)
    onehot = F.one_hot(expert_idx, E)
    pos = (onehot.cumsum(dim=0) - 1).gather(1, expert_idx[:, None]).squeeze(1)
    keep = pos < cap
    dispatch = x.new_zeros(E * cap, d)
    slot = expert_idx * cap + pos
    kept_slot = slot[keep]
    dispatch.index_copy_(0, kept_slot, x[keep])
    back = dispatch
    y = x.new_zeros(T, d)
    y[keep] = back.index_select(0, kept_slot) * gate_p[keep, None]
    return y


def fused_step(x, logits, cap):
    from adapcc_amd.ops.moe import (moe_combine, moe_dispatch,
                                    moe_route_top1)

    r = moe_route_top1(logits, cap)
    return moe_combine(moe_dispatch(x, r), r)


def torch_step_top2(x, logits, cap):
    """The plain-torch top-2 chain of ops/moe.py; the balance loss rides
    along so that its gradient is part of the backward pass."""
    from adapcc_amd.ops.moe import (moe_combine, moe_dispatch,
                                    moe_route_topk)

    r = moe_route_topk(logits, 2, cap, use_kernels=False)
    y = moe_combine(moe_dispatch(x, r, use_kernels=False), r,
                    use_kernels=False)
    return y, r.aux_loss


def fused_step_top2(x, logits, cap):
    from adapcc_amd.ops.moe import (moe_combine, moe_dispatch,
                                    moe_route_topk)

    r = moe_route_topk(logits, 2, cap)
    return moe_combine(moe_dispatch(x, r), r), r.aux_loss


def windows(fn, iters, rounds_us):
    """One window: `iters` calls between two device events -> us per call."""
    start = torch.cuda.Event(enable_timing=True)
    stop = torch.cuda.Event(enable_timing=True)
    start.record()
    for _ in range(iters):
        fn()
    stop.record()
    stop.synchronize()
    rounds_us.append(start.elapsed_time(stop) * 1e3 / iters)


def fused_bytes(T, E, cap, d, esize, kept):
    """Bytes the algorithm needs, forward + backward: each kernel reads the
    rows it gathers once and writes each output row once."""
    row = d * esize
    n = E * cap
    route = T * E * esize + 3 * 4 * T + 4 * n
    route_bwd = 2 * T * E * esize + 4 * 4 * T
    dispatch_fwd = 4 * n + kept * row + n * row
    dispatch_bwd = 4 * T + kept * row + T * row
    combine_fwd = 8 * T + kept * row + T * row
    combine_bwd = 4 * n + 4 * kept + kept * row + n * row   # dback
    rowdot = 4 * T + 2 * kept * row + 4 * T                 # dgate_p
    return (route + route_bwd + dispatch_fwd + dispatch_bwd + combine_fwd
            + combine_bwd + rowdot,
            dispatch_fwd, combine_fwd)


def fused_bytes_top2(T, E, cap, d, esize, kept, tok_kept):
    """The same model for the top-2 kernels: ``kept`` (token, choice) pairs
    hold a slot, ``tok_kept`` tokens have at least one of them. Maps and
    gates are [T, 2], every slot has a token and a choice entry."""
    row = d * esize
    n = E * cap
    route = T * E * esize + 7 * 4 * T + 2 * 4 * n + 4 * E + 4
    route_bwd = 2 * T * E * esize + 9 * 4 * T + 4 * E + 4
    dispatch_fwd = 4 * n + kept * row + n * row
    dispatch_bwd = 8 * T + kept * row + T * row             # two-source sum
    combine_fwd = 16 * T + kept * row + T * row             # scaled sum
    combine_bwd = 8 * n + 4 * kept + kept * row + n * row   # dback
    rowdot = 8 * T + (kept + tok_kept) * row + 8 * T        # dgate
    return (route + route_bwd + dispatch_fwd + dispatch_bwd + combine_fwd
            + combine_bwd + rowdot,
            dispatch_fwd, combine_fwd)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--csv", default=None, help="also write the table here")
    ap.add_argument("--top-k", type=int, default=1, choices=(1, 2))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("moe_route_bench: needs a GPU")

    from adapcc_amd.ops import moe

    rows = ["dtype,tokens,what,us_median,us_min,us_max,gbytes_per_s"]

    def emit(dtype, T, what, us, nbytes=None):
        med = statistics.median(us)
        rate = "" if nbytes is None else f"{nbytes / med / 1e3:.0f}"
        rows.append(f"{str(dtype).split('.')[-1]},{T},{what},{med:.1f},"
                    f"{min(us):.1f},{max(us):.1f},{rate}")
        print(rows[-1], flush=True)

    print(rows[0])
    for dtype in DTYPES:
        for T in TOKENS:
            E, d = EXPERTS, D_MODEL
            k = args.top_k
            cap = max(1, math.ceil(k * T / E * CAPACITY_FACTOR))
            torch.manual_seed(0)
            x = torch.randn(T, d, device="cuda", dtype=dtype,
                            requires_grad=True)
            logits = (torch.randn(T, E, device="cuda") * 2).to(dtype)
            logits.requires_grad_(True)
            gy = torch.randn(T, d, device="cuda", dtype=dtype)
            # a missing kernel is an error here, not torch against torch
            assert moe.moe_fusable(x, logits, cap, k)

            def run(step):
                x.grad = logits.grad = None
                step(x, logits, cap).backward(gy)

            def run2(step):
                x.grad = logits.grad = None
                y, aux = step(x, logits, cap)
                torch.autograd.backward([y, aux], [gy, torch.ones_like(aux)])

            if k == 1:
                paths = (("fused", lambda: run(fused_step)),
                         ("torch", lambda: run(torch_step)))
            else:
                paths = (("fused", lambda: run2(fused_step_top2)),
                         ("torch", lambda: run2(torch_step_top2)))
            us = {name: [] for name, _ in paths}
            for _, fn in paths:
                for _ in range(args.warmup):
                    fn()
            torch.cuda.synchronize()
            for _ in range(args.rounds):
                for name, fn in paths:
                    windows(fn, args.iters, us[name])

            with torch.no_grad():
                if k == 1:
                    r = moe.moe_route_top1(logits, cap)
                    kept = int((r.slot >= 0).sum())
                    total, b_disp, b_comb = fused_bytes(
                        T, E, cap, d, x.element_size(), kept)
                else:
                    r = moe.moe_route_topk(logits, 2, cap)
                    kept = int((r.slot >= 0).sum())
                    tok_kept = int((r.slot >= 0).any(dim=1).sum())
                    total, b_disp, b_comb = fused_bytes_top2(
                        T, E, cap, d, x.element_size(), kept, tok_kept)
                emit(dtype, T, "fused fwd+bwd", us["fused"], total)
                emit(dtype, T, "torch fwd+bwd", us["torch"])

                # the two forward gathers on their own
                out = torch.empty(E * cap, d, device="cuda", dtype=dtype)
                y = torch.empty(T, d, device="cuda", dtype=dtype)
                if k == 1:
                    def combine_fwd():
                        moe._launch_gather(out, r.slot, y, scale=r.gate_p)
                else:
                    def combine_fwd():
                        moe._launch_gather2(out, r.slot, y, scale=r.gate)
                kernels = (
                    ("gather dispatch fwd", b_disp,
                     lambda: moe._launch_gather(x, r.src, out)),
                    ("gather combine fwd", b_comb, combine_fwd))
                for what, nbytes, fn in kernels:
                    for _ in range(args.warmup):
                        fn()
                    ku = []
                    for _ in range(args.rounds):
                        windows(fn, args.iters, ku)
                    emit(dtype, T, what, ku, nbytes)

    if args.csv:
        with open(args.csv, "w") as f:
            f.write("\n".join(rows) + "\n")


if __name__ == "__main__":
    main()
