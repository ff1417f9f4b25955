#!/usr/bin/env python3
"""GPT-2 DDP training over the adapcc hook (reference:
models/gpt2/train_gpt2_ddp.py, re-targeted at the self-contained GPT-2 on
synthetic tokens — no dataset downloads in this environment).

    python -m torch.distributed.run --nproc-per-node 8 \
        --master-addr 127.0.0.1 examples/train_gpt2_ddp.py --model small

--pack-docs trains on documents of different lengths the way real text
comes: synthetic documents with seeded random lengths, packed back to back
into one [1, batch * seq] row with cu_seqlens, so attention stays inside
each document (the variable-length kernels) and no token is padding.
--pad-docs feeds the same documents the way it had to be done without
that: one row per document, padded to --seq.
"""

from __future__ import annotations

import argparse
import math
import os
import statistics
import sys
import time

import torch
import torch.distributed as dist
from torch.nn.parallel import DistributedDataParallel as DDP

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from adapcc_amd import AdapCC, CommArgs
from adapcc_amd.models.gpt2 import GPT2, GPT2Config
from adapcc_amd.runtime.hook import AdapccDDPState, adapcc_allreduce_hook


def synthetic_docs(tokens: int, max_len: int, vocab: int, seed: int):
    """Documents of random tokens whose lengths are drawn log-uniformly in
    [16, max_len] from `seed` and sum to `tokens` (the last one cut)."""
    gen = torch.Generator().manual_seed(seed)
    lo = min(16, max_len)
    docs, left = [], tokens
    while left > 0:
        u = torch.rand((), generator=gen).item()
        n = int(round(math.exp(math.log(lo)
                               + u * (math.log(max_len) - math.log(lo)))))
        n = min(max(n, lo), max_len, left)
        docs.append(torch.randint(0, vocab, (n,), generator=gen))
        left -= n
    return docs


def next_token_targets(doc: torch.Tensor) -> torch.Tensor:
    """The document shifted by one; its last position has no target."""
    t = torch.roll(doc, -1)
    t[-1] = -100
    return t


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--model", default="small", choices=["tiny", "small", "medium"])
    p.add_argument("--steps", type=int, default=20)
    p.add_argument("--batch", type=int, default=8)
    p.add_argument("--seq", type=int, default=512)
    p.add_argument("--lr", type=float, default=3e-4)
    p.add_argument("--entry_point", type=int, default=-1)
    p.add_argument("--relay", action="store_true")
    p.add_argument("--dropout", type=float, default=0.0,
                   help="attention, residual and embedding dropout (the "
                        "reference's GPT2Config default is 0.1); attention "
                        "dropout runs inside the flash attention kernels, "
                        "residual dropout inside the fused add+LayerNorm")
    p.add_argument("--pack-docs", action="store_true",
                   help="documents of seeded random lengths packed into one "
                        "[1, batch*seq] row with cu_seqlens")
    p.add_argument("--pad-docs", action="store_true",
                   help="the documents of --pack-docs, one per row, padded "
                        "to --seq")
    args = p.parse_args()
    if args.pack_docs and args.pad_docs:
        p.error("--pack-docs and --pad-docs exclude each other")

    rank = int(os.environ.get("RANK", 0))
    local_rank = int(os.environ.get("LOCAL_RANK", 0))
    world = int(os.environ.get("WORLD_SIZE", 1))
    use_cuda = torch.cuda.is_available()
    dev_idx = local_rank % max(1, torch.cuda.device_count() or 1)
    device = torch.device(f"cuda:{dev_idx}" if use_cuda else "cpu")
    if use_cuda:
        torch.cuda.set_device(device)
    if world > 1:
        dist.init_process_group("nccl" if use_cuda else "gloo")

    cfg = getattr(GPT2Config, args.model)()
    cfg.dropout = args.dropout
    cfg.resid_dropout = args.dropout
    torch.manual_seed(1)
    model = GPT2(cfg).to(device)
    AdapCC.init(CommArgs(entry_point=args.entry_point, relay=args.relay),
                local_rank, rank, world)
    AdapCC.setup()

    if world > 1:
        model = DDP(model, device_ids=[device.index] if use_cuda else None,
                    bucket_cap_mb=100)
        state = AdapccDDPState(AdapCC.communicator)
        model.register_comm_hook(state, adapcc_allreduce_hook)
    else:
        state = None

    opt = torch.optim.AdamW(model.parameters(), lr=args.lr)
    T = min(args.seq, cfg.n_positions)
    torch.manual_seed(100 + rank)
    data = torch.randint(0, cfg.vocab_size, (args.batch, T + 1), device=device)
    x, y = data[:, :-1], data[:, 1:].contiguous()
    cu_seqlens = None
    if args.pack_docs or args.pad_docs:
        docs = synthetic_docs(args.batch * T, T, cfg.vocab_size, 100 + rank)
        if args.pack_docs:
            x = torch.cat(docs)[None].to(device)
            # boundary targets masked: no document predicts the next one
            y = torch.cat([next_token_targets(d) for d in docs])[None]
            y = y.to(device)
            offsets = [0]
            for d in docs:
                offsets.append(offsets[-1] + len(d))
            cu_seqlens = torch.tensor(offsets, dtype=torch.int32,
                                      device=device)
        else:
            x = torch.zeros(len(docs), T, dtype=torch.long)
            y = torch.full((len(docs), T), -100, dtype=torch.long)
            for i, d in enumerate(docs):
                x[i, :len(d)] = d
                y[i, :len(d)] = next_token_targets(d)
            x, y = x.to(device), y.to(device)
        if rank == 0:
            print(f"{len(docs)} documents, {sum(len(d) for d in docs)} "
                  f"tokens, input {tuple(x.shape)}", flush=True)
    kw = {} if cu_seqlens is None else {"cu_seqlens": cu_seqlens}

    times = []
    for step in range(args.steps):
        t0 = time.perf_counter()
        if state is not None:
            state.on_step(step)
        opt.zero_grad(set_to_none=True)
        with torch.autocast(device.type, dtype=torch.bfloat16,
                            enabled=use_cuda):
            _, loss = model(x, y, **kw)
        loss.backward()
        opt.step()
        if use_cuda:
            torch.cuda.synchronize()
        times.append(1000 * (time.perf_counter() - t0))
        if rank == 0:
            print(f"step {step}: loss {loss.item():.4f} "
                  f"({times[-1]:.1f} ms)", flush=True)
    if rank == 0 and len(times) > 10:
        print(f"median of the last {len(times) - 10} steps: "
              f"{statistics.median(times[10:]):.1f} ms/step", flush=True)

    AdapCC.clear()
    if world > 1:
        dist.destroy_process_group()


if __name__ == "__main__":
    main()
