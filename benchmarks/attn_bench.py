"""Flash-attention kernel timing: hand-written CDNA4 kernels vs torch SDPA.

Run on a GPU box:  python benchmarks/attn_bench.py
                       [--shape gpt2|vit|gpt2-d128|vit-d128|varlen|decode|extend]
                       [--dropout P] [--head-dim 64|128] [--kv-heads N]

gpt2 (default): B64 H12 S1024 D64, causal. vit: B64 H12 S197 D64, non-causal
(ViT-base at 224 px). gpt2-d128: B32 H16 S1024 D128, causal; vit-d128: B64 H8
S197 D128, non-causal: the head_dim 128 kernels. --dropout P times both paths with attention dropout at
rate P (ours inside the kernels, a fresh seed drawn per call as in training).
varlen: 131072 tokens of H12 D64 causal packed sequences through
flash_attention_qkv_varlen, first as 128 sequences of 1024 against the
fixed-length packed kernel on the same work (the cost of the mode), then as
a seeded mix of lengths drawn log-uniformly in [16, 1024] against the same
documents padded to 1024 and against SDPA under a dense block-diagonal mask
(what the mode is for), and the plan kernel by itself. --head-dim 128 (varlen
only) runs the same token count as H6 D128.
--kv-heads N (the fixed shapes and varlen): grouped-query attention with N
K/V heads. Times, alternating in one process, (a) the GQA call, (b) what
GQA costs without it: K/V repeat_interleave'd to H heads in front of the
same kernels and autograd summing dk/dv over the group, with those passes
and (K/V expanded beforehand, per-head dk/dv left as they are) without, and
(c) torch SDPA with enable_gqa=True.
decode: one query row per sequence over a full KV cache of 1024 and 16384
keys, B 1 and 32; --head-dim 128 is H16 with 16, 4 and 1 K/V heads,
--head-dim 64 H12 with 12 and 1 (--kv-heads N: that count alone). Times,
alternating in one process, flash_attention_decode (and, as "no checks",
the launch helper under it: the difference is what the entry point's
argument checks cost on the host) against torch SDPA under the key-length mask
with enable_gqa and against this project's flash_attention(causal=False) on
the one-row query (which, its kernels being self-attention only, resolves to
SDPA without a mask on the cache cut to the common length), and prints microseconds and the K/V bytes per second,
2 * B * Hk * len * D * 2 bytes over the time. --sweep adds forced split
counts, the measurement behind the split policy's constants. --fp8 (decode
and extend) instead times the e4m3 cache of the same keys against the bf16
one, and with --page-size both through a block table as well; for extend at
three shapes of its split sweep (byte-, split- and compute-bound).
extend: a block of Sq query rows per sequence over a KV cache, causal, with
the same heads as decode: pure prefill (B8, Sq 1024 and 1000, empty cache),
chunked prefill (B8, Sq 512 over 3584 cached keys) and short chunks (B32 and
B1, Sq 8 over 4096 and 16384). Times, alternating in one process,
flash_attention_extend on a cache that already holds the chunk's keys, the
same call appending them itself, the composed route on the same cache (torch
SDPA under the explicit [B,1,Sq,Smax] mask with enable_gqa: the only route
for these calls before the kernel), and, where the old prefill applies
(empty cache, Sq % 128 == 0), flash_attention(causal=True) on q, k_new,
v_new plus the two zero-filled cache copies that prefill made, and that
forward alone. Prints the
time with the spread of the rounds and the achieved FLOP/s (4 * B * H * D *
visible (row, key) pairs) or, for the short chunks, K/V bytes per second,
and for those the workgroup count against the CUs and the key splits the
policy chose. --sweep adds forced split counts, the measurement behind
keeping decode's policy constants.
"""
import argparse
import math
import os
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

SHAPES = {
    # name: (B, H, S, D, causal)
    "gpt2": (64, 12, 1024, 64, True),
    "vit": (64, 12, 197, 64, False),
    "gpt2-d128": (32, 16, 1024, 128, True),
    "vit-d128": (64, 8, 197, 128, False),
}


def bench(fn, iters=20, warmup=5):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(iters):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / iters * 1e3  # ms


def main():
    from adapcc_amd.ops.attention import fa_supported, flash_attention

    ap = argparse.ArgumentParser()
    ap.add_argument("--shape", choices=sorted(SHAPES) + ["varlen", "decode",
                                                       "extend"],
                    default="gpt2")
    ap.add_argument("--sweep", action="store_true",
                    help="decode and extend: also time forced split counts")
    ap.add_argument("--iters", type=int, default=None,
                    help="timed calls per figure (default 20; 200 for vit, "
                         "whose calls are ~10x shorter)")
    ap.add_argument("--dropout", type=float, default=0.0,
                    help="attention dropout rate for both paths")
    ap.add_argument("--head-dim", type=int, choices=(64, 128), default=64,
                    help="varlen only: 128 halves the heads, same tokens")
    ap.add_argument("--kv-heads", type=int, default=0,
                    help="K/V heads (must divide the shape's heads): the "
                         "grouped-query comparison instead of the usual one")
    ap.add_argument("--page-size", type=int, default=0,
                    help="decode and extend: time a paged cache of this page "
                         "size (a power of two >= 16) against the contiguous "
                         "one instead")
    ap.add_argument("--fp8", action="store_true",
                    help="decode and extend: time an e4m3 KV cache against "
                         "the bf16 one (with --page-size also both paged)")
    args = ap.parse_args()
    drop = args.dropout
    if args.fp8:
        if args.shape == "extend":
            return fp8_extend_path(args.page_size)
        if args.shape != "decode":
            ap.error("--fp8 goes with --shape decode or extend")
        return fp8_path(args.head_dim, args.kv_heads, args.page_size)
    if args.page_size:
        if args.shape not in ("decode", "extend"):
            ap.error("--page-size goes with --shape decode or extend")
        return paged_path(args.shape, args.page_size)
    if args.shape == "decode":
        return decode_path(args.head_dim, args.kv_heads, args.sweep)
    if args.shape == "extend":
        return extend_path(args.head_dim, args.kv_heads, args.sweep)
    if args.shape == "varlen":
        H = 12 * 64 // args.head_dim
        if args.kv_heads:
            return gqa_varlen_path(H, args.kv_heads, args.head_dim, drop)
        return varlen_path(args.iters or 20, drop, H=H, D=args.head_dim)
    B, H, S, D, causal = SHAPES[args.shape]
    if args.kv_heads:
        return gqa_path(B, H, args.kv_heads, S, D, causal, drop)
    iters = args.iters or (200 if args.shape.startswith("vit") else 20)

    scale = 1.0 / math.sqrt(D)
    torch.manual_seed(0)
    q = torch.randn(B, H, S, D, device="cuda", dtype=torch.bfloat16,
                    requires_grad=True)
    k = torch.randn_like(q, requires_grad=True)
    v = torch.randn_like(q, requires_grad=True)
    g = torch.randn(B, H, S, D, device="cuda", dtype=torch.bfloat16)
    # a missing kernel is an error here, not a silent SDPA-vs-SDPA run
    assert fa_supported(q, k, v, causal, drop)

    # FLOPs: fwd 2 matmuls, bwd 5; the causal mask halves both
    fwd_flops = 4 * B * H * S * S * D / (2 if causal else 1)
    bwd_flops = 2.5 * fwd_flops

    def fa_fwd():
        return flash_attention(q, k, v, causal=causal, dropout_p=drop,
                               scale=scale)

    def sdpa_fwd():
        return torch.nn.functional.scaled_dot_product_attention(
            q, k, v, is_causal=causal, dropout_p=drop)

    for name, f in (("adapcc-fa", fa_fwd), ("torch-sdpa", sdpa_fwd)):
        ms = bench(lambda: f(), iters)
        print(f"{name} fwd:  {ms:7.3f} ms  {fwd_flops/ms/1e9:8.1f} TF/s")

        def fb():
            q.grad = k.grad = v.grad = None
            o = f()
            o.backward(g)

        ms = bench(fb, iters)
        print(f"{name} f+b:  {ms:7.3f} ms  {(fwd_flops+bwd_flops)/ms/1e9:8.1f} TF/s")

    layer_path(B, H, S, D, causal, fwd_flops, bwd_flops, iters, drop)


def layer_path(B, H, S, D, causal, fwd_flops, bwd_flops, iters, drop=0.0):
    """What one transformer layer pays: packed projection [B,T,3C] in,
    [B,T,C] out, contiguous [B,T,C] upstream gradient. 'composed' is
    split + head views + flash_attention + transpose/contiguous (autograd
    cats the three gradients); 'packed' is flash_attention_qkv."""
    from adapcc_amd.ops.attention import (_attention_qkv_composed,
                                          flash_attention_qkv)

    C = H * D
    qkv = torch.randn(B, S, 3 * C, device="cuda", dtype=torch.bfloat16,
                      requires_grad=True)
    gy = torch.randn(B, S, C, device="cuda", dtype=torch.bfloat16)
    for name, f in (("layer composed", _attention_qkv_composed),
                    ("layer packed", flash_attention_qkv)):
        ms = bench(lambda: f(qkv, H, dropout_p=drop, causal=causal), iters)
        print(f"{name} fwd:  {ms:7.3f} ms  {fwd_flops/ms/1e9:8.1f} TF/s")

        def fb():
            qkv.grad = None
            f(qkv, H, dropout_p=drop, causal=causal).backward(gy)

        ms = bench(fb, iters)
        print(f"{name} f+b:  {ms:7.3f} ms  {(fwd_flops+bwd_flops)/ms/1e9:8.1f} TF/s")


def alternate(fns, window=0.5, rounds=5):
    """Times the callables of `fns` (name -> fn) against each other: after
    a warmup of each, `rounds` rounds that run every candidate in turn for
    window/rounds seconds' worth of calls (from a first estimate), each
    block ended by a synchronise. Returns name -> (mean ms per call over
    all rounds, fastest round, slowest round)."""
    calls = {}
    for name, fn in fns.items():
        ms = bench(fn, iters=3, warmup=3)
        calls[name] = max(2, int(math.ceil(window / rounds * 1e3 / ms)))
    per_round = {name: [] for name in fns}
    for _ in range(rounds):
        for name, fn in fns.items():
            per_round[name].append(bench(fn, iters=calls[name], warmup=0))
    return {name: (sum(r) / len(r), min(r), max(r))
            for name, r in per_round.items()}


def decode_path(D, kv_heads, sweep):
    from adapcc_amd.ops.attention import (_launch_decode, fa_decode_supported,
                                          fa_supported, flash_attention,
                                          flash_attention_decode)

    H = 16 if D == 128 else 12
    kv = [kv_heads] if kv_heads else ([16, 4, 1] if D == 128 else [12, 1])
    sdpa = torch.nn.functional.scaled_dot_product_attention
    scale = 1.0 / math.sqrt(D)
    for B in (1, 32):
        for Hk in kv:
            for n in (1024, 16384):
                torch.manual_seed(0)
                q = torch.randn(B, H, D, device="cuda", dtype=torch.bfloat16)
                k = torch.randn(B, Hk, n, D, device="cuda",
                                dtype=torch.bfloat16)
                v = torch.randn_like(k)
                lens = torch.full((B,), n, dtype=torch.int32, device="cuda")
                mask = (torch.arange(n, device="cuda").view(1, 1, 1, n)
                        < lens.view(B, 1, 1, 1))
                q4 = q.unsqueeze(2)
                # a missing kernel is an error, not a silent SDPA-vs-SDPA run
                assert fa_decode_supported(q, k, v, lens)
                # the training kernels take q, k, v of one length only, so
                # flash_attention hands this shape to SDPA (no mask: the
                # cache is cut to the common length, here all of it)
                assert not fa_supported(q4, k, v, False, 0.0)
                fns = {
                    "decode": lambda: flash_attention_decode(q, k, v, lens),
                    "decode, no checks": lambda: _launch_decode(
                        q, k, v, lens, None, None, scale, None, False),
                    "sdpa masked": lambda: sdpa(q4, k, v, attn_mask=mask,
                                                enable_gqa=Hk != H),
                    "flash_attention->sdpa": lambda: flash_attention(
                        q4, k, v, causal=False),
                }
                if sweep:
                    for ns in (1, 4, 16, 32, 64, 128):
                        fns[f"decode splits={ns}"] = (
                            lambda ns=ns: flash_attention_decode(
                                q, k, v, lens, num_splits=ns))
                ref = sdpa(q4.float(), k.float(), v.float(),
                           enable_gqa=Hk != H).squeeze(2)
                err = (flash_attention_decode(q, k, v, lens).float()
                       - ref).abs().max().item()
                nbytes = 2 * B * Hk * n * D * 2
                print(f"B{B} H{H} Hk{Hk} D{D} len{n}  "
                      f"(K/V {nbytes / 2**20:.1f} MiB, max err vs fp32 "
                      f"{err:.2e})")
                base = None
                for name, (ms, lo, hi) in alternate(fns, window=0.3).items():
                    base = base or ms
                    print(f"  {name:<22} {ms * 1e3:9.1f} us  (rounds "
                          f"{lo * 1e3:.1f}..{hi * 1e3:.1f})  "
                          f"{nbytes / ms / 1e9:6.2f} TB/s  "
                          f"this/decode {ms / base:.2f}")
                del q, k, v, mask, ref


def fp8_path(D, kv_heads, P):
    """--fp8: decode over an e4m3 cache against the bf16 cache of the same
    keys, alternating in one process, at decode_path's shapes; with
    --page-size also both through a block table. 'bf16 again' is the first
    candidate a second time: what two timings of one code differ by. Bytes
    per second count the K/V bytes of the candidate's own cache; the bound on
    fp8 / bf16 time is the byte ratio, 0.5."""
    from adapcc_amd.ops.attention import (fa_decode_supported,
                                          flash_attention_decode,
                                          kv_quantize_reference)

    H = 16 if D == 128 else 12
    kv = [kv_heads] if kv_heads else ([16, 4, 1] if D == 128 else [12, 1])
    for B in (1, 32):
        for Hk in kv:
            for n in (1024, 16384):
                torch.manual_seed(0)
                q = torch.randn(B, H, D, device="cuda", dtype=torch.bfloat16)
                k = torch.randn(B, Hk, n, D, device="cuda",
                                dtype=torch.bfloat16)
                v = torch.randn_like(k)
                lens = torch.full((B,), n, dtype=torch.int32, device="cuda")
                ks = torch.full((Hk,), 6.0 / 448, device="cuda")
                vs = ks.clone()
                k8 = kv_quantize_reference(k, ks)
                v8 = kv_quantize_reference(v, vs)
                sc = dict(k_scale=ks, v_scale=vs)
                # a missing kernel is an error, not a composed-route run
                assert fa_decode_supported(q, k, v, lens)
                assert fa_decode_supported(q, k8, v8, lens, **sc)
                fns = {
                    "bf16": lambda: flash_attention_decode(q, k, v, lens),
                    "fp8": lambda: flash_attention_decode(q, k8, v8, lens,
                                                          **sc),
                    "bf16 again": lambda: flash_attention_decode(q, k, v,
                                                                 lens),
                }
                if P:
                    mp = n // P
                    table = torch.randperm(B * mp, device="cuda").view(B, mp)
                    pools = []
                    for t in (k, v, k8.view(torch.uint8), v8.view(torch.uint8)):
                        pool = torch.empty(B * mp, Hk, P, D, device="cuda",
                                           dtype=t.dtype)
                        pool[table.view(-1)] = t.view(
                            B, Hk, mp, P, D).transpose(1, 2).reshape(
                                -1, Hk, P, D)
                        pools.append(pool)
                    kp, vp = pools[:2]
                    kp8, vp8 = (t.view(k8.dtype) for t in pools[2:])
                    table = table.int()
                    assert fa_decode_supported(q, kp8, vp8, lens, table, **sc)
                    fns[f"bf16 paged P={P}"] = lambda: flash_attention_decode(
                        q, kp, vp, lens, block_table=table)
                    fns[f"fp8 paged P={P}"] = lambda: flash_attention_decode(
                        q, kp8, vp8, lens, block_table=table, **sc)
                err = (flash_attention_decode(q, k8, v8, lens, **sc).float()
                       - flash_attention_decode(q, k, v, lens).float()
                       ).abs().max().item()
                nbytes = 2 * B * Hk * n * D * 2
                print(f"B{B} H{H} Hk{Hk} D{D} len{n}  (bf16 K/V "
                      f"{nbytes / 2**20:.1f} MiB, max |fp8 - bf16| {err:.2e})")
                base = None
                for name, (ms, lo, hi) in alternate(fns, window=0.3).items():
                    base = base or ms
                    nb = nbytes // 2 if name.startswith("fp8") else nbytes
                    print(f"  {name:<22} {ms * 1e3:9.1f} us  (rounds "
                          f"{lo * 1e3:.1f}..{hi * 1e3:.1f})  "
                          f"{nb / ms / 1e9:6.2f} TB/s  "
                          f"this/bf16 {ms / base:.3f}")
                del q, k, v, k8, v8, fns


def fp8_extend_path(P):
    """--fp8 --shape extend: flash_attention_extend over an e4m3 cache
    against the bf16 cache of the same keys, fp8_path's method (alternating
    in one process, 'bf16 again' the noise figure), at three shapes of the
    split sweep in attn_extend.hip's header: byte-bound (the bound on fp8 /
    bf16 time is the byte ratio, 0.5), split- and launch-bound, and
    compute-bound, where fp8 can only cost its conversion. The cache holds
    the chunk's keys already; '+ append' has the call write them. With
    --page-size also both through a block table."""
    from adapcc_amd.ops.attention import (_core, fa_extend_supported,
                                          flash_attention_extend,
                                          kv_quantize_reference)

    bf = dict(device="cuda", dtype=torch.bfloat16)
    for B, H, Hk, D, Sq, keys in ((32, 16, 16, 128, 8, 16384),
                                  (1, 16, 4, 128, 8, 16384),
                                  (8, 12, 12, 64, 512, 3584)):
        torch.manual_seed(0)
        q = torch.randn(B, H, Sq, D, **bf)
        k = torch.randn(B, Hk, keys, D, **bf)
        v = torch.randn_like(k)
        lens = torch.full((B,), keys, dtype=torch.int32, device="cuda")
        lens0 = lens - Sq
        kn, vn = k[:, :, keys - Sq:].clone(), v[:, :, keys - Sq:].clone()
        ks = torch.full((Hk,), 6.0 / 448, device="cuda")
        vs = ks.clone()
        k8, v8 = kv_quantize_reference(k, ks), kv_quantize_reference(v, vs)
        sc = dict(k_scale=ks, v_scale=vs)
        # a missing kernel is an error, not a composed-route run
        assert fa_extend_supported(q, k, v, lens)
        assert fa_extend_supported(q, k8, v8, lens, **sc)
        fns = {
            "bf16": lambda: flash_attention_extend(q, k, v, lens),
            "fp8": lambda: flash_attention_extend(q, k8, v8, lens, **sc),
            "bf16 again": lambda: flash_attention_extend(q, k, v, lens),
            "bf16 + append": lambda: flash_attention_extend(q, k, v, lens0,
                                                            kn, vn),
            "fp8 + append": lambda: flash_attention_extend(q, k8, v8, lens0,
                                                           kn, vn, **sc),
        }
        if P:
            mp = keys // P
            table = torch.randperm(B * mp, device="cuda").view(B, mp)
            pools = []
            for t in (k, v, k8.view(torch.uint8), v8.view(torch.uint8)):
                pool = torch.empty(B * mp, Hk, P, D, device="cuda",
                                   dtype=t.dtype)
                pool[table.view(-1)] = t.view(B, Hk, mp, P, D).transpose(
                    1, 2).reshape(-1, Hk, P, D)
                pools.append(pool)
            kp, vp = pools[:2]
            kp8, vp8 = (t.view(k8.dtype) for t in pools[2:])
            table = table.int()
            assert fa_extend_supported(q, kp8, vp8, lens, None, table, **sc)
            fns[f"bf16 paged P={P}"] = lambda: flash_attention_extend(
                q, kp, vp, lens, block_table=table)
            fns[f"fp8 paged P={P}"] = lambda: flash_attention_extend(
                q, kp8, vp8, lens, block_table=table, **sc)
        err = (fns["fp8"]().float() - fns["bf16"]().float()).abs().max().item()
        nbytes = 2 * B * Hk * keys * D * 2
        ns = _core().fa_extend_splits(B, Hk, Sq, H // Hk, keys, 0, 0)
        print(f"B{B} H{H} Hk{Hk} D{D} Sq{Sq} keys{keys}  (bf16 K/V "
              f"{nbytes / 2**20:.1f} MiB, {ns} splits, max |fp8 - bf16| "
              f"{err:.2e})")
        base = None
        for name, (ms, lo, hi) in alternate(fns, window=0.5).items():
            base = base or ms
            nb = nbytes // 2 if name.startswith("fp8") else nbytes
            print(f"  {name:<22} {ms * 1e3:9.1f} us  (rounds "
                  f"{lo * 1e3:.1f}..{hi * 1e3:.1f})  "
                  f"{nb / ms / 1e9:6.2f} TB/s  this/bf16 {ms / base:.3f}")
        del q, k, v, k8, v8, fns


def paged_path(shape, P):
    """--page-size: the paged call (a pool [N,Hk,P,D] under a shuffled block
    table) against the contiguous call on the same keys, alternating in one
    process, at the shapes the kernel headers quote. 'contiguous again' is
    the first candidate a second time: what two timings of one code differ
    by. 'gather + contiguous' is what a caller with pages had to do before
    block_table: build the slab, then call."""
    from adapcc_amd.ops.attention import (fa_decode_supported,
                                          fa_extend_supported,
                                          flash_attention_decode,
                                          flash_attention_extend)

    bf = dict(device="cuda", dtype=torch.bfloat16)
    decode = shape == "decode"
    cases = (((32, 16, 4, 128, 1, 16383), (1, 16, 16, 128, 1, 16383))
             if decode else
             ((1, 16, 4, 128, 8, 16384), (8, 12, 12, 64, 512, 3584)))
    for B, H, Hk, D, Sq, past in cases:
        torch.manual_seed(0)
        mp = -(-(past + Sq) // P)
        Smax = mp * P
        q = torch.randn(B, H, Sq, D, **bf)
        k = torch.randn(B, Hk, Smax, D, **bf)
        v = torch.randn_like(k)
        lens = torch.full((B,), past + Sq, dtype=torch.int32, device="cuda")
        table = torch.randperm(B * mp, device="cuda").view(B, mp).int()
        tl = table.long()
        pools = []
        for t in (k, v):
            pool = torch.empty(B * mp, Hk, P, D, **bf)
            pool[tl.view(-1)] = t.view(B, Hk, mp, P, D).transpose(
                1, 2).reshape(-1, Hk, P, D)
            pools.append(pool)
        kp, vp = pools

        def call(kc, vc, **kw):
            if decode:
                return flash_attention_decode(q[:, :, 0], kc, vc, lens, **kw)
            return flash_attention_extend(q, kc, vc, lens, **kw)

        def gather():
            return call(*(t[tl].transpose(1, 2).reshape(B, Hk, Smax, D)
                          for t in (kp, vp)))

        # a missing kernel is an error, not a silent composed-route run
        assert (fa_decode_supported(q[:, :, 0], kp, vp, lens,
                                    block_table=table) if decode else
                fa_extend_supported(q, kp, vp, lens, block_table=table))
        assert torch.equal(call(k, v), call(kp, vp, block_table=table))
        assert torch.equal(call(k, v), gather())
        fns = {
            "contiguous": lambda: call(k, v),
            f"paged P={P}": lambda: call(kp, vp, block_table=table),
            "contiguous again": lambda: call(k, v),
            "gather + contiguous": gather,
        }
        nbytes = 2 * B * Hk * Smax * D * 2
        print(f"{shape} B{B} H{H} Hk{Hk} D{D} Sq{Sq} keys{past + Sq} P{P} "
              f"({mp} pages a sequence, K/V {nbytes / 2**20:.1f} MiB)")
        base = None
        for name, (ms, lo, hi) in alternate(fns, window=0.3).items():
            base = base or ms
            print(f"  {name:<22} {ms * 1e3:9.1f} us  (rounds "
                  f"{lo * 1e3:.1f}..{hi * 1e3:.1f})  "
                  f"{nbytes / ms / 1e9:6.2f} TB/s  "
                  f"this/contiguous {ms / base:.3f}")
        del q, k, v, kp, vp, pools


def extend_path(D, kv_heads, sweep):
    from adapcc_amd.ops.attention import (_core, _extend_composed,
                                          fa_extend_supported, fa_supported,
                                          flash_attention,
                                          flash_attention_extend)

    H = 16 if D == 128 else 12
    kv = [kv_heads] if kv_heads else ([16, 4, 1] if D == 128 else [12, 1])
    n_cu = torch.cuda.get_device_properties(0).multi_processor_count
    bf = dict(device="cuda", dtype=torch.bfloat16)
    for B, Sq, past in ((8, 1024, 0), (8, 1000, 0), (8, 512, 3584),
                        (32, 8, 4096), (32, 8, 16384), (1, 8, 4096),
                        (1, 8, 16384)):
        for Hk in kv:
            torch.manual_seed(0)
            Smax = past + Sq
            q = torch.randn(B, H, Sq, D, **bf)
            k = torch.randn(B, Hk, Smax, D, **bf)
            v = torch.randn_like(k)
            kn = k[:, :, past:].clone()
            vn = v[:, :, past:].clone()
            lens0 = torch.full((B,), past, dtype=torch.int32, device="cuda")
            lens1 = lens0 + Sq
            # a missing kernel is an error, not a silent SDPA-vs-SDPA run
            assert fa_extend_supported(q, k, v, lens0)
            fns = {
                "extend": lambda: flash_attention_extend(q, k, v, lens1),
                "extend + append": lambda: flash_attention_extend(
                    q, k, v, lens0, kn, vn),
                "composed sdpa mask": lambda: _extend_composed(
                    q, k, v, lens1, None, None, None, True, None, False),
            }
            if past == 0 and Sq % 128 == 0:
                assert fa_supported(q, kn, vn, True, 0.0)

                def old_prefill():
                    for t in (kn, vn):
                        c = t.new_zeros(B, Smax, Hk, D)
                        c[:, :Sq] = t.transpose(1, 2)
                    return flash_attention(q, kn, vn, causal=True)

                fns["forward + 2 cache copies"] = old_prefill
                fns["forward alone"] = lambda: flash_attention(
                    q, kn, vn, causal=True)
            policy = _core().fa_extend_splits(B, Hk, Sq, H // Hk, Smax, 0, 0)
            if sweep:
                for ns in (1, 2, 4, 8, 16, 32):
                    fns[f"extend splits={ns}"] = (
                        lambda ns=ns: flash_attention_extend(
                            q, k, v, lens1, num_splits=ns))
            want = _extend_composed(q.float(), k.float(), v.float(), lens1,
                                    None, None, None, True, None, False)
            err = (fns["extend"]().float() - want).abs().max().item()
            pairs = Sq * past + Sq * (Sq + 1) // 2
            flops = 4 * B * H * D * pairs
            nbytes = 2 * B * Hk * Smax * D * 2
            short = Sq < 128
            wgs = B * Hk * -(-Sq * (H // Hk) // 128)
            print(f"B{B} H{H} Hk{Hk} D{D} Sq{Sq} past{past}  "
                  f"({flops / 1e9:.1f} GFLOP, K/V {nbytes / 2**20:.1f} MiB, "
                  f"{wgs} workgroups x {policy} splits on {n_cu} CUs, max "
                  f"err vs fp32 {err:.2e})")
            base = None
            for name, (ms, lo, hi) in alternate(fns, window=0.3).items():
                base = base or ms
                rate = (f"{nbytes / ms / 1e9:6.2f} TB/s" if short
                        else f"{flops / ms / 1e9:7.1f} TF/s")
                print(f"  {name:<26} {ms * 1e3:9.1f} us  (rounds "
                      f"{lo * 1e3:.1f}..{hi * 1e3:.1f})  {rate}  "
                      f"this/extend {ms / base:.2f}")
            del q, k, v, kn, vn, want


def report(title, res, flops):
    print(title)
    base = res["gqa"][0]
    for name, (ms, lo, hi) in res.items():
        print(f"  {name:<26} {ms:8.3f} ms  (rounds {lo:.3f}..{hi:.3f})  "
              f"{flops / ms / 1e9:7.1f} TF/s  gqa/this {base / ms:.3f}")


def gqa_candidates(q, k, v, g, attn, sdpa):
    """name -> (forward fn, forward+backward fn). attn(q, k, v) is the
    project's call, sdpa(q, k, v) torch's with enable_gqa; the head
    dimension is 1."""
    G = q.shape[1] // k.shape[1]
    ke = k.detach().repeat_interleave(G, dim=1).requires_grad_(True)
    ve = v.detach().repeat_interleave(G, dim=1).requires_grad_(True)

    def expanded(q, k, v):
        return attn(q, k.repeat_interleave(G, dim=1),
                    v.repeat_interleave(G, dim=1))

    out = {}
    for name, f, kk, vv in (("gqa", attn, k, v),
                            ("expanded + passes", expanded, k, v),
                            ("expanded, kernels only", attn, ke, ve),
                            ("sdpa enable_gqa", sdpa, k, v)):
        if f is None:
            continue

        def fwd(f=f, kk=kk, vv=vv):
            return f(q, kk, vv)

        def fb(f=f, kk=kk, vv=vv):
            q.grad = kk.grad = vv.grad = None
            f(q, kk, vv).backward(g)

        out[name] = (fwd, fb)
    return out


def run_gqa(cands, fwd_flops, bwd_flops):
    report("forward", alternate({n: c[0] for n, c in cands.items()}),
           fwd_flops)
    report("forward + backward",
           alternate({n: c[1] for n, c in cands.items()}),
           fwd_flops + bwd_flops)


def gqa_path(B, H, Hk, S, D, causal, drop):
    from adapcc_amd.ops.attention import fa_supported, flash_attention

    assert H % Hk == 0 and Hk < H
    torch.manual_seed(0)

    def make(h):
        return torch.randn(B, h, S, D, device="cuda", dtype=torch.bfloat16,
                           requires_grad=True)

    q, k, v = make(H), make(Hk), make(Hk)
    g = torch.randn(B, H, S, D, device="cuda", dtype=torch.bfloat16)
    # a missing kernel is an error here, not a silent SDPA-vs-SDPA run
    assert fa_supported(q, k, v, causal, drop)
    fwd_flops = 4 * B * H * S * S * D / (2 if causal else 1)
    kv_bytes = 2 * B * Hk * S * D * 2
    print(f"B{B} H{H} Hk{Hk} (G={H // Hk}) S{S} D{D} causal={causal} "
          f"dropout={drop}")
    print(f"tile-loop FLOPs (as MHA): fwd {fwd_flops / 1e9:.1f} G, bwd "
          f"{2.5 * fwd_flops / 1e9:.1f} G; K+V bytes {kv_bytes / 2**20:.0f} "
          f"MiB (expanded: {kv_bytes * (H // Hk) / 2**20:.0f} MiB)")

    def attn(q, k, v):
        return flash_attention(q, k, v, causal=causal, dropout_p=drop)

    def sdpa(q, k, v):
        return torch.nn.functional.scaled_dot_product_attention(
            q, k, v, is_causal=causal, dropout_p=drop, enable_gqa=True)

    run_gqa(gqa_candidates(q, k, v, g, attn, sdpa), fwd_flops,
            2.5 * fwd_flops)


def gqa_varlen_path(H, Hk, D, drop, tokens=131072, S=1024):
    """The mixed lengths of varlen_path through flash_attention_varlen with
    Hk K/V heads; SDPA (dense block-diagonal mask) on the first 8192
    tokens' documents, where the GQA call is timed again."""
    from adapcc_amd.ops.attention import (fa_varlen_supported,
                                          flash_attention_varlen)

    assert H % Hk == 0 and Hk < H
    torch.manual_seed(0)

    def cu_of(lens):
        cu = torch.tensor([0] + lens, dtype=torch.int64).cumsum(0)
        return cu.to(torch.int32).cuda()

    def make(rows, h, grad=True):
        return torch.randn(rows, h, D, device="cuda", dtype=torch.bfloat16,
                           requires_grad=grad)

    def flops(lens):
        return sum(4 * H * n * n * D / 2 for n in lens)

    lens = mixed_lengths(tokens, 16, S, seed=0)
    sub, rows = [], 0
    for m in lens:
        if rows + m > 8192:
            break
        sub.append(m)
        rows += m
    for name, ls, with_sdpa in (("mixed", lens, False),
                                ("subset for SDPA", sub, True)):
        n = sum(ls)
        cu = cu_of(ls)
        q, k, v = make(n, H), make(n, Hk), make(n, Hk)
        g = make(n, H, grad=False)
        assert fa_varlen_supported(q, k, v, cu, True, drop)
        kv_bytes = 2 * n * Hk * D * 2
        print(f"{name}: {len(ls)} sequences, {n} tokens, H{H} Hk{Hk} D{D} "
              f"causal dropout={drop}; tile-loop FLOPs (as MHA, exact "
              f"triangles) fwd {flops(ls) / 1e9:.1f} G; K+V bytes "
              f"{kv_bytes / 2**20:.1f} MiB (expanded: "
              f"{kv_bytes * (H // Hk) / 2**20:.1f} MiB)")

        def attn(q, k, v, cu=cu):
            return flash_attention_varlen(q, k, v, cu, causal=True,
                                          dropout_p=drop)

        sdpa = None
        if with_sdpa:
            doc = torch.repeat_interleave(
                torch.arange(len(ls), device="cuda"),
                torch.tensor(ls, device="cuda"))
            mask = (doc.view(-1, 1) == doc.view(1, -1)).tril_()

            def sdpa(q, k, v, mask=mask):
                y = torch.nn.functional.scaled_dot_product_attention(
                    q.transpose(0, 1)[None], k.transpose(0, 1)[None],
                    v.transpose(0, 1)[None], attn_mask=mask,
                    dropout_p=drop, enable_gqa=True)
                return y[0].transpose(0, 1)

        run_gqa(gqa_candidates(q, k, v, g, attn, sdpa), flops(ls),
                2.5 * flops(ls))


def _fwd_and_fb(name, f, x, gy, iters):
    """Times f(x) and f(x).backward(gy); returns (fwd ms, fwd+bwd ms)."""
    fwd = bench(lambda: f(x), iters)

    def fb():
        x.grad = None
        f(x).backward(gy)

    both = bench(fb, iters)
    print(f"{name} fwd:  {fwd:7.3f} ms   f+b:  {both:7.3f} ms")
    return fwd, both


def mixed_lengths(tokens, lo, hi, seed):
    """Seeded lengths, log-uniform in [lo, hi], that sum to `tokens` (the
    last one cut to fit)."""
    gen = torch.Generator().manual_seed(seed)
    lens, left = [], tokens
    while left > 0:
        u = torch.rand((), generator=gen).item()
        span = math.log(hi) - math.log(lo)
        n = int(round(math.exp(math.log(lo) + u * span)))
        n = min(max(n, lo), hi, left)
        lens.append(n)
        left -= n
    return lens


def varlen_path(iters, drop=0.0, tokens=131072, H=12, D=64, S=1024):
    from adapcc_amd.ops.attention import (_varlen_plan,
                                          fa_qkv_varlen_supported,
                                          flash_attention_qkv,
                                          flash_attention_qkv_varlen)

    C = H * D
    torch.manual_seed(0)

    def cu_of(lens):
        cu = torch.tensor([0] + lens, dtype=torch.int64).cumsum(0)
        return cu.to(torch.int32).cuda()

    def make(rows):
        x = torch.randn(rows, 3 * C, device="cuda", dtype=torch.bfloat16,
                        requires_grad=True)
        return x, torch.randn(rows, C, device="cuda", dtype=torch.bfloat16)

    # 1. the cost of the mode: identical work, both ways
    n = tokens // S
    cu = cu_of([S] * n)
    x, gy = make(tokens)
    assert fa_qkv_varlen_supported(x, H, cu, drop)
    print(f"uniform: {n} sequences of {S}, H{H} D{D}, causal")
    vf, vb = _fwd_and_fb(
        "varlen packed      ",
        lambda t: flash_attention_qkv_varlen(t, H, cu, dropout_p=drop),
        x, gy, iters)
    x3 = x.detach().view(n, S, 3 * C).requires_grad_(True)
    ff, fb = _fwd_and_fb(
        "fixed-length packed",
        lambda t: flash_attention_qkv(t, H, dropout_p=drop),
        x3, gy.view(n, S, C), iters)
    print(f"varlen / fixed: fwd {vf / ff:.3f}  f+b {vb / fb:.3f}")

    # 2. what the mode is for: mixed lengths, no padding
    lens = mixed_lengths(tokens, 16, S, seed=0)
    n = len(lens)
    tiles = [-(-m // 128) for m in lens]
    full = (S // 128) * (S // 128 + 1) // 2
    work = sum(t * (t + 1) // 2 for t in tiles) / (n * full)
    print(f"mixed: {n} sequences, lengths {min(lens)}..{max(lens)}, "
          f"{tokens} tokens; padded to {S}: {n * S} tokens")
    print(f"work ratio (tile pairs, varlen / padded): {work:.3f}")
    cu = cu_of(lens)
    vf, vb = _fwd_and_fb(
        "varlen packed      ",
        lambda t: flash_attention_qkv_varlen(t, H, cu, dropout_p=drop),
        x, gy, iters)
    xp, gp = make(n * S)
    pf, pb = _fwd_and_fb(
        "padded fixed-length",
        lambda t: flash_attention_qkv(t, H, dropout_p=drop),
        xp.detach().view(n, S, 3 * C).requires_grad_(True),
        gp.view(n, S, C), iters)
    print(f"varlen / padded: fwd {vf / pf:.3f}  f+b {vb / pb:.3f}  "
          f"(work ratio {work:.3f})")
    del xp, gp

    # SDPA under the dense block-diagonal mask, at a size whose mask fits:
    # the first documents, up to 8192 tokens
    sub, rows = [], 0
    for m in lens:
        if rows + m > 8192:
            break
        sub.append(m)
        rows += m
    cu_s = cu_of(sub)
    xs, gs = make(rows)
    doc = torch.repeat_interleave(torch.arange(len(sub), device="cuda"),
                                  torch.tensor(sub, device="cuda"))
    mask = (doc.view(-1, 1) == doc.view(1, -1)).tril_()

    def sdpa(t):
        q, k, v = (u.view(1, rows, H, D).transpose(1, 2)
                   for u in t.split(C, dim=1))
        y = torch.nn.functional.scaled_dot_product_attention(
            q, k, v, attn_mask=mask, dropout_p=drop)
        return y.transpose(1, 2).reshape(rows, C)

    print(f"subset for SDPA: {len(sub)} sequences, {rows} tokens")
    sv = _fwd_and_fb(
        "varlen packed      ",
        lambda t: flash_attention_qkv_varlen(t, H, cu_s, dropout_p=drop),
        xs, gs, iters)
    sd = _fwd_and_fb("SDPA dense mask    ", sdpa, xs, gs, iters)
    print(f"varlen / SDPA: fwd {sv[0] / sd[0]:.3f}  f+b {sv[1] / sd[1]:.3f}")

    ms = bench(lambda: _varlen_plan(cu, tokens), 200)
    print(f"plan kernel alone ({n} sequences, with its output "
          f"allocation): {ms * 1e3:7.1f} us")


if __name__ == "__main__":
    main()
