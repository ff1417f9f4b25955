"""Flash-attention kernel timing: hand-written CDNA4 kernels vs torch SDPA.

Run on a GPU box:  python benchmarks/attn_bench.py
                       [--shape gpt2|vit|gpt2-d128|vit-d128|varlen]
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
    ap.add_argument("--shape", choices=sorted(SHAPES) + ["varlen"],
                    default="gpt2")
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
    args = ap.parse_args()
    drop = args.dropout
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
