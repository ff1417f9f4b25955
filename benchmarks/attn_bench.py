"""Flash-attention kernel timing: hand-written CDNA4 kernels vs torch SDPA.

Run on a GPU box:  python benchmarks/attn_bench.py [--shape gpt2|vit]
                                                   [--dropout P]

gpt2 (default): B64 H12 S1024 D64, causal. vit: B64 H12 S197 D64, non-causal
(ViT-base at 224 px). --dropout P times both paths with attention dropout at
rate P (ours inside the kernels, a fresh seed drawn per call as in training).
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
    ap.add_argument("--shape", choices=sorted(SHAPES), default="gpt2")
    ap.add_argument("--iters", type=int, default=None,
                    help="timed calls per figure (default 20; 200 for vit, "
                         "whose calls are ~10x shorter)")
    ap.add_argument("--dropout", type=float, default=0.0,
                    help="attention dropout rate for both paths")
    args = ap.parse_args()
    drop = args.dropout
    B, H, S, D, causal = SHAPES[args.shape]
    iters = args.iters or (200 if args.shape == "vit" else 20)

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


if __name__ == "__main__":
    main()
