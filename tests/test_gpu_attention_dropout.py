"""Attention dropout inside the hand-written CDNA4 flash attention
(csrc/attn.hip, csrc/attn_drop.h, ops/attention.py): the kernels' mask is the
torch replica's bit for bit, forward and the three gradients match an fp32
reference that applies that mask after the softmax, lse ignores dropout, the
packed entry equals the composed one, the seed rules, a captured graph that
redraws the seed on every replay, and the models' routing.

Tolerances are those of test_gpu_attention_noncausal.py (rtol = atol = 2e-2
forward, 5e-2 gradients) with atol multiplied by 1/(1-p): every output and
gradient carries that factor."""

import math

import pytest
import torch

from attn_util import record_launches, ref_attention_f32

pytestmark = pytest.mark.gpu

B, H, D = 2, 3, 64
SCALE = 1.0 / math.sqrt(D)
SEED_HI = 0x7123456789ABCDEF  # high word set


def rand(S, seed, b=B, h=H):
    torch.manual_seed(seed)
    return torch.randn(b, h, S, D, device="cuda", dtype=torch.bfloat16)


def seed_tensor(value):
    return torch.tensor([value], dtype=torch.int64, device="cuda")


def ref_dropout_attention_f32(q, k, v, scale, causal, keep, p):
    """fp32 attention with the [B,H,S,S] bool mask ``keep`` and 1/(1-p)
    applied to the probabilities after the softmax."""
    qf, kf, vf = q.float(), k.float(), v.float()
    s = torch.matmul(qf, kf.transpose(-1, -2)) * scale
    if causal:
        S = q.shape[-2]
        future = torch.ones(S, S, dtype=torch.bool, device=q.device).triu(1)
        s = s.masked_fill(future, float("-inf"))
    prob = torch.softmax(s, dim=-1)
    prob = prob * keep.to(prob.dtype) / (1.0 - p)
    return torch.matmul(prob, vf)


def replica(seed, b, h, S, p):
    from adapcc_amd.ops.attention import dropout_keep_mask_reference

    return dropout_keep_mask_reference(seed, b, h, S, p).cuda()


def check_against_reference(q, k, v, g, o, grads, causal, keep, p):
    f = 1.0 / (1.0 - p)
    ref = ref_dropout_attention_f32(q, k, v, SCALE, causal, keep, p)
    torch.testing.assert_close(o.float(), ref, rtol=2e-2, atol=2e-2 * f)
    qr, kr, vr = (t.detach().float().requires_grad_(True) for t in (q, k, v))
    ref_dropout_attention_f32(qr, kr, vr, SCALE, causal, keep,
                              p).backward(g.float())
    for name, got, want in zip(("dq", "dk", "dv"), grads,
                               (qr.grad, kr.grad, vr.grad)):
        torch.testing.assert_close(got.float(), want, rtol=5e-2,
                                   atol=5e-2 * f,
                                   msg=lambda m, n=name: f"{n}: {m}")


@pytest.mark.parametrize("seed", [1234, SEED_HI])
@pytest.mark.parametrize("p", [0.1, 0.5])
@pytest.mark.parametrize("shape", [(2, 3, 197), (1, 2, 256)])
def test_mask_kernel_equals_replica(shape, p, seed):
    from adapcc_amd.ops.attention import fa_dropout_mask

    b, h, S = shape
    got = fa_dropout_mask(seed_tensor(seed), b, h, S, p)
    assert got.is_cuda and got.dtype == torch.bool
    assert got.shape == (b, h, S, S)
    assert torch.equal(got, replica(seed, b, h, S, p))


# causal S % 128 == 0; non-causal aligned (128), ragged over two
# workgroups (197), ragged with a one-row tile (65), one key (1)
CASES = [(True, 128, 0.1), (True, 256, 0.1), (False, 128, 0.1),
         (False, 197, 0.1), (False, 65, 0.1), (False, 1, 0.1),
         (True, 256, 0.5), (False, 197, 0.5)]


@pytest.mark.parametrize("causal,S,p", CASES)
def test_fwd_bwd_matches_reference(causal, S, p):
    from adapcc_amd.ops.attention import fa_supported, flash_attention

    q = rand(S, 0).requires_grad_(True)
    k = rand(S, 1).requires_grad_(True)
    v = rand(S, 2).requires_grad_(True)
    g = rand(S, 3)
    assert fa_supported(q, k, v, causal, p)

    o = flash_attention(q, k, v, causal=causal, dropout_p=p,
                        dropout_seed=seed_tensor(SEED_HI))
    o.backward(g)
    keep = replica(SEED_HI, B, H, S, p)
    check_against_reference(q, k, v, g, o.detach(),
                            (q.grad, k.grad, v.grad), causal, keep, p)


@pytest.mark.parametrize("causal,S", [(True, 256), (False, 197)])
def test_lse_ignores_dropout(causal, S):
    from adapcc_amd.ops.attention import _fa_forward_lse

    q, k, v = rand(S, 4), rand(S, 5), rand(S, 6)
    o0, lse0 = _fa_forward_lse(q, k, v, SCALE, causal)
    o1, lse1 = _fa_forward_lse(q, k, v, SCALE, causal, dropout_p=0.1,
                               seed=seed_tensor(1234))
    torch.testing.assert_close(lse1, lse0, rtol=0, atol=1e-4)
    assert not torch.equal(o0, o1)


@pytest.mark.parametrize("causal,T", [(True, 128), (False, 197)])
def test_packed_equals_composed_bitwise(causal, T):
    from adapcc_amd.ops.attention import (_attention_qkv_composed,
                                          fa_qkv_supported,
                                          flash_attention_qkv)

    C = H * D
    torch.manual_seed(30)
    qkv = torch.randn(B, T, 3 * C, device="cuda", dtype=torch.bfloat16)
    g = torch.randn(B, T, C, device="cuda", dtype=torch.bfloat16)
    s = seed_tensor(99)
    assert fa_qkv_supported(qkv, H, 0.1, causal=causal)

    x0 = qkv.clone().requires_grad_(True)
    want = _attention_qkv_composed(x0, H, dropout_p=0.1, causal=causal,
                                   dropout_seed=s)
    want.backward(g)
    x1 = qkv.clone().requires_grad_(True)
    y = flash_attention_qkv(x1, H, dropout_p=0.1, causal=causal,
                            dropout_seed=s)
    y.backward(g)
    torch.testing.assert_close(y.detach(), want.detach(), rtol=0, atol=0)
    assert torch.isfinite(x1.grad).all()
    torch.testing.assert_close(x1.grad, x0.grad, rtol=0, atol=0)
    # and dropout did act
    y0 = flash_attention_qkv(qkv, H, causal=causal)
    assert not torch.equal(y.detach(), y0)


def _run(S, causal, seed=None, p=0.1):
    """o, dq, dk, dv of one seeded problem."""
    from adapcc_amd.ops.attention import flash_attention

    q = rand(S, 10).requires_grad_(True)
    k = rand(S, 11).requires_grad_(True)
    v = rand(S, 12).requires_grad_(True)
    g = rand(S, 13)
    o = flash_attention(q, k, v, causal=causal, dropout_p=p,
                        dropout_seed=seed)
    o.backward(g)
    return [o.detach(), q.grad, k.grad, v.grad]


def _same(a, b):
    return all(torch.equal(x, y) for x, y in zip(a, b))


@pytest.mark.parametrize("causal,S", [(True, 128), (False, 65)])
def test_explicit_seed(causal, S):
    a = _run(S, causal, seed_tensor(5))
    b = _run(S, causal, seed_tensor(5))
    c = _run(S, causal, seed_tensor(6))
    assert _same(a, b)
    for x, y in zip(a, c):
        assert not torch.equal(x, y)


def test_seed_from_torch_generator():
    """No explicit seed: it comes from torch's generator on the device, so
    torch.manual_seed reproduces a call and the next call draws anew."""
    from adapcc_amd.ops.attention import flash_attention

    q, k, v, g = (rand(128, 20 + i) for i in range(4))

    def run():
        leaves = [t.clone().requires_grad_(True) for t in (q, k, v)]
        o = flash_attention(*leaves, dropout_p=0.1)
        o.backward(g)
        return [o.detach()] + [t.grad for t in leaves]

    torch.manual_seed(7)
    a = run()
    torch.manual_seed(7)
    b = run()
    c = run()  # no reseed: a new mask
    assert _same(a, b)
    for x, y in zip(b, c):
        assert not torch.equal(x, y)


def test_bad_seed_refused():
    from adapcc_amd.ops.attention import flash_attention

    q, k, v = rand(128, 20), rand(128, 21), rand(128, 22)
    with pytest.raises(ValueError):
        flash_attention(q, k, v, dropout_p=0.1,
                        dropout_seed=torch.tensor([1], dtype=torch.int64))
    with pytest.raises(ValueError):
        flash_attention(q, k, v, dropout_p=0.1,
                        dropout_seed=torch.zeros(1, device="cuda"))


def test_graph_capture_redraws_seed():
    """seed.random_() + forward + backward in one captured graph: every
    replay reads the seed it has just drawn, in all three kernels."""
    from adapcc_amd.ops.attention import flash_attention

    b, h, S, p = 1, 2, 128, 0.1
    q = rand(S, 40, b, h).requires_grad_(True)
    k = rand(S, 41, b, h).requires_grad_(True)
    v = rand(S, 42, b, h).requires_grad_(True)
    g = rand(S, 43, b, h)
    seed = torch.zeros(1, dtype=torch.int64, device="cuda")

    def step():
        seed.random_()
        o = flash_attention(q, k, v, causal=True, dropout_p=p,
                            dropout_seed=seed)
        return (o,) + torch.autograd.grad(o, (q, k, v), g)

    for _ in range(2):  # allocator warmup on a side stream
        s = torch.cuda.Stream()
        s.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(s):
            step()
        torch.cuda.current_stream().wait_stream(s)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        outs = step()

    seeds = []
    for _ in range(2):
        graph.replay()
        torch.cuda.synchronize()
        seeds.append(int(seed.item()))
        keep = replica(seeds[-1], b, h, S, p)
        check_against_reference(q, k, v, g, outs[0].detach(), outs[1:],
                                True, keep, p)
    assert seeds[0] != seeds[1]


def test_gpt2_routes_dropout_to_kernels(monkeypatch):
    from adapcc_amd.models.gpt2 import GPT2, GPT2Config

    cfg = GPT2Config(vocab_size=256, n_positions=128, n_embd=128, n_layer=1,
                     n_head=2, dropout=0.1)
    torch.manual_seed(50)
    model = GPT2(cfg).to("cuda").to(torch.bfloat16)
    data = torch.randint(0, cfg.vocab_size, (2, 129), device="cuda")
    x, t = data[:, :-1], data[:, 1:].contiguous()
    calls = record_launches(monkeypatch)

    model.train()
    _, loss = model(x, t)
    loss.backward()
    assert calls == [("fwd", True, 0.1, False), ("bwd", True, 0.1, False)]
    assert torch.isfinite(loss)
    assert all(torch.isfinite(p.grad).all() for p in model.parameters()
               if p.grad is not None)

    del calls[:]
    model.eval()
    with torch.no_grad():
        model(x, t)
    assert calls == [("fwd", True, 0.0, False)]


def test_vit_routes_dropout_to_kernels(monkeypatch):
    from adapcc_amd.models.vit import ViT, ViTConfig

    cfg = ViTConfig(image_size=32, patch_size=8, num_classes=10, dim=128,
                    depth=1, heads=2, mlp_dim=256, attn_dropout=0.1)
    torch.manual_seed(51)
    model = ViT(cfg).to("cuda").to(torch.bfloat16)
    x = torch.randn(2, 3, 32, 32, device="cuda", dtype=torch.bfloat16)
    calls = record_launches(monkeypatch)

    model.train()
    model(x).float().sum().backward()
    assert calls == [("fwd", False, 0.1, False), ("bwd", False, 0.1, False)]

    del calls[:]
    model.eval()
    with torch.no_grad():
        model(x)
    assert calls == [("fwd", False, 0.0, False)]


def test_reference_helper_reduces_to_plain_attention():
    """The helper above with an all-ones mask at p = 0 is the shared fp32
    reference, so the two cannot drift apart."""
    S = 65
    q, k, v = rand(S, 60), rand(S, 61), rand(S, 62)
    keep = torch.ones(B, H, S, S, dtype=torch.bool, device="cuda")
    for causal in (True, False):
        torch.testing.assert_close(
            ref_dropout_attention_f32(q, k, v, SCALE, causal, keep, 0.0),
            ref_attention_f32(q, k, v, SCALE, causal), rtol=0, atol=0)
