"""Fused residual dropout + add + LayerNorm (csrc/lnorm.hip, ops/fused.py):
without dropout it is torch's add followed by FusedLayerNorm bit for bit, the
kernels' mask is the torch replica's bit for bit, forward and every gradient
match an fp32 reference that applies that mask, the seed rules, a captured
graph that redraws the seed on every replay, and GPT-2's routing.

Tolerances are those of test_gpu_fused_ln.py (rtol = atol = tol with tol 1e-5
for f32, 1e-2 for f16, 3e-2 for bf16; atol x5 for the input gradients and
x sqrt(rows) for dgamma/dbeta) with atol multiplied by 1/(1-p), as in
test_gpu_attention_dropout.py: x_new and both input gradients carry that
factor."""

import time

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

TOL = {torch.float32: 1e-5, torch.float16: 1e-2, torch.bfloat16: 3e-2}
DTYPES = list(TOL)
SEEDS = [1234, 0x7123456789ABCDEF]
EPS = 1e-5


def seed_tensor(value):
    return torch.tensor([value], dtype=torch.int64, device="cuda")


def replica(seed, rows, cols, p, site=0):
    from adapcc_amd.ops.fused import dropout_add_keep_mask_reference

    return dropout_add_keep_mask_reference(seed, rows, cols, p, site).cuda()


def inputs(rows, cols, dtype, seed=0):
    """h, residual, weight, bias (leaves) and the two output gradients."""
    torch.manual_seed(seed)

    def leaf(t):
        return t.to("cuda", dtype).requires_grad_(True)

    h, r = leaf(torch.randn(rows, cols)), leaf(torch.randn(rows, cols))
    w = leaf(torch.empty(cols).normal_(1.0, 0.2))
    b = leaf(torch.empty(cols).normal_(0.0, 0.2))
    gx = torch.randn(rows, cols).to("cuda", dtype)
    gy = torch.randn(rows, cols).to("cuda", dtype)
    return h, r, w, b, gx, gy


def op(h, r, w, b, p=0.0, seed=None, site=0):
    from adapcc_amd.ops.fused import (_dropadd_fusable,
                                      fused_dropout_add_layer_norm)

    assert _dropadd_fusable(h, r, w, b)
    return fused_dropout_add_layer_norm(h, r, w, b, EPS, p, seed, site)


def pick(pattern, x, y, gx, gy):
    """The outputs that receive a gradient, and those gradients."""
    outs = {"both": ((x, y), (gx, gy)), "y": ((y,), (gy,)),
            "x": ((x,), (gx,))}
    return outs[pattern]


def grads_of(pattern, x, y, gx, gy, leaves):
    outs, gs = pick(pattern, x, y, gx, gy)
    got = torch.autograd.grad(outs, leaves, gs, allow_unused=True)
    return [torch.zeros_like(t) if g is None else g
            for g, t in zip(got, leaves)]


def check_against_reference(h, r, w, b, gx, gy, keep, p, x_new, y, grads,
                            pattern="both"):
    """x_new, y and grads = (dh, dresidual, dgamma, dbeta) against fp32
    torch with the mask ``keep`` applied to h."""
    rows, cols = h.shape
    tol = TOL[h.dtype]
    f = 1.0 / (1.0 - p)
    leaves = [t.detach().float().requires_grad_(True) for t in (h, r, w, b)]
    hf, rf, wf, bf = leaves
    xr = rf + hf * keep.float() / (1.0 - p)
    yr = F.layer_norm(xr, (cols,), wf, bf, EPS)
    torch.testing.assert_close(x_new.float(), xr, rtol=tol, atol=tol * f,
                               msg=lambda m: f"x_new: {m}")
    torch.testing.assert_close(y.float(), yr, rtol=tol, atol=tol * f,
                               msg=lambda m: f"y: {m}")
    want = grads_of(pattern, xr, yr, gx.float(), gy.float(), leaves)
    wide = tol * max(1.0, rows ** 0.5) * f
    for name, got, ref, atol in zip(
            ("dh", "dresidual", "dgamma", "dbeta"), grads, want,
            (tol * 5 * f, tol * 5 * f, wide, wide)):
        assert got.dtype == h.dtype and torch.isfinite(got).all(), name
        torch.testing.assert_close(got.float(), ref, rtol=tol, atol=atol,
                                   msg=lambda m, n=name: f"{n}: {m}")
    assert (grads[0][~keep] == 0).all(), "dh where dropped"


# rows that do not fill a 4-wave block (1, 5, 333, 31); a row narrower than
# one wave of vectors (128), a partial second chunk (768), exact chunks
# (1024), the widest instantiation (4096)
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("rows,cols", [(1, 128), (5, 768), (333, 1024),
                                       (31, 4096)])
def test_without_dropout_is_add_then_fused_ln_bitwise(rows, cols, dtype):
    from adapcc_amd.ops.fused import FusedLayerNorm

    h, r, w, b, _, _ = inputs(rows, cols, dtype)
    x_new, y = op(h, r, w, b)
    torch.testing.assert_close(x_new, r + h, rtol=0, atol=0)
    ln = FusedLayerNorm(cols, eps=EPS).to("cuda", dtype)
    with torch.no_grad():
        ln.weight.copy_(w)
        ln.bias.copy_(b)
        torch.testing.assert_close(y, ln(x_new.detach()), rtol=0, atol=0)


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("seed", SEEDS)
@pytest.mark.parametrize("p", [0.1, 0.5])
@pytest.mark.parametrize("rows,cols", [(5, 768), (333, 128)])
def test_mask_is_the_replica(rows, cols, p, seed, dtype):
    from adapcc_amd.ops.fused import FusedLayerNorm

    _, r, w, b, _, _ = inputs(rows, cols, dtype)
    keep = replica(seed, rows, cols, p)
    s = seed_tensor(seed)
    with torch.no_grad():
        ones, zeros = torch.ones_like(r), torch.zeros_like(r)
        x_new, _ = op(ones, zeros, w, b, p, s)
        assert torch.equal(x_new != 0, keep)
        kept = torch.tensor(1.0 / (1.0 - p)).float().to(dtype)
        assert (x_new[keep] == kept).all()

        h = torch.randn_like(r)
        x_new, y = op(h, r, w, b, p, s)
        assert torch.equal(x_new[~keep], r[~keep])
        assert not torch.equal(x_new[keep], r[keep])
        # and y is the LayerNorm of the x_new it returns, dropout or not
        ln = FusedLayerNorm(cols, eps=EPS).to("cuda", dtype)
        ln.weight.copy_(w)
        ln.bias.copy_(b)
        torch.testing.assert_close(y, ln(x_new), rtol=0, atol=0)
        # another site under the same seed is another mask
        x_site, _ = op(ones, zeros, w, b, p, s, site=1)
        assert torch.equal(x_site != 0, replica(seed, rows, cols, p, 1))
        assert not torch.equal(x_site, x_new)


# every shape with both outputs used; (4100, 128) makes the backward's
# grid-stride loop iterate (its grid stops at 1024 blocks of 4 rows)
CASES = [(rows, cols, dtype, 0.1, "both")
         for rows, cols in [(1, 128), (5, 768), (333, 1024), (31, 4096),
                            (333, 128)]
         for dtype in DTYPES]
CASES += [(rows, cols, dtype, 0.1, pattern)
          for rows, cols in [(5, 768), (333, 1024)]
          for dtype in DTYPES for pattern in ("y", "x")]
CASES += [(5, 768, torch.bfloat16, 0.5, "both"),
          (333, 128, torch.float32, 0.5, "both"),
          (4100, 128, torch.bfloat16, 0.1, "both")]


@pytest.mark.parametrize("rows,cols,dtype,p,pattern", CASES)
def test_fwd_bwd_matches_reference(rows, cols, dtype, p, pattern):
    h, r, w, b, gx, gy = inputs(rows, cols, dtype)
    x_new, y = op(h, r, w, b, p, seed_tensor(SEEDS[1]), site=2)
    grads = grads_of(pattern, x_new, y, gx, gy, (h, r, w, b))
    keep = replica(SEEDS[1], rows, cols, p, site=2)
    check_against_reference(h, r, w, b, gx, gy, keep, p, x_new.detach(),
                            y.detach(), grads, pattern)


@pytest.mark.parametrize("pattern", ["both", "y", "x"])
def test_fwd_bwd_without_dropout_matches_reference(pattern):
    rows, cols = 333, 768
    h, r, w, b, gx, gy = inputs(rows, cols, torch.bfloat16)
    x_new, y = op(h, r, w, b)
    grads = grads_of(pattern, x_new, y, gx, gy, (h, r, w, b))
    assert torch.equal(grads[0], grads[1])  # dh is dresidual at p = 0
    keep = torch.ones(rows, cols, dtype=torch.bool, device="cuda")
    check_against_reference(h, r, w, b, gx, gy, keep, 0.0, x_new.detach(),
                            y.detach(), grads, pattern)


def _run(problem, seed=None, p=0.1):
    """x_new, y and the four gradients of one problem (from inputs())."""
    h, r, w, b, gx, gy = problem
    x_new, y = op(h, r, w, b, p, seed)
    return [x_new.detach(), y.detach()] + grads_of("both", x_new, y, gx, gy,
                                                   (h, r, w, b))


def test_seed_from_torch_generator():
    """No explicit seed: it comes from torch's generator on the device, so
    torch.manual_seed reproduces a call and the next call draws anew."""
    problem = inputs(64, 256, torch.bfloat16, seed=10)
    torch.manual_seed(7)
    a = _run(problem)
    torch.manual_seed(7)
    b = _run(problem)
    c = _run(problem)  # no reseed: a new mask
    assert all(torch.equal(x, y) for x, y in zip(a, b))
    for i in (0, 1, 2):  # x_new, y, dh
        assert not torch.equal(b[i], c[i])


def test_explicit_seed_and_bad_seeds():
    problem = inputs(64, 256, torch.bfloat16, seed=10)
    a, b, c = (_run(problem, seed_tensor(s)) for s in (5, 5, 6))
    assert all(torch.equal(x, y) for x, y in zip(a, b))
    assert not torch.equal(a[0], c[0])
    h, r, w, b, _, _ = inputs(4, 128, torch.bfloat16)
    with pytest.raises(ValueError):  # on the CPU
        op(h, r, w, b, 0.1, torch.tensor([1], dtype=torch.int64))
    with pytest.raises(ValueError):  # not int64
        op(h, r, w, b, 0.1, torch.zeros(1, device="cuda"))


def test_graph_capture_redraws_seed():
    """seed.random_() + forward + backward in one captured graph: every
    replay reads the seed it has just drawn, in both kernels."""
    rows, cols, p = 37, 768, 0.1
    h, r, w, b, gx, gy = inputs(rows, cols, torch.bfloat16, seed=40)
    seed = torch.zeros(1, dtype=torch.int64, device="cuda")

    def step():
        seed.random_()
        x_new, y = op(h, r, w, b, p, seed)
        return (x_new, y) + torch.autograd.grad((x_new, y), (h, r, w, b),
                                                (gx, gy))

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

    seeds, masks = [], []
    for _ in range(2):
        graph.replay()
        torch.cuda.synchronize()
        seeds.append(int(seed.item()))
        keep = replica(seeds[-1], rows, cols, p)
        masks.append(outs[0].detach() != r.detach())
        check_against_reference(h, r, w, b, gx, gy, keep, p,
                                outs[0].detach(), outs[1].detach(), outs[2:])
    assert seeds[0] != seeds[1]
    assert not torch.equal(masks[0], masks[1])


def _gpt2(resid_dropout):
    from adapcc_amd.models.gpt2 import GPT2, GPT2Config

    cfg = GPT2Config(vocab_size=256, n_positions=128, n_embd=128, n_layer=2,
                     n_head=2, dropout=0.0, resid_dropout=resid_dropout)
    torch.manual_seed(50)
    model = GPT2(cfg).to("cuda").to(torch.bfloat16).train()
    data = torch.randint(0, cfg.vocab_size, (2, 129), device="cuda")
    return model, data[:, :-1], data[:, 1:].contiguous()


def _count_launches(monkeypatch):
    from adapcc_amd.ops import fused

    calls = []
    real = fused._launch_dropadd_fwd

    def fwd(*a, **kw):
        calls.append(a[9])  # dropout_p
        return real(*a, **kw)

    monkeypatch.setattr(fused, "_launch_dropadd_fwd", fwd)
    return calls


def _step(model, x, t):
    model.zero_grad(set_to_none=True)
    torch.manual_seed(60)
    _, loss = model(x, t)
    loss.backward()
    return loss.detach(), {n: p.grad.clone()
                           for n, p in model.named_parameters()}


def test_gpt2_routes_resid_dropout_to_kernels(monkeypatch):
    from adapcc_amd.ops import fused

    model, x, t = _gpt2(0.1)
    calls = _count_launches(monkeypatch)
    loss, grads = _step(model, x, t)
    assert calls == [0.1] * (2 * model.cfg.n_layer)
    assert torch.isfinite(loss)
    assert len(grads) == len(list(model.parameters()))
    assert all(torch.isfinite(g).all() for g in grads.values())

    # the same weights and seeds through the composed fallback
    del calls[:]
    monkeypatch.setattr(fused, "_dropadd_fusable", lambda *a: False)
    loss_c, grads_c = _step(model, x, t)
    assert calls == []
    tol, f = TOL[torch.bfloat16], 1.0 / (1.0 - 0.1)
    torch.testing.assert_close(loss, loss_c, rtol=tol, atol=tol * f)
    for name, g in grads.items():
        torch.testing.assert_close(g.float(), grads_c[name].float(),
                                   rtol=tol, atol=tol * f,
                                   msg=lambda m, n=name: f"{n}: {m}")


def test_gpt2_without_resid_dropout_keeps_its_path(monkeypatch):
    model, x, t = _gpt2(0.0)
    calls = _count_launches(monkeypatch)
    loss, _ = _step(model, x, t)
    assert calls == [] and torch.isfinite(loss)
    # and with it set, eval mode does not use it either
    model, x, t = _gpt2(0.1)
    with torch.no_grad():
        model.eval()(x, t)
    assert calls == []


def test_dropout_add_ln_bench():
    """Wall-clock sanity at the GPT-2 shape, forward + backward, against
    F.dropout + add + FusedLayerNorm (printed for the profile log; the only
    bound is "never catastrophically slower")."""
    from adapcc_amd.ops.fused import (FusedLayerNorm,
                                      fused_dropout_add_layer_norm)

    rows, cols, p = 65536, 768, 0.1
    dt = torch.bfloat16
    h = torch.randn(rows, cols, device="cuda", dtype=dt, requires_grad=True)
    r = torch.randn(rows, cols, device="cuda", dtype=dt, requires_grad=True)
    gx = torch.randn(rows, cols, device="cuda", dtype=dt)
    gy = torch.randn(rows, cols, device="cuda", dtype=dt)
    ln = FusedLayerNorm(cols).to("cuda", dt)

    def fused():
        return fused_dropout_add_layer_norm(h, r, ln.weight, ln.bias, ln.eps,
                                            p)

    def composed():
        x = r + F.dropout(h, p, training=True)
        return x, ln(x)

    def bench(fn):
        def once():
            x, y = fn()
            torch.autograd.backward((x, y), (gx, gy))
            h.grad = r.grad = ln.weight.grad = ln.bias.grad = None

        for _ in range(3):
            once()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(10):
            once()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) / 10 * 1000

    t_fused = bench(fused)
    t_composed = bench(composed)
    print(f"\ndropout+add+LN fwd+bwd {rows}x{cols} bf16 p={p}: fused "
          f"{t_fused:.3f} ms vs composed {t_composed:.3f} ms "
          f"({t_composed / t_fused:.2f}x)")
    assert t_fused < t_composed * 1.5  # never catastrophically slower
