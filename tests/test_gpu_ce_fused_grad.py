"""Cross-entropy with the gradient from the forward's one read of the logits
(csrc/ce.hip ce_fwd_grad, ops/fused.py FUSE_CE_GRAD) against the two-kernel
path on the same inputs: per-row loss and lse, the mean, and logits.grad for
an upstream gradient of 1.0 (the saved dlogits) and of 0.5 (the recompute
branch of ce_bwd) are the same bits.

Widths: 50257 / 50258 (rows start misaligned / aligned, 25 vectors a thread),
300 (fewer vectors than threads), 7 (no whole vector in most rows), and the
widest instantiation's cap and one past it (the two-kernel fallback)."""

import pytest
import torch

pytestmark = pytest.mark.gpu

IGNORE = -100
DTYPES = [torch.bfloat16, torch.float32]
ROWS = [1, 3, 64]
COLS = [7, 300, 50257, 50258, "cap", "cap+1"]


def _core_dt(dtype):
    import adapcc_amd._core as c

    return c, {torch.float32: c.DTYPE_F32, torch.bfloat16: c.DTYPE_BF16}[dtype]


def _cols(cols, dtype):
    c, dt = _core_dt(dtype)
    cap = c.ce_fused_max_cols(dt)
    return {"cap": cap, "cap+1": cap + 1}.get(cols, cols)


def _inputs(rows, cols, dtype, ignore, salt=0):
    g = torch.Generator(device="cuda").manual_seed(
        rows * 100003 + cols + salt * 7919)
    logits = (torch.randn(rows, cols, device="cuda", generator=g) * 3.0
              ).to(dtype)
    targets = torch.randint(0, cols, (rows,), device="cuda", generator=g)
    if ignore == "all":
        targets.fill_(IGNORE)
    elif rows > 1:
        targets[1::3] = IGNORE  # some rows ignored, row 0 kept
    return logits, targets


def _kernels(logits, targets, fused):
    """Per-row loss and lse, and dlogits at gscale 1 / n_valid, straight from
    the kernels: ce_fwd + ce_bwd, or ce_fwd_grad."""
    c, dt = _core_dt(logits.dtype)
    rows, cols = logits.shape
    loss = torch.empty(rows, dtype=torch.float32, device="cuda")
    lse = torch.empty_like(loss)
    dlogits = torch.empty_like(logits)
    n_valid = (targets != IGNORE).sum().float().clamp(min=1)
    g0 = (torch.ones_like(n_valid) / n_valid).reshape(1)
    s = torch.cuda.current_stream().cuda_stream
    if fused:
        c.ce_fwd_grad(dt, logits.data_ptr(), targets.data_ptr(),
                      g0.data_ptr(), loss.data_ptr(), lse.data_ptr(),
                      dlogits.data_ptr(), rows, cols, IGNORE, s)
    else:
        c.ce_fwd(dt, logits.data_ptr(), targets.data_ptr(), loss.data_ptr(),
                 lse.data_ptr(), rows, cols, IGNORE, s)
        c.ce_bwd(dt, logits.data_ptr(), targets.data_ptr(), lse.data_ptr(),
                 g0.data_ptr(), 0, dlogits.data_ptr(), rows, cols, IGNORE, s)
    return loss, lse, dlogits


def _autograd(logits, targets, upstream):
    from adapcc_amd.ops.fused import fused_cross_entropy

    x = logits.detach().clone().requires_grad_(True)
    mean = fused_cross_entropy(x, targets, IGNORE)
    (mean * upstream).backward()
    return mean.detach(), x.grad


def _check(rows, cols, dtype, ignore, monkeypatch):
    from adapcc_amd.ops import fused

    cols = _cols(cols, dtype)
    logits, targets = _inputs(rows, cols, dtype, ignore)
    c, dt = _core_dt(dtype)
    want = {}
    monkeypatch.setattr(fused, "FUSE_CE_GRAD", False)
    for up in (1.0, 0.5):
        want[up] = _autograd(logits, targets, up)
    monkeypatch.setattr(fused, "FUSE_CE_GRAD", True)
    for up in (1.0, 0.5):
        mean, grad = _autograd(logits, targets, up)
        assert torch.equal(mean, want[up][0]), f"mean, upstream {up}"
        assert torch.equal(grad, want[up][1]), f"logits.grad, upstream {up}"
    assert torch.isfinite(want[1.0][0])
    if ignore == "all":
        assert not want[1.0][1].any() and float(want[1.0][0]) == 0.0

    if cols <= c.ce_fused_max_cols(dt):
        loss0, lse0, d0 = _kernels(logits, targets, fused=False)
        loss1, lse1, d1 = _kernels(logits, targets, fused=True)
        assert torch.equal(loss1, loss0), "per-row loss"
        assert torch.equal(lse1, lse0), "lse"
        assert torch.equal(d1, d0), "dlogits"
        # and these are what the wrapper hands out
        assert torch.equal(d1, want[1.0][1])
        # a sanity anchor outside the two kernels
        ref = torch.logsumexp(logits.double(), dim=1)
        torch.testing.assert_close(lse1.double(), ref, rtol=1e-5, atol=1e-5)


@pytest.mark.parametrize("dtype", DTYPES, ids=["bf16", "f32"])
@pytest.mark.parametrize("cols", COLS)
@pytest.mark.parametrize("rows", ROWS)
def test_bits_equal_two_kernel_path(rows, cols, dtype, monkeypatch):
    _check(rows, cols, dtype, "some", monkeypatch)


@pytest.mark.parametrize("dtype", DTYPES, ids=["bf16", "f32"])
def test_all_rows_ignored(dtype, monkeypatch):
    _check(3, 300, dtype, "all", monkeypatch)


def test_past_the_cap_takes_the_two_kernels(monkeypatch):
    """One past the cap must not reach ce_fwd_grad (the wrapper's choice; the
    launcher refuses it too)."""
    import adapcc_amd._core as c
    from adapcc_amd.ops import fused

    class Spy:
        def __init__(self):
            self.fused_calls = 0

        def __getattr__(self, name):
            if name == "ce_fwd_grad":
                self.fused_calls += 1
            return getattr(c, name)

    spy = Spy()
    assert fused._core() is c  # loaded, dtype table filled
    monkeypatch.setattr(fused, "_CORE", spy)
    cap = c.ce_fused_max_cols(c.DTYPE_BF16)
    for cols, n in ((cap, 1), (cap + 1, 1)):
        logits, targets = _inputs(3, cols, torch.bfloat16, "some")
        _autograd(logits, targets, 1.0)
        assert spy.fused_calls == n
    with pytest.raises(RuntimeError):
        _kernels(*_inputs(1, cap + 8, torch.bfloat16, "some"), fused=True)


def test_no_grad_forward_allocates_no_gradient(monkeypatch):
    import adapcc_amd._core as c
    from adapcc_amd.ops import fused
    from adapcc_amd.ops.fused import fused_cross_entropy

    logits, targets = _inputs(64, 50257, torch.bfloat16, "some")
    want, _ = _autograd(logits, targets, 1.0)

    called = []

    class Spy:
        def __getattr__(self, name):
            called.append(name)
            return getattr(c, name)

    assert fused._core() is c
    monkeypatch.setattr(fused, "_CORE", Spy())
    x = logits.detach().clone().requires_grad_(True)
    torch.cuda.synchronize()
    before = torch.cuda.memory_allocated()
    with torch.no_grad():
        got = fused_cross_entropy(x, targets, IGNORE)
    torch.cuda.synchronize()
    grown = torch.cuda.memory_allocated() - before
    assert torch.equal(got, want)
    assert "ce_fwd" in called and "ce_fwd_grad" not in called
    assert not got.requires_grad
    assert grown < logits.numel() * logits.element_size() // 2
    # logits that want no gradient take the plain forward as well
    del called[:]
    got = fused_cross_entropy(logits, targets, IGNORE)
    assert torch.equal(got, want)
    assert "ce_fwd_grad" not in called


def test_second_backward_recomputes(monkeypatch):
    """retain_graph: the saved dlogits may have become the leaf's .grad, so a
    second backward computes into a fresh tensor."""
    from adapcc_amd.ops.fused import fused_cross_entropy

    logits, targets = _inputs(3, 300, torch.bfloat16, "some")
    _, want = _autograd(logits, targets, 1.0)
    x = logits.detach().clone().requires_grad_(True)
    mean = fused_cross_entropy(x, targets, IGNORE)
    mean.backward(retain_graph=True)
    assert torch.equal(x.grad, want)
    mean.backward()
    assert torch.equal(x.grad, want + want)


def test_graph_capture_and_replay(monkeypatch):
    from adapcc_amd.ops import fused
    from adapcc_amd.ops.fused import fused_cross_entropy

    rows, cols = 64, 50257
    batches = [_inputs(rows, cols, torch.bfloat16, "some", salt=i)
               for i in range(3)]
    monkeypatch.setattr(fused, "FUSE_CE_GRAD", False)
    want = [_autograd(lg, tg, 1.0) for lg, tg in batches]
    monkeypatch.setattr(fused, "FUSE_CE_GRAD", True)

    x = batches[0][0].clone().requires_grad_(True)
    t = batches[0][1].clone()

    def step():
        x.grad = None
        mean = fused_cross_entropy(x, t, IGNORE)
        mean.backward()
        return mean.detach(), x.grad

    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        step()
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        mean, grad = step()
    for (lg, tg), (wm, wg) in zip(batches[1:], want[1:]):
        with torch.no_grad():
            x.copy_(lg)
            t.copy_(tg)
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(mean, wm)
        assert torch.equal(grad, wg)
