"""Residual dropout + add + LayerNorm, the parts that need no GPU: the torch
replica of the kernels' keep(seed, site, row, col) mask (ops/fused.py,
csrc/attn_drop.h) is the attention replica made rectangular and is
statistically a Bernoulli(1-p) field, the plain-torch composition that CPU
inputs take has the op's semantics, and GPT-2's ``resid_dropout`` acts in
training only.

Keep counts are compared with their binomial expectation: 4 sigma for the
whole mask, 5 sigma for each row and each column (columns only where there
are at least 128 rows to count). For exactly these seeds, rates and shapes
the definition's worst values are |z| 1.9, 3.9 and 3.8 (printed per case)."""

import math

import pytest
import torch
import torch.nn.functional as F

SEEDS = [1234, 0x7123456789ABCDEF]


def _replica(seed, rows, cols, p, site=0):
    from adapcc_amd.ops.fused import dropout_add_keep_mask_reference

    return dropout_add_keep_mask_reference(seed, rows, cols, p, site)


def _worst_z(count, n, pi):
    """count: tensor of counts, each out of n trials of probability pi."""
    sd = math.sqrt(n * pi * (1.0 - pi))
    return ((count.double() - n * pi).abs() / sd).max().item()


def test_replica_equals_attention_replica_on_a_square():
    from adapcc_amd.ops.attention import dropout_keep_mask_reference

    S = 64
    got = _replica(1234, S, S, 0.1)
    assert got.shape == (S, S) and got.dtype == torch.bool
    assert torch.equal(got, dropout_keep_mask_reference(1234, 1, 1, S,
                                                        0.1)[0, 0])
    # a tensor seed is the same seed
    assert torch.equal(got, _replica(torch.tensor([1234]), S, S, 0.1))


@pytest.mark.parametrize("seed", SEEDS)
@pytest.mark.parametrize("p", [0.1, 0.5])
@pytest.mark.parametrize("rows,cols", [(5, 768), (333, 128), (333, 1024),
                                       (4100, 128)])
def test_replica_statistics(rows, cols, p, seed):
    m = _replica(seed, rows, cols, p)
    assert m.shape == (rows, cols) and m.dtype == torch.bool
    k = 1.0 - p
    z_all = _worst_z(m.sum(), m.numel(), k)
    z_row = _worst_z(m.sum(dim=1), cols, k)
    z_col = _worst_z(m.sum(dim=0), rows, k)
    print(f"total {z_all:.2f} rows {z_row:.2f} columns {z_col:.2f} sigma")
    assert z_all <= 4.0
    assert z_row <= 5.0
    if rows >= 128:
        assert z_col <= 5.0


@pytest.mark.parametrize("seed", SEEDS)
def test_sites_draw_independent_masks(seed):
    """Two independent Bernoulli(1/2) masks agree on an element with
    probability 1/2; the count is held to 5 binomial sigma."""
    rows, cols = 333, 1024
    a = _replica(seed, rows, cols, 0.5, site=0)
    b = _replica(seed, rows, cols, 0.5, site=1)
    z = _worst_z((a == b).sum(), a.numel(), 0.5)
    print(f"agreement {z:.2f} sigma")
    assert z <= 5.0


def _params(cols, dtype=torch.float32):
    torch.manual_seed(3)
    w = torch.empty(cols, dtype=dtype).normal_(1.0, 0.2).requires_grad_(True)
    b = torch.empty(cols, dtype=dtype).normal_(0.0, 0.2).requires_grad_(True)
    return w, b


def test_fallback_without_dropout_is_add_then_layer_norm():
    from adapcc_amd.ops.fused import fused_dropout_add_layer_norm

    rows, cols = 5, 96  # a width no kernel takes, and the CPU besides
    torch.manual_seed(0)
    h = torch.randn(rows, cols, requires_grad=True)
    r = torch.randn(rows, cols, requires_grad=True)
    w, b = _params(cols)
    gx, gy = torch.randn(rows, cols), torch.randn(rows, cols)

    state = torch.get_rng_state()
    x_new, y = fused_dropout_add_layer_norm(h, r, w, b, 1e-5)
    assert torch.equal(torch.get_rng_state(), state)  # no seed drawn
    assert torch.equal(x_new, r + h)
    assert torch.equal(y, F.layer_norm(r + h, (cols,), w, b, 1e-5))
    got = torch.autograd.grad((x_new, y), (h, r, w, b), (gx, gy))

    xr = r + h
    want = torch.autograd.grad((xr, F.layer_norm(xr, (cols,), w, b, 1e-5)),
                               (h, r, w, b), (gx, gy))
    for g, e in zip(got, want):
        assert torch.equal(g, e)


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_fallback_with_explicit_seed_matches_replica_reference(dtype):
    from adapcc_amd.ops.fused import fused_dropout_add_layer_norm

    rows, cols, p, site = 7, 128, 0.5, 3
    torch.manual_seed(1)
    h = torch.randn(2, rows, cols).to(dtype)
    r = torch.randn(2, rows, cols).to(dtype)
    w, b = _params(cols, dtype)
    seed = torch.tensor([SEEDS[1]], dtype=torch.int64)

    x1, y1 = fused_dropout_add_layer_norm(h, r, w, b, 1e-5, p, seed, site)
    x2, y2 = fused_dropout_add_layer_norm(h, r, w, b, 1e-5, p, seed, site)
    assert torch.equal(x1, x2) and torch.equal(y1, y2)
    assert x1.dtype == dtype and x1.shape == h.shape

    # rows are flattened: row index = b * rows + t
    keep = _replica(seed, 2 * rows, cols, p, site).view(2, rows, cols)
    want = (r.float() + h.float() * keep / (1.0 - p)).to(dtype)
    assert torch.equal(x1, want)
    assert torch.equal(x1[~keep], r[~keep])
    assert torch.equal(y1, F.layer_norm(want, (cols,), w, b, 1e-5))
    # another site, another mask
    x3, _ = fused_dropout_add_layer_norm(h, r, w, b, 1e-5, p, seed, site + 1)
    assert not torch.equal(x1, x3)


def test_fallback_draws_its_seed_from_torch_generator():
    from adapcc_amd.ops.fused import fused_dropout_add_layer_norm

    h, r = torch.randn(4, 64), torch.randn(4, 64)
    w, b = _params(64)
    torch.manual_seed(9)
    a = fused_dropout_add_layer_norm(h, r, w, b, dropout_p=0.3)[0]
    torch.manual_seed(9)
    c = fused_dropout_add_layer_norm(h, r, w, b, dropout_p=0.3)[0]
    d = fused_dropout_add_layer_norm(h, r, w, b, dropout_p=0.3)[0]
    assert torch.equal(a, c)
    assert not torch.equal(c, d)


def test_validation():
    from adapcc_amd.ops.fused import fused_dropout_add_layer_norm

    h, r = torch.randn(4, 64), torch.randn(4, 64)
    w, b = _params(64)
    for p in (1.0, -0.1, 1.5):
        with pytest.raises(ValueError):
            fused_dropout_add_layer_norm(h, r, w, b, dropout_p=p)
    with pytest.raises(ValueError):  # wrong dtype
        fused_dropout_add_layer_norm(h, r, w, b, dropout_p=0.1,
                                     dropout_seed=torch.zeros(1))
    with pytest.raises(ValueError):  # two elements
        fused_dropout_add_layer_norm(
            h, r, w, b, dropout_p=0.1,
            dropout_seed=torch.zeros(2, dtype=torch.int64))
    with pytest.raises(ValueError):
        fused_dropout_add_layer_norm(h, r, w, b, dropout_p=0.1, site=-1)
    with pytest.raises(ValueError):
        fused_dropout_add_layer_norm(h, r[:2], w, b)


def _gpt2(resid_dropout):
    from adapcc_amd.models.gpt2 import GPT2, GPT2Config

    cfg = GPT2Config(vocab_size=128, n_positions=32, n_embd=32, n_layer=2,
                     n_head=2, resid_dropout=resid_dropout)
    torch.manual_seed(11)
    return GPT2(cfg)


def test_gpt2_resid_dropout_is_off_in_eval():
    from adapcc_amd.models.gpt2 import GPT2Config

    assert GPT2Config().resid_dropout == 0.0
    plain, dropped = _gpt2(0.0), _gpt2(0.3)
    assert list(plain.state_dict()) == list(dropped.state_dict())
    for a, b in zip(plain.state_dict().values(),
                    dropped.state_dict().values()):
        assert torch.equal(a, b)
    idx = torch.randint(0, 128, (2, 16))
    with torch.no_grad():
        want, _ = plain.eval()(idx)
        got, _ = dropped.eval()(idx)
    torch.testing.assert_close(got, want, rtol=0, atol=0)


def test_gpt2_resid_dropout_acts_in_training():
    model = _gpt2(0.3)
    idx = torch.randint(0, 128, (2, 16))
    with torch.no_grad():
        quiet, _ = model.eval()(idx)
    model.train()
    torch.manual_seed(5)
    a, loss = model(idx, idx)
    torch.manual_seed(5)
    b, _ = model(idx, idx)
    c, _ = model(idx, idx)
    assert torch.equal(a, b)
    assert not torch.equal(b, c)
    assert not torch.equal(a, quiet)
    loss.backward()
    assert all(torch.isfinite(p.grad).all() for p in model.parameters())
