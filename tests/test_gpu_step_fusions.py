"""One GPT-2 training step in bf16 with the pass fusions of ops/fused.py all
on against all off (FUSE_CE_GRAD, FUSE_GELU_BIAS_GRAD, FUSE_COLSUM_FOLD):
n_embd 128, 2 layers, vocab 257 so the cross-entropy rows are odd-width.

Loss, logits and every parameter gradient are the same bits, except the
gradients whose summation order the fusions change: c_fc.bias (summed inside
the GeLU backward) and the LayerNorm weights and biases (folded by
colsum_fold). Those are held to test_gpu_dropout_add_ln.py's bf16 tolerance
(rtol = atol = 3e-2)."""

import pytest
import torch

pytestmark = pytest.mark.gpu

SWITCHES = ("FUSE_CE_GRAD", "FUSE_GELU_BIAS_GRAD", "FUSE_COLSUM_FOLD")
TOL = 3e-2


def _reordered(name):
    return (name.endswith("c_fc.bias") or ".ln_1." in name
            or ".ln_2." in name or name.startswith("ln_f."))


def _step(model, x, t):
    model.zero_grad(set_to_none=True)
    torch.manual_seed(60)
    logits, loss = model(x, t)
    loss.backward()
    return (loss.detach().clone(), logits.detach().clone(),
            {n: p.grad.clone() for n, p in model.named_parameters()})


@pytest.mark.parametrize("resid_dropout", [0.0, 0.1])
def test_step_with_fusions_equals_step_without(resid_dropout, monkeypatch):
    from adapcc_amd.models.gpt2 import GPT2, GPT2Config
    from adapcc_amd.ops import fused

    cfg = GPT2Config(vocab_size=257, n_positions=128, n_embd=128, n_layer=2,
                     n_head=2, dropout=0.0, resid_dropout=resid_dropout)
    torch.manual_seed(50)
    model = GPT2(cfg).to("cuda").to(torch.bfloat16).train()
    data = torch.randint(0, cfg.vocab_size, (2, 129), device="cuda")
    x, t = data[:, :-1], data[:, 1:].contiguous()
    t[0, 5] = -100  # an ignored row

    launched = []
    real = fused._core()

    class Spy:
        def __getattr__(self, name):
            launched.append(name)
            return getattr(real, name)

    monkeypatch.setattr(fused, "_CORE", Spy())
    for s in SWITCHES:
        assert getattr(fused, s) is True  # the defaults
    loss1, logits1, g1 = _step(model, x, t)
    on = set(launched)
    del launched[:]
    for s in SWITCHES:
        monkeypatch.setattr(fused, s, False)
    loss0, logits0, g0 = _step(model, x, t)
    off = set(launched)

    assert {"ce_fwd_grad", "gelu_bwd_bias", "colsum_fold"} <= on
    assert not {"ce_fwd_grad", "gelu_bwd_bias", "colsum_fold"} & off
    assert torch.isfinite(loss0)
    assert torch.equal(loss1, loss0)
    assert torch.equal(logits1, logits0)
    assert set(g1) == set(g0)
    names = [n for n in g0 if _reordered(n)]
    assert len(names) == 2 + 4 * 2 + 2  # c_fc.bias x2, ln_1/ln_2 x2, ln_f
    for n in g0:
        if _reordered(n):
            torch.testing.assert_close(g1[n].float(), g0[n].float(),
                                       rtol=TOL, atol=TOL,
                                       msg=lambda m, n=n: f"{n}: {m}")
        else:
            assert torch.equal(g1[n], g0[n]), n
