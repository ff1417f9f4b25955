"""GPT2.generate: the cached decode steps against plain forwards."""

import pytest
import torch

from adapcc_amd.models.gpt2 import GPT2, GPT2Config

pytestmark = pytest.mark.gpu


def test_cached_logits_match_plain_forward():
    """After each generated token, the logits of the cached step equal those
    at the last position of model(idx_so_far), to 2e-2 of the logits' max
    magnitude. Logits, not token ids: an argmax tie in bf16 cannot flip it."""
    torch.manual_seed(0)
    cfg = GPT2Config(vocab_size=512, n_positions=64, n_embd=256, n_layer=2,
                     n_head=4, n_kv_head=2)
    model = GPT2(cfg).to("cuda", torch.bfloat16).eval()
    idx = torch.randint(0, cfg.vocab_size, (2, 20), device="cuda")
    T, new = idx.shape[1], 6
    out, logits = model.generate(idx, new, return_logits=True)
    assert out.shape == (2, T + new) and torch.equal(out[:, :T], idx)
    assert torch.equal(out[:, T:], logits.argmax(-1))
    with torch.no_grad():
        for i in range(new):
            want = model(out[:, :T + i])[0][:, -1].float()
            err = (logits[:, i].float() - want).abs().max()
            assert err <= 2e-2 * want.abs().max(), (i, float(err))
