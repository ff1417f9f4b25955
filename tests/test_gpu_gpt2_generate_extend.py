"""GPT2.generate with a chunked prefill and with ragged prompts: the logits
against the one-shot call and against each prompt generated alone, to 2e-2
of the logits' max magnitude. Logits, not token ids: an argmax tie in bf16
cannot flip the comparison."""

import pytest
import torch

from adapcc_amd.models.gpt2 import GPT2, GPT2Config

pytestmark = pytest.mark.gpu

T, NEW = 20, 6


@pytest.fixture(scope="module")
def model_idx():
    torch.manual_seed(0)
    cfg = GPT2Config(vocab_size=512, n_positions=64, n_embd=256, n_layer=2,
                     n_head=4, n_kv_head=2)
    model = GPT2(cfg).to("cuda", torch.bfloat16).eval()
    return model, torch.randint(0, cfg.vocab_size, (2, T), device="cuda")


def assert_logits_close(got, want):
    for i in range(NEW):
        err = (got[:, i].float() - want[:, i].float()).abs().max()
        assert err <= 2e-2 * want[:, i].float().abs().max(), (i, float(err))


def test_chunked_prefill_matches_one_shot(model_idx):
    model, idx = model_idx
    want_tok, want = model.generate(idx, NEW, return_logits=True)
    got_tok, got = model.generate(idx, NEW, return_logits=True,
                                  prefill_chunk=7)
    assert got_tok.shape == (2, T + NEW)
    assert torch.equal(got_tok[:, :T], idx)
    assert_logits_close(got, want)


@pytest.mark.parametrize("chunk", [None, 7])
def test_ragged_prompts_match_each_alone(model_idx, chunk):
    model, idx = model_idx
    lens = [T, 13]
    plens = torch.tensor(lens, dtype=torch.int32, device="cuda")
    got_tok, got = model.generate(idx, NEW, return_logits=True,
                                  prompt_lens=plens, prefill_chunk=chunk)
    assert got_tok.shape == (2, NEW) and plens.tolist() == lens
    for b, n in enumerate(lens):
        want = model.generate(idx[b:b + 1, :n], NEW, return_logits=True)[1]
        assert_logits_close(got[b:b + 1], want)
