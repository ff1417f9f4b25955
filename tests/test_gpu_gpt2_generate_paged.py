"""GPT2.generate over a paged KV cache (``kv_page_size``): the tokens of the
unpaged run. At these lengths neither call splits the keys, and paging
changes addresses only, so the logits are equal too."""

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


@pytest.mark.parametrize("ragged,chunk", [(False, None), (True, 7)])
def test_paged_generate_gives_the_unpaged_tokens(model_idx, ragged, chunk):
    model, idx = model_idx
    kw = dict(return_logits=True, prefill_chunk=chunk)
    if ragged:
        kw["prompt_lens"] = torch.tensor([T, 13], dtype=torch.int32,
                                         device="cuda")
    want_tok, want = model.generate(idx, NEW, **kw)
    got_tok, got = model.generate(idx, NEW, kv_page_size=16, **kw)
    assert torch.equal(got_tok, want_tok)
    assert torch.equal(got, want)
