"""GPT2.generate with e4m3 KV caches (``kv_cache_dtype``): every chunk and
step attends over the stored codes, so chunking, ragged prompts and paging
must not change the logits beyond 2e-2 of their max magnitude, the bound of
test_gpu_gpt2_generate_extend.py. fp8-cache logits are not held to bf16-cache
logits: that gap belongs to e4m3 at the chosen scales, not to this code."""

import pytest
import torch

from adapcc_amd.models.gpt2 import GPT2, GPT2Config

pytestmark = pytest.mark.gpu

T, NEW = 20, 6
F8 = dict(kv_cache_dtype=torch.float8_e4m3fn, return_logits=True)


@pytest.fixture(scope="module")
def model_idx():
    torch.manual_seed(0)
    cfg = GPT2Config(vocab_size=512, n_positions=64, n_embd=256, n_layer=2,
                     n_head=4, n_kv_head=2)
    model = GPT2(cfg).to("cuda", torch.bfloat16).eval()
    return model, torch.randint(0, cfg.vocab_size, (2, T), device="cuda")


@pytest.fixture(scope="module")
def one_shot(model_idx):
    model, idx = model_idx
    return model.generate(idx, NEW, **F8)[1]


def assert_logits_close(got, want):
    for i in range(NEW):
        err = (got[:, i].float() - want[:, i].float()).abs().max()
        assert err <= 2e-2 * want[:, i].float().abs().max(), (i, float(err))


@pytest.mark.parametrize("kw", [dict(prefill_chunk=7), dict(kv_page_size=16),
                                dict(prefill_chunk=7, kv_page_size=16)])
def test_chunked_and_paged_match_one_shot(model_idx, one_shot, kw):
    model, idx = model_idx
    tok, got = model.generate(idx, NEW, **F8, **kw)
    assert tok.shape == (2, T + NEW) and torch.isfinite(got).all()
    assert_logits_close(got, one_shot)


def test_ragged_prompts_match_each_alone(model_idx):
    model, idx = model_idx
    lens = [T, 13]
    plens = torch.tensor(lens, dtype=torch.int32, device="cuda")
    got = model.generate(idx, NEW, prompt_lens=plens, prefill_chunk=7,
                         **F8)[1]
    for b, n in enumerate(lens):
        want = model.generate(idx[b:b + 1, :n], NEW, **F8)[1]
        assert_logits_close(got[b:b + 1], want)


def test_scales_reach_the_kernels(model_idx, one_shot):
    """Per-layer, per-head scales that fit the values (not ones): the logits
    move, finite, and chunking still changes nothing."""
    model, idx = model_idx
    s = torch.tensor([[0.01, 0.02], [0.03, 0.015]], device="cuda")
    kw = dict(kv_scales=(s, s.flip(0)), **F8)
    want = model.generate(idx, NEW, **kw)[1]
    assert torch.isfinite(want).all() and not torch.equal(want, one_shot)
    assert_logits_close(model.generate(idx, NEW, prefill_chunk=7, **kw)[1],
                        want)


def test_bad_arguments_raise(model_idx):
    model, idx = model_idx
    with pytest.raises(ValueError):
        model.generate(idx, NEW, kv_cache_dtype=torch.float16)
    with pytest.raises(ValueError):
        model.generate(idx, NEW, kv_scales=(torch.ones(2, 2, device="cuda"),) * 2)
