"""Variable-length (packed sequences, cu_seqlens) attention, the parts that
need no GPU: the torch fallback against the per-sequence fp32 reference,
the packed entry point, the tile-map plan in Python with its clamping, the
argument checks, and GPT-2 on packed documents against the documents run
one by one."""

import math

import pytest
import torch

from attn_util import ref_attention_f32

H, D = 3, 64
SCALE = 1.0 / math.sqrt(D)
# 1: one key; 33: half-filled second 32-key half; 64: a whole 64-tile in a
# partial q tile; 65: a tile with one valid row; 128: aligned; 129: second
# tile of one row; 197: two tiles, ragged tail; 0: empty, in the middle;
# 256: two full tiles that start off a tile boundary
LENS = [1, 33, 64, 65, 128, 129, 197, 0, 256]
TOTAL = sum(LENS)


def cu_of(lens):
    cu = [0]
    for n in lens:
        cu.append(cu[-1] + n)
    return torch.tensor(cu, dtype=torch.int32)


def spans(lens):
    cu = cu_of(lens).tolist()
    return [(a, b) for a, b in zip(cu[:-1], cu[1:]) if b > a]


def per_sequence_reference(q, k, v, lens, causal):
    """ref_attention_f32 on each sequence by itself; [total,H,D] in, out."""
    out = torch.empty(q.shape, dtype=torch.float32)
    for a, b in spans(lens):
        qs, ks, vs = (t[a:b].transpose(0, 1)[None] for t in (q, k, v))
        out[a:b] = ref_attention_f32(qs, ks, vs, SCALE, causal)[0].transpose(
            0, 1)
    return out


def test_shape_constants():
    assert TOTAL == 873
    assert sum(-(-n // 128) for n in LENS) == 11


def test_not_supported_on_cpu():
    from adapcc_amd.ops.attention import (fa_qkv_varlen_supported,
                                          fa_varlen_supported)

    q = torch.randn(TOTAL, H, D, dtype=torch.bfloat16)
    cu = cu_of(LENS)
    assert not fa_varlen_supported(q, q, q, cu, True, 0.0)
    assert not fa_varlen_supported(q, q, q, cu, False, 0.0)
    qkv = torch.randn(TOTAL, 3 * H * D, dtype=torch.bfloat16)
    assert not fa_qkv_varlen_supported(qkv, H, cu, 0.0)
    assert not fa_qkv_varlen_supported(qkv, H, cu, 0.0, causal=False)


@pytest.mark.parametrize("causal", [True, False])
def test_fallback_matches_per_sequence_reference(causal):
    from adapcc_amd.ops.attention import flash_attention_varlen

    torch.manual_seed(0)
    q, k, v = (torch.randn(TOTAL, H, D).requires_grad_(True)
               for _ in range(3))
    g = torch.randn(TOTAL, H, D)
    o = flash_attention_varlen(q, k, v, cu_of(LENS), causal=causal)
    assert o.shape == (TOTAL, H, D)
    o.backward(g)

    qr, kr, vr = (t.detach().clone().requires_grad_(True) for t in (q, k, v))
    ref = per_sequence_reference(qr, kr, vr, LENS, causal)
    ref.backward(g)
    torch.testing.assert_close(o.detach(), ref.detach(), rtol=1e-5,
                               atol=1e-5)
    for name, got, want in (("dq", q.grad, qr.grad), ("dk", k.grad, kr.grad),
                            ("dv", v.grad, vr.grad)):
        torch.testing.assert_close(got, want, rtol=1e-5, atol=1e-5,
                                   msg=lambda m, n=name: f"{n}: {m}")


@pytest.mark.parametrize("causal", [True, False])
def test_packed_equals_strided(causal):
    from adapcc_amd.ops.attention import (flash_attention_qkv_varlen,
                                          flash_attention_varlen)

    C = H * D
    torch.manual_seed(1)
    qkv = torch.randn(TOTAL, 3 * C)
    g = torch.randn(TOTAL, C)
    cu = cu_of(LENS)

    x0 = qkv.clone().requires_grad_(True)
    y = flash_attention_qkv_varlen(x0, H, cu, causal=causal)
    assert y.shape == (TOTAL, C)
    y.backward(g)

    x1 = qkv.clone().requires_grad_(True)
    q, k, v = (t.view(TOTAL, H, D) for t in x1.split(C, dim=1))
    want = flash_attention_varlen(q, k, v, cu, causal=causal)
    want.backward(g.view(TOTAL, H, D))
    torch.testing.assert_close(y.detach(), want.detach().reshape(TOTAL, C),
                               rtol=0, atol=0)
    torch.testing.assert_close(x0.grad, x1.grad, rtol=0, atol=0)


# a decreasing pair, a last entry above total, a negative first entry
MALFORMED = [
    ([0, 300, 200, 500, 873], 873),
    ([0, 100, 400, 2000], 873),
    ([-50, 100, 300, 873], 873),
]


def test_plan_on_lens():
    from adapcc_amd.ops.attention import varlen_tile_map_reference

    tmap = varlen_tile_map_reference(cu_of(LENS), TOTAL)
    n_seqs = len(LENS)
    assert tmap.dtype == torch.int32
    assert tmap.shape == (TOTAL // 128 + n_seqs, 4)
    want = [(0, 0), (1, 0), (2, 0), (3, 0), (4, 0), (5, 0), (5, 1), (6, 0),
            (6, 1), (8, 0), (8, 1)]
    assert [tuple(r) for r in tmap[:11, :2].tolist()] == want
    assert (tmap[11:] == -1).all()
    cu = cu_of(LENS).tolist()
    for seq, tile, start, length in tmap[:11].tolist():
        assert start == cu[seq] and length == LENS[seq]
        assert tile * 128 < length


@pytest.mark.parametrize("cu,total", MALFORMED)
def test_plan_clamps_malformed(cu, total):
    from adapcc_amd.ops.attention import varlen_tile_map_reference

    n_seqs = len(cu) - 1
    tmap = varlen_tile_map_reference(torch.tensor(cu, dtype=torch.int32),
                                     total)
    assert tmap.shape == (total // 128 + n_seqs, 4)
    used = tmap[tmap[:, 0] >= 0]
    assert (tmap[len(used):] == -1).all()  # used entries first, then -1
    covered = torch.zeros(total, dtype=torch.int32)
    for seq, tile, start, length in used.tolist():
        assert 0 <= seq < n_seqs
        assert 0 <= start and length >= 1 and start + length <= total
        assert 0 <= tile * 128 < length
        lo = start + tile * 128
        covered[lo:min(lo + 128, start + length)] += 1
    # no row belongs to two tiles
    assert int(covered.max()) <= 1


def test_plan_expected_values_malformed():
    from adapcc_amd.ops.attention import varlen_tile_map_reference

    # decreasing pair: the running maximum makes sequence 1 empty and
    # starts sequence 2 at 300
    tmap = varlen_tile_map_reference(
        torch.tensor(MALFORMED[0][0], dtype=torch.int32), 873)
    rows = [tuple(r) for r in tmap.tolist() if r[0] >= 0]
    assert rows == [(0, 0, 0, 300), (0, 1, 0, 300), (0, 2, 0, 300),
                    (2, 0, 300, 200), (2, 1, 300, 200),
                    (3, 0, 500, 373), (3, 1, 500, 373), (3, 2, 500, 373)]


def test_argument_errors():
    from adapcc_amd.ops.attention import (flash_attention_qkv_varlen,
                                          flash_attention_varlen)

    q = torch.randn(TOTAL, H, D)
    cu = cu_of(LENS)
    with pytest.raises(ValueError):
        flash_attention_varlen(q, q, q, cu.long())
    with pytest.raises(ValueError):
        flash_attention_varlen(q, q, q, cu.view(2, -1))
    with pytest.raises(ValueError):
        flash_attention_varlen(q, q[:-1], q, cu)
    with pytest.raises(ValueError):
        flash_attention_varlen(q, q, q[:, :2], cu)
    qkv = torch.randn(TOTAL, 3 * H * D)
    with pytest.raises(ValueError):
        flash_attention_qkv_varlen(qkv, H, cu.long())
    with pytest.raises(ValueError):
        flash_attention_qkv_varlen(qkv, H, cu.view(2, -1))
    with pytest.raises(ValueError):
        flash_attention_qkv_varlen(qkv[:, :-1], H, cu)


# ---------------------------------------------------------------------------
# GPT-2 tiny on packed documents
# ---------------------------------------------------------------------------
DOCS = [5, 1, 130, 64]


@pytest.fixture(scope="module")
def tiny():
    from adapcc_amd.models.gpt2 import GPT2, GPT2Config

    torch.manual_seed(2)
    model = GPT2(GPT2Config.tiny()).eval()
    docs = [torch.randint(0, model.cfg.vocab_size, (n,)) for n in DOCS]
    return model, docs


def test_gpt2_packed_equals_per_document(tiny):
    model, docs = tiny
    idx = torch.cat(docs)[None]
    with torch.no_grad():
        packed, _ = model(idx, cu_seqlens=cu_of(DOCS))
        single = torch.cat([model(d[None])[0][0] for d in docs])
    assert packed.shape == (1, sum(DOCS), model.cfg.vocab_size)
    # logits are O(1); fp32 GEMM reassociation across different M is ~1e-5
    # at K <= 512; a leaked token or a wrong position id moves them > 1e-2
    torch.testing.assert_close(packed[0], single, rtol=1e-4, atol=1e-4)


def test_gpt2_packed_loss_is_token_weighted_mean(tiny):
    model, docs = tiny
    idx = torch.cat(docs)[None]
    # next-token targets; each document's last position has none
    tgt_docs = []
    for d in docs:
        t = torch.roll(d, -1)
        t[-1] = -100
        tgt_docs.append(t)
    with torch.no_grad():
        _, loss = model(idx, torch.cat(tgt_docs)[None],
                        cu_seqlens=cu_of(DOCS))
        num, den = 0.0, 0
        for d, t in zip(docs, tgt_docs):
            n = len(d) - 1
            if n == 0:
                continue  # a one-token document predicts nothing
            _, l = model(d[None], t[None])
            num, den = num + float(l) * n, den + n
    torch.testing.assert_close(float(loss), num / den, rtol=1e-4, atol=1e-4)


def test_gpt2_without_cu_seqlens_is_unchanged(tiny):
    model, _ = tiny
    torch.manual_seed(3)
    idx = torch.randint(0, model.cfg.vocab_size, (2, 64))
    with torch.no_grad():
        got, _ = model(idx)
        # the forward as it was before cu_seqlens existed
        x = model.drop(model.wte(idx) + model.wpe(torch.arange(64)))
        for block in model.h:
            x = x + block.attn(block.ln_1(x))
            x = x + block.mlp(block.ln_2(x))
        want = model.lm_head(model.ln_f(x))
    torch.testing.assert_close(got, want, rtol=0, atol=0)


@pytest.mark.parametrize("name,n_ptrs,n_strides", [("fa_fwd", 5, 12),
                                                   ("fa_bwd", 10, 24)])
def test_tile_map_needs_one_batch(name, n_ptrs, n_strides):
    """The variable-length mode of the launchers is B = 1, S = total: a
    tile map with B = 2 is refused on the host, before any launch, so the
    pointers are never followed."""
    core = pytest.importorskip("adapcc_amd._core")
    ptr = 4096
    B, S = 2, 256
    with pytest.raises(RuntimeError, match="tile map needs B == 1"):
        getattr(core, name)(*[ptr] * n_ptrs, B, H, S, [64] * n_strides,
                            SCALE, 0, True, tmap=ptr, n_seqs=2)
