"""Variable-length (packed sequences, cu_seqlens) flash attention on the
GPU: bits against the fixed-length kernels run one sequence at a time,
numerics against fp32, isolation of the sequences from each other and of
the buffers from their surroundings, the plan kernel, dropout, the packed
entry point, graph replay with a refilled cu_seqlens, and GPT-2."""

import math

import pytest
import torch
from torch.utils._python_dispatch import TorchDispatchMode

from attn_util import record_launches, ref_attention_f32

pytestmark = pytest.mark.gpu

H, D = 3, 64
C = H * D
SCALE = 1.0 / math.sqrt(D)
# see tests/test_attention_varlen_cpu.py for what each length exercises
LENS = [1, 33, 64, 65, 128, 129, 197, 0, 256]
TOTAL = sum(LENS)  # 873, 11 q tiles
MID = 5            # the middle sequence test 3 poisons (129 rows)
# a decreasing pair, a last entry above total, a negative first entry
MALFORMED = [
    ([0, 300, 200, 500, 873], 873),
    ([0, 100, 400, 2000], 873),
    ([-50, 100, 300, 873], 873),
]


def cu_of(lens, device="cuda"):
    cu = [0]
    for n in lens:
        cu.append(cu[-1] + n)
    return torch.tensor(cu, dtype=torch.int32, device=device)


def spans(lens):
    cu = cu_of(lens, "cpu").tolist()
    return [(i, a, b) for i, (a, b) in enumerate(zip(cu[:-1], cu[1:]))
            if b > a]


def rand(seed, total=TOTAL):
    torch.manual_seed(seed)
    return torch.randn(total, H, D, device="cuda", dtype=torch.bfloat16)


def seq4(t, a, b):
    """Rows a..b-1 of a [total,H,D] tensor as a [1,H,len,D] batch."""
    return t[a:b].transpose(0, 1)[None]


def run_varlen(q, k, v, g, lens, causal, **kw):
    """o, lse, dq, dk, dv of one packed forward + backward."""
    from adapcc_amd.ops.attention import (_fa_forward_lse, _rows4,
                                          _varlen_plan, fa_varlen_supported,
                                          flash_attention_varlen)

    cu = cu_of(lens)
    assert fa_varlen_supported(q, k, v, cu, causal, kw.get("dropout_p", 0.0))
    qr, kr, vr = (t.detach().clone().requires_grad_(True) for t in (q, k, v))
    o = flash_attention_varlen(qr, kr, vr, cu, causal=causal, **kw)
    o.backward(g)
    seed = kw.get("dropout_seed")
    o2, lse = _fa_forward_lse(
        _rows4(q), _rows4(k), _rows4(v), SCALE, causal,
        dropout_p=kw.get("dropout_p", 0.0), seed=seed,
        tmap=_varlen_plan(cu, q.shape[0]))
    o2, lse = o2[0].transpose(0, 1), lse[0]
    # (a poisoned sequence holds NaN in both, on purpose)
    torch.testing.assert_close(o.detach(), o2, rtol=0, atol=0,
                               equal_nan=True)
    return {"o": o.detach(), "lse": lse, "dq": qr.grad, "dk": kr.grad,
            "dv": vr.grad}


@pytest.fixture(scope="module")
def data():
    return {"q": rand(0), "k": rand(1), "v": rand(2), "g": rand(3)}


@pytest.fixture(scope="module")
def packed(data):
    """The packed LENS batch, forward and backward, both modes, once."""
    return {causal: run_varlen(data["q"], data["k"], data["v"], data["g"],
                               LENS, causal)
            for causal in (True, False)}


def assert_bits(got, want, what):
    torch.testing.assert_close(got, want, rtol=0, atol=0,
                               msg=lambda m: f"{what}: {m}")


# ---------------------------------------------------------------------------
# 1. bits against the fixed-length kernels
# ---------------------------------------------------------------------------
def test_noncausal_bits_equal_fixed_length(data, packed):
    from adapcc_amd.ops.attention import _fa_forward_lse, flash_attention

    got = packed[False]
    for i, a, b in spans(LENS):
        q, k, v = (seq4(data[n], a, b).detach().clone().requires_grad_(True)
                   for n in ("q", "k", "v"))
        o = flash_attention(q, k, v, causal=False)
        o.backward(seq4(data["g"], a, b))
        _, lse = _fa_forward_lse(q.detach(), k.detach(), v.detach(), SCALE,
                                 False)
        assert_bits(seq4(got["o"], a, b), o.detach(), f"o seq {i}")
        assert_bits(got["lse"][:, a:b], lse[0], f"lse seq {i}")
        for n, t in (("dq", q), ("dk", k), ("dv", v)):
            assert_bits(seq4(got[n], a, b), t.grad, f"{n} seq {i}")


def test_causal_bits_equal_fixed_length_zero_padded(data, packed):
    from adapcc_amd.ops.attention import _fa_forward_lse, flash_attention

    got = packed[True]
    for i, a, b in spans(LENS):
        n = b - a
        P = -(-n // 128) * 128

        def pad(t):
            x = torch.zeros(1, H, P, D, device="cuda", dtype=torch.bfloat16)
            x[:, :, :n] = seq4(t, a, b)
            return x

        q, k, v = (pad(data[m]).requires_grad_(True)
                   for m in ("q", "k", "v"))
        o = flash_attention(q, k, v, causal=True)
        o.backward(pad(data["g"]))  # dO zero in the padding
        _, lse = _fa_forward_lse(q.detach(), k.detach(), v.detach(), SCALE,
                                 True)
        assert_bits(seq4(got["o"], a, b), o.detach()[:, :, :n], f"o seq {i}")
        assert_bits(got["lse"][:, a:b], lse[0, :, :n], f"lse seq {i}")
        for m, t in (("dq", q), ("dk", k), ("dv", v)):
            assert_bits(seq4(got[m], a, b), t.grad[:, :, :n], f"{m} seq {i}")


# ---------------------------------------------------------------------------
# 2. numerics against fp32
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("causal", [True, False])
def test_matches_fp32_reference(data, packed, causal):
    got = packed[causal]
    for i, a, b in spans(LENS):
        q, k, v = (seq4(data[n], a, b).float().requires_grad_(True)
                   for n in ("q", "k", "v"))
        ref = ref_attention_f32(q, k, v, SCALE, causal)
        ref.backward(seq4(data["g"], a, b).float())
        torch.testing.assert_close(seq4(got["o"], a, b).float(), ref.detach(),
                                   rtol=2e-2, atol=2e-2,
                                   msg=lambda m: f"o seq {i}: {m}")
        for n, t in (("dq", q), ("dk", k), ("dv", v)):
            torch.testing.assert_close(
                seq4(got[n], a, b).float(), t.grad, rtol=5e-2, atol=5e-2,
                msg=lambda m, n=n: f"{n} seq {i}: {m}")
    for t in got.values():
        assert torch.isfinite(t.float()).all()


@pytest.mark.parametrize("causal", [True, False])
def test_lse_counts_keys(data, causal):
    from adapcc_amd.ops.attention import _fa_forward_lse, _varlen_plan

    q = torch.zeros_like(data["q"])
    _, lse = _fa_forward_lse(q, data["k"], data["v"], SCALE, causal,
                             tmap=_varlen_plan(cu_of(LENS), TOTAL))
    lse = lse[0]
    want = torch.empty(TOTAL, device="cuda")
    for _, a, b in spans(LENS):
        n = b - a
        count = (torch.arange(1, n + 1, device="cuda").float() if causal
                 else torch.full((n,), float(n), device="cuda"))
        want[a:b] = count.log()
    torch.testing.assert_close(lse, want.expand(H, TOTAL), rtol=0, atol=1e-4)


# ---------------------------------------------------------------------------
# 3. no leak across sequences
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("causal", [True, False])
def test_nan_sequence_stays_inside(data, packed, causal):
    _, a, b = [s for s in spans(LENS) if s[0] == MID][0]
    k, v = data["k"].clone(), data["v"].clone()
    k[a:b] = float("nan")
    v[a:b] = float("nan")
    got = run_varlen(data["q"], k, v, data["g"], LENS, causal)
    clean = packed[causal]
    for name in ("o", "dq", "dk", "dv"):
        for lo, hi in ((0, a), (b, TOTAL)):
            assert torch.isfinite(got[name][lo:hi].float()).all(), name
            assert_bits(got[name][lo:hi], clean[name][lo:hi], name)
    for lo, hi in ((0, a), (b, TOTAL)):
        assert torch.isfinite(got["lse"][:, lo:hi]).all()
        assert_bits(got["lse"][:, lo:hi], clean["lse"][:, lo:hi], "lse")


# ---------------------------------------------------------------------------
# 4. nothing outside [0, total) is touched
# ---------------------------------------------------------------------------
GUARD = 130  # rows in front of and behind every buffer


def _guarded(seed, fill):
    """A [GUARD + TOTAL + GUARD, H, D] buffer filled with ``fill`` and its
    middle TOTAL rows, seeded."""
    buf = torch.full((TOTAL + 2 * GUARD, H, D), fill, device="cuda",
                     dtype=torch.bfloat16)
    view = buf[GUARD:GUARD + TOTAL]
    if seed is not None:
        view.copy_(rand(seed))
    return buf, view


def _guarded_rows(fill):
    """The same for an fp32 [H, TOTAL] buffer, guards at both ends."""
    n = H * TOTAL
    buf = torch.full((n + 512,), fill, device="cuda", dtype=torch.float32)
    return buf, buf[256:256 + n].view(H, TOTAL)


def _run_raw(causal, in_fill):
    """Forward + backward through the launch helpers on guarded buffers.
    Returns the result views and the (buffer, view) pairs of the outputs."""
    from adapcc_amd.ops.attention import (_launch_bwd, _launch_fwd, _rows4,
                                          _varlen_plan)

    sent = 1234.0  # exact in bf16 and fp32
    cu = cu_of(LENS)
    q, k, v, do = (_guarded(10 + i, in_fill)[1] for i in range(4))
    outs = [_guarded(None, sent) for _ in range(4)]  # o, dq, dk, dv
    rows = [_guarded_rows(sent) for _ in range(2)]   # lse, delta
    o, dq, dk, dv = (view for _, view in outs)
    lse, delta = (view for _, view in rows)
    tmap = _varlen_plan(cu, TOTAL)
    _launch_fwd(_rows4(q), _rows4(k), _rows4(v), _rows4(o), lse, SCALE,
                causal=causal, tmap=tmap)
    _launch_bwd(_rows4(q), _rows4(k), _rows4(v), _rows4(o), _rows4(do), lse,
                _rows4(dq), _rows4(dk), _rows4(dv), SCALE, causal=causal,
                delta=delta, tmap=tmap)
    torch.cuda.synchronize()
    return [o, lse, delta, dq, dk, dv], outs + rows


@pytest.mark.parametrize("causal", [True, False])
def test_guard_rows_untouched_and_unread(causal):
    sent = 1234.0
    results = []
    for in_fill in (float("nan"), 0.0):
        views, pairs = _run_raw(causal, in_fill)
        for buf, view in pairs:
            assert torch.isfinite(view.float()).all()
            flat, inner = buf.view(-1), view.reshape(-1)
            lead = (view.data_ptr() - buf.data_ptr()) // buf.element_size()
            guards = (flat[:lead], flat[lead + inner.numel():])
            for guard in guards:
                assert guard.numel() > 0
                assert (guard == sent).all()
        results.append([t.clone() for t in views])
    # NaN in the input guards changed no bit
    for got, want in zip(*results):
        assert_bits(got, want, "input guard dependence")


# ---------------------------------------------------------------------------
# 5. the plan kernel
# ---------------------------------------------------------------------------
@pytest.mark.parametrize(
    "cu,total",
    [(cu_of(LENS, "cpu").tolist(), TOTAL)] + MALFORMED
    # 699 sequences of 3 rows and an empty last one: several per thread
    + [(list(range(0, 3 * 700, 3)) + [2097], 2097)])
def test_plan_kernel_equals_reference(cu, total):
    from adapcc_amd.ops.attention import (_varlen_plan,
                                          varlen_tile_map_reference)

    cu_t = torch.tensor(cu, dtype=torch.int32)
    got = _varlen_plan(cu_t.cuda(), total)
    want = varlen_tile_map_reference(cu_t, total)
    assert got.dtype == torch.int32 and got.shape == want.shape
    assert torch.equal(got.cpu(), want)


# ---------------------------------------------------------------------------
# 6. dropout
# ---------------------------------------------------------------------------
SEED = 0x7123456789ABCDEF  # high word set


def seed_tensor(value):
    return torch.tensor([value], dtype=torch.int64, device="cuda")


def ref_dropout_attention_f32(q, k, v, scale, causal, keep, p):
    """fp32 attention with the bool mask ``keep`` and 1/(1-p) applied to
    the probabilities after the softmax."""
    s = torch.matmul(q, k.transpose(-1, -2)) * scale
    if causal:
        S = q.shape[-2]
        future = torch.ones(S, S, dtype=torch.bool, device=q.device).triu(1)
        s = s.masked_fill(future, float("-inf"))
    prob = torch.softmax(s, dim=-1)
    prob = prob * keep.to(prob.dtype) / (1.0 - p)
    return torch.matmul(prob, v)


@pytest.mark.parametrize("p", [0.1, 0.5])
@pytest.mark.parametrize("causal", [True, False])
def test_dropout_matches_reference(data, packed, causal, p):
    from adapcc_amd.ops.attention import dropout_keep_mask_reference

    got = run_varlen(data["q"], data["k"], data["v"], data["g"], LENS,
                     causal, dropout_p=p, dropout_seed=seed_tensor(SEED))
    keep_all = dropout_keep_mask_reference(SEED, len(LENS), H, 256, p).cuda()
    f = 1.0 / (1.0 - p)
    for i, a, b in spans(LENS):
        n = b - a
        keep = keep_all[i, :, :n, :n][None]
        q, k, v = (seq4(data[m], a, b).float().requires_grad_(True)
                   for m in ("q", "k", "v"))
        ref = ref_dropout_attention_f32(q, k, v, SCALE, causal, keep, p)
        ref.backward(seq4(data["g"], a, b).float())
        torch.testing.assert_close(seq4(got["o"], a, b).float(), ref.detach(),
                                   rtol=2e-2, atol=2e-2 * f,
                                   msg=lambda m: f"o seq {i}: {m}")
        for m, t in (("dq", q), ("dk", k), ("dv", v)):
            torch.testing.assert_close(
                seq4(got[m], a, b).float(), t.grad, rtol=5e-2, atol=5e-2 * f,
                msg=lambda msg, m=m: f"{m} seq {i}: {msg}")
    # dropout does not enter lse
    assert_bits(got["lse"], packed[causal]["lse"], "lse")

    again = run_varlen(data["q"], data["k"], data["v"], data["g"], LENS,
                       causal, dropout_p=p, dropout_seed=seed_tensor(SEED))
    other = run_varlen(data["q"], data["k"], data["v"], data["g"], LENS,
                       causal, dropout_p=p, dropout_seed=seed_tensor(1234))
    for name in ("o", "dq", "dk", "dv"):
        assert_bits(again[name], got[name], name)
        assert not torch.equal(other[name], got[name]), name


# ---------------------------------------------------------------------------
# 7. the packed entry point
# ---------------------------------------------------------------------------
class _RecordOps(TorchDispatchMode):
    def __init__(self):
        super().__init__()
        self.names = []

    def __torch_dispatch__(self, func, types, args=(), kwargs=None):
        self.names.append(str(func))
        return func(*args, **(kwargs or {}))


@pytest.mark.parametrize("causal", [True, False])
def test_packed_equals_views_bitwise_no_copies(causal):
    from adapcc_amd.ops.attention import (fa_qkv_varlen_supported,
                                          flash_attention_qkv_varlen,
                                          flash_attention_varlen)

    torch.manual_seed(30)
    qkv = torch.randn(TOTAL, 3 * C, device="cuda", dtype=torch.bfloat16)
    g = torch.randn(TOTAL, C, device="cuda", dtype=torch.bfloat16)
    cu = cu_of(LENS)
    assert fa_qkv_varlen_supported(qkv, H, cu, 0.0, causal=causal)

    x0 = qkv.clone().requires_grad_(True)
    q, k, v = (t.view(TOTAL, H, D) for t in x0.split(C, dim=1))
    want = flash_attention_varlen(q, k, v, cu, causal=causal)
    want.backward(g.view(TOTAL, H, D))

    x1 = qkv.clone().requires_grad_(True)
    with _RecordOps() as rec:
        y = flash_attention_qkv_varlen(x1, H, cu, causal=causal)
        (gx,) = torch.autograd.grad(y, x1, g)
    assert y.shape == (TOTAL, C) and y.is_contiguous()
    assert_bits(y.detach(), want.detach().view(TOTAL, C), "y")
    assert torch.isfinite(gx).all()
    assert_bits(gx, x0.grad, "dqkv")

    assert rec.names, "dispatch mode saw nothing"
    copies = [n for n in rec.names
              if any(w in n for w in ("cat", "clone", "copy", "contiguous"))]
    assert not copies, copies


# ---------------------------------------------------------------------------
# 8. no host dependence: a captured graph follows a refilled cu_seqlens
# ---------------------------------------------------------------------------
def test_graph_replay_follows_cu_seqlens():
    from adapcc_amd.ops.attention import flash_attention_qkv_varlen

    torch.manual_seed(40)
    qkv = torch.randn(TOTAL, 3 * C, device="cuda",
                      dtype=torch.bfloat16).requires_grad_(True)
    g = torch.randn(TOTAL, C, device="cuda", dtype=torch.bfloat16)
    cu = cu_of(LENS)

    def fwd_bwd(x, gy, offsets):
        y = flash_attention_qkv_varlen(x, H, offsets)
        (gx,) = torch.autograd.grad(y, x, gy)
        return y, gx

    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        for _ in range(2):
            fwd_bwd(qkv, g, cu)
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()

    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        y, gx = fwd_bwd(qkv, g, cu)

    # the same total and number of sequences, split differently
    for lens in ([300, 0, 7, 128, 1, 130, 200, 64, 43],
                 [0, 0, 873, 0, 0, 0, 0, 0, 0]):
        assert sum(lens) == TOTAL and len(lens) == len(LENS)
        new_cu = cu_of(lens)
        cu.copy_(new_cu)
        graph.replay()
        torch.cuda.synchronize()
        want_y, want_gx = fwd_bwd(qkv, g, new_cu)
        assert_bits(y.detach(), want_y.detach(), "y")
        assert_bits(gx, want_gx, "dqkv")


# ---------------------------------------------------------------------------
# 9. GPT-2
# ---------------------------------------------------------------------------
DOCS = [5, 1, 130, 64]


def _gpt2_cfg(**kw):
    from adapcc_amd.models.gpt2 import GPT2Config

    # GPT2Config.tiny() with 2 heads instead of 4: head_dim 64, the one the
    # kernels take
    return GPT2Config(vocab_size=2048, n_positions=256, n_embd=128,
                      n_layer=2, n_head=2, **kw)


def test_gpt2_packed_equals_per_document(monkeypatch):
    from adapcc_amd.models.gpt2 import GPT2

    cfg = _gpt2_cfg()
    torch.manual_seed(50)
    model = GPT2(cfg).to("cuda").to(torch.bfloat16).eval()
    docs = [torch.randint(0, cfg.vocab_size, (n,), device="cuda")
            for n in DOCS]
    calls = record_launches(monkeypatch)
    with torch.no_grad():
        packed, _ = model(torch.cat(docs)[None], cu_seqlens=cu_of(DOCS))
        assert calls == [("fwd", True, 0.0, True)] * cfg.n_layer
        single = torch.cat([model(d[None])[0][0] for d in docs])
    # the single runs took other paths: no launch in either mode
    assert calls == [("fwd", True, 0.0, True)] * cfg.n_layer
    torch.testing.assert_close(packed[0].float(), single.float(), rtol=2e-2,
                               atol=2e-2)


def test_gpt2_packed_training_step(monkeypatch):
    from adapcc_amd.models.gpt2 import GPT2

    cfg = _gpt2_cfg(dropout=0.1, resid_dropout=0.1)
    torch.manual_seed(51)
    model = GPT2(cfg).to("cuda").to(torch.bfloat16).train()
    docs = [torch.randint(0, cfg.vocab_size, (n,), device="cuda")
            for n in DOCS]
    targets = []
    for d in docs:
        t = torch.roll(d, -1)
        t[-1] = -100  # no target across a document boundary
        targets.append(t)
    calls = record_launches(monkeypatch)
    _, loss = model(torch.cat(docs)[None], torch.cat(targets)[None],
                    cu_seqlens=cu_of(DOCS))
    loss.backward()
    assert calls == ([("fwd", True, 0.1, True)] * cfg.n_layer
                     + [("bwd", True, 0.1, True)] * cfg.n_layer)
    assert torch.isfinite(loss)
    grads = [p.grad for p in model.parameters() if p.grad is not None]
    assert grads and all(torch.isfinite(x).all() for x in grads)
