"""Head dimension 128 of the hand-written CDNA4 flash attention
(csrc/attn.hip, kHD = 128): numerics against the fp32 reference in every
mode, the upper 64-column block against the head_dim 64 kernels bit for bit,
the deferred rescale over four accumulators, layouts, variable-length
sequences, dropout, graph capture and the MoE block.

Every test first asserts the ``*_supported`` predicate of the entry point it
uses, so where head_dim 128 is not a kernel path it fails there.

Tolerances are those of test_gpu_attention.py (rtol = atol = 2e-2 for o,
5e-2 for the gradients, randn inputs): a softmax-weighted average and its
gradients do not grow with D at scale 1/sqrt(D)."""

import math

import pytest
import torch
from torch.utils._python_dispatch import TorchDispatchMode

from attn_util import heads, ref_attention_f32, unheads

pytestmark = pytest.mark.gpu

D = 128
SCALE = 1.0 / math.sqrt(D)
SEED = 0x7123456789ABCDEF  # high word set


def rand(shape, seed):
    torch.manual_seed(seed)
    return torch.randn(*shape, device="cuda", dtype=torch.bfloat16)


def seed_tensor(value):
    return torch.tensor([value], dtype=torch.int64, device="cuda")


def assert_bits(got, want, what):
    torch.testing.assert_close(got, want, rtol=0, atol=0,
                               msg=lambda m: f"{what}: {m}")


def ref_f32(q, k, v, g, scale, causal, keep=None, p=0.0):
    """o, dq, dk, dv of the fp32 reference; ``keep`` ([.., S, S] bool) and
    1/(1-p) are applied to the probabilities after the softmax."""
    qr, kr, vr = (t.detach().float().requires_grad_(True) for t in (q, k, v))
    if keep is None:
        o = ref_attention_f32(qr, kr, vr, scale, causal)
    else:
        s = torch.matmul(qr, kr.transpose(-1, -2)) * scale
        if causal:
            S = q.shape[-2]
            future = torch.ones(S, S, dtype=torch.bool,
                                device=q.device).triu(1)
            s = s.masked_fill(future, float("-inf"))
        prob = torch.softmax(s, dim=-1) * keep.to(s.dtype) / (1.0 - p)
        o = torch.matmul(prob, vr)
    o.backward(g.float())
    return o.detach(), qr.grad, kr.grad, vr.grad


def assert_close_to_ref(got, want, what):
    """got, want: (o, dq, dk, dv). Prints each max-abs error first."""
    for name, a, b, tol in zip(("o", "dq", "dk", "dv"), got, want,
                               (2e-2, 5e-2, 5e-2, 5e-2)):
        err = (a.float() - b).abs().max().item()
        print(f"{what} {name}: max abs err {err:.3e}")
        torch.testing.assert_close(a.float(), b, rtol=tol, atol=tol,
                                   msg=lambda m, n=name: f"{what} {n}: {m}")


def run_fixed(q, k, v, g, causal, **kw):
    from adapcc_amd.ops.attention import fa_supported, flash_attention

    assert fa_supported(q, k, v, causal, kw.get("dropout_p", 0.0))
    qr, kr, vr = (t.detach().clone().requires_grad_(True) for t in (q, k, v))
    o = flash_attention(qr, kr, vr, causal=causal, **kw)
    o.backward(g)
    return o.detach(), qr.grad, kr.grad, vr.grad


# ---------------------------------------------------------------------------
# a. numerics against fp32
# ---------------------------------------------------------------------------
# causal; non-causal even; ragged non-causal: one key, a one-row second
# half-tile, a one-row second workgroup, two workgroups
CASES = [(True, 1, 1, 128), (True, 2, 3, 256), (False, 1, 2, 128),
         (False, 2, 3, 1), (False, 2, 3, 65), (False, 2, 3, 129),
         (False, 2, 3, 197)]


@pytest.mark.parametrize("causal,B,H,S", CASES)
def test_fwd_bwd_matches_reference(causal, B, H, S):
    q, k, v, g = (rand((B, H, S, D), i) for i in range(4))
    got = run_fixed(q, k, v, g, causal)
    for t in got:
        assert torch.isfinite(t.float()).all()
    assert_close_to_ref(got, ref_f32(q, k, v, g, SCALE, causal),
                        f"causal={causal} S={S}")


# ---------------------------------------------------------------------------
# b. the upper column block
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("causal,S", [(True, 256), (False, 197)])
def test_upper_block_equals_d64_kernels_bitwise(causal, S):
    """q, k zero in columns 64..127: chunks 4..7 add exact zeros to S^T, so
    the scores, lse and P are those of the head_dim 64 kernel on the lower
    halves, and P.V is computed per 32-column block: o[..., :64] and
    o[..., 64:] are the D = 64 forward on the two halves of v."""
    from adapcc_amd.ops.attention import _fa_forward_lse, fa_supported

    B, H, s = 2, 3, 0.11
    q, k, v = (rand((B, H, S, D), 10 + i) for i in range(3))
    q[..., 64:] = 0
    k[..., 64:] = 0
    assert fa_supported(q, k, v, causal, 0.0)
    o, lse = _fa_forward_lse(q, k, v, s, causal)
    ql, kl = q[..., :64], k[..., :64]
    for name, cols in (("lower", slice(0, 64)), ("upper", slice(64, 128))):
        vh = v[..., cols]
        assert fa_supported(ql, kl, vh, causal, 0.0)
        o64, lse64 = _fa_forward_lse(ql, kl, vh, s, causal)
        assert_bits(o[..., cols], o64, f"o {name}")
        assert_bits(lse, lse64, f"lse {name}")


# ---------------------------------------------------------------------------
# c. spiked key: the deferred rescale across four accumulators
# ---------------------------------------------------------------------------
def test_extreme_values_stable():
    torch.manual_seed(2)
    B, H, S = 1, 2, 256
    q = (torch.randn(B, H, S, D, device="cuda") * 4).to(torch.bfloat16)
    k = (torch.randn(B, H, S, D, device="cuda") * 4).to(torch.bfloat16)
    k[:, :, 200, :] *= 8
    v = torch.randn(B, H, S, D, device="cuda").to(torch.bfloat16)
    o = run_fixed(q, k, v, torch.zeros_like(v), True)[0]
    assert torch.isfinite(o.float()).all()
    ref = ref_attention_f32(q, k, v, SCALE, True)
    print("spiked key: max abs err", (o.float() - ref).abs().max().item())
    torch.testing.assert_close(o.float(), ref, rtol=3e-2, atol=3e-2)


# ---------------------------------------------------------------------------
# d. layouts
# ---------------------------------------------------------------------------
class _RecordOps(TorchDispatchMode):
    def __init__(self):
        super().__init__()
        self.names = []

    def __torch_dispatch__(self, func, types, args=(), kwargs=None):
        self.names.append(str(func))
        return func(*args, **(kwargs or {}))


def test_packed_and_strided_equal_contiguous_bitwise():
    from adapcc_amd.ops.attention import (fa_qkv_supported,
                                          flash_attention_qkv)

    B, H, S = 2, 3, 256
    C = H * D
    qkv = rand((B, S, 3 * C), 20)
    g = rand((B, S, C), 21)
    assert fa_qkv_supported(qkv, H, 0.0)

    # contiguous [B,H,S,D] inputs
    qc, kc, vc = (heads(t, H).contiguous() for t in qkv.split(C, dim=2))
    want = run_fixed(qc, kc, vc, heads(g, H).contiguous(), True)
    # the strided head views of the packed tensor, read in place
    from adapcc_amd.ops.attention import fa_supported, flash_attention

    xs = qkv.clone().requires_grad_(True)
    qs, ks, vs = (heads(t, H) for t in xs.split(C, dim=2))
    assert not qs.is_contiguous() and qs.stride(2) == 3 * C
    assert fa_supported(qs, ks, vs, True, 0.0)
    o = flash_attention(qs, ks, vs, causal=True)
    o.backward(heads(g, H))
    assert_bits(o.detach(), want[0], "strided o")
    for name, a, b in zip(("dq", "dk", "dv"), xs.grad.split(C, dim=2),
                          want[1:]):
        assert_bits(heads(a, H), b, f"strided {name}")

    # the packed entry point, with no pass over the activations besides the
    # kernels
    x = qkv.clone().requires_grad_(True)
    with _RecordOps() as rec:
        y = flash_attention_qkv(x, H)
        (gx,) = torch.autograd.grad(y, x, g)
    assert y.shape == (B, S, C) and y.is_contiguous()
    assert_bits(y.detach(), unheads(want[0]), "packed y")
    assert torch.isfinite(gx).all()
    assert_bits(gx, torch.cat([unheads(t) for t in want[1:]], dim=2),
                "packed grad")
    assert rec.names, "dispatch mode saw nothing"
    copies = [n for n in rec.names
              if any(w in n for w in ("cat", "clone", "copy", "contiguous"))]
    assert not copies, copies


# ---------------------------------------------------------------------------
# e. variable-length
# ---------------------------------------------------------------------------
VH = 2
LENS = [1, 65, 0, 129, 197, 128]
TOTAL = sum(LENS)  # 520


def cu_of(lens):
    cu = [0]
    for n in lens:
        cu.append(cu[-1] + n)
    return torch.tensor(cu, dtype=torch.int32, device="cuda")


def spans(lens):
    cu = cu_of(lens).tolist()
    return [(i, a, b) for i, (a, b) in enumerate(zip(cu[:-1], cu[1:]))
            if b > a]


def seq4(t, a, b):
    """Rows a..b-1 of a [total,H,D] tensor as a [1,H,len,D] batch."""
    return t[a:b].transpose(0, 1)[None]


def run_varlen(q, k, v, g, lens, causal, **kw):
    from adapcc_amd.ops.attention import (fa_varlen_supported,
                                          flash_attention_varlen)

    cu = cu_of(lens)
    assert fa_varlen_supported(q, k, v, cu, causal, kw.get("dropout_p", 0.0))
    qr, kr, vr = (t.detach().clone().requires_grad_(True) for t in (q, k, v))
    o = flash_attention_varlen(qr, kr, vr, cu, causal=causal, **kw)
    o.backward(g)
    return o.detach(), qr.grad, kr.grad, vr.grad


@pytest.fixture(scope="module")
def vdata():
    return tuple(rand((TOTAL, VH, D), 30 + i) for i in range(4))


@pytest.fixture(scope="module")
def vpacked(vdata):
    return {causal: run_varlen(*vdata, LENS, causal)
            for causal in (True, False)}


@pytest.mark.parametrize("causal", [True, False])
def test_varlen_matches_reference_per_sequence(vdata, vpacked, causal):
    got = vpacked[causal]
    for t in got:
        assert torch.isfinite(t.float()).all()
    for i, a, b in spans(LENS):
        want = ref_f32(*(seq4(t, a, b) for t in vdata), SCALE, causal)
        assert_close_to_ref([seq4(t, a, b) for t in got], want,
                            f"varlen causal={causal} seq {i}")


def test_varlen_causal_bits_equal_fixed_length_zero_padded(vdata, vpacked):
    got = vpacked[True]
    for i, a, b in spans(LENS):
        n = b - a
        P = -(-n // 128) * 128

        def pad(t):
            x = torch.zeros(1, VH, P, D, device="cuda", dtype=torch.bfloat16)
            x[:, :, :n] = seq4(t, a, b)
            return x

        want = run_fixed(*(pad(t) for t in vdata), True)
        for name, x, y in zip(("o", "dq", "dk", "dv"), got, want):
            assert_bits(seq4(x, a, b), y[:, :, :n], f"{name} seq {i}")


@pytest.mark.parametrize("causal", [True, False])
def test_varlen_packed_equals_unpacked_bitwise(vdata, vpacked, causal):
    from adapcc_amd.ops.attention import (fa_qkv_varlen_supported,
                                          flash_attention_qkv_varlen)

    q, k, v, g = vdata
    C = VH * D
    qkv = torch.cat([t.reshape(TOTAL, C) for t in (q, k, v)],
                    dim=1).requires_grad_(True)
    cu = cu_of(LENS)
    assert fa_qkv_varlen_supported(qkv, VH, cu, 0.0, causal=causal)
    y = flash_attention_qkv_varlen(qkv, VH, cu, causal=causal)
    y.backward(g.reshape(TOTAL, C))
    o, dq, dk, dv = vpacked[causal]
    assert_bits(y.detach(), o.reshape(TOTAL, C), "y")
    assert_bits(qkv.grad, torch.cat([t.reshape(TOTAL, C)
                                     for t in (dq, dk, dv)], dim=1), "grad")


# ---------------------------------------------------------------------------
# f. dropout
# ---------------------------------------------------------------------------
P_DROP = 0.3


def replica(seed, b, h, S):
    from adapcc_amd.ops.attention import dropout_keep_mask_reference

    return dropout_keep_mask_reference(seed, b, h, S, P_DROP).cuda()


@pytest.mark.parametrize("causal,S", [(True, 128), (False, 65)])
def test_dropout_matches_reference_and_seed_rules(causal, S):
    B, H = 1, 2
    q, k, v, g = (rand((B, H, S, D), 40 + i) for i in range(4))
    got = run_fixed(q, k, v, g, causal, dropout_p=P_DROP,
                    dropout_seed=seed_tensor(SEED))
    keep = replica(SEED, B, H, S)
    assert_close_to_ref(got, ref_f32(q, k, v, g, SCALE, causal, keep, P_DROP),
                        f"dropout causal={causal} S={S}")
    again = run_fixed(q, k, v, g, causal, dropout_p=P_DROP,
                      dropout_seed=seed_tensor(SEED))
    other = run_fixed(q, k, v, g, causal, dropout_p=P_DROP,
                      dropout_seed=seed_tensor(1234))
    for name, a, b, c in zip(("o", "dq", "dk", "dv"), got, again, other):
        assert_bits(b, a, name)
        assert not torch.equal(c, a), name


@pytest.mark.parametrize("causal", [True, False])
def test_dropout_varlen_mask_plane(causal):
    """Two sequences: the mask of sequence i, head h is plane i * H + h."""
    lens = [65, 129]
    total = sum(lens)
    q, k, v, g = (rand((total, VH, D), 50 + i) for i in range(4))
    got = run_varlen(q, k, v, g, lens, causal, dropout_p=P_DROP,
                     dropout_seed=seed_tensor(SEED))
    keep_all = replica(SEED, len(lens), VH, max(lens))
    for i, a, b in spans(lens):
        n = b - a
        want = ref_f32(*(seq4(t, a, b) for t in (q, k, v, g)), SCALE, causal,
                       keep_all[i, :, :n, :n][None], P_DROP)
        assert_close_to_ref([seq4(t, a, b) for t in got], want,
                            f"varlen dropout causal={causal} seq {i}")


# ---------------------------------------------------------------------------
# g. graph capture
# ---------------------------------------------------------------------------
def test_graph_capture_replays_bitwise():
    from adapcc_amd.ops.attention import (fa_qkv_supported,
                                          flash_attention_qkv)

    B, H, S = 2, 2, 256
    C = H * D
    qkv = rand((B, S, 3 * C), 60).requires_grad_(True)
    g = rand((B, S, C), 61)
    assert fa_qkv_supported(qkv, H, 0.0)

    def fwd_bwd(x, gy):
        y = flash_attention_qkv(x, H)
        (gx,) = torch.autograd.grad(y, x, gy)
        return y, gx

    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        for _ in range(2):
            fwd_bwd(qkv, g)
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()

    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        y, gx = fwd_bwd(qkv, g)

    for seed in (62, 64):
        new_qkv = rand((B, S, 3 * C), seed)
        new_g = rand((B, S, C), seed + 1)
        with torch.no_grad():
            qkv.copy_(new_qkv)
            g.copy_(new_g)
        graph.replay()
        torch.cuda.synchronize()
        want_y, want_gx = fwd_bwd(new_qkv.requires_grad_(True), new_g)
        assert_bits(y.detach(), want_y.detach(), "y")
        assert_bits(gx, want_gx, "grad")


# ---------------------------------------------------------------------------
# h. the MoE block
# ---------------------------------------------------------------------------
def test_moe_block_fused_attention(monkeypatch):
    """The fused block against the default one on shared weights, within
    3e-2 on every element of the output and the input gradient.

    The gate weight is zero in both: all logits are exactly 0, so top-1
    routing (first expert, first ``capacity`` tokens, gate 1/2) does not
    depend on the activations and the block is a continuous function of its
    attention output. With a random gate the two attention paths, equal to
    bf16 rounding, send a token whose two logits nearly tie to different
    experts (measured: 1 token of 394, 191 of its 256 outputs off by up to
    0.36), which says nothing about the attention."""
    from adapcc_amd.models.moe import MoETransformerBlock
    from adapcc_amd.ops import attention

    kw = dict(d_model=256, n_head=2, d_hidden=512, num_local_experts=2)
    torch.manual_seed(70)
    plain = MoETransformerBlock(**kw)
    with torch.no_grad():
        plain.moe.gate.weight.zero_()
    plain = plain.to("cuda").to(torch.bfloat16)
    fused = MoETransformerBlock(fused_attention=True, **kw)
    assert list(fused.state_dict().keys()) == list(plain.state_dict().keys())
    fused = fused.to("cuda").to(torch.bfloat16)
    fused.load_state_dict(plain.state_dict())

    x = rand((2, 197, 256), 71)
    g = rand((2, 197, 256), 72)
    qkv = torch.nn.functional.linear(x, fused.attn.in_proj_weight,
                                     fused.attn.in_proj_bias)
    assert attention.fa_qkv_supported(qkv, 2, 0.0, causal=False)

    calls = []
    real_fwd = attention._launch_fwd

    def counting_fwd(*a, **k):
        calls.append(a[0].shape[3])
        return real_fwd(*a, **k)

    monkeypatch.setattr(attention, "_launch_fwd", counting_fwd)

    def run(block):
        xr = x.clone().requires_grad_(True)
        y = block(xr)
        y.backward(g)
        return y.detach(), xr.grad

    want_y, want_gx = run(plain)
    assert calls == []
    got_y, got_gx = run(fused)
    assert calls == [D]
    print("moe block: max abs err y",
          (got_y.float() - want_y.float()).abs().max().item(), "dx",
          (got_gx.float() - want_gx.float()).abs().max().item())
    torch.testing.assert_close(got_y, want_y, rtol=3e-2, atol=3e-2)
    torch.testing.assert_close(got_gx, want_gx, rtol=3e-2, atol=3e-2)
