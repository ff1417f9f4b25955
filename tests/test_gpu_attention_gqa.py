"""Grouped-query / multi-query attention on the hand-written CDNA4 kernels
(csrc/attn.hip, kGqa): k and v with Hk < H heads, query head h reading K/V
head h // G, G = H // Hk, and dk, dv summed over each group inside the dkv
kernel.

Every test first asserts the ``*_supported`` predicate of the entry point it
uses, so where GQA is not a kernel path it fails there.

What is held bit for bit (rtol = atol = 0): the forward and the dq kernel
against today's kernels on K/V expanded to H heads (they only look K/V up
elsewhere), each group member's share of dK/dV against today's dkv kernel
on that member alone, the packed layouts against the strided views, and a
graph replay against the eager call. The group sum itself is compared with
the fp32 reference on repeated K/V, whose autograd sums the group, at the
project's tolerances (rtol = atol = 2e-2 for o, 5e-2 for the gradients)."""

import math

import pytest
import torch

from attn_util import record_launches, ref_attention_f32

pytestmark = pytest.mark.gpu

DIMS = (64, 128)
SEED = 0x7123456789ABCDEF  # high word set
P_DROP = 0.1
O_TOL, G_TOL = 2e-2, 5e-2


def rand(shape, seed):
    torch.manual_seed(seed)
    return torch.randn(*shape, device="cuda", dtype=torch.bfloat16)


def seed_tensor(value=SEED):
    return torch.tensor([value], dtype=torch.int64, device="cuda")


def assert_bits(got, want, what):
    torch.testing.assert_close(got, want, rtol=0, atol=0,
                               msg=lambda m: f"{what}: {m}")


def expand(t, G, dim=1):
    return t.repeat_interleave(G, dim=dim).contiguous()


def group_sum(t, G, dim=1):
    """fp32 sum over each run of G heads of a per-head bf16 gradient."""
    shape = list(t.shape)
    shape[dim:dim + 1] = [shape[dim] // G, G]
    return t.float().view(shape).sum(dim + 1)


def launch(q, k, v, g, causal, p=0.0, o_lse=None):
    """The launch helpers themselves on [B,H,S,D] q and [B,Hk,S,D] k, v:
    dict of o, lse, delta, dq, dk, dv. o_lse: skip the forward."""
    from adapcc_amd.ops.attention import (_fa_forward_lse, _launch_bwd,
                                          fa_supported)

    assert fa_supported(q, k, v, causal, p)
    scale = 1.0 / math.sqrt(q.shape[3])
    kw = {"dropout_p": p, "seed": seed_tensor()} if p > 0.0 else {}
    o, lse = o_lse or _fa_forward_lse(q, k, v, scale, causal, **kw)
    B, H, S, _ = q.shape
    delta = torch.full((B, H, S), float("nan"), dtype=torch.float32,
                       device="cuda")
    dq, dk, dv = torch.empty_like(q), torch.empty_like(k), torch.empty_like(v)
    _launch_bwd(q, k, v, o, g, lse, dq, dk, dv, scale, causal=causal,
                delta=delta, **kw)
    return dict(o=o, lse=lse, delta=delta, dq=dq, dk=dk, dv=dv)


def ref_f32(q, k, v, g, causal, keep=None, p=0.0):
    """o, dq, dk, dv of the fp32 reference on k, v repeated to q's heads
    under autograd (dk, dv: the group sums). keep: [.., H, S, S] bool."""
    qr, kr, vr = (t.detach().float().requires_grad_(True) for t in (q, k, v))
    G = q.shape[1] // k.shape[1]
    ke, ve = kr.repeat_interleave(G, dim=1), vr.repeat_interleave(G, dim=1)
    scale = 1.0 / math.sqrt(q.shape[3])
    if keep is None:
        o = ref_attention_f32(qr, ke, ve, scale, causal)
    else:
        s = torch.matmul(qr, ke.transpose(-1, -2)) * scale
        if causal:
            S = q.shape[-2]
            future = torch.ones(S, S, dtype=torch.bool,
                                device=q.device).triu(1)
            s = s.masked_fill(future, float("-inf"))
        prob = torch.softmax(s, dim=-1) * keep.to(s.dtype) / (1.0 - p)
        o = torch.matmul(prob, ve)
    o.backward(g.float())
    return o.detach(), qr.grad, kr.grad, vr.grad


def assert_close_to_ref(got, want, what, names=("o", "dq", "dk", "dv")):
    """Prints each max-abs error first."""
    tols = {"o": O_TOL, "dq": G_TOL, "dk": G_TOL, "dv": G_TOL}
    for name, a, b in zip(names, got, want):
        assert torch.isfinite(a.float()).all(), f"{what} {name}"
        err = (a.float() - b).abs().max().item()
        print(f"{what} {name}: max abs err {err:.3e}")
        torch.testing.assert_close(a.float(), b, rtol=tols[name],
                                   atol=tols[name],
                                   msg=lambda m, n=name: f"{what} {n}: {m}")


def keep_mask(B, H, S, p=P_DROP):
    from adapcc_amd.ops.attention import dropout_keep_mask_reference

    return dropout_keep_mask_reference(SEED, B, H, S, p).cuda()


# ---------------------------------------------------------------------------
# a, c. fixed length: forward and dq bit for bit, the group sum against fp32
# ---------------------------------------------------------------------------
# (causal, B, H, Hk, S): one tile; two tiles, G = 3; multi-query, ragged two
# tiles; G = 2 of 3 K/V heads, one-row second tile; one key; a one-row
# second half-tile
CASES = [(True, 1, 4, 2, 128), (True, 2, 6, 2, 256), (False, 2, 4, 1, 197),
         (False, 1, 6, 3, 129), (False, 2, 2, 1, 1), (False, 2, 4, 2, 65)]
RUNS = [(c, 0.0) for c in CASES] + [(CASES[i], P_DROP) for i in (0, 2, 5)]

_fixed_cache = {}


def fixed_runs(D, case, p):
    """(inputs, the GQA launch, the launch on expanded K/V), made once."""
    key = (D, case, p)
    if key not in _fixed_cache:
        causal, B, H, Hk, S = case
        q, g = rand((B, H, S, D), 1), rand((B, H, S, D), 4)
        k, v = rand((B, Hk, S, D), 2), rand((B, Hk, S, D), 3)
        G = H // Hk
        _fixed_cache[key] = (
            (q, k, v, g), launch(q, k, v, g, causal, p),
            launch(q, expand(k, G), expand(v, G), g, causal, p))
    return _fixed_cache[key]


@pytest.mark.parametrize("case,p", RUNS)
@pytest.mark.parametrize("D", DIMS)
def test_fwd_and_dq_are_the_old_arithmetic(D, case, p):
    """o, lse, delta and dq against the same kernels on K/V expanded to H
    contiguous heads; with dropout this holds the mask plane to the query
    head."""
    _, got, want = fixed_runs(D, case, p)
    for name in ("o", "lse", "delta", "dq"):
        assert_bits(got[name], want[name], name)
    assert got["dk"].shape[1] == case[3] and got["dv"].shape[1] == case[3]


@pytest.mark.parametrize("case,p", RUNS)
@pytest.mark.parametrize("D", DIMS)
def test_group_sum_matches_reference(D, case, p):
    """dk, dv (and o, dq) against the fp32 reference at the project's
    tolerances. Prints beside them the error of the fp32 sum of the
    expanded run's per-head bf16 dk, dv, which is what the parent's kernels
    plus autograd give."""
    (q, k, v, g), got, exp = fixed_runs(D, case, p)
    causal, B, H, Hk, S = case
    keep = keep_mask(B, H, S) if p > 0.0 else None
    want = ref_f32(q, k, v, g, causal, keep, p)
    what = f"D={D} {case} p={p}"
    for name, r in (("dk", want[2]), ("dv", want[3])):
        e = (group_sum(exp[name], H // Hk) - r).abs().max().item()
        print(f"{what} {name}: expanded path max abs err {e:.3e}")
    assert_close_to_ref([got[n] for n in ("o", "dq", "dk", "dv")], want, what)


# ---------------------------------------------------------------------------
# b. each group member reaches dK/dV
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("causal,S", [(True, 256), (False, 197)])
@pytest.mark.parametrize("G", [2, 3])
@pytest.mark.parametrize("D", DIMS)
def test_each_group_member_reaches_dk_dv(D, G, causal, S):
    """dO zero in every query head but member j of each group: those heads
    have dP = 0, delta = 0 and dO = 0 and add exact zeros to the
    accumulators, so dk, dv are bit for bit those of today's dkv kernel on
    member j alone."""
    B, Hk = 2, 2
    H = Hk * G
    q, g = rand((B, H, S, D), 11), rand((B, H, S, D), 14)
    k, v = rand((B, Hk, S, D), 12), rand((B, Hk, S, D), 13)
    full = launch(q, k, v, g, causal)
    for j in range(G):
        gj = torch.zeros_like(g)
        gj[:, j::G] = g[:, j::G]
        got = launch(q, k, v, gj, causal, o_lse=(full["o"], full["lse"]))
        sel = [t[:, j::G].contiguous()
               for t in (q, full["o"], g, full["lse"])]
        want = launch(sel[0], k, v, sel[2], causal, o_lse=(sel[1], sel[3]))
        assert_bits(got["dk"], want["dk"], f"dk member {j}")
        assert_bits(got["dv"], want["dv"], f"dv member {j}")
        assert got["dk"].float().abs().max() > 0


# ---------------------------------------------------------------------------
# d. variable length
# ---------------------------------------------------------------------------
LENS = [1, 33, 64, 65, 128, 129, 197, 0, 256]
TOTAL = sum(LENS)  # 873: sequences start off the 128-row tile boundaries


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


def run_varlen(q, k, v, g, lens, causal, p):
    from adapcc_amd.ops.attention import (fa_varlen_supported,
                                          flash_attention_varlen)

    cu = cu_of(lens)
    assert fa_varlen_supported(q, k, v, cu, causal, p)
    kw = {"dropout_p": p, "dropout_seed": seed_tensor()} if p > 0.0 else {}
    qr, kr, vr = (t.detach().clone().requires_grad_(True) for t in (q, k, v))
    o = flash_attention_varlen(qr, kr, vr, cu, causal=causal, **kw)
    o.backward(g)
    assert kr.grad.shape == k.shape and vr.grad.shape == v.shape
    return o.detach(), qr.grad, kr.grad, vr.grad


@pytest.mark.parametrize("p", [0.0, P_DROP])
@pytest.mark.parametrize("causal", [True, False])
@pytest.mark.parametrize("H,Hk", [(4, 2), (3, 1)])
@pytest.mark.parametrize("D", DIMS)
def test_varlen(D, H, Hk, causal, p):
    """o, dq bit for bit the varlen call on expanded K/V; dk, dv against
    the fp32 reference of each sequence by itself, mask plane seq*H + h."""
    G = H // Hk
    q, g = rand((TOTAL, H, D), 21), rand((TOTAL, H, D), 24)
    k, v = rand((TOTAL, Hk, D), 22), rand((TOTAL, Hk, D), 23)
    got = run_varlen(q, k, v, g, LENS, causal, p)
    exp = run_varlen(q, expand(k, G), expand(v, G), g, LENS, causal, p)
    assert_bits(got[0], exp[0], "o")
    assert_bits(got[1], exp[1], "dq")
    keep_all = keep_mask(len(LENS), H, max(LENS)) if p > 0.0 else None
    for i, a, b in spans(LENS):
        n = b - a
        keep = keep_all[i, :, :n, :n][None] if p > 0.0 else None
        want = ref_f32(*(seq4(t, a, b) for t in (q, k, v, g)), causal, keep,
                       p)
        what = f"varlen D={D} H={H}/{Hk} causal={causal} p={p} seq {i}"
        for name, x, r in (("dk", exp[2], want[2]), ("dv", exp[3], want[3])):
            e = (group_sum(seq4(x, a, b), G) - r).abs().max().item()
            print(f"{what} {name}: expanded path max abs err {e:.3e}")
        assert_close_to_ref([seq4(t, a, b) for t in got], want, what)


# ---------------------------------------------------------------------------
# e. packed layouts
# ---------------------------------------------------------------------------
def qkv_parts(x, H, Hk, D):
    return x.split([H * D, Hk * D, Hk * D], dim=-1)


@pytest.mark.parametrize("causal,S,p", [(True, 256, 0.0), (False, 197, 0.0),
                                        (True, 128, P_DROP)])
@pytest.mark.parametrize("D", DIMS)
def test_packed_equals_strided_views_bitwise(D, causal, S, p):
    from adapcc_amd.ops.attention import (fa_qkv_supported, fa_supported,
                                          flash_attention,
                                          flash_attention_qkv)

    B, H, Hk = 2, 4, 2
    qkv = rand((B, S, (H + 2 * Hk) * D), 30)
    g = rand((B, S, H * D), 31)
    kw = {"dropout_p": p, "dropout_seed": seed_tensor()} if p > 0.0 else {}
    assert fa_qkv_supported(qkv, H, p, causal, n_kv_head=Hk)
    x0 = qkv.clone().requires_grad_(True)
    y = flash_attention_qkv(x0, H, causal=causal, n_kv_head=Hk, **kw)
    assert y.shape == (B, S, H * D) and y.is_contiguous()
    y.backward(g)

    x1 = qkv.clone().requires_grad_(True)
    q, k, v = (t.view(B, S, -1, D).transpose(1, 2)
               for t in qkv_parts(x1, H, Hk, D))
    assert k.shape == (B, Hk, S, D) and fa_supported(q, k, v, causal, p)
    o = flash_attention(q, k, v, causal=causal, **kw)
    o.backward(g.view(B, S, H, D).transpose(1, 2))
    assert_bits(y.detach(), o.detach().transpose(1, 2).reshape(B, S, H * D),
                "y")
    for name, a, b in zip(("dq", "dk", "dv"), qkv_parts(x0.grad, H, Hk, D),
                          qkv_parts(x1.grad, H, Hk, D)):
        assert torch.isfinite(a).all()
        assert_bits(a, b, name)


@pytest.mark.parametrize("causal,p", [(True, 0.0), (False, P_DROP)])
@pytest.mark.parametrize("D", DIMS)
def test_varlen_packed_equals_strided_views_bitwise(D, causal, p):
    from adapcc_amd.ops.attention import (fa_qkv_varlen_supported,
                                          flash_attention_qkv_varlen)

    H, Hk = 4, 2
    qkv = rand((TOTAL, (H + 2 * Hk) * D), 32)
    g = rand((TOTAL, H * D), 33)
    cu = cu_of(LENS)
    kw = {"dropout_p": p, "dropout_seed": seed_tensor()} if p > 0.0 else {}
    assert fa_qkv_varlen_supported(qkv, H, cu, p, causal, n_kv_head=Hk)
    x0 = qkv.clone().requires_grad_(True)
    y = flash_attention_qkv_varlen(x0, H, cu, causal=causal, n_kv_head=Hk,
                                   **kw)
    assert y.shape == (TOTAL, H * D)
    y.backward(g)

    q, k, v = (t.view(TOTAL, -1, D) for t in qkv_parts(qkv, H, Hk, D))
    o, dq, dk, dv = run_varlen(q, k, v, g.view(TOTAL, H, D), LENS, causal, p)
    assert_bits(y.detach(), o.reshape(TOTAL, H * D), "y")
    for name, a, b in zip(("dq", "dk", "dv"), qkv_parts(x0.grad, H, Hk, D),
                          (dq, dk, dv)):
        assert_bits(a, b.reshape(TOTAL, -1), name)


# ---------------------------------------------------------------------------
# f. graph capture
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("D", DIMS)
def test_graph_capture_rereads_seed(D):
    from adapcc_amd.ops.attention import fa_supported, flash_attention

    B, H, Hk, S = 2, 4, 2, 128
    q = rand((B, H, S, D), 40).requires_grad_(True)
    k = rand((B, Hk, S, D), 41).requires_grad_(True)
    v = rand((B, Hk, S, D), 42).requires_grad_(True)
    g = rand((B, H, S, D), 43)
    assert fa_supported(q, k, v, True, P_DROP)
    seed = seed_tensor(1)

    def step(s):
        o = flash_attention(q, k, v, causal=True, dropout_p=P_DROP,
                            dropout_seed=s)
        return (o,) + torch.autograd.grad(o, (q, k, v), g)

    for _ in range(2):  # allocator warmup on a side stream
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            step(seed)
        torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        outs = step(seed)

    replays = []
    for value in (SEED, 1234):
        seed.fill_(value)
        graph.replay()
        torch.cuda.synchronize()
        replays.append([t.detach().clone() for t in outs])
        want = step(seed_tensor(value))
        for name, a, b in zip(("o", "dq", "dk", "dv"), replays[-1], want):
            assert_bits(a, b.detach(), f"seed {value:#x} {name}")
    for name, a, b in zip(("o", "dq", "dk", "dv"), *replays):
        assert not torch.equal(a, b), name


# ---------------------------------------------------------------------------
# g. GPT-2
# ---------------------------------------------------------------------------
MODEL_TOL = 2 * 7.812e-3  # twice the measured control, see the test


def _gpt2(n_kv_head, seed):
    from adapcc_amd.models.gpt2 import GPT2, GPT2Config

    cfg = GPT2Config(vocab_size=512, n_positions=128, n_embd=256, n_layer=2,
                     n_head=4, n_kv_head=n_kv_head)
    torch.manual_seed(seed)
    return GPT2(cfg)


def _expand_kv_state(sd, H, Hk, hd):
    """c_attn's K and V row blocks of each K/V head repeated G times: the
    n_kv_head = H model that computes the same function."""
    G = H // Hk
    out = {}
    for name, t in sd.items():
        if ".c_attn." in name:
            q, k, v = t.split([H * hd, Hk * hd, Hk * hd], dim=0)
            k, v = (x.view(Hk, hd, *x.shape[1:]).repeat_interleave(G, dim=0)
                    .reshape(H * hd, *x.shape[1:]) for x in (k, v))
            t = torch.cat([q, k, v], dim=0)
        out[name] = t.clone()
    return out


def _permute_heads_state(sd, H, hd, perm):
    """The same n_kv_head = H model with its heads in the order `perm`:
    c_attn's rows move inside the q, k and v blocks, c_proj's columns
    follow."""
    idx = torch.cat([torch.arange(h * hd, (h + 1) * hd) for h in perm])
    out = {}
    for name, t in sd.items():
        if ".attn.c_attn." in name:
            t = torch.cat([x[idx] for x in t.split(H * hd, dim=0)], dim=0)
        elif name.endswith(".attn.c_proj.weight"):
            t = t[:, idx]
        out[name] = t.clone()
    return out


def test_gpt2_grouped_runs_kernels_and_matches_repeated_weights(monkeypatch):
    """n_kv_head = 2 of 4 heads: the kernels run with two K/V heads, the
    loss is finite, and the logits are those of the n_kv_head = 4 model
    whose c_attn repeats each K/V head's rows, within MODEL_TOL.

    MODEL_TOL is twice the max-abs difference measured between two
    n_kv_head = 4 models that compute the same function and differ only in
    the order of c_attn's rows (heads reversed, c_proj's columns
    following): what bf16 GEMMs of another shape or order do to these
    logits, attention aside. Measured on an MI355X: control 7.812e-03 (one
    bf16 step at these logits, max |logit| 1.9), grouped against repeated
    weights 0 (bit-equal). The test prints both differences."""
    from adapcc_amd.ops import attention

    H, Hk, hd, T = 4, 2, 64, 128
    grouped = _gpt2(Hk, 50)
    sd = grouped.state_dict()
    assert sd["h.0.attn.c_attn.weight"].shape == ((H + 2 * Hk) * hd, 256)
    full_sd = _expand_kv_state(sd, H, Hk, hd)
    full, turned = _gpt2(H, 51), _gpt2(H, 52)
    full.load_state_dict(full_sd)
    turned.load_state_dict(_permute_heads_state(full_sd, H, hd,
                                                [3, 2, 1, 0]))
    grouped, full, turned = (m.to("cuda").to(torch.bfloat16)
                             for m in (grouped, full, turned))
    data = torch.randint(0, 512, (2, T + 1), device="cuda")
    x, t = data[:, :-1], data[:, 1:].contiguous()
    qkv = grouped.h[0].attn.c_attn(grouped.wte(x))
    assert attention.fa_qkv_supported(qkv, H, 0.0, n_kv_head=Hk)

    # each entry ends in the head counts of q and k
    calls = record_launches(
        monkeypatch, extra=lambda q, k, *a: (q.shape[1], k.shape[1]))
    logits, loss = grouped(x, t)
    loss.backward()
    assert calls == ([("fwd", True, 0.0, False, H, Hk)] * 2
                     + [("bwd", True, 0.0, False, H, Hk)] * 2)
    assert torch.isfinite(loss)
    assert all(torch.isfinite(p.grad).all() for p in grouped.parameters())
    with torch.no_grad():
        want, other = full(x)[0], turned(x)[0]
    err = (logits.float() - want.float()).abs().max().item()
    ctrl = (other.float() - want.float()).abs().max().item()
    print(f"gpt2 logits: grouped vs repeated weights {err:.3e}, "
          f"control (row order only) {ctrl:.3e}, max |logit| "
          f"{want.float().abs().max().item():.3e}")
    assert err <= MODEL_TOL
