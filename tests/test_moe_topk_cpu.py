"""Top-k MoE routing with the load-balancing loss (adapcc_amd/ops/moe.py):
the plain-torch fallback against a numpy reference written here on the
fp64-upcast logits, and ``MoEMLP(top_k=2)`` on the CPU."""

import math
import os

import numpy as np
import pytest
import torch

from util_mp import run_mp

from adapcc_amd.models.moe import MoEMLP, MoETransformerBlock
from adapcc_amd.ops.moe import (RoutingTopK, moe_combine, moe_dispatch,
                                moe_fusable, moe_route_top1, moe_route_topk)

CASES = [(2, 2, 1), (3, 2, 1), (63, 3, 5), (64, 16, 5), (65, 16, 1),
         (257, 10, 33), (4097, 64, 81), (1000, 256, 4)]


def _logits(T, E, dtype=torch.float32):
    torch.manual_seed(0)
    return (torch.randn(T, E) * 2).to(dtype)


def route_reference(logits, k, cap, normalize=True):
    """dict of gate (fp64), expert, slot, src, src_choice, load, aux from the
    upcast logits: np.argmax takes the first maximum, the second choice is
    the argmax with the first masked out, and one running count per expert
    over all first choices and then all second choices gives the position."""
    x = logits.detach().cpu().double().numpy()
    T, E = x.shape
    rows = np.arange(T)
    e0 = np.argmax(x, axis=1)
    masked = x.copy()
    masked[rows, e0] = -np.inf
    e1 = np.argmax(masked, axis=1)
    expert = np.stack([e0, e1], axis=1)[:, :k]
    z = np.exp(x - x.max(axis=1, keepdims=True))
    p = z / z.sum(axis=1, keepdims=True)
    if k == 2 and normalize:
        r = np.exp(x[rows, e1] - x[rows, e0])
        g0 = 1.0 / (1.0 + r)
        gate = np.stack([g0, r * g0], axis=1)
    else:
        gate = p[rows[:, None], expert]
    slot = np.full((T, k), -1, dtype=np.int64)
    src = np.full(E * cap, -1, dtype=np.int64)
    src_choice = np.full(E * cap, -1, dtype=np.int64)
    seen = np.zeros(E, dtype=np.int64)
    for c in range(k):
        for t in range(T):
            e = expert[t, c]
            if seen[e] < cap:
                slot[t, c] = e * cap + seen[e]
                src[slot[t, c]] = t
                src_choice[slot[t, c]] = c
            seen[e] += 1
    load = np.bincount(e0, minlength=E)
    aux = E * float(((load / T) * p.mean(axis=0)).sum())
    return dict(gate=gate, expert=expert, slot=slot, src=src,
                src_choice=src_choice, load=load, aux=aux, p=p)


_REF = {}


def _case(T, E, cap, dtype=torch.float32, k=2, normalize=True):
    key = (T, E, cap, dtype, k, normalize)
    if key not in _REF:
        lg = _logits(T, E, dtype)
        _REF[key] = (lg, route_reference(lg, k, cap, normalize))
    return _REF[key]


def _assert_ints(r, ref):
    for name in ("expert", "slot", "src", "src_choice", "load"):
        got = getattr(r, name)
        assert got.dtype == torch.int32, name
        assert np.array_equal(got.numpy(), ref[name]), name


# ------------------------------------------------------- test-input checks

@pytest.mark.parametrize("T,E,cap", [(64, 16, 5), (1000, 256, 4)])
def test_inputs_hold_every_capacity_outcome(T, E, cap):
    _, ref = _case(T, E, cap)
    kept = ref["slot"] >= 0
    assert (~kept[:, 0] & kept[:, 1]).any()   # first dropped, second kept
    assert (kept[:, 0] & ~kept[:, 1]).any()   # first kept, second dropped
    assert (~kept[:, 0] & ~kept[:, 1]).any()  # both dropped
    assert (ref["src"] < 0).any()             # empty slots


def test_inputs_sparse_case_has_empty_slots_and_drops():
    _, ref = _case(1000, 256, 12)
    assert (ref["src"] < 0).sum() > 1000
    assert 10 <= (ref["slot"] < 0).sum() <= 100


@pytest.mark.parametrize("T,E,cap", [(4097, 64, 81), (1000, 256, 4)])
def test_inputs_bf16_hold_exact_ties(T, E, cap):
    top3 = _logits(T, E, torch.bfloat16).float().topk(3, dim=-1).values
    assert (top3[:, 0] == top3[:, 1]).sum() >= 12
    assert (top3[:, 1] == top3[:, 2]).sum() >= 12


# ----------------------------------------------------------------- routing

@pytest.mark.parametrize("T,E,cap", CASES)
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_fallback_route_matches_reference(T, E, cap, dtype):
    for normalize in (True, False):
        lg, ref = _case(T, E, cap, dtype, 2, normalize)
        r = moe_route_topk(lg, 2, cap, normalize=normalize)
        assert isinstance(r, RoutingTopK)
        assert (r.capacity, r.num_experts, r.k) == (cap, E, 2)
        _assert_ints(r, ref)
        assert r.gate.dtype == torch.float32 and r.gate.shape == (T, 2)
        np.testing.assert_allclose(r.gate.numpy(), ref["gate"], rtol=1e-5,
                                   atol=1e-5)
        assert r.aux_loss.dtype == torch.float32 and r.aux_loss.dim() == 0
        np.testing.assert_allclose(r.aux_loss.item(), ref["aux"], rtol=1e-4)


@pytest.mark.parametrize("T,E,cap", CASES)
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_fallback_k1_equals_top1(T, E, cap, dtype):
    lg, ref = _case(T, E, cap, dtype, 1)
    r = moe_route_topk(lg, 1, cap)
    r1 = moe_route_top1(lg, cap)
    assert torch.equal(r.gate[:, 0], r1.gate_p)
    assert torch.equal(r.expert[:, 0], r1.expert)
    assert torch.equal(r.slot[:, 0], r1.slot)
    assert torch.equal(r.src, r1.src)
    assert torch.equal(r.src_choice, torch.where(r1.src >= 0, 0, -1).int())
    _assert_ints(r, ref)
    np.testing.assert_allclose(r.aux_loss.item(), ref["aux"], rtol=1e-4)
    # normalising one choice would be the constant 1: k=1 ignores the flag
    assert torch.equal(moe_route_topk(lg, 1, cap, normalize=False).gate,
                       r.gate)


def test_all_equal_logits():
    T, E, cap = 64, 8, 100
    for k in (1, 2):
        r = moe_route_topk(torch.full((T, E), 0.25), k, cap)
        assert (r.expert[:, 0] == 0).all()
        if k == 2:
            assert (r.expert[:, 1] == 1).all()
            assert torch.equal(r.gate, torch.full((T, 2), 0.5))
        assert r.load.tolist() == [T] + [0] * (E - 1)
        assert r.aux_loss.item() == 1.0


def test_aux_loss_of_one_dominant_expert_is_about_E():
    T, E = 200, 8
    lg = _logits(T, E)
    lg[:, 3] += 30.0
    r = moe_route_topk(lg, 2, 10)
    assert r.load.tolist() == [0, 0, 0, T, 0, 0, 0, 0]
    np.testing.assert_allclose(r.aux_loss.item(), float(E), rtol=1e-5)


@pytest.mark.parametrize("T,E,cap", CASES)
def test_slot_and_src_are_mutually_inverse(T, E, cap):
    lg, _ = _case(T, E, cap)
    r = moe_route_topk(lg, 2, cap)
    slot, src, ch = r.slot.long(), r.src.long(), r.src_choice.long()
    kept = (slot >= 0).nonzero()  # rows of (token, choice)
    assert torch.equal(src[slot[kept[:, 0], kept[:, 1]]], kept[:, 0])
    assert torch.equal(ch[slot[kept[:, 0], kept[:, 1]]], kept[:, 1])
    filled = (src >= 0).nonzero().squeeze(1)
    assert torch.equal((ch >= 0).nonzero().squeeze(1), filled)
    assert torch.equal(slot[src[filled], ch[filled]], filled)
    assert len(kept) == len(filled)
    assert (slot < E * cap).all() and (src < T).all() and (ch < 2).all()


# ---------------------------------------------- dispatch, combine, gradients

@pytest.mark.parametrize("normalize", [True, False])
@pytest.mark.parametrize("T,E,cap", [(63, 3, 5), (64, 16, 5), (65, 16, 1),
                                     (257, 10, 33)])
def test_fallback_dispatch_combine_match_indexing(T, E, cap, normalize):
    d = 24
    lg0, ref = _case(T, E, cap, torch.float32, 2, normalize)
    logits = lg0.clone().requires_grad_(True)
    torch.manual_seed(1)
    x = torch.randn(T, d, requires_grad=True)
    back = torch.randn(E * cap, d, requires_grad=True)
    r = moe_route_topk(logits, 2, cap, normalize=normalize)
    slot, src = torch.from_numpy(ref["slot"]), torch.from_numpy(ref["src"])
    choice = torch.from_numpy(ref["src_choice"])
    gate = torch.from_numpy(ref["gate"])
    kept, filled = slot >= 0, src >= 0

    disp = moe_dispatch(x, r)
    want = torch.zeros(E * cap, d)
    want[filled] = x.detach()[src[filled]]
    assert torch.equal(disp, want)

    y = moe_combine(back, r)
    bd = back.detach().double()
    want_y = torch.zeros(T, d, dtype=torch.float64)
    for c in range(2):
        kc = kept[:, c]
        want_y[kc] += bd[slot[kc, c]] * gate[kc, c, None]
    torch.testing.assert_close(y.double(), want_y, rtol=1e-5, atol=1e-5)
    none_kept = ~kept.any(dim=1)
    assert (y[none_kept] == 0).all()

    gd, gy = torch.randn_like(disp), torch.randn_like(y)
    daux = 0.7
    (disp * gd).sum().backward(retain_graph=True)
    want_dx = torch.zeros(T, d, dtype=torch.float64)
    for c in range(2):
        kc = kept[:, c]
        want_dx[kc] += gd.double()[slot[kc, c]]
    torch.testing.assert_close(x.grad.double(), want_dx, rtol=1e-5, atol=1e-5)
    assert (x.grad[none_kept] == 0).all()

    ((y * gy).sum() + daux * r.aux_loss).backward()
    want_dback = torch.zeros(E * cap, d, dtype=torch.float64)
    want_dback[filled] = (gy.double()[src[filled]]
                          * gate[src[filled], choice[filled], None])
    torch.testing.assert_close(back.grad.double(), want_dback, rtol=1e-5,
                               atol=1e-5)
    assert (back.grad[~filled] == 0).all()

    # dlogits from the contract's formulas, in fp64
    p = torch.from_numpy(ref["p"])
    e = torch.from_numpy(ref["expert"])
    dgate = torch.zeros(T, 2, dtype=torch.float64)
    for c in range(2):
        kc = kept[:, c]
        dgate[kc, c] = (gy.double()[kc] * bd[slot[kc, c]]).sum(-1)
    want_dl = torch.zeros(T, E, dtype=torch.float64)
    rows = torch.arange(T)
    if normalize:
        dx0 = (dgate[:, 0] - dgate[:, 1]) * gate[:, 0] * gate[:, 1]
        want_dl[rows, e[:, 0]] += dx0
        want_dl[rows, e[:, 1]] -= dx0
    else:
        for c in range(2):
            onehot = torch.nn.functional.one_hot(e[:, c], E).double()
            want_dl += (dgate[:, c] * gate[:, c])[:, None] * (onehot - p)
    lw = torch.from_numpy(ref["load"] / T)
    want_dl += daux * (E / T) * p * (lw[None, :] - (p * lw).sum(-1,
                                                               keepdim=True))
    torch.testing.assert_close(logits.grad.double(), want_dl, rtol=1e-5,
                               atol=1e-5)


def test_dropped_choices_get_no_gate_gradient():
    T, E, cap, d = 64, 16, 5, 8
    lg0, ref = _case(T, E, cap)
    kept = torch.from_numpy(ref["slot"] >= 0)
    none_kept = ~kept.any(dim=1)
    assert none_kept.any()
    for normalize in (True, False):
        logits = lg0.clone().requires_grad_(True)
        r = moe_route_topk(logits, 2, cap, normalize=normalize)
        gate = r.gate.detach().requires_grad_(True)
        torch.manual_seed(2)
        back = torch.randn(E * cap, d)
        y = moe_combine(back, r._replace(gate=gate))
        y.backward(torch.randn_like(y))
        assert (gate.grad[~kept] == 0).all()
        assert (gate.grad[kept] != 0).all()
        # without a gradient on the loss, a token with nothing kept gets
        # an exact zero row
        r.gate.backward(torch.randn(T, 2))
        assert (logits.grad[none_kept] == 0).all()


def test_fallback_is_anomaly_clean():
    T, E, cap, d = 40, 4, 3, 8
    for normalize in (True, False):
        with torch.autograd.set_detect_anomaly(True):
            logits = _logits(T, E).requires_grad_(True)
            x = torch.randn(T, d, requires_grad=True)
            r = moe_route_topk(logits, 2, cap, normalize=normalize)
            assert (r.slot < 0).all(dim=1).any()
            y = moe_combine(moe_dispatch(x, r) * 2.0, r)
            (y.sum() + r.aux_loss).backward()
        assert torch.isfinite(x.grad).all()
        assert torch.isfinite(logits.grad).all()


def test_bad_arguments_raise():
    for k in (0, 3):
        with pytest.raises(ValueError):
            moe_route_topk(torch.randn(8, 4), k, 2)
    with pytest.raises(ValueError):
        moe_route_topk(torch.randn(8, 1), 2, 2)      # E < k
    with pytest.raises(ValueError):
        moe_route_topk(torch.randn(8, 4), 2, 0)      # capacity < 1
    with pytest.raises(ValueError):
        moe_route_topk(torch.randn(8), 2, 2)         # rank
    with pytest.raises(ValueError):
        moe_route_topk(torch.randn(2, 8, 4), 2, 2)
    r = moe_route_topk(torch.randn(8, 2), 2, 4)
    with pytest.raises(ValueError):
        moe_dispatch(torch.randn(9, 4), r)
    with pytest.raises(ValueError):
        moe_combine(torch.randn(9, 4), r)
    with pytest.raises(ValueError):
        MoEMLP(d_model=8, d_hidden=8, num_local_experts=2, top_k=3)
    with pytest.raises(ValueError):
        MoEMLP(d_model=8, d_hidden=8, num_local_experts=1, top_k=2)


def test_moe_fusable_takes_k():
    x = torch.randn(64, 32)
    assert not moe_fusable(x, torch.randn(64, 4), 1, k=2)   # CPU tensors
    if torch.cuda.is_available():
        xg = x.cuda()
        assert not moe_fusable(xg, torch.randn(64, 1, device="cuda"), 1, k=2)
        assert not moe_fusable(xg, torch.randn(64, 4, device="cuda"), 1, k=3)


# ------------------------------------------------------------------- module

def _moe(E=4, d=32, **kw):
    torch.manual_seed(0)
    return MoEMLP(d_model=d, d_hidden=64, num_local_experts=E, world_size=1,
                  **kw)


@pytest.mark.parametrize("capacity_factor", [1.25, 0.25])
@pytest.mark.parametrize("normalize", [True, False])
def test_moemlp_top2_equals_the_ops_composed_by_hand(capacity_factor,
                                                     normalize):
    d, E, T = 32, 4, 60
    m = _moe(E, d, top_k=2, normalize_gates=normalize, balance_loss=True,
             capacity_factor=capacity_factor)
    torch.manual_seed(1)
    x = torch.randn(T, d)
    xa, xc = (x.clone().requires_grad_(True) for _ in range(2))
    ya = m(xa)
    g = torch.randn_like(ya)
    ga = torch.autograd.grad((ya * g).sum() + 0.3 * m.aux_loss,
                             [xa, m.gate.weight, m.experts[1].w1.weight])

    cap = max(1, math.ceil(2 * T / E * capacity_factor))
    logits = m.gate(xc)
    r = moe_route_topk(logits, 2, cap, normalize=normalize)
    assert r.capacity == cap
    recv = moe_dispatch(xc, r).view(E, cap, d)
    out = torch.stack([e(recv[i]) for i, e in enumerate(m.experts)])
    yc = moe_combine(out.reshape(E * cap, d), r)
    gc = torch.autograd.grad((yc * g).sum() + 0.3 * r.aux_loss,
                             [xc, m.gate.weight, m.experts[1].w1.weight])
    assert torch.equal(ya, yc)
    assert torch.equal(m.aux_loss, r.aux_loss)
    for a, c in zip(ga, gc):
        assert torch.equal(a, c)
    none_kept = (r.slot < 0).all(dim=1)
    if capacity_factor == 0.25:
        assert none_kept.any()
    assert (ya[none_kept] == 0).all()


def test_moemlp_defaults_are_untouched():
    """The new keyword arguments at their defaults change nothing, on either
    of the two existing code paths."""
    d, E, T = 32, 4, 60
    torch.manual_seed(1)
    x = torch.randn(T, d)
    for fused in (True, False):
        a = _moe(E, d, fused_routing=fused)
        b = _moe(E, d, fused_routing=fused, top_k=1, normalize_gates=True,
                 balance_loss=False)
        b.load_state_dict(a.state_dict())
        xa, xb = (x.clone().requires_grad_(True) for _ in range(2))
        ya, yb = a(xa), b(xb)
        ya.sum().backward()
        yb.sum().backward()
        assert torch.equal(ya, yb) and torch.equal(xa.grad, xb.grad)
        assert torch.equal(a.gate.weight.grad, b.gate.weight.grad)
        assert a.aux_loss is None and b.aux_loss is None


def test_moemlp_top1_with_balance_loss():
    d, E, T = 32, 4, 60
    a = _moe(E, d)
    b = _moe(E, d, balance_loss=True)
    b.load_state_dict(a.state_dict())
    torch.manual_seed(1)
    x = torch.randn(T, d)
    torch.testing.assert_close(b(x), a(x), rtol=1e-5, atol=1e-5)
    cap = max(1, math.ceil(T / E * 1.25))
    assert torch.equal(b.aux_loss,
                       moe_route_topk(b.gate(x), 1, cap).aux_loss)


def test_transformer_block_passes_the_arguments_through():
    torch.manual_seed(0)
    blk = MoETransformerBlock(d_model=32, n_head=4, d_hidden=64,
                              num_local_experts=4, world_size=1, top_k=2,
                              normalize_gates=False, balance_loss=True)
    assert blk.moe.top_k == 2 and not blk.moe.normalize_gates
    y = blk(torch.randn(2, 12, 32))
    (y.mean() + blk.moe.aux_loss).backward()
    assert blk.moe.gate.weight.grad is not None


def _moe_top2_ep_matches_local(rank, world):
    os.environ["ADAPCC_TRANSPORT"] = "pg"
    import torch.distributed as dist

    from adapcc_amd import AdapCC, CommArgs

    AdapCC.init(CommArgs(entry_point=-1), rank, rank, world)
    AdapCC.setup()
    comm = AdapCC.communicator

    d, local_e = 16, 2
    kw = dict(capacity_factor=4.0, top_k=2, balance_loss=True)
    torch.manual_seed(123 + rank)  # per-rank expert weights differ
    dist_moe = MoEMLP(d_model=d, d_hidden=32, num_local_experts=local_e,
                      comm=comm, world_size=world, rank=rank, **kw)
    torch.manual_seed(55)  # same gate everywhere
    with torch.no_grad():
        gate_w = torch.randn_like(dist_moe.gate.weight)
        dist_moe.gate.weight.copy_(gate_w)

    # the equivalent single-process layer holding all experts rank-major
    states = [None] * world
    dist.all_gather_object(
        states,
        {k: v.clone() for k, v in dist_moe.experts.state_dict().items()})
    local = MoEMLP(d_model=d, d_hidden=32, num_local_experts=world * local_e,
                   world_size=1, **kw)
    with torch.no_grad():
        local.gate.weight.copy_(gate_w)
        for r in range(world):
            for i in range(local_e):
                local.experts[r * local_e + i].load_state_dict(
                    {k[len(f"{i}."):]: v for k, v in states[r].items()
                     if k.startswith(f"{i}.")})

    torch.manual_seed(777 + rank)  # per-rank batch
    x = torch.randn(4, 8, d)
    y_dist = dist_moe(x)
    y_local = local(x)
    # capacity_factor=4 with two choices per token: nothing overflows, so
    # the token order inside an expert cannot matter
    cap = math.ceil(2 * 32 / (world * local_e) * 4.0)
    routing = moe_route_topk(local.gate(x.reshape(-1, d)), 2, cap)
    assert (routing.slot >= 0).all()
    assert torch.allclose(y_dist, y_local, atol=1e-5), (
        (y_dist - y_local).abs().max())
    assert torch.allclose(dist_moe.aux_loss, local.aux_loss, atol=1e-6)
    (y_dist.sum() + dist_moe.aux_loss).backward()
    AdapCC.clear()
    return True


def test_moe_top2_ep_matches_local_world2():
    assert all(run_mp(_moe_top2_ep_matches_local, 2, backend="gloo",
                      timeout=180))
