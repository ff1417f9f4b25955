"""Top-1 MoE routing, dispatch and combine (adapcc_amd/ops/moe.py): the
plain-torch fallback against a reference written here, and the MoEMLP
``fused_routing`` switch on the CPU."""

import math

import numpy as np
import pytest
import torch

from adapcc_amd.models.moe import MoEMLP
from adapcc_amd.ops.moe import (moe_combine, moe_dispatch, moe_fusable,
                                moe_route_top1)

CASES = [(1, 1, 1), (63, 3, 5), (64, 16, 5), (65, 16, 1), (257, 10, 33),
         (4097, 64, 81), (1000, 256, 4)]


def route_reference(logits: torch.Tensor, cap: int):
    """(gate_p fp64, expert, slot, src) from the upcast logits: np.argmax
    takes the first maximum, a running count gives the stable position."""
    x = logits.detach().cpu().double().numpy()
    T, E = x.shape
    expert = np.argmax(x, axis=1)
    z = np.exp(x - x.max(axis=1, keepdims=True))
    gate_p = (z / z.sum(axis=1, keepdims=True))[np.arange(T), expert]
    slot = np.full(T, -1, dtype=np.int64)
    src = np.full(E * cap, -1, dtype=np.int64)
    seen = np.zeros(E, dtype=np.int64)
    for t in range(T):
        e = expert[t]
        if seen[e] < cap:
            slot[t] = e * cap + seen[e]
            src[slot[t]] = t
        seen[e] += 1
    return gate_p, expert, slot, src


def _logits(T, E, dtype=torch.float32):
    torch.manual_seed(0)
    return (torch.randn(T, E) * 2).to(dtype)


@pytest.mark.parametrize("T,E,cap", CASES)
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_fallback_route_matches_reference(T, E, cap, dtype):
    logits = _logits(T, E, dtype)
    r = moe_route_top1(logits, cap)
    gate_p, expert, slot, src = route_reference(logits, cap)
    assert r.capacity == cap and r.num_experts == E
    assert r.expert.dtype == r.slot.dtype == r.src.dtype == torch.int32
    assert r.gate_p.dtype == torch.float32
    assert np.array_equal(r.expert.numpy(), expert)
    assert np.array_equal(r.slot.numpy(), slot)
    assert np.array_equal(r.src.numpy(), src)
    np.testing.assert_allclose(r.gate_p.numpy(), gate_p, rtol=1e-5, atol=1e-5)


def test_fallback_tie_rule_all_equal():
    r = moe_route_top1(torch.zeros(10, 4), 3)
    assert r.expert.tolist() == [0] * 10
    assert r.slot.tolist() == [0, 1, 2] + [-1] * 7
    assert r.src.tolist() == [0, 1, 2] + [-1] * 9


@pytest.mark.parametrize("T,E,cap", CASES)
def test_src_and_slot_are_mutually_inverse(T, E, cap):
    r = moe_route_top1(_logits(T, E), cap)
    slot, src = r.slot.long(), r.src.long()
    kept = (slot >= 0).nonzero().squeeze(1)
    assert torch.equal(src[slot[kept]], kept)
    filled = (src >= 0).nonzero().squeeze(1)
    assert torch.equal(slot[src[filled]], filled)
    assert len(kept) == len(filled)
    assert (slot < E * cap).all() and (src < T).all()


@pytest.mark.parametrize("T,E,cap", [(63, 3, 5), (65, 16, 1), (257, 10, 33)])
def test_fallback_dispatch_combine_match_indexing(T, E, cap):
    d = 24
    logits = _logits(T, E).requires_grad_(True)
    torch.manual_seed(1)
    x = torch.randn(T, d, requires_grad=True)
    back = torch.randn(E * cap, d, requires_grad=True)
    r = moe_route_top1(logits, cap)
    gate_p, _, slot, src = route_reference(logits, cap)
    slot_t, src_t = torch.from_numpy(slot), torch.from_numpy(src)

    disp = moe_dispatch(x, r)
    want = torch.zeros(E * cap, d)
    want[src_t >= 0] = x.detach()[src_t[src_t >= 0]]
    assert torch.equal(disp, want)

    y = moe_combine(back, r)
    want_y = torch.zeros(T, d, dtype=torch.float64)
    kept = slot_t >= 0
    want_y[kept] = (back.detach().double()[slot_t[kept]]
                    * torch.from_numpy(gate_p)[kept, None])
    torch.testing.assert_close(y.double(), want_y, rtol=1e-5, atol=1e-5)
    assert (y[~kept] == 0).all()

    # gradients against the same chain written with plain indexing
    gd, gy = torch.randn_like(disp), torch.randn_like(y)
    (disp * gd).sum().backward(retain_graph=True)
    want_dx = torch.zeros(T, d)
    want_dx[kept] = gd[slot_t[kept]]
    assert torch.equal(x.grad, want_dx)

    (y * gy).sum().backward()
    want_dback = torch.zeros(E * cap, d, dtype=torch.float64)
    want_dback[slot_t[kept]] = (gy.double()[kept]
                                * torch.from_numpy(gate_p)[kept, None])
    torch.testing.assert_close(back.grad.double(), want_dback, rtol=1e-5,
                               atol=1e-5)
    # dlogits = dgate_p * p_max * (onehot - p); zero rows when dropped
    p = logits.detach().double().softmax(-1)
    dgate = torch.zeros(T, dtype=torch.float64)
    dgate[kept] = (gy.double()[kept]
                   * back.detach().double()[slot_t[kept]]).sum(-1)
    onehot = torch.nn.functional.one_hot(r.expert.long(), E).double()
    want_dl = (dgate * torch.from_numpy(gate_p))[:, None] * (onehot - p)
    torch.testing.assert_close(logits.grad.double(), want_dl, rtol=1e-5,
                               atol=1e-5)
    assert (logits.grad[~kept] == 0).all()


def _copy_moe(src_m, **kw):
    m = MoEMLP(d_model=src_m.d_model, d_hidden=src_m.experts[0].w1.out_features,
               num_local_experts=src_m.num_local, world_size=1,
               capacity_factor=src_m.capacity_factor, **kw)
    m.load_state_dict(src_m.state_dict())
    return m


@pytest.mark.parametrize("capacity_factor", [1.25, 0.25])
def test_moemlp_fused_switch_cpu(capacity_factor):
    d, E, T = 32, 4, 60
    torch.manual_seed(0)
    a = MoEMLP(d_model=d, d_hidden=64, num_local_experts=E, world_size=1,
               capacity_factor=capacity_factor, fused_routing=True)
    b = _copy_moe(a, fused_routing=False)
    assert a.fused_routing and not b.fused_routing
    x = torch.randn(T, d)
    xa, xb = (x.clone().requires_grad_(True) for _ in range(2))
    ya, yb = a(xa), b(xb)
    g = torch.randn_like(ya)
    (ya * g).sum().backward()
    (yb * g).sum().backward()
    torch.testing.assert_close(ya, yb, rtol=1e-5, atol=1e-5)
    torch.testing.assert_close(xa.grad, xb.grad, rtol=1e-5, atol=1e-5)
    torch.testing.assert_close(a.gate.weight.grad, b.gate.weight.grad,
                               rtol=1e-5, atol=1e-5)

    cap = max(1, math.ceil(T / E * capacity_factor))
    _, _, slot, _ = route_reference(a.gate(x), cap)
    dropped = torch.from_numpy(slot < 0)
    if capacity_factor == 0.25:
        assert dropped.any()
    assert (ya[dropped] == 0).all()
    assert (xa.grad[dropped] == 0).all()

    # the ops themselves compose to the same layer on the CPU
    xc = x.clone().requires_grad_(True)
    logits = a.gate(xc)
    r = moe_route_top1(logits, cap)
    recv = moe_dispatch(xc, r).view(E, cap, d)
    out = torch.stack([e(recv[i]) for i, e in enumerate(a.experts)])
    yc = moe_combine(out.reshape(E * cap, d), r)
    gw = torch.autograd.grad((yc * g).sum(), [xc, a.gate.weight])
    torch.testing.assert_close(yc, yb, rtol=1e-5, atol=1e-5)
    torch.testing.assert_close(gw[0], xb.grad, rtol=1e-5, atol=1e-5)
    torch.testing.assert_close(gw[1], b.gate.weight.grad, rtol=1e-5,
                               atol=1e-5)
    assert (yc[dropped] == 0).all() and (gw[0][dropped] == 0).all()


def test_moe_fusable_is_false_off_the_fast_path():
    x = torch.randn(64, 32)
    assert not moe_fusable(x, torch.randn(64, 4))          # CPU tensors
    assert not moe_fusable(x, torch.randn(64, 257))        # E = 257
    assert not moe_fusable(torch.randn(64, 7), torch.randn(64, 4))  # d = 7
    if torch.cuda.is_available():
        xg = x.cuda()
        assert not moe_fusable(xg, torch.randn(64, 257, device="cuda"))
        assert not moe_fusable(torch.randn(64, 7, device="cuda"),
                               torch.randn(64, 4, device="cuda"))


def test_fallback_is_anomaly_clean():
    T, E, cap, d = 40, 4, 3, 8
    with torch.autograd.set_detect_anomaly(True):
        logits = _logits(T, E).requires_grad_(True)
        x = torch.randn(T, d, requires_grad=True)
        r = moe_route_top1(logits, cap)
        assert (r.slot < 0).any()
        y = moe_combine(moe_dispatch(x, r) * 2.0, r)
        y.sum().backward()
    assert torch.isfinite(x.grad).all() and torch.isfinite(logits.grad).all()


def test_bad_arguments_raise():
    with pytest.raises(ValueError):
        moe_route_top1(torch.randn(8), 2)
    with pytest.raises(ValueError):
        moe_route_top1(torch.randn(8, 2), 0)
    r = moe_route_top1(torch.randn(8, 2), 4)
    with pytest.raises(ValueError):
        moe_dispatch(torch.randn(9, 4), r)
    with pytest.raises(ValueError):
        moe_combine(torch.randn(9, 4), r)
