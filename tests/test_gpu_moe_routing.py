"""Top-1 MoE routing, dispatch and combine kernels (csrc/moe.hip) against
references written here in numpy/torch on the CPU."""

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

DTYPES = [torch.float32, torch.float16, torch.bfloat16]
ROUTE_CASES = [(1, 1, 1), (63, 3, 5), (64, 16, 5), (65, 16, 1),
               (257, 10, 33), (4097, 64, 81), (1000, 256, 4)]
# routing cases with empty slots and dropped tokens, for the row kernels
MOVE_CASES = [(64, 16, 5), (65, 16, 1), (1000, 256, 4)]
WIDTHS = [8, 24, 64, 1024]


def _logits(T, E, dtype):
    torch.manual_seed(0)
    return (torch.randn(T, E) * 2).to(dtype)


def route_reference(logits_cpu, cap):
    """(gate_p fp64, expert, slot, src) from the upcast logits: np.argmax
    takes the first maximum, a running count gives the stable position."""
    x = logits_cpu.double().numpy()
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


_REF = {}


def _case(T, E, cap, dtype):
    """CPU logits and their reference routing, computed once per case."""
    key = (T, E, cap, dtype)
    if key not in _REF:
        lg = _logits(T, E, dtype)
        _REF[key] = (lg,) + route_reference(lg, cap)
    return _REF[key]


def _route(logits_cpu, cap):
    from adapcc_amd.ops import moe

    lg = logits_cpu.cuda()
    assert moe._route_fusable(lg, cap)
    return moe.moe_route_top1(lg, cap)


def _assert_routing(r, expert, slot, src):
    assert r.expert.dtype == r.slot.dtype == r.src.dtype == torch.int32
    assert np.array_equal(r.expert.cpu().numpy(), expert)
    assert np.array_equal(r.slot.cpu().numpy(), slot)
    assert np.array_equal(r.src.cpu().numpy(), src)


# ---------------------------------------------------------------- routing

@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("T,E,cap", ROUTE_CASES)
def test_routing_is_exact(T, E, cap, dtype):
    lg, gate_p, expert, slot, src = _case(T, E, cap, dtype)
    r = _route(lg, cap)
    _assert_routing(r, expert, slot, src)
    assert r.gate_p.dtype == torch.float32
    tol = 1e-5
    np.testing.assert_allclose(r.gate_p.cpu().numpy(), gate_p, rtol=tol,
                               atol=tol)
    # same call again: bit-identical outputs
    r2 = _route(lg, cap)
    for a, b in zip(r[:4], r2[:4]):
        assert torch.equal(a, b)


def test_routing_all_logits_equal():
    T, E, cap = 300, 7, 9
    r = _route(torch.full((T, E), 0.25), cap)
    assert (r.expert == 0).all()
    want_slot = np.full(T, -1)
    want_slot[:cap] = np.arange(cap)
    want_src = np.full(E * cap, -1)
    want_src[:cap] = np.arange(cap)
    _assert_routing(r, np.zeros(T, dtype=np.int64), want_slot, want_src)
    np.testing.assert_allclose(r.gate_p.cpu().numpy(), 1.0 / E, rtol=1e-6)


def test_routing_all_tokens_prefer_one_expert():
    T, E, cap, fav = 700, 5, 4, 3
    torch.manual_seed(0)
    lg = torch.randn(T, E)
    lg[:, fav] += 20.0
    r = _route(lg, cap)
    assert (r.expert == fav).all()
    slot = r.slot.cpu().numpy()
    assert np.array_equal(slot[:cap], fav * cap + np.arange(cap))
    assert (slot[cap:] == -1).all()
    src = r.src.cpu().numpy().reshape(E, cap)
    assert np.array_equal(src[fav], np.arange(cap))
    assert (np.delete(src, fav, axis=0) == -1).all()


def test_routing_writes_every_output_element():
    """Poisoned outputs through the launch helper: nothing is left over."""
    from adapcc_amd.ops import moe

    T, E, cap = 257, 10, 33
    lg, gate_p, expert, slot, src = _case(T, E, cap, torch.float32)
    g = torch.full((T,), float("nan"), device="cuda")
    e = torch.full((T,), -7, dtype=torch.int32, device="cuda")
    s = torch.full((T,), -7, dtype=torch.int32, device="cuda")
    sr = torch.full((E * cap,), -7, dtype=torch.int32, device="cuda")
    moe._launch_route(lg.cuda(), cap, g, e, s, sr)
    assert np.array_equal(e.cpu().numpy(), expert)
    assert np.array_equal(s.cpu().numpy(), slot)
    assert np.array_equal(sr.cpu().numpy(), src)
    assert not torch.isnan(g).any()


@pytest.mark.parametrize("dtype,tol", [(torch.float32, 1e-5),
                                       (torch.bfloat16, 2e-2),
                                       (torch.float16, 1e-2)])
@pytest.mark.parametrize("T,E,cap", [(64, 16, 5), (65, 16, 1),
                                     (4097, 64, 81), (1000, 256, 4)])
def test_dlogits_matches_reference(T, E, cap, dtype, tol):
    from adapcc_amd.ops import moe

    lg, gate_p, expert, slot, _ = _case(T, E, cap, dtype)
    torch.manual_seed(2)
    dgate = torch.randn(T)
    ref_dt = torch.float64 if dtype == torch.float32 else torch.float32
    x = lg.to(ref_dt).requires_grad_(True)
    p = x.softmax(-1).gather(1, torch.from_numpy(expert)[:, None]).squeeze(1)
    kept = torch.from_numpy(slot >= 0)
    (p * dgate.to(ref_dt) * kept).sum().backward()

    lg_g = lg.cuda().requires_grad_(True)
    r = moe.moe_route_top1(lg_g, cap)
    r.gate_p.backward(dgate.cuda())
    got = lg_g.grad
    assert got.dtype == dtype
    torch.testing.assert_close(got.cpu().to(ref_dt), x.grad, rtol=tol,
                               atol=tol)
    assert (slot < 0).any()
    assert (got[(~kept).cuda()] == 0).all()


# ------------------------------------------------------------ row movement

@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("d", WIDTHS)
@pytest.mark.parametrize("T,E,cap", MOVE_CASES)
def test_dispatch_is_a_bit_exact_copy(T, E, cap, d, dtype):
    from adapcc_amd.ops import moe

    lg, _, _, slot, src = _case(T, E, cap, torch.float32)
    assert (slot < 0).any() and (src < 0).any()
    r = _route(lg, cap)
    torch.manual_seed(3)
    x = torch.randn(T, d).to(dtype)
    gd = torch.randn(E * cap, d).to(dtype)
    slot_t, src_t = torch.from_numpy(slot), torch.from_numpy(src)
    want = torch.zeros(E * cap, d, dtype=dtype)
    want[src_t >= 0] = x[src_t[src_t >= 0]]
    want_dx = torch.zeros(T, d, dtype=dtype)
    want_dx[slot_t >= 0] = gd[slot_t[slot_t >= 0]]

    # forward and backward into NaN-filled outputs
    xg, gdg = x.cuda(), gd.cuda()
    assert moe._rows_fusable(xg)
    out = torch.full((E * cap, d), float("nan"), dtype=dtype, device="cuda")
    moe._launch_gather(xg, r.src, out)
    dx = torch.full((T, d), float("nan"), dtype=dtype, device="cuda")
    moe._launch_gather(gdg, r.slot, dx)
    for got, ref, empty in ((out, want, src_t < 0), (dx, want_dx, slot_t < 0)):
        got = got.cpu()
        assert not torch.isnan(got).any()
        assert (got[empty] == 0).all()
        assert torch.equal(got.view(torch.uint8), ref.view(torch.uint8))

    # and through autograd
    xg.requires_grad_(True)
    y = moe.moe_dispatch(xg, r)
    y.backward(gdg)
    assert torch.equal(y.cpu().view(torch.uint8), want.view(torch.uint8))
    assert torch.equal(xg.grad.cpu().view(torch.uint8),
                       want_dx.view(torch.uint8))


@pytest.mark.parametrize("dtype,rtol", [(torch.float32, 1e-5),
                                        (torch.bfloat16, 2 ** -8),
                                        (torch.float16, 2 ** -10)])
@pytest.mark.parametrize("d", WIDTHS)
@pytest.mark.parametrize("T,E,cap", MOVE_CASES)
def test_combine_scaled_movement(T, E, cap, d, dtype, rtol):
    """Against the fp32 product of the same inputs: one fp32 multiply and
    one rounding leave at most half an ulp of the output dtype."""
    from adapcc_amd.ops import moe

    lg, _, _, slot, src = _case(T, E, cap, torch.float32)
    r = _route(lg, cap)
    torch.manual_seed(4)
    back = torch.randn(E * cap, d).to(dtype)
    dy = torch.randn(T, d).to(dtype)
    gp = r.gate_p.cpu()  # the scale the kernels are given
    slot_t, src_t = torch.from_numpy(slot), torch.from_numpy(src)
    kept, filled = slot_t >= 0, src_t >= 0
    want_y = torch.zeros(T, d)
    want_y[kept] = back.float()[slot_t[kept]] * gp[kept, None]
    want_db = torch.zeros(E * cap, d)
    want_db[filled] = dy.float()[src_t[filled]] * gp[src_t[filled], None]

    bg, dyg = back.cuda(), dy.cuda()
    y = torch.full((T, d), float("nan"), dtype=dtype, device="cuda")
    moe._launch_gather(bg, r.slot, y, scale=r.gate_p)
    db = torch.full((E * cap, d), float("nan"), dtype=dtype, device="cuda")
    moe._launch_gather(dyg, r.src, db, scale=r.gate_p, scale_by_src=True)
    for got, ref, empty in ((y, want_y, ~kept), (db, want_db, ~filled)):
        got = got.cpu()
        assert not torch.isnan(got).any()
        assert (got[empty] == 0).all()
        torch.testing.assert_close(got.float(), ref, rtol=rtol, atol=1e-6)

    bg.requires_grad_(True)
    y2 = moe.moe_combine(bg, r)
    y2.backward(dyg)
    assert torch.equal(y2, y) and torch.equal(bg.grad, db)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("d", [64, 1024])
def test_dgate_p_accuracy(d, dtype):
    """|kernel - fp64| <= 4 * |torch fp32 sum - fp64| over a few thousand
    rows: the two differ only in summation order."""
    from adapcc_amd.ops import moe

    T, E, cap = 4097, 64, 81
    lg, _, _, slot, _ = _case(T, E, cap, torch.float32)
    r = _route(lg, cap)
    torch.manual_seed(5)
    back = torch.randn(E * cap, d).to(dtype)
    dy = torch.randn(T, d).to(dtype)
    slot_t = torch.from_numpy(slot)
    kept = slot_t >= 0
    rows = back[slot_t.clamp(min=0)]
    want = (dy.double() * rows.double()).sum(-1) * kept
    torch_f32 = (dy.float() * rows.float()).sum(-1) * kept

    got = torch.full((T,), float("nan"), device="cuda")
    moe._launch_rowdot(dy.cuda(), back.cuda(), r.slot, got)
    got = got.cpu()
    assert not torch.isnan(got).any()
    assert (~kept).any() and (got[~kept] == 0).all()
    err = (got.double() - want).abs().max().item()
    err_torch = (torch_f32.double() - want).abs().max().item()
    assert err <= 4 * err_torch, (
        f"kernel max abs err {err:.3e} vs torch fp32 {err_torch:.3e}")

    # the autograd path hands the same numbers to gate_p
    gp = r.gate_p.detach().requires_grad_(True)
    y = moe.moe_combine(back.cuda(), r._replace(gate_p=gp))
    y.backward(dy.cuda())
    assert torch.equal(gp.grad.cpu(), got)


# ------------------------------------------------------------ module level

def _moe_pair(d, E, **kw):
    from adapcc_amd.models.moe import MoEMLP

    torch.manual_seed(0)
    a = MoEMLP(d_model=d, d_hidden=2 * d, num_local_experts=E, world_size=1,
               fused_routing=True, **kw).cuda()
    b = MoEMLP(d_model=d, d_hidden=2 * d, num_local_experts=E, world_size=1,
               fused_routing=False, **kw).cuda()
    b.load_state_dict(a.state_dict())
    return a, b


@pytest.mark.parametrize("capacity_factor", [1.25, 0.5])
def test_moemlp_fused_matches_unfused_fp32(capacity_factor):
    d, E, T = 64, 4, 128
    a, b = _moe_pair(d, E, capacity_factor=capacity_factor)
    torch.manual_seed(1)
    x = torch.randn(T, d, device="cuda")
    top2 = a.gate(x).detach().topk(2, dim=-1).values
    gap = (top2[:, 0] - top2[:, 1]).min().item()
    assert gap > 1e-5, f"precondition: top-2 logit gap {gap:.3e}"

    xa, xb = (x.clone().requires_grad_(True) for _ in range(2))
    ya, yb = a(xa), b(xb)
    g = torch.randn_like(ya)
    (ya * g).sum().backward()
    (yb * g).sum().backward()
    torch.testing.assert_close(ya, yb, rtol=1e-5, atol=1e-5)
    torch.testing.assert_close(xa.grad, xb.grad, rtol=1e-5, atol=1e-5)
    for (n, pa), (_, pb) in zip(a.named_parameters(), b.named_parameters()):
        assert pa.grad is not None, n
        torch.testing.assert_close(pa.grad, pb.grad, rtol=1e-5, atol=1e-5,
                                   msg=lambda m, n=n: f"{n}: {m}")


def test_moemlp_runs_the_native_kernels():
    """The GPU path must run the HIP kernels, not silently fall back."""
    from adapcc_amd.ops import fused, moe

    assert fused._core(), "native _core.so missing on a GPU box"
    called = set()
    fns = (moe._RouteFn, moe._DispatchFn, moe._CombineFn)
    origs = [(f, f.forward, f.backward) for f in fns]

    def spy(name, fn):
        def wrapped(ctx, *a, **k):
            called.add(name)
            return fn(ctx, *a, **k)
        return staticmethod(wrapped)

    try:
        for f, fwd, bwd in origs:
            f.forward = spy(f.__name__ + ".forward", fwd)
            f.backward = spy(f.__name__ + ".backward", bwd)
        a, _ = _moe_pair(64, 4)
        x = torch.randn(128, 64, device="cuda", requires_grad=True)
        assert moe.moe_fusable(x, a.gate(x))
        a(x).sum().backward()
    finally:
        for f, fwd, bwd in origs:
            f.forward, f.backward = fwd, bwd
    assert called == {f.__name__ + s for f in fns
                      for s in (".forward", ".backward")}, called


def test_route_dispatch_combine_captures_into_a_graph():
    """No host sync anywhere: forward and backward capture on one stream
    and replay on new inputs."""
    from adapcc_amd.ops import moe

    T, E, d, cap = 300, 8, 64, 40
    torch.manual_seed(6)
    x_s = torch.randn(T, d, device="cuda", requires_grad=True)
    lg_s = torch.randn(T, E, device="cuda", requires_grad=True)

    def step(x, lg):
        r = moe.moe_route_top1(lg, cap)
        back = torch.tanh(moe.moe_dispatch(x, r)) * 1.5  # "the experts"
        y = moe.moe_combine(back, r)
        gx, gl = torch.autograd.grad((y * y).sum(), [x, lg])
        return y, gx, gl, r.slot

    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        for _ in range(2):
            step(x_s, lg_s)
    torch.cuda.current_stream().wait_stream(side)

    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        outs = step(x_s, lg_s)

    for seed in (7, 8):
        torch.manual_seed(seed)
        x_n = torch.randn(T, d, device="cuda")
        lg_n = torch.randn(T, E, device="cuda") * 2
        with torch.no_grad():
            x_s.copy_(x_n)
            lg_s.copy_(lg_n)
        graph.replay()
        want = step(x_n.requires_grad_(True), lg_n.requires_grad_(True))
        assert (want[3] < 0).any()
        for got, ref in zip(outs, want):
            assert torch.equal(got, ref)
