"""Top-k MoE routing, balance loss, dispatch and combine kernels
(csrc/moe.hip) against references written here in numpy/torch on the CPU."""

import numpy as np
import pytest
import torch

from adapcc_amd.ops.moe import RoutingTopK

pytestmark = pytest.mark.gpu

DTYPES = [torch.float32, torch.float16, torch.bfloat16]
ROUTE_CASES = [(2, 2, 1), (3, 2, 1), (63, 3, 5), (64, 16, 5), (65, 16, 1),
               (257, 10, 33), (4097, 64, 81), (1000, 256, 4)]
# routing cases with every capacity outcome, for the row kernels
MOVE_CASES = [(64, 16, 5), (1000, 256, 4), (1000, 256, 12)]
WIDTHS = [8, 24, 64, 1024]
COMBINE_TOL = [(torch.float32, 1e-5), (torch.bfloat16, 2 ** -8),
               (torch.float16, 2 ** -10)]


def _logits(T, E, dtype):
    torch.manual_seed(0)
    return (torch.randn(T, E) * 2).to(dtype)


def route_reference(logits_cpu, cap):
    """Top-2 routing from the fp64-upcast logits: np.argmax takes the first
    maximum, the second choice is the argmax with the first masked out, one
    running count per expert over all first and then all second choices gives
    the position. Gates in both normalisations."""
    x = logits_cpu.double().numpy()
    T, E = x.shape
    rows = np.arange(T)
    e0 = np.argmax(x, axis=1)
    masked = x.copy()
    masked[rows, e0] = -np.inf
    e1 = np.argmax(masked, axis=1)
    expert = np.stack([e0, e1], axis=1)
    z = np.exp(x - x.max(axis=1, keepdims=True))
    p = z / z.sum(axis=1, keepdims=True)
    r = np.exp(x[rows, e1] - x[rows, e0])
    g0 = 1.0 / (1.0 + r)
    slot = np.full((T, 2), -1, dtype=np.int64)
    src = np.full(E * cap, -1, dtype=np.int64)
    src_choice = np.full(E * cap, -1, dtype=np.int64)
    seen = np.zeros(E, dtype=np.int64)
    for c in range(2):
        for t in range(T):
            e = expert[t, c]
            if seen[e] < cap:
                slot[t, c] = e * cap + seen[e]
                src[slot[t, c]] = t
                src_choice[slot[t, c]] = c
            seen[e] += 1
    load = np.bincount(e0, minlength=E)
    aux = E * float(((load / T) * p.mean(axis=0)).sum())
    return dict(gate_norm=np.stack([g0, r * g0], axis=1),
                gate_raw=p[rows[:, None], expert], expert=expert, slot=slot,
                src=src, src_choice=src_choice, load=load, aux=aux)


_REF = {}


def _case(T, E, cap, dtype=torch.float32):
    """CPU logits and their reference routing, computed once per case."""
    key = (T, E, cap, dtype)
    if key not in _REF:
        lg = _logits(T, E, dtype)
        _REF[key] = (lg, route_reference(lg, cap))
    return _REF[key]


def _route(logits_cpu, cap, k=2, normalize=True):
    from adapcc_amd.ops import moe

    lg = logits_cpu.cuda()
    assert moe._route_fusable(lg, cap, k)
    return moe.moe_route_topk(lg, k, cap, normalize=normalize)


def _assert_ints(r, ref):
    for name in ("expert", "slot", "src", "src_choice", "load"):
        got = getattr(r, name)
        assert got.dtype == torch.int32, name
        assert np.array_equal(got.cpu().numpy(), ref[name]), name


def _assert_all_outcomes(ref):
    kept = ref["slot"] >= 0
    assert (~kept[:, 0] & kept[:, 1]).any()
    assert (kept[:, 0] & ~kept[:, 1]).any()
    assert (~kept[:, 0] & ~kept[:, 1]).any()
    assert (ref["src"] < 0).any()


# ---------------------------------------------------------------- routing

@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("T,E,cap", ROUTE_CASES)
def test_routing_is_exact(T, E, cap, dtype):
    lg, ref = _case(T, E, cap, dtype)
    if (T, E, cap) in ((64, 16, 5), (1000, 256, 4)):
        _assert_all_outcomes(ref)
    if dtype == torch.bfloat16 and (T, E, cap) in ((4097, 64, 81),
                                                   (1000, 256, 4)):
        top3 = lg.float().topk(3, dim=-1).values
        assert (top3[:, 0] == top3[:, 1]).sum() >= 12
        assert (top3[:, 1] == top3[:, 2]).sum() >= 12
    for normalize in (True, False):
        r = _route(lg, cap, normalize=normalize)
        assert isinstance(r, RoutingTopK)
        assert (r.capacity, r.num_experts, r.k) == (cap, E, 2)
        _assert_ints(r, ref)
        assert r.gate.dtype == torch.float32 and r.gate.shape == (T, 2)
        want = ref["gate_norm" if normalize else "gate_raw"]
        np.testing.assert_allclose(r.gate.cpu().numpy(), want, rtol=1e-5,
                                   atol=1e-5)
        assert r.aux_loss.dtype == torch.float32 and r.aux_loss.dim() == 0
        np.testing.assert_allclose(r.aux_loss.item(), ref["aux"], rtol=1e-4)
        # same call again: bit-identical outputs, the loss included
        r2 = _route(lg, cap, normalize=normalize)
        for a, b in zip(r[:7], r2[:7]):
            assert torch.equal(a, b)


def test_routing_all_logits_equal():
    T, E, cap = 512, 8, 600
    r = _route(torch.full((T, E), 0.25), cap)
    assert (r.expert[:, 0] == 0).all() and (r.expert[:, 1] == 1).all()
    assert torch.equal(r.gate.cpu(), torch.full((T, 2), 0.5))
    assert r.load.tolist() == [T] + [0] * (E - 1)
    assert r.aux_loss.item() == 1.0
    assert torch.equal(r.slot[:, 0].cpu(), torch.arange(T, dtype=torch.int32))
    assert torch.equal(r.slot[:, 1].cpu(),
                       cap + torch.arange(T, dtype=torch.int32))


def test_second_choices_queue_behind_all_first_choices():
    """Everybody wants expert 3 first and expert 1 second; expert 1 is also
    the first choice of nobody, so its queue holds second choices only."""
    T, E, cap = 700, 5, 4
    torch.manual_seed(0)
    lg = torch.randn(T, E)
    lg[:, 3] += 40.0
    lg[:, 1] += 20.0
    r = _route(lg, cap)
    slot = r.slot.cpu().numpy()
    assert np.array_equal(slot[:cap, 0], 3 * cap + np.arange(cap))
    assert np.array_equal(slot[:cap, 1], 1 * cap + np.arange(cap))
    assert (slot[cap:] == -1).all()
    src = r.src.cpu().numpy().reshape(E, cap)
    ch = r.src_choice.cpu().numpy().reshape(E, cap)
    assert np.array_equal(src[3], np.arange(cap)) and (ch[3] == 0).all()
    assert np.array_equal(src[1], np.arange(cap)) and (ch[1] == 1).all()
    assert (np.delete(src, [1, 3], axis=0) == -1).all()
    assert (np.delete(ch, [1, 3], axis=0) == -1).all()
    np.testing.assert_allclose(r.aux_loss.item(), float(E), rtol=1e-5)


@pytest.mark.parametrize("k", [1, 2])
def test_routing_writes_every_output_element(k):
    """Poisoned outputs through the launch helper: nothing is left over."""
    from adapcc_amd.ops import moe

    T, E, cap = 1000, 256, 12
    lg, ref = _case(T, E, cap)
    assert (ref["src"] < 0).any() and (ref["slot"] < 0).any()
    dev = "cuda"
    gate = torch.full((T, k), float("nan"), device=dev)
    pmax = torch.full((T,), float("nan"), device=dev)
    ints = {n: torch.full(s, -7, dtype=torch.int32, device=dev)
            for n, s in (("expert", (T, k)), ("slot", (T, k)),
                         ("src", (E * cap,)), ("src_choice", (E * cap,)),
                         ("load", (E,)))}
    aux = torch.full((), float("nan"), device=dev)
    moe._launch_route_topk(lg.cuda(), k, cap, True, gate, pmax,
                           ints["expert"], ints["slot"], ints["src"],
                           ints["src_choice"], ints["load"], aux)
    assert not torch.isnan(gate).any() and not torch.isnan(pmax).any()
    assert not torch.isnan(aux).any()
    if k == 2:
        for n, t in ints.items():
            assert np.array_equal(t.cpu().numpy(), ref[n]), n
    else:
        for t in ints.values():
            assert (t >= -1).all()
        assert np.array_equal(ints["load"].cpu().numpy(), ref["load"])


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("T,E,cap", ROUTE_CASES)
def test_k1_is_bit_equal_to_the_top1_kernels(T, E, cap, dtype):
    from adapcc_amd.ops import moe

    lg, ref = _case(T, E, cap, dtype)
    r = _route(lg, cap, k=1)
    r1 = moe.moe_route_top1(lg.cuda(), cap)
    assert r.gate.shape == r.expert.shape == r.slot.shape == (T, 1)
    assert torch.equal(r.gate[:, 0], r1.gate_p)
    assert torch.equal(r.expert[:, 0], r1.expert)
    assert torch.equal(r.slot[:, 0], r1.slot)
    assert torch.equal(r.src, r1.src)
    assert torch.equal(r.src_choice, torch.where(r1.src >= 0, 0, -1).int())
    assert np.array_equal(r.load.cpu().numpy(), ref["load"])
    np.testing.assert_allclose(r.aux_loss.item(), ref["aux"], rtol=1e-4)


def _dlogits_reference(lg, ref, normalize, dgate, daux, ref_dt, k=2):
    """Autograd through the contract written with the reference's integer
    outputs: dropped choices take no gradient, the loss differentiates
    through the mean probabilities only."""
    T, E = lg.shape
    x = lg.to(ref_dt).requires_grad_(True)
    expert = torch.from_numpy(ref["expert"])[:, :k]
    kept = torch.from_numpy(ref["slot"] >= 0)[:, :k]
    p = x.softmax(-1)
    if k == 2 and normalize:
        gate = x.gather(1, expert).softmax(-1)
    else:
        gate = p.gather(1, expert)
    loss = (gate * dgate.to(ref_dt) * kept).sum()
    if daux is not None:
        load = torch.from_numpy(ref["load"]).to(ref_dt)
        loss = loss + daux * E * ((load / T) * p.mean(0)).sum()
    loss.backward()
    return x.grad


@pytest.mark.parametrize("dtype,tol", [(torch.float32, 1e-5),
                                       (torch.bfloat16, 2e-2),
                                       (torch.float16, 1e-2)])
@pytest.mark.parametrize("normalize", [True, False])
@pytest.mark.parametrize("T,E,cap", [(64, 16, 5), (65, 16, 1),
                                     (4097, 64, 81), (1000, 256, 4)])
def test_dlogits_matches_reference(T, E, cap, normalize, dtype, tol):
    from adapcc_amd.ops import moe

    lg, ref = _case(T, E, cap, dtype)
    kept = torch.from_numpy(ref["slot"] >= 0)
    assert (~kept).any()
    torch.manual_seed(2)
    dgate = torch.randn(T, 2)
    ref_dt = torch.float64 if dtype == torch.float32 else torch.float32
    # a large weight on the loss, so its term is not lost next to the gates'
    for daux in (None, 0.5 * T):
        want = _dlogits_reference(lg, ref, normalize, dgate, daux, ref_dt)
        lg_g = lg.cuda().requires_grad_(True)
        r = moe.moe_route_topk(lg_g, 2, cap, normalize=normalize)
        loss = (r.gate * dgate.cuda()).sum()
        if daux is not None:
            loss = loss + daux * r.aux_loss
        loss.backward()
        got = lg_g.grad
        assert got.dtype == dtype
        torch.testing.assert_close(got.cpu().to(ref_dt), want, rtol=tol,
                                   atol=tol)
        if daux is None:
            none_kept = ~kept.any(dim=1)
            if (T, E, cap) != (4097, 64, 81):
                assert none_kept.any()
            assert (got[none_kept.cuda()] == 0).all()
    # the loss alone: the gate output receives no gradient at all
    want = _dlogits_reference(lg, ref, normalize, torch.zeros(T, 2), 1.0 * T,
                              ref_dt)
    lg_g = lg.cuda().requires_grad_(True)
    r = moe.moe_route_topk(lg_g, 2, cap, normalize=normalize)
    (r.aux_loss * float(T)).backward()
    torch.testing.assert_close(lg_g.grad.cpu().to(ref_dt), want, rtol=tol,
                               atol=tol)


def test_dlogits_k1_with_the_loss():
    from adapcc_amd.ops import moe

    T, E, cap = 1000, 256, 4
    lg, ref = _case(T, E, cap)
    ref1 = route_reference_k1(lg, ref, cap)
    torch.manual_seed(2)
    dgate = torch.randn(T, 1)
    want = _dlogits_reference(lg, ref1, True, dgate, 0.5 * T, torch.float64,
                              k=1)
    lg_g = lg.cuda().requires_grad_(True)
    r = moe.moe_route_topk(lg_g, 1, cap)
    ((r.gate * dgate.cuda()).sum() + 0.5 * T * r.aux_loss).backward()
    torch.testing.assert_close(lg_g.grad.cpu().double(), want, rtol=1e-5,
                               atol=1e-5)


def route_reference_k1(lg, ref, cap):
    """The k=1 slots of the same logits (first choices rank alone)."""
    T, E = lg.shape
    slot = np.full((T, 1), -1, dtype=np.int64)
    seen = np.zeros(E, dtype=np.int64)
    for t in range(T):
        e = ref["expert"][t, 0]
        if seen[e] < cap:
            slot[t, 0] = e * cap + seen[e]
        seen[e] += 1
    return dict(expert=ref["expert"], slot=slot, load=ref["load"])


# ------------------------------------------------------------ row movement

def _sum_rows(rows_of, index, n, d):
    """fp64 sum over the two choices of rows_of[index[:, c]], skipping -1."""
    out = torch.zeros(n, d, dtype=torch.float64)
    for c in range(2):
        kc = index[:, c] >= 0
        out[kc] += rows_of.double()[index[kc, c]]
    return out


@pytest.mark.parametrize("dtype,rtol", COMBINE_TOL)
@pytest.mark.parametrize("d", WIDTHS)
@pytest.mark.parametrize("T,E,cap", MOVE_CASES)
def test_dispatch_is_a_bit_exact_copy(T, E, cap, d, dtype, rtol):
    from adapcc_amd.ops import moe

    lg, ref = _case(T, E, cap)
    if cap != 12:
        _assert_all_outcomes(ref)
    assert (ref["src"] < 0).any() and (ref["slot"] < 0).any()
    r = _route(lg, cap)
    torch.manual_seed(3)
    x = torch.randn(T, d).to(dtype)
    gd = torch.randn(E * cap, d).to(dtype)
    slot_t, src_t = torch.from_numpy(ref["slot"]), torch.from_numpy(ref["src"])
    want = torch.zeros(E * cap, d, dtype=dtype)
    want[src_t >= 0] = x[src_t[src_t >= 0]]
    want_dx = _sum_rows(gd, slot_t, T, d)
    none_kept = (slot_t < 0).all(dim=1)
    one_kept = (slot_t >= 0).sum(dim=1) == 1

    # forward and backward into NaN-filled outputs
    xg, gdg = x.cuda(), gd.cuda()
    assert moe._rows_fusable(xg)
    out = torch.full((E * cap, d), float("nan"), dtype=dtype, device="cuda")
    moe._launch_gather(xg, r.src, out)
    dx = torch.full((T, d), float("nan"), dtype=dtype, device="cuda")
    moe._launch_gather2(gdg, r.slot, dx)
    out, dx = out.cpu(), dx.cpu()
    assert not torch.isnan(out).any() and not torch.isnan(dx).any()
    assert torch.equal(out.view(torch.uint8), want.view(torch.uint8))
    assert (dx[none_kept] == 0).all()
    # one source row: a copy; two: their fp32 sum, rounded once
    assert torch.equal(dx[one_kept].view(torch.uint8),
                       want_dx[one_kept].to(dtype).view(torch.uint8))
    if dtype == torch.float32:
        f32 = torch.zeros(T, d)
        for c in range(2):
            kc = slot_t[:, c] >= 0
            f32[kc] += gd[slot_t[kc, c]]
        assert torch.equal(dx, f32)
    torch.testing.assert_close(dx.double(), want_dx, rtol=rtol, atol=1e-5)

    # and through autograd
    xg.requires_grad_(True)
    y = moe.moe_dispatch(xg, r)
    y.backward(gdg)
    assert torch.equal(y.cpu().view(torch.uint8), want.view(torch.uint8))
    assert torch.equal(xg.grad.cpu().view(torch.uint8), dx.view(torch.uint8))


@pytest.mark.parametrize("dtype,rtol", COMBINE_TOL)
@pytest.mark.parametrize("d", WIDTHS)
@pytest.mark.parametrize("T,E,cap", MOVE_CASES)
def test_combine_scaled_movement(T, E, cap, d, dtype, rtol):
    """Against fp64 on the gates the kernels are given: two fp32 roundings
    on terms of magnitude at most about 5, then half an ulp of the output."""
    from adapcc_amd.ops import moe

    lg, ref = _case(T, E, cap)
    r = _route(lg, cap)
    torch.manual_seed(4)
    back = torch.randn(E * cap, d).to(dtype)
    dy = torch.randn(T, d).to(dtype)
    gate = r.gate.cpu().double()
    slot_t, src_t = torch.from_numpy(ref["slot"]), torch.from_numpy(ref["src"])
    ch_t = torch.from_numpy(ref["src_choice"])
    filled = src_t >= 0
    none_kept = (slot_t < 0).all(dim=1)
    want_y = torch.zeros(T, d, dtype=torch.float64)
    for c in range(2):
        kc = slot_t[:, c] >= 0
        want_y[kc] += back.double()[slot_t[kc, c]] * gate[kc, c, None]
    want_db = torch.zeros(E * cap, d, dtype=torch.float64)
    want_db[filled] = (dy.double()[src_t[filled]]
                       * gate[src_t[filled], ch_t[filled], None])

    bg, dyg = back.cuda(), dy.cuda()
    y = torch.full((T, d), float("nan"), dtype=dtype, device="cuda")
    moe._launch_gather2(bg, r.slot, y, scale=r.gate)
    db = torch.full((E * cap, d), float("nan"), dtype=dtype, device="cuda")
    moe._launch_gather(dyg, r.src, db, scale=r.gate, scale_by_src=True,
                       choice=r.src_choice)
    for got, want, empty in ((y, want_y, none_kept), (db, want_db, ~filled)):
        got = got.cpu()
        assert not torch.isnan(got).any()
        assert empty.any() or cap == 12  # few drops there, none of both
        assert (got[empty] == 0).all()
        torch.testing.assert_close(got.double(), want, rtol=rtol, atol=1e-5)

    bg.requires_grad_(True)
    y2 = moe.moe_combine(bg, r)
    y2.backward(dyg)
    assert torch.equal(y2, y) and torch.equal(bg.grad, db)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("d", [64, 1024])
def test_dgate_accuracy(d, dtype):
    """|kernel - fp64| <= 4 * |torch fp32 sum - fp64| over a few thousand
    rows: the two differ only in summation order."""
    from adapcc_amd.ops import moe

    T, E, cap = 4097, 64, 81
    lg, ref = _case(T, E, cap)
    r = _route(lg, cap)
    torch.manual_seed(5)
    back = torch.randn(E * cap, d).to(dtype)
    dy = torch.randn(T, d).to(dtype)
    slot_t = torch.from_numpy(ref["slot"])
    kept = slot_t >= 0
    rows = back[slot_t.clamp(min=0)]  # [T, 2, d]
    want = (dy.double()[:, None] * rows.double()).sum(-1) * kept
    torch_f32 = (dy.float()[:, None] * rows.float()).sum(-1) * kept

    got = torch.full((T, 2), float("nan"), device="cuda")
    moe._launch_rowdot(dy.cuda(), back.cuda(), r.slot, got)
    got = got.cpu()
    assert not torch.isnan(got).any()
    assert (~kept).any() and (got[~kept] == 0).all()
    err = (got.double() - want).abs().max().item()
    err_torch = (torch_f32.double() - want).abs().max().item()
    assert err <= 4 * err_torch, (
        f"kernel max abs err {err:.3e} vs torch fp32 {err_torch:.3e}")

    # the autograd path hands the same numbers to the gate
    gate = r.gate.detach().requires_grad_(True)
    y = moe.moe_combine(back.cuda(), r._replace(gate=gate))
    y.backward(dy.cuda())
    assert torch.equal(gate.grad.cpu(), got)


# ------------------------------------------------------------ module level

def _moe_pair(d, E, **kw):
    from adapcc_amd.models.moe import MoEMLP

    torch.manual_seed(0)
    a = MoEMLP(d_model=d, d_hidden=2 * d, num_local_experts=E, world_size=1,
               fused_routing=True, top_k=2, balance_loss=True, **kw).cuda()
    b = MoEMLP(d_model=d, d_hidden=2 * d, num_local_experts=E, world_size=1,
               fused_routing=False, top_k=2, balance_loss=True, **kw).cuda()
    b.load_state_dict(a.state_dict())
    return a, b


@pytest.mark.parametrize("normalize", [True, False])
@pytest.mark.parametrize("capacity_factor", [1.25, 0.5])
def test_moemlp_fused_matches_unfused_fp32(capacity_factor, normalize):
    d, E, T = 64, 4, 128
    a, b = _moe_pair(d, E, capacity_factor=capacity_factor,
                     normalize_gates=normalize)
    torch.manual_seed(1)
    x = torch.randn(T, d, device="cuda")
    top3 = a.gate(x).detach().topk(3, dim=-1).values
    gap = min((top3[:, 0] - top3[:, 1]).min().item(),
              (top3[:, 1] - top3[:, 2]).min().item())
    assert gap > 1e-5, f"precondition: logit gaps, smallest {gap:.3e}"

    xa, xb = (x.clone().requires_grad_(True) for _ in range(2))
    ya, yb = a(xa), b(xb)
    g = torch.randn_like(ya)
    ((ya * g).sum() + 3.0 * a.aux_loss).backward()
    ((yb * g).sum() + 3.0 * b.aux_loss).backward()
    torch.testing.assert_close(ya, yb, rtol=1e-5, atol=1e-5)
    torch.testing.assert_close(a.aux_loss, b.aux_loss, rtol=1e-5, atol=1e-5)
    torch.testing.assert_close(xa.grad, xb.grad, rtol=1e-5, atol=1e-5)
    for (n, pa), (_, pb) in zip(a.named_parameters(), b.named_parameters()):
        assert pa.grad is not None, n
        torch.testing.assert_close(pa.grad, pb.grad, rtol=1e-5, atol=1e-5,
                                   msg=lambda m, n=n: f"{n}: {m}")
    if capacity_factor == 0.5:
        assert (ya == 0).all(dim=1).any()  # tokens with nothing kept


def test_moemlp_runs_the_native_kernels():
    """The GPU path must run the HIP kernels, not silently fall back."""
    from adapcc_amd.ops import fused, moe

    assert fused._core(), "native _core.so missing on a GPU box"
    called = set()
    fns = (moe._RouteTopKFn, moe._Dispatch2Fn, moe._Combine2Fn)
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
        assert moe.moe_fusable(x, a.gate(x), 80, k=2)
        (a(x).sum() + a.aux_loss).backward()
    finally:
        for f, fwd, bwd in origs:
            f.forward, f.backward = fwd, bwd
    assert called == {f.__name__ + s for f in fns
                      for s in (".forward", ".backward")}, called


def test_route_dispatch_combine_captures_into_a_graph():
    """No host sync anywhere: forward and backward capture on one stream
    and replay on new inputs."""
    from adapcc_amd.ops import moe

    T, E, d, cap = 300, 8, 64, 60
    torch.manual_seed(6)
    x_s = torch.randn(T, d, device="cuda", requires_grad=True)
    lg_s = torch.randn(T, E, device="cuda", requires_grad=True)

    def step(x, lg):
        r = moe.moe_route_topk(lg, 2, cap)
        back = torch.tanh(moe.moe_dispatch(x, r)) * 1.5  # "the experts"
        y = moe.moe_combine(back, r)
        gx, gl = torch.autograd.grad((y * y).sum() + 2.0 * r.aux_loss,
                                     [x, lg])
        return y, gx, gl, r.slot, r.aux_loss, r.load

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
