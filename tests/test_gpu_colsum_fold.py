"""colsum_fold (csrc/colsum.hip): column sums of up to three [nslots, cols]
fp32 partial arrays in one launch, written in the parameter dtype.

Bound against an fp64 sum of the same fp32 values: one rounding to the output
format (2^-8 relative for bf16, 2^-24 for fp32) plus the worst case of fp32
accumulation in any order, nslots * 2^-24 * sum_i |a_ij|. torch's
sum(0).to(dtype) is held to it too. The kernel's order is fixed: two launches
give the same bits."""

import pytest
import torch

pytestmark = pytest.mark.gpu

NSLOTS = [1, 4, 4096]
COLS = [128, 768, 3072]
OUT = {torch.float32: 2.0 ** -24, torch.bfloat16: 2.0 ** -8}


@pytest.fixture(scope="module")
def base():
    g = torch.Generator(device="cuda").manual_seed(11)
    return torch.randn(3, max(NSLOTS), max(COLS), device="cuda", generator=g)


def _fold(arrays, nslots, cols, dtype):
    import adapcc_amd._core as c

    dt = {torch.float32: c.DTYPE_F32, torch.bfloat16: c.DTYPE_BF16}[dtype]
    outs = [torch.full((cols,), float("nan"), device="cuda", dtype=dtype)
            for _ in arrays]
    pad = [0] * (3 - len(arrays))
    c.colsum_fold(dt, *([a.data_ptr() for a in arrays] + pad),
                  *([o.data_ptr() for o in outs] + pad), nslots, cols,
                  torch.cuda.current_stream().cuda_stream)
    return outs


def _within_bound(got, a, dtype, what):
    nslots = a.shape[0]
    exact = a.double().sum(0)
    bound = OUT[dtype] * exact.abs() + nslots * 2.0 ** -24 * a.double().abs(
    ).sum(0)
    err = (got.double() - exact).abs()
    print(f"{what} {tuple(a.shape)} {dtype}: max err {err.max().item():.3e}, "
          f"max (err - bound) {(err - bound).max().item():.3e}")
    return bool((err <= bound).all())


@pytest.mark.parametrize("dtype", list(OUT), ids=["f32", "bf16"])
@pytest.mark.parametrize("narr", [1, 2, 3])
@pytest.mark.parametrize("cols", COLS)
@pytest.mark.parametrize("nslots", NSLOTS)
def test_fold_within_bound(base, nslots, cols, narr, dtype):
    arrays = [base[i, :nslots, :cols].contiguous() for i in range(narr)]
    outs = _fold(arrays, nslots, cols, dtype)
    again = _fold(arrays, nslots, cols, dtype)
    for i, (a, o) in enumerate(zip(arrays, outs)):
        assert _within_bound(o, a, dtype, f"kernel[{i}]")
        assert _within_bound(a.sum(0).to(dtype), a, dtype, f"torch[{i}]")
        assert torch.equal(o, again[i])


def test_wrapper_switch(base, monkeypatch):
    """_fold_partials: the kernel with the switch on, torch's reduce and cast
    with it off, over flat workspaces as the backwards hold them."""
    from adapcc_amd.ops import fused

    assert fused._core()
    nslots, cols = 4096, 768
    parts = [base[i, :nslots, :cols].contiguous().view(-1) for i in range(2)]
    on = fused._fold_partials(parts, nslots, cols, torch.bfloat16)
    monkeypatch.setattr(fused, "FUSE_COLSUM_FOLD", False)
    off = fused._fold_partials(parts, nslots, cols, torch.bfloat16)
    for p, a, b in zip(parts, on, off):
        assert a.dtype == b.dtype == torch.bfloat16 and a.shape == (cols,)
        assert _within_bound(a, p.view(nslots, cols), torch.bfloat16, "on")
        assert torch.equal(b, p.view(nslots, cols).sum(0).to(torch.bfloat16))


def test_rejects_bad_shapes():
    import adapcc_amd._core as c

    a = torch.zeros(4, 6, device="cuda")
    o = torch.zeros(6, device="cuda")
    s = torch.cuda.current_stream().cuda_stream
    with pytest.raises(RuntimeError):  # cols not a multiple of 4
        c.colsum_fold(c.DTYPE_F32, a.data_ptr(), 0, 0, o.data_ptr(), 0, 0,
                      4, 6, s)
    with pytest.raises(RuntimeError):  # array without an output
        c.colsum_fold(c.DTYPE_F32, a.data_ptr(), a.data_ptr(), 0,
                      o.data_ptr(), 0, 0, 4, 4, s)
    with pytest.raises(RuntimeError):  # no slots
        c.colsum_fold(c.DTYPE_F32, a.data_ptr(), 0, 0, o.data_ptr(), 0, 0,
                      0, 4, s)
