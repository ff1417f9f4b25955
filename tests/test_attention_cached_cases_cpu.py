"""What makes the cases of ``attn_cached_cases`` trustworthy before they
reach a GPU: the pair coverage of ``cases()``, ``cached_reference`` against
the existing fp32 references, every case through the public functions'
composed route, the floor that the kernels' documented roundings leave under
the GPU tolerance, and the wrong references that the cases must tell apart."""

import functools
from unittest import mock

import pytest
import torch

from attn_cached_cases import (EXCEPTIONS, F8, MAX_CASES, U8, axes_of, build,
                               cases, differs, mutants, reference_of,
                               uncovered_pairs)
from attn_decode_ref import decode_reference
from attn_extend_ref import extend_reference
from test_attention_extend_cpu import TOL
from test_gpu_attention_decode_fp8 import LSE_TOL, O_TOL

from adapcc_amd.ops import attention
from adapcc_amd.ops.attention import (_check_cached,
                                      flash_attention_decode,
                                      flash_attention_extend,
                                      kv_quantize_reference)

OPS = ["decode", "extend"]
ALL = [c for op in OPS for c in cases(op)]
IDS = [f"{c.op}-{c.id}" for c in ALL]

# The composed route is fp32 SDPA and an fp32 logsumexp: a score of up to
# 130 from 128 products carries about sqrt(128) * 2^-24 * 130 * (a few)
# = 4e-4 of rounding at the worst case (one_split under a wide k_scale),
# which lands in the lse one to one and in the output through the weights.
COMPOSED_TOL = dict(rtol=1e-4, atol=5e-4)


@functools.lru_cache(maxsize=None)
def built(case):
    """A case in bf16 on the CPU, for the tests that only read it."""
    return build(case, "cpu", torch.bfloat16)


@functools.lru_cache(maxsize=None)
def truth(case):
    return reference_of(built(case))


@pytest.mark.parametrize("op", OPS)
def test_pair_coverage_and_caps(op):
    cs = cases(op)
    assert len(cs) <= MAX_CASES
    assert len({c.id for c in cs}) == len(cs)
    assert cs == cases(op)                          # deterministic
    assert not uncovered_pairs(op, cs)
    assert all(getattr(c, a) in vals for c in cs if not c.special
               for a, vals in axes_of(op).items())
    kinds = [c.special for c in cs]
    assert kinds.count("shared") == 1 and kinds.count("unaligned") == 1
    assert kinds.count("long") == 2 and kinds.count("long70") == 2
    assert {c.fp8 for c in cs if c.long} == {False, True}


def test_exceptions_are_rejected_or_composed():
    """Each listed pair, put into an otherwise plain case, must fail the
    argument check or the ``*_supported`` query for a reason that does not
    depend on the device."""
    from attn_cached_cases import Case
    for a, va, b, vb in EXCEPTIONS:
        for op in OPS:
            if a not in axes_of(op) or b not in axes_of(op):
                continue
            r = build(Case(op=op, **{a: va, b: vb}), "cpu", torch.bfloat16)
            name = "flash_attention_" + op
            try:
                _check_cached(name, r.q, r.k_cache, r.v_cache, r.lens,
                              r.k_new, r.v_new, r.q_lens, r.block_table,
                              r.k_scale, r.v_scale, fp8_ok=True)
            except ValueError:
                continue        # rejected
            # composed: every condition of the kernel route but the device
            # and the built extension, which a CPU tensor cannot meet
            with mock.patch.object(torch.Tensor, "is_cuda", True), \
                    mock.patch.object(attention, "_core", lambda: True):
                if not attention._cached_kernel_ok(
                        r.q, r.k_cache, r.v_cache, r.lens, r.q_lens,
                        r.block_table):
                    continue
            pytest.fail(f"{(a, va, b, vb)} is accepted")


@pytest.mark.parametrize("case", [c for c in ALL if c.dist == "randn"],
                         ids=lambda c: f"{c.op}-{c.id}")
def test_reference_agrees_with_the_fp32_references(case):
    r = built(case)
    out, lse, k_after, v_after = truth(case)
    deq = lambda c, s: (c.float() if s is None
                        else c.float() * s.view(1, -1, 1, 1))
    k = deq(r.logical(r.k_cache), r.k_scale)
    v = deq(r.logical(r.v_cache), r.v_scale)
    kn, vn = r.k_new, r.v_new
    if kn is not None and case.fp8:
        four = lambda x: x if x.dim() == 4 else x.unsqueeze(2)
        kn = deq(kv_quantize_reference(four(kn), r.k_scale), r.k_scale)
        vn = deq(kv_quantize_reference(four(vn), r.v_scale), r.v_scale)
    if case.op == "decode":
        if kn is not None:      # decode_reference does not append
            kn, vn = (x if x.dim() == 3 else x[:, :, 0] for x in (kn, vn))
            for b, p in enumerate(r.past):
                if p < case.Smax:       # a full cache is left alone
                    k[b, :, p], v[b, :, p] = kn[b].float(), vn[b].float()
        ref, ref_lse = decode_reference(r.q, k, v, r.total,
                                        scale=case.softmax_scale)
    else:
        ref, ref_lse, ka, va = extend_reference(
            r.q, k, v, r.past, kn, vn, q_lens=r.ql, causal=case.causal,
            scale=case.softmax_scale)
        for b, n in enumerate(r.total):
            torch.testing.assert_close(k_after[b, :, :n].float(),
                                       ka[b, :, :n], rtol=0, atol=0)
            torch.testing.assert_close(v_after[b, :, :n].float(),
                                       va[b, :, :n], rtol=0, atol=0)
    torch.testing.assert_close(out.float(), ref, **TOL)
    torch.testing.assert_close(lse.float(), ref_lse, **TOL)


def expected_bases(r):
    """(k_base, v_base, wrote_k, wrote_v) after r's call: the bases before it
    with rows i < n_b of the new rows (``kv_quantize_reference`` of them for
    e4m3) at logical rows past_b + i < Smax, and the masks of those rows."""
    c = r.case
    out = []
    for base, view, new, s in ((r.k_base, r.k_view, r.k_new, r.k_scale),
                               (r.v_base, r.v_view, r.v_new, r.v_scale)):
        want = base.clone()
        wrote = torch.zeros(want.shape, dtype=torch.bool, device=want.device)
        if new is not None:
            new = new if new.dim() == 4 else new.unsqueeze(2)
            rows = kv_quantize_reference(new, s) if c.fp8 else new
            n = [c.Sq] * c.B if r.ql is None else r.ql
            bi = [(b, i) for b in range(c.B)
                  for i in range(min(n[b], c.Smax - r.past[b]))]
            b = torch.tensor([x[0] for x in bi], dtype=torch.long,
                             device=want.device)
            i = torch.tensor([x[1] for x in bi], dtype=torch.long,
                             device=want.device)
            row = torch.tensor(r.past, device=want.device)[b] + i
            if c.paged:
                P = c.P
                first, row = r.block_table[b, row // P].long(), row % P
            else:
                first = b
            wv, mv = view(want), view(wrote)
            if c.fp8:
                wv, rows = wv.view(U8), rows.view(U8)
            wv[first, :, row] = rows[b, :, i]
            mv[first, :, row] = True
        out.append((want, wrote))
    return out[0][0], out[1][0], out[0][1], out[1][1]


def assert_caches(r, want, float_equal_rows=True):
    """The bases against ``expected_bases``: bytes outside the written rows
    unchanged, written rows equal as floats (+-0 are one value)."""
    bits = lambda t: t.view(U8) if t.dtype == F8 else (
        t.view(torch.int16) if t.dtype == torch.bfloat16 else t.view(torch.int32))
    for base, w, wrote in ((r.k_base, want[0], want[2]),
                           (r.v_base, want[1], want[3])):
        assert torch.equal(bits(base)[~wrote], bits(w)[~wrote])
        if base.dtype != F8:        # rows that are copied: the same bits
            assert torch.equal(bits(base), bits(w))
        elif float_equal_rows:
            assert torch.equal(base.float()[wrote], w.float()[wrote])


def call(r):
    fn = flash_attention_decode if r.case.op == "decode" else flash_attention_extend
    return fn(r.q, r.k_cache, r.v_cache, r.lens, return_lse=True, **r.kw)


@pytest.mark.parametrize("case", ALL, ids=IDS)
def test_composed_route_matches_reference(case):
    """fp32 q on the CPU takes the composed route: the builders and the
    reference against the API's documented behaviour, no kernel involved."""
    r = build(case, "cpu", torch.float32)
    ref_out, ref_lse, _, _ = reference_of(r)
    want = expected_bases(r)
    lens0 = r.lens.clone()
    ql0 = None if r.q_lens is None else r.q_lens.clone()
    out, lse = call(r)
    assert torch.isfinite(out).all()
    torch.testing.assert_close(out.double(), ref_out, **COMPOSED_TOL)
    torch.testing.assert_close(lse.double(), ref_lse, **COMPOSED_TOL)
    dead = ref_lse == float("-inf")
    assert not out[dead].any() and (lse[dead] == float("-inf")).all()
    assert_caches(r, want)
    assert torch.equal(r.lens, lens0)
    assert ql0 is None or torch.equal(r.q_lens, ql0)


@pytest.mark.parametrize("case", ALL, ids=IDS)
def test_rounding_floor_is_under_half_the_tolerance(case):
    """bf16 inputs, P rounded to bf16 ahead of PV, the output rounded to
    bf16, all else in fp64: that error is a property of the inputs, and must
    leave half of O_TOL to the kernels."""
    ref_out = truth(case)[0]
    emu = reference_of(built(case), emulate=True)[0]
    room = 0.5 * (O_TOL["atol"] + O_TOL["rtol"] * ref_out.abs())
    err = (emu - ref_out).abs()
    assert (err <= room).all(), float((err / room).max())
    # |V| <= 4 before e4m3 rounding, which moves a value by at most 2^-4 of it
    assert ref_out.abs().max() <= 4.0 * (1 + 2.0 ** -4)


@pytest.mark.parametrize("name", list(mutants()))
def test_mutant_is_caught(name):
    applies, every, run = mutants()[name]
    hit = [c for c in ALL if applies(c)]
    assert hit, "no case exercises this mistake"
    caught = []
    for c in hit:
        ref_out, ref_lse = truth(c)[:2]
        out, lse = run(built(c))
        caught.append(differs(out, ref_out, **O_TOL)
                      or differs(lse, ref_lse, **LSE_TOL))
    if every:
        missed = [c.id for c, x in zip(hit, caught) if not x]
        assert not missed, missed
    assert any(caught)
