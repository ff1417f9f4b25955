"""The cached-attention kernels (decode and extend, bf16 and e4m3 caches)
over the joint cases of ``attn_cached_cases``: every pair of option values,
non-default softmax scales, hard input distributions and offsets past 2^31,
against the fp64 ``cached_reference`` at the project's tolerances (rtol =
atol = 2e-2 on the output, 1e-3 on the lse; the CPU file shows that the
documented roundings alone stay under half of the former). Every call
asserts ``fa_*_supported`` first, so a silent fall to the composed route
fails there."""

import pytest
import torch

from attn_cached_cases import F8, U8, build, cached_reference, cases, reference_of
from test_attention_cached_cases_cpu import assert_caches, call, expected_bases
from test_gpu_attention_decode_fp8 import LSE_TOL, O_TOL, assert_appended

import adapcc_amd._core as core
from adapcc_amd.ops.attention import (fa_decode_supported, fa_extend_supported,
                                      flash_attention_decode,
                                      flash_attention_extend, kv_cache_append,
                                      kv_quantize_reference)

pytestmark = pytest.mark.gpu


def within_one_code(got, want):
    """e4m3 bytes that are the same code or neighbours on the e4m3 grid
    (+0 and -0 being one value): what a division that rounds the last bit
    the other way can make of ``kv_quantize_reference``."""
    def rank(c):    # sign-magnitude byte -> position on the number line
        c = c.to(torch.int16)
        return torch.where(c >= 128, 128 - c, c)
    return ((rank(got) - rank(want)).abs() <= 1).all()


def supported(r):
    if r.case.op == "decode":
        return fa_decode_supported(r.q, r.k_cache, r.v_cache, r.lens,
                                   r.block_table, r.k_scale, r.v_scale)
    return fa_extend_supported(r.q, r.k_cache, r.v_cache, r.lens, r.q_lens,
                               r.block_table, r.k_scale, r.v_scale)


def policy_splits(r):
    c = r.case
    (H, Hk), dev = c.heads, r.q.get_device()
    if c.op == "decode":
        return core.fa_decode_splits(c.B, Hk, c.Smax, 0, dev)
    return core.fa_extend_splits(c.B, Hk, c.Sq, H // Hk, c.Smax, 0, dev)


def sweep(case):
    r = build(case, "cuda", torch.bfloat16)
    assert supported(r)
    pow2 = case.cache in ("bf16", "e4m3_pow2")
    want = expected_bases(r)
    k0, v0 = r.k_cache.clone(), r.v_cache.clone()
    ref = reference_of(r) if pow2 or r.k_new is None else None
    lens0 = r.lens.clone()
    ql0 = None if r.q_lens is None else r.q_lens.clone()
    out, lse = call(r)
    assert_caches(r, want, float_equal_rows=pow2)
    if case.fp8 and r.k_new is not None:
        four = lambda x: x if x.dim() == 4 else x.unsqueeze(2)
        n = [case.Sq] * case.B if r.ql is None else r.ql
        for base, w, wrote, c0, new, sc in (
                (r.k_base, want[0], want[2], k0, r.k_new, r.k_scale),
                (r.v_base, want[1], want[3], v0, r.v_new, r.v_scale)):
            # any scale: a written code is the reference's or its neighbour
            assert within_one_code(base.view(U8)[wrote], w.view(U8)[wrote])
            if pow2:    # the existing convention, on the cache as passed
                view = r.k_view if base is r.k_base else r.v_view
                assert_appended(view(base), c0, four(new), sc, r.past, n,
                                r.block_table)
    assert torch.equal(r.lens, lens0)
    assert ql0 is None or torch.equal(r.q_lens, ql0)
    if ref is None:
        # scales that are no powers of two: the kernel's division may round
        # a code the other way, so the output is held to the caches as read
        # back, the chunk's rows among them
        kn, vn, r.k_new, r.v_new = r.k_new, r.v_new, None, None
        past, r.past = r.past, r.total
        ref = reference_of(r)
        r.k_new, r.v_new, r.past = kn, vn, past
    ref_out, ref_lse = ref[0], ref[1]
    fin = torch.isfinite(ref_lse)
    # one line a case for profiles/attn_cached_sweep.txt (pytest -s shows it)
    print("sweep-err", case.op, "e4m3" if case.fp8 else "bf16", case.dist,
          float((out.double() - ref_out).abs().max()),
          float((lse.double() - ref_lse)[fin].abs().max()) if fin.any()
          else 0.0)
    assert torch.isfinite(out).all()
    torch.testing.assert_close(out.double(), ref_out, **O_TOL)
    torch.testing.assert_close(lse.double(), ref_lse, **LSE_TOL)
    dead = ~fin
    assert not out[dead].any() and (lse[dead] == float("-inf")).all()
    # again, over the caches the first call left (the append rewrites the
    # same rows with the same bytes): the same bits
    again = call(r)
    assert torch.equal(out, again[0]) and torch.equal(lse, again[1])
    if case.long:
        ns = policy_splits(r)
        assert ns > 1
        r.kw["num_splits"] = ns
        forced = call(r)
        assert torch.equal(out, forced[0]) and torch.equal(lse, forced[1])


@pytest.mark.parametrize("case", cases("decode"), ids=lambda c: c.id)
def test_decode_case(case):
    sweep(case)


@pytest.mark.parametrize("case", cases("extend"), ids=lambda c: c.id)
def test_extend_case(case):
    sweep(case)


# ---------------------------------------------------------------------------
# scale identities, tolerance-free or nearly so
# ---------------------------------------------------------------------------
SMALL = [(2, 4, 4, 64, 3, [70, 257]), (2, 6, 2, 128, 7, [1, 129]),
         (3, 8, 1, 64, 33, [33, 64, 300]), (2, 5, 5, 128, 1, [127, 320])]


def small(op, fp8, B, H, Hk, D, Sq, lens, seed=0):
    g = torch.Generator().manual_seed(seed)
    q = torch.randn(B, H, Sq, D, generator=g).bfloat16().cuda()
    k, v = torch.randn(2, B, Hk, 320, D, generator=g).cuda()
    kw = {}
    if fp8:
        ks = torch.tensor([2.0 ** -(5 + h % 2) for h in range(Hk)]).cuda()
        vs = torch.tensor([2.0 ** -(6 - h % 2) for h in range(Hk)]).cuda()
        k, v = kv_quantize_reference(k, ks), kv_quantize_reference(v, vs)
        kw = dict(k_scale=ks, v_scale=vs)
    else:
        k, v = k.bfloat16(), v.bfloat16()
    lt = torch.tensor(lens, dtype=torch.int32).cuda()
    if op == "decode":
        q = q[:, :, 0].contiguous()
        assert fa_decode_supported(q, k, v, lt, None, kw.get("k_scale"),
                                   kw.get("v_scale"))
        fn = flash_attention_decode
    else:
        assert fa_extend_supported(q, k, v, lt, None, None,
                                   kw.get("k_scale"), kw.get("v_scale"))
        fn = flash_attention_extend
    return (lambda qq, **o: fn(qq, k, v, lt, return_lse=True,
                               **dict(kw, **o))), q, kw


@pytest.mark.parametrize("shape", SMALL, ids=str)
@pytest.mark.parametrize("fp8", [False, True], ids=["bf16", "e4m3"])
@pytest.mark.parametrize("op", ["decode", "extend"])
def test_scale_identities(op, fp8, shape):
    run, q, kw = small(op, fp8, *shape)
    s = 2.0 ** -3       # exact in bf16, and in every fp32 product with it
    for ns in (1, 3):
        a = run(q, scale=s, num_splits=ns)
        b = run(q * s, scale=1.0, num_splits=ns)
        assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
        if not fp8:
            continue
        c = run(q, scale=s / 2, num_splits=ns, k_scale=kw["k_scale"] * 2)
        assert torch.equal(a[0], c[0]) and torch.equal(a[1], c[1])
        d = run(q, scale=s, num_splits=ns, v_scale=kw["v_scale"] * 2)
        # doubling is exact in fp32, so at most the final rounding differs
        twice = 2 * a[0].float()
        ulp = 2.0 ** (torch.floor(torch.log2(twice.abs().clamp(
            min=2.0 ** -120))) - 7)
        assert ((d[0].float() - twice).abs() <= ulp).all()
        assert torch.equal(a[1], d[1])


# ---------------------------------------------------------------------------
# offsets past 2^31 elements and 2^32 bytes
# ---------------------------------------------------------------------------
GIB = 1 << 30
ALLOC = 17 * GIB // 2       # bytes of the one allocation a test works in
MARGIN = GIB // 4           # q, the compact caches, workspaces, the reference
ORIGIN = 4 * GIB            # byte offset of a far view's first element
ROW = 8192                  # bytes from one key row of a far view to the next


def far_view(buf, fp8, planes, rows, D):
    """The [2,planes,rows,D] view of buf (uint8 [ALLOC]) from ORIGIN whose
    leading stride (a slab's batch stride, a pool's page stride) is 2^31 +
    2048 elements (bf16) or 2^32 + 4096 bytes (e4m3); returns it with the
    bytes one leading index spans. Key rows lie ROW bytes apart, so a
    leading offset cut to 32 bits (4096 bytes either way) lands in the gaps
    between index 0's rows, never in a row."""
    if fp8:
        t, lead = buf.view(F8), (1 << 32) + 4096
    else:
        t, lead = buf.view(torch.bfloat16), (1 << 31) + 2048
    esz = t.element_size()
    span = planes * rows * ROW
    assert ORIGIN + lead * esz + span <= ALLOC
    return t.as_strided((2, planes, rows, D),
                        (lead, rows * ROW // esz, ROW // esz, 1),
                        ORIGIN // esz), span


def poison_far(buf, fp8, span):
    """NaN (bf16) or 0x7F (e4m3) over everything a narrowed leading offset
    can reach, all of it inside buf: both indices' spans, gaps included (the
    rows are written afterwards), and for bf16 the offset sign-extended from
    32 bits (2048 - 2^31 elements: byte 4096 of buf) and the element offset
    taken as bytes (ORIGIN + 2^31 + 2048). The e4m3 offset cut to 32 bits is
    4096 bytes signed or not, and its bytes are its elements."""
    lead = (1 << 32) + 4096         # the leading stride in bytes, both dtypes
    starts = [ORIGIN, ORIGIN + lead]
    if not fp8:
        elems = (1 << 31) + 2048    # the same stride in bf16 elements
        signed = ORIGIN + 2 * (elems - (1 << 32))   # as a negative int32
        as_bytes = ORIGIN + elems
        assert signed == 4096 and as_bytes == ORIGIN + (1 << 31) + 2048
        starts += [signed, as_bytes]
    for at in starts:
        assert 0 <= at and at + span + ROW <= ALLOC
        region = buf[at:at + span + ROW]
        if fp8:
            region.fill_(0x7F)
        else:
            region.view(torch.bfloat16).fill_(float("nan"))


@pytest.mark.parametrize("D", [128, 64])
@pytest.mark.parametrize("form", ["slab", "paged16", "paged64"])
@pytest.mark.parametrize("fp8", [False, True], ids=["bf16", "e4m3"])
@pytest.mark.parametrize("op", ["decode", "extend"])
def test_offsets_past_2_31(op, fp8, form, D):
    """A slab whose sequence 1, or a pool whose page 1, lies past 2^31
    elements and 2^32 bytes from the base pointer: the reference on the
    gathered rows, and the bits of the same call on a compact copy."""
    free, _ = torch.cuda.mem_get_info()
    if free < ALLOC + MARGIN:
        pytest.skip(f"needs {ALLOC + MARGIN} bytes of free device memory, "
                    f"{free} are free")
    B, H, Hk, Sq, lens = 2, 4, 2, 5, [70, 257]
    P = None if form == "slab" else int(form[5:])
    rows = 320 if P is None else P      # key rows under one leading index
    g = torch.Generator().manual_seed(D + fp8 + rows)
    q = torch.randn(B, H, Sq, D, generator=g).bfloat16().cuda()
    kf, vf = torch.randn(2, 2, Hk, rows, D, generator=g).cuda()
    kn, vn = torch.randn(2, B, Hk, Sq, D, generator=g).bfloat16().cuda()
    kw = {}
    if fp8:
        ks = torch.tensor([2.0 ** -5, 2.0 ** -6]).cuda()
        vs = torch.tensor([2.0 ** -6, 2.0 ** -5]).cuda()
        kc, vc = kv_quantize_reference(kf, ks), kv_quantize_reference(vf, vs)
        kw = dict(k_scale=ks, v_scale=vs)
    else:
        kc, vc = kf.bfloat16(), vf.bfloat16()
    lt = torch.tensor(lens, dtype=torch.int32).cuda()
    table = None
    if P is not None:
        # both pages under every row of the table, in an order of its own
        mp = -(-max(lens) // P)
        table = (torch.arange(B * mp).view(B, mp) * 5 // 3 % 2).int()
        table[:, 0] = torch.tensor([1, 0])
        assert all(set(row.tolist()) == {0, 1} for row in table)
        table = table.cuda()
        kw.update(block_table=table)
    if op == "decode":
        q = q[:, :, 0].contiguous()
        fn, sup = flash_attention_decode, fa_decode_supported
        args = (table,)
    else:
        fn, sup = flash_attention_extend, fa_extend_supported
        args = (None, table)
    buf = torch.empty(ALLOC, dtype=U8, device="cuda")
    try:
        # K the even planes and V the odd ones of one view of twice the
        # heads: both carry the large leading stride
        both, span = far_view(buf, fp8, 2 * Hk, rows, D)
        poison_far(buf, fp8, span)
        kb, vb = both[:, 0::2], both[:, 1::2]
        kb.copy_(kc), vb.copy_(vc)
        assert sup(q, kb, vb, lt, *args, kw.get("k_scale"), kw.get("v_scale"))
        if fp8:
            # rows enter through the append kernel, in both forms: a slab's
            # last Sq rows; a pool's through a table of one page a sequence,
            # so that no page two rows name is appended into
            akw = dict(k_scale=ks, v_scale=vs)
            if P is None:
                past = [n - Sq for n in lens]
            else:
                past = [P - Sq - 2, 3]
                akw.update(block_table=table[:, :1].contiguous())
            past = torch.tensor(past, dtype=torch.int32).cuda()
            kv_cache_append(kb, vb, past, kn, vn, **akw)
            kv_cache_append(kc, vc, past, kn, vn, **akw)
            assert torch.equal(kb.view(U8), kc.view(U8))
            assert torch.equal(vb.view(U8), vc.view(U8))

        def gathered(c, s):
            x = c.view(U8) if fp8 else c
            if P is not None:
                x = x[table.long()].transpose(1, 2).reshape(B, Hk, -1, D)
            x = x.view(F8).float().double() if fp8 else x.double()
            return x if s is None else x * s.double().view(1, -1, 1, 1)

        ref = cached_reference(q, gathered(kc, kw.get("k_scale")),
                               gathered(vc, kw.get("v_scale")), lens)
        for ns in (1, 3):
            got = fn(q, kb, vb, lt, return_lse=True, num_splits=ns, **kw)
            assert torch.isfinite(got[0]).all()
            torch.testing.assert_close(got[0].double(), ref[0], **O_TOL)
            torch.testing.assert_close(got[1].double(), ref[1], **LSE_TOL)
            compact = fn(q, kc, vc, lt, return_lse=True, num_splits=ns, **kw)
            assert torch.equal(got[0], compact[0])
            assert torch.equal(got[1], compact[1])
    finally:
        buf = both = kb = vb = None
        torch.cuda.empty_cache()
