"""Cases, builders, the fp64 reference and wrong references ("mutants") for
the attention calls over a KV cache (not a test module): what
``test_attention_cached_cases_cpu.py`` makes trustworthy on the CPU and
``test_gpu_attention_cached_sweep.py`` runs against the kernels.

Axes of ``cases(op, seed)``. Every pair of values of two different axes
stands in at least one case (``uncovered_pairs`` checks it):

  cache     bf16, or e4m3 under one of four kinds of scales: ``amax`` (per
            head distinct, not powers of two, near amax / 448), ``pow2``
            (2^-7 .. 2^4 over the heads of k and v), ``big`` (scale * k_scale
            * log2(e) = 16 and more) and ``tiny`` (5e-4). The e4m3 scale kinds
            are values of this axis, so no pair of them with bf16 exists.
  layout    slab, transposed ([B,Smax,Hk,D] memory), offset (a slice of a
            larger slab, storage offset > 0), paged16 / paged32 / paged128
            (pools under a shuffled table, unused entries out of range),
            pool_t64 (a [N,P,Hk,D] pool as its transposed view)
  D, heads, num_splits, scale, dist, poison, append
  extend only: Sq, causal, ragged (q_lens from Sq down to 0), q_t (q as the
            transposed view of [B,Sq,H,D])

``EXCEPTIONS`` lists the pairs left out because the API rejects them or sends
them to the composed route. There are none: every axis value is built so
that the kernels take it with every value of every other axis (the ``extremes``
distribution, e4m3 codes, is also put into bf16 caches, which hold them
exactly).

Beside the pair fill stand the special cases, each a fixed configuration:
``shared`` (two sequences name one first page, nothing appended: appending
into a shared page is outside the contract), ``unaligned`` (new rows that are
not 16-B aligned) and four long-cache cases per op (Smax 4096, B 1,
num_splits None, two per cache dtype, one of each with only 70 keys).

How a case's numbers are made. A distribution is written in "logical" units:
scores z = q·k / sqrt(D) of the sizes its name promises. The softmax scale s
of the case and, for e4m3, the factor by which k_scale exceeds amax / 448 are
divided out of q, so the scaled scores of the dequantised keys stay z whatever
the scales are, while c1 = s * k_scale * log2(e) takes the axis's value. V is
0.5 * randn + a per-head, per-column bias of +-(1 + 0.3 hk), clamped to +-4:
outputs are O(1) and the absolute tolerance means something."""

import itertools
import math
import re
from dataclasses import dataclass
from types import SimpleNamespace
from typing import Optional

import torch

from adapcc_amd.ops.attention import kv_quantize_reference

F8, U8 = torch.float8_e4m3fn, torch.uint8
LOG2E = 1.4426950408889634

CACHES = ["bf16", "e4m3_amax", "e4m3_pow2", "e4m3_big", "e4m3_tiny"]
LAYOUTS = ["slab", "transposed", "offset", "paged16", "paged32", "paged128",
           "pool_t64"]
DISTS = ["randn", "spiked", "rising", "constant", "one_split", "extremes"]
COMMON_AXES = {
    "cache": CACHES,
    "layout": LAYOUTS,
    "D": [64, 128],
    "heads": [(4, 4), (6, 2), (5, 5), (8, 1), (32, 1)],
    "append": ["none", "rows", "strided"],
    "num_splits": [None, 1, 2, 5, 32],
    "scale": ["none", "one", "small", "wide"],
    "dist": DISTS,
    "poison": [False, True],
}
EXTEND_AXES = {
    "Sq": [1, 7, 32, 33, 64, 100],
    "causal": [True, False],
    "ragged": [False, True],
    "q_t": [False, True],
}
MAX_CASES = 64

# (axis, value, axis, value) pairs that cases() leaves out: combinations the
# API rejects or sends to the composed route. None.
EXCEPTIONS = []


def axes_of(op):
    return dict(COMMON_AXES, **(EXTEND_AXES if op == "extend" else {}))


@dataclass(frozen=True)
class Case:
    op: str
    cache: str = "bf16"
    layout: str = "slab"
    D: int = 64
    heads: tuple = (4, 4)
    append: str = "none"        # none, rows, strided, unaligned
    num_splits: Optional[int] = None
    scale: str = "none"
    dist: str = "randn"
    poison: bool = False
    Sq: int = 1
    causal: bool = True
    ragged: bool = False
    q_t: bool = False
    special: str = ""           # "", shared, unaligned, long, long70
    seed: int = 0

    @property
    def fp8(self):
        return self.cache != "bf16"

    @property
    def paged(self):
        return self.layout.startswith(("paged", "pool_t", "shared"))

    @property
    def P(self):
        return int(re.search(r"\d+$", self.layout).group()) if self.paged else None

    @property
    def long(self):
        return self.special.startswith("long")

    @property
    def Smax(self):
        if self.long:
            return 4096
        sizes = [256, 384, 512, 640] if self.P == 128 else [
            256, 320, 384, 512, 640]
        return sizes[self.seed % len(sizes)]

    @property
    def B(self):
        return 1 if self.long else 5

    @property
    def softmax_scale(self):
        return {"none": None, "one": 1.0, "small": 0.02,
                "wide": 2.5 * self.D ** -0.5}[self.scale]

    @property
    def id(self):
        H, Hk = self.heads
        parts = [self.special or "pair", self.cache, self.layout,
                 f"D{self.D}", f"H{H}k{Hk}", f"Smax{self.Smax}"]
        if self.op == "extend":
            parts += [f"Sq{self.Sq}", "causal" if self.causal else "full",
                      "ragged" if self.ragged else "even",
                      "qT" if self.q_t else "q"]
        parts += [f"app-{self.append}", f"ns{self.num_splits}",
                  f"scale-{self.scale}", self.dist,
                  "poison" if self.poison else "junk", f"s{self.seed}"]
        return "-".join(parts)


def allowed(a, va, b, vb):
    return ((a, va, b, vb) not in EXCEPTIONS
            and (b, vb, a, va) not in EXCEPTIONS)


def all_pairs(op):
    ax = axes_of(op)
    return {(a, va, b, vb)
            for a, b in itertools.combinations(ax, 2)
            for va in ax[a] for vb in ax[b] if allowed(a, va, b, vb)}


def pairs_of(case):
    ax = axes_of(case.op)
    return {(a, getattr(case, a), b, getattr(case, b))
            for a, b in itertools.combinations(ax, 2)}


def uncovered_pairs(op, cs):
    """The allowed pairs that no pair-fill or special case of cs holds."""
    left = all_pairs(op)
    for c in cs:
        left -= pairs_of(c)
    return left


def _candidate(ax, left, rng):
    order = list(ax)
    rng.shuffle(order)
    pick = {}
    for a in order:
        best, best_n = None, -1
        vals = list(ax[a])
        rng.shuffle(vals)
        for v in vals:
            if not all(allowed(a, v, b, vb) for b, vb in pick.items()):
                continue
            n = sum(((a, v, b, vb) in left) or ((b, vb, a, v) in left)
                    for b, vb in pick.items())
            if n > best_n:
                best, best_n = v, n
        pick[a] = best
    return pick


def _greedy(op, rng):
    ax = axes_of(op)
    left = all_pairs(op)
    out = []
    while left:
        # the best of a few candidate cases, each filled axis by axis with
        # the value that covers most of what is left
        cands = [_candidate(ax, left, rng) for _ in range(12)]
        pick = max(cands, key=lambda p: len(
            pairs_of(Case(op=op, **p)) & left))
        c = Case(op=op, seed=len(out), **pick)
        out.append(c)
        left -= pairs_of(c)
    return out


def _specials(op, seed):
    ext = op == "extend"
    sq = dict(Sq=5) if ext else {}
    out = [
        Case(op=op, cache="e4m3_amax", layout="shared32", D=128,
             heads=(6, 2), num_splits=2, dist="randn", poison=True,
             special="shared", seed=seed + 1, **sq),
        Case(op=op, cache="bf16", layout="slab", D=64, heads=(6, 2),
             append="unaligned", num_splits=2, dist="randn",
             special="unaligned", seed=seed + 2, **sq),
    ]
    for i, cache in enumerate(["bf16", "e4m3_amax"]):
        out.append(Case(
            op=op, cache=cache, layout=["slab", "paged32"][i], D=128,
            heads=[(8, 1), (6, 2)][i], dist="one_split", scale="one",
            append="rows" if i else "none", special="long", seed=seed + 3 + i,
            **(dict(Sq=8, causal=bool(i)) if ext else {})))
        out.append(Case(
            op=op, cache=cache, layout=["transposed", "slab"][i], D=64,
            heads=[(4, 4), (8, 1)][i], dist="spiked", poison=True,
            special="long70", seed=seed + 5 + i,
            **(dict(Sq=5, ragged=bool(i)) if ext else {})))
    return out


_CASES = {}


def cases(op, seed=0):
    """At most MAX_CASES configurations of op ("decode" or "extend"): a
    greedy pair fill (the shortest of four seeded tries) and the specials."""
    if (op, seed) not in _CASES:
        import random
        tries = [_greedy(op, random.Random(1000 * seed + t)) for t in range(4)]
        fill = min(tries, key=len)
        _CASES[op, seed] = fill + _specials(op, seed)
    return list(_CASES[op, seed])


# ---------------------------------------------------------------------------
# Builders
# ---------------------------------------------------------------------------
def _lengths(c, g):
    """(past, q_lens or None, total): python lists. total_b keys count after
    the call's own append."""
    B, Sq, Smax, P = c.B, c.Sq, c.Smax, c.P or 64
    if c.special == "long":
        past = [Smax - 37 - (Sq if c.append != "none" else 0)]
    elif c.special == "long70":
        past = [70]
    else:
        edge = sorted({x + d for x in (32, 64, 128, 256, P, 2 * P, Smax)
                       for d in (-1, 0, 1) if 1 < x + d <= Smax - Sq})
        mid = [edge[int(torch.randint(len(edge), (1,), generator=g))]
               for _ in range(2)]
        if c.special == "shared":
            past = [P + 1, 2 * P + 3, 0, 1, Smax]
        elif c.append == "none":
            past = [0, 1, mid[0], mid[1], Smax]
        else:
            # sequence 3 reaches Smax (rows are dropped when Sq > 1), 4 is full
            past = [0, mid[0], 1, Smax - Sq + min(2, Sq - 1), Smax]
    ql = None
    if c.ragged:
        ql = ([3] if B == 1 else
              [max(Sq - b * -(-Sq // (B - 1)), 0) for b in range(B)])
        ql = ql[1:] + ql[:1]    # the full-length block is not sequence 0
    n = [Sq] * B if ql is None else ql
    total = [min(p + x, Smax) if c.append != "none" else p
             for p, x in zip(past, n)]
    return past, ql, total


def _logical(c, total, g):
    """q [B,H,Sq,D], k, v [B,Hk,Smax,D] in logical units, fp32 on the CPU."""
    B, (H, Hk), Sq, D, Smax = c.B, c.heads, c.Sq, c.D, c.Smax
    G = H // Hk
    rn = lambda *s: torch.randn(*s, generator=g)
    u = torch.randint(0, 2, (B, Hk, 1, D), generator=g).float() * 2 - 1
    j = torch.arange(Smax).view(1, 1, Smax, 1)
    tot = torch.tensor(total).view(B, 1, 1, 1)
    if c.dist in ("randn", "extremes"):
        q = rn(B, H, Sq, D)
    else:
        q = 0.5 * rn(B, H, Sq, D) + u.repeat_interleave(G, 1)
    along = u / math.sqrt(D)        # q·along / sqrt(D) is about 1
    k = rn(B, Hk, Smax, D)
    if c.dist == "spiked":
        k = k + 40.0 * along * ((j == 0) | (j == 128) | (j == tot - 1))
    elif c.dist == "rising":
        k = 0.1 * k + along * (60.0 * (j + 1) / Smax)
    elif c.dist == "constant":
        k = (0.3 * k[:, :, :1] + 5.0 * along).expand(B, Hk, Smax, D).clone()
    elif c.dist == "one_split":
        heavy = ((tot - 1).clamp(min=0) // 128) // 2
        k = 0.5 * k + 120.0 * along * ((j // 128) == heavy)
    elif c.dist == "extremes":
        # e4m3 values: +-448, subnormals, +-0, ordinary codes; zero key rows
        codes = torch.randint(0, 256, (B, Hk, Smax, D), generator=g,
                              dtype=torch.int16).to(U8)
        kind = torch.randint(0, 8, (B, Hk, Smax, D), generator=g)
        codes = torch.where(kind == 0, codes & 0x87, codes)      # subnormal
        codes = torch.where(kind == 1, (codes & 0x80) | 0x7E, codes)  # 448
        codes = torch.where(kind == 2, codes & 0x80, codes)      # +-0
        codes = torch.where((codes & 0x7F) == 0x7F, codes & 0x80, codes)
        codes = torch.where(j % 7 == 3, torch.zeros_like(codes), codes)
        k = codes.view(F8).float() * 2.0 ** -6      # |k| <= 7
    sign = 1.0 - 2.0 * ((torch.arange(D).view(1, 1, 1, D)
                         + torch.arange(Hk).view(1, Hk, 1, 1)) % 2)
    bias = sign * (1.0 + 0.3 * torch.arange(Hk).view(1, Hk, 1, 1))
    v = (0.5 * rn(B, Hk, Smax, D) + bias).clamp(-4.0, 4.0)
    if c.dist == "extremes":
        vc = torch.randint(0, 256, (B, Hk, Smax, D), generator=g,
                           dtype=torch.int16).to(U8)
        vk = torch.randint(0, 8, (B, Hk, Smax, D), generator=g)
        vc = torch.where(vk == 0, vc & 0x87, vc)                 # subnormal
        vc = torch.where(vk == 1, (vc & 0x80) | 0x7E, vc)        # +-448
        vc = torch.where((vc & 0x7F) == 0x7F, vc & 0x80, vc)
        # exact codes under _extreme_v_scale, a power of two: |v| <= 3.5
        vx = _extreme_v_scale(Hk).view(1, Hk, 1, 1)
        v = torch.where(j % 3 == 0, vc.view(F8).float() * vx,
                        torch.maximum(torch.minimum(v, 448 * vx), -448 * vx))
    if c.special == "shared":
        P = c.P
        k[1, :, :P], v[1, :, :P] = k[0, :, :P], v[0, :, :P]
    return q, k, v


def _extreme_v_scale(Hk):
    """v_scale of every ``extremes`` case, whatever its kind of scales: V
    holds exact e4m3 codes, +-448 and subnormals among them, under 2^-7 for
    even heads and 2^-8 for odd ones (bf16 caches hold the same values)."""
    return 2.0 ** -(7.0 + torch.arange(Hk) % 2)


def _scales(c, k, total):
    """(k_scale, v_scale, code_scale) fp32 [Hk] for an e4m3 case: the codes
    are q8(k, code_scale), what the cache stands for is codes * k_scale."""
    Hk, Smax = c.heads[1], c.Smax
    h = torch.arange(Hk, dtype=torch.float32)
    live = (torch.arange(Smax).view(1, 1, Smax, 1)
            < torch.tensor(total).view(-1, 1, 1, 1))
    amax = (k.abs() * live).amax(dim=(0, 2, 3)).clamp(min=1.0)
    cs = amax / 448.0
    s = c.softmax_scale or c.D ** -0.5
    kind = c.cache[5:]
    vs = (4.0 / 448.0) * (1.5 + 0.25 * h)
    if kind == "amax":
        ks = cs.clone()
    elif kind == "pow2":
        ks = 2.0 ** torch.tensor([4.0, 1.0, -2.0, -5.0, 3.0])[:Hk]
        vs = 2.0 ** torch.tensor([-6.0, -3.0, 0.0, -7.0, -5.0])[:Hk]
    elif kind == "big":
        ks = 16.0 / (s * LOG2E) * (1.0 + 0.1 * h)
    else:
        ks = 5e-4 / (s * LOG2E) * (1.0 + 0.1 * h)
    if c.dist == "extremes":
        vs = _extreme_v_scale(Hk)
    return ks.float(), vs.float(), cs.float()


def _pack(c, slab, fill, table, dev):
    """The cache tensor of the case's layout that holds slab [B,Hk,Smax,D]
    (uint8 codes or a float dtype).
    Whole unused pages and the slab around an offset view hold the scalar
    tensor ``fill``. Returns (base, view): cache = view(base)."""
    B, Hk, Smax, D = slab.shape
    page_junk = fill
    if c.layout == "slab":
        return slab.contiguous(), lambda t: t
    if c.layout == "transposed":
        return (slab.transpose(1, 2).contiguous(),
                lambda t: t.transpose(1, 2))
    if c.layout == "offset":
        base = page_junk.expand(B + 1, Hk, Smax + 8, D).clone()
        view = lambda t: t[1:, :, 3:3 + Smax]
        view(base).copy_(slab)
        return base, view
    P = c.P
    mp = Smax // P
    N = B * mp + 3
    pages = slab.view(B, Hk, mp, P, D).transpose(1, 2)      # [B,mp,Hk,P,D]
    if c.layout.startswith("pool_t"):
        base = page_junk.expand(N, P, Hk, D).clone()
        view = lambda t: t.transpose(1, 2)
    else:
        base = page_junk.expand(N, Hk, P, D).clone()
        view = lambda t: t
    view(base)[table.long()] = pages
    return base, view


def build(case, device="cpu", q_dtype=torch.bfloat16):
    """The tensors of a case on ``device``. bf16 caches take q_dtype (the
    API wants one dtype), holding bf16-representable values either way.
    Returns a namespace: the call's arguments (q, k_cache, v_cache, lens,
    q_lens, k_new, v_new, block_table, k_scale, v_scale, kw), the python
    lists past, ql, total, the bases and views of the caches, and
    ``logical(cache)``: the [B,Hk,Smax,D] slab a cache tensor holds."""
    c = case
    g = torch.Generator().manual_seed(7919 * c.seed + (c.op == "extend"))
    B, (H, Hk), Sq, D, Smax = c.B, c.heads, c.Sq, c.D, c.Smax
    G = H // Hk
    past, ql, total = _lengths(c, g)
    q, k, v = _logical(c, total, g)
    s = c.softmax_scale or D ** -0.5
    q = q * (D ** -0.5 / s)
    j = torch.arange(Smax).view(1, 1, Smax, 1)
    held = torch.tensor(past).view(B, 1, 1, 1)     # rows the cache holds now
    ks = vs = None
    if c.fp8:
        ks, vs, cs = _scales(c, k, total)
        f = (ks / cs).view(1, Hk, 1, 1)
        q = q / f.repeat_interleave(G, 1)
        kc = kv_quantize_reference(k, cs).view(U8)
        vc = kv_quantize_reference(v, vs).view(U8)
        k_rows, v_rows = (k * f).to(q_dtype), v.to(q_dtype)
        fills = []
        for _ in range(2):
            fl = torch.randint(0, 0x7F, (B, Hk, Smax, D), generator=g,
                               dtype=torch.int16).to(U8)
            if c.poison:
                fl.fill_(0x7F)
            fills.append(fl)
        page_junk = torch.tensor(0x7F if c.poison else 0x35, dtype=U8)
        slabs = [torch.where(j < held, x, fl)
                 for x, fl in zip((kc, vc), fills)]
    else:
        k, v = k.bfloat16(), v.bfloat16()
        k_rows, v_rows = k.to(q_dtype), v.to(q_dtype)
        bad = float("nan") if c.poison else 3.0
        fills = [(torch.randn(B, Hk, Smax, D, generator=g) * 3).bfloat16()
                 .to(q_dtype) for _ in range(2)]
        if c.poison:
            for fl in fills:
                fl.fill_(bad)
        page_junk = torch.tensor(bad, dtype=q_dtype)
        slabs = [torch.where(j < held, x.to(q_dtype), fl)
                 for x, fl in zip((k, v), fills)]
    q = q.bfloat16().to(q_dtype)

    table = None
    if c.paged:
        P = c.P
        mp = Smax // P
        N = B * mp + 3
        table = torch.randperm(N, generator=g)[:B * mp].view(B, mp).int()
        if c.special == "shared":
            table[1, 0] = table[0, 0]
    packed = [_pack(c, sl, page_junk, table, device) for sl in slabs]
    if c.paged:
        for b, n in enumerate(total):
            table[b, -(-n // c.P):] = N + 7      # unused: out of range
        table = table.to(device)

    r = SimpleNamespace(case=c, past=past, ql=ql, total=total)
    r.k_base, r.v_base = (p[0].to(device) for p in packed)
    r.k_view, r.v_view = packed[0][1], packed[1][1]
    if c.fp8:
        r.k_base, r.v_base = r.k_base.view(F8), r.v_base.view(F8)
        ks, vs = ks.to(device), vs.to(device)
    r.k_cache, r.v_cache = r.k_view(r.k_base), r.v_view(r.v_base)
    r.k_scale, r.v_scale, r.block_table = ks, vs, table
    r.lens = torch.tensor(past, dtype=torch.int32, device=device)
    r.q_lens = (None if ql is None
                else torch.tensor(ql, dtype=torch.int32, device=device))

    n = torch.tensor([Sq] * B if ql is None else ql).view(B, 1, 1, 1)
    i = torch.arange(Sq).view(1, 1, Sq, 1)
    if c.poison and ql is not None:
        q = torch.where(i < n, q, torch.tensor(float("nan"), dtype=q_dtype))
    if c.q_t:
        q = q.transpose(1, 2).contiguous().transpose(1, 2)
    r.q = q.to(device)
    r.k_new = r.v_new = None
    if c.append != "none":
        at = (held.view(B, 1, 1) + i.view(1, 1, Sq)).clamp(max=Smax - 1)
        at = at.view(B, 1, Sq, 1).expand(B, Hk, Sq, D)
        new = []
        for rows in (k_rows, v_rows):
            x = rows.gather(2, at)
            if c.poison and ql is not None:     # rows past q_lens: not read
                x = torch.where(i < n, x,
                                torch.tensor(float("nan"), dtype=q_dtype))
            if c.append == "strided":           # [B,Sq,Hk,2D] memory
                wide = torch.zeros(B, Sq, Hk, 2 * D, dtype=q_dtype)
                wide[..., D:] = x.transpose(1, 2)
                x = wide.to(device)[..., D:].transpose(1, 2)
            elif c.append == "unaligned":       # one element off 16 B
                flat = torch.zeros(x.numel() + 1, dtype=q_dtype)
                flat[1:] = x.reshape(-1)
                x = flat.to(device)[1:].view(B, Hk, Sq, D)
            else:
                x = x.contiguous().to(device)
            new.append(x)
        r.k_new, r.v_new = new
    if c.op == "decode":
        r.q = r.q[:, :, 0]
        if r.k_new is not None:
            r.k_new, r.v_new = r.k_new[:, :, 0], r.v_new[:, :, 0]

    def logical(cache):
        if table is None:
            return cache
        x = cache.view(U8) if cache.dtype == F8 else cache
        x = x[table.clamp(0, x.shape[0] - 1).long()]     # [B,mp,Hk,P,D]
        x = x.transpose(1, 2).reshape(B, Hk, Smax, D)
        return x.view(F8) if cache.dtype == F8 else x

    r.logical = logical
    r.kw = dict(scale=c.softmax_scale, num_splits=c.num_splits)
    if c.op == "extend":
        r.kw.update(causal=c.causal, q_lens=r.q_lens)
    if table is not None:
        r.kw.update(block_table=table)
    if c.fp8:
        r.kw.update(k_scale=ks, v_scale=vs)
    if r.k_new is not None:
        r.kw.update(k_new=r.k_new, v_new=r.v_new)
    return r


# ---------------------------------------------------------------------------
# The fp64 reference
# ---------------------------------------------------------------------------
def _reference(q, k, v, past, q_lens, causal, scale, k_new, v_new,
               mut=frozenset(), emulate=False):
    decode = q.dim() == 3
    if decode:
        q = q.unsqueeze(2)
        k_new, v_new = (None if t is None else t.unsqueeze(2)
                        for t in (k_new, v_new))
    dev = q.device
    B, H, Sq, D = q.shape
    Hk, Smax = k.shape[1], k.shape[2]
    G = H // Hk
    f64 = torch.float64
    scale = D ** -0.5 if scale is None else scale
    as_t = lambda x: torch.as_tensor(x, device=dev).long().view(B, 1, 1, 1)
    p = as_t(past).clamp(0, Smax)
    n = (torch.full_like(p, Sq) if q_lens is None or "no_q_lens" in mut
         else as_t(q_lens).clamp(0, Sq))
    keys = torch.arange(Smax, device=dev).view(1, 1, 1, Smax)
    rows = torch.arange(Sq, device=dev).view(1, 1, Sq, 1)
    k, v = k.to(f64).clone(), v.to(f64).clone()
    total = p
    if k_new is not None:
        src = keys.view(1, 1, Smax, 1) - p
        hit = (src >= 0) & (src < n)
        at = src.clamp(0, Sq - 1).expand(B, Hk, Smax, D)
        k = torch.where(hit, k_new.to(f64).gather(2, at), k)
        v = torch.where(hit, v_new.to(f64).gather(2, at), v)
        total = (p + n).clamp(max=Smax)
    off = total - n
    if "causal+1" in mut:
        off = off + 1
    if "causal-1" in mut:
        off = off - 1
    limit = off + rows if causal else (total - 1).expand(B, 1, Sq, 1)
    limit = torch.minimum(limit, total - 1)
    mask = (rows < n) & (keys <= limit)                  # [B,1,Sq,Smax]
    if "drop_last" in mut:
        mask = mask & (keys != limit)
    if "drop_split_first" in mut:
        mask = mask & ~((keys % 128 == 0) & (keys > 0))
    live = (keys < total).view(B, 1, Smax, 1)
    kz, vz = torch.where(live, k, 0.0), torch.where(live, v, 0.0)
    qz = torch.where(rows < n, q.to(f64), 0.0)
    head = torch.arange(H, device=dev)
    kv_head = head % Hk if "gqa_mod" in mut else head // G
    s = torch.einsum("bhqd,bhkd->bhqk", qz, kz[:, kv_head]) * scale
    s = s.masked_fill(~mask, float("-inf"))
    some = mask.any(-1, keepdim=True)                    # [B,1,Sq,1]
    m = torch.where(some, s.amax(-1, keepdim=True), 0.0)
    pr = torch.exp(s - m)                                # masked: 0
    l = pr.sum(-1, keepdim=True)
    lse = torch.where(some, m + torch.log(l), float("-inf")).squeeze(-1)
    if emulate:     # the kernels' roundings: P to bf16 ahead of PV
        pr = pr.float().bfloat16().to(f64)
    out = torch.einsum("bhqk,bhkd->bhqd", pr, vz[:, kv_head])
    out = torch.where(some, out / torch.where(some, l, 1.0), 0.0)
    if emulate:
        out = out.float().bfloat16().to(f64)
    if decode:
        out, lse = out[:, :, 0], lse[:, :, 0]
    return out, lse, k, v


def cached_reference(q, k, v, past, q_lens=None, causal=True, scale=None,
                     k_new=None, v_new=None):
    """The documented contract of ``flash_attention_extend`` (q [B,H,Sq,D])
    and ``flash_attention_decode`` (q [B,H,D]) in fp64, vectorised, on q's
    device: k, v float [B,Hk,Smax,D] slabs (an e4m3 cache as ``cache.float()
    * scale``, new rows as the dequantised ``kv_quantize_reference`` of
    them), past and q_lens lists or tensors. One [B,1,Sq,Smax] visibility
    mask, bottom-right aligned when causal, total_b keys when not; a row that
    sees nothing or lies past q_lens gives a zero row and lse -inf. Returns
    (out, lse, k_after, v_after) in fp64."""
    return _reference(q, k, v, past, q_lens, causal, scale, k_new, v_new)


def _deq(c, s):
    return c.to(torch.float64) if s is None else (
        c.float().to(torch.float64) * s.to(torch.float64).view(1, -1, 1, 1))


def _stored(x, s, d):
    """New rows as an e4m3 cache under scale s stores them, read with d."""
    x4 = x if x.dim() == 4 else x.unsqueeze(2)
    y = _deq(kv_quantize_reference(x4, s), d)
    return y if x.dim() == 4 else y[:, :, 0]


def reference_of(r, mut=frozenset(), emulate=False, how=None):
    """``cached_reference`` of a built case r from its tensors as they are
    now. ``how``: an input-side mistake (see ``mutants``)."""
    c = r.case
    ks, vs = r.k_scale, r.v_scale
    dks, dvs = ks, vs       # what the caches are dequantised with
    if how == "kv_scale_swapped":
        dks, dvs = vs, ks
    if how == "v_scale_head0":
        dvs = vs[:1].expand_as(vs)
    kn, vn = r.k_new, r.v_new
    if c.fp8 and kn is not None and how != "append_unquantised":
        kn, vn = _stored(kn, ks, dks), _stored(vn, vs, dvs)
    k, v = r.logical(r.k_cache), r.logical(r.v_cache)
    if how == "page_swapped":
        P = c.P
        perm = torch.arange(c.Smax, device=k.device)
        perm[:2 * P] = torch.cat([perm[P:2 * P], perm[:P]])
        k, v = k[:, :, perm], v[:, :, perm]
    scale = None if how == "scale_ignored" else c.softmax_scale
    return _reference(r.q, _deq(k, dks), _deq(v, dvs), r.past, r.ql,
                      c.causal, scale, kn, vn, mut=mut, emulate=emulate)


def mutants():
    """name -> (applies(case), every, run(r)): wrong references, each one
    mistake a kernel could make. ``every``: the mutant must differ on every
    case it applies to, else on at least one."""
    ref = lambda **kw: (lambda r: reference_of(r, **kw)[:2])
    m = lambda name: ref(mut=frozenset([name]))
    ext = lambda c: c.op == "extend"
    return {
        "scale_ignored": (lambda c: c.scale != "none", True,
                          ref(how="scale_ignored")),
        "kv_scale_swapped": (lambda c: c.fp8, True,
                             ref(how="kv_scale_swapped")),
        "v_scale_head0": (lambda c: c.fp8 and c.heads[1] > 1, True,
                          ref(how="v_scale_head0")),
        "causal_off_plus": (lambda c: ext(c) and c.causal, False,
                            m("causal+1")),
        "causal_off_minus": (lambda c: ext(c) and c.causal, False,
                             m("causal-1")),
        "last_key_dropped": (lambda c: True, False, m("drop_last")),
        "split_first_key_dropped": (lambda c: True, False,
                                    m("drop_split_first")),
        "q_lens_ignored": (lambda c: c.ragged, False, m("no_q_lens")),
        "append_unquantised": (lambda c: c.fp8 and c.append != "none", False,
                               ref(how="append_unquantised")),
        "page_swapped": (lambda c: c.paged, False, ref(how="page_swapped")),
        "gqa_head_map": (lambda c: 1 < c.heads[1] < c.heads[0], False,
                         m("gqa_mod")),
    }


def differs(got, want, rtol, atol):
    """Does any element miss |got - want| <= atol + rtol |want| (a NaN or an
    infinity on one side only counts)?"""
    got, want = got.double(), want.double()
    same_inf = torch.isinf(want) & (got == want)
    ok = ((got - want).abs() <= atol + rtol * want.abs()) | same_inf
    return bool((~ok).any())
