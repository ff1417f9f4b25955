"""The paged attention tests' helpers (not a test module): a contiguous KV
cache cut into a page pool with a shuffled block table, and back. The fp32
truth stays ``extend_reference`` on the contiguous cache; the pool a paged
call must leave is that reference's cache, paged the same way."""

import torch

SPARE = 3   # pages of the pool that no table needs


def repage(cache, table, P, totals=None):
    """The pool [N,Hk,P,D] that holds cache [B,Hk,Smax,D] (Smax a multiple
    of P) under table [B,Smax/P], N = B * Smax / P + SPARE. With totals only
    the pages a sequence of totals[b] keys needs are written; every other
    page is NaN."""
    B, Hk, Smax, D = cache.shape
    mp = Smax // P
    pool = cache.new_full((B * mp + SPARE, Hk, P, D), float("nan"))
    for b in range(B):
        used = mp if totals is None else -(-totals[b] // P)
        for j in range(used):
            pool[int(table[b, j])] = cache[b, :, j * P:(j + 1) * P]
    return pool


def to_pages(k_cache, v_cache, P, seed=0, totals=None):
    """(k_pool, v_pool, table int32 [B,Smax/P] on the caches' device). Pages
    are handed out by a seeded permutation. With totals, the entries that a
    sequence of totals[b] keys does not need all name one spare (NaN) page."""
    B, _, Smax, _ = k_cache.shape
    mp = Smax // P
    assert mp * P == Smax
    perm = torch.randperm(B * mp + SPARE,
                          generator=torch.Generator().manual_seed(seed))
    table = perm[:B * mp].view(B, mp).to(torch.int32)
    if totals is not None:
        for b, n in enumerate(totals):
            table[b, -(-n // P):] = perm[-1]
    return (repage(k_cache, table, P, totals), repage(v_cache, table, P, totals),
            table.to(k_cache.device))


def from_pages(pool, table):
    """The inverse: the [B,Hk,Smax,D] slab that table names in pool."""
    _, Hk, P, D = pool.shape
    B, mp = table.shape
    return pool[table.long()].transpose(1, 2).reshape(B, Hk, mp * P, D)


def bits(t):
    return t.detach().cpu().contiguous().view(torch.int16)
