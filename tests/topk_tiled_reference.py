"""The selection schedule of csn_l2_topk_tiled (csrc/retrieval_tiled.hip) in numpy, shared by
tests/test_topk_tiled_cpu.py and tests/test_gpu_topk_tiled.py (not a test module): the split ranges the host computes, the
ascending tile walk, the strict d < tau filter, the in-tile sort, the rank-computation merge with list entries first on
equal distance, truncation at k, and the pairwise cross-split merge.  Works on a given row of distances, so the distance
arithmetic is not part of it."""
import numpy as np

TILE = 64            # gallery rows per tile (TG) and queries per workgroup (TQ) of the kernel
MAX_K = 1024
MAX_SPLITS = 64      # cap of the library's own choice
TARGET_WGS = 512     # 256 CUs about twice over


def cdiv(a, b):
    return -(-a // b)


def splits_auto(Ng, Nq, tile=TILE):
    return max(1, min(cdiv(TARGET_WGS, cdiv(Nq, tile)), MAX_SPLITS, cdiv(Ng, tile)))


def splits_cap(Ng, Nq, tile=TILE):
    """The most splits a call may use, forced or not: the scratch is sized for it."""
    return min(max(splits_auto(Ng, Nq, tile), 8), cdiv(Ng, tile))


def split_ranges(Ng, Nq, splits=0, tile=TILE):
    """[(first row, one past the last row)] of every split, as csn_l2_topk_tiled lays them out: whole tiles, none empty."""
    gtiles = cdiv(Ng, tile)
    S = splits_auto(Ng, Nq, tile) if splits == 0 else min(splits, splits_cap(Ng, Nq, tile))
    tps = cdiv(gtiles, S)
    S = cdiv(gtiles, tps)
    return [(s * tps * tile, min(Ng, (s + 1) * tps * tile)) for s in range(S)]


def scratch_bytes(Ng, Nq, k):
    up = lambda v: cdiv(v, 256) * 256
    S = splits_cap(Ng, Nq)
    return 4 * up(S * Nq * k * 8) + up(S * Nq * 2 * 4)


def _merge_tile(list_d, list_i, cand_d, cand_i, k, list_first=True):
    """Sorted list + one tile's passing candidates -> the new list (at most k), by the kernel's rank computation."""
    order = np.lexsort((cand_i, cand_d))                       # the in-tile sort by (d, idx)
    cand_d, cand_i = cand_d[order], cand_i[order]
    n, nc = len(list_d), len(cand_d)
    out_d, out_i = np.full(min(k, n + nc), np.nan), np.full(min(k, n + nc), -1, dtype=np.int64)
    side_c, side_l = ("right", "left") if list_first else ("left", "right")
    pc = np.arange(nc) + np.searchsorted(list_d, cand_d, side=side_c)      # list entries with d <= cand d go first
    pl = np.arange(n) + np.searchsorted(cand_d, list_d, side=side_l)       # candidates with d < list d go first
    for p, d, i in list(zip(pc, cand_d, cand_i)) + list(zip(pl, list_d, list_i)):
        if p < k:
            assert out_i[p] == -1, "two entries computed the same rank"
            out_d[p], out_i[p] = d, i
    assert (out_i >= 0).all(), "a rank below k was left empty"
    return out_d, out_i


def _merge_lists(a_d, a_i, b_d, b_i, k):
    """Cross-split round: list a (lower index range) absorbs list b; a's entries first on equal distance."""
    pa = np.arange(len(a_d)) + np.searchsorted(b_d, a_d, side="left")
    pb = np.arange(len(b_d)) + np.searchsorted(a_d, b_d, side="right")
    n = min(k, len(a_d) + len(b_d))
    out_d, out_i = np.full(n, np.nan), np.full(n, -1, dtype=np.int64)
    for p, d, i in list(zip(pa, a_d, a_i)) + list(zip(pb, b_d, b_i)):
        if p < k:
            assert out_i[p] == -1
            out_d[p], out_i[p] = d, i
    return out_d, out_i


def emulate_row(d, k, ranges, tile=TILE, strict=True, ascending=True, list_first=True, stats=None):
    """d: float64 distances of ONE query to every gallery row.  -> (dist[k], idx[k]) as the two kernels produce them.
    strict / ascending / list_first switch off one rule of the schedule each (the tests show what then goes wrong);
    stats, a dict, counts the tile merges."""
    lists = []
    for (g_begin, g_end) in ranges:
        ld, li = np.zeros(0), np.zeros(0, dtype=np.int64)
        tau = np.inf
        starts = list(range(g_begin, g_end, tile))
        for g0 in (starts if ascending else starts[::-1]):
            idx = np.arange(g0, min(g0 + tile, g_end))
            dd = d[idx]
            passing = dd < tau if strict else dd <= tau
            if not passing.any():
                continue
            if stats is not None:
                stats["merges"] = stats.get("merges", 0) + 1
            ld, li = _merge_tile(ld, li, dd[passing], idx[passing], k, list_first)
            tau = ld[k - 1] if len(ld) == k else np.inf
        lists.append((ld, li))
    step = 1
    while step < len(lists):                                    # list a absorbs list a + step, as the merge kernel does
        for a in range(0, len(lists) - step, 2 * step):
            lists[a] = _merge_lists(*lists[a], *lists[a + step], k)
        step *= 2
    return lists[0]


def emulate(d2, k, ranges, **kw):
    """d2 [Nq, Ng] -> (dist [Nq,k], idx [Nq,k])."""
    rows = [emulate_row(r, k, ranges, **kw) for r in d2]
    return np.stack([r[0] for r in rows]), np.stack([r[1] for r in rows])


def d2_kernel_order(q, g):
    """The kernel's accumulation: ascending d, one chain per pair (unfused here: equal to the fused chain wherever every
    partial sum is exact, within D * 2**-53 relative elsewhere)."""
    q, g = q.astype(np.float64), g.astype(np.float64)
    d2 = np.zeros((q.shape[0], g.shape[0]))
    for d in range(q.shape[1]):
        df = q[:, d, None] - g[None, :, d]
        d2 += df * df
    return d2


def exact_topk(d2, k):
    """(dist, idx): the k smallest of every row under (distance, index)."""
    idx = np.stack([np.lexsort((np.arange(len(r)), r))[:k] for r in d2])
    return np.take_along_axis(d2, idx, axis=1), idx
