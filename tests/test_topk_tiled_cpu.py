"""CPU: the tiled L2 top-k (csn_l2_topk_tiled) as far as it can be checked without a GPU -- the two
symbols and their host-side refusals, the scratch formula, the selection schedule in numpy against a plain sort,
retrieval.merge_topk, and evaluate_distributed(shard_gallery=True) on two gloo ranks with the oracle as the search."""
import os
import sys

import numpy as np
import pytest
import torch.distributed as dist
import torch.multiprocessing as mp

import __graft_entry__ as graft
import topk_tiled_reference as ref
from cerebralsignalnetworks_amd import cabi, retrieval
from oracle import retrieval as oracle_retrieval

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(cabi.LIB_PATH):
        graft.build()
    return cabi.load()


# ---- 1. ABI -------------------------------------------------------------------------------------------------------------
def test_tiled_symbols_are_exported_and_declared(lib):
    text = open(os.path.join(ROOT, "include", "csn_hip.h")).read()
    for name in ("csn_l2_topk_tiled", "csn_l2_topk_tiled_scratch_bytes"):
        assert name in cabi.SIGNATURES and hasattr(lib, name)
        assert name + "(" in text
    assert lib.csn_abi_version() == cabi.ABI_VERSION == 6, "a symbol added beside the old one does not bump the ABI"


def test_tiled_refusals_happen_on_the_host(lib):
    """No GPU here: every one of these returns before any launch, with a message."""
    one = 1 << 12                        # any non-null address: refused arguments are never dereferenced

    def call(Ng=100, Nq=10, D=4, k=5, splits=0, g=one, q=one, idx=one, dist=one, d64=None, scratch=one):
        return lib.csn_l2_topk_tiled(g, q, Ng, Nq, D, k, splits, idx, dist, d64, scratch, None)

    assert lib.csn_l2_topk_tiled(None, None, 10, 10, 4, 5, 0, None, None, None, None, None) == 1     # CSN_ERR_INVALID_ARGUMENT
    assert b"null" in lib.csn_last_error()
    for null in ("g", "q", "idx", "dist", "scratch"):
        assert call(**{null: None}) == 1 and b"null" in lib.csn_last_error(), null
    for kw, word in ((dict(k=0), b"k=0"), (dict(Ng=3, k=5), b"k=5"), (dict(Ng=5000, k=1025), b"k=1025"),
                     (dict(splits=-1), b"splits=-1"), (dict(Ng=0), b"shape"), (dict(Nq=0), b"shape"), (dict(D=0), b"shape"),
                     (dict(Ng=-4), b"shape")):
        assert call(**kw) == 1, kw
        assert word in lib.csn_last_error(), (kw, lib.csn_last_error())
    for (Ng, Nq, k) in ((100, 10, 0), (3, 10, 5), (5000, 10, 1025), (0, 10, 1), (10, 0, 1), (10, -1, 1)):
        assert lib.csn_l2_topk_tiled_scratch_bytes(Ng, Nq, k) == 0, (Ng, Nq, k)
        assert lib.csn_last_error()
    assert lib.csn_l2_topk_tiled_scratch_bytes(5000, 10, 1024) > 0


def test_tiled_scratch_does_not_scale_with_the_gallery(lib):
    """[Nq,Ng] float64 at 1<<20 x 4096 would be 32 GiB.  The lists: two buffers of 16 bytes per (split, query, rank)."""
    b20 = lib.csn_l2_topk_tiled_scratch_bytes(1 << 20, 4096, 64)
    assert 0 < b20 <= 1 << 30
    assert lib.csn_l2_topk_tiled_scratch_bytes(1 << 24, 4096, 64) == b20
    for (Ng, Nq, k) in ((1 << 20, 4096, 64), (300, 4, 65), (2048, 512, 5), (5000, 3, 1024), (1, 1, 1), (262144, 2048, 10)):
        got = lib.csn_l2_topk_tiled_scratch_bytes(Ng, Nq, k)
        assert got == ref.scratch_bytes(Ng, Nq, k)
        S = ref.splits_cap(Ng, Nq)
        assert S <= ref.MAX_SPLITS and got <= 2 * S * Nq * k * 16 + S * Nq * 8 + 5 * 256


# ---- 2. the selection schedule ------------------------------------------------------------------------------------------
SCHEDULE_CASES = [(300, 4, 8, 64, 1, 64), (300, 4, 8, 65, 3, 64), (1000, 3, 4, 256, 7, 64), (70, 2, 3, 70, 5, 16),
                  (129, 3, 2, 1, 2, 64), (500, 2, 1, 200, 4, 32)]


def _tie_heavy(Ng, Nq, D, seed):
    rng = np.random.default_rng(seed)
    g = rng.integers(-2, 3, (Ng, D)).astype(np.float32)
    q = rng.integers(-2, 3, (Nq, D)).astype(np.float32)
    return ref.d2_kernel_order(q, g)


@pytest.mark.parametrize("Ng,Nq,D,k,splits,tile", SCHEDULE_CASES)
def test_schedule_emulator_equals_the_sort(Ng, Nq, D, k, splits, tile):
    d2 = _tie_heavy(Ng, Nq, D, seed=Ng + k)
    assert len(np.unique(d2)) < Ng // 2, "not tie-heavy"
    ranges = ref.split_ranges(Ng, Nq, splits, tile)
    assert ranges[0][0] == 0 and ranges[-1][1] == Ng and all(a[1] == b[0] for a, b in zip(ranges, ranges[1:]))
    assert all(b > a for a, b in ranges) and len(ranges) <= splits
    want_d, want_i = ref.exact_topk(d2, k)
    got_d, got_i = ref.emulate(d2, k, ranges, tile=tile)
    np.testing.assert_array_equal(got_i, want_i)
    np.testing.assert_array_equal(got_d, want_d)


def test_schedule_emulator_sees_each_rule():
    """Every rule of the tie argument, switched off alone, on the six cases: which of them the comparison with the sort
    catches.  Walking the tiles in descending order breaks it (a later tile then holds LOWER indices, and 'list entries
    first' is the wrong way round), and so does merging candidates ahead of equal list entries.  Replacing < by <= in the
    filter does not change the result under THIS merge: a candidate that ties tau is ranked behind every list entry of that
    distance, which is rank k or later, and falls to the truncation -- the strict filter is what keeps it from being
    staged, sorted and merged at all, which the merge count shows (every tile of a tie-heavy row merges again)."""
    broken = {"descending": 0, "candidates_first": 0}
    merges = {"<": 0, "<=": 0}
    for (Ng, Nq, D, k, splits, tile) in SCHEDULE_CASES:
        d2 = _tie_heavy(Ng, Nq, D, seed=Ng + k)
        ranges = ref.split_ranges(Ng, Nq, splits, tile)
        _, want_i = ref.exact_topk(d2, k)
        broken["descending"] += int(not np.array_equal(ref.emulate(d2, k, ranges, tile=tile, ascending=False)[1], want_i))
        broken["candidates_first"] += int(not np.array_equal(ref.emulate(d2, k, ranges, tile=tile, list_first=False)[1], want_i))
        s_strict, s_loose = {}, {}
        ref.emulate(d2, k, ranges, tile=tile, stats=s_strict)
        loose_i = ref.emulate(d2, k, ranges, tile=tile, strict=False, stats=s_loose)[1]
        np.testing.assert_array_equal(loose_i, want_i)
        merges["<"] += s_strict["merges"]
        merges["<="] += s_loose["merges"]
    assert broken["descending"] >= 3 and broken["candidates_first"] >= 3, broken
    assert merges["<="] > merges["<"], merges


# ---- 3. merge_topk ------------------------------------------------------------------------------------------------------
def _parts(g, q, k, cuts):
    """Oracle results per contiguous gallery part [cuts[i], cuts[i+1]), indices rebased, padded to k with (+inf, -1)."""
    Dp, Ip = [], []
    for a, b in zip(cuts, cuts[1:]):
        D = np.full((len(q), k), np.inf)
        I = np.full((len(q), k), -1, dtype=np.int64)
        kr = min(k, b - a)
        if kr:
            d, i = oracle_retrieval.l2_topk(g[a:b], q, kr)
            D[:, :kr], I[:, :kr] = d, i + a
        Dp.append(D)
        Ip.append(I)
    return Dp, Ip


@pytest.mark.parametrize("cuts", [(0, 200), (0, 93, 200), (0, 7, 7, 60, 131, 200)], ids=["1part", "2parts", "5parts"])
def test_merge_topk_of_contiguous_parts_equals_the_whole(cuts):
    """5 parts: one empty (7..7), one shorter than k (0..7)."""
    rng = np.random.default_rng(5)
    g = rng.integers(-3, 4, (200, 6)).astype(np.float32)          # tie-heavy: the index decides often
    q = rng.integers(-3, 4, (9, 6)).astype(np.float32)
    k = 20
    want_d, want_i = oracle_retrieval.l2_topk(g, q, k)
    got_d, got_i = retrieval.merge_topk(*_parts(g, q, k, cuts), k)
    assert got_d.dtype == np.float64 and got_i.dtype == np.int64
    np.testing.assert_array_equal(got_i, want_i)
    np.testing.assert_array_equal(got_d, want_d)


def test_merge_topk_needs_the_float64_distances():
    """Two distances that differ in float64 and collide in float32: the smaller one sits at the HIGHER index, in the other
    part.  Merging the float32 roundings would see a tie and prefer the lower index."""
    a, b = 1.0 + 2.0 ** -30, 1.0 + 2.0 ** -31
    assert a != b and np.float32(a) == np.float32(b)
    D_parts = [np.array([[0.5, a]]), np.array([[b, np.inf]])]
    I_parts = [np.array([[0, 1]]), np.array([[2, -1]])]
    d, i = retrieval.merge_topk(D_parts, I_parts, 3)
    np.testing.assert_array_equal(i, [[0, 2, 1]])
    np.testing.assert_array_equal(d, [[0.5, b, a]])
    d32, i32 = retrieval.merge_topk([p.astype(np.float32) for p in D_parts], I_parts, 3)
    np.testing.assert_array_equal(i32, [[0, 1, 2]])               # what a float32 merge would have returned
    with pytest.raises(ValueError):
        retrieval.merge_topk(D_parts, I_parts, 4)                 # only three real candidates


# ---- 4. evaluate_distributed(shard_gallery=True), two gloo ranks ---------------------------------------------------------
TOPK = 12
SHARDS = (9, 81)                 # uneven, rank 0's shard is smaller than topK
QSHARDS = (20, 13)


def _eval_data(seed=11, ng=90, nq=33, d=8, ncls=6):
    rng = np.random.default_rng(seed)
    cents = rng.integers(-3, 4, (ncls, d)).astype(np.float64)
    gl = rng.integers(0, ncls, ng)
    ql = rng.integers(0, ncls, nq)
    gal = (cents[gl] + rng.integers(-1, 2, (ng, d))).astype(np.float32)      # integer grid: ties across the shard border
    qry = (cents[ql] + rng.integers(-1, 2, (nq, d))).astype(np.float32)
    lab = lambda k: {"ClassId": int(k), "ClassName": f"class_{int(k)}", "imagenetClassId": str(int(k))}
    return gal, qry, [lab(k) for k in gl], [lab(k) for k in ql], ncls


class _DS:
    def __init__(self, ncls):
        self.class_id_to_str = {k: f"class_{k}" for k in range(ncls)}
        self.class_str_to_id = {f"class_{k}": k for k in range(ncls)}


def _shard_worker(rank, world, port, out):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world))
    dist.init_process_group("gloo", rank=rank, world_size=world)
    sys.path.insert(0, ROOT)
    from types import SimpleNamespace
    from cerebralsignalnetworks_amd import retrieval
    from oracle import retrieval as oracle_retrieval
    gal, qry, gl, ql, ncls = _eval_data()
    g0, q0 = sum(SHARDS[:rank]), sum(QSHARDS[:rank])
    gs, qs = slice(g0, g0 + SHARDS[rank]), slice(q0, q0 + QSHARDS[rank])
    search64 = lambda g, q, k: oracle_retrieval.l2_topk(g, q, k)                       # float64 distances
    search32 = lambda g, q, k: tuple(a.astype(t) for a, t in zip(oracle_retrieval.l2_topk(g, q, k), (np.float32, np.int64)))
    res = {}
    for name, kw in (("sharded", dict(search_fn=search64, shard_gallery=True)), ("replicated", dict(search_fn=search32))):
        r = retrieval.evaluate_distributed(SimpleNamespace(topK=TOPK), gal[gs], qry[qs], gl[gs], ql[qs], _DS(ncls), **kw)
        res[name] = (r["Recall_Total"], r["Precision_Total"], r["top1"], r["I"].copy(), r["D"].copy())
    try:
        retrieval.evaluate_distributed(SimpleNamespace(topK=TOPK), gal[gs], qry[qs], gl[gs], ql[qs], _DS(ncls),
                                       search_fn=search32, shard_gallery=True)
        res["float32 refused"] = False
    except TypeError:
        res["float32 refused"] = True
    out[rank] = res
    dist.barrier()
    dist.destroy_process_group()


def test_sharded_gallery_eval_two_process_gloo():
    """The gallery stays sharded (9 + 81 rows, topK = 12 > 9): both ranks get the Recall / Precision / top-1 / I / D of
    the replicated form and of a single-process evaluation over the concatenated data."""
    world, port = 2, 29671
    out = mp.Manager().dict()
    mp.spawn(_shard_worker, args=(world, port, out), nprocs=world, join=True)
    gal, qry, gl, ql, ncls = _eval_data()
    rec, prec, _, top1, D, I = oracle_retrieval.evaluate(gal, qry, gl, ql, _DS(ncls).class_id_to_str, topK=TOPK)
    for r in range(world):
        assert out[r]["float32 refused"]
        for form in ("sharded", "replicated"):
            got = out[r][form]
            assert (got[0], got[1], got[2]) == (rec, prec, top1), (r, form, got[:3], (rec, prec, top1))
            np.testing.assert_array_equal(got[3], I, err_msg=f"I, rank {r}, {form}")
            assert got[4].dtype == np.float32
            np.testing.assert_array_equal(got[4], D.astype(np.float32), err_msg=f"D, rank {r}, {form}")
