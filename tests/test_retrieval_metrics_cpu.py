"""CPU: the host half of the device evaluation.  retrieval._fold_counts turns the integers of
csn_topk_class_metrics into the floats of retrieval._bookkeeping, retrieval.evaluate_device with a numpy engine returns the
dict of retrieval.evaluate_full, the numpy restatement of csn_topk_merge equals retrieval.merge_topk, and the library
exports the two entry points without a new ABI version."""
import os
import re
import subprocess
import sys
from types import SimpleNamespace

import numpy as np
import pytest
import torch.distributed as dist
import torch.multiprocessing as mp

import retrieval_metrics_reference as ref
import retrieval_metrics_stream_cases  # noqa: F401  (joins the stream-order case table on import)
from cerebralsignalnetworks_amd import cabi, retrieval

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NG = 120


def _labels(ids):
    return [ref.label(c) for c in ids]


def _both(I, g_cls, q_cls, n_classes, k):
    """(_fold_counts on the reference's integers, _bookkeeping) on the same neighbour lists."""
    ds = ref.Dataset(n_classes)
    out = ref.class_metrics(I, g_cls, q_cls, n_classes)
    got = retrieval._fold_counts(out["class"], k, ds.class_id_to_str, query_class=q_cls, pred=out["pred"],
                                 top1_correct=out["top1_correct"])
    want = retrieval._bookkeeping(I, _labels(g_cls), _labels(q_cls), ds.class_id_to_str, ds.class_str_to_id, k)
    return got, want


# ---- 1. _fold_counts against _bookkeeping ---------------------------------------------------------------------------------
@pytest.mark.parametrize("Nq", [1, 70])
@pytest.mark.parametrize("k", [1, 5, 64])
@pytest.mark.parametrize("n_classes", [1, 7, 40])
def test_fold_counts_equals_bookkeeping(n_classes, k, Nq):
    g_cls, q_cls = ref.label_set(n_classes, NG, Nq, seed=n_classes + k)
    if n_classes >= 3:
        assert n_classes - 1 in g_cls and n_classes - 1 not in q_cls            # a class of the gallery only
        assert Nq == 1 or (n_classes - 2 in q_cls and n_classes - 2 not in g_cls)      # and one of the queries only
    I = ref.neighbour_lists(g_cls, q_cls, k, seed=100 + k)
    (recall, precision, scores, top1), want = _both(I, g_cls, q_cls, n_classes, k)
    assert recall == want[0] and precision == want[1] and top1 == want[3]
    assert list(scores) == list(want[2])                                        # first appearance among the queries
    for name, rec in want[2].items():
        assert scores[name] == rec and list(scores[name]) == list(rec), name


def test_fold_counts_takes_the_means_in_order_of_first_appearance():
    """Label set found by a seeded search (seeds 0 .. 14 of this very construction): the mean of the per-class Recall, and
    that of the Precision, differ in the last bit between the order of first appearance and the ascending class order --
    numpy's mean is a pairwise sum."""
    n, Nq, k, seed = 40, 130, 5, 14
    rng = np.random.default_rng(seed)
    g_cls, q_cls = rng.integers(0, n, 200), rng.integers(0, n, Nq)
    I = ref.neighbour_lists(g_cls, q_cls, k, seed + 1)
    (recall, precision, scores, top1), want = _both(I, g_cls, q_cls, n, k)
    by_id = [scores[f"class_{c}"] for c in range(n) if f"class_{c}" in scores]
    assert list(scores) != [f"class_{c}" for c in range(n) if f"class_{c}" in scores]
    assert float(np.array([v["Recall"] for v in by_id]).mean()) != want[0]
    assert float(np.array([v["Precision"] for v in by_id]).mean()) != want[1]
    assert (recall, precision, scores, top1) == want


# ---- 2. evaluate_device with the numpy engine against evaluate_full -------------------------------------------------------
def _features(g_cls, q_cls, n_classes, seed, d=8):
    rng = np.random.default_rng(seed)
    cents = rng.integers(-3, 4, (n_classes, d)).astype(np.float64)
    gal = (cents[g_cls] + rng.integers(-1, 2, (len(g_cls), d))).astype(np.float32)      # integer grid: ties
    qry = (cents[q_cls] + rng.integers(-1, 2, (len(q_cls), d))).astype(np.float32)
    return gal, qry


def _assert_same_result(got, want):
    assert set(got) == set(want)
    for key in want:
        if key in ("D", "I"):
            assert np.asarray(got[key]).dtype == want[key].dtype
            np.testing.assert_array_equal(np.asarray(got[key]), want[key], err_msg=key)
        else:
            assert got[key] == want[key], key
    assert list(got["class_scores"]) == list(want["class_scores"])


@pytest.mark.parametrize("n_classes,k,Nq", [(1, 5, 70), (7, 1, 70), (7, 5, 1), (40, 5, 70), (40, 64, 70)])
def test_evaluate_device_with_numpy_engine_equals_evaluate_full(monkeypatch, n_classes, k, Nq):
    g_cls, q_cls = ref.label_set(n_classes, NG, Nq, seed=3 * n_classes + k)
    gal, qry = _features(g_cls, q_cls, n_classes, seed=k)
    ds, flags = ref.Dataset(n_classes), SimpleNamespace(topK=k)
    monkeypatch.setattr(retrieval, "l2_search", ref.search)
    want = retrieval.evaluate_full(flags, gal, qry, _labels(g_cls), _labels(q_cls), ds)
    got = retrieval.evaluate_device(flags, gal, qry, _labels(g_cls), _labels(q_cls), ds, engine=ref.NUMPY_ENGINE)
    _assert_same_result(got, want)
    # class ids instead of label dicts (the names come from the dataset), lists of rows instead of arrays
    got = retrieval.evaluate_device(flags, list(gal), list(qry), g_cls, q_cls.astype(np.int32), ds, engine=ref.NUMPY_ENGINE)
    _assert_same_result(got, want)


# ---- 3. the merge contract against merge_topk -----------------------------------------------------------------------------
MERGE_CASES = ref.merge_cases()


def test_merge_cases_cover_what_they_claim():
    ids = [c[0] for c in MERGE_CASES]
    assert len(ids) == len(set(ids)) and any("pad-inf" in i for i in ids)
    for P in (1, 3, 8):
        for k_in in (1, 5, 64):
            assert {k for _, D, _, k in MERGE_CASES if D.shape[0] == P and D.shape[2] == k_in} == \
                {k for k in (1, 5, k_in, min(P * k_in, 100)) if k <= P * k_in}
    name, D, I, k = next(c for c in MERGE_CASES if c[0] == "P3-kin64-k100-pad-inf")
    assert (I[2, :, 32:] == -1).all() and np.isinf(D[2, 0, 31]) and I[2, 0, 31] >= 0       # a real +inf beside padding
    assert len(np.unique(D[np.isfinite(D)])) <= 4                                          # ties inside and across parts


@pytest.mark.parametrize("case", MERGE_CASES, ids=lambda c: c[0])
def test_merge_reference_equals_merge_topk(case):
    _, D, I, k = case
    want_d, want_i = retrieval.merge_topk(list(D), list(I), k)
    got_d, got_i = ref.merge(D, I, k)
    np.testing.assert_array_equal(got_i, want_i)
    np.testing.assert_array_equal(got_d, want_d)


def test_merge_reference_orders_equal_pairs_like_merge_topk():
    """The same (distance, index) pair in two parts: both stay, in order of position."""
    D = np.array([[[1.0, 2.0]], [[1.0, 3.0]]])
    I = np.array([[[4, 5]], [[4, 6]]])
    want = retrieval.merge_topk(list(D), list(I), 3)
    got = ref.merge(D, I, 3)
    np.testing.assert_array_equal(got[1], [[4, 4, 5]])
    np.testing.assert_array_equal(got[0], want[0])
    np.testing.assert_array_equal(got[1], want[1])


def test_merge_with_too_few_candidates_is_refused():
    D, I = ref.merge_case(2, 3, 4, seed=5, pad_parts={0: 1, 1: 2})
    for fn in (retrieval.merge_topk, ref.merge):
        fn(list(D), list(I), 3)
        with pytest.raises(ValueError, match="fewer than k=4"):
            fn(list(D), list(I), 4)
    np.testing.assert_array_equal(ref.topk_merge(D, I, 4)[1][:, 3], [-1, -1, -1])           # the kernel's contract: padding
    assert np.isinf(ref.topk_merge(D, I, 4)[0][:, 3]).all()


# ---- 4. the precondition --------------------------------------------------------------------------------------------------
def test_evaluate_device_refuses_class_maps_it_cannot_count_by():
    g_cls, q_cls = ref.label_set(7, NG, 20, seed=1)
    gal, qry = _features(g_cls, q_cls, 7, seed=1)
    flags = SimpleNamespace(topK=5)

    searches = []
    engine = (lambda *a: searches.append(1) or ref.search(*a), ref.merge, ref.class_metrics)

    def run(ds, ql=None):
        return retrieval.evaluate_device(flags, gal, qry, _labels(g_cls), ql or _labels(q_cls), ds, engine=engine)

    good = ref.Dataset(7)
    run(good)
    assert searches == [1]
    twice = ref.Dataset(7)
    twice.class_id_to_str[6] = twice.class_id_to_str[2]                # two ids, one name
    with pytest.raises(ValueError, match="not injective.*evaluate_full"):
        run(twice)
    with pytest.raises(ValueError, match="ClassName.*evaluate_full"):   # a label whose name is not the map's
        run(good, ql=[dict(ref.label(c), ClassName="other") for c in q_cls])
    back = ref.Dataset(7)
    back.class_str_to_id["class_0"] = 3                                # Predicted would not come back to the id
    with pytest.raises(ValueError, match="class_str_to_id.*evaluate_full"):
        run(back)
    with pytest.raises(ValueError, match="not in class_id_to_str.*evaluate_full"):
        retrieval.evaluate_device(flags, gal, qry, g_cls + 1, q_cls, good, engine=engine)
    assert searches == [1]                                              # every refusal came before the search


# ---- 5. exports -----------------------------------------------------------------------------------------------------------
NAMES = ("csn_topk_merge", "csn_topk_class_metrics")


def test_header_declares_and_library_exports_both_entry_points():
    text = open(os.path.join(ROOT, "include", "csn_hip.h")).read()
    for name in NAMES:
        assert re.search(rf"^int {name}\(", text, flags=re.M), name
    assert re.search(r"^#define CSN_ABI_VERSION 6$", text, flags=re.M)
    listed = text[text.index("A symbol added beside the existing ones"):text.index("#define CSN_ABI_VERSION")]
    assert all(name in listed for name in NAMES)
    symbols = subprocess.run(["nm", "-D", "--defined-only", cabi.LIB_PATH], check=True, capture_output=True, text=True).stdout
    exported = {line.split()[-1] for line in symbols.splitlines() if line.strip()}
    assert set(NAMES) <= exported
    lib = cabi.load()
    assert lib.csn_abi_version() == 6 == cabi.ABI_VERSION
    assert lib.csn_topk_merge_staged_max() == cabi.TOPK_MERGE_STAGED_MAX


def test_bad_arguments_are_refused_on_the_host():
    """Without a GPU: every refusal below returns before anything touches the device."""
    lib = cabi.load()
    p = 0x1000                                                          # never dereferenced on the host
    for args, text in (((None, p, 2, 3, 4, 4, p, None, None, None), b"null"), ((p, p, 2, 3, 4, 4, None, None, None, None), b"null"),
                       ((p, p, 2, 3, 4, 1025, p, None, None, None), b"at most 1024"), ((p, p, 65, 3, 4, 4, p, None, None, None), b"at most 64"),
                       ((p, p, 2, 3, 1025, 4, p, None, None, None), b"at most 1024"), ((p, p, 2, 3, 4, 9, p, None, None, None), b"fewer than k"),
                       ((p, p, 2, 0, 4, 4, p, None, None, None), b"bad shape"), ((p, p, 2, 3, 4, 0, p, None, None, None), b"bad shape")):
        assert lib.csn_topk_merge(*args) == 1 and text in lib.csn_last_error(), (args, lib.csn_last_error())
    for args, text in (((None, 3, 5, p, 9, p, 4, p, None, None, None, None, None), b"null"),
                       ((p, 3, 5, None, 9, p, 4, p, None, None, None, None, None), b"null"),
                       ((p, 3, 5, p, 9, None, 4, p, None, None, None, None, None), b"null"),
                       ((p, 3, 5, p, 9, p, 4, None, None, None, None, None, None), b"every output is null"),
                       ((p, 0, 5, p, 9, p, 4, p, None, None, None, None, None), b"bad shape"),
                       ((p, 3, 1025, p, 9, p, 4, p, None, None, None, None, None), b"at most 1024"),
                       ((p, 3, 5, p, 9, p, 65537, p, None, None, None, None, None), b"at most 65536")):
        assert lib.csn_topk_class_metrics(*args) == 1 and text in lib.csn_last_error(), (args, lib.csn_last_error())


def test_bindings_refuse_host_tensors():
    import torch
    D, I = (torch.from_numpy(a) for a in ref.merge_case(2, 3, 4, seed=1))
    with pytest.raises(cabi.CsnError, match="device tensors"):
        cabi.topk_merge(D, I, 2)
    with pytest.raises(cabi.CsnError, match="device tensors"):
        cabi.topk_class_metrics(I[0], torch.zeros(9, dtype=torch.int32), torch.zeros(3, dtype=torch.int32), 1)
    with pytest.raises(cabi.CsnError, match="device tensors"):
        retrieval.l2_search_device(torch.zeros(4, 2), torch.zeros(2, 2), 1)


# ---- 6. evaluate_distributed(on_device=True), two gloo ranks, numpy engine -------------------------------------------------
TOPK = 12
SHARDS = (9, 81)                 # uneven, rank 0's shard is smaller than topK
QSHARDS = (20, 13)


def _eval_data():
    g_cls, q_cls = ref.label_set(6, sum(SHARDS), sum(QSHARDS), seed=11)
    gal, qry = _features(g_cls, q_cls, 6, seed=11)
    return gal, qry, _labels(g_cls), _labels(q_cls)


def _worker(rank, world, port, out):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world))
    dist.init_process_group("gloo", rank=rank, world_size=world)
    sys.path.insert(0, ROOT)
    gal, qry, gl, ql = _eval_data()
    g0, q0 = sum(SHARDS[:rank]), sum(QSHARDS[:rank])
    gs, qs = slice(g0, g0 + SHARDS[rank]), slice(q0, q0 + QSHARDS[rank])
    search64 = lambda g, q, k: ref.oracle_retrieval.l2_topk(g, q, k)                   # float64 distances
    res = {}
    for name, kw in (("sharded", dict(search_fn=search64, shard_gallery=True)), ("replicated", dict(search_fn=ref.search))):
        for on_device in (False, True):
            r = retrieval.evaluate_distributed(SimpleNamespace(topK=TOPK), gal[gs], qry[qs], gl[gs], ql[qs], ref.Dataset(6),
                                               on_device=on_device, engine=ref.NUMPY_ENGINE, **kw)
            res[name, on_device] = r
    out[rank] = res
    dist.barrier()
    dist.destroy_process_group()


def test_distributed_eval_on_device_two_process_gloo(monkeypatch):
    """on_device=True (merge and metrics through the engine) returns, on both ranks and for both forms, the dict of the
    default path and of a single-process evaluate_full over the concatenated data."""
    world, port = 2, 29693
    out = mp.Manager().dict()
    mp.spawn(_worker, args=(world, port, out), nprocs=world, join=True)
    gal, qry, gl, ql = _eval_data()
    monkeypatch.setattr(retrieval, "l2_search", ref.search)
    want = retrieval.evaluate_full(SimpleNamespace(topK=TOPK), gal, qry, gl, ql, ref.Dataset(6))
    for r in range(world):
        for form in ("sharded", "replicated"):
            _assert_same_result(out[r][form, False], want)
            _assert_same_result(out[r][form, True], want)
