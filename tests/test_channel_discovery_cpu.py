"""CPU: channel discovery (csrc/channel_l2.hip, channel_discovery.py) as far as it can be checked
without a GPU -- the three symbols and their host-side refusals, the decomposition of a subset's distances into per-channel
matrices against the flat feature, and the greedy driver with the numpy engine against the naive restatement of the
reference loop."""
import ctypes
import os

import numpy as np
import pytest

import __graft_entry__ as graft
import channel_discovery_reference as ref
import channel_discovery_stream_cases as stream_cases      # joins the stream-order case table on import
import stream_order as so
from cerebralsignalnetworks_amd import cabi
from oracle import retrieval as oracle_retrieval

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("csn_chan_l2_dist", "csn_chan_l2_select", "csn_chan_l2_accumulate")
INVALID = 1                              # CSN_ERR_INVALID_ARGUMENT


@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(cabi.LIB_PATH):
        graft.build()
    return cabi.load()


# ---- 1. ABI -------------------------------------------------------------------------------------------------------------
def test_channel_symbols_are_exported_and_declared(lib):
    text = open(os.path.join(ROOT, "include", "csn_hip.h")).read()
    for name in NAMES:
        assert name in cabi.SIGNATURES and hasattr(lib, name)
        assert name + "(" in text
    assert lib.csn_abi_version() == cabi.ABI_VERSION == 6, "added symbols do not bump the ABI"


def test_python_surface_exists():
    from cerebralsignalnetworks_amd import channel_discovery as cd
    for name in ("channel_distances", "discover_channels", "HIP_ENGINE"):
        assert hasattr(cd, name)
    for name in ("chan_l2_dist", "chan_l2_select", "chan_l2_accumulate"):
        assert hasattr(cabi, name)


def test_stream_order_cases_are_registered():
    """The three entry points take a csnStream_t, so each needs a stream-order case: tests/test_stream_order_cpu.py holds
    the case table against the header, tests/test_gpu_channel_discovery.py runs the cases."""
    for name in NAMES:
        cases = so.CASE_TABLE[name]
        assert cases is stream_cases.CASES[name] and cases
        assert all(isinstance(c, so.Stateless) and c.entry == name and callable(c.build) for c in cases)
    ids = [c.id for v in stream_cases.CASES.values() for c in v]
    assert len(set(ids)) == len(ids) and not set(ids) & {c.id for c in so.STATELESS_CASES}
    n = len(so.CASE_TABLE)
    stream_cases.register()
    assert len(so.CASE_TABLE) == n, "registering twice adds nothing"


# ---- 2. refusals --------------------------------------------------------------------------------------------------------
ONE = 1 << 12                            # any non-null address: refused arguments are never dereferenced


def _refused(lib, rc, word):
    msg = lib.csn_last_error()
    assert rc == INVALID, (rc, msg)
    assert word in msg, (word, msg)


def test_dist_refusals_happen_on_the_host(lib):
    """No GPU here: every one of these returns before any launch, with a message."""
    def call(g=ONE, q=ONE, Dc=ONE, Ng=10, Nq=7, C=4, T=20, t0=2, t1=18, channels=None, g_ld=None, q_ld=None):
        g_ld = g_ld or (C * T, T)
        q_ld = q_ld or (C * T, T)
        arr = None if channels is None else (ctypes.c_int32 * len(channels))(*channels)
        return lib.csn_chan_l2_dist(g, g_ld[0], g_ld[1], q, q_ld[0], q_ld[1], Ng, Nq, C, T, t0, t1, arr,
                                    0 if channels is None else len(channels), Dc, None)

    for null in ("g", "q", "Dc"):
        _refused(lib, call(**{null: None}), b"null")
    for kw in (dict(Ng=0), dict(Nq=0), dict(C=0), dict(T=0), dict(Ng=-3), dict(Nq=-1)):
        _refused(lib, call(**kw), b"shape")
    for kw in (dict(t0=-1), dict(t1=21), dict(t0=5, t1=5), dict(t0=9, t1=3), dict(t0=20, t1=21)):
        _refused(lib, call(**kw), b"window")
    for kw in (dict(channels=[0, 4]), dict(channels=[-1]), dict(channels=[1, 2, 3, 17])):
        _refused(lib, call(**kw), b"outside [0, C=4)")
    _refused(lib, call(channels=[]), b"nch")
    _refused(lib, call(g_ld=(80, 19)), b"gallery ld_c=19")
    _refused(lib, call(q_ld=(80, 19)), b"query ld_c=19")
    _refused(lib, call(g_ld=(79, 20)), b"gallery ld_n=79")
    _refused(lib, call(q_ld=(3 * 25 + 19, 25)), b"query ld_n=94")
    _refused(lib, call(Ng=64 * 65535 + 1), b"too large")


def test_select_refusals_happen_on_the_host(lib):
    def call(base=None, Dc=ONE, nc=3, Nq=7, Ng=10, gc=ONE, qc=ONE, k=5, idx=ONE, dist=ONE, hits=ONE, top1=ONE):
        return lib.csn_chan_l2_select(base, Dc, nc, Nq, Ng, gc, qc, k, idx, dist, hits, top1, None)

    _refused(lib, call(Dc=None), b"null")
    _refused(lib, call(gc=None), b"null")
    _refused(lib, call(qc=None), b"null")
    _refused(lib, call(gc=None, hits=None), b"null")                    # out_top1 still needs the gallery classes
    _refused(lib, call(idx=None, dist=None, hits=None, top1=None), b"every output is null")
    for kw in (dict(nc=0), dict(Nq=0), dict(Ng=0), dict(Ng=-5)):
        _refused(lib, call(**kw), b"shape")
    for kw, word in ((dict(k=0), b"k=0"), (dict(k=-2), b"k=-2"), (dict(k=11), b"k=11"), (dict(Ng=500, k=65), b"k=65")):
        _refused(lib, call(**kw), word)
    _refused(lib, call(nc=65536), b"too large")


def test_accumulate_refusals_happen_on_the_host(lib):
    _refused(lib, lib.csn_chan_l2_accumulate(None, ONE, 10, 0, None), b"null")
    _refused(lib, lib.csn_chan_l2_accumulate(ONE, None, 10, 1, None), b"null")
    _refused(lib, lib.csn_chan_l2_accumulate(ONE, ONE, 0, 1, None), b"n=0")
    _refused(lib, lib.csn_chan_l2_accumulate(ONE, ONE, -4, 0, None), b"n=-4")


def test_bindings_refuse_host_tensors():
    import torch
    x = torch.zeros(3, 2, 8)
    with pytest.raises(cabi.CsnError):
        cabi.chan_l2_dist(x, x, 0, 8)
    d = torch.zeros(1, 3, 3, dtype=torch.float64)
    with pytest.raises(cabi.CsnError):
        cabi.chan_l2_select(None, d, torch.zeros(3, dtype=torch.int32), torch.zeros(3, dtype=torch.int32), 1)
    with pytest.raises(cabi.CsnError):
        cabi.chan_l2_accumulate(d, d, True)


# ---- 3. the decomposition against the flat feature ------------------------------------------------------------------------
ORDERS = ([1], [1, 4], [4, 1], [0, 2, 5], [5, 0, 2, 3], [3, 2, 1, 0, 4, 5])
T0, T1 = 2, 11


def _decomposed(g, q, order):
    """The driver's arithmetic: per-channel matrices, summed ((D_s1 + D_s2) + ...) in selection order."""
    Dc = ref.chan_l2_dist(g, q, T0, T1)
    base = None
    for i, ch in enumerate(order):
        base = ref.chan_l2_accumulate(base, Dc[ch], i == 0)
    return base


@pytest.mark.parametrize("order", ORDERS, ids=lambda o: "-".join(map(str, o)))
def test_decomposition_equals_the_flat_feature_on_integer_data(order):
    """Values in [-8, 8]: every partial sum is an integer below 2**53, so every summation order gives the same bits, and
    the decomposed distances AND neighbours equal the naive flat-feature oracle's, ties included."""
    rng = np.random.default_rng(17 + len(order))
    g = rng.integers(-8, 9, (40, 6, 12)).astype(np.float32)
    q = rng.integers(-8, 9, (23, 6, 12)).astype(np.float32)
    g[7], g[30] = g[3], g[3]                     # exact duplicates: ties at every k
    q[5] = g[3]
    k = 9
    D = _decomposed(g, q, order)
    want_d, want_i = oracle_retrieval.l2_topk(ref.flat_features(g, T0, T1, order), ref.flat_features(q, T0, T1, order), k)
    got_d, got_i = ref.exact_topk(D, k)
    np.testing.assert_array_equal(got_i, want_i)
    np.testing.assert_array_equal(got_d, want_d)
    assert list(got_i[5, :3]) == [3, 7, 30] and (got_d[5, :3] == 0).all(), "the planted tie"
    sel = ref.chan_l2_select(_decomposed(g, q, order[:-1]) if len(order) > 1 else None,
                             ref.chan_l2_dist(g, q, T0, T1, [order[-1]]), np.zeros(40, np.int32), np.zeros(23, np.int32), k)
    np.testing.assert_array_equal(sel["idx"][0], want_i)
    np.testing.assert_array_equal(sel["dist"][0], want_d)


@pytest.mark.parametrize("order", ORDERS, ids=lambda o: "-".join(map(str, o)))
def test_decomposition_is_within_the_reordering_bound_on_normal_data(order):
    """Standard-normal data: the two forms sum the same Tw * (m+1) squares in different orders; each is within
    n * 2**-53 relative of the other (the bound d2_kernel_order's docstring states).  Distances only."""
    rng = np.random.default_rng(29)
    g = rng.standard_normal((40, 6, 12)).astype(np.float32)
    q = rng.standard_normal((23, 6, 12)).astype(np.float32)
    D = _decomposed(g, q, order)
    fd, fi = oracle_retrieval.l2_topk(ref.flat_features(g, T0, T1, order), ref.flat_features(q, T0, T1, order), 40)
    flat = np.empty_like(D)
    np.put_along_axis(flat, fi, fd, axis=1)
    n = (T1 - T0) * len(order)
    rel = np.abs(D - flat) / flat
    print(f"order {order}: max relative difference {rel.max():.3e}, bound {n * 2.0 ** -53:.3e}")
    assert rel.max() <= n * 2.0 ** -53


# ---- 4. the greedy driver -------------------------------------------------------------------------------------------------
def _both(problem, engine=ref.NUMPY_ENGINE, **kw):
    from cerebralsignalnetworks_amd.channel_discovery import discover_channels
    g, q, gl, ql, ds = problem
    kw.setdefault("topK", ref.PLANTED_TOPK)
    kw.setdefault("time_low", T0)
    kw.setdefault("time_high", T1)
    got = discover_channels(g, q, gl, ql, ds, engine=engine, **kw)
    kw.pop("budget_bytes", None)
    want = ref.naive_discover(g, q, gl, ql, ds.class_id_to_str, **kw)
    return ref.as_tuple(got), ref.as_tuple(want)


def test_driver_equals_the_naive_loop_on_the_planted_problem():
    got, want = _both(ref.planted())
    assert got == want                           # order, every round's (recall, precision) floats, stop reason, top-1
    order, rounds, stopped, _ = got
    print(order, stopped, rounds)
    assert set(order[:2]) == {1, 4}, "the two informative channels come first"
    assert stopped == "found no channel better than last iteration"
    assert len(rounds) == len(order) + 1, "the last round accepts nothing"
    assert all(list(r) == sorted(r) and not set(r) & set(order[:i]) for i, r in enumerate(rounds))


@pytest.mark.parametrize("kw", [dict(), dict(start=(3,)), dict(max_channels=1)], ids=str)
def test_best_is_the_leading_entry_of_all_rounds_so_far(kw):
    from cerebralsignalnetworks_amd.channel_discovery import discover_channels
    g, q, gl, ql, ds = ref.planted()
    res = discover_channels(g, q, gl, ql, ds, topK=ref.PLANTED_TOPK, time_low=T0, time_high=T1, engine=ref.NUMPY_ENGINE, **kw)
    assert len(res.best) == len(res.rounds)
    seen, lead = [], None
    for i, metrics in enumerate(res.rounds):
        fixed = tuple(res.order[:len(kw.get("start", ())) + i])
        seen += [(fixed + (ch,), m) for ch, m in metrics.items()]
        lead = None
        for subset, m in seen:                   # first strict maximum of the recall, above 0, in insertion order
            if m[0] > (lead[1][0] if lead else 0):
                lead = (subset, m)
        assert res.best[i] == lead
    if res.stopped == "found no channel better than last iteration":
        assert res.best[-1][0] == tuple(res.order), "the last round's leader is the accepted subset"


def test_all_zero_recalls_have_no_best():
    from cerebralsignalnetworks_amd.channel_discovery import discover_channels
    g, q, gl, ql, _ = ref.planted()
    ql = [ref.label(l["ClassId"] + 4) for l in ql]
    res = discover_channels(g, q, gl, ql, ref.DS(8), topK=2, time_low=T0, time_high=T1, engine=ref.NUMPY_ENGINE)
    assert res.best == [None]


def test_cli_takes_the_first_rows_of_every_class():
    import DiscoverChannels
    class_ids = [2, 0, 2, 1, 0, 2, 2, 1, 0]
    assert DiscoverChannels.first_per_class(class_ids, [8, 6, 5, 3, 2, 1, 0], 2) == [8, 1, 3, 6, 5]
    assert DiscoverChannels.first_per_class(class_ids, [4, 7], 30) == [4, 7]
    assert DiscoverChannels.first_per_class(class_ids, [], 3) == []


def test_of_two_identical_channels_the_lower_wins():
    g, q, gl, ql, ds = ref.planted()
    g[:, 0], q[:, 0] = g[:, 1], q[:, 1]          # channel 0 = channel 1, bit for bit
    got, want = _both((g, q, gl, ql, ds))
    assert got == want
    assert got[1][0][0] == got[1][0][1], "equal metrics in round 0"
    twins = [c for c in got[0] if c in (0, 1)]
    assert twins and twins[0] == 0, got[0]


def test_all_recalls_zero_stops_in_round_one():
    g, q, gl, ql, _ = ref.planted()
    ql = [ref.label(l["ClassId"] + 4) for l in ql]       # no query class occurs in the gallery
    for start in ((), (2,)):
        got, want = _both((g, q, gl, ql, ref.DS(8)), start=start)
        assert got == want
        assert got[0] == list(start) and len(got[1]) == 1 and got[2] == "found no channel better than last iteration"
        assert all(v == (0.0, 0.0) for v in got[1][0].values())


@pytest.mark.parametrize("kw", [dict(start=(3,)), dict(start=(5, 0)), dict(max_channels=1), dict(start=(2,), max_channels=2),
                                dict(start=(2,), max_channels=1), dict(topK=1), dict(topK=5), dict(topK=24),
                                dict(time_low=0, time_high=12)], ids=str)
def test_driver_options_equal_the_naive_loop(kw):
    got, want = _both(ref.planted(seed=5), **kw)
    assert got == want
    assert got[0][:len(kw.get("start", ()))] == list(kw.get("start", ()))
    if "max_channels" in kw:
        assert len(got[0]) <= max(kw["max_channels"], len(kw.get("start", ())))


def test_no_candidate_left():
    got, want = _both(ref.planted(), start=(0, 1, 2, 3, 4, 5))
    assert got == want and got[1] == [] and got[2] == "no candidate left"


def test_results_do_not_depend_on_the_block_size():
    problem = ref.planted(seed=7)
    per_channel = 24 * 24 * 8
    results, shapes = [], []
    for budget in (per_channel, 2 * per_channel, 2 * per_channel + 100, 6 * per_channel, 4 << 30):
        calls = []
        got, want = _both(problem, engine=ref.counting_engine(calls), budget_bytes=budget)
        assert got == want
        results.append(got)
        shapes.append(max(6 if c is None else len(c) for c in calls))
    assert all(r == results[0] for r in results)
    assert shapes == [1, 2, 2, 6, 6], "blocks of 1, 2 and all channels were used"


# ---- 5. class-map errors --------------------------------------------------------------------------------------------------
def test_class_map_errors():
    from cerebralsignalnetworks_amd.channel_discovery import discover_channels
    g, q, gl, ql, ds = ref.planted()
    run = lambda gl, ql, ds: discover_channels(g, q, gl, ql, ds, topK=2, time_low=T0, time_high=T1, engine=ref.NUMPY_ENGINE)
    twice = ref.DS(4)
    twice.class_id_to_str[3] = "class_2"                     # not injective
    with pytest.raises(ValueError, match="injective"):
        run(gl, ql, twice)
    wrong = [dict(l) for l in ql]
    wrong[4]["ClassName"] = "class_3"                        # ClassId 0 is class_0 in the map
    with pytest.raises(ValueError, match="ClassName"):
        run(gl, wrong, ds)
    with pytest.raises(ValueError, match="ClassName"):
        run(wrong[:len(gl)], ql, ds)
    with pytest.raises(ValueError, match="not in class_id_to_str"):
        run(gl, [ref.label(9)] * len(ql), ds)


def test_argument_errors():
    from cerebralsignalnetworks_amd.channel_discovery import discover_channels
    g, q, gl, ql, ds = ref.planted()
    for kw in (dict(time_low=5, time_high=5), dict(time_high=13), dict(topK=0), dict(topK=25), dict(start=(6,)),
               dict(start=(1, 1)), dict(layout="tcn")):
        kw = {"time_low": T0, "time_high": T1, **kw}
        with pytest.raises(ValueError):
            discover_channels(g, q, gl, ql, ds, engine=ref.NUMPY_ENGINE, **kw)
    ntc = discover_channels(np.transpose(g, (0, 2, 1)), np.transpose(q, (0, 2, 1)), gl, ql, ds, time_low=T0, time_high=T1,
                            engine=ref.NUMPY_ENGINE, layout="ntc")
    assert ref.as_tuple(ntc) == ref.as_tuple(discover_channels(g, q, gl, ql, ds, time_low=T0, time_high=T1,
                                                               engine=ref.NUMPY_ENGINE))
