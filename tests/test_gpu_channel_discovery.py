"""GPU: channel discovery (csrc/channel_l2.hip, channel_discovery.py) -- the three kernels against
their numpy contracts and against the product's own tiled search, with canaries around every output, and
``discover_channels`` with the HIP engine against the numpy engine and against a brute-force loop over
``retrieval.l2_search``."""
import numpy as np
import pytest
import torch

import channel_discovery_reference as ref
import channel_discovery_stream_cases as stream_cases
import test_gpu_stream_order as stream_tests
from cerebralsignalnetworks_amd import cabi, retrieval
from cerebralsignalnetworks_amd.channel_discovery import channel_distances, discover_channels

pytestmark = pytest.mark.gpu

PAD = 96                                   # canary elements before and behind every output
CANARY = {torch.float64: -7.25e300, torch.int64: 0x5A5A5A5A5A5A5A5A, torch.int32: 0x5A5A5A5A}


class Guarded:
    """A dense output inside a larger buffer filled with a canary pattern."""

    def __init__(self, n, dtype, dev):
        self.n = n
        self.buf = torch.full((n + 2 * PAD,), CANARY[dtype], dtype=dtype, device=dev)
        self.view = self.buf[PAD:PAD + n]

    def intact(self):
        c = torch.full((PAD,), CANARY[self.buf.dtype], dtype=self.buf.dtype, device=self.buf.device)
        return bool(torch.equal(self.buf[:PAD], c) and torch.equal(self.buf[PAD + self.n:], c))

    def untouched(self):
        return bool((self.buf == CANARY[self.buf.dtype]).all())


def bits(a):
    return np.ascontiguousarray(a).view(np.int64)


# ---- 1. csn_chan_l2_dist ------------------------------------------------------------------------------------------------
DIST_CASES = [(130, 67, 5, 45, 3, 40, [4, 0, 2]),      # odd row stride, misaligned window, partial tiles both ways, 37 samples
              (64, 64, 3, 32, 0, 32, None),
              (1, 1, 1, 1, 0, 1, None),
              (70, 200, 4, 513, 1, 513, [1, 3])]        # sixteen 32-slices


def _dist_inputs(Ng, Nq, C, T, integer, seed=0):
    rng = np.random.default_rng(1000 * Ng + T + seed)
    draw = (lambda n: rng.integers(-8, 9, (n, C, T))) if integer else (lambda n: rng.standard_normal((n, C, T)))
    return draw(Ng).astype(np.float32), draw(Nq).astype(np.float32)


def _check_dist(cuda, g_np, q_np, g_dev, q_dev, t0, t1, channels, integer):
    Ng, C, _ = g_np.shape
    Nq = q_np.shape[0]
    chans = list(range(C)) if channels is None else channels
    out = Guarded(len(chans) * Nq * Ng, torch.float64, cuda)
    Dc = cabi.chan_l2_dist(g_dev, q_dev, t0, t1, channels, out=out.view)
    torch.cuda.synchronize()
    assert out.intact(), "canary around Dc"
    got = Dc.cpu().numpy()
    assert got.shape == (len(chans), Nq, Ng)
    want = ref.chan_l2_dist(g_np, q_np, t0, t1, chans)
    if integer:
        np.testing.assert_array_equal(bits(got), bits(want))
    else:       # the contract's chain is fused, numpy's is not: each within Tw * 2**-53 relative of the exact sum
        assert (np.abs(got - want) <= 2 * (t1 - t0) * 2.0 ** -53 * want).all()
    for j, c in enumerate(chans):      # the product's own chain on the gathered [N, Tw] rows
        X = torch.from_numpy(np.ascontiguousarray(g_np[:, c, t0:t1])).to(cuda)
        Y = torch.from_numpy(np.ascontiguousarray(q_np[:, c, t0:t1])).to(cuda)
        _, idx, d64 = cabi.l2_topk_tiled(X, Y, Ng, dist64=True)
        full = torch.empty((Nq, Ng), dtype=torch.float64, device=cuda).scatter_(1, idx, d64)
        np.testing.assert_array_equal(bits(got[j]), bits(full.cpu().numpy()), err_msg=f"channel {c} against l2_topk_tiled")
    return got


@pytest.mark.parametrize("integer", [True, False], ids=["integer", "normal"])
@pytest.mark.parametrize("Ng,Nq,C,T,t0,t1,channels", DIST_CASES, ids=lambda v: str(v).replace(" ", ""))
def test_dist_equals_contract_and_tiled_search(cuda, Ng, Nq, C, T, t0, t1, channels, integer):
    g, q = _dist_inputs(Ng, Nq, C, T, integer)
    _check_dist(cuda, g, q, torch.from_numpy(g).to(cuda), torch.from_numpy(q).to(cuda), t0, t1, channels, integer)


@pytest.mark.parametrize("integer", [True, False], ids=["integer", "normal"])
def test_dist_reads_views_of_a_larger_tensor_in_place(cuda, integer):
    """The first case on slices whose ld_n and ld_c exceed the dense strides; everything around them is NaN, so one
    element read from outside the view poisons a distance."""
    Ng, Nq, C, T, t0, t1, channels = DIST_CASES[0]
    g, q = _dist_inputs(Ng, Nq, C, T, integer)
    views = []
    for x in (g, q):
        big = torch.full((x.shape[0] + 2, C + 2, T + 5), float("nan"), device=cuda)
        v = big[1:-1, 1:C + 1, 3:3 + T]
        v.copy_(torch.from_numpy(x))
        assert not v.is_contiguous() and v.stride() == ((C + 2) * (T + 5), T + 5, 1)
        assert cabi._nct_view(v, "x").data_ptr() == v.data_ptr(), "the binding passes the view, not a copy"
        views.append(v)
    got = _check_dist(cuda, g, q, views[0], views[1], t0, t1, channels, integer)
    assert np.isfinite(got).all()
    dense = cabi.chan_l2_dist(torch.from_numpy(g).to(cuda), torch.from_numpy(q).to(cuda), t0, t1, channels).cpu().numpy()
    np.testing.assert_array_equal(bits(got), bits(dense))


def test_dist_refuses_an_out_buffer_that_is_not_on_the_device(cuda):
    g, q = (torch.from_numpy(x).to(cuda) for x in _dist_inputs(6, 3, 2, 8, True))
    with pytest.raises(cabi.CsnError, match="out must be"):
        cabi.chan_l2_dist(g, q, 0, 8, out=torch.empty(2 * 3 * 6, dtype=torch.float64))
    with pytest.raises(cabi.CsnError, match="out must be"):
        cabi.chan_l2_dist(g, q, 0, 8, out=torch.empty(2 * 3 * 6, dtype=torch.float32, device=cuda))


def test_channel_distances_layouts_agree(cuda):
    g, q = _dist_inputs(70, 33, 4, 21, False)
    a = channel_distances(g, q, 2, 19, channels=[3, 1])
    b = channel_distances(np.transpose(g, (0, 2, 1)), np.transpose(q, (0, 2, 1)), 2, 19, channels=[3, 1], layout="ntc")
    assert a.is_cuda and a.dtype == torch.float64 and tuple(a.shape) == (2, 33, 70)
    assert torch.equal(a, b)


# ---- 2. csn_chan_l2_select ----------------------------------------------------------------------------------------------
NQ = 9


def _select_raw(cuda, base, Dc, gc, qc, k, skip=()):
    """The C entry point with every output (but those in ``skip``) inside a canary buffer."""
    nc, Nq, _ = Dc.shape
    outs = {"idx": Guarded(nc * Nq * k, torch.int64, cuda), "dist": Guarded(nc * Nq * k, torch.float64, cuda),
            "hits": Guarded(nc * Nq, torch.int32, cuda), "top1": Guarded(nc * Nq, torch.int32, cuda)}
    p = lambda name: None if name in skip else cabi._ptr(outs[name].view)
    cabi._check(cabi.load().csn_chan_l2_select(cabi._ptr(base), cabi._ptr(Dc), nc, Nq, Dc.shape[2], cabi._ptr(gc),
                                               cabi._ptr(qc), k, p("idx"), p("dist"), p("hits"), p("top1"), cabi._stream()))
    torch.cuda.synchronize()
    res = {}
    for name, o in outs.items():
        if name in skip:
            assert o.untouched(), f"{name} was not given"
        else:
            assert o.intact(), f"canary around {name}"
            res[name] = o.view.cpu().numpy().reshape((nc, Nq, k) if name in ("idx", "dist") else (nc, Nq))
    return res


def _check_select(cuda, base, Dc, k, seed, skip=()):
    """Expected values from the GPU's own matrices: base + Dc[j] is one IEEE add, so everything is bit-equal."""
    nc, Nq, Ng = Dc.shape
    rng = np.random.default_rng(seed)
    gc, qc = rng.integers(0, 3, Ng).astype(np.int32), rng.integers(0, 3, Nq).astype(np.int32)
    got = _select_raw(cuda, base, Dc, torch.from_numpy(gc).to(cuda), torch.from_numpy(qc).to(cuda), k, skip)
    want = ref.chan_l2_select(None if base is None else base.cpu().numpy(), Dc.cpu().numpy(), gc, qc, k)
    for name in got:
        a, b = got[name], want[name]
        np.testing.assert_array_equal(bits(a) if name == "dist" else a, bits(b) if name == "dist" else b, err_msg=name)
    return got


def _tie_heavy(cuda, shape, seed):
    return torch.from_numpy(np.random.default_rng(seed).integers(0, 5, shape).astype(np.float64)).to(cuda)


@pytest.mark.parametrize("with_base", [False, True], ids=["nobase", "base"])
@pytest.mark.parametrize("nc", [1, 7])
@pytest.mark.parametrize("Ng", [5, 64, 257, 1031, 2048, 2049, 2500])       # 2048: the longest row staged in LDS
def test_select_on_tie_heavy_matrices(cuda, Ng, nc, with_base):
    Dc = _tie_heavy(cuda, (nc, NQ, Ng), Ng + nc)
    base = _tie_heavy(cuda, (NQ, Ng), Ng + 50) if with_base else None
    for k in sorted({1, 5, min(64, Ng)}):
        got = _check_select(cuda, base, Dc, k, seed=Ng + k)
        assert (np.diff(got["dist"], axis=-1) >= 0).all()
        if k > 1:
            assert (np.diff(got["dist"], axis=-1) == 0).any(), "not tie-heavy"


@pytest.mark.parametrize("with_base", [False, True], ids=["nobase", "base"])
@pytest.mark.parametrize("nc", [1, 7])
@pytest.mark.parametrize("Ng", [5, 64, 257, 1031])
def test_select_on_matrices_from_the_distance_kernel(cuda, Ng, nc, with_base):
    for integer in (True, False):
        g, q = _dist_inputs(Ng, NQ, nc + 1, 20, integer, seed=7)
        D_all = cabi.chan_l2_dist(torch.from_numpy(g).to(cuda), torch.from_numpy(q).to(cuda), 1, 18)
        Dc, base = D_all[:nc].contiguous(), (D_all[nc].contiguous() if with_base else None)
        for k in sorted({1, 5, min(64, Ng)}):
            _check_select(cuda, base, Dc, k, seed=Ng + k)


@pytest.mark.parametrize("skip", [("idx",), ("dist",), ("hits",), ("top1",), ("idx", "dist"), ("hits", "top1"),
                                  ("idx", "dist", "hits"), ("dist", "hits", "top1")], ids="-".join)
def test_select_leaves_null_outputs_alone(cuda, skip):
    Dc, base = _tie_heavy(cuda, (3, NQ, 300), 1), _tie_heavy(cuda, (NQ, 300), 2)
    _check_select(cuda, base, Dc, 5, seed=3, skip=skip)


def test_select_binding_returns_what_was_asked_for(cuda):
    Dc = _tie_heavy(cuda, (2, NQ, 40), 5)
    gc, qc = torch.zeros(40, dtype=torch.int32, device=cuda), torch.zeros(NQ, dtype=torch.int32, device=cuda)
    out = cabi.chan_l2_select(None, Dc, gc, qc, 4)
    assert set(out) == {"idx", "dist", "hits", "top1"} and (out["hits"] == 4).all() and (out["top1"] == 0).all()
    want_d, want_i = ref.exact_topk(Dc[1].cpu().numpy(), 4)
    np.testing.assert_array_equal(out["idx"][1].cpu().numpy(), want_i)
    np.testing.assert_array_equal(out["dist"][1].cpu().numpy(), want_d)
    assert set(cabi.chan_l2_select(None, Dc, None, None, 4, want=("idx",))) == {"idx"}


# ---- 3. csn_chan_l2_accumulate ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 1000, 4096 * 256 + 77], ids=str)       # the last: more elements than threads launched
def test_accumulate_copies_then_adds(cuda, n):
    rng = np.random.default_rng(n)
    a, b = rng.standard_normal(n) * 1e3, rng.standard_normal(n)
    base = Guarded(n, torch.float64, cuda)
    A, B = torch.from_numpy(a).to(cuda), torch.from_numpy(b).to(cuda)
    cabi.chan_l2_accumulate(base.view, A, True)
    torch.cuda.synchronize()
    assert base.intact()
    np.testing.assert_array_equal(bits(base.view.cpu().numpy()), bits(a))
    cabi.chan_l2_accumulate(base.view, B, False)
    torch.cuda.synchronize()
    assert base.intact(), "nothing is written beyond n"
    np.testing.assert_array_equal(bits(base.view.cpu().numpy()), bits(a + b))
    np.testing.assert_array_equal(bits(B.cpu().numpy()), bits(b))


# ---- 4. the stream contract of the three entry points -----------------------------------------------------------------------
@pytest.mark.parametrize("case", [c for v in stream_cases.CASES.values() for c in v], ids=lambda c: c.id)
def test_entry_point_with_late_inputs(cuda, case):
    """The procedure of tests/test_gpu_stream_order.py on the cases of tests/channel_discovery_stream_cases.py."""
    stream_tests.test_stateless_entry_point_with_late_inputs(cuda, case)


# ---- 5. discover_channels, end to end -------------------------------------------------------------------------------------
def _problems():
    five = dict(C=5, ncls=3, T=45, n_gallery=130, n_query=67)
    return {"planted3": (ref.planted(seed=3), ref.PLANTED_TOPK, 2, 11, True),
            "planted5": (ref.planted(seed=5), ref.PLANTED_TOPK, 2, 11, True),
            "five-integer": (ref.planted(seed=11, **five), 5, 3, 40, True),
            "five-normal": (ref.planted(seed=12, integer=False, **five), 5, 3, 40, False)}


@pytest.fixture(scope="module")
def numpy_runs():
    """The numpy-engine result of every problem, computed once."""
    out = {}
    for name, (p, topK, t0, t1, _) in _problems().items():
        out[name] = ref.as_tuple(discover_channels(*p, topK=topK, time_low=t0, time_high=t1, engine=ref.NUMPY_ENGINE))
    return out


@pytest.mark.parametrize("name", ["planted3", "planted5", "five-integer", "five-normal"])
def test_discovery_hip_engine_equals_numpy_engine(cuda, numpy_runs, name):
    p, topK, t0, t1, integer = _problems()[name]
    g, q, gl, ql, ds = p
    want = numpy_runs[name]
    per_channel = g.shape[0] * q.shape[0] * 8
    for budget in (4 << 30, 2 * per_channel, per_channel):         # all channels resident, blocks of 2, blocks of 1
        got = ref.as_tuple(discover_channels(g, q, gl, ql, ds, topK=topK, time_low=t0, time_high=t1, budget_bytes=budget))
        assert got == want, (name, budget)                          # order, every float, stop reason, top-1
    assert len(want[1]) >= 2, "more than one round"
    side = torch.cuda.Stream()                                      # the stream contract: everything on the current stream
    with torch.cuda.stream(side):
        g_d = torch.from_numpy(g).to(cuda, non_blocking=True) * 1.0      # produced on the side stream
        q_d = torch.from_numpy(q).to(cuda, non_blocking=True) * 1.0
        got = ref.as_tuple(discover_channels(g_d, q_d, gl, ql, ds, topK=topK, time_low=t0, time_high=t1))
    side.synchronize()
    assert got == want, (name, "side stream")
    if integer:     # the parent commit's way: one search per candidate on the gathered flat feature, the product's bookkeeping
        brute = ref.naive_discover(
            g, q, gl, ql, ds.class_id_to_str, topK=topK, time_low=t0, time_high=t1,
            search=lambda gf, qf, k: retrieval.l2_search(gf, qf, k),
            fold=lambda I, a, b, k: retrieval._bookkeeping(I, a, b, ds.class_id_to_str, ds.class_str_to_id, k))
        assert ref.as_tuple(brute) == want, (name, "brute force over retrieval.l2_search")


# ---- 6. the command-line tool ---------------------------------------------------------------------------------------------
def test_cli_prints_what_discover_channels_returns(cuda, capsys):
    """DiscoverChannels.py on a small synthetic set: the dataset wiring, the per-candidate and per-round lines and the
    final line against the result it returns, and that result against a direct call on the same rows."""
    import DiscoverChannels
    from cerebralsignalnetworks_amd.dataset import EEGDataset
    from cerebralsignalnetworks_amd.trainer import split_indices
    argv = ["--synthetic", "400", "--synthetic_channels", "6", "--synthetic_samples", "64", "--time_low", "4",
            "--time_high", "60", "--samples_per_class", "5", "--topK", "3", "--fixed_channels", "2"]
    res = DiscoverChannels.main(argv)
    lines = capsys.readouterr().out.splitlines()
    assert res.order[0] == 2 and len(res.rounds) >= 1
    cand = [l for l in lines if l.startswith("TS ")]
    want = [f"TS {res.order[:1 + i]}[{ch}] Overall Recall :{r} Overall Precision: {p}"
            for i, metrics in enumerate(res.rounds) for ch, (r, p) in metrics.items()]
    assert cand == want
    best = [l for l in lines if l.startswith("best score channel: ")]
    assert best == [f"best score channel: {''.join(f',{c}' for c in b[0])}  with Scores: "
                    f"{{'Recall': {b[1][0]}, 'Precision': {b[1][1]}}}" for b in res.best if b]
    assert lines[-1].endswith(f"final channels: {res.order}")
    assert lines[-1].startswith("found no channel better" if res.stopped.startswith("found no channel") else "stopped: ")
    # the same rows, chosen here
    ds = EEGDataset(synthetic=400, synthetic_channels=6, synthetic_samples=64, time_low=0, time_high=64, seed=43, device=cuda)
    train, test = split_indices(400, (0.8, 0.2), seed=123)
    labels = ds.labels.tolist()
    rows = [[i for c in sorted(set(labels)) for i in [j for j in part.tolist() if labels[j] == c][:5]] for part in (train, test)]
    direct = discover_channels(ds.eeg_all[rows[0]], ds.eeg_all[rows[1]], [ds.getLabelbyIndex(i) for i in rows[0]],
                               [ds.getLabelbyIndex(i) for i in rows[1]], ds, topK=3, time_low=4, time_high=60, start=(2,))
    assert tuple(direct) == tuple(res)
