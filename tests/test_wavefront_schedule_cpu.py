"""CPU: the layer wavefront of the per-diagonal and CU-resident LSTM paths.

The schedule under test is the one the library runs: csn::wavefront_schedule (csrc/lstm_schedule.h), which forward_v1 /
backward_v1, forward_resident / backward_resident and forward_il / backward_il (csrc/lstm.hip) enqueue launch by launch,
printed by the host-only program of tests/lstm_schedule_probe.py.  tests/wavefront_model.py is the six loops those
functions wrote out by hand before; the two must agree field by field over the sweep, and the C++ output must hold the
invariants of a wavefront on its own: every (layer, step) in exactly one cell, at most four cells and one per layer in a
launch, chunk follow-ups only behind the launch that closes a diagonal, a layer's cells in time order and behind the
follow-up that feeds them, and the closed-form launch count."""
import itertools

import pytest

import lstm_schedule_probe as sp
import wavefront_model as wm

TS = (1, 2, 3, 4, 5, 7, 8, 9, 11, 33)
LS = tuple(range(1, 9))
CHUNKS = (1, 2, 3, 4, 32)
SWEEP = [(v, T, L, chunk) for v in wm.VARIANTS for T, L, chunk in itertools.product(TS, LS, CHUNKS)]


@pytest.fixture(scope="module")
def swept(tmp_path_factory):
    """[(variant, T, L, chunk, the library's schedule)] over SWEEP: one process."""
    ask = sp.build(tmp_path_factory.mktemp("wave_schedule"))
    raw = ask([sp.wave_query(*p) for p in SWEEP])
    return [(*p, q) for p, q in zip(SWEEP, raw)]


def _geometry(variant, T, L, chunk):
    """(units, lag in units) of a variant's diagonals"""
    by_chunk, lag, _ = sp.WAVE_VARIANTS[variant]
    return (-(-T // chunk), lag) if by_chunk else (T, lag * chunk)


def _on_diagonal(variant, T, L, chunk, dg):
    units, lag = _geometry(variant, T, L, chunk)
    return sum(1 for i in range(L) if 0 <= dg - lag * i < units)


def _diagonals(variant, T, L, chunk):
    units, lag = _geometry(variant, T, L, chunk)
    return range(units + lag * (L - 1))


def _follows(variant, L, done):
    """the chunk follow-ups a host function issues for a closing launch's `done` list (csrc/lstm.hip)"""
    if variant.startswith("forward"):
        return [tuple(d) for d in done if d[0] + 1 < L]
    if variant == "backward_il":
        return [tuple(d) for d in done]
    return [tuple(d) for d in done if d[0] > 0]


def _steps(variant, cell):
    _, _, t, nsteps, *_ = cell
    return range(t, t + nsteps) if variant.startswith("forward") else range(t, t - nsteps, -1)


def test_sweep_size_and_corners(swept):
    assert len(swept) == 2400 == len(set(SWEEP))
    assert any(T == 1 for _, T, _, _, _ in swept) and any(chunk == 1 for _, _, _, chunk, _ in swept)
    for variant in wm.VARIANTS:
        mine = [(T, L, chunk, q) for v, T, L, chunk, q in swept if v == variant]
        # a split diagonal: more than four layers in range, the first launch of the two does not close it
        assert any(not launch["closes"] for _, L, _, q in mine for launch in q if L >= 5), variant
        # a short last chunk behind a full one (its cells' fields: test_cell_fields)
        assert any(T > chunk and T % chunk and any(c[1] == T // chunk for launch in q for c in launch["cells"])
                   for T, L, chunk, q in mine), variant
        # an empty diagonal: the layers further apart than the sequence is long (step units only: chunk diagonals lag one unit)
        empty = any(_on_diagonal(variant, T, L, chunk, dg) == 0 for T, L, chunk, _ in mine for dg in _diagonals(variant, T, L, chunk))
        assert empty == (not sp.WAVE_VARIANTS[variant][0]), variant
    # the split diagonal of the chunk unit needs five chunks
    assert any(not launch["closes"] for v, T, L, chunk, q in swept if v.endswith("resident") and -(-T // chunk) >= 5 for launch in q)


def test_library_schedule_is_the_hand_written_loops(swept):
    for variant, T, L, chunk, q in swept:
        model = wm.run(variant, T, L, chunk)
        key = (variant, T, L, chunk)
        assert len(q) == len(model), key
        fwd = variant.startswith("forward")
        for launch, ref in zip(q, model):
            assert [tuple(c[:4]) for c in launch["cells"]] == ref["cells"], key
            assert _follows(variant, L, launch["done"]) == ref["follow"], key
            if variant.endswith("_il"):         # the events waited for in front of the launch
                waits = [(c[0], c[1]) if fwd else (c[0] + 1, c[1]) for c in launch["cells"] if c[4] and (c[0] > 0 if fwd else c[0] < L - 1)]
                assert waits == ref["waits"], key
        n_launch, n_cells = wm.counts(variant, T, L, chunk)
        if variant.endswith("_il"):
            assert (n_launch, n_cells) == (len(q), sum(len(launch["cells"]) for launch in q)) and n_cells == T * L, key


def test_cell_fields(swept):
    """enters / ends / last by their definitions, and done = the cells of the diagonal that ended a chunk"""
    for variant, T, L, chunk, q in swept:
        key = (variant, T, L, chunk)
        by_chunk = sp.WAVE_VARIANTS[variant][0]
        fwd = variant.startswith("forward")
        nch = -(-T // chunk)
        diagonal = []
        for launch in q:
            for layer, c, t, nsteps, enters, ends, last in launch["cells"]:
                if by_chunk:
                    t0 = t if fwd else T - 1 - t
                    assert t0 == c * chunk and nsteps == min(chunk, T - t0), key
                    assert (enters, ends, last) == (1, 1, int(c == nch - 1)), key
                else:
                    u = t if fwd else T - 1 - t
                    assert nsteps == 1 and c == u // chunk, key
                    assert (enters, ends, last) == (int(u % chunk == 0), int(wm.ends_chunk(T, chunk, u)), int(u == T - 1)), key
            diagonal += launch["cells"]
            if launch["closes"]:
                assert launch["done"] == [[c[0], c[1], c[6]] for c in diagonal if c[5]], key
                diagonal = []
        assert not diagonal, key        # the last launch closes


def test_every_step_once_and_launch_shape(swept):
    for variant, T, L, chunk, q in swept:
        key = (variant, T, L, chunk)
        seen = []
        for launch in q:
            layers = [c[0] for c in launch["cells"]]
            assert 1 <= len(layers) <= 4 and len(set(layers)) == len(layers), key
            if not launch["closes"]:
                assert launch["done"] == [] and len(layers) == 4, key
            seen += [(c[0], t) for c in launch["cells"] for t in _steps(variant, c)]
        assert len(seen) == T * L and set(seen) == set(itertools.product(range(L), range(T))), key


def test_order(swept):
    """A layer's cells come in time order, and the cells of (layer, chunk) strictly behind the follow-up that feeds
    them: that of (layer - 1, chunk) in the forward, of (layer + 1, chunk) in the backward."""
    for variant, T, L, chunk, q in swept:
        key = (variant, T, L, chunk)
        fwd = variant.startswith("forward")
        followed = {}        # (layer, chunk) -> index of the launch whose follow-ups hold it
        for n, launch in enumerate(q):
            for layer, c, _ in _follows(variant, L, launch["done"]):
                assert (layer, c) not in followed, key
                followed[(layer, c)] = n
        at = {l: [] for l in range(L)}
        for n, launch in enumerate(q):
            for cell in launch["cells"]:
                layer, c = cell[0], cell[1]
                at[layer] += list(_steps(variant, cell))
                feeder = (layer - 1, c) if fwd else (layer + 1, c)
                if 0 <= feeder[0] < L:
                    assert followed[feeder] < n, key
        for l in range(L):
            assert at[l] == (list(range(T)) if fwd else list(range(T - 1, -1, -1))), key


def test_launch_count_closed_form(swept):
    for variant, T, L, chunk, q in swept:
        key = (variant, T, L, chunk)
        units, lag = _geometry(variant, T, L, chunk)
        on = [_on_diagonal(variant, T, L, chunk, dg) for dg in _diagonals(variant, T, L, chunk)]
        assert len(q) == sum(1 for n in on if n > 0) + sum(1 for n in on if n > 4), key
        assert sum(1 for launch in q if launch["closes"]) == sum(1 for n in on if n > 0), key
        if units >= lag or L == 1:      # no empty diagonal
            assert all(n > 0 for n in on) and len(on) == units + lag * (L - 1), key
            if L <= 4:
                assert len(q) == units + lag * (L - 1), key
        if sp.WAVE_VARIANTS[variant][0] and L <= 4:
            assert len(q) == -(-T // chunk) + L - 1, key
