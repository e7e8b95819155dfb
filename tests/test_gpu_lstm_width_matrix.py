"""GPU: every LSTM kernel instantiation with state, lengths and plan features (tests/lstm_width_matrix.py).

One test per (regime, feature set) of lstm_width_matrix.REGIMES, on the runner of tests/test_gpu_lstm_feature_fuzz.py: the
plan triple of the featured, baseline and plain plans is the regime's; the 32-row launch counts and dgates_copies are
what the mirror of the launch schedule derives; the featured results are the baseline's bits after undoing the layout
(_bit_identities, unchanged); NaN / Inf in the padding changes nothing; no status word is raised; both results lie
within st._bounds of the float64 reference and, bf16, within oracle.compare.BF16_EMU_BOUNDS of the bf16-faithful
emulator, whose failure message names the (step, 64-row tile, 32-unit slice) block.  Row 64 of every input (and the
last row where that is another one) is a copy of row 0: alone in its tile, it must give row 0's bits in every per-row
output -- a row's arithmetic does not depend on the rows that share its tile.  With dropout on
(`all`, `all_stateless`) the rows draw different masks, so the row copy is asserted on the other feature sets.

Two cross-form tests per bf16 weight-stationary width (H 128, 384, 512) that the older files run at other widths only:
32-row against 64-row groups, and path 3 against paths 1 and 2 with every workgroup walking K in one order, bit for bit,
with state and with lengths.

No tolerance is new.  Worst measured errors over the 144 tests of this file (MI355X, baseline and featured), all under the
bounds in brackets: bf16 against float64: outputs and states 3.9e-3 (3e-2), gradients 6.5e-3 relative norm (4e-2); bf16
against the emulator, relative norm / max element: y and h_n 9.1e-4 / 7.5e-3 (2.4e-3 / 1.3e-2), c_n 1.3e-4 / 1.9e-4
(2.9e-4 / 3.1e-4), dx 2.2e-3 / 2.8e-3 (7e-3 / 1e-2), dh0 1.0e-3 / 1.2e-3 (2.3e-3 / 5.4e-3), dc0 3.6e-4 / 4.1e-3
(9.6e-4 / 9e-3), parameter gradients 2.3e-3 / 2.7e-3 (6e-3 / 7e-3); float32: outputs 3.3e-7 (2e-5), gradients 1.3e-6
(1e-5).  The whole file takes 44 s; the slowest test (H 1024, `all`) 1.5 s."""
import pytest
import torch

import lstm_feature_fuzz as fz
import lstm_width_matrix as wm
import test_gpu_lstm_feature_fuzz as ff
import test_gpu_lstm_state as st
from cerebralsignalnetworks_amd import cabi

pytestmark = pytest.mark.gpu

RECORDS = wm.records()
_ROW_KEYS = ("y_last", "y_all", "dx")            # [B, ...]
_LAYER_ROW_KEYS = ("h_n", "c_n", "dh0", "dc0")    # [L, B, H]


def _geometry(plan, c, what):
    assert (plan.half_tile_launches(0), plan.half_tile_launches(1)) == wm.half_tile_launches(c), (
        what, plan.half_tile_launches(0), plan.half_tile_launches(1), wm.half_tile_launches(c))
    assert plan.dgates_copies() == wm.dgates_copies(c), (what, plan.dgates_copies())


def _rows_are_copies(c, res, what):
    for row in wm.copy_rows(c["B"]):
        for k in _ROW_KEYS + _LAYER_ROW_KEYS:
            if k not in res:
                continue
            t = res[k] if k in _ROW_KEYS else res[k].transpose(0, 1)
            assert torch.equal(t[row], t[0]), (what, k, f"row {row} is not row 0", float((t[row] - t[0]).abs().max()))


@pytest.mark.parametrize("c", RECORDS, ids=[c["id"] for c in RECORDS])
def test_width_with_features_is_the_baseline_and_the_reference(c, monkeypatch):
    ff._setenv(c, monkeypatch)
    a = wm.make_inputs(c)
    w = ff._weights(a, c["L"])
    featured, baseline, plain = ff._plan(c), ff._plan(c, reverse=False), ff._plan(c, dropout=False, reverse=False)
    want_plan = wm.REGIMES[c["regime"]]["plan"]
    assert ff._triple(featured) == ff._triple(baseline) == ff._triple(plain) == fz.expected_plan(c) == want_plan, (
        c["id"], ff._triple(featured))
    lib = cabi.load()
    assert lib.csn_lstm_plan_workspace_bytes(featured._plan) == lib.csn_lstm_plan_workspace_bytes(baseline._plan) > 0
    assert featured.reverse == c["reverse"] and not baseline.reverse

    got = ff._featured(featured, c, w, a)
    base = ff._baseline(baseline, c, w, a)
    _geometry(featured, c, c["id"] + " featured")
    _geometry(baseline, c, c["id"] + " baseline")
    ff._bit_identities(c, a, got, base, c["id"])
    if c["lengths"] is not None:
        ff._same_bits(got, ff._featured(featured, c, w, a, poison=True), c["id"] + " NaN / Inf padding")
    torch.cuda.synchronize()
    assert featured.status() == 0 and baseline.status() == 0 and plain.status() == 0

    plain_terms = dict(c, dx_add=False, accumulate=False)
    want = fz.reference(plain_terms, a)
    emu = fz.reference(plain_terms, a, rounding=True) if c["dtype"] == "bf16" else None
    base_keys = [k for k in base if c["state"] or k not in ("h_n", "c_n")]
    line_b, bad_b = ff._against_reference(c, base, base_keys, want, emu, c["id"] + " baseline")
    want, emu = fz.add_previous(c, a, want), (fz.add_previous(c, a, emu) if emu is not None else None)
    line_f, bad_f = ff._against_reference(c, got, [k for k in got if k in want], want, emu, c["id"] + " featured")
    print(line_b)
    print(line_f)
    assert not bad_b + bad_f, (bad_b + bad_f)[:4]

    if c["dropout"] is None:
        _rows_are_copies(c, base, c["id"] + " baseline")
        _rows_are_copies(c, got, c["id"] + " featured")


def _run(c, monkeypatch, a, expect):
    """One forward + backward of the record under its environment -> (results, 32-row launch counts)."""
    with monkeypatch.context() as m:
        ff._setenv(c, m)
        plan = ff._plan(c)
        assert ff._triple(plan) == fz.expected_plan(c) == expect, (c["id"], ff._triple(plan))
        res = ff._featured(plan, c, ff._weights(a, c["L"]), a)
        torch.cuda.synchronize()
        assert plan.status() == 0
        _geometry(plan, c, c["id"])
        for k, v in res.items():
            assert not torch.is_tensor(v) or k in ("ybuf", "dybuf") or bool(torch.isfinite(v).all()), (c["id"], k)
        return res, (plan.half_tile_launches(0), plan.half_tile_launches(1))


@pytest.mark.parametrize("pair", wm.half_tile_records(), ids=[p[0]["id"] for p in wm.half_tile_records()])
def test_32_row_groups_give_the_bits_of_64_row_groups(pair, monkeypatch):
    half, full = pair
    a = wm.make_inputs(half)
    got, counts = _run(half, monkeypatch, a, st.P3)
    want, none = _run(full, monkeypatch, a, st.P3)
    assert counts[0] > 0 and counts[1] > 0 and none == (0, 0), (half["id"], counts, none)
    ff._same_bits(got, want, half["id"] + " against CSN_NO_HALF_TILES")
    assert set(k for k, v in got.items() if torch.is_tensor(v)) >= {"y_all", "h_n", "c_n", "dx", "dh0", "dc0"} | set(a["lp"])


@pytest.mark.parametrize("trio", wm.diagonal_records(), ids=[t[0]["id"] for t in wm.diagonal_records()])
def test_weight_stationary_kernels_give_the_bits_of_the_per_diagonal_cells(trio, monkeypatch):
    """With every workgroup walking K in one order, the projection a GEMM and the K-split forward, path 3 computes the bits
    of path 1 and of path 2: every output, both state gradients, every parameter gradient."""
    ws, diag, diag_bwd = trio
    a = wm.make_inputs(ws)
    got, _ = _run(ws, monkeypatch, a, st.P3)
    for other, expect in ((diag, st.IL), (diag_bwd, st.P2)):
        want, _ = _run(other, monkeypatch, a, expect)
        ff._same_bits(got, want, f"{ws['id']} against {other['id']}")
    assert set(k for k, v in got.items() if torch.is_tensor(v)) >= {"y_last", "y_all", "h_n", "c_n", "dx", "dh0", "dc0"} | set(a["lp"])
