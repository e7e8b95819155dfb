"""CPU tests of the bf16-faithful LSTM emulator (oracle.lstm.lstm_forward_bf16 / lstm_backward_bf16) and of the comparison
helper (oracle.compare): the rounding matches torch's bf16 cast, the emulator without rounding IS the float64 oracle, and
the bounds the GPU tests hold the bf16 kernels to (compare.BF16_EMU_BOUNDS) flag -- and locate -- defects that the
float64 bounds let through."""
import numpy as np
import pytest
import torch

from oracle import compare, lstm

B, T, I, H, L = 70, 75, 24, 128, 2          # a ragged last row tile (rows 64-69), 4 unit slices, 2 layers


def _torch_bf16(a):
    return torch.from_numpy(np.asarray(a, np.float32)).to(torch.bfloat16).float().numpy().astype(np.float64)


def test_bf16_round_matches_torch_cast():
    rng = np.random.default_rng(0)
    bits = rng.integers(0, 2 ** 32, 200000, dtype=np.uint64).astype(np.uint32)
    v = bits.view(np.float32)
    v = v[~np.isnan(v)]
    # ties: exactly half an ulp above an even and an odd bf16 mantissa; subnormals; the overflow edge; zeros; infinities
    ties = np.array([0x3F808000, 0x3F818000, 0xBF808000, 0xBF818000, 0x00008000, 0x00018000, 0x7F7F8000, 0x7F7F7FFF,
                     0xFF7F8000, 0x00000001, 0x807FFFFF, 0x00000000, 0x80000000, 0x7F800000, 0xFF800000], np.uint32)
    v = np.concatenate([v, ties.view(np.float32), rng.standard_normal(1000).astype(np.float32) * 1e-39])
    got, want = lstm.bf16_round(v), _torch_bf16(v)
    assert np.array_equal(got, want, equal_nan=False), v[got != want][:10]
    assert np.isnan(lstm.bf16_round(np.array([np.nan, np.float32(np.nan)]))).all()
    assert np.isinf(lstm.bf16_round(np.float32(3.4e38)))            # past the largest bf16: +inf, as the cast gives


def _case(seed=1):
    p = lstm.init_params(I, H, L, 8, None, seed=5)
    lp = {k[len("lstm."):]: v for k, v in p.items() if k.startswith("lstm.")}
    rng = np.random.default_rng(seed)
    x = rng.standard_normal((B, T, I)).astype(np.float32)
    dy = (rng.standard_normal((B, T, H)) * 0.1).astype(np.float32).astype(np.float64)
    dy[:, -1] += rng.standard_normal((B, H)).astype(np.float32)
    return lp, x, dy


def test_emulator_without_rounding_is_the_f64_oracle():
    lp, x, dy = _case()
    y, saved = lstm.lstm_forward(x, lp, L, return_saved=True)
    dx, g = lstm.lstm_backward(dy, lp, saved, L)
    ye, se = lstm.lstm_forward_bf16(x, lp, L, rounding=False)
    dxe, ge, _ = lstm.lstm_backward_bf16(dy, se, L, rounding=False)
    np.testing.assert_allclose(ye, y, rtol=0, atol=1e-13)
    np.testing.assert_allclose(dxe, dx, rtol=0, atol=1e-13 * np.abs(dx).max())
    for k, v in g.items():
        np.testing.assert_allclose(ge[k], v, rtol=0, atol=1e-13 * np.abs(v).max())


def test_emulator_with_rounding_is_within_bf16_distance_of_f64():
    """Rounding moves the results by about the bf16 quantisation (2^-9 relative per operand: ~2e-3 of the norm here)
    -- more than float32 arithmetic would, less than the float64 bounds the GPU tests used before the emulator."""
    lp, x, dy = _case()
    y, saved = lstm.lstm_forward(x, lp, L, return_saved=True)
    dx, g = lstm.lstm_backward(dy, lp, saved, L)
    ye, se = lstm.lstm_forward_bf16(x, lp, L)
    dxe, ge, dge = lstm.lstm_backward_bf16(dy, se, L)
    assert np.array_equal(ye, lstm.bf16_round(ye))                         # outputs are bf16 values
    assert all(np.array_equal(d, lstm.bf16_round(d)) for d in dge.values())
    for got, want in [(ye, y), (dxe, dx)] + [(ge[k], g[k]) for k in g]:
        r, _ = compare.errors(got, want)
        assert 3e-4 < r < 1e-2, r


# ---- sensitivity: defects the float64 bounds pass and the emulator bounds flag, with their block named --------------
def _stale_rows(kind, l, t, v, hs):            # the ragged last row tile reads h_{t-2} at one step of layer 1
    if kind == "h_prev" and l == 1 and t == 40:
        v = v.copy()
        v[64:] = hs[64:, t - 2]
    return v


def _stale_slice(kind, l, t, v, hs):           # layer 1, step 35: one unit slice (32-63) of h_{t-1} arrives late for row
    if kind == "h_prev" and l == 1 and t == 35:   # tile 0, which reads that slice's h_{t-2} instead
        v = v.copy()
        v[:64, 32:64] = hs[:64, t - 2, 32:64]
    return v


def _swapped_gates(kind, l, t, v, hs):         # input and forget gate swapped in units 96-127 of layer 1
    if kind == "gates" and l == 1:
        i, f, g, o = (q.copy() for q in v)
        i[:, 96:128], f[:, 96:128] = v[1][:, 96:128], v[0][:, 96:128]
        return i, f, g, o
    return v


@pytest.mark.parametrize("defect,where", [(_stale_rows, ("t=40 ", "rows 64-69")), (_stale_slice, ("t=35 ", "rows 0-63")),
                                          (_swapped_gates, ("units 96-127",))])
def test_emulator_bounds_catch_and_locate_defects(defect, where):
    lp, x, _ = _case()
    y64 = lstm.lstm_forward(x, lp, L)
    ye, _ = lstm.lstm_forward_bf16(x, lp, L)
    # a kernel stand-in: the same roundings with float32 products (accumulation noise, rounding flips)
    clean, _ = lstm.lstm_forward_bf16(x, lp, L, acc=np.float32)
    compare.check("clean", clean, ye, *compare.bf16_emu_bound("y_all"), layout="bth")
    bad, _ = lstm.lstm_forward_bf16(x, lp, L, acc=np.float32, defect=defect)
    # what the float64 bounds allow: test_fast_path_matches_oracle_and_v1 (max |y - y_ref| < 3e-2), fuzz_lstm.py (2e-2 of the norm)
    assert np.abs(bad - y64).max() < 3e-2 and compare.errors(bad, y64)[0] < 2e-2
    with pytest.raises(AssertionError) as e:
        compare.check("defect", bad, ye, *compare.bf16_emu_bound("y_all"), layout="bth")
    worst = str(e.value).split("worst blocks:\n")[1].splitlines()[0]
    assert all(w in worst for w in where), str(e.value)


def test_report_names_gate_and_slice_of_a_weight_gradient():
    rng = np.random.default_rng(3)
    want = rng.standard_normal((4 * H, 40))
    got = want.copy()
    got[2 * H + 70, 33] += 0.5                     # gate g, unit 70, column 33
    with pytest.raises(AssertionError) as e:
        compare.check("dW", got, want, 1e-6, 1e-6, layout=compare.layout_of("lstm.weight_ih_l0"))
    assert "gate g units 64-95 cols 32-39" in str(e.value).split("worst blocks:\n")[1].splitlines()[0]
    assert "1 of " in str(e.value)


@pytest.mark.parametrize("key", ["h_n", "c_n", "dh0", "dc0"])
def test_state_layout_names_layer_and_row_tile(key):
    """A defect planted in one row tile of one layer of a [L, B, H] state tensor (the ragged tile, rows 64-69, of layer
    1), under accumulation-size noise everywhere: the emulator bound flags it and the report names that layer and tile."""
    assert compare.layout_of(key) == "lbh"
    rng = np.random.default_rng(5)
    want = rng.standard_normal((3, B, H))
    got = want * (1 + 1e-5 * rng.standard_normal(want.shape))
    got[1, 64:] += 0.02 * np.abs(want).max() * rng.standard_normal((B - 64, H))
    compare.check(key, got[[0, 2]], want[[0, 2]], *compare.bf16_emu_bound(key), layout="lbh")     # the other layers pass
    with pytest.raises(AssertionError) as e:
        compare.check(key, got, want, *compare.bf16_emu_bound(key), layout=compare.layout_of(key))
    worst = str(e.value).split("worst blocks:\n")[1].splitlines()
    assert all("layer 1 rows 64-69 units " in w for w in worst[:H // 32]), str(e.value)
