"""oracle.eeg_filter.scan_emulator: the chunk-parallel filter kernel's arithmetic in numpy (float64 phases, float32 samples
between them, 16 chunks of 32, right-aligned row) against the plain float64 oracle.  It justifies, without a GPU, the inputs
tests/test_gpu_stateless_kernels.py gives the kernels under the 5e-6 bound: DC offsets up to 1e5, rows scaled by powers of two."""
import numpy as np
import pytest

from oracle import eeg_filter

ATOL = 5e-6            # the bound of tests/test_gpu_parity.py::test_filter_shapes_layouts_dtypes
OFFSETS = (0.0, 10.0, 1e3, 1e5)


def _rows(R, T, seed):
    return np.random.default_rng(seed).standard_normal((R, T)).astype(np.float32)


def _oracle(x, sos, ddof):
    y = eeg_filter.sosfilt_rows(sos, x) if len(sos) else np.asarray(x, np.float64)
    return eeg_filter.zscore_rows(y, ddof)


@pytest.mark.parametrize("order", [0, 1, 2, 3, 4, 5])
@pytest.mark.parametrize("T,ddof", [(500, 0), (440, 1), (36, 0), (512, 1), (8, 0)])
def test_emulator_matches_oracle_on_unit_noise(order, T, ddof):
    sos = eeg_filter.design_bandpass_sos(1000, order) if order else np.zeros((0, 6))
    x = _rows(32, T, seed=100 * order + T)
    err = np.abs(eeg_filter.scan_emulator(x, sos, ddof) - _oracle(x, sos, ddof)).max()
    print(f"order {order} T {T} ddof {ddof}: max |emulator - oracle| = {err:.3g}")
    assert err <= ATOL


@pytest.mark.parametrize("order", [3, 5])
def test_emulator_holds_the_bound_with_dc_offsets(order):
    """64 rows of unit noise, T = 500, each with one of the offsets 0 / 10 / 1e3 / 1e5: the band-pass removes DC, but the
    float32 samples between the phases carry the transient of the offset; measured 6.3e-7 at worst, the bound is 5e-6."""
    sos = eeg_filter.design_bandpass_sos(1000, order)
    x = _rows(64, 500, seed=order)
    off = np.asarray(OFFSETS, np.float32)[np.arange(64) % 4]
    x = x + off[:, None]
    d = np.abs(eeg_filter.scan_emulator(x, sos) - _oracle(x, sos, 0)).max(axis=1)
    for i, o in enumerate(OFFSETS):
        print(f"order {order} offset {o:g}: max |emulator - oracle| = {d[i::4].max():.3g}")
    assert d.max() <= ATOL


@pytest.mark.parametrize("order", [1, 3, 5])
@pytest.mark.parametrize("T", [36, 440, 500])
def test_power_of_two_row_scaling_changes_no_bit(order, T):
    """Every operation is linear or a correctly rounded sqrt / divide and nothing reaches the denormal range: a row scaled by
    2**k, k in [-40, 40], gives the same bits -- in the float64 oracle and in the emulated kernel arithmetic."""
    sos = eeg_filter.design_bandpass_sos(1000, order)
    x = _rows(32, T, seed=7 * order + T)
    k = np.random.default_rng(T).integers(-40, 41, size=32)
    xs = np.ldexp(x, k[:, None]).astype(np.float32)
    np.testing.assert_array_equal(eeg_filter.scan_emulator(xs, sos), eeg_filter.scan_emulator(x, sos))
    np.testing.assert_array_equal(_oracle(xs, sos, 0), _oracle(x, sos, 0))


def test_dead_and_non_finite_rows_stay_in_their_row():
    sos = eeg_filter.design_bandpass_sos(1000, 3)
    x = _rows(8, 500, seed=3)
    bad = x.copy()
    bad[1] = 0.0
    bad[4, 100] = np.nan
    bad[6, 499] = np.inf
    with np.errstate(all="ignore"):
        for f in (lambda a: eeg_filter.scan_emulator(a, sos), lambda a: _oracle(a, sos, 0)):
            y, yb = f(x), f(bad)
            keep = [0, 2, 3, 5, 7]
            np.testing.assert_array_equal(yb[keep], y[keep])
            assert np.isnan(yb[1]).all()                      # 0 / 0: normlizeEEG has no epsilon
            assert not np.isfinite(yb[4, 100:]).any() and not np.isfinite(yb[6, 499:]).any()
