"""CPU: the stateful band-pass without a GPU -- the numpy emulator of its kernels against scipy.signal.sosfilt on every
input the GPU tests use (the measured errors are the table the GPU tests take their bounds from), the two piece
identities on the emulator, the host checks and the dispatch report of the C entry point, the argument errors of
BandpassStream.

``python tests/test_eeg_stream_cpu.py`` re-measures and prints the two tables of tests/eeg_stream_reference.py."""
import ctypes
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import eeg_stream_reference as sref                                  # noqa: E402
from cerebralsignalnetworks_amd import cabi, BandpassStream, EEGFilters          # noqa: E402

SPLITS = {"aligned": sref.ALIGNED_PIECES, "unaligned": sref.UNALIGNED_PIECES, "odd": sref.ODD_PIECES}


def _round_up(v):
    """Three significant digits, never below the measurement."""
    if v == 0.0:
        return 0.0
    q = 10.0 ** (np.floor(np.log10(v)) - 2)
    return float(f"{np.ceil(v / q) * q:.3g}")


def _measure_case(B, C, T, nsec, state, affine):
    x, st, mean, inv_std = sref.inputs(B, C, T, nsec, state, affine)
    sos = sref.sos_of(nsec)
    y_ref, s_ref = sref.reference(x, sos, st, mean, inv_std)
    y, s = sref.emulate(x, sos, st, mean, inv_std, scan=sref.takes_scan(C, T, nsec))
    ey, es = sref.errors(y, s, y_ref, s_ref)
    return ey, es, sref.reference_spread(x, sos, st, s_ref)


def _measure_pieces(offset, nsec, split):
    x = sref.pieces_input(offset)
    sos = sref.sos_of(nsec)
    y_ref, s_ref = sref.reference(x, sos)
    y, s = sref.emulate_pieces(x, sos, SPLITS[split])
    ey, es = sref.errors(y, s, y_ref, s_ref)
    return ey, es, sref.reference_spread(x, sos, None, s_ref)


def _piece_keys():
    return [(off, nsec, split) for off in (0, 50) for nsec in (3, 5) for split in SPLITS]


def _close(measured, listed):
    """(y error, state error, reference's spread) against the table's row.  The y error is float32 rounding of the output:
    the table holds it rounded up at three digits.  The two state columns are float64 reassociation noise of numpy's
    matrix product and of scipy's sosfilt (1e-16 .. 1e-8), which another BLAS, numpy or scipy build may move: they agree
    with the table within a factor of 2 either way, and a 0 is a 0."""
    ey, ty = measured[0], listed[0]
    if not ey <= ty <= ey * 1.011 + 1e-300:
        return False
    return all((m == 0.0 and t == 0.0) or 0.5 * t <= m <= 2.0 * t for m, t in zip(measured[1:], listed[1:]))


CASES = list(sref.all_cases())


@pytest.mark.parametrize("B,C,T", sref.SCAN_SHAPES + sref.ROW_SHAPES, ids=lambda v: str(v))
def test_emulator_against_reference_and_table(B, C, T):
    """What the kernels' arithmetic loses against sosfilt, per case; the table the GPU tests import says the same."""
    for case in [c for c in CASES if c[:3] == (B, C, T)]:
        key = sref.case_key(*case)
        got = _measure_case(*case)
        print(f"{key}: |y - ref| {got[0]:.3g}, state {got[1]:.3g} (reference's spread {got[2]:.3g})")
        assert key in sref.ERRORS, f"{key} is not in eeg_stream_reference.ERRORS"
        assert _close(got, sref.ERRORS[key]), (key, got, sref.ERRORS[key])
        # sanity of the measurement itself: about one float32 ulp of the output, a state good to 1e-7
        y_ref, _ = sref.reference(*_ref_args(case))
        assert got[0] <= 2.0 ** -22 * max(1.0, np.abs(y_ref).max()) and got[1] < 1e-7, (key, got)


def _ref_args(case):
    x, st, mean, inv_std = sref.inputs(*case)
    return x, sref.sos_of(case[3]), st, mean, inv_std


@pytest.mark.parametrize("offset,nsec,split", _piece_keys(), ids=lambda v: str(v))
def test_emulator_pieces_against_reference_and_table(offset, nsec, split):
    key = f"off{offset}-n{nsec}-{split}"
    got = _measure_pieces(offset, nsec, split)
    print(f"{key}: |y - ref| {got[0]:.3g}, state {got[1]:.3g} (reference's spread {got[2]:.3g})")
    assert _close(got, sref.PIECE_ERRORS[key]), (key, got, sref.PIECE_ERRORS[key])


@pytest.mark.parametrize("offset", [0, 50])
@pytest.mark.parametrize("nsec", [3, 5])
def test_emulator_piece_identities(offset, nsec):
    """Pieces that are whole tiles reproduce the one-shot run bit for bit (output and final state); pieces that are not
    differ from it by float32 rounding of the output only."""
    x = sref.pieces_input(offset)
    sos = sref.sos_of(nsec)
    y1, s1 = sref.emulate(x, sos)
    ya, sa = sref.emulate_pieces(x, sos, sref.ALIGNED_PIECES)
    assert np.array_equal(ya, y1) and np.array_equal(sa, s1)
    for split in ("unaligned", "odd"):
        yu, su = sref.emulate_pieces(x, sos, SPLITS[split])
        dy = float(np.abs(yu.astype(np.float64) - y1).max())
        ds = float(np.abs(su - s1).max() / np.abs(s1).max())
        print(f"offset {offset}, {nsec} sections, {split}: |pieces - one shot| {dy:.3g}, state {ds:.3g}")
        assert 0 < dy <= 2.0 ** -21 * np.abs(y1).max() and ds < 1e-7


# ---------------------------------------------------------------------------------------------------------------------
# the C entry point without a GPU: every refusal happens on the host, before any launch
# ---------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def lib():
    return cabi.load()


def _call(lib, x=0x1000, stride=8, B=1, C=4, T=8, sos=None, nsec=1, state_in=None, state_out=None, mean=None,
          inv_std=None, y=0x2000, out_dtype=0, time_major=0):
    """The pointers are never dereferenced: every call below is refused before anything is launched."""
    if sos is None:
        sos = np.array([[1.0, 0.0, 0.0, 1.0, 0.0, 0.0]] * 8)
    sos = np.ascontiguousarray(sos, np.float64)
    rc = lib.csn_eeg_bandpass_stream(x, stride, B, C, T, sos.ctypes.data_as(ctypes.POINTER(ctypes.c_double)), nsec,
                                     state_in, state_out, mean, inv_std, y, out_dtype, time_major, None)
    return rc, lib.csn_last_error().decode()


@pytest.mark.parametrize("kw,needle", [
    (dict(x=None), "null"),
    (dict(y=None), "null"),
    (dict(B=0), "bad shape"),
    (dict(C=0), "bad shape"),
    (dict(T=0), "bad shape"),
    (dict(stride=7), "x_row_stride"),
    (dict(nsec=-1), "outside 0..8"),
    (dict(nsec=9), "outside 0..8"),
    (dict(sos=np.array([[1.0, 0.0, 0.0, 0.0, 0.0, 0.0]])), "a0 == 0"),
    (dict(out_dtype=2), "out_dtype"),
    (dict(mean=0x3000), "mean and inv_std"),
    (dict(inv_std=0x3000), "mean and inv_std"),
], ids=lambda v: "-".join(f"{k}" for k in v) if isinstance(v, dict) else None)
def test_host_checks_refuse_before_any_launch(lib, kw, needle):
    rc, msg = _call(lib, **kw)
    assert rc == 1 and "csn_eeg_bandpass_stream" in msg and needle in msg, (rc, msg)


def test_stream_path_reports_the_dispatch(lib, monkeypatch):
    monkeypatch.delenv("CSN_FILTER_V1", raising=False)
    path = lib.csn_eeg_bandpass_stream_path
    assert path(0x1000, 512, 8, 512, 3) == 1
    assert path(0x1000, 4572, 8, 4, 5) == 1 and path(0x1000, 512, 8, 512, 0) == 1
    assert path(0x1000, 512, 8, 512, 6) == 0                 # more than 5 sections
    assert path(0x1000, 512, 6, 512, 3) == 0                 # C % 4
    assert path(0x1000, 516, 8, 510, 3) == 0                 # T % 4
    assert path(0x1000, 514, 8, 512, 3) == 0                 # x_row_stride % 4
    assert path(0x1004, 512, 8, 512, 3) == 0                 # x not 16-byte aligned
    monkeypatch.setenv("CSN_FILTER_V1", "1")                 # read per call
    assert path(0x1000, 512, 8, 512, 3) == 0
    monkeypatch.delenv("CSN_FILTER_V1")
    assert path(0x1000, 512, 8, 512, 3) == 1
    for C, T, nsec, stride, off in [(8, 512, 3, 512, 0), (6, 512, 3, 512, 0), (8, 100, 5, 4572, 1212), (8, 4, 3, 4572, 1213)]:
        assert path(0x1000 + 4 * off, stride, C, T, nsec) == int(sref.takes_scan(C, T, nsec, stride, off))


def test_bandpass_stream_argument_errors():
    sos = sref.sos_of(3)
    with pytest.raises(cabi.CsnError, match="GPU"):
        BandpassStream(sos, 2, 8, "cpu")
    with pytest.raises(cabi.CsnError, match="together"):
        BandpassStream(sos, 2, 8, "cuda:0", std=np.ones(8))
    with pytest.raises(cabi.CsnError, match="together"):
        EEGFilters(1000).stream(2, 8, "cuda:0", mean=np.zeros(8))
    with pytest.raises(cabi.CsnError):
        cabi.eeg_bandpass_stream(torch.zeros(1, 4, 8), sos)                  # a CPU tensor
    s = BandpassStream(sos, 2, 8, "cuda:0")                                  # (device memory is taken at the first use)
    with pytest.raises(cabi.CsnError, match="device tensors"):
        s.stream(torch.zeros(2, 8, 16))
    with pytest.raises(cabi.CsnError, match=r"\[2,8,T\]"):
        s.stream(torch.zeros(2, 7, 16))
    with pytest.raises(cabi.CsnError, match="set_zi"):
        s.set_zi(np.zeros((3, 2, 7, 2)))


if __name__ == "__main__":
    print("ERRORS = {")
    for case in CASES:
        e = _measure_case(*case)
        print(f'    "{sref.case_key(*case)}": ({", ".join(repr(_round_up(v)) for v in e)}),')
    print("}\nPIECE_ERRORS = {")
    for off, nsec, split in _piece_keys():
        e = _measure_pieces(off, nsec, split)
        print(f'    "off{off}-n{nsec}-{split}": ({", ".join(repr(_round_up(v)) for v in e)}),')
    print("}")
