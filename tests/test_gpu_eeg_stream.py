"""The stateful band-pass (csn_eeg_bandpass_stream, BandpassStream) on the GPU: both kernels against
scipy.signal.sosfilt with a state, the bit-exact piece identities, unaligned pieces, guard zones around everything that
is written, the Python stream object, and filter + LSTM driven piece by piece.

Bounds: 2 x what the numpy emulator of the kernels' arithmetic loses against the float64 reference on the same input
(tests/eeg_stream_reference.py: ERRORS / PIECE_ERRORS, measured and pinned by tests/test_eeg_stream_cpu.py; the floors
under a measured 0 are explained at eeg_stream_reference.bound).  bf16 output: 2^-8 |ref| on top of the float32 bound.
"""
import ctypes
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import eeg_stream_reference as sref                                  # noqa: E402
from cerebralsignalnetworks_amd import cabi, BandpassStream, EEGFilters, LSTM      # noqa: E402

pytestmark = pytest.mark.gpu
GUARD_BYTES = 4096


def dev_t(a, cuda):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(cuda)


def _bct(y, time_major):
    """[B,T,C] or [T,B,C] device tensor -> float64 numpy [B,C,T]."""
    y = y.float().cpu().numpy().astype(np.float64)
    return np.transpose(y, (1, 2, 0) if time_major else (0, 2, 1))


def _rel(s, s_ref):
    return float(np.abs(s - s_ref).max() / np.abs(s_ref).max()) if s_ref.size else 0.0


_REFS = {}


def _case(cuda, case):
    """Inputs, device copies and the float64 reference of a case: computed once, shared, never written to."""
    if case not in _REFS:
        x, st, mean, inv_std = sref.inputs(*case)
        y_ref, s_ref = sref.reference(x, sref.sos_of(case[3]), st, mean, inv_std)
        _REFS[case] = dict(x=dev_t(x, cuda), st=dev_t(st, cuda), mean=dev_t(mean, cuda), inv_std=dev_t(inv_std, cuda),
                           y_ref=y_ref, s_ref=s_ref)
    return _REFS[case]


# ---------------------------------------------------------------------------------------------------------------------
# 1. against the float64 reference
# ---------------------------------------------------------------------------------------------------------------------
SHAPE_NSEC = ([(s, n) for s in sref.SCAN_SHAPES for n in sref.SCAN_NSEC] +
              [(s, n) for s in sref.ROW_SHAPES for n in sref.ROW_NSEC])


@pytest.mark.parametrize("shape,nsec", SHAPE_NSEC, ids=[f"{s[0]}x{s[1]}x{s[2]}-{n}sec" for s, n in SHAPE_NSEC])
def test_stream_against_float64_reference(cuda, monkeypatch, shape, nsec):
    monkeypatch.delenv("CSN_FILTER_V1", raising=False)
    B, C, T = shape
    sos = sref.sos_of(nsec)
    scan = sref.takes_scan(C, T, nsec)
    assert scan == (shape in sref.SCAN_SHAPES)
    for state in (False, True):
        for affine in (False, True):
            case = (B, C, T, nsec, state, affine)
            key = sref.case_key(*case)
            d = _case(cuda, case)
            by, bs = sref.bound(key, d["y_ref"], d["s_ref"])
            assert cabi.eeg_bandpass_stream_path(d["x"], nsec) == int(scan), key
            for time_major in (False, True):
                y, s = cabi.eeg_bandpass_stream(d["x"], sos, state_in=d["st"], mean=d["mean"], inv_std=d["inv_std"],
                                                time_major=time_major)
                assert y.shape == ((T, B, C) if time_major else (B, T, C)) and s.shape == (B, C, nsec, 2)
                ey = float(np.abs(_bct(y, time_major) - d["y_ref"]).max())
                es = _rel(s.cpu().numpy(), d["s_ref"])
                print(f"{key} {'[T,B,C]' if time_major else '[B,T,C]'}: |y - ref| {ey:.3g} (bound {by:.3g}), "
                      f"state {es:.3g} (bound {bs:.3g})")
                assert ey <= by and es <= bs, (key, time_major, ey, by, es, bs)
            yb, sb = cabi.eeg_bandpass_stream(d["x"], sos, state_in=d["st"], mean=d["mean"], inv_std=d["inv_std"],
                                              out_dtype=torch.bfloat16)
            assert yb.dtype == torch.bfloat16
            over = np.abs(_bct(yb, False) - d["y_ref"]) - (2.0 ** -8 * np.abs(d["y_ref"]) + by)
            assert over.max() <= 0, (key, "bf16", float(over.max()))
            assert _rel(sb.cpu().numpy(), d["s_ref"]) <= bs


def test_filter_v1_switch_takes_the_row_kernel(cuda, monkeypatch):
    """CSN_FILTER_V1 (read per call) sends a scan-path shape to the row-walking kernel: the report says so, the output
    stays within the bound and differs in last bits (float32 samples between the scan kernel's phases)."""
    case = (3, 36, 1500, 3, True, False)
    d = _case(cuda, case)
    sos = sref.sos_of(3)
    monkeypatch.delenv("CSN_FILTER_V1", raising=False)
    assert cabi.eeg_bandpass_stream_path(d["x"], 3) == 1
    y_scan, s_scan = cabi.eeg_bandpass_stream(d["x"], sos, state_in=d["st"])
    monkeypatch.setenv("CSN_FILTER_V1", "1")
    assert cabi.eeg_bandpass_stream_path(d["x"], 3) == 0
    y_rows, s_rows = cabi.eeg_bandpass_stream(d["x"], sos, state_in=d["st"])
    monkeypatch.delenv("CSN_FILTER_V1")
    by, bs = sref.bound(sref.case_key(*case), d["y_ref"], d["s_ref"])
    assert np.abs(_bct(y_rows, False) - d["y_ref"]).max() <= by and _rel(s_rows.cpu().numpy(), d["s_ref"]) <= bs
    ndiff = int((y_scan != y_rows).sum())
    print(f"scan and rows kernels differ in {ndiff} of {y_scan.numel()} outputs")
    assert ndiff > 0, "CSN_FILTER_V1 changed nothing: the row-walking kernel did not run"


# ---------------------------------------------------------------------------------------------------------------------
# 2. / 3. a recording in pieces
# ---------------------------------------------------------------------------------------------------------------------
def _in_pieces(x, sos, pieces, contiguous=False, alias=True, first_state="null", **kw):
    """The pieces as time slices of the one tensor (x_row_stride > T), the state threaded through."""
    B, C, T = x.shape
    nsec = len(sos)
    st = torch.zeros(B, C, nsec, 2, dtype=torch.float64, device=x.device) if first_state == "zeros" else None
    ys, t, paths = [], 0, []
    for n in pieces:
        xs = x[:, :, t:t + n]
        if contiguous:
            xs = xs.contiguous()
        else:
            assert xs.data_ptr() == x.data_ptr() + 4 * t and (n == T or not xs.is_contiguous())
        paths.append(cabi.eeg_bandpass_stream_path(xs, nsec))
        if alias and st is not None:
            y, st = cabi.eeg_bandpass_stream(xs, sos, state_in=st, state_out=st, **kw)
        else:
            y, st = cabi.eeg_bandpass_stream(xs, sos, state_in=st, **kw)
        ys.append(y)
        t += n
    return torch.cat(ys, dim=1), st, paths


@pytest.mark.parametrize("nsec", [3, 5])
def test_aligned_pieces_have_the_bits_of_one_call(cuda, monkeypatch, nsec):
    monkeypatch.delenv("CSN_FILTER_V1", raising=False)
    x = dev_t(sref.pieces_input(0), cuda)
    sos = sref.sos_of(nsec)
    y1, s1 = cabi.eeg_bandpass_stream(x, sos)
    yp, sp, paths = _in_pieces(x, sos, sref.ALIGNED_PIECES)
    assert paths == [1] * len(sref.ALIGNED_PIECES)
    assert torch.equal(yp, y1) and torch.equal(sp, s1), "tile-aligned pieces differ from the one-shot call"
    # state_in = NULL equals an explicit zero state
    yz, sz, _ = _in_pieces(x, sos, sref.ALIGNED_PIECES, first_state="zeros")
    assert torch.equal(yz, y1) and torch.equal(sz, s1)
    # state_out aliasing state_in equals separate buffers
    yn, sn, _ = _in_pieces(x, sos, sref.ALIGNED_PIECES, alias=False)
    assert torch.equal(yn, y1) and torch.equal(sn, s1)
    # contiguous copies of the pieces equal the slices
    yc, sc, _ = _in_pieces(x, sos, sref.ALIGNED_PIECES, contiguous=True)
    assert torch.equal(yc, y1) and torch.equal(sc, s1)


@pytest.mark.parametrize("split", ["unaligned", "odd"])
@pytest.mark.parametrize("offset", [0, 50])
@pytest.mark.parametrize("nsec", [3, 5])
def test_unaligned_pieces_against_the_one_shot_reference(cuda, monkeypatch, nsec, offset, split):
    """Pieces that are not whole tiles: every cut of UNALIGNED_PIECES is a multiple of 4 samples, so these slices are
    16-byte aligned and take the scan kernel with a partial last tile; ODD_PIECES moves cuts by one sample, and the
    pieces with an odd length or an odd offset take the row-walking kernel."""
    monkeypatch.delenv("CSN_FILTER_V1", raising=False)
    pieces = {"unaligned": sref.UNALIGNED_PIECES, "odd": sref.ODD_PIECES}[split]
    x_np = sref.pieces_input(offset)
    B, C, T = x_np.shape
    x = dev_t(x_np, cuda)
    sos = sref.sos_of(nsec)
    y_ref, s_ref = sref.reference(x_np, sos)
    yp, sp, paths = _in_pieces(x, sos, pieces)
    starts = np.concatenate([[0], np.cumsum(pieces)[:-1]])
    assert paths == [int(sref.takes_scan(C, n, nsec, T, int(t))) for n, t in zip(pieces, starts)]
    assert (0 in paths) == (split == "odd") and 1 in paths
    ey_m, es_m, own = sref.PIECE_ERRORS[f"off{offset}-n{nsec}-{split}"]
    by = 2.0 * max(ey_m, 2.0 ** -24 * float(np.abs(y_ref).max()))
    bs = 2.0 * max(es_m, own, 2.0 ** -52)
    ey = float(np.abs(_bct(yp, False) - y_ref).max())
    es = _rel(sp.cpu().numpy(), s_ref)
    print(f"offset {offset}, {nsec} sections, {split}: |y - ref| {ey:.3g} (bound {by:.3g}), state {es:.3g} (bound {bs:.3g})")
    assert ey <= by and es <= bs


# ---------------------------------------------------------------------------------------------------------------------
# 4. nothing else is written
# ---------------------------------------------------------------------------------------------------------------------
def _guarded(n, dtype, cuda):
    """n elements inside a NaN-filled buffer with 4 KB guard zones on both sides: (buffer, view, guard elements)."""
    g = GUARD_BYTES // torch.empty((), dtype=dtype).element_size()
    buf = torch.full((g + n + g,), float("nan"), dtype=dtype, device=cuda)
    return buf, buf[g:g + n], g


@pytest.mark.parametrize("nsec", [3, 6], ids=["scan", "rows"])
@pytest.mark.parametrize("time_major", [False, True], ids=["BTC", "TBC"])
def test_nothing_else_is_written(cuda, monkeypatch, nsec, time_major):
    """y and state_out sit inside NaN-filled buffers with 4 KB guards; x sits at the very end of its allocation (the
    partial last tile's loads are clamped inside the row).  Every element of the results is finite, no guard is touched."""
    monkeypatch.delenv("CSN_FILTER_V1", raising=False)
    B, C, T = 3, 36, 1500
    x_np, st_np, _, _ = sref.inputs(B, C, T, nsec, True, False)
    sos = np.ascontiguousarray(sref.sos_of(nsec))
    n = B * C * T
    xbuf = torch.zeros(1024 + n, dtype=torch.float32, device=cuda)
    x = xbuf[1024:]
    x.copy_(torch.from_numpy(x_np).reshape(-1))
    assert x.data_ptr() + 4 * n == xbuf.data_ptr() + 4 * xbuf.numel() and x.data_ptr() % 16 == 0
    st_in = dev_t(st_np, cuda)
    lib = cabi.load()
    assert lib.csn_eeg_bandpass_stream_path(x.data_ptr(), T, C, T, nsec) == int(nsec <= 5)
    for dtype in (torch.float32, torch.bfloat16):
        ybuf, y, gy = _guarded(n, dtype, cuda)
        sbuf, s, gs = _guarded(B * C * nsec * 2, torch.float64, cuda)
        cabi._check(lib.csn_eeg_bandpass_stream(x.data_ptr(), T, B, C, T, sos.ctypes.data_as(ctypes.POINTER(ctypes.c_double)),
                                                nsec, st_in.data_ptr(), s.data_ptr(), None, None, y.data_ptr(),
                                                cabi._dt(dtype), int(time_major), cabi._stream()))
        torch.cuda.synchronize()
        assert bool(torch.isfinite(y).all()) and bool(torch.isfinite(s).all()), "an element of the result was not written"
        for name, buf, g in (("y", ybuf, gy), ("state_out", sbuf, gs)):
            assert bool(torch.isnan(buf[:g]).all()) and bool(torch.isnan(buf[-g:]).all()), f"a guard of {name} was written"
        want, s_want = cabi.eeg_bandpass_stream(dev_t(x_np, cuda), sos, state_in=st_in, out_dtype=dtype, time_major=time_major)
        assert torch.equal(y.view(want.shape), want) and torch.equal(s.view(s_want.shape), s_want)


# ---------------------------------------------------------------------------------------------------------------------
# 5. BandpassStream
# ---------------------------------------------------------------------------------------------------------------------
def test_bandpass_stream_object(cuda, monkeypatch):
    monkeypatch.delenv("CSN_FILTER_V1", raising=False)
    from scipy.signal import sosfilt
    B, C, T = 2, 32, 1500
    pieces = [512, 500, 488]
    x_np, _, mean, inv_std = sref.inputs(B, C, T, 3, False, True)
    std = 1.0 / inv_std.astype(np.float64)
    x = dev_t(x_np, cuda)
    filt = EEGFilters(1000, order=3)
    stream = filt.stream(B, C, cuda, mean=mean, std=std)
    assert isinstance(stream, BandpassStream) and stream.state.shape == (B, C, 3, 2) and not stream.state.any()
    inv_t = dev_t((1.0 / std).astype(np.float32), cuda)
    st, t, ys = None, 0, []
    for i, n in enumerate(pieces):
        xs = x[:, :, t:t + n]
        want, st = cabi.eeg_bandpass_stream(xs, filt.sos, state_in=st, mean=dev_t(mean, cuda), inv_std=inv_t)
        got = stream.stream(xs)
        assert torch.equal(got, want) and torch.equal(stream.state, st), f"piece {i}"
        ys.append(got)
        t += n
        if i == 0:
            zi_mid, t_mid = stream.zi(), t
    # zi() is scipy's layout: the reference continued from it gives the rest of the recording
    assert zi_mid.shape == (3, B, C, 2) and zi_mid.dtype == np.float64
    rest, _ = sosfilt(filt.sos, x_np[:, :, t_mid:].astype(np.float64), axis=-1, zi=zi_mid)
    rest = (rest - mean.astype(np.float64)[None, :, None]) * (1.0 / std).astype(np.float32).astype(np.float64)[None, :, None]
    got_rest = _bct(torch.cat(ys[1:], dim=1), False)
    assert np.abs(got_rest - rest).max() <= 2.0 * 2.0 ** -23 * np.abs(rest).max()
    # a stream resumed from zi() continues bit-identically
    other = BandpassStream(filt.sos, B, C, cuda, mean=mean, std=std)
    other.set_zi(zi_mid)
    assert np.array_equal(other.zi(), zi_mid)
    t = t_mid
    for i, n in enumerate(pieces[1:]):
        assert torch.equal(other(x[:, :, t:t + n]), ys[1 + i])
        t += n
    assert torch.equal(other.state, stream.state)
    # reset(rows=[1]) zeroes that slot only
    before = stream.state.clone()
    stream.reset(rows=[1])
    assert not stream.state[1].any() and torch.equal(stream.state[0], before[0]) and before[1].any()
    stream.reset()
    assert not stream.state.any()


# ---------------------------------------------------------------------------------------------------------------------
# 6. filter and LSTM in pieces
# ---------------------------------------------------------------------------------------------------------------------
def test_filter_and_lstm_in_pieces(cuda, monkeypatch):
    """A (2, 32, 2048) recording through a BandpassStream (order 3, bf16 output, an affine) and LSTM(32, 96, 2) with the
    state chained, in pieces of [512, 1024, 512]: output, h_n and c_n have the bits of the one-shot run (tile-aligned
    filter pieces + the LSTM's chunk identity), and no plan raised its status word."""
    monkeypatch.delenv("CSN_FILTER_V1", raising=False)
    B, C, T = 2, 32, 2048
    pieces = [512, 1024, 512]
    x_np, _, mean, inv_std = sref.inputs(B, C, T, 3, False, True)
    std = 1.0 / inv_std.astype(np.float64)
    x = dev_t(x_np, cuda)
    filt = EEGFilters(1000, order=3)
    torch.manual_seed(11)
    lstm = LSTM(32, 96, 2).to(cuda)
    with torch.no_grad():
        one = filt.stream(B, C, cuda, mean=mean, std=std, out_dtype=torch.bfloat16)
        eeg = one(x)
        assert eeg.dtype == torch.bfloat16 and eeg.shape == (B, T, C)
        out1, (h1, c1) = lstm(eeg)
        stream = filt.stream(B, C, cuda, mean=mean, std=std, out_dtype=torch.bfloat16)
        hx, outs, t = None, [], 0
        for n in pieces:
            out, hx = lstm(stream(x[:, :, t:t + n]), hx)
            outs.append(out)
            t += n
    torch.cuda.synchronize()
    assert torch.equal(stream.state, one.state)
    assert torch.equal(torch.cat(outs, dim=1), out1), "LSTM output in pieces differs from the one-shot run"
    assert torch.equal(hx[0], h1) and torch.equal(hx[1], c1)
    assert bool(torch.isfinite(out1).all()) and float(out1.abs().max()) > 0
    plans = list(lstm.all_plans())
    assert plans and all(pl.status() == 0 for pl in plans)
