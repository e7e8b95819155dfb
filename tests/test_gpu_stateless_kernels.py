"""The stateless kernels around the LSTM -- band-pass + z-score (both kernels), zero-phase filter, cosine loss, Barlow
reduction, L2 top-k -- on every row, in every launch regime of the chunk-parallel filter kernel, on inputs that are not unit
noise, and at their argument edges.  References: oracle.eeg_filter (float64 numpy), scipy.signal.sosfiltfilt, torch's
cosine_similarity with autograd in float64 on the CPU, a stable float64 argsort.

Bounds: the filter's 5e-6 is the one of test_gpu_parity.test_filter_shapes_layouts_dtypes (float32 output rounding of a
z-scored value <= ~4 plus the float32 samples between the scan kernel's phases; tests/test_filter_scan_emulator_cpu.py pins
what that arithmetic loses on these inputs without a GPU: 6.3e-7 at worst).  filtfilt: tools/fuzz_entry_points.py's 2e-5 of
max|ref| (float64 spread of the reference at 5 - 8 sections, scipy against an 80-bit evaluation of the same cascade: 1.3e-12).
"""
import numpy as np
import pytest
import torch

from cerebralsignalnetworks_amd import cabi, Model
from oracle import eeg_filter, lstm

pytestmark = pytest.mark.gpu
ATOL = 5e-6
SCAN_ROWS = 32          # rows per tile of eeg_filter_scan_kernel
ROWS_WG = 64            # rows per workgroup of eeg_filter_rows_kernel


def dev_t(a, cuda):
    return torch.from_numpy(np.ascontiguousarray(a)).to(cuda)


def _sos(nsec):
    """design_bandpass_sos(fs 1000, order n) has n sections; 0 sections = z-score only."""
    return eeg_filter.design_bandpass_sos(1000, nsec) if nsec else None


def _oracle(x, nsec, ddof):
    if nsec == 0:
        return np.transpose(eeg_filter.zscore_rows(x, ddof), (0, 2, 1))
    return eeg_filter.eeg_bandpass_znorm(x, _sos(nsec), ddof=ddof)


def _launch_regime(cuda, B, C):
    """Mirrors launch_scan() of csrc/eeg_filter.hip: at most two resident workgroups per CU, each walks tiles
    blockIdx.x, + gridDim.x, ... -- a second loop iteration (prefetch, LDS reuse) exists only where per_wg >= 2."""
    cus = torch.cuda.get_device_properties(cuda).multi_processor_count
    slots = 2 * cus
    ntiles = -(-B * C // SCAN_ROWS)
    per_wg = -(-ntiles // slots)
    grid = -(-ntiles // per_wg)
    return dict(cus=cus, ntiles=ntiles, per_wg=per_wg, grid=grid)


def _takes_scan(C, T, nsec):
    """The dispatch rule of csn_eeg_bandpass_znorm (without CSN_FILTER_V1)."""
    return T <= 512 and T % 4 == 0 and C % 4 == 0 and nsec <= 5


def _filter(monkeypatch, kernel, xt, sos, **kw):
    """kernel 'scan': the default dispatch; 'rows': CSN_FILTER_V1 (read per call), the row-walking kernel."""
    if kernel == "rows":
        monkeypatch.setenv("CSN_FILTER_V1", "1")
    else:
        monkeypatch.delenv("CSN_FILTER_V1", raising=False)
    try:
        return cabi.eeg_bandpass_znorm(xt, sos, **kw)
    finally:
        monkeypatch.delenv("CSN_FILTER_V1", raising=False)


_REPORTS = {}


def _update_report(name, key, obj):
    """One JSON report per topic, one entry per test case: the cases of this run accumulate and the whole listing is
    rewritten after each (where and how: test_gpu_fullsize._write_report)."""
    from test_gpu_fullsize import _write_report
    _REPORTS.setdefault(name, {})[key] = obj
    _write_report(name, _REPORTS[name])


def _tile_errors(y_btc, want_btc):
    """max |y - want| per 32-row tile of the scan kernel (rows = (b, c) in memory order); NaN counts as infinite."""
    err = np.abs(y_btc - want_btc).max(axis=1).reshape(-1)            # [B*C]
    err = np.where(np.isnan(err), np.inf, err)
    pad = (-err.size) % SCAN_ROWS
    return np.concatenate([err, np.zeros(pad)]).reshape(-1, SCAN_ROWS).max(axis=1)


def _assert_all_rows(y_btc, want_btc, regime, what):
    te = _tile_errors(y_btc, want_btc)
    worst = float(te.max())
    print(f"{what}: max |hip - oracle| = {worst:.3g} over {y_btc.size} outputs")
    bad = np.nonzero(te > ATOL)[0]
    if bad.size:
        it = bad // regime["grid"]
        raise AssertionError(f"{what}: {bad.size} of {te.size} tiles over {ATOL:g} (max error {worst:.3g}); first bad tile "
                             f"{bad[0]}, bad tiles lie in loop iterations {sorted(set(it.tolist()))} of their workgroup "
                             f"(grid {regime['grid']}, per_wg {regime['per_wg']})")
    return worst


# ----------------------------------------------------------------------------------------------
# A. every row against the float64 oracle in every launch regime of the scan kernel
# ----------------------------------------------------------------------------------------------
def _regime_case(cuda, name):
    """(B, C, T, ddof, regime); B follows the CU count so that the premise holds (the figures in the comments: 256 CUs).
    The premise is asserted: on another device the case fails loudly, it never degrades to one tile per workgroup."""
    cus = torch.cuda.get_device_properties(cuda).multi_processor_count
    if name in ("cfg2", "cfg4"):                       # 256 x 128: 1024 tiles = 2 per workgroup, all workgroups even
        B, C = cus, 128
        T, ddof = (500, 0) if name == "cfg2" else (440, 1)      # 440: 14 of the 16 chunk lanes carry samples
        r = _launch_regime(cuda, B, C)
        assert r["per_wg"] == 2 and r["ntiles"] % r["grid"] == 0, r
    elif name == "uneven":                             # 275 x 128: 1100 tiles, grid 367 x 3 = 1101: the last workgroup does 2
        B, C, T, ddof = cus + cus // 16 + 3, 128, 500, 0
        if (4 * B) % 3 == 0:
            B += 1
        r = _launch_regime(cuda, B, C)
        assert r["per_wg"] >= 3 and r["ntiles"] < r["per_wg"] * r["grid"], r
    else:                                              # 130 x 132: 537 tiles, grid 269, the last tile has 8 rows
        assert name == "ragged"
        B, C, T, ddof = 2 * cus * SCAN_ROWS // 132 + 6, 132, 500, 0
        if B % 8 == 0:
            B += 1
        r = _launch_regime(cuda, B, C)
        assert r["per_wg"] >= 2 and (B * C) % SCAN_ROWS != 0 and r["ntiles"] - 1 >= r["grid"], r
    return B, C, T, ddof, r


REGIME_CASES = [("cfg2", 3), ("cfg4", 3)] + [(n, s) for n in ("uneven", "ragged") for s in range(6)]


@pytest.mark.parametrize("name,nsec", REGIME_CASES, ids=[f"{n}-{s}sec" for n, s in REGIME_CASES])
def test_filter_every_row_in_every_launch_regime(cuda, monkeypatch, name, nsec):
    """All B*T*C outputs of BOTH filter kernels against the float64 oracle where a workgroup of the scan kernel walks two or
    more tiles: the prefetch of the next tile (1 - 3 sections), the load at the top (0, 4, 5), the reuse of the one LDS
    buffer, the `tl + gridDim.x < ntiles` guard, a ragged last tile reached in a second iteration.  Every row has its own
    content, so a misplaced row is an error of order 1."""
    B, C, T, ddof, regime = _regime_case(cuda, name)
    assert _takes_scan(C, T, nsec)
    x = eeg_filter.synthetic_eeg(B, C, T, seed=1000 + 10 * nsec + len(name))
    sos = _sos(nsec)
    want = _oracle(x, nsec, ddof)                                       # [B,T,C] float64
    xt = dev_t(x, cuda)
    out = {}
    for kernel in ("scan", "rows"):
        y = _filter(monkeypatch, kernel, xt, sos, ddof=ddof)
        out[kernel] = y.cpu().numpy()
        worst = _assert_all_rows(out[kernel], want, regime, f"{name} B{B} C{C} T{T} {nsec} sections, {kernel} kernel")
        entry = dict(regime, B=B, C=C, T=T, ddof=ddof, sections=nsec, kernel=kernel, max_abs_err=worst,
                     rows_kernel_grid=-(-B * C // ROWS_WG))
        _update_report("filter_regimes.json", f"{name}-{nsec}sec-{kernel}", entry)
        if name in ("cfg2", "cfg4"):
            # the float32 [B,T,C] output is held to the oracle on every element: these two bit-equalities carry that
            # comparison over to the other layout and the other output type
            y_tm = _filter(monkeypatch, kernel, xt, sos, ddof=ddof, time_major=True)
            assert torch.equal(y_tm, y.permute(1, 0, 2)), f"{kernel}: time_major differs from the transpose"
            y_bf = _filter(monkeypatch, kernel, xt, sos, ddof=ddof, out_dtype=torch.bfloat16)
            assert torch.equal(y_bf, y.to(torch.bfloat16)), f"{kernel}: bf16 output is not the rounded float32 output"
            y_bt = _filter(monkeypatch, kernel, xt, sos, ddof=ddof, out_dtype=torch.bfloat16, time_major=True)
            assert torch.equal(y_bt, y_bf.permute(1, 0, 2)), f"{kernel}: bf16 time_major differs from the transpose"
    # The switch took effect: the scan kernel keeps float32 samples between its phases, the rows kernel does not, so with
    # a filter the two outputs differ in last bits somewhere.  Without sections both z-score the same float32 samples
    # with float64 statistics and round once: bit-equality is the expected outcome there, and the dispatch is the one
    # `if` these other section counts prove live.
    ndiff = int((out["scan"] != out["rows"]).sum())
    print(f"{name} {nsec} sections: scan and rows kernels differ in {ndiff} of {want.size} outputs")
    if nsec > 0:
        assert ndiff > 0, "CSN_FILTER_V1 changed nothing: the rows kernel did not run"


@pytest.mark.parametrize("nsec", [6, 7, 8])
@pytest.mark.parametrize("B,C,T", [(3, 50, 460),     # 150 rows: three 64-row workgroups, the last with 22 rows
                                   (2, 100, 600),    # T > 512 (float4 loads)
                                   (3, 50, 461)])    # T % 4 != 0 (scalar loads)
def test_rows_kernel_six_to_eight_sections(cuda, monkeypatch, nsec, B, C, T):
    """eeg_filter_rows_kernel<6..8>: the section counts only this kernel takes."""
    assert not _takes_scan(C, T, nsec) and B * C > 2 * ROWS_WG and (B * C) % ROWS_WG != 0
    x = eeg_filter.synthetic_eeg(B, C, T, seed=nsec * 1000 + T)
    for ddof in (0, 1):
        want = _oracle(x, nsec, ddof)
        y = _filter(monkeypatch, "scan", dev_t(x, cuda), _sos(nsec), ddof=ddof).cpu().numpy()
        err = float(np.abs(y - want).max())
        print(f"rows kernel {nsec} sections B{B} C{C} T{T} ddof{ddof}: max |hip - oracle| = {err:.3g}")
        assert err <= ATOL
    y_tm = cabi.eeg_bandpass_znorm(dev_t(x, cuda), _sos(nsec), ddof=1, time_major=True).cpu().numpy()
    np.testing.assert_array_equal(y_tm, np.transpose(y, (1, 0, 2)))


@pytest.mark.parametrize("band", [(14.0, 70.0), (1.0, 50.0)], ids=["14-70Hz", "1-50Hz"])
@pytest.mark.parametrize("nsec", [5, 6, 7, 8])
def test_filtfilt_five_to_eight_sections(cuda, nsec, band):
    """eeg_filtfilt_kernel<5..8> against scipy's sosfiltfilt in float64, at T = padlen + 1 (the shortest the ABI takes:
    the odd extension then reads every sample of the row) and at an ordinary length, S*C > 64 and not a multiple of 64.
    Bands: the fuzzer's, and the one Utilities.remove_noise applies."""
    import scipy.signal
    sos = scipy.signal.butter(nsec, band, btype="band", fs=1000, output="sos")
    assert sos.shape == (nsec, 6)
    padlen = 3 * (2 * nsec + 1)
    rng = np.random.default_rng(nsec)
    for (S, T, C) in ((3, padlen + 1, 50), (2, 333, 67)):
        assert S * C > 64 and (S * C) % 64 != 0
        x = rng.standard_normal((S, T, C)).astype(np.float32) + rng.standard_normal((S, 1, C)).astype(np.float32)
        ref = scipy.signal.sosfiltfilt(sos, x.astype(np.float64), axis=1, padlen=padlen)
        out = cabi.eeg_filtfilt(dev_t(x, cuda), sos).cpu().numpy()
        rel = float(np.abs(out - ref).max() / np.abs(ref).max())
        print(f"filtfilt {nsec} sections band {band} S{S} T{T} C{C}: max |hip - scipy| / max|ref| = {rel:.3g}")
        assert rel <= 2e-5
    with pytest.raises(cabi.CsnError):                                  # T == padlen: refused on the host
        cabi.eeg_filtfilt(torch.zeros(1, padlen, 4, device=cuda), sos)
    torch.cuda.synchronize()


# ----------------------------------------------------------------------------------------------
# B. inputs that are not unit noise; a row's trouble stays in its row
# ----------------------------------------------------------------------------------------------
KERNELS = ["scan", "rows"]
B_SHAPE = (4, 64, 500)         # 256 rows = 8 tiles of the scan kernel, 4 workgroups of the rows kernel
B_NSEC = 3


@pytest.mark.parametrize("kernel", KERNELS)
def test_filter_rows_with_dc_offsets(cuda, monkeypatch, kernel):
    """offset[b, c] from {0, 10, 1e3, 1e5} on unit noise: the band-pass removes it, its transient passes through the scan
    kernel's float32 hand-over between phases (emulated on the CPU: <= 6.3e-7, test_filter_scan_emulator_cpu.py)."""
    B, C, T = B_SHAPE
    assert _takes_scan(C, T, B_NSEC)
    rng = np.random.default_rng(11)
    off = rng.choice(np.asarray([0.0, 10.0, 1e3, 1e5], np.float32), size=(B, C, 1))
    x = (rng.standard_normal((B, C, T)).astype(np.float32) + off).astype(np.float32)
    want = _oracle(x, B_NSEC, 0)
    y = _filter(monkeypatch, kernel, dev_t(x, cuda), _sos(B_NSEC)).cpu().numpy()
    err = np.abs(y - want).max(axis=1)                                  # [B,C]
    for o in (0.0, 10.0, 1e3, 1e5):
        print(f"{kernel} kernel, offset {o:g}: max |hip - oracle| = {err[off[:, :, 0] == o].max():.3g}")
    assert err.max() <= ATOL


@pytest.mark.parametrize("kernel", KERNELS)
@pytest.mark.parametrize("nsec,T", [(3, 500), (1, 36), (5, 440), (0, 500)])
def test_filter_power_of_two_row_scaling_is_bit_exact(cuda, monkeypatch, kernel, nsec, T):
    """Each row scaled by its own 2**k, k in [-40, 40]: every operation is linear or a correctly rounded sqrt / divide and
    nothing reaches the denormal range, so no output bit may change (the oracle and the emulator have this property)."""
    B, C, _ = B_SHAPE
    rng = np.random.default_rng(12 + T)
    x = rng.standard_normal((B, C, T)).astype(np.float32)
    k = rng.integers(-40, 41, size=(B, C, 1))
    xs = np.ldexp(x, k).astype(np.float32)
    y = _filter(monkeypatch, kernel, dev_t(x, cuda), _sos(nsec))
    ys = _filter(monkeypatch, kernel, dev_t(xs, cuda), _sos(nsec))
    if not torch.equal(y, ys):
        ulps = (y.view(torch.int32).long() - ys.view(torch.int32).long()).abs()
        raise AssertionError(f"{kernel} kernel: {int((ulps > 0).sum())} outputs change under power-of-two row scaling, "
                             f"by up to {int(ulps.max())} ulp")


@pytest.mark.parametrize("kernel", KERNELS)
def test_filter_dead_and_non_finite_rows_leave_their_neighbours_alone(cuda, monkeypatch, kernel):
    """A dead electrode (all zeros), one NaN sample, one Inf sample -- first row of a tile, a middle row of a wave, last
    row of a tile, three different tiles.  In the scan kernel a row's statistics and scan travel over the 16 lanes of a DPP
    row and 32 rows share one LDS tile: every other row must keep its bits."""
    B, C, T = B_SHAPE
    x = eeg_filter.synthetic_eeg(B, C, T, seed=13)
    dead, nan_row, inf_row = 0 * SCAN_ROWS + 0, 3 * SCAN_ROWS + 13, 6 * SCAN_ROWS + 31      # (tile, row in tile)
    t_nan, t_inf = 200, 37
    bad = x.copy().reshape(B * C, T)
    bad[dead] = 0.0
    bad[nan_row, t_nan] = np.nan
    bad[inf_row, t_inf] = np.inf
    bad = bad.reshape(B, C, T)

    def rows(t):                                                        # [B,T,C] -> one row per (b, c)
        return t.permute(0, 2, 1).reshape(B * C, T)
    y = rows(_filter(monkeypatch, kernel, dev_t(x, cuda), _sos(B_NSEC)))
    yb = rows(_filter(monkeypatch, kernel, dev_t(bad, cuda), _sos(B_NSEC)))
    torch.cuda.synchronize()
    others = torch.ones(B * C, dtype=torch.bool, device=cuda)
    others[[dead, nan_row, inf_row]] = False
    assert torch.isfinite(y).all()
    changed = (y[others] != yb[others]).any(dim=1)
    assert not changed.any(), f"{int(changed.sum())} untouched rows changed (first: kept row {int(changed.nonzero()[0])})"
    assert torch.isnan(yb[dead]).all()                 # 0 / 0: normlizeEEG has no epsilon, and neither has the oracle
    with np.errstate(all="ignore"):
        assert np.isnan(_oracle(bad[:1, :1], B_NSEC, 0)).all()
    assert not torch.isfinite(yb[nan_row, t_nan:]).any()
    assert not torch.isfinite(yb[inf_row, t_inf:]).any()


# ----------------------------------------------------------------------------------------------
# C. cosine loss, top-k and argument edges (formerly tests/diag/cosine_edge.py, topk_edge.py, degenerate_args.py)
# ----------------------------------------------------------------------------------------------
def _cosine_inputs(B, D, seed):
    """Unit noise with the degenerate rows of the former cosine_edge.py: all-zero student, all-zero teacher, 1e-20
    student, 1e20 teacher (as far as B has room for them)."""
    rng = np.random.default_rng(seed)
    s = rng.standard_normal((B, D)).astype(np.float32)
    t = rng.standard_normal((B, D)).astype(np.float32)
    for row, (arr, val) in enumerate(((s, 0.0), (t, 0.0), (s, 1e-20), (t, 1e20)), start=1):
        if row < B:
            arr[row] = val
    return s, t


def _cosine_reference(s, t):
    st = torch.from_numpy(s).double().requires_grad_(True)
    loss = (1.0 - torch.nn.functional.cosine_similarity(st, torch.from_numpy(t).double(), dim=1, eps=1e-8)).mean()
    loss.backward()
    return float(loss.detach()), st.grad.numpy()


def _cosine_grad_check(g, ref, s, scale):
    """Per row, relative to that row's largest reference entry: 1e-6 (the float32 output rounding is 6e-8).  A gradient
    entry is the difference of two terms of magnitude <= scale / (B * max(|s|, eps)); where they cancel (D = 1: the
    gradient is zero) the float64 reference itself carries their rounding, ~1e-16 of that magnitude, so that much
    (with four decades of room: 1e-12) is the floor of the row's bound.  Returns (error, bound) per row."""
    B = s.shape[0]
    sn = np.maximum(np.sqrt((s.astype(np.float64) ** 2).sum(1)), 1e-8)
    tol = 1e-6 * np.abs(ref).max(axis=1) + 1e-12 * abs(scale) / (B * sn)
    return np.abs(g.astype(np.float64) - ref).max(axis=1), tol


def _assert_cosine_grad(g, ref, s, scale, what):
    err, tol = _cosine_grad_check(g, ref, s, scale)
    worst = float((err / tol).max())
    print(f"{what}: worst row at {worst:.3g} of its bound")
    assert np.isfinite(g).all() and (err <= tol).all(), (what, np.nonzero(err > tol)[0][:8], worst)


COSINE_SHAPES = [(6, 33)] + [(B, D) for B in (1, 63, 65, 300) for D in (1, 63, 64, 65, 384)]


@pytest.mark.parametrize("B,D", COSINE_SHAPES)
def test_cosine_loss_degenerate_rows_and_odd_shapes(cuda, B, D):
    """The eps clamp (zero and 1e-20 rows), a 1e20 teacher, one row per workgroup quarter (4 rows each) and row lengths
    around the 64 lanes of a wave, against torch's cosine_similarity with autograd in float64 -- the function the
    reference program calls."""
    s, t = _cosine_inputs(B, D, seed=B * 1000 + D)
    loss_ref, grad_ref = _cosine_reference(s, t)
    loss, g = cabi.cosine_loss(dev_t(s, cuda), dev_t(t, cuda))
    print(f"cosine B{B} D{D}: loss {float(loss):.7f}, reference {loss_ref:.7f}")
    assert abs(float(loss) - loss_ref) <= 2e-6
    g1 = g.cpu().numpy()
    _assert_cosine_grad(g1, grad_ref, s, 1.0, f"cosine B{B} D{D} gradient")
    # grad_scale: exactly the scaled gradient; a power of two changes only the exponent of every entry
    for scale in (3.0, -0.37):
        _, gs = cabi.cosine_loss(dev_t(s, cuda), dev_t(t, cuda), grad_scale=scale)
        scale32 = float(np.float32(scale))                             # the ABI takes a float
        _assert_cosine_grad(gs.cpu().numpy(), scale32 * grad_ref, s, scale32, f"cosine B{B} D{D} grad_scale {scale}")
    for scale in (4.0, 2.0 ** -7):
        _, gs = cabi.cosine_loss(dev_t(s, cuda), dev_t(t, cuda), grad_scale=scale)
        np.testing.assert_array_equal(gs.cpu().numpy(), g1 * np.float32(scale))
    loss_only, none = cabi.cosine_loss(dev_t(s, cuda), dev_t(t, cuda), want_grad=False)
    assert none is None and float(loss_only) == float(loss)


def _d2_kernel_order(q, g):
    """Squared distances in float64 accumulated over d in the kernel's order (one term per dimension, ascending)."""
    q, g = q.astype(np.float64), g.astype(np.float64)
    d2 = np.zeros((q.shape[0], g.shape[0]))
    for d in range(q.shape[1]):
        df = q[:, d, None] - g[None, :, d]
        d2 += df * df
    return d2


def _check_topk(g, q, k, idx, dist, what):
    """idx / dist [Nq,k] as csn_l2_topk returned them, against a stable float64 argsort."""
    d2 = _d2_kernel_order(q, g)
    ref = np.argsort(d2, axis=1, kind="stable")[:, :k]
    assert idx.shape == (q.shape[0], k) and idx.dtype == np.int64
    assert ((idx >= 0) & (idx < g.shape[0])).all(), what
    assert all(len(set(r.tolist())) == k for r in idx), f"{what}: an index is returned twice"
    mism = idx != ref
    if mism.any():
        # Exact ties (duplicate rows) have identical bits in any evaluation order and must resolve to the lower index.
        # What may differ is the ORDER of two distances that differ by rounding alone: the kernel fuses each
        # multiply-add, numpy does not -- at most D * 2**-53 of the distance (4.3e-14 at D = 384); the fuzzer's
        # distance-gap rule with that figure (and a factor 20) instead of its 1e-5.
        r, c = np.nonzero(mism)
        a, b = d2[r, idx[r, c]], d2[r, ref[r, c]]
        assert (a != b).all(), f"{what}: an exact tie did not go to the lower index (query {r[a == b][:4]})"
        assert (np.abs(a - b) <= 1e-12 * b).all(), f"{what}: wrong neighbours for queries {sorted(set(r.tolist()))[:8]}"
    want = np.take_along_axis(d2, idx, axis=1)
    with np.errstate(over="ignore"):
        want32 = want.astype(np.float32)                                # may be inf where the float64 distance is finite
    fin = np.isfinite(want32)
    np.testing.assert_array_equal(np.isfinite(dist), fin, err_msg=what)
    np.testing.assert_array_equal(dist[~fin], want32[~fin], err_msg=what)
    np.testing.assert_allclose(dist[fin], want32[fin], rtol=1.2e-7, atol=0, err_msg=what)      # one float32 ulp
    assert (np.diff(want, axis=1) >= -1e-12 * want[:, 1:]).all(), f"{what}: not ascending"


def _assert_topk(cuda, g, q, k, what):
    dist, idx = cabi.l2_topk(dev_t(g, cuda), dev_t(q, cuda), k)
    idx, dist = idx.cpu().numpy(), dist.cpu().numpy()
    _check_topk(g, q, k, idx, dist, what)
    return idx


def _gallery(Ng, Nq, D, seed):
    rng = np.random.default_rng(seed)
    return rng.standard_normal((Ng, D)).astype(np.float32), rng.standard_normal((Nq, D)).astype(np.float32)


@pytest.mark.parametrize("Ng,Nq,D,k", [(100, 7, 33, 64), (1, 1, 1, 1), (257, 1, 384, 17),          # the former topk_edge.py
                                       (64, 3, 20, 64), (65, 5, 63, 64), (257, 17, 65, 64), (5000, 3, 384, 64),
                                       (37, 19, 1, 37), (1001, 33, 63, 10), (250, 50, 65, 5), (523, 21, 384, 9)])
def test_l2_topk_at_its_edges(cuda, Ng, Nq, D, k):
    """k up to the gallery size and up to 64, sizes that are no multiple of the 16 x 16 distance tile or of the 256-thread
    selection, D around the 64-wide LDS slice; a duplicate of gallery row 0 in the middle (the tie goes to the lower
    index) and one query equal to it."""
    g, q = _gallery(Ng, Nq, D, seed=Ng + Nq + D)
    g[Ng // 2] = g[0]
    q[0] = g[0]
    idx = _assert_topk(cuda, g, q, k, f"top-k Ng{Ng} Nq{Nq} D{D} k{k}")
    if Ng > 1 and k >= 2:
        assert idx[0, 0] == 0 and idx[0, 1] == Ng // 2


@pytest.mark.parametrize("Ng,Nq,D,k,why", [(100, 7, 33, 100, "k > 64"), (5000, 3, 384, 200, "k > 64"),
                                           (3, 2, 8, 5, "k > Ng"), (100, 7, 33, 0, "k == 0")])
def test_l2_topk_refuses_k_it_cannot_serve(cuda, Ng, Nq, D, k, why):
    """include/csn_hip.h: 1 <= k <= min(64, Ng); a violation is refused on the host before any launch."""
    g, q = _gallery(Ng, Nq, D, seed=1)
    with pytest.raises(cabi.CsnError):
        cabi.l2_topk(dev_t(g, cuda), dev_t(q, cuda), k)
    torch.cuda.synchronize()


def test_l2_topk_every_distance_ties(cuda):
    """An all-equal gallery: every round of the selection is a tie over the whole row -- the strided scan inside a thread,
    the tree reduction across threads -- and the answer is exactly 0 .. k-1 for every query."""
    for (Ng, Nq, D, k) in ((1000, 5, 33, 64), (300, 3, 384, 7), (64, 2, 1, 64)):
        g, q = _gallery(Ng, Nq, D, seed=Ng)
        g[:] = g[0]
        idx = _assert_topk(cuda, g, q, k, f"all-equal gallery Ng{Ng}")
        np.testing.assert_array_equal(idx, np.broadcast_to(np.arange(k), (Nq, k)))


def test_l2_topk_duplicates_on_both_sides_of_the_selection(cuda):
    """Duplicates of gallery row 0 at g = 0 (mod 256) -- the same thread of the strided scan meets them again -- and at
    g = 255 (mod 256): another thread holds them and the tree reduction decides.  Lower index first, in both."""
    Ng, Nq, D, k = 1000, 4, 48, 8
    g, q = _gallery(Ng, Nq, D, seed=77)
    dups = [0, 255, 256, 511, 512, 767, 768]
    g[dups] = g[0]
    q[0] = g[0]
    q[1] = g[0] + np.float32(0.25)
    idx = _assert_topk(cuda, g, q, k, "duplicates at 0 and 255 mod 256")
    np.testing.assert_array_equal(idx[0, :7], dups)
    np.testing.assert_array_equal(idx[1, :7], dups)


def test_l2_topk_rows_of_magnitude_1e18(cuda):
    """Rows of magnitude 1e18: the float64 distances stay finite (1e36 * D), the float32 out_dist may overflow to inf --
    the selection works on the float64 values, so the order among the overflowing ones is still the exact one."""
    Ng, Nq, D, k = 203, 6, 384, 32
    g, q = _gallery(Ng, Nq, D, seed=18)
    g[::5] *= np.float32(1e18)
    q[1] *= np.float32(1e18)
    q[2] = g[5]
    g[9, :] = 0.0
    g[9, 0] = np.float32(1e18)                         # distance 1e36 to an ordinary query: finite in float32
    idx = _assert_topk(cuda, g, q, k, "1e18 rows")
    assert idx[2, 0] == 5


def test_zero_size_arguments_are_refused_not_faulted(cuda):
    """Every entry point's header contract (include/csn_hip.h) is 'shape violations are rejected on the host before any
    launch': zero-size calls raise CsnError -- none is promised a result -- and the device is still usable."""
    for (B, T, C, H, L) in ((0, 10, 8, 128, 1), (4, 0, 8, 128, 1), (4, 10, 0, 128, 1), (4, 10, 8, 0, 1), (4, 10, 8, 128, 0)):
        with pytest.raises(cabi.CsnError):
            cabi.LstmPlan(B, T, C, H, L, torch.bfloat16, cuda)

    def e(*shape):
        return torch.empty(*shape, device=cuda)
    calls = {"gemm_nt M=0": lambda: cabi.gemm_nt(e(0, 8), e(4, 8)),
             "gemm_nt N=0": lambda: cabi.gemm_nt(e(4, 8), e(0, 8)),
             "cosine B=0": lambda: cabi.cosine_loss(e(0, 8), e(0, 8)),
             "cosine D=0": lambda: cabi.cosine_loss(e(4, 0), e(4, 0)),
             "topk Ng=0": lambda: cabi.l2_topk(e(0, 8), torch.randn(3, 8, device=cuda), 1),
             "topk Nq=0": lambda: cabi.l2_topk(torch.randn(3, 8, device=cuda), e(0, 8), 1),
             "bandpass B=0": lambda: cabi.eeg_bandpass_znorm(e(0, 8, 100), np.ones((1, 6))),
             "bandpass C=0": lambda: cabi.eeg_bandpass_znorm(e(2, 0, 100), np.ones((1, 6))),
             "bandpass T=1": lambda: cabi.eeg_bandpass_znorm(torch.randn(2, 8, 1, device=cuda), np.ones((1, 6))),
             "filtfilt S=0": lambda: cabi.eeg_filtfilt(e(0, 100, 8), np.ones((1, 6))),
             "barlow D=0": lambda: cabi.barlow_offdiag_sqsum(e(0, 0))}
    for name, fn in calls.items():
        with pytest.raises(cabi.CsnError):
            fn()
            pytest.fail(f"{name} was accepted")
        torch.cuda.synchronize()
    # still alive, still right
    loss, _ = cabi.cosine_loss(torch.ones(2, 8, device=cuda), torch.ones(2, 8, device=cuda))
    assert abs(float(loss)) < 1e-7


@pytest.mark.parametrize("B,T,C,H,L", [(64, 20, 16, 128, 5), (32, 12, 8, 256, 6), (64, 40, 128, 768, 5)])
def test_more_layers_than_the_weight_stationary_paths_take(cuda, B, T, C, H, L):
    """(from the former degenerate_args.py) five and six layers: output against the float64 oracle, finite gradients."""
    p = lstm.init_params(C, H, L, 8, None, seed=1)
    lp = {k[len("lstm."):]: v for k, v in p.items() if k.startswith("lstm.")}
    x = np.random.default_rng(2).standard_normal((B, T, C)).astype(np.float32)
    y = lstm.lstm_forward(x, lp, L)
    y = y[0] if isinstance(y, tuple) else y
    m = Model(input_size=C, lstm_size=H, lstm_layers=L, output_size=8, include_top=False)
    m.load_state_dict({k: torch.from_numpy(v) for k, v in p.items()})
    m = m.to(cuda)
    out = m.lstm(dev_t(x, cuda))
    out.sum().backward()
    torch.cuda.synchronize()
    err = float(np.linalg.norm(out.detach().cpu().numpy() - y[:, -1]) / np.linalg.norm(y[:, -1]))
    assert err < 2e-2 and all(bool(torch.isfinite(q.grad).all()) for q in m.lstm.parameters()), err


def test_barlow_reduction_needs_a_square_matrix(cuda):
    c = torch.randn(96, 96, device=cuda)
    out = cabi.barlow_offdiag_sqsum(c).cpu().numpy()
    cd = c.double().cpu().numpy()
    on = ((np.diag(cd) - 1) ** 2).sum()
    np.testing.assert_allclose(out, [on, (cd ** 2).sum() - (np.diag(cd) ** 2).sum()], rtol=1e-6)
    for bad in (torch.randn(96, 32, device=cuda), torch.randn(32, 96, device=cuda), torch.randn(96, device=cuda),
                torch.randn(2, 8, 8, device=cuda)):
        with pytest.raises(cabi.CsnError):
            cabi.barlow_offdiag_sqsum(bad)
    torch.cuda.synchronize()
