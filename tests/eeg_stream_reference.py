"""References for the stateful band-pass (csn_eeg_bandpass_stream), shared by tests/test_eeg_stream_cpu.py and
tests/test_gpu_eeg_stream.py (not a test module):
  (a) the float64 reference: scipy.signal.sosfilt(sos, x, zi=...) with the layout conversion of the state,
  (b) a numpy emulator of the two kernels' arithmetic, built on oracle.eeg_filter._cascade_steps (imported unmodified),
  (c) the seeded inputs of the tests, and ERRORS: what the emulator loses against (a) on each of them, measured by
      tests/test_eeg_stream_cpu.py (which fails when the table and a fresh measurement disagree) and imported by the GPU
      tests as the basis of their bounds.
"""
import numpy as np
from scipy.signal import sosfilt

from oracle import eeg_filter

CHUNKS, LENGTH = 16, 32
TILE = CHUNKS * LENGTH

# ---------------------------------------------------------------------------------------------------------------------
# the cases: (B, C, T) -> what the shape exercises; section counts per path
# ---------------------------------------------------------------------------------------------------------------------
SCAN_SHAPES = [
    (1, 4, 4),          # one float4
    (1, 4, 32),         # one chunk
    (1, 4, 512),        # one full tile
    (2, 32, 1024),      # two full tiles, the carry between tiles
    (3, 36, 1500),      # 108 rows = 3 row tiles + 12 rows; two full tiles + 476 samples; a partial chunk of 28
    (2, 8, 544),        # the partial tile is exactly one chunk, no re-run
    (1, 8, 20000),      # 40 tiles of carry
]
ROW_SHAPES = [(2, 6, 513), (1, 5, 96)]          # the row-walking path by T % 4 and by C % 4
SCAN_NSEC = (0, 1, 3, 5)
ROW_NSEC = (6,)
PIECES_SHAPE = (2, 32, 4096 + 476)
ALIGNED_PIECES = [512, 1024, 2048, 988]
UNALIGNED_PIECES = [100, 412, 700, 4, 832, 1000, 1524]
ODD_PIECES = [101, 411, 700, 4, 832, 1001, 1523]      # the same cuts moved by one sample: odd lengths and odd offsets


def takes_scan(C, T, nsec, row_stride=None, offset=0):
    """The dispatch rule of csn_eeg_bandpass_stream for a 16-byte aligned base pointer (without CSN_FILTER_V1);
    ``offset``: the piece starts that many samples into its buffer."""
    row_stride = T if row_stride is None else row_stride
    return nsec <= 5 and C % 4 == 0 and T % 4 == 0 and row_stride % 4 == 0 and offset % 4 == 0


def sos_of(nsec):
    """A Butterworth band-pass of order n has n sections."""
    return eeg_filter.design_bandpass_sos(1000, nsec) if nsec else np.zeros((0, 6))


def case_key(B, C, T, nsec, state, affine):
    return f"{B}x{C}x{T}-n{nsec}-{'rand' if state else 'zero'}-{'affine' if affine else 'plain'}"


def inputs(B, C, T, nsec, state, affine):
    """x[B,C,T] float32 after the recipe of oracle.eeg_filter.synthetic_eeg -- with a DC offset of 50 where the case has an
    affine (the dataset-level (x - mu) / sigma is what takes such an offset out) --, the start state [B,C,nsec,2] float64
    (None = start of a recording; otherwise a state that a preceding piece of such a signal leaves behind) and the affine (mean[C], inv_std[C]) float32 or (None, None)."""
    seed = 7000 + 131 * B + 17 * C + T + 3 * nsec + (1 if state else 0) + (2 if affine else 0)
    x = eeg_filter.synthetic_eeg(B, C, T, seed=seed)
    rng = np.random.default_rng(seed + 1)
    mean = inv_std = None
    if affine:
        x = (x.astype(np.float64) + 50.0).astype(np.float32)
    st = None
    if state:
        # a state the filter can be in: where 300 samples of the same kind of signal leave it, times a random factor per
        # row (independent normal components would be a state no input produces: the output would start with a
        # transient of order 1e3)
        lead = rng.standard_normal((B, C, 300)) + (50.0 if affine else 0.0)
        st = reference(lead, sos_of(nsec))[1] * (0.5 + rng.random((B, C, 1, 1)))
    if affine:
        mean = (0.5 * rng.standard_normal(C)).astype(np.float32)
        inv_std = (1.0 / (1.0 + rng.random(C))).astype(np.float32)
    return x, st, mean, inv_std


def pieces_input(offset):
    """The recording of the piece tests: PIECES_SHAPE, with or without a DC offset of 50."""
    B, C, T = PIECES_SHAPE
    x = eeg_filter.synthetic_eeg(B, C, T, seed=4572 + int(offset))
    return (x.astype(np.float64) + offset).astype(np.float32) if offset else x


# ---------------------------------------------------------------------------------------------------------------------
# (a) the float64 reference
# ---------------------------------------------------------------------------------------------------------------------
def to_zi(state):
    """[B,C,nsec,2] -> scipy's zi[nsec,B,C,2]."""
    return np.ascontiguousarray(np.transpose(state, (2, 0, 1, 3)))


def from_zi(zi):
    return np.ascontiguousarray(np.transpose(zi, (1, 2, 0, 3)))


def reference(x_bct, sos, state=None, mean=None, inv_std=None):
    """float64: y[B,C,T] = (sosfilt(sos, x, zi) - mean[c]) * inv_std[c] and the final state [B,C,nsec,2]."""
    sos = np.asarray(sos, np.float64).reshape(-1, 6)
    x = np.asarray(x_bct, np.float64)
    B, C, T = x.shape
    nsec = len(sos)
    if nsec:
        zi = to_zi(state) if state is not None else np.zeros((nsec, B, C, 2))
        y, zf = sosfilt(sos, x, axis=-1, zi=zi)
        out_state = from_zi(zf)
    else:
        y, out_state = x.copy(), np.zeros((B, C, 0, 2))
    if mean is not None:
        y = (y - np.asarray(mean, np.float64)[None, :, None]) * np.asarray(inv_std, np.float64)[None, :, None]
    return y, out_state


def reference_extended(x_bct, sos, state=None):
    """The same cascade in numpy's extended precision (80-bit on x86): what the float64 reference itself loses is the
    distance between the two.  Returns (filtered [B,C,T], state [B,C,nsec,2]) as longdouble."""
    sos = np.asarray(sos, np.float64).reshape(-1, 6).astype(np.longdouble)
    x = np.asarray(x_bct, np.float64).astype(np.longdouble)
    B, C, T = x.shape
    nsec = len(sos)
    s = (np.asarray(state, np.float64).astype(np.longdouble).reshape(B, C, 2 * nsec).copy() if state is not None
         else np.zeros((B, C, 2 * nsec), np.longdouble))
    y = eeg_filter._cascade_steps(sos, x, s) if nsec else x
    return y, s.reshape(B, C, nsec, 2)


def reference_fused(x_bct, sos, state=None):
    """The same cascade in float64 with every multiply-add FUSED (one rounding), in the form the kernels spell out:
    y = fma(b0, v, s1); s1 = fma(b1, v, fma(-a1, y, s2)); s2 = fma(b2, v, -(a2 y)).  numpy has no fma: the product and
    the sum are formed in extended precision (64-bit mantissa: the product carries a relative 2^-64 instead of 0) and
    rounded to float64 once.  scipy rounds every product and every sum; both are legitimate float64 evaluations of the
    reference, and their distance is how far a correct float64 implementation may sit from scipy's bits.  Returns the
    state [B,C,nsec,2] float64."""
    LD = np.longdouble
    sos = np.asarray(sos, np.float64).reshape(-1, 6)
    x = np.asarray(x_bct, np.float64)
    B, C, T = x.shape
    nsec = len(sos)
    c = [[LD(v) for v in (sec[0] / sec[3], sec[1] / sec[3], sec[2] / sec[3], sec[4] / sec[3], sec[5] / sec[3])] for sec in sos]
    s = (np.asarray(state, np.float64).reshape(B * C, nsec, 2).copy() if state is not None else np.zeros((B * C, nsec, 2)))
    rows = x.reshape(B * C, T)
    for n in range(T):
        v = rows[:, n].astype(LD)
        for k in range(nsec):
            b0, b1, b2, a1, a2 = c[k]
            s1, s2 = s[:, k, 0].astype(LD), s[:, k, 1].astype(LD)
            y = (b0 * v + s1).astype(np.float64).astype(LD)
            inner = (-a1 * y + s2).astype(np.float64).astype(LD)
            s[:, k, 0] = (b1 * v + inner).astype(np.float64)
            prod = (-a2 * y).astype(np.float64).astype(LD)
            s[:, k, 1] = (b2 * v + prod).astype(np.float64)
            v = y
    return s.reshape(B, C, nsec, 2)


def reference_spread(x_bct, sos, state, s_ref):
    """How far legitimate evaluations of the float64 reference lie from scipy's, relative to the largest state: the larger
    of its distance from the 80-bit evaluation (its own rounding error) and from the fused float64 evaluation."""
    if not s_ref.size:
        return 0.0
    _, s_ext = reference_extended(x_bct, sos, state)
    s_fma = reference_fused(x_bct, sos, state)
    m = np.abs(s_ref).max()
    return float(max(np.abs(s_ref - s_ext).max(), np.abs(s_ref - s_fma).max()) / m)


# ---------------------------------------------------------------------------------------------------------------------
# (b) the emulator
# ---------------------------------------------------------------------------------------------------------------------
def _affine_f32(y64, mean, inv_std):
    if mean is not None:
        y64 = (y64 - np.asarray(mean, np.float64)[:, None]) * np.asarray(inv_std, np.float64)[:, None]
    return y64.astype(np.float32)


def _emulate_scan_rows(x, sos, carry):
    """x[R,T] float32, carry[R,ns] float64 (updated copy returned) -> filtered float32 [R,T]: left-aligned tiles of
    16 chunks x 32 samples; per tile the zero-state response rounded to float32, e_0 += A carry, the Kogge-Stone scan with
    the powers of A, the homogeneous response added in float64 and rounded to float32; the state after a partial last
    tile by re-running the chunk that holds sample T from its true start state (nothing to re-run where T % 32 == 0)."""
    R, T = x.shape
    ns = 2 * len(sos)
    unit = np.eye(ns)
    phi = eeg_filter._cascade_steps(sos, np.zeros((ns, LENGTH)), unit)      # [i][n]; unit is now A e_i: A[j][i] = unit[i][j]
    A1 = unit.T.copy()
    out = np.empty((R, T), np.float32)
    carry = carry.copy()
    for t0 in range(0, T, TILE):
        valid = min(TILE, T - t0)
        v = np.zeros((R, TILE))
        v[:, :valid] = x[:, t0:t0 + valid]
        v = v.reshape(R, CHUNKS, LENGTH)
        S = np.zeros((R, CHUNKS, ns))
        v = eeg_filter._cascade_steps(sos, v, S).astype(np.float32).astype(np.float64)
        S[:, 0] = S[:, 0] + carry @ A1.T
        A, m = A1, 1
        while m < CHUNKS:
            S[:, m:] = S[:, m:] + S[:, :-m] @ A.T
            A, m = A @ A, 2 * m
        prev = np.concatenate([carry[:, None, :], S[:, :-1]], axis=1)        # the start state of every chunk
        y = (v + prev @ phi).astype(np.float32)
        out[:, t0:t0 + valid] = y.reshape(R, TILE)[:, :valid]
        kc, rem = valid // LENGTH, valid % LENGTH
        if rem == 0:
            carry = S[:, kc - 1].copy()
        else:
            carry = prev[:, kc].copy()
            eeg_filter._cascade_steps(sos, x[:, t0 + kc * LENGTH:t0 + valid].astype(np.float64), carry)
    return out, carry


def emulate(x_bct, sos, state=None, mean=None, inv_std=None, scan=True):
    """One call of csn_eeg_bandpass_stream in numpy: (y[B,C,T] float32, state_out [B,C,nsec,2] float64).  ``scan``: the
    tile-walking kernel (float32 samples between its phases, the affine applied to the rounded value in float64 and
    rounded again) or the row-walking one (the float64 cascade, the affine in float64, rounded once)."""
    sos = np.asarray(sos, np.float64).reshape(-1, 6)
    x = np.asarray(x_bct, np.float32)
    B, C, T = x.shape
    nsec = len(sos)
    rows = x.reshape(B * C, T)
    carry = (np.asarray(state, np.float64).reshape(B * C, 2 * nsec).copy() if state is not None
             else np.zeros((B * C, 2 * nsec)))
    if nsec == 0:
        f = rows.astype(np.float64)
    elif scan:
        f32, carry = _emulate_scan_rows(rows, sos, carry)
        f = f32.astype(np.float64)
    else:
        f = eeg_filter._cascade_steps(sos, rows.astype(np.float64), carry)
    f = f.reshape(B, C, T)
    y = np.stack([_affine_f32(f[b], mean, inv_std) for b in range(B)])
    return y, carry.reshape(B, C, nsec, 2)


def emulate_pieces(x_bct, sos, pieces, mean=None, inv_std=None):
    """The recording piece by piece, the state threaded through; every piece takes the kernel its length and offset
    select.  Returns (y[B,C,T] float32, final state)."""
    nsec = len(np.asarray(sos).reshape(-1, 6))
    B, C, T = x_bct.shape
    assert sum(pieces) == T
    ys, st, t = [], None, 0
    for n in pieces:
        y, st = emulate(x_bct[:, :, t:t + n], sos, st, mean, inv_std, scan=takes_scan(C, n, nsec, T, t))
        ys.append(y)
        t += n
    return np.concatenate(ys, axis=2), st


def errors(y, state, y_ref, state_ref):
    """(max |y - ref|, max |state - ref| / max |ref state|); the second is 0 where there is no state."""
    ey = float(np.abs(np.asarray(y, np.float64) - y_ref).max())
    es = float(np.abs(state - state_ref).max() / np.abs(state_ref).max()) if state_ref.size else 0.0
    return ey, es


def all_cases():
    for shapes, nsecs in ((SCAN_SHAPES, SCAN_NSEC), (ROW_SHAPES, ROW_NSEC)):
        for (B, C, T) in shapes:
            for nsec in nsecs:
                for state in (False, True):
                    for affine in (False, True):
                        yield B, C, T, nsec, state, affine


def bound(key, y_ref, state_ref):
    """The GPU's bounds for a case: 2 x what the emulator loses on it (ERRORS[key]) -- the factor because the device
    contracts and orders its float64 operations differently from numpy.  Where the emulator happens to perform the
    reference's own operations in the reference's order (a single chunk, the row-walking arithmetic) it measures 0 or a
    last bit of float64, which says nothing about a device that fuses multiply and add; the measured error is therefore
    taken no smaller than what the formats and the reference itself allow (except without a filter and without an affine,
    where the kernel copies and the bound is 0): half a float32 ulp of max |y| for the output,
    and for the state the spread of the float64 reference itself (ERRORS[key][2] = reference_spread: scipy against an
    80-bit and against a fused float64 evaluation of the same cascade, all measured without a GPU), at least one float64
    ulp of the largest state."""
    ey, es, ref_own = ERRORS[key]
    if "-n0-" in key and key.endswith("plain"):
        return 0.0, 0.0           # no filter, no affine: a copy, and a copy has every bit (the emulator's 0 is the bound)
    fy = 2.0 ** -24 * float(np.abs(y_ref).max())
    fs = max(ref_own, 2.0 ** -52)
    return 2.0 * max(ey, fy), 2.0 * max(es, fs)


# ---------------------------------------------------------------------------------------------------------------------
# (c) measured by tests/test_eeg_stream_cpu.py::test_emulator_against_reference_and_table with numpy 2.2.6 and
# scipy 1.15.3: key -> (max |y - ref|, max |state - ref| / max |ref state|, reference_spread of the case).
# The state columns are float64 reassociation noise of numpy's matrix product and scipy's sosfilt: another build of
# either may move them, which is why the CPU test holds them to a factor of 2 and not to the digits.  The GPU tests'
# bounds come from THIS table, whatever a fresh measurement says.
# ---------------------------------------------------------------------------------------------------------------------
ERRORS = {
    "1x4x4-n0-zero-plain": (0.0, 0.0, 0.0),
    "1x4x4-n0-zero-affine": (1.44e-06, 0.0, 0.0),
    "1x4x4-n0-rand-plain": (0.0, 0.0, 0.0),
    "1x4x4-n0-rand-affine": (1.8e-06, 0.0, 0.0),
    "1x4x4-n1-zero-plain": (1.57e-08, 0.0, 5.76e-16),
    "1x4x4-n1-zero-affine": (1.6e-06, 0.0, 2.5e-16),
    "1x4x4-n1-rand-plain": (5.03e-08, 0.0, 2.48e-16),
    "1x4x4-n1-rand-affine": (2.24e-06, 0.0, 7.18e-16),
    "1x4x4-n3-zero-plain": (2.46e-09, 0.0, 4.33e-16),
    "1x4x4-n3-zero-affine": (4.76e-07, 0.0, 6.57e-16),
    "1x4x4-n3-rand-plain": (2.85e-08, 0.0, 6.89e-16),
    "1x4x4-n3-rand-affine": (2.23e-06, 0.0, 1.64e-15),
    "1x4x4-n5-zero-plain": (4.4e-10, 0.0, 4.04e-16),
    "1x4x4-n5-zero-affine": (1.41e-08, 0.0, 2.96e-16),
    "1x4x4-n5-rand-plain": (1.46e-08, 0.0, 5.48e-16),
    "1x4x4-n5-rand-affine": (1.48e-06, 0.0, 9.57e-16),
    "1x4x32-n0-zero-plain": (0.0, 0.0, 0.0),
    "1x4x32-n0-zero-affine": (9.47e-07, 0.0, 0.0),
    "1x4x32-n0-rand-plain": (0.0, 0.0, 0.0),
    "1x4x32-n0-rand-affine": (1.81e-06, 0.0, 0.0),
    "1x4x32-n1-zero-plain": (5.73e-08, 0.0, 1.63e-15),
    "1x4x32-n1-zero-affine": (2.75e-06, 0.0, 4.43e-15),
    "1x4x32-n1-rand-plain": (5.68e-08, 6.76e-15, 4.03e-15),
    "1x4x32-n1-rand-affine": (4.75e-06, 5.34e-15, 4.46e-15),
    "1x4x32-n3-zero-plain": (5.35e-08, 0.0, 4.13e-14),
    "1x4x32-n3-zero-affine": (2.87e-06, 0.0, 1.41e-14),
    "1x4x32-n3-rand-plain": (5.37e-08, 8.95e-14, 3.79e-14),
    "1x4x32-n3-rand-affine": (3.34e-06, 2.73e-14, 2.15e-14),
    "1x4x32-n5-zero-plain": (5.31e-08, 0.0, 1.7e-14),
    "1x4x32-n5-zero-affine": (3.43e-06, 0.0, 1.31e-14),
    "1x4x32-n5-rand-plain": (5.37e-08, 9.13e-15, 7.34e-15),
    "1x4x32-n5-rand-affine": (3.83e-06, 2.73e-14, 1.78e-14),
    "1x4x512-n0-zero-plain": (0.0, 0.0, 0.0),
    "1x4x512-n0-zero-affine": (9.53e-07, 0.0, 0.0),
    "1x4x512-n0-rand-plain": (0.0, 0.0, 0.0),
    "1x4x512-n0-rand-affine": (1.91e-06, 0.0, 0.0),
    "1x4x512-n1-zero-plain": (9.76e-08, 1.02e-14, 6.57e-15),
    "1x4x512-n1-zero-affine": (4.98e-06, 3.82e-14, 1.43e-14),
    "1x4x512-n1-rand-plain": (1.11e-07, 1.23e-13, 5.41e-14),
    "1x4x512-n1-rand-affine": (3.1e-06, 3.15e-14, 1.16e-14),
    "1x4x512-n3-zero-plain": (9.29e-08, 7.5e-13, 3.43e-13),
    "1x4x512-n3-zero-affine": (3.99e-06, 1.49e-11, 1.99e-12),
    "1x4x512-n3-rand-plain": (1.14e-07, 1.9e-12, 1.08e-12),
    "1x4x512-n3-rand-affine": (3.07e-06, 4.8e-11, 8.63e-13),
    "1x4x512-n5-zero-plain": (1.08e-07, 5.26e-12, 7.36e-13),
    "1x4x512-n5-zero-affine": (4.3e-06, 2.77e-11, 1.69e-12),
    "1x4x512-n5-rand-plain": (9.2e-08, 1.12e-11, 3.08e-12),
    "1x4x512-n5-rand-affine": (3.04e-06, 7.84e-11, 7.4e-13),
    "2x32x1024-n0-zero-plain": (0.0, 0.0, 0.0),
    "2x32x1024-n0-zero-affine": (1.91e-06, 0.0, 0.0),
    "2x32x1024-n0-rand-plain": (0.0, 0.0, 0.0),
    "2x32x1024-n0-rand-affine": (1.91e-06, 0.0, 0.0),
    "2x32x1024-n1-zero-plain": (1.16e-07, 1.97e-14, 9.2e-15),
    "2x32x1024-n1-zero-affine": (4.99e-06, 1.09e-13, 3.19e-14),
    "2x32x1024-n1-rand-plain": (1.16e-07, 1.87e-14, 9.28e-15),
    "2x32x1024-n1-rand-affine": (5.19e-06, 8.72e-14, 3.18e-14),
    "2x32x1024-n3-zero-plain": (1.16e-07, 2.34e-11, 2.48e-12),
    "2x32x1024-n3-zero-affine": (5.18e-06, 3.57e-10, 9.53e-12),
    "2x32x1024-n3-rand-plain": (1.18e-07, 3.46e-11, 2.45e-12),
    "2x32x1024-n3-rand-affine": (4.74e-06, 7.95e-10, 6.46e-12),
    "2x32x1024-n5-zero-plain": (1.16e-07, 1.25e-11, 3.36e-12),
    "2x32x1024-n5-zero-affine": (5.16e-06, 1.14e-10, 7.3e-12),
    "2x32x1024-n5-rand-plain": (1.16e-07, 1.88e-11, 3.58e-12),
    "2x32x1024-n5-rand-affine": (4.01e-06, 1.95e-10, 5.11e-12),
    "3x36x1500-n0-zero-plain": (0.0, 0.0, 0.0),
    "3x36x1500-n0-zero-affine": (1.91e-06, 0.0, 0.0),
    "3x36x1500-n0-rand-plain": (0.0, 0.0, 0.0),
    "3x36x1500-n0-rand-affine": (1.91e-06, 0.0, 0.0),
    "3x36x1500-n1-zero-plain": (1.29e-07, 3.57e-14, 1.34e-14),
    "3x36x1500-n1-zero-affine": (5.25e-06, 1.33e-13, 3.54e-14),
    "3x36x1500-n1-rand-plain": (1.18e-07, 2.33e-14, 1.06e-14),
    "3x36x1500-n1-rand-affine": (5.5e-06, 9.92e-14, 2.96e-14),
    "3x36x1500-n3-zero-plain": (1.17e-07, 6.7e-11, 4.02e-12),
    "3x36x1500-n3-zero-affine": (5.33e-06, 1.28e-09, 1.22e-11),
    "3x36x1500-n3-rand-plain": (1.18e-07, 5.08e-11, 3.67e-12),
    "3x36x1500-n3-rand-affine": (4.29e-06, 2.04e-09, 8.38e-12),
    "3x36x1500-n5-zero-plain": (1.17e-07, 3.08e-11, 5.05e-12),
    "3x36x1500-n5-zero-affine": (5.13e-06, 4.17e-10, 1.04e-11),
    "3x36x1500-n5-rand-plain": (1.16e-07, 2.32e-11, 4.53e-12),
    "3x36x1500-n5-rand-affine": (3.48e-06, 6.91e-10, 7.21e-12),
    "2x8x544-n0-zero-plain": (0.0, 0.0, 0.0),
    "2x8x544-n0-zero-affine": (1.91e-06, 0.0, 0.0),
    "2x8x544-n0-rand-plain": (0.0, 0.0, 0.0),
    "2x8x544-n0-rand-affine": (1.91e-06, 0.0, 0.0),
    "2x8x544-n1-zero-plain": (1.17e-07, 1.36e-14, 8.08e-15),
    "2x8x544-n1-zero-affine": (4.96e-06, 6.21e-14, 3.22e-14),
    "2x8x544-n1-rand-plain": (1.18e-07, 3.05e-14, 8.1e-15),
    "2x8x544-n1-rand-affine": (3.77e-06, 5.92e-14, 2.11e-14),
    "2x8x544-n3-zero-plain": (1.11e-07, 4.55e-12, 1.2e-12),
    "2x8x544-n3-zero-affine": (4.93e-06, 3.25e-11, 2.3e-12),
    "2x8x544-n3-rand-plain": (1.1e-07, 5.24e-12, 1.36e-12),
    "2x8x544-n3-rand-affine": (3.83e-06, 9.55e-11, 2.52e-12),
    "2x8x544-n5-zero-plain": (1.06e-07, 1.9e-12, 1.35e-12),
    "2x8x544-n5-zero-affine": (4.96e-06, 1.99e-11, 3.25e-12),
    "2x8x544-n5-rand-plain": (1.1e-07, 3.88e-12, 1.33e-12),
    "2x8x544-n5-rand-affine": (3.27e-06, 5.76e-11, 1.2e-12),
    "1x8x20000-n0-zero-plain": (0.0, 0.0, 0.0),
    "1x8x20000-n0-zero-affine": (1.91e-06, 0.0, 0.0),
    "1x8x20000-n0-rand-plain": (0.0, 0.0, 0.0),
    "1x8x20000-n0-rand-affine": (1.91e-06, 0.0, 0.0),
    "1x8x20000-n1-zero-plain": (1.18e-07, 9.52e-15, 1.58e-14),
    "1x8x20000-n1-zero-affine": (4.79e-06, 4.29e-13, 1.3e-14),
    "1x8x20000-n1-rand-plain": (1.18e-07, 4.71e-14, 1.77e-14),
    "1x8x20000-n1-rand-affine": (4.79e-06, 4.54e-13, 8.15e-15),
    "1x8x20000-n3-zero-plain": (1.16e-07, 2.39e-10, 1.43e-11),
    "1x8x20000-n3-zero-affine": (5.37e-06, 9.91e-11, 5.92e-13),
    "1x8x20000-n3-rand-plain": (1.19e-07, 4.29e-10, 7.06e-12),
    "1x8x20000-n3-rand-affine": (4.35e-06, 2.46e-10, 5.76e-13),
    "1x8x20000-n5-zero-plain": (1.17e-07, 9.48e-11, 1.93e-11),
    "1x8x20000-n5-zero-affine": (4.49e-06, 6.16e-10, 4.71e-12),
    "1x8x20000-n5-rand-plain": (1.18e-07, 1.1e-10, 9.41e-12),
    "1x8x20000-n5-rand-affine": (3.58e-06, 4.89e-10, 3.08e-12),
    "2x6x513-n6-zero-plain": (5.96e-08, 0.0, 1.05e-12),
    "2x6x513-n6-zero-affine": (1.91e-06, 0.0, 1.53e-12),
    "2x6x513-n6-rand-plain": (5.96e-08, 0.0, 8.38e-13),
    "2x6x513-n6-rand-affine": (9.54e-07, 0.0, 1.01e-12),
    "1x5x96-n6-zero-plain": (4.12e-08, 0.0, 1.06e-13),
    "1x5x96-n6-zero-affine": (1.89e-06, 0.0, 8.23e-14),
    "1x5x96-n6-rand-plain": (5.21e-08, 0.0, 1.78e-13),
    "1x5x96-n6-rand-affine": (1.84e-06, 0.0, 1.02e-13),
}
PIECE_ERRORS = {
    "off0-n3-aligned": (1.18e-07, 2.4e-10, 7.72e-12),
    "off0-n3-unaligned": (1.18e-07, 2.66e-10, 7.72e-12),
    "off0-n3-odd": (1.18e-07, 1.35e-10, 7.72e-12),
    "off0-n5-aligned": (1.19e-07, 9.03e-11, 1.91e-11),
    "off0-n5-unaligned": (1.19e-07, 1.25e-10, 1.91e-11),
    "off0-n5-odd": (1.15e-07, 1.15e-10, 1.91e-11),
    "off50-n3-aligned": (3.79e-06, 2.62e-08, 4e-11),
    "off50-n3-unaligned": (3.78e-06, 2.65e-08, 4e-11),
    "off50-n3-odd": (2.83e-06, 1.13e-08, 4e-11),
    "off50-n5-aligned": (3.8e-06, 7.13e-09, 3.8e-11),
    "off50-n5-unaligned": (3.8e-06, 7.3e-09, 3.8e-11),
    "off50-n5-odd": (2.85e-06, 5.62e-09, 3.8e-11),
}
