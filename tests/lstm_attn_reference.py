"""The attention readout of the LSTM (csn_lstm_plan_set_attention, include/csn_hip.h) restated in numpy float64: not a
test module.

`v` is the float32 [B, T, H] output sequence of the top layer at the caller's times (a y_all without output dropout), `q`
the float32 [H] query, `lengths` the valid steps per row (None: every row has T).  Everything is computed in float64 from
the float32 inputs and NOT rounded, unless the name says 32: the tests hold the library's float32 results against these
within the bounds below.

    weights(v, q, scale, lengths)             a64 [B, T]: softmax over t < n of scale <v[b, t], q>, max-subtracted; 0 from
                                              n on and on rows of length 0
    forward(v, q, scale, lengths)             (y64 [B, H] = sum over t < n of a64 v, a64)
    dscore(v, q, scale, lengths, dy_last)     (w64 [B, T] = scale a64 (g64 - s64), g64 [B, T] = <dy_last[b], v[b, t]>)
    expand(a32, w32, q, dy_last, lengths)     G [B, T, H] float32 = fl32(fl32(a32 dy_last) + fl32(w32 q)) for t < n, else 0:
                                              the term of the header, three separately rounded float32 operations
    dq(w32, v, lengths)                       float64 [H] = sum over b, t < n of w32[b, t] v[b, t, h]

The bounds (ulp32(x) = the spacing of float32 at |x|: half of it is the final rounding to nearest, a whole one covers a
result next to a binade's edge):

    value_bound(y)          ulp32(y) + 2^-40.  All arithmetic is float64 with one rounding; |v| < 1 (the tests assert it)
                            and sum a = 1, so the exact value lies in (-1, 1).  The logits err by about 2 scale H max|q|
                            2^-53 (2^-46 at scale H^-1/2, H 96, |q| <= 4), which moves every weight by that relative
                            amount; the sums over T <= 37 steps err by about T 2^-53.  2^-40 leaves a 64-fold margin, and
                            a float32 accumulation anywhere (about 1e-7) fails it.
    attn_bound(a)           ulp32(a) + 2^-40 a: the same relative error of a weight, and its rounding.
    dscore_bound(w, scale, gmax)   ulp32(w) + 2^-40 scale gmax, gmax = max over t of |g64|: w = scale a (g - s) with a <= 1
                            and |g - s| <= 2 gmax, every factor in float64.
    dq_bound(dq, B, T, w32) ulp32(dq) + B T 2^-53 sum|w32|: a float64 sum of B T products |w32 v| <= |w32| in any order."""
import numpy as np

from lstm_readout_reference import rows  # noqa: F401  (re-exported: the same row lengths rule)


def weights(v, q, scale, lengths=None):
    v, q = np.asarray(v, np.float32).astype(np.float64), np.asarray(q, np.float32).astype(np.float64)
    B, T, _ = v.shape
    a = np.zeros((B, T), np.float64)
    for b, n in enumerate(rows(lengths, B, T)):
        if n == 0:
            continue
        z = float(np.float32(scale)) * (v[b, :n] @ q)
        e = np.exp(z - z.max())
        a[b, :n] = e / e.sum()
    return a


def forward(v, q, scale, lengths=None):
    a = weights(v, q, scale, lengths)
    return np.einsum("bt,bth->bh", a, np.asarray(v, np.float32).astype(np.float64)), a


def dscore(v, q, scale, lengths, dy_last):
    a = weights(v, q, scale, lengths)
    g = np.einsum("bh,bth->bt", np.asarray(dy_last, np.float32).astype(np.float64), np.asarray(v, np.float32).astype(np.float64))
    B, T = a.shape
    valid = np.arange(T)[None, :] < np.array(rows(lengths, B, T))[:, None]
    g = np.where(valid, g, 0.0)
    s = (a * g).sum(axis=1, keepdims=True)
    return float(np.float32(scale)) * a * (g - s) * valid, g


def expand(a32, w32, q, dy_last, lengths=None):
    a32, w32 = np.asarray(a32, np.float32), np.asarray(w32, np.float32)
    q, dy_last = np.asarray(q, np.float32), np.asarray(dy_last, np.float32)
    B, T = a32.shape
    G = (a32[:, :, None] * dy_last[:, None, :]).astype(np.float32) + (w32[:, :, None] * q[None, None, :]).astype(np.float32)
    assert G.dtype == np.float32
    valid = np.arange(T)[None, :] < np.array(rows(lengths, B, T))[:, None]
    return np.where(valid[:, :, None], G, np.float32(0)).astype(np.float32)


def dq(w32, v, lengths=None):
    w = np.asarray(w32, np.float32).astype(np.float64)
    B, T = w.shape
    valid = np.arange(T)[None, :] < np.array(rows(lengths, B, T))[:, None]
    vv = np.where(valid[:, :, None], np.asarray(v, np.float32).astype(np.float64), 0.0)      # (a NaN in the padding is not read)
    return np.einsum("bt,bth->h", w * valid, vv)


def ulp32(x):
    return np.spacing(np.abs(np.asarray(x, np.float32))).astype(np.float64)


def value_bound(y):
    return ulp32(y) + 2.0 ** -40


def attn_bound(a):
    return ulp32(a) + 2.0 ** -40 * np.abs(np.asarray(a, np.float64))


def dscore_bound(w, scale, gmax):
    return ulp32(w) + 2.0 ** -40 * float(scale) * np.asarray(gmax, np.float64)


def dq_bound(dq_value, B, T, w32):
    return ulp32(dq_value) + B * T * 2.0 ** -53 * float(np.abs(np.asarray(w32, np.float64)).sum())
