"""The pooled readout of the LSTM (csn_lstm_plan_set_readout, include/csn_hip.h) restated in numpy: not a test module.

`v` is the float32 [B, T, H] output sequence of the top layer at the caller's times (a y_all without output dropout),
`lengths` the valid steps per row (None: every row has T).

    pooled(v, lengths, mode)            y_last under "mean" / "max": [B, H] float32; rows of length 0 give zeros
    first_max(v, lengths)               the first caller time that attains a column's maximum (a NaN wins, the first NaN);
                                        -1 for rows of length 0
    expand(dy_last, v, lengths, mode)   G [B, T, H] float32: where dy_last enters -- dy_last / float32(n) at every valid
                                        step under "mean"; dy_last at first_max and +0 elsewhere under "max"
    mean_bound(result, T)               the derived bound on |mean under test - float64 mean|: ulp32(result) + T 2^-50

Also the fixtures of tests/test_gpu_lstm_readout.py that the CPU tests check first (saturated_params)."""
import numpy as np

MODES = ("mean", "max")


def rows(lengths, B, T):
    n = [T] * B if lengths is None else [int(k) for k in lengths]
    assert len(n) == B and all(0 <= k <= T for k in n), (n, B, T)
    return n


def first_max(v, lengths=None):
    v = np.asarray(v, np.float32)
    B, T, H = v.shape
    out = np.full((B, H), -1, np.int64)
    for b, n in enumerate(rows(lengths, B, T)):
        if n > 0:
            out[b] = np.argmax(v[b, :n], axis=0)      # (numpy: the first maximum, and a NaN counts as the maximum)
    return out


def pooled(v, lengths, mode):
    assert mode in MODES, mode
    v = np.asarray(v, np.float32)
    B, T, H = v.shape
    out = np.zeros((B, H), np.float32)
    at = first_max(v, lengths)
    for b, n in enumerate(rows(lengths, B, T)):
        if n == 0:
            continue
        if mode == "mean":
            out[b] = (v[b, :n].astype(np.float64).sum(axis=0) / n).astype(np.float32)
        else:
            out[b] = v[b, at[b], np.arange(H)]
    return out


def expand(dy_last, v, lengths, mode):
    assert mode in MODES, mode
    dy_last = np.asarray(dy_last, np.float32)
    v = np.asarray(v, np.float32)
    B, T, H = v.shape
    G = np.zeros((B, T, H), np.float32)
    at = first_max(v, lengths)
    for b, n in enumerate(rows(lengths, B, T)):
        if n == 0:
            continue
        if mode == "mean":
            G[b, :n] = dy_last[b] / np.float32(n)
        else:
            G[b, at[b], np.arange(H)] = dy_last[b]
    return G


def mean_bound(result, T):
    """|float32 mean under test - float64 mean of the same values|: the final rounding moves the quotient by at most one
    float32 ulp of the result (half of one, rounded to nearest; a whole one covers a result next to a binade's edge), and
    float64 partial sums of n <= T values |v| < 1 in any order err by at most T 2^-53 sum|v| <= T n 2^-53, that is
    T 2^-53 after the division by n: T 2^-50 leaves a factor of eight."""
    return np.spacing(np.abs(np.asarray(result, np.float32))).astype(np.float64) + T * 2.0 ** -50


def saturated_params(I, H, seed=5):
    """One layer whose every gate bias is +20 over small weights: i, f, o and g round to 1, c grows by 1 per step, and
    h = o tanh(c) is exactly bf16 1.0 from the step where tanh(c) rounds to it -- columns whose maximum is attained at many
    steps (the tie fixture).  nn.LSTM key names, float32."""
    g = np.random.default_rng(seed)
    return {"weight_ih_l0": (0.01 * g.standard_normal((4 * H, I))).astype(np.float32),
            "weight_hh_l0": (0.01 * g.standard_normal((4 * H, H))).astype(np.float32),
            "bias_ih_l0": np.full(4 * H, 20.0, np.float32), "bias_hh_l0": np.zeros(4 * H, np.float32)}


def tied_columns(v, lengths=None):
    """[B, H] bool: is the column's maximum attained at two or more valid steps?"""
    v = np.asarray(v, np.float32)
    B, T, H = v.shape
    out = np.zeros((B, H), bool)
    for b, n in enumerate(rows(lengths, B, T)):
        if n > 0:
            out[b] = (v[b, :n] == v[b, :n].max(axis=0)).sum(axis=0) >= 2
    return out
