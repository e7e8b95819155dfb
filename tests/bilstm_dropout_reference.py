"""References for the bidirectional LSTM's inter-layer dropout, shared by tests/test_bilstm_dropout_cpu.py and
tests/test_gpu_bilstm_dropout.py (not a test module).  Built from parts that exist without the feature: the numpy Philox
keep rule of tests/dropout_reference.py, and the bidirectional stack composed from single-layer modules
(tests/bilstm_reference.py) with ``where(keep, out * s, 0)`` between the layers."""
import numpy as np
import torch

import bilstm_reference as bref
import dropout_reference as dref


def element_index(first, index_pitch, B, T, H):
    """[B, T, H] uint64: the index csn_lstm_plan_set_output_dropout gives element (b, t, h) of a plan's y_all."""
    r = np.arange(B * T, dtype=np.uint64).reshape(B, T, 1)
    return np.uint64(first) + r * np.uint64(index_pitch) + np.arange(H, dtype=np.uint64)


def keep_at(seed, subsequence, p, e):
    """The keep rule of tests/dropout_reference.py (keep) at arbitrary indices: e a uint64 array -> bool array of its
    shape.  (A pitched plan's elements are not consecutive.)"""
    e = np.asarray(e, dtype=np.uint64)
    quad = e >> np.uint64(2)
    words = dref.philox4x32_10((quad & dref._LO, quad >> dref._S32, int(subsequence), 0),
                               (int(seed) & 0xFFFFFFFF, (int(seed) >> 32) & 0xFFFFFFFF))
    w = np.stack([np.broadcast_to(v, e.shape) for v in words], axis=-1)
    w = np.take_along_axis(w, (e & np.uint64(3)).astype(np.int64)[..., None], axis=-1)[..., 0]
    return w.astype(np.uint64) >= np.uint64(dref.threshold(p))


def plan_keep(seed, subsequence, p, first, index_pitch, B, T, H):
    """[B, T, H] bool torch tensor: the keep mask of one plan's y_all / dy_all under (p, seed, subsequence, first,
    index_pitch)."""
    return torch.from_numpy(keep_at(seed, subsequence, p, element_index(first, index_pitch, B, T, H)))


def interface_masks(seed, subsequence, p, L, B, T, H):
    """masks[l] [B, T, 2H] bool for l < L - 1: interface l (the concatenated output of layer l) is the consecutive
    elements l B T 2H ... of ONE stream, as torch drops the concatenation once."""
    n = B * T * 2 * H
    return [torch.from_numpy(dref.keep(seed, subsequence, p, l * n, n).reshape(B, T, 2 * H)) for l in range(L - 1)]


def apply_mask(out, keep, s):
    """where(keep, out * s, 0): a dropped element is a selected zero (s = inf at p = 1, where nothing is kept)."""
    if not np.isfinite(s):
        assert not bool(keep.any())
        return torch.zeros_like(out)
    return torch.where(keep.to(out.device), out * s, torch.zeros_like(out))


def composed(layers, call, x, hx, lengths, masks, s):
    """bilstm_reference.composed with the mask and scale between the layers (masks = None: nothing between them)."""
    inp, hs, cs = x, [], []
    for l, pair in enumerate(layers):
        sub = None if hx is None else (hx[0][2 * l:2 * l + 2], hx[1][2 * l:2 * l + 2])
        inp, (h, c) = bref.composed([pair], call, inp, sub, lengths)
        hs.append(h)
        cs.append(c)
        if masks is not None and l + 1 < len(layers):
            inp = apply_mask(inp, masks[l], s)
    return inp, (torch.cat(hs, 0), torch.cat(cs, 0))
