"""Comparison of a kernel's output with an oracle's, with a localisation report on failure (test infrastructure only).

``check(name, got, want, rel, elem, layout)`` asserts
  * a relative-norm bound:   ||got - want|| <= rel * ||want||
  * a per-element bound:     max |got - want| <= elem * max |want|
and, when either fails, raises an AssertionError that names the worst blocks of the tensor -- for the LSTM's outputs
(layout "bth": [B, T, N]) a block is (step t, 64-row tile, 32-unit slice), for a weight gradient (layout "gk":
[4H, K], gate-major rows as torch.nn.LSTM keeps them) (gate, 32-unit slice, 32-column block), for a bias gradient
(layout "g": [4H]) (gate, 32-unit slice), for y_last (layout "bh": [B, N]) (64-row tile, 32-unit slice), for the state
and its gradients h_n, c_n, dh0, dc0 (layout "lbh": [L, B, H]) (layer, 64-row tile, 32-unit slice).  A stale
hand-off then reads as one block (or one step of one row tile), a wrong gate mapping as one gate of one slice, a
summation-order difference as scattered blocks of similar size.
"""
import numpy as np

ROW_TILE, UNIT_SLICE = 64, 32


def _blocks(d, layout):
    """(per-block max |d| as an array, function: block index -> label), from reductions over a padded reshape."""
    a = np.abs(np.asarray(d, np.float64))
    if layout == "bth":
        B, T, N = a.shape
        nb, nn_ = -(-B // ROW_TILE), -(-N // UNIT_SLICE)
        p = np.zeros((nb * ROW_TILE, T, nn_ * UNIT_SLICE))
        p[:B, :, :N] = a
        m = p.reshape(nb, ROW_TILE, T, nn_, UNIT_SLICE).max(axis=(1, 4))          # [row tile, t, slice]
        return m, lambda ix: f"t={ix[1]} rows {ix[0] * ROW_TILE}-{min(B, (ix[0] + 1) * ROW_TILE) - 1} " \
                             f"units {ix[2] * UNIT_SLICE}-{min(N, (ix[2] + 1) * UNIT_SLICE) - 1}"
    if layout == "bh":
        B, N = a.shape
        nb, nn_ = -(-B // ROW_TILE), -(-N // UNIT_SLICE)
        p = np.zeros((nb * ROW_TILE, nn_ * UNIT_SLICE))
        p[:B, :N] = a
        m = p.reshape(nb, ROW_TILE, nn_, UNIT_SLICE).max(axis=(1, 3))
        return m, lambda ix: f"rows {ix[0] * ROW_TILE}-{min(B, (ix[0] + 1) * ROW_TILE) - 1} " \
                             f"units {ix[1] * UNIT_SLICE}-{min(N, (ix[1] + 1) * UNIT_SLICE) - 1}"
    if layout == "lbh":
        NL, B, N = a.shape
        nb, nn_ = -(-B // ROW_TILE), -(-N // UNIT_SLICE)
        p = np.zeros((NL, nb * ROW_TILE, nn_ * UNIT_SLICE))
        p[:, :B, :N] = a
        m = p.reshape(NL, nb, ROW_TILE, nn_, UNIT_SLICE).max(axis=(2, 4))          # [layer, row tile, slice]
        return m, lambda ix: f"layer {ix[0]} rows {ix[1] * ROW_TILE}-{min(B, (ix[1] + 1) * ROW_TILE) - 1} " \
                             f"units {ix[2] * UNIT_SLICE}-{min(N, (ix[2] + 1) * UNIT_SLICE) - 1}"
    if layout in ("gk", "g"):
        a2 = a.reshape(a.shape[0], -1)
        G, K = a2.shape
        H = G // 4
        ns, nk = -(-H // UNIT_SLICE), -(-K // UNIT_SLICE)
        p = np.zeros((4, ns * UNIT_SLICE, nk * UNIT_SLICE))
        p[:, :H, :K] = a2.reshape(4, H, K)
        m = p.reshape(4, ns, UNIT_SLICE, nk, UNIT_SLICE).max(axis=(2, 4))           # [gate, slice, k block]
        return m, lambda ix: f"gate {'ifgo'[ix[0]]} units {ix[1] * UNIT_SLICE}-{min(H, (ix[1] + 1) * UNIT_SLICE) - 1}" + \
                             (f" cols {ix[2] * UNIT_SLICE}-{min(K, (ix[2] + 1) * UNIT_SLICE) - 1}" if layout == "gk" else "")
    m = a.reshape(1, -1).max(axis=1)
    return m, lambda ix: "whole tensor"


def errors(got, want):
    """(relative-norm error, max |got - want| / max |want|) in float64."""
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    d = got - want
    rel = float(np.linalg.norm(d) / max(1e-30, np.linalg.norm(want)))
    elem = float(np.abs(d).max() / max(1e-30, np.abs(want).max())) if d.size else 0.0
    return rel, elem


def report(got, want, layout, top=6):
    """The `top` blocks with the largest |got - want|, worst first, each with its share of the tensor's max |want|;
    and the fraction of blocks that differ at all (1 block out of many = a localised defect)."""
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    m, label = _blocks(got - want, layout)
    scale = max(1e-30, np.abs(want).max())
    flat = np.argsort(m, axis=None)[::-1][:top]
    lines = [f"  {label(np.unravel_index(i, m.shape))}: max |diff| {m.flat[i]:.3g} ({m.flat[i] / scale:.2e} of max |want|)"
             for i in flat]
    nz = int((m > 0).sum())
    return f"{nz} of {m.size} blocks differ; worst blocks:\n" + "\n".join(lines)


def check(name, got, want, rel, elem, layout=None):
    """Assert both bounds; the message carries the measured errors and the localisation report.  Returns (rel, elem)."""
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    assert got.shape == want.shape, (name, got.shape, want.shape)
    if not np.isfinite(got).all():
        raise AssertionError(f"{name}: {int((~np.isfinite(got)).sum())} non-finite values")
    e_rel, e_elem = errors(got, want)
    if e_rel > rel or e_elem > elem:
        raise AssertionError(f"{name}: relative-norm error {e_rel:.3e} (bound {rel:.1e}), max element error "
                             f"{e_elem:.3e} of max |want| (bound {elem:.1e})\n" + report(got, want, layout or "flat"))
    return e_rel, e_elem


def layout_of(key):
    """Block layout of an LSTM output / gradient by its name (torch.nn.LSTM parameter names, y_all, y_last, dx, h_n, c_n,
    dh0, dc0)."""
    if key in ("y_all", "dx"):
        return "bth"
    if key == "y_last":
        return "bh"
    if key in ("h_n", "c_n", "dh0", "dc0"):
        return "lbh"
    if key.split(".")[-1].startswith("weight_"):
        return "gk"
    if key.split(".")[-1].startswith("bias_"):
        return "g"
    return "flat"


# Bounds of the bf16 kernels against the bf16-faithful emulator (oracle.lstm.lstm_forward_bf16 / lstm_backward_bf16):
# (relative-norm bound, per-element bound as a fraction of max |want|) per kind of tensor.  Shared by the GPU tests
# (tests/test_gpu_parity.py, tests/test_gpu_fullsize.py, tests/diag/fuzz_lstm.py) and by the CPU tests that check these
# bounds catch the defects they are meant to catch (tests/test_oracle_bf16_cpu.py).
# Measured on MI355X, worst over every bf16 case of the GPU suite and 30 fuzz cases (v1 cells, per-diagonal launches at
# L = 1..8, K-split fused / projection GEMM, N-split fused / unfused, weight-stationary backward, full size cfg2 / cfg4):
#   y_all / y_last  rel 1.18e-3 (K-split, I = 500 view, y_last)   elem 6.3e-3 (H 512 and H 256 x 4 layers, y_all)
#   dx              rel 3.36e-3 (per-diagonal, L = 8, T = 300)     elem 4.3e-3 (same case)
#   gradients       rel 2.97e-3 (per-diagonal, L = 8: weight_ih_l0) elem 3.3e-3 (B 1, H 768)
# Bounds = 2 x those.  What is left is float32 summation order and the exp2 / rcp activations turning into bf16 rounding
# flips of h and dgates that the recurrence carries on: it grows with T and with the layers a gradient crosses (the
# bottom layer's gradients after 8 layers are the worst), the per-step v1 cells sit about 2 x below the MFMA paths.
# State (CSN_LSTM_STATE plans), measured on MI355X, worst over every bf16 case of tests/test_gpu_lstm_state.py (random
# state through the drop-in, dh0 tile edges at H 32 / 160, B 1 / 33 / 512, L = 8 over 300 steps, c0 x 5, chunks chained
# through the state, and every subset of the state arguments and incoming gradients on paths 0-3); h_n takes the "y" bound
# (measured rel 6.5e-4, elem 4.1e-3):
#   c_n   rel 1.44e-4 (per-diagonal, L = 8, T = 300)  elem 1.52e-4 (same case)
#   dh0   rel 1.13e-3 (path 2, argument subsets)      elem 2.66e-3 (same case)
#   dc0   rel 4.77e-4 (K-split flags, subsets)        elem 4.45e-3 (CSN_LSTM_CHUNK 4, L = 3)
# Bounds = 2 x those.  c_n never leaves float32: its error is what the bf16 flips of h feed back through the gates, 4 x
# (norm) to 25 x (element) below h_n's.  The c0 x 5 state stays within these bounds (it saturates the first steps only).
BF16_EMU_BOUNDS = {"y": (2.4e-3, 1.3e-2), "dx": (7e-3, 1e-2), "grad": (6e-3, 7e-3),
                   "c_n": (2.9e-4, 3.1e-4), "dh0": (2.3e-3, 5.4e-3), "dc0": (9.6e-4, 9e-3)}
# Saturated cells (+5 forget bias, 200 steps: f ~ 0.993, c grows and tanh(c) saturates) forget nothing, so a rounding flip
# stays in c for the rest of the sequence instead of decaying.  Measured: y rel 1.48e-3 elem 4.7e-2, dx 7.4e-3 / 5.6e-3,
# gradients 1.08e-2 / 1.07e-2; bounds 2 x those.
BF16_EMU_BOUNDS_SATURATED = {"y": (3e-3, 1e-1), "dx": (1.5e-2, 1.2e-2), "grad": (2.2e-2, 2.2e-2)}


def bf16_emu_bound(key, saturated=False):
    b = BF16_EMU_BOUNDS_SATURATED if saturated else BF16_EMU_BOUNDS
    if key in ("y_all", "y_last", "feat", "h_n"):
        return b["y"]
    if key in ("dx", "c_n", "dh0", "dc0"):
        return b[key]
    return b["grad"]
