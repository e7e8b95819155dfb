"""Host side of K1+K2: filter design + the fused HIP band-pass / z-score.

Mirrors /root/reference/utils/EEGFilters.py:4-28 (``EEGFilters(fs)`` with attributes
``fs, low_cutoff, high_cutoff, low_cutoff_norm, high_cutoff_norm``).  The reference only
*designs* Butterworth band-passes (orders 3/4/5, 0.1-60 Hz) and discards the coefficients;
here the design is kept in second-order sections (the polynomial form of this band is
unstable for order >= 4) and ``apply`` runs the fused HIP kernel.
"""
import numpy as np
import torch
from scipy.signal import butter

from . import cabi


class EEGFilters:
    orders = (3, 4, 5)   # EEGFilters.py:19

    def __init__(self, fs, order=3) -> None:
        self.low_cutoff = 0.1      # EEGFilters.py:10
        self.high_cutoff = 60.0    # EEGFilters.py:11
        self.fs = fs
        self.low_cutoff_norm = self.low_cutoff / (self.fs / 2)
        self.high_cutoff_norm = self.high_cutoff / (self.fs / 2)
        self.order = order
        self.Butterworth_sos = {
            o: np.asarray(butter(o, [self.low_cutoff_norm, self.high_cutoff_norm], btype="bandpass", output="sos"),
                          dtype=np.float64)
            for o in self.orders
        }

    @property
    def sos(self):
        return self.Butterworth_sos[self.order]

    def apply(self, eeg_bct, ddof=0, out_dtype=torch.float32, time_major=False):
        """eeg[B,C,T] float32 on the GPU -> band-passed, per-channel z-scored [B,T,C] (or [T,B,C])."""
        return eeg_bandpass_znorm(eeg_bct, self.sos, ddof=ddof, out_dtype=out_dtype, time_major=time_major)

    def stream(self, B, C, device, **kw):
        """A ``BandpassStream`` of the selected order for ``B`` recordings of ``C`` channels delivered in pieces."""
        return BandpassStream(self.sos, B, C, device, **kw)


def eeg_bandpass_znorm(eeg_bct, sos, ddof=0, out_dtype=torch.float32, time_major=False):
    return cabi.eeg_bandpass_znorm(eeg_bct, sos, ddof=ddof, out_dtype=out_dtype, time_major=time_major)


class BandpassStream:
    """The causal band-pass of ``B`` recordings of ``C`` channels that arrive in pieces: ``scipy.signal.sosfilt`` with
    its ``zi`` threaded from piece to piece, on the GPU.  ``stream(x_piece)`` filters ``x_piece[B,C,T]`` (any ``T``; a
    time slice of a longer tensor is not copied), returns ``y[B,T,C]`` (or ``[T,B,C]``) and advances ``state`` in place.
    Normalisation is a fixed per-channel affine ``(filtered - mean) / std`` -- dataset-level statistics, not the
    per-call z-score of ``EEGFilters.apply``, whose statistics would differ from piece to piece."""

    def __init__(self, sos, B, C, device, mean=None, std=None, out_dtype=torch.float32, time_major=False):
        device = torch.device(device)
        if device.type != "cuda":
            raise cabi.CsnError("BandpassStream needs a GPU device (no CPU fallback)")
        if (mean is None) != (std is None):
            raise cabi.CsnError("BandpassStream: mean and std are given together or not at all")
        self.sos = np.ascontiguousarray(np.asarray(sos, dtype=np.float64).reshape(-1, 6))
        self.B, self.C, self.device = int(B), int(C), device
        self.out_dtype, self.time_major = out_dtype, bool(time_major)
        self._state = self._affine = None            # device memory is taken at the first use
        self._mean_host = self._inv_std_host = None
        if mean is not None:
            m = np.broadcast_to(np.asarray(mean.cpu() if torch.is_tensor(mean) else mean, dtype=np.float64), (self.C,))
            sd = np.broadcast_to(np.asarray(std.cpu() if torch.is_tensor(std) else std, dtype=np.float64), (self.C,))
            # 1 / std once, in float64, rounded once to the float32 the kernel takes
            self._mean_host = m.astype(np.float32)
            self._inv_std_host = (1.0 / sd).astype(np.float32)

    @property
    def state(self):
        """[B,C,nsec,2] float64 on the device: the (s1, s2) of every section of every row, advanced in place."""
        if self._state is None:
            self._state = torch.zeros((self.B, self.C, self.sos.shape[0], 2), dtype=torch.float64, device=self.device)
        return self._state

    def _device_affine(self):
        if self._affine is None:
            self._affine = ((None, None) if self._mean_host is None else
                            (torch.from_numpy(self._mean_host).to(self.device),
                             torch.from_numpy(self._inv_std_host).to(self.device)))
        return self._affine

    def __call__(self, x_piece):
        return self.stream(x_piece)

    def stream(self, x_piece):
        if not torch.is_tensor(x_piece) or x_piece.dim() != 3 or x_piece.shape[0] != self.B or x_piece.shape[1] != self.C:
            raise cabi.CsnError(f"BandpassStream: expected a piece [{self.B},{self.C},T], got "
                                f"{tuple(x_piece.shape) if torch.is_tensor(x_piece) else type(x_piece)}")
        if not x_piece.is_cuda:
            raise cabi.CsnError("BandpassStream needs device tensors (no CPU fallback)")
        mean, inv_std = self._device_affine()
        y, _ = cabi.eeg_bandpass_stream(x_piece, self.sos, state_in=self.state, state_out=self.state, mean=mean,
                                        inv_std=inv_std, out_dtype=self.out_dtype, time_major=self.time_major)
        return y

    def reset(self, rows=None):
        """Zero state: every recording, or only the batch slots ``rows`` where a new recording starts."""
        if rows is None:
            self.state.zero_()
        else:
            self.state[torch.as_tensor(rows, dtype=torch.long, device=self.device)] = 0.0

    def zi(self):
        """The state in scipy's layout: float64 numpy ``[nsec,B,C,2]``, what ``sosfilt(sos, x[B,C,T], zi=...)`` takes."""
        return np.ascontiguousarray(self.state.permute(2, 0, 1, 3).cpu().numpy())

    def set_zi(self, zi):
        zi = np.asarray(zi, dtype=np.float64)
        want = (self.sos.shape[0], self.B, self.C, 2)
        if zi.shape != want:
            raise cabi.CsnError(f"BandpassStream.set_zi: expected shape {want}, got {zi.shape}")
        self.state.copy_(torch.from_numpy(np.ascontiguousarray(np.transpose(zi, (1, 2, 0, 3)))).to(self.device))


def remove_noise(eeg_data, sampling_rate):
    """``Utilities.remove_noise`` (/root/reference/utils/Utilities.py:411-428) on the GPU: Butterworth order 4,
    1-50 Hz, zero-phase (forward-backward) filtering of eeg[S,T,C]; returns a tensor of the same shape."""
    nyquist_freq = 0.5 * sampling_rate
    sos = butter(4, [1.0 / nyquist_freq, 50.0 / nyquist_freq], btype='band', output='sos')
    return cabi.eeg_filtfilt(eeg_data, sos)
