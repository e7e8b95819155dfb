"""ctypes binding of libcsn_hip.so (the C ABI declared in include/csn_hip.h).

This is the only place the Python host touches native code.  There is no CPU fallback:
if the library is missing or a call fails, an exception is raised.  Tensors are passed
as raw device pointers (``tensor.data_ptr()``) together with the current HIP stream of
PyTorch; PyTorch itself is used only for device memory, streams and torch.distributed.
"""
import ctypes
import os

import torch

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("CSN_LIB_PATH") or os.path.join(_HERE, "lib", "libcsn_hip.so")

CSN_F32, CSN_BF16 = 0, 1
STATUS_TIMEOUT, STATUS_NONFINITE, STATUS_STALE_SLOT = 1, 2, 4      # bits of csn_lstm_status_read (include/csn_hip.h)
ABI_VERSION = 6
LSTM_STATE = 0x100      # csn_lstm_plan_create flag CSN_LSTM_STATE (include/csn_hip.h)
LSTM_DROPOUT = 0x200    # csn_lstm_plan_create flag CSN_LSTM_DROPOUT (include/csn_hip.h)
LSTM_REVERSE = 0x400    # csn_lstm_plan_create flag CSN_LSTM_REVERSE (include/csn_hip.h)
LSTM_RESIDENT = 0x800   # csn_lstm_plan_create flag CSN_LSTM_RESIDENT: the CU-resident recurrence, H <= 128 (path 5)
RESIDENT_MAX_H = 128
TOPK_MERGE_STAGED_MAX = 2048      # csn_topk_merge keeps up to this many candidates of a query (P * k_in) in LDS
GRAD_OVERWRITE, GRAD_ACCUMULATE = 0, 1      # csn_lstm_plan_set_grad_mode (include/csn_hip.h)
SEG_DECAYED, SEG_SCALED = 1, 2              # per-segment flags of csn_flat_segments_prepare (include/csn_hip.h)

_c_void_p, _c_int, _c_i64, _c_size_t, _c_float = (ctypes.c_void_p, ctypes.c_int, ctypes.c_int64,
                                                  ctypes.c_size_t, ctypes.c_float)
_c_double = ctypes.c_double


class LstmDesc(ctypes.Structure):
    _fields_ = [("B", ctypes.c_int32), ("T", ctypes.c_int32), ("I", ctypes.c_int32),
                ("H", ctypes.c_int32), ("L", ctypes.c_int32), ("dtype", ctypes.c_int32)]


# name -> (restype, argtypes): every symbol include/csn_hip.h declares
SIGNATURES = {
    "csn_abi_version": (_c_int, []),
    "csn_last_error": (ctypes.c_char_p, []),
    "csn_target_arch": (ctypes.c_char_p, []),
    "csn_eeg_bandpass_znorm": (_c_int, [_c_void_p, _c_int, _c_int, _c_int, ctypes.POINTER(ctypes.c_double), _c_int,
                                        _c_int, _c_void_p, _c_int, _c_int, _c_void_p]),
    "csn_eeg_filtfilt_scratch_bytes": (_c_size_t, [_c_int, _c_int, _c_int, _c_int]),
    "csn_eeg_filtfilt": (_c_int, [_c_void_p, _c_int, _c_int, _c_int, ctypes.POINTER(ctypes.c_double), _c_int,
                                  _c_void_p, _c_void_p, _c_void_p]),
    "csn_eeg_bandpass_stream": (_c_int, [_c_void_p, _c_i64, _c_int, _c_int, _c_int, ctypes.POINTER(ctypes.c_double), _c_int,
                                         _c_void_p, _c_void_p, _c_void_p, _c_void_p, _c_void_p, _c_int, _c_int, _c_void_p]),
    "csn_eeg_bandpass_stream_path": (_c_int, [_c_void_p, _c_i64, _c_int, _c_int, _c_int]),
    "csn_lstm_plan_create": (_c_int, [ctypes.POINTER(LstmDesc), _c_int, ctypes.POINTER(_c_void_p)]),
    "csn_lstm_plan_destroy": (None, [_c_void_p]),
    "csn_lstm_plan_workspace_bytes": (_c_size_t, [_c_void_p]),
    "csn_lstm_plan_path": (_c_int, [_c_void_p]),
    "csn_lstm_plan_dgates_copies": (_c_int, [_c_void_p]),
    "csn_lstm_plan_half_tile_launches": (_c_int, [_c_void_p, _c_int]),
    "csn_lstm_plan_kernel_name": (ctypes.c_char_p, [_c_void_p, _c_int]),
    "csn_lstm_plan_set_grad_callback": (_c_int, [_c_void_p, _c_void_p, _c_void_p]),
    "csn_lstm_plan_set_grad_mode": (_c_int, [_c_void_p, _c_int]),
    "csn_lstm_plan_set_lengths": (_c_int, [_c_void_p, ctypes.POINTER(ctypes.c_int32)]),
    "csn_lstm_plan_set_views": (_c_int, [_c_void_p, ctypes.POINTER(ctypes.c_int32), ctypes.POINTER(ctypes.c_int32),
                                         ctypes.c_int32, ctypes.c_int32]),
    "csn_lstm_plan_set_io": (_c_int, [_c_void_p, _c_i64, _c_i64, _c_int]),
    "csn_lstm_plan_set_readout": (_c_int, [_c_void_p, _c_int]),
    "csn_lstm_plan_set_attention": (_c_int, [_c_void_p, _c_void_p, ctypes.c_float, _c_void_p, _c_void_p, _c_void_p]),
    "csn_lstm_plan_set_dropout": (_c_int, [_c_void_p, _c_float, ctypes.c_uint64, ctypes.c_uint32]),
    "csn_lstm_plan_set_output_dropout": (_c_int, [_c_void_p, _c_float, ctypes.c_uint64, ctypes.c_uint32, ctypes.c_uint64,
                                                  _c_i64]),
    "csn_lstm_dropout_keep": (_c_int, [ctypes.c_uint64, ctypes.c_uint32, _c_float, _c_i64, _c_i64, _c_void_p]),
    "csn_lstm_workspace_bytes": (_c_size_t, [ctypes.POINTER(LstmDesc), _c_int]),
    "csn_lstm_forward": (_c_int, [_c_void_p, _c_void_p, _c_i64, _c_i64,
                                  ctypes.POINTER(_c_void_p), ctypes.POINTER(_c_void_p),
                                  ctypes.POINTER(_c_void_p), ctypes.POINTER(_c_void_p),
                                  _c_void_p, _c_void_p,                        # h0, c0
                                  _c_void_p, _c_void_p, _c_void_p,             # workspace, y_last, y_all
                                  _c_void_p, _c_void_p, _c_void_p]),           # h_n, c_n, stream
    "csn_lstm_backward": (_c_int, [_c_void_p, _c_void_p, _c_void_p,
                                   _c_void_p, _c_void_p,                       # dh_n, dc_n
                                   _c_void_p,
                                   ctypes.POINTER(_c_void_p), ctypes.POINTER(_c_void_p),
                                   ctypes.POINTER(_c_void_p), ctypes.POINTER(_c_void_p),
                                   _c_void_p, _c_void_p, _c_void_p, _c_void_p]),   # dx, dh0, dc0, stream
    "csn_lstm_workspace_init": (_c_int, [_c_void_p, _c_void_p, _c_void_p]),
    "csn_lstm_status_clear": (_c_int, [_c_void_p, _c_void_p, _c_void_p]),
    "csn_lstm_status_read": (_c_int, [_c_void_p, _c_void_p, ctypes.POINTER(_c_int)]),
    "csn_lstm_status_raise": (_c_int, [_c_void_p, _c_void_p, _c_void_p]),
    "csn_lstm_profile_enable": (_c_int, [_c_void_p, _c_int]),
    "csn_lstm_profile_read": (_c_int, [_c_void_p, ctypes.POINTER(ctypes.c_double), ctypes.POINTER(_c_int),
                                       ctypes.POINTER(_c_int), ctypes.POINTER(ctypes.c_double), ctypes.POINTER(_c_int),
                                       ctypes.POINTER(_c_int)]),
    "csn_gemm_nt": (_c_int, [_c_void_p, _c_void_p, _c_void_p, _c_void_p, _c_i64, _c_i64, _c_i64,
                             _c_int, _c_int, _c_int, _c_void_p]),
    "csn_gemm_tn_scratch_bytes": (_c_size_t, [_c_i64, _c_i64, _c_i64]),
    "csn_gemm_tn": (_c_int, [_c_void_p, _c_void_p, _c_void_p, _c_i64, _c_i64, _c_i64, _c_int, _c_void_p, _c_void_p]),
    "csn_lstm_cell_forward": (_c_int, [_c_void_p, _c_void_p, _c_void_p, _c_i64, _c_void_p, _c_void_p, _c_void_p,
                                       _c_void_p, _c_int, _c_int, _c_int, _c_void_p]),
    "csn_lstm_cell_backward": (_c_int, [_c_void_p, _c_void_p, _c_void_p, _c_i64, _c_void_p, _c_void_p, _c_void_p,
                                        _c_void_p, _c_void_p, _c_int, _c_int, _c_int, _c_void_p]),
    "csn_cosine_loss_scratch_bytes": (_c_size_t, [_c_int]),
    "csn_cosine_loss": (_c_int, [_c_void_p, _c_void_p, _c_int, _c_int, _c_void_p, _c_void_p, _c_float, _c_void_p, _c_void_p]),
    "csn_distill_loss_scratch_bytes": (_c_size_t, [_c_int]),
    "csn_distill_loss": (_c_int, [_c_void_p, _c_void_p, _c_int, _c_int, _c_void_p, _c_int, _c_void_p, _c_int, _c_double,
                                  _c_double, _c_double, _c_void_p, _c_void_p, _c_void_p, _c_float, _c_void_p, _c_void_p]),
    "csn_dino_loss_scratch_bytes": (_c_size_t, [_c_int, _c_int]),
    "csn_dino_loss": (_c_int, [_c_void_p, _c_void_p, _c_int, _c_int, _c_int, _c_int, _c_void_p, _c_i64, _c_double,
                               _c_double, _c_int, _c_void_p, _c_void_p, _c_float, _c_void_p, _c_void_p]),
    "csn_rmsprop_step": (_c_int, [_c_void_p, _c_void_p, _c_void_p, _c_i64, _c_float, _c_float, _c_float, _c_void_p]),
    "csn_flat_segments_scratch_bytes": (_c_size_t, [_c_int, _c_i64]),
    "csn_flat_segments_prepare": (_c_int, [ctypes.POINTER(ctypes.c_int64), ctypes.POINTER(ctypes.c_int32), _c_int, _c_i64,
                                           _c_void_p, _c_void_p]),
    "csn_flat_segment_norms": (_c_int, [_c_void_p, _c_void_p, _c_float, _c_i64, _c_int, _c_void_p, _c_void_p, _c_void_p]),
    "csn_flat_clip": (_c_int, [_c_void_p, _c_i64, _c_int, _c_void_p, _c_float, _c_void_p, _c_void_p]),
    "csn_adam_step": (_c_int, [_c_void_p, _c_void_p, _c_void_p, _c_void_p, _c_i64, _c_int, _c_void_p, _c_i64,
                               _c_double, _c_double, _c_double, _c_double, _c_double, _c_int, _c_double, _c_void_p,
                               _c_void_p]),
    "csn_lars_step": (_c_int, [_c_void_p, _c_void_p, _c_void_p, _c_i64, _c_int, _c_void_p, _c_double, _c_double,
                               _c_double, _c_double, _c_void_p]),
    "csn_grad_guard_scratch_bytes": (_c_size_t, [_c_i64]),
    "csn_grad_guard": (_c_int, [_c_void_p, _c_i64, _c_double, _c_void_p, _c_void_p, _c_void_p]),
    "csn_rmsprop_step_guarded": (_c_int, [_c_void_p, _c_void_p, _c_void_p, _c_i64, _c_float, _c_float, _c_float, _c_void_p,
                                          _c_void_p]),
    "csn_adam_step_guarded": (_c_int, [_c_void_p, _c_void_p, _c_void_p, _c_void_p, _c_i64, _c_int, _c_void_p, _c_i64,
                                       _c_double, _c_double, _c_double, _c_double, _c_double, _c_int, _c_double, _c_void_p,
                                       _c_void_p, _c_void_p]),
    "csn_lars_step_guarded": (_c_int, [_c_void_p, _c_void_p, _c_void_p, _c_i64, _c_int, _c_void_p, _c_double, _c_double,
                                       _c_double, _c_double, _c_void_p, _c_void_p]),
    "csn_barlow_offdiag_sqsum": (_c_int, [_c_void_p, _c_int, _c_void_p, _c_void_p]),
    "csn_barlow_saved_bytes": (_c_size_t, [_c_int]),
    "csn_barlow_scratch_bytes": (_c_size_t, [_c_int, _c_int]),
    "csn_barlow_corr": (_c_int, [_c_void_p, _c_void_p, _c_int, _c_int, _c_double, _c_double, _c_void_p, _c_void_p, _c_void_p,
                                 _c_void_p, _c_double, _c_void_p]),
    "csn_barlow_grad": (_c_int, [_c_void_p, _c_void_p, _c_int, _c_int, _c_void_p, _c_void_p, _c_void_p, _c_double, _c_double,
                                 _c_float, _c_void_p, _c_void_p, _c_void_p, _c_void_p, _c_void_p]),
    "csn_contrastive_scratch_bytes": (_c_size_t, [_c_int, _c_int, _c_int]),
    "csn_contrastive_lse": (_c_int, [_c_void_p, _c_void_p, _c_void_p, _c_int, _c_int, _c_int, _c_int, _c_double, _c_double,
                                     _c_double, _c_void_p, _c_void_p, _c_void_p, _c_void_p]),
    "csn_contrastive_grad": (_c_int, [_c_void_p, _c_void_p, _c_void_p, _c_int, _c_int, _c_int, _c_int, _c_double, _c_void_p,
                                      _c_void_p, _c_double, _c_double, _c_double, _c_void_p, _c_void_p, _c_void_p, _c_void_p]),
    "csn_bank_norms": (_c_int, [_c_void_p, _c_int, _c_int, _c_void_p, _c_void_p]),
    "csn_bank_contrastive_scratch_bytes": (_c_size_t, [_c_int, _c_int, _c_int]),
    "csn_bank_contrastive": (_c_int, [_c_void_p, _c_int, _c_int, _c_void_p, _c_void_p, _c_void_p, _c_int, _c_void_p, _c_double,
                                      _c_double, _c_double, _c_void_p, _c_void_p, _c_void_p, _c_void_p, _c_void_p, _c_void_p]),
    "csn_l2_topk_scratch_bytes": (_c_size_t, [_c_i64, _c_i64]),
    "csn_l2_topk": (_c_int, [_c_void_p, _c_void_p, _c_i64, _c_i64, _c_int, _c_int, _c_void_p, _c_void_p,
                             _c_void_p, _c_void_p]),
    "csn_l2_topk_tiled_scratch_bytes": (_c_size_t, [_c_i64, _c_i64, _c_int]),
    "csn_l2_topk_tiled": (_c_int, [_c_void_p, _c_void_p, _c_i64, _c_i64, _c_int, _c_int, _c_int, _c_void_p, _c_void_p,
                                   _c_void_p, _c_void_p, _c_void_p]),
    "csn_chan_l2_dist": (_c_int, [_c_void_p, _c_i64, _c_i64, _c_void_p, _c_i64, _c_i64, _c_i64, _c_i64, _c_int, _c_int,
                                  _c_int, _c_int, ctypes.POINTER(ctypes.c_int32), _c_int, _c_void_p, _c_void_p]),
    "csn_chan_l2_select": (_c_int, [_c_void_p, _c_void_p, _c_int, _c_i64, _c_i64, _c_void_p, _c_void_p, _c_int,
                                    _c_void_p, _c_void_p, _c_void_p, _c_void_p, _c_void_p]),
    "csn_chan_l2_accumulate": (_c_int, [_c_void_p, _c_void_p, _c_i64, _c_int, _c_void_p]),
    "csn_topk_merge_staged_max": (_c_int, []),
    "csn_topk_merge": (_c_int, [_c_void_p, _c_void_p, _c_int, _c_i64, _c_int, _c_int, _c_void_p, _c_void_p, _c_void_p,
                                _c_void_p]),
    "csn_topk_class_metrics": (_c_int, [_c_void_p, _c_i64, _c_int, _c_void_p, _c_i64, _c_void_p, _c_int, _c_void_p,
                                        _c_void_p, _c_void_p, _c_void_p, _c_void_p, _c_void_p]),
}


GRAD_READY_FN = ctypes.CFUNCTYPE(None, ctypes.c_void_p, ctypes.c_int)      # csnGradReadyFn(user, layer)


class CsnError(RuntimeError):
    pass


_lib = None


def load():
    """Loads libcsn_hip.so (after torch, so both share one HIP runtime).  Raises if absent."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise CsnError(f"{LIB_PATH} not found: build it with `python -c 'import __graft_entry__ as g; g.build()'` "
                       "(there is no CPU fallback)")
    lib = ctypes.CDLL(LIB_PATH, mode=ctypes.RTLD_LOCAL)
    for name, (res, args) in SIGNATURES.items():
        fn = getattr(lib, name)      # AttributeError if a declared symbol is not exported
        fn.restype, fn.argtypes = res, args
    if lib.csn_abi_version() != ABI_VERSION:
        raise CsnError(f"libcsn_hip.so ABI {lib.csn_abi_version()} != binding ABI {ABI_VERSION}")
    _lib = lib
    return lib


def _check(rc):
    if rc != 0:
        raise CsnError(f"libcsn_hip status {rc}: {load().csn_last_error().decode()}")


def _ptr(t):
    return None if t is None else ctypes.c_void_p(t.data_ptr())


def _stream():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def _dt(dtype):
    if dtype in (torch.float32, "f32", "float32", CSN_F32):
        return CSN_F32
    if dtype in (torch.bfloat16, "bf16", "bfloat16", CSN_BF16):
        return CSN_BF16
    raise CsnError(f"unsupported dtype {dtype}")


def torch_dtype(code):
    return torch.bfloat16 if code == CSN_BF16 else torch.float32


def _need_cuda(*ts):
    for t in ts:
        if t is not None and not t.is_cuda:
            raise CsnError("libcsn_hip needs device tensors (no CPU fallback)")


# ------------------------------------------------------------------------------------------
def eeg_bandpass_znorm(x_bct, sos, ddof=0, out_dtype=torch.float32, time_major=False):
    """x[B,C,T] float32 (device) -> y[B,T,C] or [T,B,C]; sos = [nsec,6] (host array)."""
    import numpy as np
    _need_cuda(x_bct)
    x = x_bct.contiguous()
    if x.dtype != torch.float32:
        raise CsnError("eeg_bandpass_znorm expects float32 input")
    B, C, T = x.shape
    sos = np.ascontiguousarray(np.asarray(sos, dtype=np.float64).reshape(-1, 6)) if sos is not None else np.zeros((0, 6))
    y = torch.empty((T, B, C) if time_major else (B, T, C), dtype=out_dtype, device=x.device)
    with torch.cuda.device(x.device):
        _check(load().csn_eeg_bandpass_znorm(_ptr(x), B, C, T, sos.ctypes.data_as(ctypes.POINTER(ctypes.c_double)),
                                             sos.shape[0], int(ddof), _ptr(y), _dt(out_dtype), int(time_major), _stream()))
    return y


def _stream_rows(x_bct):
    """x[B,C,T] as the stream entry point takes it: the tensor itself where its rows are equally spaced runs of
    consecutive samples (a time slice of a longer [B,C,Ttotal] buffer is), a contiguous copy otherwise."""
    B, C, T = x_bct.shape
    if not (x_bct.stride(2) == 1 and x_bct.stride(0) == C * x_bct.stride(1) and x_bct.stride(1) >= T):
        x_bct = x_bct.contiguous()
    return x_bct, x_bct.stride(1)


def _stream_state(t, name, shape, dtype):
    if t is None:
        return
    _need_cuda(t)
    if t.dtype != dtype or tuple(t.shape) != tuple(shape) or not t.is_contiguous():
        raise CsnError(f"eeg_bandpass_stream: {name} must be a contiguous {dtype} tensor of shape {tuple(shape)}, "
                       f"got {t.dtype} {tuple(t.shape)}")


def eeg_bandpass_stream(x_bct, sos, state_in=None, state_out=None, mean=None, inv_std=None, out_dtype=torch.float32,
                        time_major=False):
    """One piece of a recording through the causal band-pass: x[B,C,T] float32 (device; may be a time slice of a longer
    tensor, no copy) -> (y[B,T,C] or [T,B,C], state_out).  ``state_in`` / ``state_out``: [B,C,nsec,2] float64 on the
    device (``scipy.signal.sosfilt``'s zi with the section axis moved inward); ``state_in=None`` starts a recording,
    ``state_out=None`` allocates the result, and the two may be the same tensor.  ``mean`` / ``inv_std``: optional [C]
    float32, ``y = (filtered - mean) * inv_std``."""
    import numpy as np
    _need_cuda(x_bct)
    if x_bct.dtype != torch.float32:
        raise CsnError("eeg_bandpass_stream expects float32 input")
    if x_bct.dim() != 3:
        raise CsnError(f"eeg_bandpass_stream expects x[B,C,T], got shape {tuple(x_bct.shape)}")
    x, row_stride = _stream_rows(x_bct)
    B, C, T = x.shape
    sos = np.ascontiguousarray(np.asarray(sos, dtype=np.float64).reshape(-1, 6)) if sos is not None else np.zeros((0, 6))
    nsec = sos.shape[0]
    if (mean is None) != (inv_std is None):
        raise CsnError("eeg_bandpass_stream: mean and inv_std are given together or not at all")
    _stream_state(state_in, "state_in", (B, C, nsec, 2), torch.float64)
    _stream_state(mean, "mean", (C,), torch.float32)
    _stream_state(inv_std, "inv_std", (C,), torch.float32)
    if state_out is None:
        state_out = torch.empty((B, C, nsec, 2), dtype=torch.float64, device=x.device)
    _stream_state(state_out, "state_out", (B, C, nsec, 2), torch.float64)
    y = torch.empty((T, B, C) if time_major else (B, T, C), dtype=out_dtype, device=x.device)
    with torch.cuda.device(x.device):
        _check(load().csn_eeg_bandpass_stream(_ptr(x), row_stride, B, C, T, sos.ctypes.data_as(ctypes.POINTER(ctypes.c_double)),
                                              nsec, _ptr(state_in), _ptr(state_out), _ptr(mean), _ptr(inv_std), _ptr(y),
                                              _dt(out_dtype), int(time_major), _stream()))
    return y, state_out


def eeg_bandpass_stream_path(x_bct, nsec):
    """Which kernel ``eeg_bandpass_stream`` runs for this piece: 1 = tile-walking scan, 0 = stateful row-walking."""
    x, row_stride = _stream_rows(x_bct)
    B, C, T = x.shape
    return load().csn_eeg_bandpass_stream_path(_ptr(x), row_stride, C, T, int(nsec))


def eeg_filtfilt(x_stc, sos):
    """Zero-phase band-pass of eeg[S,T,C] float32 (device); sos = [nsec,6] host array."""
    import numpy as np
    _need_cuda(x_stc)
    x = x_stc.float().contiguous()
    S, T, C = x.shape
    sos = np.ascontiguousarray(np.asarray(sos, dtype=np.float64).reshape(-1, 6))
    lib = load()
    scratch = torch.empty(max(1, lib.csn_eeg_filtfilt_scratch_bytes(S, T, C, sos.shape[0])), dtype=torch.uint8,
                          device=x.device)
    y = torch.empty_like(x)
    with torch.cuda.device(x.device):
        _check(lib.csn_eeg_filtfilt(_ptr(x), S, T, C, sos.ctypes.data_as(ctypes.POINTER(ctypes.c_double)), sos.shape[0],
                                    _ptr(y), _ptr(scratch), _stream()))
    return y


def gemm_nt(a, bt, bias=None, out_dtype=torch.float32, out=None, accumulate=False):
    _need_cuda(a, bt)
    a, bt = a.contiguous(), bt.contiguous()
    M, K = a.shape
    N = bt.shape[0]
    assert bt.shape[1] == K and a.dtype == bt.dtype
    c = out if out is not None else torch.empty((M, N), dtype=out_dtype, device=a.device)
    _check(load().csn_gemm_nt(_ptr(a), _ptr(bt), _ptr(bias), _ptr(c), M, N, K, _dt(a.dtype), _dt(c.dtype),
                              int(accumulate), _stream()))
    return c


def gemm_nt_w4_offsets_fit(M, N, K):
    """True where csn_gemm_nt's four-wave 256 x 192 kernel can address A[M, K] and Bt[N, K] with its 32-bit offsets (host
    only).  Bound on use, not in SIGNATURES: an older library given through CSN_LIB_PATH for an A/B run still loads."""
    fn = load().csn_gemm_nt_w4_offsets_fit
    fn.restype, fn.argtypes = _c_int, [_c_i64, _c_i64, _c_i64]
    return bool(fn(M, N, K))


def gemm_nt_w4_lds_bytes():
    """Dynamic LDS bytes of a launch of the four-wave 256 x 192 kernel (host only; bound on use as above)."""
    fn = load().csn_gemm_nt_w4_lds_bytes
    fn.restype, fn.argtypes = _c_int, []
    return int(fn())


# the values of NtRoute (csrc/gemm_nt.hip) and TnRoute (csrc/gemm_tn.hip): TN as (route, kernel behind it)
GEMM_NT_ROUTES = ("generic", "bf16", "dma", "tile256x128", "wide192", "wide256", "wide192w4")
GEMM_TN_ROUTES = (("generic", "generic"), ("tile128", "tn128"), ("tile128", "tn128-notr"), ("tile256", "ring3"),
                  ("tile256", "ring4"), ("tile256", "ring5"), ("tile256", "w4-128"), ("tile256", "w4-256"))


def gemm_nt_route(M, N, K, dtype=torch.bfloat16, aligned16=True):
    """The kernel csn_gemm_nt takes for this shape under the current environment's switches, one of GEMM_NT_ROUTES (host
    only; bound on use as gemm_nt_w4_offsets_fit).  aligned16: A, Bt, C and bias are all 16-byte aligned."""
    fn = load().csn_gemm_nt_route
    fn.restype, fn.argtypes = _c_int, [_c_i64, _c_i64, _c_i64, _c_int, _c_int]
    return GEMM_NT_ROUTES[fn(M, N, K, _dt(dtype), int(aligned16))]


def gemm_tn_route(M, N, K, dtype=torch.bfloat16, aligned16=True, colsum=False):
    """(route, kernel) the weight-gradient GEMM takes, one of GEMM_TN_ROUTES (host only; bound on use).  colsum: the caller
    asks for the column sums of A as well (the LSTM's bias gradient)."""
    fn = load().csn_gemm_tn_route
    fn.restype, fn.argtypes = _c_int, [_c_i64, _c_i64, _c_i64, _c_int, _c_int, _c_int]
    return GEMM_TN_ROUTES[fn(M, N, K, _dt(dtype), int(aligned16), int(colsum))]


def gemm_tn(a_km, b_kn):
    _need_cuda(a_km, b_kn)
    a, b = a_km.contiguous(), b_kn.contiguous()
    K, M = a.shape
    N = b.shape[1]
    assert b.shape[0] == K and a.dtype == b.dtype
    lib = load()
    scratch = torch.empty(max(1, lib.csn_gemm_tn_scratch_bytes(M, N, K)), dtype=torch.uint8, device=a.device)
    c = torch.empty((M, N), dtype=torch.float32, device=a.device)
    _check(lib.csn_gemm_tn(_ptr(a), _ptr(b), _ptr(c), M, N, K, _dt(a.dtype), _ptr(scratch), _stream()))
    return c


def lstm_cell_forward(h_prev, w_hh, xproj, c_prev, want_gates=True):
    _need_cuda(w_hh, xproj)
    B, G = xproj.shape
    H = G // 4
    dt = w_hh.dtype
    gates = torch.empty((B, G), dtype=dt, device=xproj.device) if want_gates else None
    c_out = torch.empty((B, H), dtype=torch.float32, device=xproj.device)
    h_out = torch.empty((B, H), dtype=dt, device=xproj.device)
    _check(load().csn_lstm_cell_forward(_ptr(h_prev), _ptr(w_hh), _ptr(xproj), G, _ptr(c_prev), _ptr(gates),
                                        _ptr(c_out), _ptr(h_out), B, H, _dt(dt), _stream()))
    return h_out, c_out, gates


def lstm_cell_backward(dgates_next, w_hh_t, dy, gates, c, c_prev, dc_carry):
    _need_cuda(gates, c, dc_carry)
    B, G = gates.shape
    H = G // 4
    out = torch.empty_like(gates)
    _check(load().csn_lstm_cell_backward(_ptr(dgates_next), _ptr(w_hh_t), _ptr(dy), H, _ptr(gates), _ptr(c),
                                         _ptr(c_prev), _ptr(dc_carry), _ptr(out), B, H, _dt(gates.dtype), _stream()))
    return out


def _ptr_array(tensors):
    arr = (ctypes.c_void_p * len(tensors))()
    for i, t in enumerate(tensors):
        arr[i] = t.data_ptr()
    return arr


READOUT_LAST, READOUT_MEAN, READOUT_MAX = 0, 1, 2      # csn_lstm_plan_set_readout (include/csn_hip.h)
READOUTS = {"last": READOUT_LAST, "mean": READOUT_MEAN, "max": READOUT_MAX}


def readout_mode(readout):
    """"last" / "mean" / "max" (or a READOUT_* integer) -> the mode of csn_lstm_plan_set_readout; anything else is refused."""
    if isinstance(readout, str) and readout in READOUTS:
        return READOUTS[readout]
    if isinstance(readout, int) and not isinstance(readout, bool) and readout in READOUTS.values():
        return readout
    raise CsnError(f"LSTM readout must be one of {sorted(READOUTS)}, got {readout!r}")


class LstmPlan:
    """One stacked-LSTM problem: a native plan handle (csn_lstm_plan_create: layout, switches, side streams, events
    -- all per plan, the library has no global state) + one workspace; forward()/backward() enqueue on the
    current stream."""

    def __init__(self, B, T, I, H, L, dtype, device, training=True, state=False, dropout=False, reverse=False,
                 resident=False):
        """state=True: a CSN_LSTM_STATE plan, which takes the state keywords of forward() / backward() (and runs the
        per-step cell kernels, path 0 or 1).  dropout=True: a CSN_LSTM_DROPOUT plan, whose workspace holds the dropped
        layer outputs and which takes set_dropout(p > 0).  reverse=True: a CSN_LSTM_REVERSE plan, which walks every
        row backwards in time from its own last valid step (the reverse direction of a bidirectional layer).
        resident=True: a CSN_LSTM_RESIDENT plan (H <= 128), which runs the steps of a chunk inside one launch per layer
        (path 5) with the workspace and, bit for bit, the results of the per-step cells (path 0)."""
        self.desc = LstmDesc(B, T, I, H, L, _dt(dtype))
        self.training = bool(training)
        self.state = bool(state)
        self.dropout = bool(dropout)
        self.reverse = bool(reverse)
        self.resident = bool(resident)
        self._io = (0, 0, False)
        self._views = None          # (src_rows, src_T) while input windows are set (set_views)
        self.device = torch.device(device)
        lib = load()
        handle = _c_void_p()
        with torch.cuda.device(self.device):
            _check(lib.csn_lstm_plan_create(ctypes.byref(self.desc), int(self.training) | (LSTM_STATE if self.state else 0) |
                                            (LSTM_DROPOUT if self.dropout else 0) | (LSTM_REVERSE if self.reverse else 0) |
                                            (LSTM_RESIDENT if self.resident else 0),
                                            ctypes.byref(handle)))
        self._plan = handle
        nbytes = lib.csn_lstm_plan_workspace_bytes(self._plan)
        self.workspace = torch.empty(nbytes + 256, dtype=torch.uint8, device=self.device)
        off = (-self.workspace.data_ptr()) % 256
        self._ws_ptr = ctypes.c_void_p(self.workspace.data_ptr() + off)
        self.busy = False
        with torch.cuda.device(self.device):      # torch.empty memory: status word, zero initial state, ...
            _check(lib.csn_lstm_workspace_init(self._plan, self._ws_ptr, _stream()))

    def __del__(self):
        plan, self._plan = getattr(self, "_plan", None), None
        if plan and _lib is not None:
            _lib.csn_lstm_plan_destroy(plan)

    def key(self):
        d = self.desc
        return ((d.B, d.T, d.I, d.H, d.L, d.dtype, self.training) + ((True,) if self.state else ()) +
                (("dropout plan",) if self.dropout else ()) + (("reverse plan",) if self.reverse else ()) +
                (("resident plan",) if getattr(self, "resident", False) else ()))

    def path(self):
        """0 generic cells, 1 per-diagonal bf16 launches, 2 weight-stationary forward, 3 + weight-stationary backward, 4 the
        exact-float32 path's weight-stationary recurrence, 5 the CU-resident recurrence of a resident=True plan."""
        return load().csn_lstm_plan_path(self._plan)

    def kernel_names(self):
        """(forward, backward) recurrence kernel of this plan's path, as a rocprofv3 kernel trace names them."""
        lib = load()
        return tuple((lib.csn_lstm_plan_kernel_name(self._plan, k) or b"").decode() for k in (0, 1))

    def set_grad_callback(self, fn):
        """fn(layer) is called on this thread from inside backward() once layer's gradient kernels are enqueued (top layer
        first); None removes it.  The ctypes thunk is kept alive by the plan."""
        if getattr(self, "_grad_cb_fn", None) is fn and (fn is None or getattr(self, "_grad_cb", None) is not None):
            return                                  # unchanged since the last backward: keep the installed thunk
        self._grad_cb_fn = fn
        self._grad_cb = GRAD_READY_FN(lambda _user, layer: fn(int(layer))) if fn is not None else None
        _check(load().csn_lstm_plan_set_grad_callback(self._plan, ctypes.cast(self._grad_cb, _c_void_p) if fn is not None
                                                      else None, None))

    def set_grad_mode(self, accumulate):
        """accumulate=True: later backward() calls ADD the weight / bias gradients to what their tensors hold (every
        element becomes fl32(prev + g), g the value the overwriting mode stores: the bits of ``p.grad += g``); False (the
        plan's default): they overwrite.  Sticky until set again."""
        _check(load().csn_lstm_plan_set_grad_mode(self._plan, GRAD_ACCUMULATE if accumulate else GRAD_OVERWRITE))

    def set_lengths(self, lengths):
        """Per-row numbers of valid steps for the following forward() / backward() calls (csn_lstm_plan_set_lengths):
        a sequence of B ints in [0, T] (or a CPU int tensor), or None = every row is T.  Sticky until set again; a
        backward must run with the lengths of its forward.  Needs a plan created with state=True."""
        if lengths is None:
            _check(load().csn_lstm_plan_set_lengths(self._plan, None))
            return
        vals = [int(v) for v in (lengths.tolist() if isinstance(lengths, torch.Tensor) else lengths)]
        if len(vals) != self.desc.B:
            raise CsnError(f"LSTM lengths: {len(vals)} entries for a batch of {self.desc.B}")
        _check(load().csn_lstm_plan_set_lengths(self._plan, (ctypes.c_int32 * len(vals))(*vals)))

    def set_views(self, rows, starts=None, src_rows=None, src_T=None):
        """Input windows of the following forward() calls (csn_lstm_plan_set_views): row b of the LSTM batch is row
        ``rows[b]`` of a source tensor [src_rows, src_T, I] from step ``starts[b]`` on, for lengths[b] steps (T without
        lengths); forward() then takes that source tensor, whatever its strides, instead of a [B, T, I] input, and reads
        nothing past a row's window.  Two sequences of B ints (or CPU int tensors); ``set_views(None)`` turns windows
        off.  Sticky until set again.  Every result has the bits of the call on the gathered dense rows."""
        if rows is None:
            _check(load().csn_lstm_plan_set_views(self._plan, None, None, 0, 0))
            self._views = None
            return
        r = [int(v) for v in (rows.tolist() if isinstance(rows, torch.Tensor) else rows)]
        t = [int(v) for v in (starts.tolist() if isinstance(starts, torch.Tensor) else starts)]
        if len(r) != self.desc.B or len(t) != self.desc.B:
            raise CsnError(f"LSTM views: {len(r)} rows and {len(t)} starts for a batch of {self.desc.B}")
        _check(load().csn_lstm_plan_set_views(self._plan, (ctypes.c_int32 * len(r))(*r), (ctypes.c_int32 * len(t))(*t),
                                              int(src_rows), int(src_T)))
        self._views = (int(src_rows), int(src_T))

    def set_io(self, y_all_pitch=0, dy_all_pitch=0, dx_add=False):
        """Where the following calls find y_all / dy_all and how they store dx (csn_lstm_plan_set_io).  A pitch is the
        number of elements per (b, t) row, 0 = dense (H): forward(y_all=view) then writes, and backward(dy_all=view) reads,
        a [B,T,H] view of a wider tensor in place -- one half of a [B,T,2H] buffer.  dx_add=True: backward ADDS the input
        gradient to dx over the valid steps.  Sticky until set again."""
        _check(load().csn_lstm_plan_set_io(self._plan, int(y_all_pitch), int(dy_all_pitch), int(bool(dx_add))))
        self._io = (int(y_all_pitch), int(dy_all_pitch), bool(dx_add))

    def set_readout(self, mode):
        """What y_last of the following forward() calls is and where dy_last of the following backward() calls enters
        (csn_lstm_plan_set_readout): "last" (the default), "mean" or "max" over each row's valid steps, or the
        READOUT_* integer.  Sticky until set again; a backward must run with the setting of its forward."""
        _check(load().csn_lstm_plan_set_readout(self._plan, readout_mode(mode)))

    def set_attention(self, q=None, scale=None, dq=None, attn_out=None, dscore_out=None):
        """The attention readout of the following forward() / backward() calls (csn_lstm_plan_set_attention): with a query
        ``q`` ([H] float32 on the device) y_last is the weighted mean over each row's valid steps under the weights
        softmax_t(scale <h_t, q>) (scale: H ** -0.5 unless given), whatever set_readout says, and backward() takes
        dy_last as its gradient.  dq: [H] float32 that backward() writes the query's gradient into (added to after
        set_grad_mode(True)), or None for a frozen query.  attn_out / dscore_out: dense [B,T] float32 tensors that
        receive the weights (forward and backward) and the score gradients (backward), or None.  ``set_attention()``
        turns it off.  Sticky until set again; the tensors must stay alive while the setting is in use, and a backward
        must run with the setting of its forward."""
        d = self.desc
        if q is None:
            if dq is not None or attn_out is not None or dscore_out is not None:
                raise CsnError("LSTM attention: dq, attn_out or dscore_out without a query")
            _check(load().csn_lstm_plan_set_attention(self._plan, None, 0.0, None, None, None))
            return
        for t, shape, name in ((q, (d.H,), "q"), (dq, (d.H,), "dq"), (attn_out, (d.B, d.T), "attn_out"),
                               (dscore_out, (d.B, d.T), "dscore_out")):
            if t is None:
                continue
            _need_cuda(t)
            if t.dtype != torch.float32 or tuple(t.shape) != shape or not t.is_contiguous():
                raise CsnError(f"LSTM attention {name}: a dense float32 tensor of shape {list(shape)} is needed, got "
                               f"{t.dtype} {list(t.shape)}")
        scale = float(d.H) ** -0.5 if scale is None else float(scale)
        _check(load().csn_lstm_plan_set_attention(self._plan, _ptr(q.detach()), scale, _ptr(dq), _ptr(attn_out),
                                                  _ptr(dscore_out)))

    def _pitched(self, t, pitch, name):
        """t must be a float32 [B,T,H] device view with strides (T * pitch, pitch, 1), 16-byte aligned."""
        d = self.desc
        _need_cuda(t)
        pitch = pitch or d.H
        if (t.dtype != torch.float32 or tuple(t.shape) != (d.B, d.T, d.H) or t.stride() != (d.T * pitch, pitch, 1)
                or t.data_ptr() % 16):
            raise CsnError(f"LSTM {name}: a float32 [B,T,H] view with pitch {pitch} is needed, got {t.dtype} "
                           f"{tuple(t.shape)} strides {t.stride()}")
        return t

    def set_dropout(self, p, seed=0, subsequence=0):
        """Inter-layer dropout of the following forward() / backward() calls (csn_lstm_plan_set_dropout): probability p
        in [0, 1] (0 = off), a 64-bit seed and a 32-bit subsequence (e.g. the data-parallel rank).  Sticky until set
        again; a backward must run with the setting of its forward.  p > 0 needs a plan created with dropout=True."""
        _check(load().csn_lstm_plan_set_dropout(self._plan, float(p), int(seed) & 0xFFFFFFFFFFFFFFFF,
                                                int(subsequence) & 0xFFFFFFFF))

    def set_output_dropout(self, p, seed=0, subsequence=0, first=0, index_pitch=0):
        """Dropout on y_all as the following forward() calls store it and on dy_all as the following backward() calls read
        it (csn_lstm_plan_set_output_dropout): element (b, t, h) is kept iff ``lstm_dropout_keep(seed, subsequence, p,
        first + (b * T + t) * index_pitch + h, 1)``, t the caller's time also on a reverse plan, and a kept element is
        scaled by 1 / (1 - p).  p = 0 = off.  Sticky until set again; a backward must run with the setting of its forward.
        With p > 0: first and index_pitch multiples of 4, index_pitch >= H."""
        _check(load().csn_lstm_plan_set_output_dropout(self._plan, float(p), int(seed) & 0xFFFFFFFFFFFFFFFF,
                                                       int(subsequence) & 0xFFFFFFFF, int(first), int(index_pitch)))

    def dgates_copies(self):
        """Copies of the gate gradients the last backward wrote per step (csn_hip.h): 2, or 0 before any backward."""
        return load().csn_lstm_plan_dgates_copies(self._plan)

    def half_tile_launches(self, which):
        """Recurrence launches of the last forward (which = 0) / backward (which = 1) that ran on 32-row hand-off groups
        (csn_hip.h); 0 under CSN_NO_HALF_TILES=1."""
        return load().csn_lstm_plan_half_tile_launches(self._plan, which)

    def bwd_launches(self, which):
        """Recurrence launches of the last weight-stationary backward (which = 0) and the chunk diagonals its merged
        launch covered (which = 1; 0: none merged, e.g. under CSN_BWD_NO_MERGE=1) (csrc/lstm.hip).  Bound on use, not in
        SIGNATURES: an older library given through CSN_LIB_PATH for an A/B run still loads."""
        fn = load().csn_lstm_plan_bwd_launches
        fn.restype, fn.argtypes = _c_int, [_c_void_p, _c_int]
        return int(fn(self._plan, which))

    def forward(self, x_bti, w_ih, w_hh, b_ih, b_hh, want_all=False, h0=None, c0=None, want_state=False, y_all=None,
                state_out=None):
        """-> (y_last, y_all); with want_state=True -> (y_last, y_all, h_n, c_n).  With input windows set (set_views)
        x_bti is the SOURCE [src_rows, src_T, I], passed with its own strides.  h0 / c0: [L,B,H] initial state or
        None (zeros); the state keywords need a plan created with state=True.  y_all: a [B,T,H] view to write every step
        into (its pitch set with set_io) instead of a new tensor.  state_out: (h_n, c_n), dense float32 [L,B,H] tensors (or
        slices of larger ones) to write the final state into, with want_state=True."""
        d = self.desc
        _need_cuda(x_bti)
        if x_bti.dtype != torch.float32 or x_bti.stride(2) != 1:
            x_bti = x_bti.float().contiguous()
        want = (d.B, d.T, d.I) if self._views is None else self._views + (d.I,)
        assert x_bti.shape == want, (tuple(x_bti.shape), want)
        y_last = torch.empty((d.B, d.H), dtype=torch.float32, device=x_bti.device)
        if y_all is not None:
            y_all = self._pitched(y_all, self._io[0], "y_all")
        elif want_all:
            if self._io[0]:
                raise CsnError("LSTM y_all: the plan has a y_all pitch set (set_io): pass the view to write into")
            y_all = torch.empty((d.B, d.T, d.H), dtype=torch.float32, device=x_bti.device)
        ws = [[p.detach() for p in group] for group in (w_ih, w_hh, b_ih, b_hh)]
        for group in ws:
            for p in group:
                assert p.dtype == torch.float32 and p.is_contiguous() and p.is_cuda
        h0, c0 = self._state_in(h0), self._state_in(c0)
        if want_state and state_out is not None:
            h_n, c_n = state_out
            for out in state_out:
                assert out.dtype == torch.float32 and out.is_contiguous() and out.shape == (d.L, d.B, d.H) and out.is_cuda
        else:
            h_n = torch.empty((d.L, d.B, d.H), dtype=torch.float32, device=x_bti.device) if want_state else None
            c_n = torch.empty((d.L, d.B, d.H), dtype=torch.float32, device=x_bti.device) if want_state else None
        with torch.cuda.device(self.device):
            _check(load().csn_lstm_forward(self._plan, _ptr(x_bti), x_bti.stride(0), x_bti.stride(1),
                                           _ptr_array(ws[0]), _ptr_array(ws[1]), _ptr_array(ws[2]), _ptr_array(ws[3]),
                                           _ptr(h0), _ptr(c0), self._ws_ptr, _ptr(y_last), _ptr(y_all),
                                           _ptr(h_n), _ptr(c_n), _stream()))
        if want_state:
            return y_last, y_all, h_n, c_n
        return y_last, y_all

    def _state_in(self, t):
        """[L,B,H] state / state gradient -> dense float32 on the plan's device (None stays None)."""
        if t is None:
            return None
        d = self.desc
        t = t.detach()
        if tuple(t.shape) != (d.L, d.B, d.H):
            raise CsnError(f"LSTM state must be [L, B, H] = {[d.L, d.B, d.H]}, got {list(t.shape)}")
        return t.to(device=self.device, dtype=torch.float32).contiguous()

    def backward(self, dy_last, dy_all, grads, dx=None, dh_n=None, dc_n=None, dh0=None, dc0=None):
        """grads: 4 lists (dw_ih, dw_hh, db_ih, db_hh) of float32 device tensors: overwritten, or added to after
        set_grad_mode(True) -- the mode governs these four groups only.  dx and dh0 / dc0 ([L,B,H] float32 outputs, or
        None) are overwritten in both modes.  dh_n / dc_n: [L,B,H] incoming gradients of the final state or None."""
        if dy_last is not None:
            dy_last = dy_last.float().contiguous()
        if dy_all is not None:
            dy_all = self._pitched(dy_all, self._io[1], "dy_all") if self._io[1] else dy_all.float().contiguous()
        dh_n, dc_n = self._state_in(dh_n), self._state_in(dc_n)
        for out in (dh0, dc0):
            if out is not None:
                assert out.dtype == torch.float32 and out.is_contiguous() and out.shape == (self.desc.L, self.desc.B,
                                                                                            self.desc.H)
        with torch.cuda.device(self.device):
            _check(load().csn_lstm_backward(self._plan, _ptr(dy_last), _ptr(dy_all), _ptr(dh_n), _ptr(dc_n), self._ws_ptr,
                                            _ptr_array(grads[0]), _ptr_array(grads[1]), _ptr_array(grads[2]),
                                            _ptr_array(grads[3]), _ptr(dx), _ptr(dh0), _ptr(dc0), _stream()))

    # ---- sticky status word of the workspace ------------------------------------------------------
    def clear_status(self):
        with torch.cuda.device(self.device):
            _check(load().csn_lstm_status_clear(self._plan, self._ws_ptr, _stream()))

    def inject_timeout(self):
        """Test hook: leaves the status word as a timed-out in-kernel wait would."""
        with torch.cuda.device(self.device):
            _check(load().csn_lstm_status_raise(self._plan, self._ws_ptr, _stream()))

    def status(self, clear=False):
        """Blocking: 0 if every in-kernel hand-off since the last clear completed; bit STATUS_TIMEOUT = a bounded wait
        gave up, bit STATUS_NONFINITE = a NaN / Inf gradient reached the backward (the word is sticky: an event in ANY
        forward / backward since the last clear keeps it raised)."""
        out = _c_int(0)
        _check(load().csn_lstm_status_read(self._plan, self._ws_ptr, ctypes.byref(out)))
        if clear and out.value != 0:
            self.clear_status()
        return out.value

    # ---- per-plan event timing of the recurrence launches -----------------------------------------
    def profile_enable(self, on=True):
        _check(load().csn_lstm_profile_enable(self._plan, int(on)))

    def profile_read(self):
        """-> dict(fwd_ms, fwd_launches, fwd_cells, bwd_ms, bwd_launches, bwd_cells) of the last fwd/bwd."""
        fm, bm = ctypes.c_double(), ctypes.c_double()
        fl, fc, bl, bc = _c_int(), _c_int(), _c_int(), _c_int()
        _check(load().csn_lstm_profile_read(self._plan, ctypes.byref(fm), ctypes.byref(fl), ctypes.byref(fc),
                                            ctypes.byref(bm), ctypes.byref(bl), ctypes.byref(bc)))
        return dict(fwd_ms=fm.value, fwd_launches=fl.value, fwd_cells=fc.value,
                    bwd_ms=bm.value, bwd_launches=bl.value, bwd_cells=bc.value)


def lstm_dropout_keep(seed, subsequence, p, first, n):
    """The dropout mask of csn_lstm_plan_set_dropout(p, seed, subsequence) for the elements first .. first + n - 1
    (e = ((l T + t) B + b) H + u) as a numpy uint8 array, 1 = kept.  Host code: needs no GPU."""
    import numpy as np
    keep = np.empty(int(n), dtype=np.uint8)
    _check(load().csn_lstm_dropout_keep(int(seed) & 0xFFFFFFFFFFFFFFFF, int(subsequence) & 0xFFFFFFFF, float(p), int(first),
                                        int(n), keep.ctypes.data_as(_c_void_p)))
    return keep


def cosine_loss(student, teacher, want_grad=True, grad_scale=1.0):
    _need_cuda(student, teacher)
    s, t = student.float().contiguous(), teacher.float().contiguous()
    B, D = s.shape
    loss = torch.empty(1, dtype=torch.float32, device=s.device)
    ds = torch.empty_like(s) if want_grad else None
    lib = load()
    scratch = torch.empty(lib.csn_cosine_loss_scratch_bytes(B) // 8, dtype=torch.float64, device=s.device)   # caller-owned
    with torch.cuda.device(s.device):
        _check(lib.csn_cosine_loss(_ptr(s), _ptr(t), B, D, _ptr(loss), _ptr(ds), float(grad_scale), _ptr(scratch), _stream()))
    return loss, ds


SOFT_KL, SOFT_CE_OF_PROBS = 0, 1            # csn_distill_loss soft_mode (include/csn_hip.h)
DINO_SKIP_FIRST, DINO_SKIP_SAME = 0, 1      # csn_dino_loss pairing (include/csn_hip.h)


def _f32_rows(t, name, ndim):
    if t.dtype != torch.float32 or t.dim() != ndim:
        raise CsnError(f"{name}: expected a float32 tensor of {ndim} dimensions, got {t.dtype} {tuple(t.shape)}")
    return t.contiguous()


def distill_loss(student, teacher, soft_mode, T, w_soft, logits=None, labels=None, w_ce=0.0, want_grad=True,
                 grad_scale=1.0):
    """csn_distill_loss on student / teacher [B,D] float32 -> (loss[1], dstudent | None, dlogits | None).
    ``logits`` may be ``student`` itself (the alias: K == D; the CE gradient is then part of dstudent and dlogits is None).
    ``want_grad``: a bool for both gradients or a pair (dstudent, dlogits)."""
    _need_cuda(student, teacher, logits, labels)
    alias = logits is student
    s, t = _f32_rows(student, "student", 2), _f32_rows(teacher, "teacher", 2)
    B, D = s.shape
    if t.shape != s.shape:
        raise CsnError(f"distill_loss: teacher {tuple(t.shape)} against student {tuple(s.shape)}")
    if (logits is None) != (labels is None):
        raise CsnError("distill_loss: logits and labels go together")
    lg, lab, K = None, None, 0
    if logits is not None:
        lg = s if alias else _f32_rows(logits, "logits", 2)
        K = lg.shape[1]
        lab = labels.to(torch.int64).contiguous()
        if lg.shape[0] != B or lab.shape != (B,):
            raise CsnError(f"distill_loss: logits {tuple(lg.shape)} / labels {tuple(lab.shape)} against B = {B}")
    want_ds, want_dl = want_grad if isinstance(want_grad, (tuple, list)) else (want_grad, want_grad)
    loss = torch.empty(1, dtype=torch.float32, device=s.device)
    ds = torch.empty_like(s) if want_ds else None
    dl = torch.empty_like(lg) if (want_dl and lg is not None and not alias) else None
    lib = load()
    scratch = torch.empty(lib.csn_distill_loss_scratch_bytes(B) // 8, dtype=torch.float64, device=s.device)   # caller-owned
    with torch.cuda.device(s.device):
        _check(lib.csn_distill_loss(_ptr(s), _ptr(t), B, D, _ptr(lg), K, _ptr(lab), int(soft_mode), float(T), float(w_soft),
                                    float(w_ce), _ptr(loss), _ptr(ds), _ptr(dl), float(grad_scale), _ptr(scratch), _stream()))
    return loss, ds, dl


def dino_loss(student, teacher, center, teacher_temp, student_temp, pairing, want_grad=True, grad_scale=1.0):
    """csn_dino_loss on student [V,B,D], teacher [G,B,D], center [D] or [B,D] (float32) -> (loss[1], dstudent | None)."""
    _need_cuda(student, teacher, center)
    s, t = _f32_rows(student, "student", 3), _f32_rows(teacher, "teacher", 3)
    V, B, D = s.shape
    G = t.shape[0]
    if t.shape[1:] != s.shape[1:]:
        raise CsnError(f"dino_loss: teacher {tuple(t.shape)} against student {tuple(s.shape)}")
    if center.dtype != torch.float32 or center.numel() not in (D, B * D) or center.shape[-1] != D:
        raise CsnError(f"dino_loss: center {center.dtype} {tuple(center.shape)} is neither [D] nor [B,D] float32")
    c = center.contiguous()
    stride = D if (c.numel() == B * D and c.dim() > 1 and c.shape[-2] == B) else 0
    loss = torch.empty(1, dtype=torch.float32, device=s.device)
    ds = torch.empty_like(s) if want_grad else None
    lib = load()
    scratch = torch.empty(lib.csn_dino_loss_scratch_bytes(B, D) // 8, dtype=torch.float64, device=s.device)   # caller-owned
    with torch.cuda.device(s.device):
        _check(lib.csn_dino_loss(_ptr(s), _ptr(t), V, G, B, D, _ptr(c), stride, float(teacher_temp), float(student_temp),
                                 int(pairing), _ptr(loss), _ptr(ds), float(grad_scale), _ptr(scratch), _stream()))
    return loss, ds


def rmsprop_step(params_flat, grads_flat, square_avg_flat, lr, alpha=0.99, eps=1e-8):
    """In place, on the current stream: one fused pass over the flat float32 buffers."""
    _need_cuda(params_flat, grads_flat, square_avg_flat)
    n = params_flat.numel()
    assert grads_flat.numel() == n and square_avg_flat.numel() == n
    assert params_flat.dtype == grads_flat.dtype == square_avg_flat.dtype == torch.float32
    with torch.cuda.device(params_flat.device):
        _check(load().csn_rmsprop_step(_ptr(params_flat), _ptr(grads_flat), _ptr(square_avg_flat), n, float(lr), float(alpha),
                                       float(eps), _stream()))


# ---- optimiser tails over flat segmented buffers (csrc/optim.hip) ---------------------------------------------------------
class SegmentTable:
    """The device table of csn_flat_segments_prepare for a flat float32 buffer of ``n`` elements cut at ``seg_end``
    (exclusive ends, one per tensor) with per-segment ``flags`` (SEG_DECAYED | SEG_SCALED).  Caller-owned scratch, like
    every other scratch of the library; built once, on the current stream."""

    def __init__(self, seg_end, flags, device):
        device = torch.device(device)
        if device.type != "cuda":
            raise CsnError("libcsn_hip needs device tensors (no CPU fallback)")
        self.seg_end, self.flags = [int(e) for e in seg_end], [int(f) for f in flags]
        self.nseg, self.n = len(self.seg_end), (self.seg_end[-1] if self.seg_end else 0)
        if len(self.flags) != self.nseg:
            raise CsnError(f"SegmentTable: {len(self.flags)} flags for {self.nseg} segments")
        lib = load()
        nbytes = lib.csn_flat_segments_scratch_bytes(self.nseg, self.n)
        if nbytes == 0:
            raise CsnError(f"libcsn_hip: {lib.csn_last_error().decode()}")
        self.buf = torch.empty(nbytes // 8, dtype=torch.float64, device=device)       # (torch allocations are 256-B aligned)
        ends = (ctypes.c_int64 * self.nseg)(*self.seg_end)
        flg = (ctypes.c_int32 * self.nseg)(*self.flags)
        with torch.cuda.device(device):
            _check(lib.csn_flat_segments_prepare(ends, flg, self.nseg, self.n, _ptr(self.buf), _stream()))


def _flat_check(table, *bufs):
    _need_cuda(*bufs)
    for b in bufs:
        if b is not None and (b.dtype != torch.float32 or b.numel() != table.n or not b.is_contiguous()):
            raise CsnError(f"flat buffers must be contiguous float32 of {table.n} elements")


def flat_segment_norms(table, a, b=None, weight_decay=0.0):
    """Per-segment L2 norms of ``a`` ([nseg] float32, device); with ``b`` also of d = b + weight_decay a on decayed
    segments, b elsewhere ([2, nseg]).  Deterministic: two runs give the same bits."""
    _flat_check(table, a, b)
    out = torch.empty((2, table.nseg) if b is not None else (table.nseg,), dtype=torch.float32, device=a.device)
    with torch.cuda.device(a.device):
        _check(load().csn_flat_segment_norms(_ptr(a), _ptr(b), float(weight_decay), table.n, table.nseg, _ptr(table.buf),
                                             _ptr(out), _stream()))
    return out


def flat_clip(table, grads, clip):
    """grads_s <- min(1, clip / (|grads_s| + 1e-6)) grads_s in place; returns the pre-clip norms ([nseg], device)."""
    _flat_check(table, grads)
    out = torch.empty(table.nseg, dtype=torch.float32, device=grads.device)
    with torch.cuda.device(grads.device):
        _check(load().csn_flat_clip(_ptr(grads), table.n, table.nseg, _ptr(table.buf), float(clip), _ptr(out), _stream()))
    return out


def adam_step(table, params, grads, exp_avg, exp_avg_sq, step, lr, beta1, beta2, eps, weight_decay, decoupled, clip=None,
              norms_out=None):
    """One fused Adam / AdamW step in place on the current stream (csn_adam_step); ``clip``: per-tensor clip of the
    gradient used by the step (``grads`` itself is not written), pre-clip norms into ``norms_out``."""
    _flat_check(table, params, grads, exp_avg, exp_avg_sq)
    _need_cuda(norms_out)
    with torch.cuda.device(params.device):
        _check(load().csn_adam_step(_ptr(params), _ptr(grads), _ptr(exp_avg), _ptr(exp_avg_sq), table.n, table.nseg,
                                    _ptr(table.buf), int(step), float(lr), float(beta1), float(beta2), float(eps),
                                    float(weight_decay), int(bool(decoupled)), float(clip or 0.0), _ptr(norms_out), _stream()))


def lars_step(table, params, grads, mu, lr, weight_decay, momentum, eta):
    """One fused LARS step in place on the current stream (csn_lars_step: the norm pass and the update)."""
    _flat_check(table, params, grads, mu)
    with torch.cuda.device(params.device):
        _check(load().csn_lars_step(_ptr(params), _ptr(grads), _ptr(mu), table.n, table.nseg, _ptr(table.buf), float(lr),
                                    float(weight_decay), float(momentum), float(eta), _stream()))


# ---- global-norm clip and non-finite skip on the device (csn_grad_guard and the guarded steps) ---------------------------------
class StepGuard:
    """Owner of one csnStepGuard record (16 bytes, zeroed once here) and of the scratch of csn_grad_guard.  ``norm`` and
    ``scale`` are 0-dim float32 DEVICE views into the record (no host read); ``finite`` a 0-dim int32 view;
    ``skipped()`` is one blocking host read of the count of non-finite buffers measured so far."""

    def __init__(self, device):
        device = torch.device(device)
        if device.type != "cuda":
            raise CsnError("libcsn_hip needs device tensors (no CPU fallback)")
        self.device = device
        self.record = torch.zeros(4, dtype=torch.float32, device=device)       # (torch allocations are 256-B aligned)
        self.norm, self.scale = self.record[0], self.record[1]
        words = self.record.view(torch.int32)
        self.finite, self._skipped = words[2], words[3]
        self.scratch, self._n = None, 0

    def measure(self, grads, max_norm=None):
        """Enqueues csn_grad_guard over the contiguous float32 device buffer ``grads`` on the current stream;
        ``max_norm`` None / inf: measure and gate only.  Returns ``self.norm``."""
        _need_cuda(grads)
        if grads.dtype != torch.float32 or not grads.is_contiguous() or grads.device != self.device:
            raise CsnError("StepGuard: the gradient buffer must be contiguous float32 on the guard's device")
        lib, n = load(), grads.numel()
        if self.scratch is None or self._n != n:
            nbytes = lib.csn_grad_guard_scratch_bytes(n)
            if nbytes == 0:
                raise CsnError(f"libcsn_hip: {lib.csn_last_error().decode()}")
            self.scratch, self._n = torch.empty(nbytes // 8, dtype=torch.float64, device=self.device), n
        with torch.cuda.device(self.device):
            _check(lib.csn_grad_guard(_ptr(grads), n, float("inf") if max_norm is None else float(max_norm),
                                      _ptr(self.scratch), _ptr(self.record), _stream()))
        return self.norm

    def skipped(self):
        return int(self._skipped.item())

    def set_skipped(self, count):
        self._skipped.fill_(int(count))


def rmsprop_step_guarded(guard, params_flat, grads_flat, square_avg_flat, lr, alpha=0.99, eps=1e-8):
    """rmsprop_step behind ``guard`` (a StepGuard measured earlier on this stream): the step of scale * g, or nothing."""
    _need_cuda(params_flat, grads_flat, square_avg_flat)
    n = params_flat.numel()
    assert grads_flat.numel() == n and square_avg_flat.numel() == n
    assert params_flat.dtype == grads_flat.dtype == square_avg_flat.dtype == torch.float32
    with torch.cuda.device(params_flat.device):
        _check(load().csn_rmsprop_step_guarded(_ptr(params_flat), _ptr(grads_flat), _ptr(square_avg_flat), n, float(lr),
                                               float(alpha), float(eps), _ptr(guard.record), _stream()))


def adam_step_guarded(guard, table, params, grads, exp_avg, exp_avg_sq, step, lr, beta1, beta2, eps, weight_decay, decoupled,
                      clip=None, norms_out=None):
    """adam_step behind ``guard``; ``step`` counts the calls, skipped ones included; with ``clip`` the per-tensor clip
    works on the globally scaled gradient and ``norms_out`` holds ITS norms (untouched by a skipped step)."""
    _flat_check(table, params, grads, exp_avg, exp_avg_sq)
    _need_cuda(norms_out)
    with torch.cuda.device(params.device):
        _check(load().csn_adam_step_guarded(_ptr(params), _ptr(grads), _ptr(exp_avg), _ptr(exp_avg_sq), table.n, table.nseg,
                                            _ptr(table.buf), int(step), float(lr), float(beta1), float(beta2), float(eps),
                                            float(weight_decay), int(bool(decoupled)), float(clip or 0.0), _ptr(norms_out),
                                            _ptr(guard.record), _stream()))


def lars_step_guarded(guard, table, params, grads, mu, lr, weight_decay, momentum, eta):
    """lars_step behind ``guard``."""
    _flat_check(table, params, grads, mu)
    with torch.cuda.device(params.device):
        _check(load().csn_lars_step_guarded(_ptr(params), _ptr(grads), _ptr(mu), table.n, table.nseg, _ptr(table.buf),
                                            float(lr), float(weight_decay), float(momentum), float(eta), _ptr(guard.record),
                                            _stream()))


def barlow_offdiag_sqsum(c):
    _need_cuda(c)
    if c.dim() != 2 or c.shape[0] != c.shape[1]:
        raise CsnError(f"barlow_offdiag_sqsum expects a square matrix, got shape {tuple(c.shape)}")
    c = c.float().contiguous()
    out = torch.empty(2, dtype=torch.float32, device=c.device)
    with torch.cuda.device(c.device):
        _check(load().csn_barlow_offdiag_sqsum(_ptr(c), c.shape[0], _ptr(out), _stream()))
    return out


def _barlow_pair(z1, z2, who):
    _need_cuda(z1, z2)
    a, b = _f32_rows(z1, "z1", 2), _f32_rows(z2, "z2", 2)
    if a.shape != b.shape or a.device != b.device:
        raise CsnError(f"{who}: z2 {tuple(b.shape)} on {b.device} against z1 {tuple(a.shape)} on {a.device}")
    return a, b


def barlow_corr(z1, z2, batch_size, eps=1e-5, running_mean=None, running_var=None, momentum=0.1):
    """csn_barlow_corr on z1 / z2 [B,D] float32 -> (c [D,D] float64: THIS rank's term, saved [4,D] float64).
    ``batch_size`` is the GLOBAL batch.  ``running_mean`` / ``running_var`` (float32 [D], contiguous, both or neither) are
    updated in place, for z1 and then for z2."""
    a, b = _barlow_pair(z1, z2, "barlow_corr")
    B, D = a.shape
    if (running_mean is None) != (running_var is None):
        raise CsnError("barlow_corr: running_mean and running_var go together")
    for name, r in (("running_mean", running_mean), ("running_var", running_var)):
        if r is not None and (r.dtype != torch.float32 or r.shape != (D,) or not r.is_contiguous() or r.device != a.device):
            raise CsnError(f"barlow_corr: {name} must be a contiguous float32 [{D}] tensor on {a.device}, "
                           f"got {r.dtype} {tuple(r.shape)} on {r.device}")
    lib = load()
    c = torch.empty((D, D), dtype=torch.float64, device=a.device)
    saved = torch.empty((4, D), dtype=torch.float64, device=a.device)       # csn_barlow_saved_bytes(D) bytes, caller-owned
    with torch.cuda.device(a.device):
        _check(lib.csn_barlow_corr(_ptr(a), _ptr(b), B, D, float(eps), 1.0 / float(batch_size), _ptr(c), _ptr(saved),
                                   _ptr(running_mean), _ptr(running_var), float(momentum), _stream()))
    return c, saved


def barlow_grad(z1, z2, c, c_local, saved, batch_size, lambd, grad_scale=1.0, want=(True, True)):
    """csn_barlow_grad -> (loss[1], dz1 | None, dz2 | None).  ``c``: the sum of every rank's term, ``c_local``: this rank's,
    as barlow_corr returned it (the same tensor on one rank); ``want``: which of (dz1, dz2) to compute."""
    a, b = _barlow_pair(z1, z2, "barlow_grad")
    B, D = a.shape
    _need_cuda(c, c_local, saved)
    for name, t, shape in (("c", c, (D, D)), ("c_local", c_local, (D, D)), ("saved", saved, (4, D))):
        if t.dtype != torch.float64 or tuple(t.shape) != shape or not t.is_contiguous() or t.device != a.device:
            raise CsnError(f"barlow_grad: {name} must be a contiguous float64 {list(shape)} tensor on {a.device}, "
                           f"got {t.dtype} {tuple(t.shape)} on {t.device}")
    lib = load()
    loss = torch.empty(1, dtype=torch.float32, device=a.device)
    dz1 = torch.empty_like(a) if want[0] else None
    dz2 = torch.empty_like(b) if want[1] else None
    scratch = torch.empty(lib.csn_barlow_scratch_bytes(B, D) // 8, dtype=torch.float64, device=a.device)     # caller-owned
    with torch.cuda.device(a.device):
        _check(lib.csn_barlow_grad(_ptr(a), _ptr(b), B, D, _ptr(c), _ptr(c_local), _ptr(saved), 1.0 / float(batch_size),
                                   float(lambd), float(grad_scale), _ptr(loss), _ptr(dz1), _ptr(dz2), _ptr(scratch), _stream()))
    return loss, dz1, dz2


def _contrastive_inputs(s_all, t_all, group_all, row0, B, who):
    _need_cuda(s_all, t_all, group_all)
    s, t = _f32_rows(s_all, "s_all", 2), _f32_rows(t_all, "t_all", 2)
    if s.shape != t.shape or s.device != t.device:
        raise CsnError(f"{who}: t_all {tuple(t.shape)} on {t.device} against s_all {tuple(s.shape)} on {s.device}")
    N, D = s.shape
    if group_all is not None:
        if group_all.dtype != torch.int32 or tuple(group_all.shape) != (N,) or group_all.device != s.device:
            raise CsnError(f"{who}: group_all must be an int32 [{N}] tensor on {s.device}, got {group_all.dtype} "
                           f"{tuple(group_all.shape)} on {group_all.device}")
        group_all = group_all.contiguous()
    B = N - row0 if B is None else B
    return s, t, group_all, N, D, int(B)


def _contrastive_scratch(lib, B, N, D, device):
    return torch.empty(lib.csn_contrastive_scratch_bytes(B, N, D) // 8, dtype=torch.float64, device=device)       # caller-owned


def contrastive_lse(s_all, t_all, logit_scale, group_all=None, row0=0, B=None, w_a=0.5, w_b=0.5):
    """csn_contrastive_lse on the gathered rows s_all / t_all [N,D] float32 (group_all: int32 [N] or None) for the local rows
    row0 .. row0+B-1 (default: all from row0 on) -> (rows_out [3,B] float64: lA, lB, p; loss_part [1] float64: the local
    rows' part of the global loss)."""
    s, t, g, N, D, B = _contrastive_inputs(s_all, t_all, group_all, row0, B, "contrastive_lse")
    lib = load()
    rows_out = torch.empty((3, max(B, 0)), dtype=torch.float64, device=s.device)
    loss_part = torch.empty(1, dtype=torch.float64, device=s.device)
    scratch = _contrastive_scratch(lib, B, N, D, s.device)
    with torch.cuda.device(s.device):
        _check(lib.csn_contrastive_lse(_ptr(s), _ptr(t), _ptr(g), N, D, int(row0), B, float(logit_scale), float(w_a),
                                       float(w_b), _ptr(rows_out), _ptr(loss_part), _ptr(scratch), _stream()))
    return rows_out, loss_part


def contrastive_grad(s_all, t_all, logit_scale, lse_a_local, lse_b_all, group_all=None, row0=0, B=None, w_a=0.5, w_b=0.5,
                     grad_scale=1.0, want_dscale=False):
    """csn_contrastive_grad -> (ds [B,D] float32, holding grad_scale; dscale_part [1] float64 | None: the local rows' part
    of dL/d logit_scale).  ``lse_a_local`` [B] and ``lse_b_all`` [N] float64: rows 0 and 1 of contrastive_lse's rows_out on
    one rank, lB all-gathered in rank order on several."""
    s, t, g, N, D, B = _contrastive_inputs(s_all, t_all, group_all, row0, B, "contrastive_grad")
    _need_cuda(lse_a_local, lse_b_all)
    for name, v, n in (("lse_a_local", lse_a_local, B), ("lse_b_all", lse_b_all, N)):
        if v.dtype != torch.float64 or tuple(v.shape) != (n,) or not v.is_contiguous() or v.device != s.device:
            raise CsnError(f"contrastive_grad: {name} must be a contiguous float64 [{n}] tensor on {s.device}, "
                           f"got {v.dtype} {tuple(v.shape)} on {v.device}")
    lib = load()
    ds = torch.empty((max(B, 0), D), dtype=torch.float32, device=s.device)
    dscale = torch.empty(1, dtype=torch.float64, device=s.device) if want_dscale else None
    scratch = _contrastive_scratch(lib, B, N, D, s.device)
    with torch.cuda.device(s.device):
        _check(lib.csn_contrastive_grad(_ptr(s), _ptr(t), _ptr(g), N, D, int(row0), B, float(logit_scale), _ptr(lse_a_local),
                                        _ptr(lse_b_all), float(w_a), float(w_b), float(grad_scale), _ptr(ds), _ptr(dscale),
                                        _ptr(scratch), _stream()))
    return ds, dscale


def bank_norms(bank):
    """csn_bank_norms on bank [M,D] float32 -> inv_norm [M] float64 = 1 / max(|t_m|, 1e-12); once per bank."""
    _need_cuda(bank)
    b = _f32_rows(bank, "bank", 2)
    M, D = b.shape
    inv = torch.empty(max(M, 0), dtype=torch.float64, device=b.device)
    with torch.cuda.device(b.device):
        _check(load().csn_bank_norms(_ptr(b), M, D, _ptr(inv), _stream()))
    return inv


def bank_contrastive(student, bank, bank_inv_norm, pos, logit_scale, bank_group=None, inv_rows=None, grad_scale=1.0,
                     want_grad=True, want_dscale=False):
    """csn_bank_contrastive on student [B,D] and bank [M,D] float32, bank_inv_norm [M] float64 (bank_norms), pos int32 [B]
    (bank_group: int32 [M] or None) -> (rows_out [2,B] float64: l, p; loss_part [1] float64; ds [B,D] float32 holding
    grad_scale | None; dscale_part [1] float64 | None).  ``inv_rows``: 1 / the rows the mean is over (default 1 / B)."""
    _need_cuda(student, bank, bank_inv_norm, pos, bank_group)
    s, b = _f32_rows(student, "student", 2), _f32_rows(bank, "bank", 2)
    B, D = s.shape
    M = b.shape[0]
    if b.shape[1] != D or b.device != s.device:
        raise CsnError(f"bank_contrastive: bank {tuple(b.shape)} on {b.device} against student {tuple(s.shape)} on {s.device}")
    for name, v, dtype, n in (("bank_inv_norm", bank_inv_norm, torch.float64, M), ("pos", pos, torch.int32, B),
                              ("bank_group", bank_group, torch.int32, M)):
        if v is not None and (v.dtype != dtype or tuple(v.shape) != (n,) or not v.is_contiguous() or v.device != s.device):
            raise CsnError(f"bank_contrastive: {name} must be a contiguous {dtype} [{n}] tensor on {s.device}, "
                           f"got {v.dtype} {tuple(v.shape)} on {v.device}")
    lib = load()
    rows_out = torch.empty((2, max(B, 0)), dtype=torch.float64, device=s.device)
    loss_part = torch.empty(1, dtype=torch.float64, device=s.device)
    ds = torch.empty((max(B, 0), D), dtype=torch.float32, device=s.device) if want_grad else None
    dscale = torch.empty(1, dtype=torch.float64, device=s.device) if want_dscale else None
    scratch = torch.empty(lib.csn_bank_contrastive_scratch_bytes(B, M, D) // 8, dtype=torch.float64, device=s.device)   # caller-owned
    with torch.cuda.device(s.device):
        _check(lib.csn_bank_contrastive(_ptr(s), B, D, _ptr(b), _ptr(bank_inv_norm), _ptr(bank_group), M, _ptr(pos),
                                        float(logit_scale), float(1.0 / B if inv_rows is None else inv_rows), float(grad_scale),
                                        _ptr(rows_out), _ptr(loss_part), _ptr(ds), _ptr(dscale), _ptr(scratch), _stream()))
    return rows_out, loss_part, ds, dscale


def l2_topk(gallery, query, k):
    _need_cuda(gallery, query)
    g, q = gallery.float().contiguous(), query.float().contiguous()
    Ng, D = g.shape
    Nq = q.shape[0]
    lib = load()
    scratch = torch.empty(lib.csn_l2_topk_scratch_bytes(Ng, Nq), dtype=torch.uint8, device=g.device)
    idx = torch.empty((Nq, k), dtype=torch.int64, device=g.device)
    dist = torch.empty((Nq, k), dtype=torch.float32, device=g.device)
    _check(lib.csn_l2_topk(_ptr(g), _ptr(q), Ng, Nq, D, k, _ptr(idx), _ptr(dist), _ptr(scratch), _stream()))
    return dist, idx


def l2_topk_tiled(gallery, query, k, splits=0, dist64=False):
    """csn_l2_topk_tiled: k up to 1024, no [Nq,Ng] scratch.  -> (dist, idx), or (dist, idx, dist64) with dist64=True."""
    _need_cuda(gallery, query)
    g, q = gallery.float().contiguous(), query.float().contiguous()
    Ng, D = g.shape
    Nq = q.shape[0]
    lib = load()
    nbytes = lib.csn_l2_topk_tiled_scratch_bytes(Ng, Nq, k)
    if nbytes == 0:
        raise CsnError(f"libcsn_hip: {lib.csn_last_error().decode()}")
    with torch.cuda.device(g.device):
        scratch = torch.empty(nbytes, dtype=torch.uint8, device=g.device)
        idx = torch.empty((Nq, k), dtype=torch.int64, device=g.device)
        dist = torch.empty((Nq, k), dtype=torch.float32, device=g.device)
        d64 = torch.empty((Nq, k), dtype=torch.float64, device=g.device) if dist64 else None
        _check(lib.csn_l2_topk_tiled(_ptr(g), _ptr(q), Ng, Nq, D, k, splits, _ptr(idx), _ptr(dist), _ptr(d64), _ptr(scratch),
                                     _stream()))
    return (dist, idx, d64) if dist64 else (dist, idx)


def _nct_view(x, name):
    """A float32 [N,C,T] device tensor whose time stride is 1 and whose strides csn_chan_l2_dist can address in place
    (a slice of a larger tensor is); anything else is made contiguous."""
    if x.dim() != 3:
        raise CsnError(f"chan_l2_dist: {name} must be [N,C,T], got shape {tuple(x.shape)}")
    x = x.float()
    N, C, T = x.shape
    if N and C and T and (x.stride(2) != 1 or x.stride(1) < T or x.stride(0) < (C - 1) * x.stride(1) + T):
        x = x.contiguous()
    return x


def chan_l2_dist(gallery_nct, query_nct, t0, t1, channels=None, out=None):
    """csn_chan_l2_dist: per-channel squared-L2 matrices Dc[nch,Nq,Ng] float64 of the window [t0, t1) of channel-first
    recordings, read in place.  channels: a host sequence (None = all, ascending).  out: a dense float64 buffer to fill."""
    _need_cuda(gallery_nct, query_nct)
    g, q = _nct_view(gallery_nct, "gallery"), _nct_view(query_nct, "query")
    Ng, C, T = g.shape
    Nq = q.shape[0]
    if tuple(q.shape[1:]) != (C, T):
        raise CsnError(f"chan_l2_dist: gallery is [*, {C}, {T}], query [*, {q.shape[1]}, {q.shape[2]}]")
    if channels is None:
        nch, arr = C, None
    else:
        nch = len(channels)
        arr = (ctypes.c_int32 * max(nch, 1))(*[int(c) for c in channels])
    with torch.cuda.device(g.device):
        if out is None:
            out = torch.empty((max(nch, 0), Nq, Ng), dtype=torch.float64, device=g.device)
        elif (not out.is_cuda or out.device != g.device or out.dtype != torch.float64 or not out.is_contiguous()
              or out.numel() != nch * Nq * Ng):
            raise CsnError("chan_l2_dist: out must be a dense float64 buffer of nch*Nq*Ng elements on the gallery's device")
        _check(load().csn_chan_l2_dist(_ptr(g), g.stride(0), g.stride(1), _ptr(q), q.stride(0), q.stride(1), Ng, Nq, C, T,
                                       int(t0), int(t1), arr, nch, _ptr(out), _stream()))
    return out.view(nch, Nq, Ng)


def chan_l2_select(base, Dc, gallery_class, query_class, k, want=("idx", "dist", "hits", "top1")):
    """csn_chan_l2_select: for every (candidate, query) the k smallest of base + Dc[j] under (value, index).  base may be
    None.  -> dict with the outputs named in ``want``: idx [nc,Nq,k] int64, dist [nc,Nq,k] float64, hits / top1 [nc,Nq]
    int32."""
    _need_cuda(base, Dc, gallery_class, query_class)
    if Dc.dim() != 3 or Dc.dtype != torch.float64 or not Dc.is_contiguous():
        raise CsnError("chan_l2_select: Dc must be a dense float64 [nc,Nq,Ng] tensor")
    nc, Nq, Ng = Dc.shape
    if base is not None and (base.dtype != torch.float64 or not base.is_contiguous() or tuple(base.shape) != (Nq, Ng)):
        raise CsnError("chan_l2_select: base must be a dense float64 [Nq,Ng] tensor")
    for t, n, name in ((gallery_class, Ng, "gallery_class"), (query_class, Nq, "query_class")):
        if t is not None and (t.dtype != torch.int32 or not t.is_contiguous() or t.numel() != n):
            raise CsnError(f"chan_l2_select: {name} must be a dense int32 tensor of {n} elements")
    unknown = set(want) - {"idx", "dist", "hits", "top1"}
    if unknown:
        raise CsnError(f"chan_l2_select: unknown outputs {sorted(unknown)}")
    k = int(k)
    kk = max(k, 0)
    with torch.cuda.device(Dc.device):
        out = {}
        if "idx" in want:
            out["idx"] = torch.empty((nc, Nq, kk), dtype=torch.int64, device=Dc.device)
        if "dist" in want:
            out["dist"] = torch.empty((nc, Nq, kk), dtype=torch.float64, device=Dc.device)
        if "hits" in want:
            out["hits"] = torch.empty((nc, Nq), dtype=torch.int32, device=Dc.device)
        if "top1" in want:
            out["top1"] = torch.empty((nc, Nq), dtype=torch.int32, device=Dc.device)
        _check(load().csn_chan_l2_select(_ptr(base), _ptr(Dc), nc, Nq, Ng, _ptr(gallery_class), _ptr(query_class), k,
                                         _ptr(out.get("idx")), _ptr(out.get("dist")), _ptr(out.get("hits")),
                                         _ptr(out.get("top1")), _stream()))
    return out


def chan_l2_accumulate(base, D_one, first):
    """csn_chan_l2_accumulate, in place: base = D_one if first else base + D_one (float64, element-wise)."""
    _need_cuda(base, D_one)
    if (base.dtype != torch.float64 or D_one.dtype != torch.float64 or not base.is_contiguous() or not D_one.is_contiguous()
            or base.numel() != D_one.numel()):
        raise CsnError("chan_l2_accumulate: base and D_one must be dense float64 tensors of one size")
    with torch.cuda.device(base.device):
        _check(load().csn_chan_l2_accumulate(_ptr(base), _ptr(D_one), base.numel(), int(bool(first)), _stream()))
    return base


def topk_merge(D_parts, I_parts, k, want=("idx", "dist64", "dist")):
    """csn_topk_merge: the exact merge of P candidate lists.  D_parts [P,Nq,k_in] float64, I_parts [P,Nq,k_in] int64,
    dense device tensors, padding (+inf, -1).  -> dict with the outputs named in ``want``: idx [Nq,k] int64 (always),
    dist64 [Nq,k] float64, dist [Nq,k] float32.  A query with fewer than k real candidates has index -1 in its last
    places; the caller checks."""
    _need_cuda(D_parts, I_parts)
    if D_parts.dim() != 3 or D_parts.dtype != torch.float64 or not D_parts.is_contiguous():
        raise CsnError("topk_merge: D_parts must be a dense float64 [P,Nq,k_in] tensor")
    if I_parts.dtype != torch.int64 or not I_parts.is_contiguous() or I_parts.shape != D_parts.shape:
        raise CsnError(f"topk_merge: I_parts must be a dense int64 tensor of D_parts' shape {tuple(D_parts.shape)}")
    if I_parts.device != D_parts.device:
        raise CsnError("topk_merge: D_parts and I_parts are on different devices")
    unknown = set(want) - {"idx", "dist64", "dist"}
    if unknown:
        raise CsnError(f"topk_merge: unknown outputs {sorted(unknown)}")
    P, Nq, k_in = D_parts.shape
    k = int(k)
    kk = max(k, 0)
    dev = D_parts.device
    with torch.cuda.device(dev):
        out = {"idx": torch.empty((Nq, kk), dtype=torch.int64, device=dev)}
        if "dist64" in want:
            out["dist64"] = torch.empty((Nq, kk), dtype=torch.float64, device=dev)
        if "dist" in want:
            out["dist"] = torch.empty((Nq, kk), dtype=torch.float32, device=dev)
        _check(load().csn_topk_merge(_ptr(D_parts), _ptr(I_parts), P, Nq, k_in, k, _ptr(out["idx"]),
                                     _ptr(out.get("dist64")), _ptr(out.get("dist")), _stream()))
    return out


def topk_class_metrics(idx, gallery_class, query_class, n_classes,
                       want=("hits", "top1", "pred", "class", "top1_correct")):
    """csn_topk_class_metrics: per-query hit counts of neighbour lists idx [Nq,k] int64 and their per-class integer sums.
    gallery_class [Ng] / query_class [Nq]: dense int32 device tensors of class ids in [0, n_classes).  -> dict with the
    outputs named in ``want``: hits / top1 / pred [Nq] int32, class [n_classes,4] int64 (queries, queries with a hit, sum
    of hits, first query index or -1), top1_correct [1] int64."""
    _need_cuda(idx, gallery_class, query_class)
    if idx.dim() != 2 or idx.dtype != torch.int64 or not idx.is_contiguous():
        raise CsnError("topk_class_metrics: idx must be a dense int64 [Nq,k] tensor")
    Nq, k = idx.shape
    Ng = gallery_class.numel()
    for t, n, name in ((gallery_class, Ng, "gallery_class"), (query_class, Nq, "query_class")):
        if t.dtype != torch.int32 or not t.is_contiguous() or t.dim() != 1 or t.numel() != n or t.device != idx.device:
            raise CsnError(f"topk_class_metrics: {name} must be a dense int32 tensor of {n} elements on idx's device")
    unknown = set(want) - {"hits", "top1", "pred", "class", "top1_correct"}
    if unknown:
        raise CsnError(f"topk_class_metrics: unknown outputs {sorted(unknown)}")
    n_classes = int(n_classes)
    dev = idx.device
    with torch.cuda.device(dev):
        out = {}
        for name in ("hits", "top1", "pred"):
            if name in want:
                out[name] = torch.empty(Nq, dtype=torch.int32, device=dev)
        if "class" in want:
            out["class"] = torch.empty((max(n_classes, 0), 4), dtype=torch.int64, device=dev)
        if "top1_correct" in want:
            out["top1_correct"] = torch.empty(1, dtype=torch.int64, device=dev)
        _check(load().csn_topk_class_metrics(_ptr(idx), Nq, k, _ptr(gallery_class), Ng, _ptr(query_class), n_classes,
                                             _ptr(out.get("hits")), _ptr(out.get("top1")), _ptr(out.get("pred")),
                                             _ptr(out.get("class")), _ptr(out.get("top1_correct")), _stream()))
    return out
