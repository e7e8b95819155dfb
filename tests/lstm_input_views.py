"""Strided and misaligned views of an LSTM input, shared by tests/test_lstm_input_views_cpu.py and
tests/test_gpu_lstm_input_views.py (not a test module).

csn_lstm_forward takes x with two element strides and asks nothing else of them (include/csn_hip.h); three kernels turn
that x into the workspace copies everything downstream reads, two of them with a 16-byte branch and a scalar branch.
Here: the views that select each branch, carved out of NaN-filled buffers so that a wrong index shows; the matrix of
plans the GPU test runs them on; and Python mirrors of the branch predicates, so that which branch a (case, view) pair
takes is checkable without a GPU."""
import torch

NAN = float("nan")


def _buffer(x, *shape):
    return torch.full(shape, NAN, dtype=torch.float32, device=x.device)


def _filled(view, x):
    view.copy_(x)
    return view, x.clone()


def _time_major(x):                     # strides (I, B*I): the form trainer.embed hands over; s0 < s1
    B, T, I = x.shape
    return _filled(_buffer(x, T + 2, B, I)[1:T + 1].transpose(0, 1), x)


def _chan_slice_aligned(x):             # padded rows, every row start on 16 bytes (I + 8 keeps I's residue mod 4)
    B, T, I = x.shape
    return _filled(_buffer(x, B, T, I + 8)[:, :, :I], x)


def _chan_slice_off1(x):                # the base is 4-byte aligned only
    B, T, I = x.shape
    return _filled(_buffer(x, B, T, I + 8)[:, :, 1:I + 1], x)


def _chan_slice_odd_pitch(x):           # aligned base, strides that are no multiple of 4
    B, T, I = x.shape
    return _filled(_buffer(x, B, T, I + 3)[:, :, :I], x)


def _time_slice(x):                     # base offset 3 I
    B, T, I = x.shape
    return _filled(_buffer(x, B, T + 5, I)[:, 3:3 + T], x)


def _time_step2(x):
    B, T, I = x.shape
    return _filled(_buffer(x, B, 2 * T, I)[:, ::2], x)


def _batch_step2(x):
    B, T, I = x.shape
    return _filled(_buffer(x, 2 * B, T, I)[::2], x)


def _batch_broadcast(x):                # stride 0: every row IS row 0, so the dense equivalent is row 0 repeated
    B, T, I = x.shape
    row = _buffer(x, 3, T, I)[1:2]
    row.copy_(x[:1])
    return row.expand(B, T, I), x[:1].expand(B, T, I).contiguous()


# name -> builder(dense [B,T,I] float32) -> (view, dense equivalent): view.shape == x.shape, view.stride(2) == 1,
# torch.equal(view, dense equivalent), and every element of the view's storage outside the view is NaN
VIEWS = {
    "time_major": _time_major,
    "chan_slice_aligned": _chan_slice_aligned,
    "chan_slice_off1": _chan_slice_off1,
    "chan_slice_odd_pitch": _chan_slice_odd_pitch,
    "time_slice": _time_slice,
    "time_step2": _time_step2,
    "batch_step2": _batch_step2,
    "batch_broadcast": _batch_broadcast,
}


def backing(view):
    """The whole storage behind `view` as one flat float32 tensor (an alias, not a copy)."""
    return torch.empty(0, dtype=view.dtype, device=view.device).set_(view.untyped_storage())


def covered(view):
    """bool [storage elements]: which elements of the storage `view` addresses."""
    n = backing(view).numel()
    idx = torch.arange(n).as_strided(view.shape, view.stride(), view.storage_offset())
    mask = torch.zeros(n, dtype=torch.bool)
    mask[idx.reshape(-1)] = True
    return mask


def byte_offset(view):
    """Offset of the view's first element from its allocation, in bytes.  Allocator bases are at least 64-byte aligned
    on the host and on the device, so this decides 16-byte alignment."""
    return view.storage_offset() * view.element_size()


# ---- the plans the views run on: name -> ((B, T, I, H, L), dtype, kind, environment) ---------------------------------
# kind: what turns x into the workspace copies --
#   "row_major"  launch_cast_strided alone (paths 0 and 4, prep_row_major)
#   "cast"       kPrepCastX alone (bf16 paths 1-3 without the fused layer-0 projection)
#   "ks_fused"   kPrepCastX + kPrepBlockifyX feeding the K-split weight-stationary forward
#   "ns_fused"   kPrepCastX + kPrepBlockifyX feeding the N-split one
MATRIX = {
    "p0_f32": ((20, 5, 24, 96, 2), "f32", "row_major", {}),
    "p4_f32": ((70, 5, 24, 128, 2), "f32", "row_major", {}),
    "p0_bf16": ((8, 5, 24, 96, 2), "bf16", "row_major", {}),
    "p1_env": ((16, 5, 32, 128, 2), "bf16", "cast", {"CSN_NO_PERSIST": "1"}),
    "ks_gemm_i24": ((63, 5, 24, 128, 2), "bf16", "cast", {}),
    "ks_gemm_i12": ((63, 5, 12, 128, 2), "bf16", "cast", {}),
    "ks_fused_i32": ((63, 5, 32, 128, 2), "bf16", "ks_fused", {}),           # Bpad 64: one pad row
    "ks_fused_i96": ((65, 3, 96, 256, 2), "bf16", "ks_fused", {}),           # 3 k-blocks, Bpad 128: 63 pad rows
    "ns_fused_i128": ((65, 3, 128, 128, 2), "bf16", "ns_fused", {"CSN_FWD_NSPLIT": "1"}),
    # one fused shape with the fusion switched off: the same views through kPrepCastX + the projection GEMM
    "ks_nofuse_i32": ((63, 5, 32, 128, 2), "bf16", "cast", {"CSN_NO_FUSE_X": "1"}),
}
FUSED = tuple(n for n, c in MATRIX.items() if c[2].endswith("_fused"))


# ---- mirrors of the branch predicates --------------------------------------------------------------------------------
def cast_x_vector(I, sb, st, ptr):
    """kPrepCastX takes its two-float4 branch: csrc/lstm_cell_blk.hip, `case kPrepCastX`, line 231:
    (I & 7) == 0 && (J.s0 & 3) == 0 && (J.s1 & 3) == 0 && (uintptr_t(J.a) & 15) == 0."""
    return I % 8 == 0 and sb % 4 == 0 and st % 4 == 0 and ptr % 16 == 0


def blockify_x_vector(sb, st, ptr):
    """kPrepBlockifyX takes its two-float4 branch for the rows r < B: csrc/lstm_cell_blk.hip, `case kPrepBlockifyX`,
    line 254: ((J.s0 | J.s1) & 3) == 0 && (uintptr_t(J.a) & 15) == 0."""
    return (sb | st) % 4 == 0 and ptr % 16 == 0


def fuse_x(path_is_ns, I, H):
    """Layer 0's projection runs inside the weight-stationary forward (x_blk and wih0_blk exist): csrc/lstm.hip,
    make_layout, lines 125-126, for a plan on paths 2-3 without CSN_NO_FUSE_X:
    w.fwd_ns ? d.I == 128 : (d.I % 32 == 0 && d.I <= 128 && d.H != 512)."""
    return I == 128 if path_is_ns else (I % 32 == 0 and I <= 128 and H != 512)


def branches(case, view):
    """(cast_x_vector, blockify_x_vector or None where the case does not fuse) of `view` on MATRIX[case]."""
    (B, T, I, H, L), _, kind, _ = MATRIX[case]
    sb, st, ptr = view.stride(0), view.stride(1), byte_offset(view)
    return cast_x_vector(I, sb, st, ptr), (blockify_x_vector(sb, st, ptr) if kind.endswith("_fused") else None)
