"""GPU: the LSTM on strided and misaligned views of its input, bit for bit against the dense copy of the same values.

csn_lstm_forward takes x with two element strides; cast_strided_kernel (paths 0 and 4), kPrepCastX (bf16 paths 1-3) and
kPrepBlockifyX (the fused layer-0 projection) turn it into the workspace copies everything downstream -- the dW_ih GEMM
of the backward included -- reads.  They are pure copies and casts, so a view must give the bits of its dense copy; the
views (tests/lstm_input_views.py) sit in NaN-filled buffers, so an index outside the view shows as a non-finite output.
Which branch of each kernel a (case, view) pair takes: tests/test_lstm_input_views_cpu.py.  Every case checks the plan's
path and kernels and the workspace status word."""
import ctypes

import numpy as np
import pytest
import torch

import lstm_input_views as lv
import test_gpu_lstm_state as st
from cerebralsignalnetworks_amd import cabi, filters, LSTM
from cerebralsignalnetworks_amd.lstm_model import HipLSTM
from oracle import compare, lstm as olstm

pytestmark = pytest.mark.gpu

DEV, BF16, F32 = st.DEV, st.BF16, st.F32
DTYPES = {"f32": F32, "bf16": BF16}
P4 = (4, "lstm_fwd_f32_persist_kernel", "lstm_bwd_f32_persist_kernel")
# (path, forward kernel, backward kernel) of a HipLSTM plan of the case; an LSTM (state) plan takes the same for bf16 and
# the per-step cells for float32 (p4_f32 is reached by the plain plan alone)
EXPECT = {"p0_f32": st.V1, "p4_f32": P4, "p0_bf16": st.V1, "p1_env": st.IL, "ks_gemm_i24": st.P3, "ks_gemm_i12": st.P3,
          "ks_fused_i32": st.P3, "ks_fused_i96": st.P3, "ns_fused_i128": st.P3_NS, "ks_nofuse_i32": st.P3}
EXPECT_STATE = dict(EXPECT, p4_f32=st.V1_KS)
CASE_VIEW = [(c, v) for c in lv.MATRIX for v in lv.VIEWS]


def _workspace_bytes(shape, dtype, flags, monkeypatch, no_fuse):
    with monkeypatch.context() as mp:
        if no_fuse:
            mp.setenv("CSN_NO_FUSE_X", "1")
        d = cabi.LstmDesc(*shape, cabi._dt(dtype))
        return cabi.load().csn_lstm_workspace_bytes(ctypes.byref(d), flags)


def _setup(case, monkeypatch, state=False, seed=0):
    """Environment of the case, a module with seeded weights, and that the case fuses layer 0 exactly where the matrix
    says: x_blk and wih0_blk are laid out only then, so the workspace is larger than under CSN_NO_FUSE_X=1."""
    shape, dtype, kind, env = lv.MATRIX[case]
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    flags = 1 | (cabi.LSTM_STATE if state else 0)
    here = _workspace_bytes(shape, DTYPES[dtype], flags, monkeypatch, False)
    unfused = _workspace_bytes(shape, DTYPES[dtype], flags, monkeypatch, True)
    if kind.endswith("_fused"):
        assert here > unfused > 0, (case, here, unfused)
    else:
        assert here == unfused > 0, (case, here, unfused)
    B, T, I, H, L = shape
    torch.manual_seed(seed)
    m = (LSTM if state else HipLSTM)(I, H, L, compute_dtype=DTYPES[dtype]).to(DEV)
    m._case_T = T
    return shape, DTYPES[dtype], m


def _inputs(shape, seed=0):
    B, T, I, H, L = shape
    g = torch.Generator(device="cpu").manual_seed(seed + 1)
    x = torch.randn(B, T, I, generator=g)
    dy_last = torch.randn(B, H, generator=g)
    dy_all = torch.randn(B, T, H, generator=g)
    return [t.to(DEV) for t in (x, dy_last, dy_all)]


def _check_plans(m, case):
    """Path, kernel names and a zero status word of every plan of `m` (st._check_plans for a state module)."""
    plans = m.all_plans()
    assert plans, "no plan was created"
    if isinstance(m, LSTM):
        st._check_plan(m, EXPECT_STATE[case])
        return
    for plan in plans:
        assert not plan.state
        assert (plan.path(),) + plan.kernel_names() == EXPECT[case], (case, plan.path(), plan.kernel_names())
        assert plan.status() == 0


def _run(m, x, dy_last, dy_all, after_forward=None):
    """One training step of a HipLSTM on `x` AS IT IS (no clone: its strides are the subject): y_all and dx asked for,
    loss <y_all, dy_all> + <y_last, dy_last>.  `after_forward` runs between the forward and the backward."""
    xr = x.detach().requires_grad_(True)
    assert xr.stride() == x.stride() and xr.data_ptr() == x.data_ptr()
    for p in m.parameters():
        p.grad = None
    y_all, y_last = m(xr, want_all=True)
    if after_forward is not None:
        after_forward()
    ((y_all * dy_all).sum() + (y_last * dy_last).sum()).backward()
    grads = {k: p.grad.detach().clone() for k, p in m.named_parameters()}
    return dict(y_last=y_last.detach(), y_all=y_all.detach(), dx=xr.grad.detach(), **grads)


def _same_bits(got, want, what):
    assert set(got) == set(want)
    bad = [f"{k} (max |diff| {float((got[k].float() - want[k].float()).abs().max()):.3e})" for k in want
           if not torch.equal(got[k], want[k])]
    assert not bad, f"{what}: not bit-equal: " + ", ".join(bad)


def _all_finite(res, what):
    bad = [k for k, v in res.items() if not bool(torch.isfinite(v).all())]
    assert not bad, f"{what}: non-finite values in {bad}"


def _oracle(m, dtype, dense, dy_last, dy_all):
    """_run's call on oracle.lstm: the bf16-faithful emulator, or without rounding (float64) for a float32 plan."""
    lp = {k: v.detach().cpu().numpy() for k, v in m.state_dict().items()}
    rounding = dtype == BF16
    y, saved = olstm.lstm_forward_bf16(st._np(dense), lp, m.num_layers, rounding=rounding)
    dy = dy_all.cpu().numpy().copy()
    dy[:, -1] += dy_last.cpu().numpy()              # float32, as the library adds them
    dx, g, _ = olstm.lstm_backward_bf16(dy, saved, m.num_layers, rounding=rounding)
    return dict(y_last=y[:, -1], y_all=y, dx=dx, **g)


def _check_against_oracle(tag, dtype, got, want):
    line = []
    if dtype == BF16:
        for k, w in want.items():
            line.append("%s %.2e/%.2e" % ((k,) + compare.errors(st._np(got[k]), w)))
        print(f"measured bf16 vs emulator {tag} (rel/elem): " + " ".join(line))
        for k, w in want.items():
            compare.check(f"{tag}: {k}", st._np(got[k]), w, *compare.bf16_emu_bound(k), layout=compare.layout_of(k))
        return
    elem, rel = st._bounds(F32)                     # outputs: max |difference|; gradients: relative norm
    errs = {k: float(np.abs(st._np(got[k]) - w).max()) if k in ("y_last", "y_all") else compare.errors(st._np(got[k]), w)[0]
            for k, w in want.items()}
    print(f"measured float32 vs float64 oracle {tag} (outputs max |diff|, gradients rel): " +
          " ".join(f"{k} {e:.2e}" for k, e in errs.items()))
    for k, e in errs.items():
        assert e < (elem if k in ("y_last", "y_all") else rel), (tag, k, e)


@pytest.mark.parametrize("case,view", CASE_VIEW)
def test_view_gives_the_bits_of_its_dense_copy(case, view, monkeypatch):
    shape, dtype, m = _setup(case, monkeypatch)
    x, dy_last, dy_all = _inputs(shape)
    v, dense = lv.VIEWS[view](x)
    assert torch.equal(v, dense) and v.stride(2) == 1 and not v.is_contiguous()
    first = _run(m, dense, dy_last, dy_all)
    second = _run(m, dense, dy_last, dy_all)
    got = _run(m, v, dy_last, dy_all)
    torch.cuda.synchronize()
    assert len(m.all_plans()) == 1                  # the three runs shared one training plan
    _check_plans(m, case)
    for res, what in ((first, "dense"), (got, view)):
        _all_finite(res, f"{case} {what}")
    _same_bits(second, first, f"{case}: dense run against dense run")
    _same_bits(got, first, f"{case} {view} against its dense copy")


# (p4_f32 and p0_bf16 beside the three the views were introduced with: cast_strided_kernel has ONE branch, so a wrong
# index in it moves the dense run and the view together and the bit comparison above cannot see it -- its two
# instantiations and both paths that launch it are held against the oracle here.  Likewise ks_gemm_i12, whose dense run
# takes kPrepCastX's scalar branch too)
@pytest.mark.parametrize("case", ["p0_f32", "ks_gemm_i12", "ks_fused_i32", "p4_f32", "p0_bf16"])
@pytest.mark.parametrize("view", ["time_major", "chan_slice_off1"])
def test_view_matches_the_oracle(case, view, monkeypatch):
    """Against oracle.lstm, so that the file does not rest on the dense path being right."""
    shape, dtype, m = _setup(case, monkeypatch, seed=2)
    x, dy_last, dy_all = _inputs(shape, seed=2)
    v, dense = lv.VIEWS[view](x)
    got = _run(m, v, dy_last, dy_all)
    torch.cuda.synchronize()
    _check_plans(m, case)
    _all_finite(got, f"{case} {view}")
    _check_against_oracle(f"{case} {view}", dtype, got, _oracle(m, dtype, dense, dy_last, dy_all))


def _random_with_zeros(B, T, seed=0):
    # the pattern of that name in tests/test_gpu_lstm_lengths.py: a full row, empty rows at both ends of the batch
    n = np.random.default_rng(1000 + seed).integers(0, T + 1, B).tolist()
    n[0], n[1], n[B - 1] = T, 0, 0
    return [int(k) for k in n]


def _state_args(shape, seed=0):
    B, T, I, H, L = shape
    g = torch.Generator(device="cpu").manual_seed(seed + 7)
    ts = (0.5 * torch.randn(L, B, H, generator=g), torch.randn(L, B, H, generator=g), torch.randn(B, T, H, generator=g),
          torch.randn(L, B, H, generator=g), torch.randn(L, B, H, generator=g))
    return [t.to(DEV) for t in ts]


def _run_state(m, x, h0, c0, dy, dh, dc, lengths):
    """The LSTM drop-in on `x` as it is, with (h0, c0) and lengths: loss <out, dy> + <h_n, dh> + <c_n, dc>."""
    xr = x.detach().requires_grad_(True)
    assert xr.stride() == x.stride() and xr.data_ptr() == x.data_ptr()
    h0, c0 = h0.clone().requires_grad_(True), c0.clone().requires_grad_(True)
    for p in m.parameters():
        p.grad = None
    out, (h_n, c_n) = m(xr, (h0, c0), lengths=lengths)
    torch.autograd.backward([out, h_n, c_n], [dy, dh, dc])
    grads = {k: p.grad.detach().clone() for k, p in m.named_parameters()}
    return dict(out=out.detach(), h_n=h_n.detach(), c_n=c_n.detach(), dx=xr.grad.detach(), dh0=h0.grad, dc0=c0.grad, **grads)


def _bits(view):
    return lv.backing(view).view(torch.int32).clone()        # (int32: NaN == NaN)


@pytest.mark.parametrize("case,view", CASE_VIEW)
def test_caller_buffers_are_left_alone(case, view, monkeypatch):
    shape, dtype, m = _setup(case, monkeypatch, seed=3)
    x, dy_last, dy_all = _inputs(shape, seed=3)
    v, _ = lv.VIEWS[view](x)
    before = _bits(v)
    got = _run(m, v, dy_last, dy_all)
    torch.cuda.synchronize()
    assert torch.equal(_bits(v), before)
    _all_finite(got, f"{case} {view}")
    _check_plans(m, case)


@pytest.mark.parametrize("case", ["p0_f32", "p1_env", "ks_fused_i32"])
@pytest.mark.parametrize("view", list(lv.VIEWS))
def test_caller_buffers_are_left_alone_with_lengths(case, view, monkeypatch):
    """mask_tm_kernel and mask_x_blk_kernel zero the padding of the workspace copies, never of x."""
    shape, dtype, m = _setup(case, monkeypatch, state=True, seed=3)
    x, _, _ = _inputs(shape, seed=3)
    v, _ = lv.VIEWS[view](x)
    before = _bits(v)
    got = _run_state(m, v, *_state_args(shape), _random_with_zeros(*shape[:2]))
    torch.cuda.synchronize()
    assert torch.equal(_bits(v), before)
    _all_finite(got, f"{case} {view}")
    _check_plans(m, case)


@pytest.mark.parametrize("case,view", CASE_VIEW)
def test_backward_reads_the_copy_not_x(case, view, monkeypatch):
    """csn_lstm_backward takes no x: dW_ih comes from the workspace copy, and the forward has read x by the time its
    work is on the stream -- the caller may reuse the buffer at once."""
    shape, dtype, m = _setup(case, monkeypatch, seed=4)
    x, dy_last, dy_all = _inputs(shape, seed=4)
    v, _ = lv.VIEWS[view](x)
    want = _run(m, v, dy_last, dy_all)
    got = _run(m, v, dy_last, dy_all, after_forward=lambda: lv.backing(v).fill_(lv.NAN))
    torch.cuda.synchronize()
    assert bool(lv.backing(v).isnan().all())
    _all_finite(got, f"{case} {view}")
    _same_bits(got, want, f"{case} {view}: x overwritten with NaN between forward and backward")
    _check_plans(m, case)


@pytest.mark.parametrize("case", ["ks_fused_i32", "p1_env", "p0_f32"])
@pytest.mark.parametrize("view", ["time_major", "chan_slice_off1", "time_step2"])
def test_views_with_state_and_lengths(case, view, monkeypatch):
    shape, dtype, m = _setup(case, monkeypatch, state=True, seed=5)
    B, T = shape[:2]
    x, _, _ = _inputs(shape, seed=5)
    args = _state_args(shape, seed=5)
    lengths = _random_with_zeros(B, T, seed=5)
    v, dense = lv.VIEWS[view](x)
    want = _run_state(m, dense, *args, lengths)
    again = _run_state(m, dense, *args, lengths)
    got = _run_state(m, v, *args, lengths)
    torch.cuda.synchronize()
    _check_plans(m, case)
    _all_finite(got, f"{case} {view}")
    _same_bits(again, want, f"{case}: dense run against dense run")
    _same_bits(got, want, f"{case} {view} with state and lengths against its dense copy")
    for b, n in enumerate(lengths):
        assert not got["dx"][b, n:].any() and not got["out"][b, n:].any(), (case, view, b, n)
    assert got["dx"][0].any()                       # (row 0 is full: its gradient is there)


@pytest.mark.parametrize("case", ["ns_fused_i128", "ks_fused_i128"])
def test_trainer_embed_view(case, monkeypatch):
    """What trainer.embed hands the model: the filter's time-major [T,B,C] output, transposed."""
    B, C, T, H, L = 65, 128, 8, 128, 2
    ns = case == "ns_fused_i128"
    if ns:
        monkeypatch.setenv("CSN_FWD_NSPLIT", "1")
    assert lv.fuse_x(ns, C, H)
    flags = 1
    assert (_workspace_bytes((B, T, C, H, L), BF16, flags, monkeypatch, False) >
            _workspace_bytes((B, T, C, H, L), BF16, flags, monkeypatch, True))
    g = torch.Generator(device="cpu").manual_seed(8)
    eeg = torch.randn(B, C, T, generator=g).to(DEV)
    sos = filters.EEGFilters(1000).sos
    x = filters.eeg_bandpass_znorm(eeg, sos, time_major=True).transpose(0, 1)
    assert x.shape == (B, T, C) and x.stride() == (C, B * C, 1) and bool(torch.isfinite(x).all())
    torch.manual_seed(8)
    m = HipLSTM(C, H, L).to(DEV)
    dy_last = torch.randn(B, H, generator=g).to(DEV)
    dy_all = torch.randn(B, T, H, generator=g).to(DEV)
    want = _run(m, x.contiguous(), dy_last, dy_all)
    got = _run(m, x, dy_last, dy_all)
    torch.cuda.synchronize()
    (plan,) = m.all_plans()
    assert (plan.path(),) + plan.kernel_names() == (st.P3_NS if ns else st.P3) and plan.status() == 0
    _all_finite(got, case)
    _same_bits(got, want, f"{case}: trainer.embed's view against its contiguous copy")
