"""GPU: LSTM input windows -- csn_lstm_plan_set_views, LstmPlan.set_views, LSTM.forward(views=...),
HipLSTM.forward_views, MultiCropWrapper.forward_views and the --fused_views step of LstmDistillation.py.

The defining identity, bit for bit: a call with windows has every output and every gradient of the same plan called with
the same lengths on the materialised dense input xm[b, t] = x[src_row[b], t0[b] + t] (t < n), NaN from n on.  One shape
per x read site and path; source layouts that take the 16-byte and the scalar branch; reverse, dropout and inference
plans; a dense call after a windowed one; the host checks; the fused DINO step against the per-view step with a float64
restatement as the yardstick; the trainer end to end."""
import numpy as np
import pytest
import torch

import lengths_reference  # noqa: F401  (the references the lengths tests are built on; imported as the issue names them)
import lstm_input_views as lv
import test_gpu_lstm_lengths as ll
import test_gpu_lstm_state as st
from cerebralsignalnetworks_amd import cabi, LSTM, Model
from cerebralsignalnetworks_amd.dino import DINOHead, DINOLoss, MultiCropWrapper, temporal_crops, view_rows
from cerebralsignalnetworks_amd.lstm_model import HipLSTM

pytestmark = pytest.mark.gpu

DEV, BF16, F32 = st.DEV, st.BF16, st.F32
NAN = float("nan")

# the case of tests/test_gpu_lstm_lengths.py -> the kernel(s) that read x in it
READ_SITES = {
    "v1_h96": "cast_strided_kernel<bf16> (path 0, prep_row_major)",
    "p1_l5": "kPrepCastX alone (path 1, per-diagonal launches: I = 16 has no fused projection)",
    "chunk4_l3": "kPrepCastX + kPrepBlockifyX (path 3, K-split forward with the fused layer-0 projection, I = 32, chunks of 4)",
    "ks_fused_h768": "kPrepCastX + kPrepBlockifyX (path 3, K-split forward, I = 128, B = 256 = Bpad, three chunks)",
    "ns_fused_h1024_t33": "kPrepCastX + kPrepBlockifyX (path 3, N-split forward, I = 128, B = 65: 63 pad rows)",
    "f32_h128": "cast_strided_kernel<float> (path 0, exact float32)",
}
CASES = {name: ll.CASES[name] for name in READ_SITES}
WINDOWS = ("identity", "t0_zero", "ends_at_source_end", "random", "one_row")
LENGTHS = ("all_T", "two_mixed", "random_with_zeros")


def _lengths(name, pattern):
    B, T = CASES[name][0][:2]
    if pattern == "all_T":
        return [T] * B
    if pattern == "two_mixed":              # the DINO pattern, view-major: the first third of the rows T, the rest 2T/3
        return [T if b < max(1, B // 3) else (2 * T) // 3 for b in range(B)]
    return ll._lengths(name, "random_with_zeros")


def _source(S, Tsrc, I, seed=0, layout="aligned"):
    """A random float32 source [S, Tsrc, I] cut out of a larger NaN-filled buffer, innermost stride 1.
    aligned: base on 16 bytes, both strides multiples of 4 (I % 4 == 0); off1_odd: storage offset of one element and an
    odd time stride; time_major: x_stride_b < x_stride_t."""
    g = torch.Generator(device="cpu").manual_seed(100 + seed)
    data = torch.randn(S, Tsrc, I, generator=g).to(DEV)
    if layout == "aligned":
        src = torch.full((S + 2, Tsrc + 4, I), NAN, device=DEV)[1:S + 1, 2:2 + Tsrc]
        assert I % 4 == 0 and lv.byte_offset(src) % 16 == 0 and src.stride(0) % 4 == 0 and src.stride(1) % 4 == 0
    elif layout == "off1_odd":
        src = torch.full((S, Tsrc, I + 3), NAN, device=DEV)[:, :, 1:I + 1]
        assert src.storage_offset() == 1 and src.stride(1) % 2 == 1
    elif layout == "time_major":
        src = torch.full((Tsrc + 2, S, I), NAN, device=DEV)[1:Tsrc + 1].transpose(0, 1)
        assert src.stride(0) < src.stride(1)
    src.copy_(data)
    assert src.stride(2) == 1 and torch.equal(src, data)
    return src


def _windows(pattern, B, Tsrc, lengths, seed=0):
    """-> (S, src_row[B], t0[B])"""
    rng = np.random.default_rng(500 + seed)
    S = max(1, B // 3)
    n = np.asarray(lengths)
    if pattern == "identity":
        return B, list(range(B)), [0] * B
    if pattern == "one_row":
        return 1, [0] * B, rng.integers(0, Tsrc - n + 1).tolist()
    rows = rng.integers(0, S, B).tolist()
    if pattern == "t0_zero":
        return S, rows, [0] * B
    if pattern == "ends_at_source_end":
        return S, rows, (Tsrc - n).tolist()
    return S, rows, rng.integers(0, Tsrc - n + 1).tolist()


def _materialise(src, rows, starts, lengths, T):
    """xm[b, t] = src[rows[b], starts[b] + t] for t < lengths[b], NaN from there on: dense [B, T, I]."""
    Tsrc = src.shape[1]
    r = torch.tensor(rows, device=DEV)[:, None]
    t = torch.arange(T, device=DEV)[None, :]
    idx = (torch.tensor(starts, device=DEV)[:, None] + t).clamp(max=Tsrc - 1)
    xm = src[r, idx].clone()
    xm[(t >= torch.tensor(lengths, device=DEV)[:, None])] = NAN
    return xm.contiguous()


def _run(m, x, args, lengths, views=None):
    """LSTM forward with state, lengths (and windows) + backward of <out,dy> + <h_n,dh> + <c_n,dc>; x takes no gradient."""
    h0, c0, dy, dh, dc = (t.clone() for t in args)
    h0.requires_grad_(True), c0.requires_grad_(True)
    for p in m.parameters():
        p.grad = None
    out, (h_n, c_n) = m(x, (h0, c0), lengths=lengths, views=views)
    torch.autograd.backward([out, h_n, c_n], [dy, dh, dc])
    grads = {k: p.grad.detach().clone() for k, p in m.named_parameters()}
    return dict(out=out.detach(), h_n=h_n.detach(), c_n=c_n.detach(), dh0=h0.grad, dc0=c0.grad, **grads)


def _plan_run(plan, m, x, args, lengths, views, src_shape=None, backward=True):
    """The same call on a cabi.LstmPlan, with dx (the dense [B, T, I] gradient of the gathered rows)."""
    h0, c0, dy, dh, dc = args
    d, L = plan.desc, m.num_layers
    w = [[getattr(m, f"{n}_l{k}").detach() for k in range(L)] for n in ("weight_ih", "weight_hh", "bias_ih", "bias_hh")]
    if plan.state:
        plan.set_lengths(lengths)
    if views is None:
        plan.set_views(None)
    else:
        plan.set_views(views[0], views[1], *(src_shape or x.shape[:2]))
    kw = dict(h0=h0, c0=c0, want_state=True) if plan.state else {}
    res = plan.forward(x, *w, want_all=True, **kw)
    out = dict(zip(("y_last", "y_all", "h_n", "c_n"), res))
    if backward:
        out["dx"] = torch.empty(d.B, d.T, d.I, device=DEV)
        grads = [[torch.empty_like(p) for p in group] for group in w]
        if plan.state:
            out["dh0"], out["dc0"] = torch.empty(L, d.B, d.H, device=DEV), torch.empty(L, d.B, d.H, device=DEV)
            plan.backward(None, dy, grads, dx=out["dx"], dh_n=dh, dc_n=dc, dh0=out["dh0"], dc0=out["dc0"])
        else:
            plan.backward(None, dy, grads, dx=out["dx"])
        for n, group in zip(("weight_ih", "weight_hh", "bias_ih", "bias_hh"), grads):
            out.update({f"{n}_l{k}": t for k, t in enumerate(group)})
    plan.set_views(None)
    torch.cuda.synchronize()
    return out


def _same_bits(got, want, what):
    assert set(got) == set(want), (what, sorted(got), sorted(want))
    bad = [f"{k} (max |diff| {float((got[k].float() - want[k].float()).abs().max()):.3e})" for k in want
           if not torch.equal(got[k], want[k])]
    assert not bad, f"{what}: not bit-equal: " + ", ".join(bad)


def _all_finite(res, what):
    bad = [k for k, v in res.items() if not bool(torch.isfinite(v).all())]
    assert not bad, f"{what}: non-finite values in {bad}"


def _setup(name, monkeypatch, seed=0):
    shape, dtype, expect, env, _ = CASES[name]
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    m, _, args = st._make(shape, dtype, seed=seed)
    return shape, dtype, expect, m, args[1:]


# ---- 1. the identity, bit for bit ------------------------------------------------------------------------------------
# one module (one pooled training plan) per case: every window and length pattern runs on it, which is also the
# stickiness check -- a setting left behind by one combination would show in the next
@pytest.mark.parametrize("lp", LENGTHS)
@pytest.mark.parametrize("name", list(CASES))
def test_windows_give_the_bits_of_the_materialised_input(name, lp, monkeypatch):
    shape, dtype, expect, m, args = _setup(name, monkeypatch)
    B, T, I, H, L = shape
    Tsrc = T + 7
    lengths = _lengths(name, lp)
    assert max(lengths) == T                        # the plan of the windowed call is the case's (B, T) plan
    for wp in WINDOWS:
        what = f"{name} [{READ_SITES[name]}] {wp} {lp}"
        S, rows, starts = _windows(wp, B, Tsrc, lengths)
        src = _source(S, Tsrc, I)
        if wp == "ends_at_source_end":
            assert all(t + n == Tsrc for t, n in zip(starts, lengths))
        xm = _materialise(src, rows, starts, lengths, T)
        want = _run(m, xm, args, lengths)
        got = _run(m, src, args, lengths, views=(rows, starts))
        _all_finite(want, what + " (materialised)")
        _same_bits(got, want, what)
        if wp == "identity":                        # ... and the call without views on the same rows
            _same_bits(_run(m, src[:, :T], args, lengths), got, what + " against the call without views")
        # dx, at the LstmPlan level, on the module's own training plan
        (plan,) = [pl for pl in m.all_plans() if pl.training]
        assert not plan.busy
        p_want = _plan_run(plan, m, xm, args, lengths, None)
        p_got = _plan_run(plan, m, src, args, lengths, (rows, starts))
        _same_bits(p_got, p_want, what + " (LstmPlan, with dx)")
        pad = torch.arange(T, device=DEV)[None, :] >= torch.tensor(lengths, device=DEV)[:, None]
        assert not p_got["dx"][pad].any(), what
        assert torch.equal(p_got["y_all"], got["out"]) and torch.equal(p_got["h_n"], got["h_n"])
    torch.cuda.synchronize()
    assert len([pl for pl in m.all_plans() if pl.training]) == 1
    ll._check_plan(m, expect)


# ---- 2. layouts of the source ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["v1_h96", "ks_fused_h768"])
def test_source_layouts(name, monkeypatch):
    shape, dtype, expect, m, args = _setup(name, monkeypatch, seed=1)
    B, T, I, H, L = shape
    Tsrc = T + 7
    lengths = _lengths(name, "two_mixed")
    S, rows, starts = _windows("random", B, Tsrc, lengths, seed=1)
    want = None
    for layout in ("aligned", "off1_odd", "time_major"):
        src = _source(S, Tsrc, I, seed=1, layout=layout)
        sb, s_t, off = src.stride(0), src.stride(1), lv.byte_offset(src)
        vector = lv.cast_x_vector(I, sb, s_t, off) and lv.blockify_x_vector(sb, s_t, off)
        assert vector == (layout != "off1_odd"), (layout, sb, s_t, off)       # the branch the fast-path kernels take
        if want is None:
            want = _run(m, _materialise(src, rows, starts, lengths, T), args, lengths)
            _all_finite(want, f"{name} materialised")
        _same_bits(_run(m, src, args, lengths, views=(rows, starts)), want, f"{name} {layout}")
    torch.cuda.synchronize()
    ll._check_plan(m, expect)


# ---- 3. plan bits ----------------------------------------------------------------------------------------------------
# (B, T, I, H, L), dtype, the read site
PLAN_SHAPES = {
    "p0_bf16": ((8, 10, 24, 96, 2), BF16),          # cast_strided_kernel
    "p0_f32": ((9, 10, 24, 96, 2), F32),
    "p1_i16": ((8, 10, 16, 128, 2), BF16),          # kPrepCastX
    "p3_fused_i32": ((63, 9, 32, 128, 2), BF16),    # kPrepCastX + kPrepBlockifyX, one pad row
}


def _plan_case(rep, seed=0, **flags):
    (B, T, I, H, L), dtype = PLAN_SHAPES[rep]
    torch.manual_seed(seed)
    m = LSTM(I, H, L, compute_dtype=dtype).to(DEV)
    g = torch.Generator(device="cpu").manual_seed(seed + 1)
    args = [t.to(DEV) for t in (0.5 * torch.randn(L, B, H, generator=g), torch.randn(L, B, H, generator=g),
                                torch.randn(B, T, H, generator=g), torch.randn(L, B, H, generator=g),
                                torch.randn(L, B, H, generator=g))]
    flags.setdefault("state", True)
    plan = cabi.LstmPlan(B, T, I, H, L, dtype, DEV, **flags)
    rng = np.random.default_rng(seed)
    lengths = rng.integers(0, T + 1, B).tolist()
    lengths[0], lengths[1] = T, 0
    if not flags["state"]:
        lengths = [T] * B
    Tsrc = T + 7
    S, rows, starts = _windows("random", B, Tsrc, lengths, seed=seed)
    src = _source(S, Tsrc, I, seed=seed)
    return plan, m, args, lengths, src, rows, starts, _materialise(src, rows, starts, lengths, T)


@pytest.mark.parametrize("rep", list(PLAN_SHAPES))
@pytest.mark.parametrize("state", [True, False])
def test_reverse_plan_with_windows(rep, state):
    plan, m, args, lengths, src, rows, starts, xm = _plan_case(rep, seed=2, training=True, reverse=True, state=state)
    want = _plan_run(plan, m, xm, args, lengths, None)
    got = _plan_run(plan, m, src, args, lengths, (rows, starts))
    _all_finite(want, rep)
    _same_bits(got, want, f"reverse plan {rep} state={state}")
    # the reverse plan really walks each window backwards: row 0 (length T) against a plain plan on the flipped window
    (B, T, I, H, L), dtype = PLAN_SHAPES[rep]
    plain = cabi.LstmPlan(B, T, I, H, L, dtype, DEV, training=True, state=state)
    flipped = xm.clone()
    flipped[0] = xm[0].flip(0)
    fwd = _plan_run(plain, m, torch.nan_to_num(flipped), args, [T] * B, None, backward=False)
    assert torch.equal(fwd["y_all"][0].flip(0), got["y_all"][0])
    assert plan.status() == 0


@pytest.mark.parametrize("rep", list(PLAN_SHAPES))
def test_dropout_plan_with_windows(rep):
    plan, m, args, lengths, src, rows, starts, xm = _plan_case(rep, seed=3, training=True, dropout=True)
    plan.set_dropout(0.5, seed=1234, subsequence=1)
    want = _plan_run(plan, m, xm, args, lengths, None)
    got = _plan_run(plan, m, src, args, lengths, (rows, starts))
    _all_finite(want, rep)
    _same_bits(got, want, f"dropout plan {rep}")
    plan.set_dropout(0.0)
    off = _plan_run(plan, m, src, args, lengths, (rows, starts))
    assert not torch.equal(off["y_all"], got["y_all"])          # the mask was on
    assert plan.status() == 0


@pytest.mark.parametrize("rep", list(PLAN_SHAPES))
def test_inference_plan_with_windows(rep):
    plan, m, args, lengths, src, rows, starts, xm = _plan_case(rep, seed=4, training=True)
    (B, T, I, H, L), dtype = PLAN_SHAPES[rep]
    infer = cabi.LstmPlan(B, T, I, H, L, dtype, DEV, training=False, state=True)
    train = _plan_run(plan, m, src, args, lengths, (rows, starts), backward=False)
    got = _plan_run(infer, m, src, args, lengths, (rows, starts), backward=False)
    _same_bits(got, train, f"inference plan {rep}")
    _same_bits(got, _plan_run(infer, m, xm, args, lengths, None, backward=False), f"inference plan {rep} on xm")
    assert plan.status() == 0 and infer.status() == 0


# ---- 4. stickiness and reset -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("rep", list(PLAN_SHAPES))
def test_views_are_sticky_until_cleared_and_leave_nothing_behind(rep):
    plan, m, args, lengths, src, rows, starts, xm = _plan_case(rep, seed=5, training=True)
    (B, T, I, H, L), dtype = PLAN_SHAPES[rep]
    dense = torch.nan_to_num(xm)
    w = [[getattr(m, f"{n}_l{k}").detach() for k in range(L)] for n in ("weight_ih", "weight_hh", "bias_ih", "bias_hh")]
    plan.set_lengths(lengths)
    plan.set_views(rows, starts, *src.shape[:2])
    first = plan.forward(src, *w, want_all=True, h0=args[0], c0=args[1])[1].clone()
    second = plan.forward(src, *w, want_all=True, h0=args[0], c0=args[1])[1].clone()       # sticky: no second set_views
    assert torch.equal(first, second)
    with pytest.raises(AssertionError):                                 # a [B, T, I] input is no longer what the plan takes
        plan.forward(dense, *w, want_all=True)
    plan.set_views(None)
    plan.set_lengths(None)
    after = _plan_run(plan, m, dense, args, None, None)
    fresh = cabi.LstmPlan(B, T, I, H, L, dtype, DEV, training=True, state=True)
    _same_bits(after, _plan_run(fresh, m, dense, args, None, None), f"{rep}: dense call after windows against a fresh plan")
    # the modules clear the windows of their pooled plans themselves
    mod_first = _run(m, src, args, lengths, views=(rows, starts))
    (pooled,) = m.all_plans()
    assert pooled._views is None
    mod_dense = _run(m, dense, args, None)
    assert len(m.all_plans()) == 1
    m2 = LSTM(I, H, L, compute_dtype=dtype).to(DEV)
    m2.load_state_dict(m.state_dict())
    _same_bits(mod_dense, _run(m2, dense, args, None), f"{rep}: module, dense call after windows against a fresh module")
    assert torch.equal(mod_first["out"], first)
    assert plan.status() == 0 and pooled.status() == 0


# ---- 5. host checks --------------------------------------------------------------------------------------------------
def test_set_views_host_checks():
    import ctypes
    lib = cabi.load()
    B, T, I, H, L = 3, 5, 8, 32, 2
    S, Tsrc = 2, 9
    torch.manual_seed(0)
    m = LSTM(I, H, L).to(DEV)
    w = [[getattr(m, f"{n}_l{k}").detach() for k in range(L)] for n in ("weight_ih", "weight_hh", "bias_ih", "bias_hh")]
    src = _source(S, Tsrc, I)
    arr = lambda v: (ctypes.c_int32 * len(v))(*v)
    for state in (False, True):
        plan = cabi.LstmPlan(B, T, I, H, L, BF16, DEV, training=True, state=state)
        rows, starts = [1, 0, 1], [4, 0, 2]
        plan.set_views(rows, starts, S, Tsrc)
        want = plan.forward(src, *w)[0].clone()
        bad = {
            "null plan": (None, arr(rows), arr(starts), S, Tsrc),
            "exactly one": (plan._plan, arr(rows), None, S, Tsrc),
            "exactly one of": (plan._plan, None, arr(starts), S, Tsrc),
            "src_row[1] = 2 outside": (plan._plan, arr([0, 2, 0]), arr(starts), S, Tsrc),
            "src_row[0] = -1 outside": (plan._plan, arr([-1, 0, 0]), arr(starts), S, Tsrc),
            "t0[2] = -1": (plan._plan, arr(rows), arr([0, 0, -1]), S, Tsrc),
            "src_T = 0": (plan._plan, arr(rows), arr(starts), S, 0),
        }
        for msg, a in bad.items():
            assert lib.csn_lstm_plan_set_views(*a) == 1, msg
            assert msg.encode() in lib.csn_last_error(), (msg, lib.csn_last_error())
            assert torch.equal(plan.forward(src, *w)[0], want), f"{msg}: the earlier setting is no longer in force"
        # in the forward: a window that ends past the source, with T or with the lengths -- nothing is enqueued
        plan.set_views(rows, [5, 0, 2], S, Tsrc)         # 5 + 5 > 9
        y = torch.full((B, H), 7.0, device=DEV)
        rc = lib.csn_lstm_forward(plan._plan, cabi._ptr(src), src.stride(0), src.stride(1), cabi._ptr_array(w[0]),
                                  cabi._ptr_array(w[1]), cabi._ptr_array(w[2]), cabi._ptr_array(w[3]), None, None,
                                  plan._ws_ptr, cabi._ptr(y), None, None, None, cabi._stream())
        assert rc == 1 and b"ends past the source" in lib.csn_last_error()
        torch.cuda.synchronize()
        assert bool((y == 7.0).all())
        if state:
            plan.set_lengths([4, 5, 5])                  # the lengths came after the views: now it fits
            got = plan.forward(src, *w)[0]
            plan.set_lengths([5, 5, 5])                  # ... and no longer
            with pytest.raises(cabi.CsnError, match="ends past the source"):
                plan.forward(src, *w)
            assert bool(torch.isfinite(got).all())
        with pytest.raises(cabi.CsnError, match="2 rows and 3 starts"):
            plan.set_views([0, 1], [0, 0, 0], S, Tsrc)
        plan.set_views(None)
        assert plan.status() == 0
    # the modules
    x = src.clone().requires_grad_(True)
    with pytest.raises(ValueError, match="requires grad"):
        m(x, lengths=[5, 5, 5], views=([0, 1, 0], [0, 0, 0]))
    with pytest.raises(ValueError, match="need lengths"):
        m(src, views=([0, 1, 0], [0, 0, 0]))
    h = HipLSTM(I, H, L).to(DEV)
    with pytest.raises(ValueError, match="requires grad"):
        h.forward_views(x, ([0, 1, 0], [0, 0, 0]), [5, 5, 5])
    assert not m.all_plans() and not h.all_plans()      # refused before any plan or launch


# ---- 6. the fused step against the per-view step ---------------------------------------------------------------------
STEP = dict(B=4, C=32, T=64, n_global=2, n_local=4, global_len=40, local_len=24, hidden=32, layers=2, out_dim=48)


def _wrapper(dtype, seed):
    torch.manual_seed(seed)
    s = STEP
    backbone = Model(input_size=s["C"], lstm_size=s["hidden"], lstm_layers=s["layers"], output_size=s["hidden"],
                     include_top=False, compute_dtype=dtype)
    return MultiCropWrapper(backbone, DINOHead(s["hidden"], s["out_dim"], hidden_dim=64, bottleneck_dim=32)).to(DEV)


class _Float64Step(torch.nn.Module):
    """The float64 CPU restatement of one wrapped encoder: torch.nn.LSTM, the last step of every view (MultiCropWrapper
    replaces the Model's Linear by the identity, so there is none here), DINOHead."""

    def __init__(self, wrapper):
        super().__init__()
        s = STEP
        self.lstm = torch.nn.LSTM(s["C"], s["hidden"], num_layers=s["layers"], batch_first=True)
        self.head = DINOHead(s["hidden"], s["out_dim"], hidden_dim=64, bottleneck_dim=32)
        sd = {k.replace("backbone.lstm.", "lstm."): v.detach().cpu() for k, v in wrapper.state_dict().items()}
        self.load_state_dict(sd)
        self.double()

    def forward(self, views):
        feats = [self.lstm(v)[0][:, -1] for v in views]
        return torch.stack(feats), torch.stack([self.head(f) for f in feats])


def _loss_module(device, dtype=torch.float32):
    s = STEP
    return DINOLoss(s["out_dim"], s["n_global"] + s["n_local"], 0.04, 0.04, 0, 1).to(device=device, dtype=dtype)


def _step(student, teacher, eeg, starts, lengths, fused):
    """One student and teacher step as LstmDistillation.py runs it (accumulating direct gradients): features of the
    student backbone [V, B, hidden], the loss, every student gradient."""
    s = STEP
    feats = []
    hook = student.backbone.register_forward_hook(lambda mod, inp, out: feats.append(out.detach()))
    for mod in student.modules():
        if isinstance(mod, HipLSTM):
            mod.direct_grads = "accumulate"
    for p in student.parameters():
        p.grad = torch.zeros_like(p)
    n_g = s["n_global"]
    if fused:
        with torch.no_grad():
            t_out = teacher.forward_views(eeg, starts[:n_g], lengths[:n_g])
        s_out = student.forward_views(eeg, starts, lengths)
    else:
        views = [eeg[:, a:a + n] for a, n in zip(starts, lengths)]
        with torch.no_grad():
            t_out = torch.stack([teacher(v.contiguous()) for v in views[:n_g]], dim=0)
        s_out = torch.stack([student(v.contiguous()) for v in views], dim=0)
    loss = _loss_module(DEV)(s_out, t_out, 0)
    loss.backward()
    hook.remove()
    torch.cuda.synchronize()
    feat = torch.cat(feats).reshape(len(lengths), eeg.shape[0], -1)
    return feat, loss.detach(), {k: p.grad.detach().clone() for k, p in student.named_parameters() if p.requires_grad}


@pytest.mark.parametrize("dtype", [BF16, F32], ids=["bf16", "f32"])
def test_fused_step_against_per_view_step_and_float64(dtype):
    """(a) per view, (b) MultiCropWrapper.forward_views, (c) float64 on the CPU, the yardstick.  Measured on one MI355X
    (DESIGN.md section 19): features max |difference| bf16 5.4e-4 in (a) and (b), float32 3.9e-8; LSTM gradients relative
    norm bf16 8.4e-3 .. 1.1e-2 in both, float32 (a) 0.94 .. 1.10e-6, (b) 1.10 .. 1.36e-6; loss error bf16 2.0e-3 / 2.0e-3,
    float32 2.97e-7 / 2.97e-7; head gradients bf16 7.24e-3 / 7.24e-3, float32 9.56e-7 / 1.02e-6; the losses of (a) and
    (b) were equal to the last bit."""
    s = STEP
    student, teacher = _wrapper(dtype, seed=11), _wrapper(dtype, seed=12)
    teacher.load_state_dict(student.state_dict())
    for p in teacher.parameters():
        p.requires_grad = False
    student.train(), teacher.train()
    g = torch.Generator(device="cpu").manual_seed(13)
    eeg = torch.randn(s["B"], s["T"], s["C"], generator=g).to(DEV)
    starts, lengths = temporal_crops(eeg, s["n_global"], s["n_local"], s["global_len"], s["local_len"],
                                     rng=np.random.RandomState(14), as_views=True)
    assert lengths == [40, 40, 24, 24, 24, 24]
    # (c) float64 on the CPU: the yardstick
    ref_s, ref_t = _Float64Step(student), _Float64Step(teacher)
    views64 = [eeg.double().cpu()[:, a:a + n] for a, n in zip(starts, lengths)]
    with torch.no_grad():
        _, t64 = ref_t(views64[:s["n_global"]])
    f64, s64 = ref_s(views64)
    loss64 = _loss_module("cpu", torch.float64)(s64, t64, 0)
    loss64.backward()
    g64 = {("backbone." + k if k.startswith("lstm.") else k): p.grad for k, p in ref_s.named_parameters() if p.requires_grad}
    # (a) per view, (b) fused
    student_a = _wrapper(dtype, seed=11)          # (a weight-normalised module does not deep-copy)
    student_a.load_state_dict(student.state_dict())
    student_a.train()
    f_a, loss_a, g_a = _step(student_a, teacher, eeg, starts, lengths, fused=False)
    f_b, loss_b, g_b = _step(student, teacher, eeg, starts, lengths, fused=True)
    assert set(g_a) == set(g_b) == set(g64)
    rel = lambda got, want: float((got.double().cpu() - want).norm() / want.norm())
    # the backbone: the bounds every LSTM output keeps against float64 (tests/test_gpu_lstm_lengths.py::_bounds)
    elem, relb = ll._bounds(dtype)
    feat_err = {tag: float((f.double().cpu() - f64.detach()).abs().max()) for tag, f in (("a", f_a), ("b", f_b))}
    print(f"measured fused step {dtype}: features max |diff| vs float64: per-view {feat_err['a']:.3e} fused {feat_err['b']:.3e} (bound {elem:g})")
    lstm_keys = [k for k in g64 if k.startswith("backbone.lstm.")]
    lstm_err = {k: (rel(g_a[k], g64[k]), rel(g_b[k], g64[k])) for k in lstm_keys}
    print("measured LSTM gradients rel vs float64 (per-view / fused): " + " ".join(f"{k.split('.')[-1]} {a:.2e}/{b:.2e}" for k, (a, b) in lstm_err.items()))
    # behind the head: (a) against float64 is the measure, (b) may be twice as far off
    loss_err = (abs(float(loss_a) - float(loss64.detach())), abs(float(loss_b) - float(loss64.detach())))
    head_keys = [k for k in g64 if not k.startswith("backbone.lstm.")]
    cat = lambda gr: torch.cat([gr[k].double().cpu().reshape(-1) for k in head_keys])
    head_err = (rel(cat(g_a), cat(g64)), rel(cat(g_b), cat(g64)))
    print(f"measured loss {float(loss64):.9f}: |error| per-view {loss_err[0]:.3e} fused {loss_err[1]:.3e}; "
          f"head gradients rel per-view {head_err[0]:.3e} fused {head_err[1]:.3e}; "
          f"fused against per-view: loss {abs(float(loss_a) - float(loss_b)):.3e}")
    assert feat_err["b"] < elem, feat_err
    for k, (_, b) in lstm_err.items():
        assert b < relb, (k, b)
    assert loss_err[1] <= 2 * loss_err[0], loss_err
    assert head_err[1] <= 2 * head_err[0], head_err
    for mod in (student, teacher):
        for pl in mod.backbone.lstm.all_plans():
            assert pl.status() == 0
    # one pass: the student ran ONE plan of 6 B rows and 40 steps, the teacher one of 2 B rows
    assert [(pl.desc.B, pl.desc.T) for pl in student.backbone.lstm.all_plans()] == [(6 * s["B"], 40)]
    assert [(pl.desc.B, pl.desc.T) for pl in teacher.backbone.lstm.all_plans() if pl.state] == [(2 * s["B"], 40)]


def test_forward_views_with_batchnorm_head_runs_the_head_per_view():
    s = STEP
    torch.manual_seed(21)
    backbone = Model(input_size=s["C"], lstm_size=s["hidden"], lstm_layers=s["layers"], output_size=s["hidden"],
                     include_top=False, compute_dtype=F32)
    w = MultiCropWrapper(backbone, DINOHead(s["hidden"], s["out_dim"], use_bn=True, hidden_dim=64, bottleneck_dim=32)).to(DEV)
    w.train()
    eeg = torch.randn(s["B"], s["T"], s["C"], device=DEV)
    starts, lengths = [3, 20, 40], [40, 40, 24]
    with torch.no_grad():
        per_view = torch.stack([w(eeg[:, a:a + n].contiguous()) for a, n in zip(starts, lengths)])
        fused = w.forward_views(eeg, starts, lengths)
    assert fused.shape == per_view.shape == (3, s["B"], s["out_dim"])
    # batch statistics per view, not over all rows (which would move the outputs by O(0.1)).  Float32 LSTM rows agree to
    # 2e-5 at the worst (ll._bounds); BatchNorm over 4 rows divides by a standard deviation of the order of the
    # features' spread, the unit-norm bottleneck and the unit-norm prototypes add no gain: 1e-3 holds a factor 50
    assert float((fused - per_view).abs().max()) < 1e-3
    rows, t0, n = view_rows(starts, lengths, s["B"])
    assert len(rows) == 3 * s["B"]


# ---- 7. the trainer --------------------------------------------------------------------------------------------------
def _train(tmp_path, monkeypatch, tag, *flags):
    import LstmDistillation
    from cerebralsignalnetworks_amd import trainer
    seen, real = [], trainer.check_device_status

    def spy(model, *a, **k):
        torch.cuda.synchronize()
        seen.append((model, [pl.status() for mod in model.modules() if isinstance(mod, HipLSTM) for pl in mod.all_plans()]))
        return real(model, *a, **k)

    monkeypatch.setattr(trainer, "check_device_status", spy)
    history = LstmDistillation.main(["--synthetic", "64", "--batch_size_per_gpu", "8", "--epochs", "1", "--seed", "43",
                                     "--log_dir", str(tmp_path / tag), *flags])
    monkeypatch.setattr(trainer, "check_device_status", real)
    assert len(seen) == 2                           # student and teacher
    for model, status in seen:
        assert status and all(v == 0 for v in status), status
    return history, seen


def test_trainer_fused_views(tmp_path, monkeypatch):
    history, seen = _train(tmp_path, monkeypatch, "fused", "--fused_views")
    assert len(history) == 1 and np.isfinite(history).all()
    # one plan of (2 + 4) * 8 rows and 300 steps for the student, one of 2 * 8 rows for the teacher
    student, teacher = seen[0][0], seen[1][0]
    assert [(pl.desc.B, pl.desc.T) for pl in student.backbone.lstm.all_plans()] == [(48, 300)]
    assert [(pl.desc.B, pl.desc.T) for pl in teacher.backbone.lstm.all_plans()] == [(16, 300)]
    per_sample, _ = _train(tmp_path, monkeypatch, "per_sample", "--fused_views", "--per_sample_crops")
    assert len(per_sample) == 1 and np.isfinite(per_sample).all()
    assert per_sample != history                    # other crops


def test_trainer_default_path_is_untouched(tmp_path, monkeypatch):
    """Without the flag the step is the per-view code it was: it never reaches the window forms, and it repeats itself."""
    def refuse(*a, **k):
        raise AssertionError("the default path reached the fused-views code")

    monkeypatch.setattr(MultiCropWrapper, "forward_views", refuse)
    monkeypatch.setattr(HipLSTM, "forward_views", refuse)
    monkeypatch.setattr(cabi.LstmPlan, "set_views", refuse)
    first, seen = _train(tmp_path, monkeypatch, "default_1")
    second, _ = _train(tmp_path, monkeypatch, "default_2")
    assert len(first) == 1 and np.isfinite(first).all()
    assert first == second
    student = seen[0][0]
    plans = student.backbone.lstm.all_plans()
    assert sorted({(pl.desc.B, pl.desc.T) for pl in plans}) == [(8, 200), (8, 300)] and not any(pl.state for pl in plans)
