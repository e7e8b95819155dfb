"""GPU: the bidirectional LSTM's inter-layer dropout -- csn_lstm_plan_set_output_dropout and ``BiLSTM.dropout``.

A plan with an output dropout differs from the plan without it in its two layout passes only, so (1) its y_all is
``where(keep, y_plain * s, 0)`` and every other output the plain plan's, and its backward is the plain plan's backward fed
``where(keep, dy * s, 0)``, BIT FOR BIT; (2) BiLSTM with the attribute set equals the stack composed from single-layer LSTM
modules with torch mask ops between the layers, bit for bit, and (3) the float64 composition within the project's LSTM
bounds; then (4) modes and seeds."""
import numpy as np
import pytest
import torch
from torch.nn.utils.rnn import pack_padded_sequence, pad_packed_sequence

import bilstm_dropout_reference as bdref
import bilstm_reference as bref
import dropout_reference as dref
import test_bilstm_dropout_cpu as cpu_checks
import test_gpu_lstm_state as st
from cerebralsignalnetworks_amd import cabi, BiLSTM, LSTM, lstm_model

pytestmark = pytest.mark.gpu

DEV, BF16, F32 = st.DEV, st.BF16, st.F32
NAN, INF = float("nan"), float("inf")
PS = (0.1, 0.5, 0.9, 1.0)
FIRSTS = (0, 2 ** 32 - 64, 2 ** 40 + 4)
# one trip of the two masked kernels' grid: 4096 blocks of 256 threads, four elements each (csrc/lstm_boundary.hip)
ONE_TRIP = 4096 * 256 * 4


# ---- 1. plan identity ---------------------------------------------------------------------------------------------------
def _inputs(B, T, I, H, seed=0, L=1):
    torch.manual_seed(seed)
    ref = torch.nn.LSTM(I, H, L, batch_first=True)
    w = [[getattr(ref, f"{n}_l{k}").detach().to(DEV) for k in range(L)] for n in bref.NAMES]
    g = torch.Generator().manual_seed(seed + 1)
    a = dict(x=torch.randn(B, T, I, generator=g), dy_all=0.1 * torch.randn(B, T, H, generator=g), dy_last=torch.randn(B, H, generator=g),
             h0=0.5 * torch.randn(L, B, H, generator=g), c0=torch.randn(L, B, H, generator=g), dh_n=torch.randn(L, B, H, generator=g),
             dc_n=torch.randn(L, B, H, generator=g))
    return w, {k: v.to(DEV) for k, v in a.items()}


def _call(plan, w, a, lengths, y_view=None, dy_view=None):
    """forward + backward with every argument the plan takes (the state arguments and the lengths on a state plan only);
    every result.  y_view / dy_view: pitched views."""
    d = plan.desc
    st_in = dict(h0=a["h0"], c0=a["c0"]) if plan.state else {}
    if plan.state:
        plan.set_lengths(lengths)
    else:
        assert lengths is None
    outs = plan.forward(a["x"], *w, want_all=y_view is None, want_state=plan.state, y_all=y_view, **st_in)
    out = dict(zip(("y_last", "y_all", "h_n", "c_n"), outs), dx=torch.full((d.B, d.T, d.I), NAN, device=DEV))
    st_bwd = {}
    if plan.state:
        out.update(dh0=torch.empty(d.L, d.B, d.H, device=DEV), dc0=torch.empty(d.L, d.B, d.H, device=DEV))
        st_bwd = dict(dh_n=a["dh_n"], dc_n=a["dc_n"], dh0=out["dh0"], dc0=out["dc0"])
    grads = [[torch.empty_like(p) for p in group] for group in w]
    plan.backward(a["dy_last"], a["dy_all"] if dy_view is None else dy_view, grads, dx=out["dx"], **st_bwd)
    out.update({f"{n}_l{k}": t for n, group in zip(bref.NAMES, grads) for k, t in enumerate(group)})
    return out


LAYOUTS = {            # name -> (pitch, offset of the view) in units of (H, elements)
    "pitch_H": lambda H: (H, 0),
    "pitch_2H_at_H": lambda H: (2 * H, H),
    "pitch_2H+4": lambda H: (2 * H + 4, 0),
}


def _check_identity(plain, drop, w, a, lengths, layout, p, first, seed=0x1234567890ABCDEF, sub=3):
    """One call of `drop` under (layout, p, first) against `plain`, a plan of the same flags that never heard of the symbol."""
    d = drop.desc
    B, T, H = d.B, d.T, d.H
    pitch, off = LAYOUTS[layout](H)
    what = (layout, p, first, lengths is not None)
    s = dref.scale(p)
    keep = bdref.plan_keep(seed, sub, p, first + off, pitch, B, T, H).to(DEV)
    valid = torch.ones(B, T, 1, dtype=torch.bool, device=DEV)
    if lengths is not None:
        valid = (torch.arange(T, device=DEV)[None, :] < torch.tensor(lengths, device=DEV)[:, None])[:, :, None]
    live = keep & valid
    zeros = torch.zeros(B, T, H, device=DEV)
    masked = lambda t: torch.where(live, t * s, zeros) if np.isfinite(s) else zeros      # noqa: E731
    assert p == 1.0 or (0 < int(keep.sum()) < keep.numel())
    want = _call(plain, w, dict(a, dy_all=masked(a["dy_all"])), lengths)
    want["y_all"] = masked(want["y_all"])
    # the caller's tensors: NaN in the gaps and in the other half; NaN / Inf in dy at the dropped and the padded elements
    ybuf = torch.full((B, T, pitch), NAN, device=DEV)
    dybuf = torch.full((B, T, pitch), NAN, device=DEV)
    dy = torch.where(live, a["dy_all"], torch.full_like(zeros, NAN))
    dy[:, ::2] = torch.where(live, a["dy_all"], torch.full_like(zeros, INF))[:, ::2]
    dybuf[:, :, off:off + H] = dy
    drop.set_io(pitch, pitch, False)
    drop.set_output_dropout(p, seed, sub, first + off, pitch)
    got = _call(drop, w, a, lengths, y_view=ybuf[:, :, off:off + H], dy_view=dybuf[:, :, off:off + H])
    got["y_all"] = ybuf[:, :, off:off + H]
    outside = torch.ones(pitch, dtype=torch.bool, device=DEV)
    outside[off:off + H] = False
    assert torch.isnan(ybuf[:, :, outside]).all(), what                 # gaps and the other half are untouched
    assert set(got) == set(want)
    for k in want:
        assert torch.equal(got[k], want[k]), (what, k, float((got[k] - want[k]).abs().max()))
        assert bool(torch.isfinite(got[k]).all()), (what, k)
    for b, n in enumerate(lengths or ()):
        assert not got["y_all"][b, n:].any() and not got["dx"][b, n:].any(), (what, b)


def _ragged(B, T):
    n = np.random.default_rng(B * 100 + T).integers(0, T + 1, B).tolist()
    n[0], n[B - 1] = T, 0
    return [int(v) for v in n]


def _pair(B, T, I, H, dtype, reverse, resident=False, L=1, state=True, dropout=False):
    flags = dict(training=True, state=state, reverse=reverse, resident=resident, dropout=dropout)
    return cabi.LstmPlan(B, T, I, H, L, dtype, DEV, **flags), cabi.LstmPlan(B, T, I, H, L, dtype, DEV, **flags)


@pytest.mark.parametrize("dtype", [BF16, F32], ids=["bf16", "f32"])
@pytest.mark.parametrize("reverse", [False, True], ids=["plain", "reverse"])
@pytest.mark.parametrize("shape", [(3, 7, 8, 32), (5, 9, 16, 64), (2, 40, 8, 32)], ids=str)      # (2, 40, ...) crosses a chunk
def test_output_dropout_plan_identity(shape, reverse, dtype):
    B, T, I, H = shape
    plain, drop = _pair(B, T, I, H, dtype, reverse)
    cpu_checks.check_set_output_dropout_arguments(cabi.load(), drop._plan, H)
    w, a = _inputs(B, T, I, H)
    i = 0
    for layout in LAYOUTS:
        for lengths in (None, _ragged(B, T)):
            _check_identity(plain, drop, w, a, lengths, layout, PS[i % len(PS)], FIRSTS[i % len(FIRSTS)])
            i += 1
    # p = 0 after p > 0 on the same plan: a fresh plan's bits, on its dense defaults
    drop.set_io()
    drop.set_output_dropout(0.0)
    for lengths in (None, _ragged(B, T)):
        got, want = _call(drop, w, a, lengths), _call(plain, w, a, lengths)
        for k in want:
            assert torch.equal(got[k], want[k]), ("p = 0 again", k)
    torch.cuda.synchronize()
    assert plain.status() == 0 and drop.status() == 0


@pytest.mark.parametrize("p", PS)
@pytest.mark.parametrize("first", FIRSTS)
def test_every_p_and_first(p, first):
    B, T, I, H = 3, 7, 8, 32
    plain, drop = _pair(B, T, I, H, BF16, True)
    w, a = _inputs(B, T, I, H, seed=2)
    _check_identity(plain, drop, w, a, _ragged(B, T), "pitch_2H_at_H", p, first)


# One plan per path csn_lstm_plan_path returns among those the BiLSTM tests reach (tests/test_gpu_bilstm.py PLAN_CASES and
# MODEL_SHAPES, tests/test_gpu_lstm_resident.py): the setter is a feature of any plan, whatever its L, state or path, and
# the launch sites it changes are shared by all of them.  name -> ((B, T, I, H, L), dtype, plan flags, expected path or
# (path, forward kernel, backward kernel), environment)
PATH4 = (4, "lstm_fwd_f32_persist_kernel", "lstm_bwd_f32_persist_kernel")
PATH_CASES = {
    "path0_bf16": ((8, 40, 24, 96, 1), BF16, {}, 0, {}),
    "path0_f32": ((20, 17, 24, 128, 1), F32, {}, 0, {}),
    "path1_l5": ((8, 30, 16, 128, 5), BF16, {}, st.IL, {}),
    "path3": ((64, 33, 128, 256, 1), BF16, {}, 3, {}),
    "path3_ns_forward": ((65, 33, 128, 1024, 2), BF16, {}, st.P3_NS, {}),
    "path4_f32_stateless": ((64, 9, 32, 128, 2), F32, dict(state=False), PATH4, {}),
    "path5_resident": ((16, 20, 96, 96, 1), BF16, dict(resident=True), 5, {}),
    # more elements than one trip of the kernels' grid-stride loop
    "two_trips": ((96, 90, 8, 512, 1), BF16, {}, None, {}),
    # independent of csn_lstm_plan_set_dropout: a plan may carry both (both plans of the pair carry the in-plan dropout)
    "with_in_plan_dropout": ((8, 40, 24, 96, 2), BF16, dict(dropout=True), 0, {}),
}


@pytest.mark.parametrize("name", list(PATH_CASES))
def test_output_dropout_on_every_path(name, monkeypatch):
    (B, T, I, H, L), dtype, flags, expect, env = PATH_CASES[name]
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    if expect is None:
        assert B * T * H > ONE_TRIP
    state = flags.get("state", True)
    w, a = _inputs(B, T, I, H, seed=4, L=L)
    for reverse in (False, True):
        plain, drop = _pair(B, T, I, H, dtype, reverse, L=L, **flags)
        seen = (drop.path(),) + drop.kernel_names()
        assert seen == (plain.path(),) + plain.kernel_names()
        assert expect is None or (seen == expect if isinstance(expect, tuple) else seen[0] == expect), (name, seen)
        lengths = _ragged(B, T) if reverse and state else None
        if flags.get("dropout"):
            off = _call(plain, w, a, lengths)
            for plan in (plain, drop):
                plan.set_dropout(0.3, 77, 1)
            assert not torch.equal(_call(plain, w, a, lengths)["y_all"], off["y_all"])      # the in-plan mask is on
        _check_identity(plain, drop, w, a, lengths, "pitch_2H_at_H", 0.5, B * T * 2 * H)
        torch.cuda.synchronize()
        assert drop.status() == 0 and plain.status() == 0


def test_misaligned_tensors_are_refused_before_anything_is_written():
    B, T, I, H = 3, 7, 8, 32
    _, plan = _pair(B, T, I, H, BF16, False)
    w, a = _inputs(B, T, I, H)
    lib = cabi.load()
    pitch = 2 * H + 4
    plan.set_io(pitch, pitch, False)
    plan.set_output_dropout(0.5, 1, 0, 0, pitch)
    plan.set_lengths(None)
    ybuf = torch.full((B * T * pitch + 4,), NAN, device=DEV)
    y_last = torch.full((B, H), NAN, device=DEV)
    x = a["x"].contiguous()
    args = lambda y: (plan._plan, cabi._ptr(x), x.stride(0), x.stride(1), *(cabi._ptr_array(g) for g in w), None, None,    # noqa: E731
                      plan._ws_ptr, cabi._ptr(y_last), cabi._ptr(y), None, None, cabi._stream())
    assert lib.csn_lstm_forward(*args(ybuf[1:])) == 1 and b"y_all must be 16-B aligned" in lib.csn_last_error()
    torch.cuda.synchronize()
    assert torch.isnan(ybuf).all() and torch.isnan(y_last).all()
    assert lib.csn_lstm_forward(*args(ybuf[4:])) == 0                   # (16 bytes further on it runs)
    torch.cuda.synchronize()
    assert torch.isfinite(y_last).all() and torch.isnan(ybuf[:4]).all()
    dybuf = torch.zeros(B * T * pitch + 4, device=DEV)
    dx = torch.full((B, T, I), NAN, device=DEV)
    grads = [[torch.full_like(p, NAN) for p in group] for group in w]
    rc = lib.csn_lstm_backward(plan._plan, None, cabi._ptr(dybuf[1:]), None, None, plan._ws_ptr, *(cabi._ptr_array(g) for g in grads),
                               cabi._ptr(dx), None, None, cabi._stream())
    assert rc == 1 and b"dy_all must be 16-B aligned" in lib.csn_last_error()
    torch.cuda.synchronize()
    assert torch.isnan(dx).all() and all(torch.isnan(g[0]).all() for g in grads)
    assert plan.status() == 0


# ---- 2. BiLSTM = the composition with torch mask ops, bit for bit -------------------------------------------------------
MODEL_CASES = {
    "l2_bf16": ((5, 9, 16, 64, 2), BF16, False),
    "l3_f32": ((3, 7, 8, 32, 3), F32, False),
    "l2_bf16_path3": ((64, 33, 128, 256, 2), BF16, False),
    "l2_bf16_resident": ((4, 12, 8, 32, 2), BF16, True),
}


def _model(shape, dtype, resident=False, seed=0, p=0.5):
    B, T, I, H, L = shape
    torch.manual_seed(seed)
    m = BiLSTM(I, H, L, compute_dtype=dtype, resident=resident).to(DEV)
    m.dropout, m.dropout_subsequence = p, 5
    g = torch.Generator().manual_seed(seed + 1)
    x = torch.randn(B, T, I, generator=g)
    h0 = 0.5 * torch.randn(2 * L, B, H, generator=g)
    c0, dh, dc = (torch.randn(2 * L, B, H, generator=g) for _ in range(3))
    dy = torch.randn(B, T, 2 * H, generator=g)
    return m, [t.to(DEV) for t in (x, h0, c0, dy, dh, dc)]


def _drawn(m, seed):
    """(p, seed, subsequence) the module's next call draws after torch.manual_seed(seed), which is set again."""
    torch.manual_seed(seed)
    drop = lstm_model._draw_dropout(m)
    torch.manual_seed(seed)
    return drop


def _run_model(m, args, lengths, hx, seed):
    x, h0, c0, dy, dh, dc = args
    drop = _drawn(m, seed)
    res = bref.run(lambda xx, s: m(xx, s, lengths=lengths), m.named_parameters(), x, h0 if hx else None, c0 if hx else None, dy, dh, dc)
    return res, drop


def _run_composition(m, layers, call, args, lengths, hx, drop, device=DEV):
    x, h0, c0, dy, dh, dc = args
    B, T, H, L = x.shape[0], x.shape[1], m.hidden_size, m.num_layers
    masks, s = None, 1.0
    if drop is not None:
        p, seed, sub = drop
        masks, s = [k.to(device) for k in bdref.interface_masks(seed, sub, p, L, B, T, H)], dref.scale(p)
    return bref.run(lambda xx, st_: bdref.composed(layers, call, xx, st_, lengths, masks, s), bref.composed_named_params(layers),
                    x, h0 if hx else None, c0 if hx else None, dy, dh, dc)


def _same(got, want, what):
    assert set(got) == set(want)
    for k in want:
        assert torch.equal(got[k], want[k]), (what, k, float((got[k] - want[k]).abs().max()))


@pytest.mark.parametrize("name", list(MODEL_CASES))
def test_bilstm_dropout_is_the_composition_bit_for_bit(name):
    shape, dtype, resident = MODEL_CASES[name]
    B, T, I, H, L = shape
    m, args = _model(shape, dtype, resident)
    layers = bref.single_layer_modules(m, lambda i, h: LSTM(i, h, 1, compute_dtype=dtype, resident=resident).to(DEV))
    ragged = _ragged(B, T)
    for k, (lengths, hx) in enumerate(((None, True), (None, False), (ragged, True))):
        got, drop = _run_model(m, args, lengths, hx, seed=20 + k)
        assert drop is not None and drop[0] == 0.5 and drop[2] == 5
        want = _run_composition(m, layers, bref.call_lengths, args, lengths, hx, drop)
        _same(got, want, f"{name} lengths={lengths is not None} hx={hx}")
        # the mask reached the result: the same call without it differs
        plain = _run_composition(m, layers, bref.call_lengths, args, lengths, hx, None)
        assert not torch.equal(plain["out"], want["out"]) and not torch.equal(plain["dx"], want["dx"])
    # a PackedSequence = the padded call with its lengths and the same draw
    lens = [max(n, 1) for n in ragged]
    x, h0, c0, dy, dh, dc = args
    want, _ = _run_model(m, args, lens, True, seed=30)
    torch.manual_seed(30)
    xr = x.clone().requires_grad_(True)
    for q in m.parameters():
        q.grad = None
    out_p, (h_n, c_n) = m(pack_padded_sequence(xr, torch.tensor(lens), batch_first=True, enforce_sorted=False), (h0, c0))
    out, _ = pad_packed_sequence(out_p, batch_first=True, total_length=T)
    torch.autograd.backward([out, h_n, c_n], [dy, dh, dc])
    got = dict(out=out.detach(), h_n=h_n.detach(), c_n=c_n.detach(), dx=xr.grad, **{k: q.grad for k, q in m.named_parameters()})
    for k, v in got.items():
        assert torch.equal(v, want[k]), (name, "packed", k)
    torch.cuda.synchronize()
    assert m.all_plans() and all(pl.status() == 0 and not pl.busy for pl in m.all_plans())
    assert all(pl.resident == resident for pl in m.all_plans())


# ---- 3. against the float64 composition ---------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["v1_h96", "f32_h128"])
@pytest.mark.parametrize("ragged", [False, True], ids=["dense", "ragged"])
def test_bilstm_dropout_matches_the_float64_composition(name, ragged):
    """Bounds: test_gpu_lstm_state._bounds as they are (outputs and states max |difference| 3e-2 bf16 / 2e-5 float32;
    gradients relative norm 4e-2 / 1e-5)."""
    shape, dtype = {"v1_h96": ((8, 40, 24, 96, 2), BF16), "f32_h128": ((20, 17, 24, 128, 2), F32)}[name]
    B, T, I, H, L = shape
    m, args = _model(shape, dtype, seed=2)
    lengths = _ragged(B, T) if ragged else None
    got, drop = _run_model(m, args, lengths, True, seed=40)
    torch.cuda.synchronize()
    ref = torch.nn.LSTM(I, H, L, batch_first=True, bidirectional=True).double()
    ref.load_state_dict({k: v.double().cpu() for k, v in m.state_dict().items()})
    layers = bref.single_layer_modules(ref, lambda i, h: torch.nn.LSTM(i, h, 1, batch_first=True).double())
    want = _run_composition(m, layers, bref.call_packed, [t.double().cpu() for t in args], lengths, True, drop, device="cpu")
    elem, rel = st._bounds(dtype)
    line, failures = [], []
    for k, w in want.items():
        g = got[k].double().cpu()
        if k in ("out", "h_n", "c_n"):
            err, bound = float((g - w).abs().max()), elem
        else:
            err, bound = float((g - w).norm() / w.norm()), rel
        line.append(f"{k} {err:.2e}")
        if not err < bound:
            failures.append((k, err, bound))
    print(f"measured vs the float64 composition {name} {'ragged' if ragged else 'dense'}: " + " ".join(line))
    assert not failures, failures


# ---- 4. modes and seeds -------------------------------------------------------------------------------------------------
def test_modes_and_seeds():
    shape, dtype, _ = MODEL_CASES["l2_bf16"]
    m, args = _model(shape, dtype, seed=3)
    off, _ = _model(shape, dtype, seed=3, p=0.0)
    _same(dict(m.state_dict()), dict(off.state_dict()), "twins")
    lengths = _ragged(shape[0], shape[1])
    base, none = _run_model(off, args, lengths, True, seed=1)
    assert none is None
    m.eval()
    got, none = _run_model(m, args, lengths, True, seed=1)
    assert none is None
    _same(got, base, "eval() = p 0")
    m.train()
    a, da = _run_model(m, args, lengths, True, seed=7)
    b, db = _run_model(m, args, lengths, True, seed=7)
    assert da == db
    _same(a, b, "same manual_seed")
    assert not torch.equal(a["out"], base["out"])
    torch.manual_seed(7)
    with torch.no_grad():                              # on in train() also without a graph
        out, _ = m(args[0], (args[1], args[2]), lengths=lengths)
        again, _ = m(args[0], (args[1], args[2]), lengths=lengths)
    assert torch.equal(out, a["out"]) and not torch.equal(again, out)       # consecutive calls draw again
    assert not any(pl.busy for pl in m.all_plans())


def test_output_gradient_at_an_odd_storage_offset():
    """A dense float32 gradient whose storage starts 4 bytes past a 16-byte boundary (which neither a pitched dy_all of the
    binding nor the 16-byte loads of the masked pass take) is copied once: the bits of the aligned one, with dropout on."""
    shape, dtype, _ = MODEL_CASES["l2_bf16"]
    B, T, I, H, L = shape
    m, (x, h0, c0, dy, dh, dc) = _model(shape, dtype, seed=5)
    odd = torch.empty(dy.numel() + 1, device=DEV)[1:].view_as(dy).copy_(dy)
    assert odd.is_contiguous() and odd.data_ptr() % 16 == 4 and dy.data_ptr() % 16 == 0
    res = []
    for grad in (dy, odd):
        torch.manual_seed(11)
        xr = x.clone().requires_grad_(True)
        for q in m.parameters():
            q.grad = None
        out, _ = m(xr, (h0, c0))
        out.backward(grad)
        res.append(dict(dx=xr.grad, **{k: q.grad for k, q in m.named_parameters()}))
    _same(res[1], res[0], "odd offset")
    assert bool(res[0]["dx"].any())


def test_bilstm_dropout_on_a_side_stream_with_late_inputs():
    """The masked layout passes run on the stream of their call: BiLSTM with dropout on, forward and backward inside
    `with torch.cuda.stream(s)`, x, h0, c0 and the output gradients arriving late behind a Delay, outputs cloned and inputs
    poisoned directly behind each call (tests/stream_order.py): the bits of the synchronised run on the default stream."""
    import stream_order as so
    import test_gpu_stream_order as gso
    shape, dtype, _ = MODEL_CASES["l2_bf16_path3"]
    m, args = _model(shape, dtype, seed=6)
    lengths = _ragged(shape[0], shape[1])
    ins = dict(zip(("x", "h0", "c0", "dy", "dh", "dc"), args))
    params = dict(m.named_parameters())

    def run(a, stream):
        with torch.cuda.stream(stream):
            x, h0, c0 = (a[k].detach().requires_grad_(True) for k in ("x", "h0", "c0"))
            for q in params.values():
                q.grad = None
            torch.manual_seed(12)
            out, (h_n, c_n) = m(x, (h0, c0), lengths=lengths)
            snaps = so.snapshot_then_poison(stream, {"out": out.detach(), "h_n": h_n.detach(), "c_n": c_n.detach()},
                                            [a[k].data for k in ("x", "h0", "c0")])
            torch.autograd.backward([out, h_n, c_n], [a["dy"], a["dh"], a["dc"]])
            grads = {"dx": x.grad, "dh0": h0.grad, "dc0": c0.grad, **{k: q.grad for k, q in params.items()}}
            snaps.update(so.snapshot_then_poison(stream, grads, [a[k] for k in ("dy", "dh", "dc")]))
        return snaps
    d = torch.cuda.default_stream()
    want = gso._synced(lambda: run(gso._clone(ins), d))
    m.dropout = 0.0
    assert not torch.equal(gso._synced(lambda: run(gso._clone(ins), d))["out"], want["out"])     # the mask is in `want`
    m.dropout = 0.5
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        a = gso._clone(ins)
        s.synchronize()
        _, t_host = so.timed(lambda: run(a, s))
        s.synchronize()
        for pl in m.all_plans():
            gso._forget_workspace(pl)
    delay, late = so.late_all(s, ins, so.delay_ms_for(t_host))
    snaps = run(late, s)
    s.synchronize()
    so.assert_same_bits(snaps, want, "BiLSTM with dropout, late inputs on a side stream")
    assert all(pl.status() == 0 for pl in m.all_plans())


def test_two_outstanding_forwards_backpropagated_in_reverse_order():
    shape, dtype, _ = MODEL_CASES["l2_bf16"]
    m, args = _model(shape, dtype, seed=4)
    layers = bref.single_layer_modules(m, lambda i, h: LSTM(i, h, 1, compute_dtype=dtype).to(DEV))
    x, h0, c0, dy, dh, dc = args
    xs = (x, x.flip(0).contiguous())
    drops, outs, leaves = [], [], []
    torch.manual_seed(9)
    state = torch.get_rng_state()
    for xx in xs:
        drops.append(lstm_model._draw_dropout(m))
    torch.set_rng_state(state)
    params = [q for _, q in m.named_parameters()]
    for xx in xs:
        leaf = [t.clone().requires_grad_(True) for t in (xx, h0, c0)]
        out, (h_n, c_n) = m(leaf[0], (leaf[1], leaf[2]))
        outs.append((out, h_n, c_n))
        leaves.append(leaf)
    assert drops[0] != drops[1] and sum(pl.busy for pl in m.all_plans()) == 2 * 2 * m.num_layers
    grads = [None, None]
    for i in (1, 0):
        grads[i] = torch.autograd.grad(outs[i], leaves[i] + params, [dy, dh, dc])
    assert not any(pl.busy for pl in m.all_plans())
    for i, xx in enumerate(xs):
        want = _run_composition(m, layers, bref.call_lengths, [xx, h0, c0, dy, dh, dc], None, True, drops[i])
        got = dict(zip(("out", "h_n", "c_n"), (t.detach() for t in outs[i])))
        got.update(zip(("dx", "dh0", "dc0"), grads[i][:3]))
        got.update({k: g for (k, _), g in zip(m.named_parameters(), grads[i][3:])})
        _same(got, want, f"forward {i}")
