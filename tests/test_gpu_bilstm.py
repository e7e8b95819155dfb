"""GPU: the bidirectional LSTM -- CSN_LSTM_REVERSE plans, csn_lstm_plan_set_io, cerebralsignalnetworks_amd.BiLSTM.

A reverse plan runs the unchanged recurrence on internally reversed data, so it equals the plan without the bit on
explicitly reversed tensors BIT FOR BIT, outputs and every gradient (test 1); the pitch and the adding dx store equal the
dense, overwriting call (test 2); BiLSTM equals the stack composed from existing single-layer LSTM modules, torch.cat and
the reversal R of tests/bilstm_reference.py, bit for bit (test 3), and float64 nn.LSTM(bidirectional=True) within the
project's LSTM bounds (test 4); then its uses (test 5).  Every case checks the plans' path and kernels against a plan
without the bit, and the workspace status word."""
import os

import numpy as np
import pytest
import torch
from torch.nn.utils.rnn import pack_padded_sequence, pad_packed_sequence

import bilstm_reference as bref
import lstm_input_views as views
import test_bilstm_cpu as cpu_checks
import test_gpu_lstm_state as st
from cerebralsignalnetworks_amd import cabi, BiLSTM, LSTM, Model

pytestmark = pytest.mark.gpu

DEV, BF16, F32 = st.DEV, st.BF16, st.F32
R = bref.R


def _check_plans(plans):
    """A reverse plan (and a BiLSTM's plain ones) takes the path and kernels of the plan without the bits; status 0."""
    assert plans
    for plan in plans:
        d = plan.desc
        plain = cabi.LstmPlan(d.B, d.T, d.I, d.H, d.L, cabi.torch_dtype(d.dtype), DEV, training=plan.training, state=plan.state)
        assert (plan.path(),) + plan.kernel_names() == (plain.path(),) + plain.kernel_names(), (plan.key(), plan.path())
        assert plan.status() == 0


def _lengths(B, T, pattern, edges, seed=0):
    """The patterns of tests/test_gpu_lstm_lengths.py::_lengths, built the same way."""
    rng = np.random.default_rng(1000 + seed)
    if pattern == "all_1":
        n = [1] * B
    elif pattern == "random_with_zeros":
        n = rng.integers(0, T + 1, B).tolist()
        n[0], n[1 % B], n[B - 1] = T, 0, 0
        if B == 1:
            n[0] = T
    elif pattern == "chunk_edges":
        vals = [e for e in edges if e <= T] + [T, T - 1]
        n = [vals[i % len(vals)] for i in rng.permutation(B)]
    return [int(v) for v in n]


# ---- 1. a reverse plan = the plain plan on reversed data, bit for bit ----------------------------------------------------
# one case per branch of the layout passes: (shape, dtype, expected plan, environment) of test_gpu_lstm_state.CASES, and a
# stateless float32 plan on the exact-float32 weight-stationary path (4), which takes no state
PLAN_CASES = {name: st.CASES[name] + (True,) for name in ("v1_h96", "p1_l5", "ks_fused_h768_t32", "ks_gemm_i24_t31", "ns_fused_h1024_t33",
                                                          "chunk4_l3", "f32_h128", "f32_cell_v1")}
PLAN_CASES["f32_path4_stateless"] = ((64, 9, 32, 128, 2), F32, (4, "lstm_fwd_f32_persist_kernel", "lstm_bwd_f32_persist_kernel"), {}, False)
PATTERNS = (None, "all_1", "random_with_zeros", "chunk_edges")


def _plan_inputs(shape, state, seed=0):
    B, T, I, H, L = shape
    torch.manual_seed(seed)
    ref = torch.nn.LSTM(I, H, L, batch_first=True)
    w = [[getattr(ref, f"{n}_l{k}").detach().to(DEV) for k in range(L)] for n in bref.NAMES]
    g = torch.Generator().manual_seed(seed + 1)
    a = dict(x=torch.randn(B, T, I, generator=g), dy_all=0.1 * torch.randn(B, T, H, generator=g), dy_last=torch.randn(B, H, generator=g))
    if state:
        a.update(h0=0.5 * torch.randn(L, B, H, generator=g), c0=torch.randn(L, B, H, generator=g),
                 dh_n=torch.randn(L, B, H, generator=g), dc_n=torch.randn(L, B, H, generator=g))
    return w, {k: v.to(DEV) for k, v in a.items()}


def _plan_call(plan, w, a, lengths, x=None):
    """forward + backward through cabi.LstmPlan with every argument the plan takes; every result."""
    d = plan.desc
    if plan.state:
        plan.set_lengths(lengths)
    x = a["x"] if x is None else x
    outs = plan.forward(x, *w, want_all=True, h0=a.get("h0"), c0=a.get("c0"), want_state=plan.state)
    out = dict(zip(("y_last", "y_all", "h_n", "c_n"), outs))
    out["dx"] = torch.full((d.B, d.T, d.I), float("nan"), device=DEV)
    if plan.state:
        out.update(dh0=torch.empty(d.L, d.B, d.H, device=DEV), dc0=torch.empty(d.L, d.B, d.H, device=DEV))
    grads = [[torch.empty_like(p) for p in group] for group in w]
    plan.backward(a["dy_last"], a["dy_all"], grads, dx=out["dx"], dh_n=a.get("dh_n"), dc_n=a.get("dc_n"), dh0=out.get("dh0"),
                  dc0=out.get("dc0"))
    for n, group in zip(bref.NAMES, grads):
        out.update({f"{n}_l{k}": t for k, t in enumerate(group)})
    return out


def _same(got, want, what):
    assert set(got) == set(want)
    for k in want:
        assert torch.equal(got[k], want[k]), (what, k, float((got[k] - want[k]).abs().max()))


@pytest.mark.parametrize("name", list(PLAN_CASES))
def test_reverse_plan_is_the_plain_plan_on_reversed_data(name, monkeypatch):
    shape, dtype, expect, env, state = PLAN_CASES[name]
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    B, T, I, H, L = shape
    plain = cabi.LstmPlan(B, T, I, H, L, dtype, DEV, training=True, state=state)
    rev = cabi.LstmPlan(B, T, I, H, L, dtype, DEV, training=True, state=state, reverse=True)
    assert rev.reverse and rev.key() != plain.key()
    assert (rev.path(),) + rev.kernel_names() == (plain.path(),) + plain.kernel_names() == expect
    assert cabi.load().csn_lstm_plan_workspace_bytes(rev._plan) == cabi.load().csn_lstm_plan_workspace_bytes(plain._plan)
    w, a = _plan_inputs(shape, state)
    edges = (3, 4, 5) if name == "chunk4_l3" else (31, 32, 33)
    for pattern in (PATTERNS if state else PATTERNS[:1]):
        lengths = None if pattern is None else _lengths(B, T, pattern, edges)
        what = f"{name} {pattern}"
        got = _plan_call(rev, w, a, lengths)
        want = _plan_call(plain, w, dict(a, x=R(a["x"], lengths), dy_all=R(a["dy_all"], lengths)), lengths)
        want["y_all"], want["dx"] = R(want["y_all"], lengths), R(want["dx"], lengths)
        _same(got, want, what)
        # the padding of y_all and dx is exactly zero; NaN / Inf in the padding of x and dy_all is never read
        for b, n in enumerate(lengths or ()):
            assert not got["y_all"][b, n:].any() and not got["dx"][b, n:].any(), (what, b)
        if lengths is not None:
            poisoned = dict(a, x=a["x"].clone(), dy_all=a["dy_all"].clone())
            for b, n in enumerate(lengths):
                poisoned["x"][b, n:] = float("nan") if b % 2 else float("inf")
                poisoned["dy_all"][b, n:] = float("inf") if b % 2 else float("nan")
            _same(_plan_call(rev, w, poisoned, lengths), got, what + " NaN padding")
        # x as a strided view (16-byte loads from a time-major buffer; scalar loads from a base on 4 bytes)
        if pattern in (None, "random_with_zeros"):
            for view in ("time_major", "chan_slice_off1"):
                xv, dense = views.VIEWS[view](a["x"])
                assert torch.equal(dense, a["x"]) and torch.equal(xv, dense)
                _same(_plan_call(rev, w, a, lengths, x=xv), got, f"{what} {view}")
    torch.cuda.synchronize()
    for plan in (plain, rev):
        assert plan.status() == 0


# ---- 2. pitch and add ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["v1_h96", "chunk4_l3", "f32_h128"])
@pytest.mark.parametrize("reverse", [False, True], ids=["plain", "reverse"])
def test_pitch_and_add(name, reverse, monkeypatch):
    shape, dtype, _, env, _ = PLAN_CASES[name]
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    B, T, I, H, L = shape
    plan = cabi.LstmPlan(B, T, I, H, L, dtype, DEV, training=True, state=True, reverse=reverse)
    cpu_checks.check_set_io_arguments(cabi.load(), plan._plan, H)
    w, a = _plan_inputs(shape, True, seed=5)
    for lengths in (None, _lengths(B, T, "random_with_zeros", (3, 4, 5))):
        dense = _plan_call(plan, w, a, lengths)
        # y_all and dy_all as the right half of a [B,T,2H] buffer whose left half is poisoned; dx added onto a random tensor
        ybuf = torch.full((B, T, 2 * H), float("nan"), device=DEV)
        dybuf = torch.full((B, T, 2 * H), float("nan"), device=DEV)
        dybuf[:, :, H:] = a["dy_all"]
        prev = torch.randn(B, T, I, device=DEV)
        dx = prev.clone()
        plan.set_io(2 * H, 2 * H, True)
        plan.set_lengths(lengths)
        with pytest.raises(cabi.CsnError, match="pitch"):
            plan.forward(a["x"], *w, want_all=True)                     # (a dense y_all is not what the plan was told)
        y_last, y_all, h_n, c_n = plan.forward(a["x"], *w, h0=a["h0"], c0=a["c0"], want_state=True, y_all=ybuf[:, :, H:])
        grads = [[torch.empty_like(p) for p in group] for group in w]
        dh0, dc0 = torch.empty(L, B, H, device=DEV), torch.empty(L, B, H, device=DEV)
        plan.backward(a["dy_last"], dybuf[:, :, H:], grads, dx=dx, dh_n=a["dh_n"], dc_n=a["dc_n"], dh0=dh0, dc0=dc0)
        assert torch.isnan(ybuf[:, :, :H]).all()                        # the left half is untouched
        assert torch.equal(ybuf[:, :, H:], dense["y_all"])
        got = dict(y_last=y_last, h_n=h_n, c_n=c_n, dh0=dh0, dc0=dc0)
        for n, group in zip(bref.NAMES, grads):
            got.update({f"{n}_l{k}": t for k, t in enumerate(group)})
        for k, v in got.items():
            assert torch.equal(v, dense[k]), (name, k)
        assert torch.equal(dx, prev + dense["dx"])                      # fl32(prev + g): the bits of a torch add
        for b, n in enumerate(lengths or ()):
            assert torch.equal(dx[b, n:], prev[b, n:])                  # the padding rows are left as they were
        # a following call with the defaults is dense and overwriting again
        plan.set_io()
        _same(_plan_call(plan, w, a, lengths), dense, f"{name} defaults again")
    _check_plans([plan])


# ---- 3. BiLSTM = the composition, bit for bit; 4. against float64 nn.LSTM(bidirectional=True) ---------------------------
MODEL_SHAPES = {
    "v1_h96": ((8, 40, 24, 96, 2), BF16),
    "ks_h256": ((64, 33, 128, 256, 2), BF16),
    "ks_fused_h768_l1": ((64, 32, 128, 768, 1), BF16),
    "ns_h1024_l1": ((65, 33, 128, 1024, 1), BF16),
    "f32_h128": ((20, 17, 24, 128, 2), F32),
}
F64_SHAPES = ("v1_h96", "ks_h256", "f32_h128")


def _model(name, seed=0):
    (B, T, I, H, L), dtype = MODEL_SHAPES[name]
    torch.manual_seed(seed)
    m = BiLSTM(I, H, L, compute_dtype=dtype).to(DEV)
    g = torch.Generator().manual_seed(seed + 1)
    x = torch.randn(B, T, I, generator=g)
    h0 = 0.5 * torch.randn(2 * L, B, H, generator=g)
    c0, dh, dc = (torch.randn(2 * L, B, H, generator=g) for _ in range(3))
    dy = torch.randn(B, T, 2 * H, generator=g)
    return m, [t.to(DEV) for t in (x, h0, c0, dy, dh, dc)]


def _composition(m):
    """The same network from existing single-layer LSTM modules holding the same parameter values."""
    return bref.single_layer_modules(m, lambda i, h: LSTM(i, h, 1, compute_dtype=m.compute_dtype).to(DEV))


def _run_model(m, args, lengths, hx=True):
    x, h0, c0, dy, dh, dc = args
    if not hx:
        h0 = c0 = None
    return bref.run(lambda xx, s: m(xx, s, lengths=lengths), m.named_parameters(), x, h0, c0, dy, dh, dc)


def _run_composition(layers, args, lengths, hx=True):
    x, h0, c0, dy, dh, dc = args
    if not hx:
        h0 = c0 = None
    return bref.run(lambda xx, s: bref.composed(layers, bref.call_lengths, xx, s, lengths), bref.composed_named_params(layers),
                    x, h0, c0, dy, dh, dc)


@pytest.mark.parametrize("name", list(MODEL_SHAPES))
def test_bilstm_is_the_composition_bit_for_bit(name):
    (B, T, I, H, L), dtype = MODEL_SHAPES[name]
    m, args = _model(name)
    layers = _composition(m)
    ragged = _lengths(B, T, "random_with_zeros", (31, 32, 33))
    for lengths, hx in ((None, True), (None, False), (ragged, True)):
        got = _run_model(m, args, lengths, hx)
        _same(got, _run_composition(layers, args, lengths, hx), f"{name} lengths={lengths is not None} hx={hx}")
        assert got["out"].shape == (B, T, 2 * H) and got["h_n"].shape == (2 * L, B, H)
        for b, n in enumerate(lengths or [T] * B):
            # the top layer's final state in each direction is its output at the row's last / first step
            if n > 0:
                assert torch.equal(got["h_n"][-2, b], got["out"][b, n - 1, :H]) and torch.equal(got["h_n"][-1, b], got["out"][b, 0, H:])
            assert not got["out"][b, n:].any() and not got["dx"][b, n:].any()
    # inference: the training forward's bits, on inference plans
    want = _run_model(m, args, ragged)
    with torch.no_grad():
        out, (h_n, c_n) = m(args[0], (args[1], args[2]), lengths=torch.tensor(ragged))
    assert torch.equal(out, want["out"]) and torch.equal(h_n, want["h_n"]) and torch.equal(c_n, want["c_n"])
    assert any(not pl.training for pl in m.all_plans()) and not any(pl.busy for pl in m.all_plans())
    # a PackedSequence (enforce_sorted=False; torch packs no empty rows) = the padded call with its lengths
    lens = [max(n, 1) for n in ragged]
    x, h0, c0, dy, dh, dc = args
    want = _run_model(m, args, lens)
    xr = x.clone().requires_grad_(True)
    for p in m.parameters():
        p.grad = None
    out_p, (h_n, c_n) = m(pack_padded_sequence(xr, torch.tensor(lens), batch_first=True, enforce_sorted=False), (h0, c0))
    out, out_lens = pad_packed_sequence(out_p, batch_first=True, total_length=T)
    assert out_lens.tolist() == lens
    torch.autograd.backward([out, h_n, c_n], [dy, dh, dc])
    got = dict(out=out.detach(), h_n=h_n.detach(), c_n=c_n.detach(), dx=xr.grad, **{k: p.grad for k, p in m.named_parameters()})
    for k, v in got.items():
        assert torch.equal(v, want[k]), (name, "packed", k)
    torch.cuda.synchronize()
    _check_plans(m.all_plans())
    assert {pl.reverse for pl in m.all_plans()} == {False, True} and all(pl.desc.L == 1 and pl.state for pl in m.all_plans())


@pytest.mark.parametrize("name", F64_SHAPES)
@pytest.mark.parametrize("ragged", [False, True], ids=["dense", "ragged"])
def test_bilstm_matches_float64_bidirectional_nn_lstm(name, ragged):
    """Bounds: test_gpu_lstm_state._bounds (outputs and states max |difference| 3e-2 bf16 / 2e-5 float32; gradients
    relative norm 4e-2 / 1e-5)."""
    (B, T, I, H, L), dtype = MODEL_SHAPES[name]
    m, args = _model(name, seed=2)
    lengths = _lengths(B, T, "random_with_zeros", (31, 32, 33)) if ragged else None
    got = _run_model(m, args, lengths)
    torch.cuda.synchronize()
    ref = torch.nn.LSTM(I, H, L, batch_first=True, bidirectional=True).double()
    ref.load_state_dict({k: v.double().cpu() for k, v in m.state_dict().items()})
    want = bref.nn_bilstm_f64(ref, args[0].double().cpu(), lengths, *(t.double().cpu() for t in args[1:]))
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
    print(f"measured vs float64 nn.LSTM(bidirectional=True) {name} {'ragged' if ragged else 'dense'}: " + " ".join(line))
    assert not failures, failures
    _check_plans(m.all_plans())


# ---- 5. use -------------------------------------------------------------------------------------------------------------
def test_two_forwards_outstanding_before_their_backwards():
    m, args = _model("ks_h256", seed=3)
    x, h0, c0, dy, dh, dc = args
    x2 = x.flip(0).contiguous()
    alone = [_run_model(m, [xx, h0, c0, dy, dh, dc], None) for xx in (x, x2)]
    for p in m.parameters():
        p.grad = None
    outs = [m(xx, (h0, c0)) for xx in (x, x2)]
    assert sum(pl.busy for pl in m.all_plans()) == 2 * 2 * m.num_layers        # every workspace is leased until its backward
    for out, (h_n, c_n) in outs:
        torch.autograd.backward([out, h_n, c_n], [dy, dh, dc])
    assert not any(pl.busy for pl in m.all_plans())
    for (out, (h_n, c_n)), one in zip(outs, alone):
        assert torch.equal(out.detach(), one["out"]) and torch.equal(h_n.detach(), one["h_n"]) and torch.equal(c_n.detach(), one["c_n"])
    for k, p in m.named_parameters():
        assert torch.equal(p.grad, alone[0][k] + alone[1][k]), k
    _check_plans(m.all_plans())


def test_state_dict_from_a_stock_bidirectional_nn_lstm():
    torch.manual_seed(6)
    B, T, I, H, L = 8, 12, 24, 96, 2
    ref = torch.nn.LSTM(I, H, L, batch_first=True, bidirectional=True)          # never on a device
    m = BiLSTM(I, H, L, compute_dtype=F32).to(DEV)
    m.load_state_dict(ref.state_dict(), strict=True)
    x = torch.randn(B, T, I)
    with torch.no_grad():
        want, (w_h, w_c) = ref.double()(x.double())
        out, (h_n, c_n) = m(x.to(DEV))
    for a, b in ((out, want), (h_n, w_h), (c_n, w_c)):
        assert float((a.double().cpu() - b).abs().max()) < 2e-5
    _check_plans(m.all_plans())


def test_model_bidirectional_trains_through_the_trainer():
    from cerebralsignalnetworks_amd.trainer import DistillTrainer
    B, T, C, H, L, D = 16, 40, 32, 128, 2, 24
    torch.manual_seed(7)
    model = Model(input_size=C, lstm_size=H, lstm_layers=L, output_size=D, include_top=False, bidirectional=True).to(DEV)
    tr = DistillTrainer(model, None, loss="cosine", lr=1e-3, optimizer="rmsprop", preprocess=False)
    assert tr._lstm is None                 # the direct gradient path is for HipLSTM: BiLSTM's go through autograd
    g = torch.Generator().manual_seed(8)
    x, tgt = torch.randn(B, C, T, generator=g).to(DEV), torch.randn(B, D, generator=g).to(DEV)
    losses = [float(tr.train_step(x, tgt)) for _ in range(5)]
    assert all(np.isfinite(losses)) and all(b < a for a, b in zip(losses, losses[1:])), losses
    # every parameter receives a gradient (a fresh backward outside the trainer, which zeroes its buffer per step)
    for p in model.parameters():
        p.grad = None
    model(x.transpose(1, 2)).square().sum().backward()
    for k, p in model.named_parameters():
        assert p.grad is not None and bool(p.grad.any()) and bool(torch.isfinite(p.grad).all()), k
    tr.check_device_status()
    _check_plans(model.lstm.all_plans())


def test_cli_train_bidirectional(tmp_path, monkeypatch):
    import LstmDistillFromDinoV2Train as train
    plans = []
    init = cabi.LstmPlan.__init__

    def recording_init(self, *a, **kw):
        init(self, *a, **kw)
        plans.append(self)
    monkeypatch.setattr(cabi.LstmPlan, "__init__", recording_init)
    hist = train.main(["--synthetic", "64", "--batch_size", "16", "--num_epochs", "1", "--log_dir", str(tmp_path),
                       "--hidden_size", "128", "--lstm_layers", "2", "--loss", "cosine", "--bidirectional"])
    torch.cuda.synchronize()
    assert len(hist) == 1 and np.isfinite(hist[0]) and 0.5 < hist[0] < 1.5      # cosine loss vs random targets ~ 1
    ckpt = os.path.join(str(tmp_path), "lstm_dinov2_best_loss.pth")
    assert os.path.exists(ckpt)
    sd = torch.load(ckpt, map_location="cpu", weights_only=True)
    assert "lstm.weight_ih_l1_reverse" in sd and sd["fc.weight"].shape[1] == 2 * 128
    assert plans and {pl.reverse for pl in plans} == {False, True} and all(pl.desc.L == 1 and pl.status() == 0 for pl in plans)
