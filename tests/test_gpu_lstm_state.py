"""GPU: lstm_model.LSTM / the state arguments of csn_lstm_forward / csn_lstm_backward (CSN_LSTM_STATE plans).

Against float64 torch.nn.LSTM with a random (h0, c0) and incoming gradients on output, h_n and c_n; chunks chained
through (h_n, c_n) against one run over the whole sequence; zero state against no state; a stateless call after a
stateful one against a fresh plan; the reference's nn.LSTM call patterns.  The bf16 results also against the
bf16-faithful emulator with state (oracle.lstm, bounds oracle.compare.BF16_EMU_BOUNDS); every subset of the state
arguments and incoming gradients, and of the outputs, on one plan per path.  Every case checks the plan's path and
kernels and the workspace status word."""
import itertools

import numpy as np
import pytest
import torch

from cerebralsignalnetworks_amd import cabi, LSTM
from oracle import compare, lstm as olstm

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda:0")
BF16, F32 = torch.bfloat16, torch.float32
# (path, forward kernel, backward kernel) of a state plan
V1 = (0, "lstm_cell_fwd_kernel", "lstm_cell_bwd_kernel")
V1_KS = (0, "lstm_cell_fwd_ks_kernel", "lstm_cell_bwd_ks_kernel")
IL = (1, "lstm_cell_fwd_il_kernel", "lstm_cell_bwd_il_kernel")
_PF, _NSF, _PB, _ILB = "lstm_fwd_persist_kernel", "lstm_fwd_ns_kernel", "lstm_bwd_persist_kernel", "lstm_cell_bwd_il_kernel"
P2 = (2, _PF, _ILB)
P3 = (3, _PF, _PB)
P3_NS = (3, _NSF, _PB)
PLAIN = None        # the path a plan without CSN_LSTM_STATE takes for the shape (checked to be the same)

# name: (B, T, I, H, L, compute dtype, expected plan, environment); the weight-stationary shapes are those of
# test_gpu_parity._BF16_MATRIX
CASES = {
    "v1_h96": ((8, 40, 24, 96, 2), BF16, V1, {}),
    "v1_h256_ks": ((8, 20, 32, 256, 2), BF16, V1_KS, {"CSN_CELL_V1": "1"}),
    "p1_env": ((16, 40, 32, 128, 2), BF16, IL, {"CSN_NO_PERSIST": "1"}),
    "p1_l5": ((8, 30, 16, 128, 5), BF16, IL, {}),
    "p2_nopersist_bwd": ((64, 40, 128, 768, 2), BF16, P2, {"CSN_NO_PERSIST_BWD": "1"}),
    "ks_fused_h768_t32": ((256, 32, 128, 768, 2), BF16, P3, {}),
    "ks_gemm_i24_t31": ((1, 31, 24, 128, 2), BF16, P3, {}),
    "ns_fused_h1024_t33": ((65, 33, 128, 1024, 2), BF16, P3_NS, {}),
    "ns_env_h128_t3": ((129, 3, 16, 128, 2), BF16, P3_NS, {"CSN_FWD_NSPLIT": "1"}),
    "t1": ((65, 1, 32, 256, 2), BF16, P3, {}),
    "t4_l3": ((63, 4, 32, 128, 3), BF16, P3, {}),
    "ks_flags": ((64, 40, 128, 768, 2), BF16, P3, {"CSN_FWD_FLAGS": "1", "CSN_BWD_FLAGS": "1"}),
    "no_beside_l3": ((64, 40, 32, 256, 3), BF16, P3, {"CSN_NO_BESIDE": "1"}),
    "chunk4_l3": ((64, 23, 32, 256, 3), BF16, P3, {"CSN_LSTM_CHUNK": "4"}),
    "f32_h128": ((70, 37, 24, 128, 2), F32, V1_KS, {}),
    "f32_cell_v1": ((20, 17, 24, 96, 2), F32, V1, {"CSN_CELL_V1": "1"}),
    "ref_h96": ((16, 460, 96, 96, 2), BF16, V1, {}),
    "ref_h128_l4": ((16, 460, 128, 128, 4), BF16, PLAIN, {}),
}


def _bounds(dtype):
    # bf16: as test_fast_path_matches_oracle_and_v1; float32: as test_f32_weight_stationary_recurrence
    return (3e-2, 4e-2) if dtype == BF16 else (2e-5, 1e-5)


def _rel(got, want):
    return float((got.double() - want).norm() / max(float(want.norm()), 1e-30))


def _make(shape, dtype, seed=0):
    B, T, I, H, L = shape
    torch.manual_seed(seed)
    m = LSTM(I, H, L, compute_dtype=dtype).to(DEV)
    m._case_T = T
    ref = torch.nn.LSTM(I, H, num_layers=L, batch_first=True).double().to(DEV)
    ref.load_state_dict({k: v.double() for k, v in m.state_dict().items()})
    g = torch.Generator(device="cpu").manual_seed(seed + 1)
    x = torch.randn(B, T, I, generator=g)
    h0 = 0.5 * torch.randn(L, B, H, generator=g)
    c0 = torch.randn(L, B, H, generator=g)
    dy = torch.randn(B, T, H, generator=g)
    dh = torch.randn(L, B, H, generator=g)
    dc = torch.randn(L, B, H, generator=g)
    return m, ref, [t.to(DEV) for t in (x, h0, c0, dy, dh, dc)]


def _plan_of(m):
    plans = m.all_plans()
    assert plans, "no plan was created"
    return plans[-1]


def _check_plan(m, expect):
    _check_plans(m.all_plans(), expect, getattr(m, "_case_T", None))


def _check_plans(plans, expect, case_T=None):
    for plan in plans:
        assert plan.state
        got = (plan.path(),) + plan.kernel_names()
        if expect is PLAIN or plan.desc.dtype == cabi.CSN_BF16:
            d = plan.desc
            plain = cabi.LstmPlan(d.B, d.T, d.I, d.H, d.L, BF16, DEV, training=plan.training)
            assert got == (plain.path(),) + plain.kernel_names(), (got, plain.path())   # bf16: the stateless plan's path
        if expect is not PLAIN and (case_T is None or plan.desc.T == case_T):
            assert got == expect, (got, expect)
        assert plan.status() == 0


def _run(m, x, h0, c0, dy, dh, dc):
    """forward with state + backward of <out,dy> + <h_n,dh> + <c_n,dc>: outputs and every gradient."""
    x = x.clone().requires_grad_(True)
    h0 = h0.clone().requires_grad_(True)
    c0 = c0.clone().requires_grad_(True)
    for p in m.parameters():
        p.grad = None
    out, (h_n, c_n) = m(x, (h0, c0))
    ((out * dy).sum() + (h_n * dh).sum() + (c_n * dc).sum()).backward()
    grads = {k: p.grad.detach().clone() for k, p in m.named_parameters()}
    return dict(out=out.detach(), h_n=h_n.detach(), c_n=c_n.detach(), dx=x.grad, dh0=h0.grad, dc0=c0.grad, **grads)


def _np(t):
    return t.detach().double().cpu().numpy() if torch.is_tensor(t) else t


def _emu_run(m, x, h0, c0, dy, dh, dc):
    """_run's call on the bf16-faithful emulator (oracle.lstm): the same keys."""
    lp = {k: v.detach().cpu().numpy() for k, v in m.state_dict().items()}
    y, saved = olstm.lstm_forward_bf16(_np(x), lp, m.num_layers, h0=_np(h0), c0=_np(c0))
    h_n, c_n = olstm.final_state(saved)
    dx, g, _, dh0, dc0 = olstm.lstm_backward_bf16(_np(dy), saved, m.num_layers, dh_n=_np(dh), dc_n=_np(dc),
                                                 return_state=True)
    return dict(out=y, h_n=h_n, c_n=c_n, dx=dx, dh0=dh0, dc0=dc0, **g)


def _emu_errors(got, want):
    """{key: (relative-norm error, element error)} of every tensor of `want` that `got` holds."""
    return {k: compare.errors(_np(got[k]), w) for k, w in want.items() if k in got}


def _emu_check(case, got, want, saturated=False):
    """Every tensor of `want` (the emulator's) that `got` holds within compare.BF16_EMU_BOUNDS; prints the measured errors
    first (the record behind the bounds)."""
    measured = _emu_errors(got, want)
    print(f"measured bf16 vs emulator {case} (rel/elem): " + " ".join(f"{k} {r:.2e}/{e:.2e}" for k, (r, e) in measured.items()))
    for k in measured:
        kk = "y_all" if k == "out" else k
        compare.check(f"{case}: {k}", _np(got[k]), want[k], *compare.bf16_emu_bound(kk, saturated),
                      layout=compare.layout_of(kk))


@pytest.mark.parametrize("name", list(CASES))
def test_random_state_matches_float64_nn_lstm(name, monkeypatch):
    shape, dtype, expect, env = CASES[name]
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    m, ref, (x, h0, c0, dy, dh, dc) = _make(shape, dtype)
    got = _run(m, x, h0, c0, dy, dh, dc)
    torch.cuda.synchronize()
    _check_plan(m, expect)
    want = _run(ref, x.double(), h0.double(), c0.double(), dy.double(), dh.double(), dc.double())
    elem, rel = _bounds(dtype)
    for k in ("out", "h_n", "c_n"):
        err = float((got[k].double() - want[k]).abs().max())
        assert err < elem, (name, k, err)
    for k in want:
        if k in ("out", "h_n", "c_n"):
            continue
        r = _rel(got[k], want[k])
        assert r < rel, (name, k, r)
    # h_n of the top layer is the last output, bit for bit
    assert torch.equal(got["h_n"][-1], got["out"][:, -1])
    if dtype == BF16:
        _emu_check(name, got, _emu_run(m, x, h0, c0, dy, dh, dc))


# bf16 state cases against the emulator alone: lstm_dh0_kernel's tile edges (32 rows x 64 units; H = 32 is half a tile,
# H = 160 two and a half, B = 1 and 33 rows), many row tiles of its fragment-major form on path 1 (B 512, H 768:
# 16 x 12 tiles), 8 layers over 300 steps, and a saturated cell state.  name: (shape, expected plan, c0 scale)
EMU_CASES = {
    "v1_h32_b1": ((1, 20, 24, 32, 2), V1, 1.0),
    "v1_h32_b33": ((33, 20, 24, 32, 2), V1, 1.0),
    "v1_h160_b1": ((1, 20, 24, 160, 2), V1, 1.0),
    "v1_h160_b33": ((33, 20, 24, 160, 2), V1, 1.0),
    "p1_b512_h768": ((512, 4, 128, 768, 2), IL, 1.0),
    "p1_l8_t300": ((8, 300, 24, 128, 8), IL, 1.0),
    "sat_c0x5": ((64, 40, 32, 256, 2), P3, 5.0),
}


@pytest.mark.parametrize("name", list(EMU_CASES))
def test_random_state_matches_bf16_emulator(name):
    shape, expect, c0_scale = EMU_CASES[name]
    m, _, (x, h0, c0, dy, dh, dc) = _make(shape, BF16, seed=4)
    c0 = c0 * c0_scale
    got = _run(m, x, h0, c0, dy, dh, dc)
    torch.cuda.synchronize()
    _check_plan(m, expect)
    assert torch.equal(got["h_n"][-1], got["out"][:, -1])
    _emu_check(name, got, _emu_run(m, x, h0, c0, dy, dh, dc))


def test_inference_forward_with_state():
    m, ref, (x, h0, c0, *_rest) = _make((16, 40, 32, 128, 2), BF16)
    with torch.no_grad():
        out, (h_n, c_n) = m(x, (h0, c0))
        r_out, (r_h, r_c) = ref(x.double(), (h0.double(), c0.double()))
    _check_plan(m, PLAIN)
    assert not _plan_of(m).training
    for a, b in ((out, r_out), (h_n, r_h), (c_n, r_c)):
        assert float((a.double() - b).abs().max()) < 3e-2


CHAIN_CASES = {
    "v1_h96": ((8, 41, 24, 96, 2), BF16, {}),
    "p1_env": ((16, 41, 32, 128, 2), BF16, {"CSN_NO_PERSIST": "1"}),
    "p1_l5": ((8, 30, 16, 128, 5), BF16, {}),
    "p3_ks": ((64, 41, 128, 256, 2), BF16, {}),
    "p3_ks_flags": ((64, 41, 32, 256, 2), BF16, {"CSN_FWD_FLAGS": "1", "CSN_BWD_FLAGS": "1"}),
    "p3_ns": ((65, 33, 128, 1024, 2), BF16, {}),
    "p2": ((64, 41, 128, 768, 2), BF16, {"CSN_NO_PERSIST_BWD": "1"}),
    "f32_h128": ((20, 37, 24, 128, 2), F32, {}),
}


@pytest.mark.parametrize("name", list(CHAIN_CASES))
@pytest.mark.parametrize("split", ["first", "half", "uneven"])
def test_chunked_equals_continuous(name, split, monkeypatch):
    (B, T, I, H, L), dtype, env = CHAIN_CASES[name]
    for kk, v in env.items():
        monkeypatch.setenv(kk, v)
    k = {"first": 1, "half": T // 2, "uneven": (2 * T) // 7}[split]
    if split == "half":             # two outstanding forwards of one plan key: equal halves
        T = 2 * k
    m, ref, (x, h0, c0, dy, dh, dc) = _make((B, T, I, H, L), dtype, seed=7)
    whole = _run(m, x, h0, c0, dy, dh, dc)
    # chained: x[:, :k] then x[:, k:] from the carried state, one autograd graph
    xr = x.clone().requires_grad_(True)
    h0r, c0r = h0.clone().requires_grad_(True), c0.clone().requires_grad_(True)
    for p in m.parameters():
        p.grad = None
    out1, s1 = m(xr[:, :k], (h0r, c0r))
    out2, (h_n, c_n) = m(xr[:, k:], s1)
    torch.cuda.synchronize()
    assert sum(pl.busy for pl in m.all_plans()) == 2       # both forwards await their backward
    out = torch.cat([out1, out2], 1)
    ((out * dy).sum() + (h_n * dh).sum() + (c_n * dc).sum()).backward()
    _check_plan(m, PLAIN if dtype == BF16 else V1_KS)
    # forward: the same bits as one run over the whole sequence
    assert torch.equal(out.detach(), whole["out"]), float((out.detach() - whole["out"]).abs().max())
    assert torch.equal(h_n.detach(), whole["h_n"])
    assert torch.equal(c_n.detach(), whole["c_n"])
    # gradients: the float64 reference over the whole sequence
    want = _run(ref, x.double(), h0.double(), c0.double(), dy.double(), dh.double(), dc.double())
    _, rel = _bounds(dtype)
    got = dict(dx=xr.grad, dh0=h0r.grad, dc0=c0r.grad, **{kk: p.grad for kk, p in m.named_parameters()})
    for kk, g in got.items():
        assert _rel(g, want[kk]) < rel, (name, split, kk, _rel(g, want[kk]))
    # bf16: and the emulator over the whole sequence (the chained forward has its bits, so it is the reference)
    if dtype == BF16:
        _emu_check(f"{name} {split}", got, _emu_run(m, x, h0, c0, dy, dh, dc))


@pytest.mark.parametrize("name", ["v1_h96", "p1_env", "p1_l5", "ks_fused_h768_t32", "ns_fused_h1024_t33", "ks_flags",
                                  "p2_nopersist_bwd", "f32_h128"])
def test_zero_state_is_no_state_and_leaves_nothing_stale(name, monkeypatch):
    shape, dtype, _, env = CASES[name]
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    B, T, I, H, L = shape
    m, _, (x, h0, c0, dy, dh, dc) = _make(shape, dtype, seed=3)

    def plain(mod, hx):
        xr = x.clone().requires_grad_(True)
        for p in mod.parameters():
            p.grad = None
        out, (h_n, c_n) = mod(xr, hx)
        (out * dy).sum().backward()
        return [out.detach(), h_n.detach(), c_n.detach(), xr.grad] + [p.grad.clone() for p in mod.parameters()]

    no_state = plain(m, None)
    zeros = torch.zeros(L, B, H, device=DEV)
    zero_state = plain(m, (zeros, zeros.clone()))
    for a, b in zip(no_state, zero_state):
        assert torch.equal(a, b)
    _run(m, x, h0, c0, dy, dh, dc)          # a stateful forward + backward on the same plan ...
    after = plain(m, None)                   # ... then stateless: as a fresh plan
    fresh = LSTM(I, H, L, compute_dtype=dtype).to(DEV)
    fresh.load_state_dict(m.state_dict())
    ref_bits = plain(fresh, None)
    assert len(m.all_plans()) == 1
    for a, b, c in zip(after, ref_bits, no_state):
        assert torch.equal(a, b) and torch.equal(a, c)
    _check_plan(m, CASES[name][2])


def test_drop_in_call_patterns():
    torch.manual_seed(11)
    B, T, I, H, L = 16, 60, 32, 128, 2
    lstm = LSTM(I, H, L).to(DEV)
    x = torch.randn(B, T, I, device=DEV)
    # LSTMDistill.py: lstm_out, (ht, ct) = self.lstm(x)
    lstm_out, (ht, ct) = lstm(x)
    assert ht.shape == ct.shape == (L, B, H) and lstm_out.shape == (B, T, H)
    assert torch.equal(ht[-1], lstm_out[:, -1])
    # LSTMDistillRetreival.py: self.lstm(x, lstm_init)[0][:, -1, :]
    lstm_init = (0.5 * torch.randn(L, B, H, device=DEV), torch.randn(L, B, H, device=DEV))
    last = lstm(x, lstm_init)[0][:, -1, :]
    ref = torch.nn.LSTM(I, H, L, batch_first=True).double().to(DEV)
    ref.load_state_dict({k: v.double() for k, v in lstm.state_dict().items()})
    want = ref(x.double(), tuple(t.double() for t in lstm_init))[0][:, -1, :]
    assert float((last.detach().double() - want.detach()).abs().max()) < 3e-2
    _check_plan(lstm, PLAIN)


def test_encoder_on_final_hidden_state_trains_like_nn_lstm():
    # utils/LSTMAutoEncoders.py: x, (hidden_n, _) = self.rnn(x); the encoder's output is hidden_n
    torch.manual_seed(5)
    B, T, I, H = 12, 50, 24, 64
    enc = LSTM(I, H, 1, compute_dtype=F32).to(DEV)
    ref = torch.nn.LSTM(I, H, 1, batch_first=True).double().to(DEV)
    ref.load_state_dict({k: v.double() for k, v in enc.state_dict().items()})
    x = torch.randn(B, T, I, device=DEV)
    target = torch.randn(B, H, device=DEV)
    opt = torch.optim.SGD(enc.parameters(), lr=0.1)
    opt_ref = torch.optim.SGD(ref.parameters(), lr=0.1)
    for mod, o, xx, tt in ((enc, opt, x, target), (ref, opt_ref, x.double(), target.double())):
        o.zero_grad()
        _, (hidden_n, _) = mod(xx)
        loss = ((hidden_n[-1] - tt) ** 2).mean()
        loss.backward()
        o.step()
    _check_plan(enc, V1)
    for (k, p), (_, q) in zip(enc.named_parameters(), ref.named_parameters()):
        assert float((p.detach().double() - q.detach()).abs().max()) < 2e-5, k
        assert _rel(p.grad, q.grad) < 1e-5, k


def test_state_arguments_are_checked_on_the_host():
    B, T, I, H, L = 4, 6, 32, 128, 2
    plain = cabi.LstmPlan(B, T, I, H, L, BF16, DEV, training=True)
    torch.manual_seed(0)
    ref = torch.nn.LSTM(I, H, L, batch_first=True).to(DEV)
    params = [[getattr(ref, f"{n}_l{k}").detach() for k in range(L)] for n in ("weight_ih", "weight_hh", "bias_ih", "bias_hh")]
    x = torch.randn(B, T, I, device=DEV)
    h0 = torch.zeros(L, B, H, device=DEV)
    with pytest.raises(cabi.CsnError, match="without CSN_LSTM_STATE"):
        plain.forward(x, *params, h0=h0)
    with pytest.raises(cabi.CsnError, match="without CSN_LSTM_STATE"):
        plain.forward(x, *params, want_state=True)
    st = cabi.LstmPlan(B, T, I, H, L, BF16, DEV, training=True, state=True)
    with pytest.raises(cabi.CsnError, match="L, B, H"):
        st.forward(x, *params, h0=torch.zeros(L, B + 1, H, device=DEV))
    # misaligned state pointer: refused before any launch
    buf = torch.zeros(L * B * H + 1, device=DEV)
    y_last = torch.empty(B, H, device=DEV)
    rc = cabi.load().csn_lstm_forward(st._plan, cabi._ptr(x), x.stride(0), x.stride(1), cabi._ptr_array(params[0]),
                                      cabi._ptr_array(params[1]), cabi._ptr_array(params[2]), cabi._ptr_array(params[3]),
                                      cabi._ptr(buf[1:]), None, st._ws_ptr, cabi._ptr(y_last), None, None, None, None)
    assert rc == 1
    assert b"16-B aligned" in cabi.load().csn_last_error()
    # no output at all / no incoming gradient at all
    rc = cabi.load().csn_lstm_forward(st._plan, cabi._ptr(x), x.stride(0), x.stride(1), cabi._ptr_array(params[0]),
                                      cabi._ptr_array(params[1]), cabi._ptr_array(params[2]), cabi._ptr_array(params[3]),
                                      None, None, st._ws_ptr, None, None, None, None, None)
    assert rc == 1 and b"no output" in cabi.load().csn_last_error()
    # final state alone is an output; a bf16 state plan takes the stateless plan's path
    y_last, _, h_n, c_n = st.forward(x, *params, want_state=True)
    torch.cuda.synchronize()
    assert torch.equal(h_n[-1], y_last)
    assert st.path() == plain.path() and st.kernel_names() == plain.kernel_names() and st.status() == 0


# ---- every subset of the state arguments, of the incoming gradients and of the outputs (cabi.LstmPlan / the C ABI) ------
# One small plan per path and cell kernel: (B, T, I, H, L), dtype, expected plan, environment
SUBSET_REPS = {
    "p0_bf16": ((8, 10, 24, 96, 2), BF16, V1, {}),
    "p0_f32_ks": ((70, 9, 24, 128, 2), F32, V1_KS, {}),
    "p0_f32_cell_v1": ((20, 9, 24, 96, 2), F32, V1, {"CSN_CELL_V1": "1"}),
    "p1_env": ((16, 10, 32, 128, 2), BF16, IL, {"CSN_NO_PERSIST": "1"}),
    "p2_nopersist_bwd": ((64, 9, 32, 256, 2), BF16, P2, {"CSN_NO_PERSIST_BWD": "1"}),
    "p3_ks_dpoll": ((63, 9, 24, 128, 2), BF16, P3, {}),
    "p3_ks_flags": ((64, 9, 32, 256, 2), BF16, P3, {"CSN_FWD_FLAGS": "1", "CSN_BWD_FLAGS": "1"}),
    "p3_ns_env_h128": ((129, 3, 16, 128, 2), BF16, P3_NS, {"CSN_FWD_NSPLIT": "1"}),
}
_FWD_IN = ("h0", "c0")
_BWD_IN = ("dy_last", "dy_all", "dh_n", "dc_n")
_FWD_SUBSETS = [s for n in range(3) for s in itertools.combinations(_FWD_IN, n)]
_BWD_SUBSETS = [s for n in range(1, 5) for s in itertools.combinations(_BWD_IN, n)]
_OUT_KEYS = ("y_last", "y_all", "h_n", "c_n")


def _plan_case(rep, seed=0):
    """A state plan of `rep`, its parameters (numpy, nn.LSTM names, and on the device as cabi groups) and random inputs
    for every argument (device tensors)."""
    (B, T, I, H, L), dtype, _, _ = SUBSET_REPS[rep]
    torch.manual_seed(seed)
    lp = {k: v.detach().numpy() for k, v in torch.nn.LSTM(I, H, L, batch_first=True).state_dict().items()}
    w = [[torch.from_numpy(lp[f"{n}_l{k}"]).to(DEV) for k in range(L)] for n in ("weight_ih", "weight_hh", "bias_ih", "bias_hh")]
    g = torch.Generator(device="cpu").manual_seed(seed + 1)
    a = dict(x=torch.randn(B, T, I, generator=g), h0=0.5 * torch.randn(L, B, H, generator=g),
             c0=torch.randn(L, B, H, generator=g), dy_last=torch.randn(B, H, generator=g),
             dy_all=0.1 * torch.randn(B, T, H, generator=g), dh_n=torch.randn(L, B, H, generator=g),
             dc_n=torch.randn(L, B, H, generator=g))
    plan = cabi.LstmPlan(B, T, I, H, L, dtype, DEV, training=True, state=True)
    return plan, lp, w, {k: v.to(DEV) for k, v in a.items()}


def _call(plan, w, a, fwd, bwd, dh0=True, dc0=True):
    """Forward with the state arguments named in `fwd`, backward with the incoming gradients named in `bwd` (the others
    NULL); every output, on the host."""
    d = plan.desc
    y_last, y_all, h_n, c_n = plan.forward(a["x"], *w, want_all=True, h0=a["h0"] if "h0" in fwd else None,
                                           c0=a["c0"] if "c0" in fwd else None, want_state=True)
    out = dict(y_last=y_last, y_all=y_all, h_n=h_n, c_n=c_n, dx=torch.empty(d.B, d.T, d.I, device=DEV),
               dh0=torch.empty(d.L, d.B, d.H, device=DEV) if dh0 else None,
               dc0=torch.empty(d.L, d.B, d.H, device=DEV) if dc0 else None)
    grads = [[torch.empty_like(p) for p in group] for group in w]
    gin = {k: a[k] if k in bwd else None for k in _BWD_IN}
    plan.backward(gin["dy_last"], gin["dy_all"], grads, dx=out["dx"], dh_n=gin["dh_n"], dc_n=gin["dc_n"], dh0=out["dh0"],
                  dc0=out["dc0"])
    for n, group in zip(("weight_ih", "weight_hh", "bias_ih", "bias_hh"), grads):
        out.update({f"{n}_l{k}": t for k, t in enumerate(group)})
    torch.cuda.synchronize()
    return {k: v.cpu() for k, v in out.items() if v is not None}


def _emu_call(lp, a_np, L, fwd, saved, y, bwd, rounding):
    """The emulator's answer to _call(fwd, bwd), from its forward (saved, y) with the state arguments in `fwd`."""
    h_n, c_n = olstm.final_state(saved)
    dy = a_np["dy_all"].copy() if "dy_all" in bwd else np.zeros(y.shape, np.float32)
    if "dy_last" in bwd:
        dy[:, -1] += a_np["dy_last"]                 # float32, as the library adds them
    dx, g, _, dh0, dc0 = olstm.lstm_backward_bf16(dy, saved, L, rounding=rounding,
                                                 dh_n=a_np["dh_n"] if "dh_n" in bwd else None,
                                                 dc_n=a_np["dc_n"] if "dc_n" in bwd else None, return_state=True)
    return dict(y_last=y[:, -1], y_all=y, h_n=h_n, c_n=c_n, dx=dx, dh0=dh0, dc0=dc0, **g)


def _f32_errors(got, want):
    """float32 plans against the emulator without rounding (= float64 nn.LSTM): max |diff| of the outputs, relative norm
    of the gradients -- the bounds of _bounds(F32)."""
    return {k: float(np.abs(_np(got[k]) - w).max()) if k in _OUT_KEYS else compare.errors(_np(got[k]), w)[0]
            for k, w in want.items()}


@pytest.mark.parametrize("rep", list(SUBSET_REPS))
def test_every_state_argument_subset(rep, monkeypatch):
    """The 4 subsets of (h0, c0) x the 15 non-empty subsets of (dy_last, dy_all, dh_n, dc_n), dh0 and dc0 always asked for.
    Each result (a) equals, bit for bit, the call with every missing argument passed as an explicit zero tensor -- with
    h0 = c0 = NULL that is the gradient w.r.t. a zero state after a stateless forward -- and (b) meets the emulator bounds
    (bf16) or the float32 bounds against the emulator without rounding."""
    shape, dtype, expect, env = SUBSET_REPS[rep]
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    L = shape[4]
    plan, lp, w, a = _plan_case(rep)
    a_np = {k: v.cpu().numpy() for k, v in a.items()}
    rounding = dtype == BF16
    worst, failures = {}, []
    for fwd in _FWD_SUBSETS:
        y, saved = olstm.lstm_forward_bf16(a_np["x"], lp, L, rounding=rounding, h0=a_np["h0"] if "h0" in fwd else None,
                                           c0=a_np["c0"] if "c0" in fwd else None)
        for bwd in _BWD_SUBSETS:
            tag = f"{rep} [{'+'.join(fwd) or 'no state'} | {'+'.join(bwd)}]"
            got = _call(plan, w, a, fwd, bwd)
            zeros = {k: (v if k == "x" or k in fwd + bwd else torch.zeros_like(v)) for k, v in a.items()}
            explicit = _call(plan, w, zeros, _FWD_IN, _BWD_IN)
            for k, v in got.items():
                if not torch.equal(v, explicit[k]):
                    failures.append(f"{tag}: {k} differs from the explicit-zero call by {float((v - explicit[k]).abs().max()):.3e}")
            want = _emu_call(lp, a_np, L, fwd, saved, y, bwd, rounding)
            if rounding:
                errs = _emu_errors(got, want)
                for k, e in errs.items():
                    worst[k] = tuple(max(p, q) for p, q in zip(worst.get(k, (0.0, 0.0)), e))
                    try:
                        compare.check(f"{tag}: {k}", _np(got[k]), want[k], *compare.bf16_emu_bound(k), layout=compare.layout_of(k))
                    except AssertionError as e_:
                        failures.append(str(e_))
            else:
                for k, e in _f32_errors(got, want).items():
                    worst[k] = max(worst.get(k, 0.0), e)
                    if e >= (2e-5 if k in _OUT_KEYS else 1e-5):
                        failures.append(f"{tag}: {k} float32 error {e:.3e}")
    print(f"measured {rep} worst over {len(_FWD_SUBSETS) * len(_BWD_SUBSETS)} argument subsets "
          f"({'bf16 vs emulator, rel/elem' if rounding else 'float32: outputs max |diff|, gradients rel'}): " +
          " ".join(f"{k} {v[0]:.2e}/{v[1]:.2e}" if rounding else f"{k} {v:.2e}" for k, v in worst.items()))
    assert not failures, f"{len(failures)} failures; first: " + failures[0]
    _check_plans([plan], expect)


def _forward_raw(plan, w, a, outs):
    """csn_lstm_forward with h0, c0 and exactly the outputs `outs` holds (None = NULL)."""
    x = a["x"]
    lib = cabi.load()
    rc = lib.csn_lstm_forward(plan._plan, cabi._ptr(x), x.stride(0), x.stride(1), *[cabi._ptr_array(g) for g in w],
                              cabi._ptr(a["h0"]), cabi._ptr(a["c0"]), plan._ws_ptr, cabi._ptr(outs["y_last"]),
                              cabi._ptr(outs["y_all"]), cabi._ptr(outs["h_n"]), cabi._ptr(outs["c_n"]), cabi._stream())
    assert rc == 0, lib.csn_last_error()
    torch.cuda.synchronize()


@pytest.mark.parametrize("rep", list(SUBSET_REPS))
def test_output_subsets_match_the_all_outputs_call(rep, monkeypatch):
    """Forward with only y_last, only y_all, only h_n, only c_n; backward with dh0 only, dc0 only, neither: each output
    that is there has the bits of the call that asks for all of them."""
    shape, dtype, expect, env = SUBSET_REPS[rep]
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    B, T, I, H, L = shape
    plan, _, w, a = _plan_case(rep, seed=2)
    full = _call(plan, w, a, _FWD_IN, _BWD_IN)
    shapes = dict(y_last=(B, H), y_all=(B, T, H), h_n=(L, B, H), c_n=(L, B, H))
    for only in _OUT_KEYS:
        outs = {k: torch.full(s, float("nan"), device=DEV) if k == only else None for k, s in shapes.items()}
        _forward_raw(plan, w, a, outs)
        assert torch.equal(outs[only].cpu(), full[only]), (rep, only)
    for dh0, dc0 in ((True, False), (False, True), (False, False)):
        got = _call(plan, w, a, _FWD_IN, _BWD_IN, dh0=dh0, dc0=dc0)
        assert ("dh0" in got, "dc0" in got) == (dh0, dc0)
        for k, v in got.items():
            assert torch.equal(v, full[k]), (rep, dh0, dc0, k)
    _check_plans([plan], expect)
