"""GPU: the pooled readout of the LSTM (csn_lstm_plan_set_readout), through the C ABI and the modules.

1. forward      y_last under "mean" / "max" against the SAME call's y_all (tests/lstm_readout_reference.py): the maximum
                exactly, the mean within ulp32(result) + T 2^-50 of the float64 mean (derived there), two calls the same
                bits; y_all, h_n, c_n with the bits of the call under "last".
2. backward     THE IDENTITY: every gradient of a pooled call has the bits of the same plan under "last" fed dy_last = NULL
                and dy_all' = fl32(dy_all + G), G the restatement's expanded term (plain G without dy_all); x and dy_all
                hold NaN past each row's length in both calls; a row of length 0 gets nothing from dy_last (dh0 = dh_n).
3. ties         a saturated bf16 fixture whose columns hold their maximum at many steps: the gradient lands on the first
                caller time, on a plain and on a reverse plan.
4. features     lengths, input windows, inter-layer dropout and pitched y_all / dy_all together, plain and reverse; output
                dropout leaves the pooled value alone.
5. hygiene      the setter's refusals on real plans; "last" after "mean" on one plan is a fresh plan's call, launches included.
6. modules      HipLSTM(readout=), LSTM.pooled, BiLSTM.pooled, Model(readout=) with views, a CLI round trip.
7. stream order the pooled forward and backward on a side stream with late inputs (tests/lstm_readout_stream_cases.py).

Regimes of 1 and 2: B 5, T 37, I 24, L 2 (ragged, a resident chunk boundary at 32 with a 5-step tail) at H 32 and 96 in bf16
and float32 on path 0 and path 5, and one regime of tests/lstm_width_matrix.py (B 65, T 9) per path 1, 2, 3, 4."""
import contextlib
import os
import time

import numpy as np
import pytest
import torch

import lstm_readout_reference as rref
import lstm_readout_stream_cases as stream_cases
import lstm_width_matrix as wm
import stream_order as so
import test_gpu_lstm_state as st
import test_lstm_readout_cpu as cpu_checks
from cerebralsignalnetworks_amd import cabi
from cerebralsignalnetworks_amd.lstm_model import BiLSTM, HipLSTM, LSTM, Model

pytestmark = pytest.mark.gpu

DEV, BF16, F32 = st.DEV, st.BF16, st.F32
NAN = float("nan")
GROUPS = ("weight_ih", "weight_hh", "bias_ih", "bias_hh")
GRAD_KEYS = tuple(f"d{g}" for g in GROUPS) + ("dx", "dh0", "dc0")


# ---- regimes --------------------------------------------------------------------------------------------------------------
def _regimes():
    out = {}
    for resident in (False, True):
        for H in (32, 96):
            for name, dtype in (("bf16", BF16), ("f32", F32)):
                out[f"p{5 if resident else 0}_h{H}_{name}"] = dict(shape=(5, 37, 24, H, 2), dtype=dtype, env={}, state=True,
                                                                   resident=resident, path=5 if resident else 0)
    for path, name in ((1, "p1_384"), (2, "p2_384"), (3, "ks384_gemm"), (4, "f32p_256")):
        r = wm.REGIMES[name]
        out[f"p{path}_{name}"] = dict(shape=r["shape"], dtype=BF16 if r["dtype"] == "bf16" else F32, env=r["env"],
                                      state=r["sets"] != wm.STATELESS_SETS, resident=False, path=path)
    return out


REGIMES = _regimes()


def _lengths(B, T):
    """0, 1, T - 1 and T among them."""
    n = wm.hand_lengths(B, T)
    n[2], n[3] = 1, T - 1
    assert {0, 1, T - 1, T} <= set(n)
    return n


@contextlib.contextmanager
def _env(kv):
    old = {k: os.environ.get(k) for k in kv}
    os.environ.update(kv)
    try:
        yield
    finally:
        for k, v in old.items():
            os.environ.pop(k, None) if v is None else os.environ.__setitem__(k, v)


def _plan(r, training=True, **bits):
    B, T, I, H, L = r["shape"]
    kw = dict(state=r["state"], resident=r["resident"])
    kw.update(bits)
    with _env(r["env"]):
        return cabi.LstmPlan(B, T, I, H, L, r["dtype"], DEV, training=training, **kw)


def _inputs(shape, seed=3, params=None):
    B, T, I, H, L = shape
    torch.manual_seed(seed)
    ref = torch.nn.LSTM(I, H, L, batch_first=True)
    if params is not None:
        ref.load_state_dict({k: torch.from_numpy(v) for k, v in params.items()})
    w = [[getattr(ref, f"{n}_l{k}").detach().to(DEV) for k in range(L)] for n in GROUPS]
    g = torch.Generator().manual_seed(seed + 1)
    a = dict(x=torch.randn(B, T, I, generator=g), dy_all=0.1 * torch.randn(B, T, H, generator=g), dy_last=torch.randn(B, H, generator=g),
             h0=0.5 * torch.randn(L, B, H, generator=g), c0=torch.randn(L, B, H, generator=g), dh_n=torch.randn(L, B, H, generator=g),
             dc_n=torch.randn(L, B, H, generator=g))
    a["prev"] = [[0.25 * torch.randn(p.shape, generator=g) for p in group] for group in w]
    return w, so._map(a, lambda t: t.to(DEV))


_WORLD = {}


def _world(name):
    """One regime at a time: its training plan (asserted to take the path the regime names) and inputs."""
    if name not in _WORLD:
        _WORLD.clear()
        r = REGIMES[name]
        plan = _plan(r)
        assert plan.path() == r["path"], (name, plan.path())
        _WORLD[name] = (r, plan, *_inputs(r["shape"]))
    return _WORLD[name]


def _pad(lengths, B, T):
    """[B, T, 1] bool: t >= n."""
    n = torch.tensor(rref.rows(lengths, B, T), device=DEV)
    return (torch.arange(T, device=DEV)[None, :] >= n[:, None])[:, :, None]


def _call(plan, w, a, mode, lengths=None, dy_last=None, dy_all=None, state_grads=False, accumulate=False, backward=True):
    """forward (every output) + backward of one plan under `mode`; x and dy_all hold NaN past each row's length."""
    d = plan.desc
    pad = _pad(lengths, d.B, d.T)
    if plan.state:
        plan.set_lengths(lengths)
    else:
        assert lengths is None
    plan.set_readout(mode)
    kw = dict(h0=a["h0"], c0=a["c0"]) if plan.state else {}
    x = torch.where(pad, torch.full_like(a["x"], NAN), a["x"])
    outs = plan.forward(x, *w, want_all=True, want_state=plan.state, **kw)
    out = dict(zip(("y_last", "y_all", "h_n", "c_n"), outs))
    if not backward:
        return out
    grads = [[p.clone() if accumulate else torch.full_like(p, NAN) for p in group] for group in a["prev"]]
    out["dx"] = torch.full((d.B, d.T, d.I), NAN, device=DEV)
    st_kw = {}
    if plan.state:
        out["dh0"], out["dc0"] = (torch.full((d.L, d.B, d.H), NAN, device=DEV) for _ in range(2))
        st_kw = dict(dh0=out["dh0"], dc0=out["dc0"])
        if state_grads:
            st_kw.update(dh_n=a["dh_n"], dc_n=a["dc_n"])
    if dy_all is not None:
        dy_all = torch.where(pad, torch.full_like(dy_all, NAN), dy_all)
    plan.set_grad_mode(accumulate)
    try:
        plan.backward(dy_last, dy_all, grads, dx=out["dx"], **st_kw)
    finally:
        plan.set_grad_mode(False)
    out.update({f"d{n}": g for n, g in zip(GROUPS, grads)})      # (per group: the list of its layers' gradients)
    return out


def _same(got, want, keys, what):
    for k in keys:
        if k not in want and k not in got:
            continue
        so.assert_same_bits({k: got[k]}, {k: want[k]}, f"{what}: {k}")


def _check_pooled_value(y_last, y_all, lengths, mode, T, what):
    """y_last against the same call's y_all."""
    v = y_all.cpu().numpy()
    got = y_last.cpu().numpy()
    assert np.abs(v).max() < 1.0                                       # (the premise of the mean's bound: |h| < 1)
    if mode == "max":
        want = rref.pooled(v, lengths, "max")
        assert np.array_equal(got, want), (what, float(np.abs(got - want).max()))
    else:
        n = np.array(rref.rows(lengths, *v.shape[:2]), np.float64)[:, None]
        exact = np.where(n > 0, v.astype(np.float64).sum(axis=1) / np.maximum(n, 1), 0.0)
        err, bound = np.abs(got.astype(np.float64) - exact), rref.mean_bound(got, T)
        print(f"{what}: mean error {err.max():.3e}, largest error / bound {float((err / bound).max()):.3f}")
        assert (err <= bound).all(), (what, float((err / bound).max()))
    for b, k in enumerate(rref.rows(lengths, *v.shape[:2])):
        if k == 0:
            assert not got[b].any() and not np.signbit(got[b]).any(), (what, "a row of length 0 gives zeros")


# ---- 1. forward -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", rref.MODES)
@pytest.mark.parametrize("name", list(REGIMES))
def test_forward_pools_the_calls_own_y_all(cuda, name, mode):
    r, plan, w, a = _world(name)
    B, T = r["shape"][:2]
    for lengths in ([None, _lengths(B, T)] if r["state"] else [None]):
        what = f"{name} {mode} lengths {'yes' if lengths else 'no'}"
        got = _call(plan, w, a, mode, lengths, backward=False)
        again = _call(plan, w, a, mode, lengths, backward=False)
        last = _call(plan, w, a, "last", lengths, backward=False)
        _check_pooled_value(got["y_last"], got["y_all"], lengths, mode, T, what)
        _same(again, got, ("y_last", "y_all", "h_n", "c_n"), what + " (second call)")
        _same(got, last, ("y_all", "h_n", "c_n"), what + " (against last)")
        if lengths is None:
            assert not so.same_bits(got["y_last"], last["y_last"])
    torch.cuda.synchronize()
    assert plan.status() == 0


def test_an_inference_plan_pools_too(cuda):
    r = REGIMES["p0_h32_bf16"]
    plan, (w, a) = _plan(r, training=False), _inputs(r["shape"])
    lengths = _lengths(*r["shape"][:2])
    for mode in rref.MODES:
        got = _call(plan, w, a, mode, lengths, backward=False)
        _check_pooled_value(got["y_last"], got["y_all"], lengths, mode, r["shape"][1], f"inference {mode}")


# ---- 2. the backward identity ---------------------------------------------------------------------------------------------
def _identity(plan, w, a, mode, lengths, with_dy_all, state_grads, accumulate, what):
    d = plan.desc
    got = _call(plan, w, a, mode, lengths, a["dy_last"], a["dy_all"] if with_dy_all else None, state_grads, accumulate)
    G = torch.from_numpy(rref.expand(a["dy_last"].cpu().numpy(), got["y_all"].cpu().numpy(), lengths, mode)).to(DEV)
    want = _call(plan, w, a, "last", lengths, None, a["dy_all"] + G if with_dy_all else G, state_grads, accumulate)
    _same(got, want, GRAD_KEYS + ("y_all", "h_n", "c_n"), what)
    assert all(bool(torch.isfinite(t).all()) for k in GRAD_KEYS if k in got for t in so._leaves(got[k])), what
    if lengths is not None and state_grads:
        for b in (b for b, n in enumerate(lengths) if n == 0):       # nothing of dy_last reaches an empty row: dh0 = dh_n
            assert so.same_bits(got["dh0"][:, b], a["dh_n"][:, b]) and so.same_bits(got["dc0"][:, b], a["dc_n"][:, b]), what
    return got


@pytest.mark.parametrize("mode", rref.MODES)
@pytest.mark.parametrize("name", list(REGIMES))
def test_backward_is_the_last_mode_call_on_the_expanded_gradient(cuda, name, mode):
    r, plan, w, a = _world(name)
    B, T = r["shape"][:2]
    cases = [("dy_last", None, False, False, False), ("dy_last + dy_all", None, True, False, False),
             ("dy_last + dy_all, accumulate", None, True, False, True)]
    if r["state"]:
        n = _lengths(B, T)
        cases += [("dy_last + dh_n + dc_n", None, False, True, False), ("dy_last, lengths", n, False, False, False),
                  ("everything, lengths", n, True, True, False), ("everything, lengths, accumulate", n, True, True, True)]
    seen = {}
    for label, lengths, with_dy_all, state_grads, accumulate in cases:
        seen[label] = _identity(plan, w, a, mode, lengths, with_dy_all, state_grads, accumulate, f"{name} {mode} {label}")
    assert not so.same_bits(seen["dy_last"]["dweight_hh"][0], seen["dy_last + dy_all"]["dweight_hh"][0])
    torch.cuda.synchronize()
    assert plan.status() == 0


# ---- 3. ties under MAX ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("reverse", [False, True], ids=["plain", "reverse"])
def test_max_gradient_lands_on_the_first_caller_time_of_a_tie(cuda, reverse):
    shape = (5, 24, 8, 32, 1)
    B, T, I, H, _ = shape
    w, a = _inputs(shape, params=rref.saturated_params(I, H))
    a["x"] = torch.from_numpy(np.random.default_rng(6).standard_normal((B, T, I)).astype(np.float32)).to(DEV)
    plan = cabi.LstmPlan(*shape, BF16, DEV, training=True, state=True, reverse=reverse)
    a0 = dict(a, h0=torch.zeros_like(a["h0"]), c0=torch.zeros_like(a["c0"]))
    got = _call(plan, w, a0, "max", None, a["dy_last"])
    v = got["y_all"].cpu().numpy()
    tied = rref.tied_columns(v)
    assert tied.mean() >= 0.5, f"only {tied.mean():.2f} of the columns tie: the fixture proves nothing"
    assert (v.max(axis=1) == 1.0).mean() >= 0.5                          # saturated at exactly bf16 1.0
    first = rref.first_max(v)
    # (the recurrence of a reverse plan saturates towards the caller's time 0: the first caller time is its LAST step)
    assert (first[tied] == 0).all() if reverse else (first[tied] > 0).all()
    G = torch.from_numpy(rref.expand(a["dy_last"].cpu().numpy(), v, None, "max")).to(DEV)
    want = _call(plan, w, a0, "last", None, None, G)
    _same(got, want, GRAD_KEYS, f"ties reverse={reverse}")
    # ... and the comparison can tell.  The saturated gates pass nothing on (o (1 - o) is exactly 0 in float32): what is left
    # of dy is the cell-state gradient dh o (1 - tanh(c)^2) carried down to dc0, which is non-zero from the step where h
    # first rounds to 1 (c about 4) and exactly zero from c about 10 on -- the same gradient on the LAST maximum of every
    # column gives another dc0
    last = (T - 1) - rref.first_max(v[:, ::-1])
    G_last = torch.zeros_like(G)
    G_last[torch.arange(B, device=DEV)[:, None], torch.from_numpy(last).to(DEV), torch.arange(H, device=DEV)[None, :]] = a["dy_last"]
    assert int((last != first).sum()) >= B * H // 2
    other = _call(plan, w, a0, "last", None, None, G_last)
    assert not so.same_bits(other["dc0"], got["dc0"]) and bool(got["dc0"].any() or other["dc0"].any())


# ---- 4. plan features -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", rref.MODES)
@pytest.mark.parametrize("reverse", [False, True], ids=["plain", "reverse"])
def test_every_plan_feature_at_once(cuda, reverse, mode):
    """Lengths, input windows, inter-layer dropout at p 0.5 and pitched y_all / dy_all on one plan."""
    shape = (5, 37, 24, 32, 2)
    B, T, I, H, L = shape
    GAP, S, TSRC = 4, 3, 50
    w, a = _inputs(shape, seed=8)
    lengths, rows, starts = _lengths(B, T), [2, 0, 1, 2, 0], [13, 50, 49, 1, 7]
    src = torch.randn(S, TSRC, I, generator=torch.Generator().manual_seed(9)).to(DEV)
    plan = cabi.LstmPlan(*shape, BF16, DEV, training=True, state=True, dropout=True, reverse=reverse)
    plan.set_lengths(lengths)
    plan.set_dropout(0.5, 0x1234ABCD5678, 3)
    plan.set_io(H + GAP, H + GAP, False)
    plan.set_views(rows, starts, S, TSRC)
    pad = _pad(lengths, B, T)

    def run(readout, dy_last, dy_all):
        plan.set_readout(readout)
        y_buf = torch.full((B, T, H + GAP), 7.0, device=DEV)
        y_last, _, h_n, c_n = plan.forward(src, *w, want_state=True, y_all=y_buf[:, :, :H], h0=a["h0"], c0=a["c0"])
        dy_buf = torch.full((B, T, H + GAP), NAN, device=DEV)
        dy_buf[:, :, :H] = torch.where(pad, torch.full_like(dy_all, NAN), dy_all)
        grads = [[torch.full_like(p, NAN) for p in group] for group in w]
        out = dict(y_last=y_last, y_buf=y_buf, h_n=h_n, c_n=c_n, dx=torch.full((B, T, I), NAN, device=DEV),
                   dh0=torch.full((L, B, H), NAN, device=DEV), dc0=torch.full((L, B, H), NAN, device=DEV))
        plan.backward(dy_last, dy_buf[:, :, :H], grads, dx=out["dx"], dh_n=a["dh_n"], dc_n=a["dc_n"], dh0=out["dh0"], dc0=out["dc0"])
        out.update({f"d{n}_l{k}": t for n, g in zip(GROUPS, grads) for k, t in enumerate(g)})
        return out

    got = run(mode, a["dy_last"], a["dy_all"])
    y_all = got["y_buf"][:, :, :H].contiguous()
    assert bool((got["y_buf"][:, :, H:] == 7.0).all())
    _check_pooled_value(got["y_last"], y_all, lengths, mode, T, f"features reverse={reverse} {mode}")
    G = torch.from_numpy(rref.expand(a["dy_last"].cpu().numpy(), y_all.cpu().numpy(), lengths, mode)).to(DEV)
    want = run("last", None, a["dy_all"] + G)
    keys = [k for k in got if k != "y_last"]
    so.assert_same_bits({k: got[k] for k in keys}, {k: want[k] for k in keys}, f"features reverse={reverse} {mode}")
    torch.cuda.synchronize()
    assert plan.status() == 0


@pytest.mark.parametrize("mode", rref.MODES)
def test_output_dropout_leaves_the_pooled_value_alone(cuda, mode):
    r = REGIMES["p0_h32_bf16"]
    B, T, I, H, L = r["shape"]
    plan, (w, a) = _plan(r), _inputs(r["shape"])
    lengths = _lengths(B, T)
    clean = _call(plan, w, a, mode, lengths, backward=False)
    plan.set_output_dropout(0.5, 0xFEEDFACE, 1, first=0, index_pitch=H)
    dropped = _call(plan, w, a, mode, lengths, backward=False)
    plan.set_output_dropout(0.0)
    assert so.same_bits(dropped["y_last"], clean["y_last"])
    kept = dropped["y_all"] != 0
    assert 0.3 < float(kept.float().mean()) / (sum(lengths) / (B * T)) < 0.7         # the mask was on, at p = 0.5
    assert bool((dropped["y_all"][kept] == 2.0 * clean["y_all"][kept]).all())
    _check_pooled_value(dropped["y_last"], clean["y_all"], lengths, mode, T, f"output dropout {mode}")


# ---- 5. the sticky setter -------------------------------------------------------------------------------------------------
def test_setter_refusals_on_real_plans_keep_the_setting(cuda):
    lib = cabi.load()
    r = REGIMES["p0_h32_bf16"]
    w, a = _inputs(r["shape"])
    for bits in (dict(), dict(state=False), dict(reverse=True), dict(dropout=True), dict(resident=True), dict(training=False)):
        plan = _plan(r, **bits)
        cpu_checks.check_set_readout_arguments(lib, plan._plan)
    plan = _plan(r)
    plan.set_readout("mean")
    assert lib.csn_lstm_plan_set_readout(plan._plan, 5) == 1          # refused: the plan still pools
    plan.set_lengths(None)
    y_last, y_all = plan.forward(a["x"], *w, want_all=True)
    _check_pooled_value(y_last, y_all, None, "mean", r["shape"][1], "kept setting")
    ws = cabi.load().csn_lstm_plan_workspace_bytes(plan._plan)
    for mode in ("max", "last"):
        plan.set_readout(mode)
        assert cabi.load().csn_lstm_plan_workspace_bytes(plan._plan) == ws


@pytest.mark.parametrize("name", ["p0_h32_bf16", "p5_h96_bf16", "p3_ks384_gemm", "p4_f32p_256"])
def test_last_after_mean_is_a_fresh_plans_call(cuda, name):
    r = REGIMES[name]
    w, a = _inputs(r["shape"])
    used, fresh = _plan(r), _plan(r)
    for plan in (used, fresh):
        plan.profile_enable(True)
    lengths = _lengths(*r["shape"][:2]) if r["state"] else None
    for mode in ("mean", "max"):
        _call(used, w, a, mode, lengths, a["dy_last"], a["dy_all"], r["state"])
    got = _call(used, w, a, "last", lengths, a["dy_last"], a["dy_all"], r["state"])
    want = _call(fresh, w, a, "last", lengths, a["dy_last"], a["dy_all"], r["state"])
    torch.cuda.synchronize()
    _same(got, want, GRAD_KEYS + ("y_last", "y_all", "h_n", "c_n"), f"{name} last after mean")
    if r["state"]:
        assert so.same_bits(got["y_last"], got["h_n"][-1])              # under CSN_READOUT_LAST h_n[L-1] == y_last
    p_used, p_fresh = used.profile_read(), fresh.profile_read()
    for k in ("fwd_launches", "fwd_cells", "bwd_launches", "bwd_cells"):
        # (the per-step cells of path 0 are not counted by the profile: 0 on both plans there)
        assert p_used[k] == p_fresh[k] and (p_used[k] > 0 or r["path"] == 0), (k, p_used, p_fresh)
    assert used.status() == 0 and fresh.status() == 0


# ---- 6. modules -----------------------------------------------------------------------------------------------------------
MB, MT, MI, MH, ML = 5, 37, 24, 32, 2
M_LENGTHS = (37, 0, 1, 36, 20)


def _module_x(seed=11):
    return torch.randn(MB, MT, MI, generator=torch.Generator().manual_seed(seed)).to(DEV)


def _torch_mean(output, lengths):
    """(output * mask).sum(1) / n: torch's backward of it hands every valid step the float32 quotient dy / n."""
    n = torch.tensor(lengths, device=DEV)
    mask = (torch.arange(output.shape[1], device=DEV)[None, :] < n[:, None])[:, :, None].float()
    return (output * mask).sum(1) / n.clamp(min=1)[:, None].float()      # (n = 0: the masked sum is zero already)


def _param_grads(m, loss):
    for p in m.parameters():
        p.grad = None
    loss.backward()
    return {k: p.grad.clone() for k, p in m.named_parameters()}


@pytest.mark.parametrize("mode", rref.MODES)
def test_hiplstm_readout(cuda, mode):
    torch.manual_seed(12)
    m = HipLSTM(MI, MH, ML, readout=mode).to(DEV)
    x = _module_x()
    y_all, y = m(x, want_all=True)
    assert y.shape == (MB, MH) and so.same_bits(m(x), y)
    _check_pooled_value(y.detach(), y_all.detach(), None, mode, MT, f"HipLSTM {mode}")
    assert all(pl.status() == 0 for pl in m.all_plans())
    if mode == "mean":
        dyw = torch.randn(MB, MH, generator=torch.Generator().manual_seed(13)).to(DEV)
        got = _param_grads(m, (m(x) * dyw).sum())
        twin = HipLSTM(MI, MH, ML).to(DEV)
        twin.load_state_dict(m.state_dict())
        want = _param_grads(twin, (_torch_mean(twin(x, want_all=True)[0], [MT] * MB) * dyw).sum())
        so.assert_same_bits(got, want, "HipLSTM mean parameter gradients")


@pytest.mark.parametrize("mode", rref.MODES)
@pytest.mark.parametrize("cls", [LSTM, BiLSTM], ids=["LSTM", "BiLSTM"])
def test_drop_in_pooled(cuda, cls, mode):
    torch.manual_seed(14)
    m = cls(MI, MH, ML).to(DEV)
    dirs = 2 if cls is BiLSTM else 1
    x = _module_x()
    g = torch.Generator().manual_seed(15)
    hx = tuple(t.to(DEV) for t in (0.5 * torch.randn(dirs * ML, MB, MH, generator=g), torch.randn(dirs * ML, MB, MH, generator=g)))
    dyw = torch.randn(MB, dirs * MH, generator=g).to(DEV)
    for lengths in (None, M_LENGTHS):
        what = f"{cls.__name__}.pooled {mode} lengths {lengths is not None}"
        with torch.no_grad():
            y = m.pooled(x, hx, lengths=lengths, readout=mode)
            output, _ = m(x, hx, lengths=lengths)
        assert y.shape == (MB, dirs * MH)
        _check_pooled_value(y, output, lengths, mode, MT, what)
        if mode == "mean":
            xg = x.clone().requires_grad_(True)
            got = _param_grads(m, (m.pooled(xg, hx, lengths=lengths) * dyw).sum())
            got["x"] = xg.grad.clone()
            xg = x.clone().requires_grad_(True)
            want = _param_grads(m, (_torch_mean(m(xg, hx, lengths=lengths)[0], lengths or [MT] * MB) * dyw).sum())
            want["x"] = xg.grad.clone()
            so.assert_same_bits(got, want, what + " gradients")
    packed = torch.nn.utils.rnn.pack_padded_sequence(x[[0, 3, 4]], torch.tensor([37, 36, 20]), batch_first=True)
    hx3 = tuple(t[:, [0, 3, 4]].contiguous() for t in hx)
    with torch.no_grad():
        assert so.same_bits(m.pooled(packed, hx3, readout=mode), m.pooled(x[[0, 3, 4]], hx3, lengths=[37, 36, 20], readout=mode))
    assert all(pl.status() == 0 and not pl.busy for pl in m.all_plans())


@pytest.mark.parametrize("mode", rref.MODES)
@pytest.mark.parametrize("bidirectional", [False, True], ids=["uni", "bi"])
def test_model_readout_with_and_without_views(cuda, bidirectional, mode):
    """Model(readout=): fc reads the pooled output.  Held against fc of the restatement's pooling of the drop-in's own output
    (a drop-in on the model's parameters): under "max" the same bits, under "mean" within |W| times the mean's bound."""
    torch.manual_seed(16)
    D = 16
    model = Model(MI, MH, ML, D, include_top=False, bidirectional=bidirectional, readout=mode).to(DEV).eval()
    drop_in = (BiLSTM if bidirectional else LSTM)(MI, MH, ML).to(DEV)
    drop_in.load_state_dict(model.lstm.state_dict())
    src = torch.randn(3, 50, MI, generator=torch.Generator().manual_seed(17)).to(DEV)
    views, lengths = ([2, 0, 1, 2, 0], [13, 50, 49, 1, 7]), list(M_LENGTHS)
    with torch.no_grad():
        for what, feat, (output, _), n in (("dense", model(src[:, :MT]), drop_in(src[:, :MT].contiguous()), None),
                                           ("views", model(src, views=views, lengths=lengths), drop_in(src, None, lengths, views), lengths)):
            assert feat.shape == (len(output), D)
            pooled = torch.from_numpy(rref.pooled(output.cpu().numpy(), n, mode)).to(DEV)
            want = model.fc(pooled)
            if mode == "max":
                assert so.same_bits(feat, want), (what, float((feat - want).abs().max()))
            else:
                bound = float(model.fc.weight.abs().sum(1).max()) * 2.0 ** -23 + 1e-6       # (|W| 1 times the bound on the input, + fc's own rounding)
                assert float((feat - want).abs().max()) <= bound, (what, float((feat - want).abs().max()), bound)
    model.train()
    feat = model(src, views=views, lengths=lengths)
    feat.square().sum().backward()
    assert all(p.grad is not None and bool(torch.isfinite(p.grad).all()) for p in model.parameters())
    assert all(pl.status() == 0 and not pl.busy for pl in model.lstm.all_plans())


def test_cli_train_then_eval_with_mean_readout(cuda, tmp_path, monkeypatch):
    import LstmDistillFromDinoV2Eval as evaluate_cli
    import LstmDistillFromDinoV2Train as train
    from cerebralsignalnetworks_amd.trainer import DistillTrainer
    args = ["--synthetic", "64", "--batch_size", "16", "--num_epochs", "1", "--log_dir", str(tmp_path), "--hidden_size", "32",
            "--lstm_layers", "2", "--loss", "cosine", "--output_size", "24", "--dtype", "bf16", "--readout", "mean"]
    hist = train.main(args)
    assert len(hist) == 1 and np.isfinite(hist[0])
    ckpt = os.path.join(str(tmp_path), "lstm_dinov2_best_loss.pth")
    seen = []
    embed_all = DistillTrainer.embed_all

    def spy(self, eeg_all, batch):
        out = embed_all(self, eeg_all, batch)
        seen.append((self, eeg_all.clone(), batch, out.clone()))
        return out
    monkeypatch.setattr(DistillTrainer, "embed_all", spy)
    r = evaluate_cli.main(args + ["--custom_model_weights", ckpt, "--topK", "5"])
    monkeypatch.setattr(DistillTrainer, "embed_all", embed_all)
    assert 0.0 <= r["Recall_Total"] <= 100.0 and len(seen) == 2
    trainer, eeg, batch, emb = seen[0]
    assert trainer.model.lstm.readout == "mean"
    outs = {}
    for readout in ("mean", "last"):
        model = Model(input_size=eeg.shape[1], lstm_size=32, lstm_layers=2, output_size=24, include_top=False, compute_dtype=torch.bfloat16,
                      readout=readout).to(DEV)
        evaluate_cli.load_checkpoint_into(model, ckpt)
        outs[readout] = DistillTrainer(model, trainer.sos, loss="cosine").embed_all(eeg, batch)
    assert so.same_bits(outs["mean"], emb) and not so.same_bits(outs["last"], emb)


# ---- 7. stream order ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", stream_cases.MODES)
def test_pooled_calls_on_a_side_stream_with_late_inputs(cuda, mode):
    """The procedure of tests/test_gpu_stream_order.py on the case of tests/lstm_readout_stream_cases.py: the pooling
    reduction behind the recurrence, then the argmax pre-pass and the pooled dy_in, each with its inputs late behind a Delay
    and overwritten directly behind the call."""
    t0 = time.perf_counter()
    shape, lengths = stream_cases.SHAPE, list(stream_cases.LENGTHS)
    B, T, I, H, L = shape
    plan = cabi.LstmPlan(*shape, BF16, DEV, training=True, state=True)
    w, a = _inputs(shape, seed=21)
    fwd_in = {"x": a["x"], "w": w, "h0": a["h0"], "c0": a["c0"]}
    bwd_in = {k: a[k] for k in ("dy_last", "dy_all", "dh_n", "dc_n")}
    plan.set_lengths(lengths)
    plan.set_readout(mode)

    def forward(f):
        return dict(zip(("y_last", "y_all", "h_n", "c_n"), plan.forward(f["x"], *f["w"], want_all=True, want_state=True, h0=f["h0"], c0=f["c0"])))

    def backward(g):
        out = dict(dx=torch.full((B, T, I), NAN, device=DEV), dh0=torch.full((L, B, H), NAN, device=DEV), dc0=torch.full((L, B, H), NAN, device=DEV))
        grads = [[torch.full_like(p, NAN) for p in group] for group in w]
        plan.backward(g["dy_last"], g["dy_all"], grads, dx=out["dx"], dh_n=g["dh_n"], dc_n=g["dc_n"], dh0=out["dh0"], dc0=out["dc0"])
        out["grads"] = grads
        return out

    torch.cuda.synchronize()
    want_fwd = forward(fwd_in)
    want_bwd = backward(bwd_in)
    torch.cuda.synchronize()
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        forward(fwd_in)
        backward(bwd_in)
        s.synchronize()
        _, t_fwd = so.timed(lambda: forward(fwd_in))
        s.synchronize()
        _, t_bwd = so.timed(lambda: backward(bwd_in))
        s.synchronize()
        plan.workspace.fill_(0xff)      # (the warm-up ran on these very inputs: forget what it left in the workspace)
        cabi._check(cabi.load().csn_lstm_workspace_init(plan._plan, plan._ws_ptr, cabi._stream()))
        s.synchronize()
    delay, late = so.late_all(s, fwd_in, so.delay_ms_for(t_fwd))
    with torch.cuda.stream(s):
        out = forward(late)
    running_fwd = delay.still_running()
    snaps_fwd = so.snapshot_then_poison(s, out, late)
    delay2, late_g = so.late_all(s, bwd_in, so.delay_ms_for(t_bwd))
    with torch.cuda.stream(s):
        out = backward(late_g)
    running_bwd = delay2.still_running()
    snaps_bwd = so.snapshot_then_poison(s, out, late_g)
    s.synchronize()
    print(f"stream order readout {mode}: t_host {1e3 * t_fwd:.2f} / {1e3 * t_bwd:.2f} ms, delays ran {delay.measured_ms():.1f} / "
          f"{delay2.measured_ms():.1f} ms, still running at return: {running_fwd} / {running_bwd}, wall {time.perf_counter() - t0:.2f} s")
    assert running_fwd and running_bwd
    so.assert_same_bits(snaps_fwd, want_fwd, f"readout {mode} forward")
    so.assert_same_bits(snaps_bwd, want_bwd, f"readout {mode} backward")
    assert plan.status() == 0
