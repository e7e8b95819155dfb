"""GPU: the stream contract of every entry point that takes a csnStream_t (include/csn_hip.h, "Stream contract").

Every test runs on a fresh non-blocking side stream while the default stream stays idle, and nothing but the stream's own
order stands between the inputs and the call (tests/stream_order.py):

  1. a reference run of the same plan / entry point on the same inputs, on the default stream, the device synchronised
     before and after it;
  2. twice, the two required to be equal bit for bit (every entry point was: none needed a bound instead);
  3. one warm-up call on the side stream (lazy allocations, dynamic-LDS attributes, the plan's side streams), a second one
     whose host time t_host is taken;
  4. the inputs LATE behind a Delay of at least 3 t_host + 20 ms, the call, snapshot_then_poison, ONE stream.synchronize();
  5. the Delay was still running when the call returned to the host (printed: "delay still running at return"), every
     snapshot has the bits of the reference run, and a plan's status word is 0.

Shapes are the smallest that take their path: the LSTM's from CASES of tests/test_gpu_lstm_state.py, one per path, the
plan's path and kernels checked as there.  Each test prints t_host, the Delay and its wall time.

The launches, copies and host staging that inter-layer dropout, reverse plans with csn_lstm_plan_set_io, input windows and
the gradient-ready callback add to the forward and backward run under the same five steps (so.FEATURE_SETS on
FEATURE_NAMES; settings changed between unsynchronised calls; the callback's point; BiLSTM through autograd).  In those
tests the workspace is filled with 0xff and initialised again in front of the late call (_forget_workspace): the warm-up
calls ran on the late call's own inputs, and a launch that runs too early would otherwise find the right values of the
call before it in the workspace.

Measured on one MI355X, one process: the whole file 233 tests, 24.7 s in pytest (27.5 s wall with start-up); the 105 tests
the file held before the feature tests 13.0 s (15.4 s wall) in the same session; the 128 feature tests 12.4 s in all, the
slowest 1.0 s (the first BiLSTM case, which creates the module's plans), every other one under 0.4 s."""
import os
import time

import numpy as np
import pytest
import torch

import stream_order as so
import test_gpu_bilstm as bl
import test_gpu_lstm_state as st
import test_gpu_lstm_views as vw
from cerebralsignalnetworks_amd import cabi, Model
from cerebralsignalnetworks_amd.trainer import DistillTrainer

pytestmark = pytest.mark.gpu

DEV = st.DEV
NAN = so.NAN


def _report(what, t_host, delay, t0, running=None):
    line = f"stream order {what}: t_host {1e3 * t_host:.2f} ms, delay asked {delay.ms:.1f} ms ran {delay.measured_ms():.1f} ms"
    if running is not None:
        line += f", delay still running at return: {running}"
    print(line + f", wall {time.perf_counter() - t0:.2f} s")


def _clone(tree):
    return so._map(tree, lambda t: t.clone())


def _synced(fn):
    torch.cuda.synchronize()
    out = fn()
    torch.cuda.synchronize()
    return out


# ---------------------------------------------------------------------------------------------------------------------------
# stateless entry points
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", so.STATELESS_CASES, ids=lambda c: c.id)
def test_stateless_entry_point_with_late_inputs(cuda, case):
    t0 = time.perf_counter()
    ins, call = case.build(cuda)
    want = _synced(lambda: call(_clone(ins)))
    so.assert_same_bits(_synced(lambda: call(_clone(ins))), want, f"{case.id}: second synchronised run")
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        call(_clone(ins))
        s.synchronize()
        a = _clone(ins)
        s.synchronize()
        _, t_host = so.timed(lambda: call(a))
    s.synchronize()
    delay, a = so.late_all(s, ins, so.delay_ms_for(t_host))
    with torch.cuda.stream(s):
        out = call(a)
    running = delay.still_running()
    snaps = so.snapshot_then_poison(s, out, a)
    s.synchronize()
    _report(case.id, t_host, delay, t0, running)
    assert running, "the call returned only after the Delay had drained: it blocked the host, or the Delay is too short"
    so.assert_same_bits(snaps, want, case.id)
    for k, t in a.items():          # the inputs really were overwritten behind the call
        assert bool(torch.isnan(t).all()) if t.is_floating_point() else bool((t == so.INT_POISON).all()), k


# ---------------------------------------------------------------------------------------------------------------------------
# LSTM plans
# ---------------------------------------------------------------------------------------------------------------------------
# beside CASES of tests/test_gpu_lstm_state.py, as (shape, dtype, expected plan, environment, CSN_LSTM_STATE plan?):
#   the per-layer-stream form of forward_persist (csrc/lstm.hip; every path 2 / 3 shape of CASES takes the grouped form):
#   forced by CSN_PERSIST_STREAMS, and taken on its own by 2 slots x 5 row tiles > 8 hand-off groups.  Either way the
#   backward then is the per-diagonal one ON A PATH 3 PLAN, which the expected kernel names show.
#   path 4, the exact-float32 weight-stationary recurrence, which takes no state: a plan without CSN_LSTM_STATE.
EXTRA_CASES = {
    "streams_env_h768": ((64, 40, 128, 768, 2), st.BF16, (3, st._PF, st._ILB), {"CSN_PERSIST_STREAMS": "1"}, True),
    "streams_b320_h256": ((320, 40, 32, 256, 2), st.BF16, (3, st._PF, st._ILB), {}, True),
    "p4_f32_h128": ((70, 37, 24, 128, 2), st.F32, (4, "lstm_fwd_f32_persist_kernel", "lstm_bwd_f32_persist_kernel"), {}, False),
}
LSTM_CASES = ("v1_h96", "p1_l5", "p2_nopersist_bwd", "ks_fused_h768_t32", "ns_fused_h1024_t33", "chunk4_l3", "f32_h128",
              "ref_h128_l4") + tuple(EXTRA_CASES)
# which form of forward_persist each path 2 / 3 case must take (asserted against the mirror of its rule below)
STREAM_FORM = {"p2_nopersist_bwd": False, "ks_fused_h768_t32": False, "ns_fused_h1024_t33": False, "chunk4_l3": False,
               "ref_h128_l4": False, "streams_env_h768": True, "streams_b320_h256": True}


def _case(name):
    return EXTRA_CASES[name] if name in EXTRA_CASES else st.CASES[name] + (True,)


def _forward_takes_layer_streams(shape, env, fwd_kernel):
    """Mirror of forward_persist() in csrc/lstm.hip: the grouped form needs at most 4 slots, slots x row tiles <= 8, at
    most 32 slices and no CSN_PERSIST_STREAMS; otherwise every layer >= 1 runs on a stream of its own, provided all
    layers' workgroups fit the chip together (L x slices x row tiles <= 256; else everything stays on the caller's)."""
    B, T, I, H, L = shape
    chunk = int(env.get("CSN_LSTM_CHUNK", 32))
    slots, mt = min(L, -(-T // chunk)), -(-B // 64)
    slices = H // 32 if fwd_kernel == st._NSF else H // (4 * (6 if H % 24 == 0 else 8))
    grouped = slots <= 4 and slots * mt <= 8 and slices <= 32 and env.get("CSN_PERSIST_STREAMS") != "1"
    return not grouped and L * slices * mt <= 256
# one per path family: generic cells, per-diagonal, weight-stationary forward, weight-stationary both, float32
LENGTHS_CASES = ("v1_h96", "p1_l5", "p2_nopersist_bwd", "ks_fused_h768_t32", "f32_h128")
GROUPS = ("w_ih", "w_hh", "b_ih", "b_hh")
LR = 1e-2


class _Lstm:
    """One CSN_LSTM_STATE plan of a case of test_gpu_lstm_state.CASES, its real inputs (ready) and the synchronised
    reference runs.  features: a name of so.FEATURE_SETS, or a settings dict as so.feature_settings returns one -- the
    plan then carries the dropout and / or reverse bit and the sticky settings (so.feature_settings):
      dropout     set_dropout(p, seed, subsequence), set again before every backward;
      reverse_io  a reverse plan under set_io(2H, 2H, dx_add): forward() writes y_all into the right half of a [B, T, 2H]
                  buffer of NaN (the whole buffer is the output "y_all"), backward() reads the left half of the [B, T, 2H]
                  buffer "dy_all" and adds to the values "dx0" (in place: "dx0" is an input and, as "dx", an output);
      windows     set_views: "x" is the source [S, Tsrc, I];  lengths: the two_mixed pattern."""

    def __init__(self, name, lengths=False, features=None):
        shape, dtype, expect, env, state = _case(name)
        self.name, self.shape, self.dtype, self.state = name, shape, dtype, state
        B, T, I, H, L = shape
        if features is not None:
            assert so.FEATURE_CASES[name] == (shape, state) and L >= 2 and not lengths
        none = {"dropout": None, "reverse_io": False, "lengths": None, "views": None}
        f = none if features is None else so.feature_settings(name, features) if isinstance(features, str) else features
        self.f = self.cur = f
        old = {k: os.environ.get(k) for k in env}
        os.environ.update(env)          # the switches are read once, at plan creation
        try:
            # (a plan with the dropout and reverse bits takes the path and kernels of the plan without them)
            self.plan = cabi.LstmPlan(B, T, I, H, L, dtype, DEV, training=True, state=state, dropout=f["dropout"] is not None,
                                      reverse=f["reverse_io"])
            if name in EXTRA_CASES:
                assert (self.plan.path(),) + self.plan.kernel_names() == expect and self.plan.status() == 0
            else:
                st._check_plans([self.plan], expect, T)
            if name in STREAM_FORM:
                assert self.plan.path() in (2, 3)
                assert _forward_takes_layer_streams(shape, env, self.plan.kernel_names()[0]) == STREAM_FORM[name]
        finally:
            for k, v in old.items():
                os.environ.pop(k, None) if v is None else os.environ.__setitem__(k, v)
        if f["reverse_io"]:
            self.plan.set_io(2 * H, 2 * H, dx_add=True)
        self.apply(f)
        g = torch.Generator(device="cpu").manual_seed(5)
        k = 1.0 / np.sqrt(H)

        def u(*s):
            return ((2 * torch.rand(*s, generator=g) - 1) * k).to(DEV)

        def n(*s, scale=1.0):
            return (scale * torch.randn(*s, generator=g)).to(DEV)
        self.fwd_in = {"x": n(*self.x_shape(f)), "w_ih": [u(4 * H, I if l == 0 else H) for l in range(L)],
                       "w_hh": [u(4 * H, H) for _ in range(L)], "b_ih": [u(4 * H) for _ in range(L)],
                       "b_hh": [u(4 * H) for _ in range(L)], "h0": n(L, B, H, scale=0.5), "c0": n(L, B, H)}
        self.bwd_in = {"dy_last": n(B, H), "dy_all": n(B, T, H), "dh_n": n(L, B, H), "dc_n": n(L, B, H)}
        if not state:
            for k_ in ("h0", "c0"):
                self.fwd_in[k_] = None
            for k_ in ("dh_n", "dc_n"):
                self.bwd_in[k_] = None
        self.grads0 = {k_: [n(*w.shape, scale=0.25) for w in self.fwd_in[k_]] for k_ in GROUPS}     # accumulate mode: what is there before
        if f["reverse_io"]:
            self.bwd_in["dy_all"] = torch.cat([self.bwd_in["dy_all"], torch.full((B, T, H), NAN, device=DEV)], dim=2)
            self.bwd_in["dx0"] = n(B, T, I)
        self._n = n
        self.lengths = None
        if lengths:
            rng = np.random.default_rng(1000)           # "random_with_zeros" of tests/test_gpu_lstm_lengths.py
            ln = rng.integers(0, T + 1, B).tolist()
            ln[0], ln[1], ln[B - 1] = T, 0, 0
            self.lengths = [int(v) for v in ln]
            self.plan.set_lengths(self.lengths)
        torch.cuda.synchronize()
        self.want_fwd = _synced(lambda: self.forward(self.fwd_in))
        so.assert_same_bits(_synced(lambda: self.forward(self.fwd_in)), self.want_fwd, f"{name}: second synchronised forward")
        self.want_bwd = {}
        for mode in ("overwrite", "accumulate"):
            self.want_bwd[mode] = _synced(lambda: self.backward(self.bwd_in, self.grads_for(mode), mode))
            _synced(lambda: self.forward(self.fwd_in))
            so.assert_same_bits(_synced(lambda: self.backward(self.bwd_in, self.grads_for(mode), mode)), self.want_bwd[mode],
                                f"{name}: second synchronised backward, {mode}")
            _synced(lambda: self.forward(self.fwd_in))
        self._check_features_are_on()
        assert self.plan.status() == 0

    def x_shape(self, f):
        B, T, I, H, L = self.shape
        return (B, T, I) if f["views"] is None else (f["views"][2], f["views"][3], I)

    def apply(self, f):
        """The sticky settings `f` (lengths, windows, dropout triple) from now on; host only."""
        if f["lengths"] is not None:
            self.plan.set_lengths(f["lengths"])
        if f["views"] is not None:
            self.plan.set_views(*f["views"])
        if f["dropout"] is not None:
            self.plan.set_dropout(*f["dropout"])
        self.cur = f

    def _check_features_are_on(self):
        """Once per plan: the dropout mask really is applied, the pitched y_all leaves its other half alone, and the
        windowed run has the bits of the run on the materialised dense input."""
        B, T, I, H, L = self.shape
        f = self.f
        if f["reverse_io"]:
            assert self.want_fwd["y_all"].shape == (B, T, 2 * H) and bool(torch.isnan(self.want_fwd["y_all"][:, :, :H]).all())
            assert bool(torch.isfinite(self.want_fwd["y_all"][:, :, H:]).all())
        if f["dropout"] is not None:
            self.plan.set_dropout(0.0)
            off = _synced(lambda: self.forward(self.fwd_in))
            self.plan.set_dropout(*f["dropout"])
            assert not so.same_bits(off["y_all"], self.want_fwd["y_all"]), f"{self.name}: the dropout mask changed nothing"
        if f["views"] is not None:
            rows, starts, S, Tsrc = f["views"]
            n = f["lengths"] or [T] * B
            assert (S, rows, starts) == vw._windows("random", B, Tsrc, n)
            xm = vw._materialise(self.fwd_in["x"], rows, starts, n, T)
            self.plan.set_views(None)
            dense = _synced(lambda: self.forward({**self.fwd_in, "x": xm}))
            self.plan.set_views(*f["views"])
            so.assert_same_bits(dense, self.want_fwd, f"{self.name}: the materialised dense input against the windows")
        if any(f.values()):
            _synced(lambda: self.forward(self.fwd_in))          # the workspace holds the forward the backwards belong to

    def forward(self, a):
        B, T, I, H, L = self.shape
        kw, ybuf = {}, None
        if self.f["reverse_io"]:
            ybuf = torch.full((B, T, 2 * H), NAN, device=DEV)          # (on the current stream, in front of the call)
            kw["y_all"] = ybuf[:, :, H:]
        if self.state:
            kw.update(h0=a["h0"], c0=a["c0"], want_state=True)
        res = self.plan.forward(a["x"], a["w_ih"], a["w_hh"], a["b_ih"], a["b_hh"], want_all=True, **kw)
        out = dict(zip(("y_last", "y_all", "h_n", "c_n"), res))
        if ybuf is not None:
            out["y_all"] = ybuf
        return out

    def grads_for(self, mode):
        """The gradient tensors a backward of `mode` starts from: NaN, or the known values it adds to -- filled on the
        current stream, in front of the call (no host synchronisation: this runs behind a Delay too)."""
        if mode != "accumulate":
            return so._map(self.grads0, lambda t: torch.full_like(t, NAN))
        return _clone(self.grads0)

    def backward(self, g, grads, mode="overwrite"):
        """mode "overwrite_tail": overwriting, without dh0 / dc0 -- whose kernels are the last thing a backward puts on the
        caller's stream, so that with them a reader behind the call is a dozen launches away from the end of the side
        stream's work -- and with the outputs in the order that reads the side stream's LAST results first (the bias
        gradients of layer 0, then its weight gradients, then dx)."""
        B, T, I, H, L = self.shape
        tail = mode == "overwrite_tail"
        dx, dy_all = torch.full((B, T, I), NAN, device=DEV), g["dy_all"]
        if self.f["reverse_io"]:
            dx = g["dx0"].clone() if g is self.bwd_in else g["dx0"]          # dx_add: what dx holds is read
            dy_all = dy_all[:, :, :H]
        if self.cur["dropout"] is not None:
            self.plan.set_dropout(*self.cur["dropout"])          # a backward runs with the setting of its forward
        dh0 = None if tail or not self.state else torch.full((L, B, H), NAN, device=DEV)
        dc0 = None if tail or not self.state else torch.full((L, B, H), NAN, device=DEV)
        self.plan.set_grad_mode(mode == "accumulate")
        try:
            self.plan.backward(g["dy_last"], dy_all, [grads[k] for k in GROUPS], dx=dx, dh_n=g["dh_n"], dc_n=g["dc_n"],
                               dh0=dh0, dc0=dc0)
        finally:
            self.plan.set_grad_mode(False)
        if tail:
            return {**{k: grads[k] for k in reversed(GROUPS)}, "dx": dx}
        return {"dx": dx, "dh0": dh0, "dc0": dc0, **grads}

    # forward, backward, in-place weight update, forward, backward: `sync` = device synchronise after every call
    def two_steps(self, s1, s2, sync):
        def after():
            if sync:
                torch.cuda.synchronize()
        with torch.cuda.stream(s1):
            a = _clone(self.fwd_in)
            g = _clone(self.bwd_in)
            after()
            o1 = self.forward(a)
            after()
            b1 = self.backward(g, self.grads_for("overwrite"))
            after()
        if s2 is not s1:
            s2.wait_stream(s1)
        with torch.cuda.stream(s2):
            for k in GROUPS:
                for w, dw in zip(a[k], b1[k]):
                    w.add_(dw, alpha=-LR)
            a["x"] = a["x"].flip(0)
            after()
            o2 = self.forward(a)
            after()
            b2 = self.backward(g, self.grads_for("overwrite"))
            after()
        return {"step1": {**o1, **b1}, "step2": {**o2, **b2}, "weights": {k: a[k] for k in GROUPS}}, (a, g)


_LSTMS = {}


def _lstm(name, features=None):
    if (name, features) not in _LSTMS:
        _LSTMS.clear()                  # one case's plan and references at a time
        _LSTMS[name, features] = _Lstm(name, features=features)
    return _LSTMS[name, features]


def _warm(s, fn):
    """fn() once on `s` to warm it up, once more for its host time."""
    with torch.cuda.stream(s):
        fn()
        s.synchronize()
        _, t_host = so.timed(fn)
        s.synchronize()
    return t_host


def _forget_workspace(plan):
    """On the current stream: 0xff into every byte of the plan's workspace (a NaN in either compute dtype), then
    csn_lstm_workspace_init -- what a first call finds in memory nobody has used.  The warm-up calls ran on the very
    inputs of the late call, so without this a launch that runs too early reads, from the workspace, the right values of
    the call before it."""
    plan.workspace.fill_(0xff)
    cabi._check(cabi.load().csn_lstm_workspace_init(plan._plan, plan._ws_ptr, cabi._stream()))


@pytest.mark.parametrize("name", LSTM_CASES)
def test_lstm_forward_with_late_inputs(cuda, name):
    """x, the four weight groups, h0 and c0 arrive behind the Delay; behind the call all of them are overwritten."""
    t0 = time.perf_counter()
    c = _lstm(name)
    s = torch.cuda.Stream()
    t_host = _warm(s, lambda: c.forward(c.fwd_in))
    delay, a = so.late_all(s, c.fwd_in, so.delay_ms_for(t_host))
    with torch.cuda.stream(s):
        out = c.forward(a)
    running = delay.still_running()
    snaps = so.snapshot_then_poison(s, out, a)
    s.synchronize()
    _report(f"{name} forward", t_host, delay, t0, running)
    assert running
    so.assert_same_bits(snaps, c.want_fwd, f"{name} forward")
    assert c.plan.status() == 0


@pytest.mark.parametrize("mode", ["overwrite", "accumulate", "overwrite_tail"])
@pytest.mark.parametrize("name", LSTM_CASES)
def test_lstm_backward_with_late_inputs(cuda, name, mode):
    """dy_last, dy_all, dh_n, dc_n (accumulate mode: and what the gradient tensors hold) arrive behind the Delay.  The
    forward before it ran on the same stream without a synchronisation and had its x, weights, h0 and c0 overwritten
    directly behind it: the backward reads none of them (include/csn_hip.h).  overwrite_tail (_Lstm.backward): the
    snapshot directly behind the last launch on the caller's stream -- the form that notices a missing closing join."""
    t0 = time.perf_counter()
    c = _lstm(name)
    s = torch.cuda.Stream()

    def both():
        c.forward(c.fwd_in)
        return c.backward(c.bwd_in, c.grads_for(mode), mode)
    with torch.cuda.stream(s):
        both()
        s.synchronize()
        c.forward(c.fwd_in)
        grads = c.grads_for(mode)
        s.synchronize()
        _, t_host = so.timed(lambda: c.backward(c.bwd_in, grads, mode))
        s.synchronize()
        a = _clone(c.fwd_in)
        c.forward(a)
        so.snapshot_then_poison(s, None, a)          # x, weights, h0, c0 of the forward are gone before the backward runs
    late_in = {"g": c.bwd_in, "grads": c.grads0} if mode == "accumulate" else {"g": c.bwd_in}
    delay, la = so.late_all(s, late_in, so.delay_ms_for(t_host))
    with torch.cuda.stream(s):
        out = c.backward(la["g"], la["grads"] if mode == "accumulate" else c.grads_for(mode), mode)
    running = delay.still_running()
    snaps = so.snapshot_then_poison(s, out, la["g"])
    s.synchronize()
    _report(f"{name} backward {mode}", t_host, delay, t0, running)
    assert running
    want = c.want_bwd["overwrite" if mode == "overwrite_tail" else mode]
    so.assert_same_bits(snaps, {k: want[k] for k in snaps}, f"{name} backward {mode}")
    assert c.plan.status() == 0


@pytest.mark.parametrize("streams", ["one_stream", "second_step_on_a_second_stream"])
@pytest.mark.parametrize("name", LSTM_CASES)
def test_lstm_two_steps_back_to_back(cuda, name, streams):
    """forward, backward, w.add_(g, alpha=-lr) on the stream, forward, backward on one plan with no synchronisation between
    them (the second step on a second stream that waits for the first, or on the same one), all of it enqueued while a
    Delay still holds the stream: equal to the same sequence with a device synchronisation after every call.  Call N + 1
    rewinds the plan's event pool, zeroes its workspace regions and re-lays the weights out while call N's side-stream
    tail has not run yet."""
    t0 = time.perf_counter()
    c = _lstm(name)
    d = torch.cuda.default_stream()
    want, _ = c.two_steps(d, d, sync=True)
    again, _ = c.two_steps(d, d, sync=True)
    so.assert_same_bits(again, want, f"{name}: second synchronised run of the two steps")
    s1 = torch.cuda.Stream()
    s2 = s1 if streams == "one_stream" else torch.cuda.Stream()
    c.two_steps(s1, s2, sync=False)
    torch.cuda.synchronize()
    _, t_host = so.timed(lambda: c.two_steps(s1, s2, sync=False))
    torch.cuda.synchronize()
    delay = so.Delay(s1, so.delay_ms_for(t_host))
    out, ins = c.two_steps(s1, s2, sync=False)
    running = delay.still_running()
    snaps = so.snapshot_then_poison(s2, out, ins)
    s2.synchronize()
    _report(f"{name} two steps, {streams}", t_host, delay, t0, running)
    assert running
    so.assert_same_bits(snaps, want, f"{name} two steps, {streams}")
    assert c.plan.status() == 0


@pytest.mark.parametrize("name", LENGTHS_CASES)
def test_lstm_lengths_with_late_inputs(cuda, name):
    """The late-input forward and backward on a plan with per-row lengths (some 0, one T).  The lengths are host memory and
    are read during the call.  A call with lengths waits on the host for the lengths upload of the plan's PREVIOUS call
    with lengths (include/csn_hip.h): the stream is therefore synchronised once between the forward and the backward here,
    and neither call then blocks."""
    t0 = time.perf_counter()
    _LSTMS.clear()
    c = _Lstm(name, lengths=True)
    s = torch.cuda.Stream()
    t_host = _warm(s, lambda: c.forward(c.fwd_in))
    delay, a = so.late_all(s, c.fwd_in, so.delay_ms_for(t_host))
    with torch.cuda.stream(s):
        out = c.forward(a)
    running = delay.still_running()
    snaps = so.snapshot_then_poison(s, out, a)
    s.synchronize()
    _report(f"{name} lengths forward", t_host, delay, t0, running)
    assert running
    so.assert_same_bits(snaps, c.want_fwd, f"{name} lengths forward")
    for mode in ("overwrite", "accumulate"):
        with torch.cuda.stream(s):
            grads = c.grads_for(mode)
            s.synchronize()
            _, t_host = so.timed(lambda: c.backward(c.bwd_in, grads, mode))
            c.forward(c.fwd_in)
            s.synchronize()
        late_in = {"g": c.bwd_in, "grads": c.grads0} if mode == "accumulate" else {"g": c.bwd_in}
        delay, la = so.late_all(s, late_in, so.delay_ms_for(t_host))
        with torch.cuda.stream(s):
            out = c.backward(la["g"], la["grads"] if mode == "accumulate" else c.grads_for(mode), mode)
        running = delay.still_running()
        snaps = so.snapshot_then_poison(s, out, la["g"])
        s.synchronize()
        _report(f"{name} lengths backward {mode}", t_host, delay, t0, running)
        assert running
        so.assert_same_bits(snaps, c.want_bwd[mode], f"{name} lengths backward {mode}")
        with torch.cuda.stream(s):
            c.forward(c.fwd_in)
        s.synchronize()
    assert c.plan.status() == 0


# ---------------------------------------------------------------------------------------------------------------------------
# LSTM plans with dropout, reverse + set_io, input windows (so.FEATURE_SETS)
# ---------------------------------------------------------------------------------------------------------------------------
# the path families of LENGTHS_CASES, the N-split forward, the per-layer-stream form of forward_persist (where the
# dropout launches land on layer streams) and the stateless float32 path 4 (no lengths)
FEATURE_NAMES = LENGTHS_CASES + ("ns_fused_h1024_t33", "streams_b320_h256", "p4_f32_h128")
assert FEATURE_NAMES == tuple(so.FEATURE_CASES)


def _untouched_half_is_nan(c, y_all, what):
    if c.f["reverse_io"]:
        H = c.shape[3]
        assert bool(torch.isnan(y_all[:, :, :H]).all()), f"{what}: the half of the y buffer the plan was not given was written"


@pytest.mark.parametrize("features", list(so.FEATURE_SETS))
@pytest.mark.parametrize("name", FEATURE_NAMES)
def test_lstm_feature_forward_with_late_inputs(cuda, name, features):
    """test_lstm_forward_with_late_inputs on a plan with a feature set.  x (with windows: the source [S, Tsrc, I]), the
    weights, h0 and c0 arrive behind the Delay and are overwritten behind the call; the [B, T, 2H] y buffer is filled with
    NaN on the stream in front of the call.  What a wrong stream would do here: a drop_fwd launch off the stream of the
    GEMM behind it (xproj_chunk_gemm on the side stream, the layer streams of forward_persist) masks h before the
    recurrence wrote it; y_out (lstm_boundary.hip) off the caller's stream writes the half before the NaN fill or after the
    snapshot; kPrepCastX / kPrepBlockifyX / cast_strided_kernel off it read the poisoned source; the windows upload on
    another stream than the layout kernels leaves them with the previous call's arrays -- which hold the same values here,
    so THAT one is test_lstm_settings_change_between_unsynchronised_calls'.  The stream is synchronised once between the
    warm-up calls and the late one: a forward with lengths or windows waits for the plan's previous upload (BLOCKING)."""
    t0 = time.perf_counter()
    c = _lstm(name, features)
    what = f"{name} {features} forward"
    s = torch.cuda.Stream()
    t_host = _warm(s, lambda: c.forward(c.fwd_in))
    with torch.cuda.stream(s):
        _forget_workspace(c.plan)
    delay, a = so.late_all(s, c.fwd_in, so.delay_ms_for(t_host))
    with torch.cuda.stream(s):
        out = c.forward(a)
    running = delay.still_running()
    snaps = so.snapshot_then_poison(s, out, a)
    s.synchronize()
    _report(what, t_host, delay, t0, running)
    assert running
    so.assert_same_bits(snaps, c.want_fwd, what)
    _untouched_half_is_nan(c, snaps["y_all"], what)
    assert c.plan.status() == 0


def _backward_with_late_inputs(c, s, mode, t0, what, hook=lambda grads: None):
    """The body of test_lstm_backward_with_late_inputs for a plan with features: hook(grads) runs in front of every
    backward with the gradient tensors that backward writes.  -> (snapshots, Delay still running at return)"""
    def grads_for():
        grads = c.grads_for(mode)
        hook(grads)
        return grads
    with torch.cuda.stream(s):
        c.forward(c.fwd_in)
        c.backward(c.bwd_in, grads_for(), mode)
        s.synchronize()
        c.forward(c.fwd_in)
        grads = grads_for()
        s.synchronize()
        _, t_host = so.timed(lambda: c.backward(c.bwd_in, grads, mode))
        s.synchronize()
        _forget_workspace(c.plan)                    # what the backward finds there is its own forward's, or NaN
        a = _clone(c.fwd_in)
        c.forward(a)
        so.snapshot_then_poison(s, None, a)          # x, weights, h0, c0 of the forward are gone before the backward runs
    late_in = {"g": c.bwd_in, "grads": c.grads0} if mode == "accumulate" else {"g": c.bwd_in}
    delay, la = so.late_all(s, late_in, so.delay_ms_for(t_host))
    with torch.cuda.stream(s):
        grads = la["grads"] if mode == "accumulate" else c.grads_for(mode)
        hook(grads)
        out = c.backward(la["g"], grads, mode)
    running = delay.still_running()
    snaps = so.snapshot_then_poison(s, out, la["g"])
    s.synchronize()
    _report(what, t_host, delay, t0, running)
    return snaps, running


@pytest.mark.parametrize("mode", ["accumulate", "overwrite_tail"])
@pytest.mark.parametrize("features", list(so.FEATURE_SETS))
@pytest.mark.parametrize("name", FEATURE_NAMES)
def test_lstm_feature_backward_with_late_inputs(cuda, name, features, mode):
    """test_lstm_backward_with_late_inputs on a plan with a feature set: dy_last, the whole pitched [B, T, 2H] dy buffer
    (its other half NaN), dh_n, dc_n, under dx_add what dx holds and under accumulate what the gradients hold arrive
    behind the Delay; the forward before it ran on the same stream and had its inputs (the window source included)
    overwritten directly behind it.  What a wrong stream would do: a drop_bwd launch off the stream of its GEMM
    (dx_chunk_gemm on the side stream; the caller's stream in backward_persist) masks dx before the GEMM produced it, or
    the dh_n rows are added before the mask; dy_in off the caller's stream reads the poisoned dy buffer;
    dx_out (emit_dx, on the side stream in backward_il) adds to a dx whose late values have not arrived --
    or, with the closing join missing, is overtaken by the snapshot, which overwrite_tail takes of dx last."""
    t0 = time.perf_counter()
    c = _lstm(name, features)
    what = f"{name} {features} backward {mode}"
    snaps, running = _backward_with_late_inputs(c, torch.cuda.Stream(), mode, t0, what)
    assert running
    want = c.want_bwd["overwrite" if mode == "overwrite_tail" else mode]
    so.assert_same_bits(snaps, {k: want[k] for k in snaps}, what)
    assert c.plan.status() == 0


@pytest.mark.parametrize("name", so.SETTINGS_CASES)
def test_lstm_settings_change_between_unsynchronised_calls(cuda, name):
    """forward A, backward A, then other lengths, windows (another Tsrc) and dropout triple, forward B, backward B on one
    state + dropout plan, without a host synchronisation and all behind one Delay: equal to the same sequence with a
    device synchronisation after every call.  Call N + 1 rewrites the pinned staging arrays of the lengths and of the
    windows while call N's copy out of them has not run: only the hipEventSynchronize of upload_lengths / upload_views
    stands between A's kernels and B's values (a copy on another stream than the kernels that read the device arrays
    shows here too, A and B differing in every row).  Only forward A is required to return while the Delay runs: the
    later calls wait on the host for A's uploads, as the header says, so the wall time holds one Delay."""
    t0 = time.perf_counter()
    _LSTMS.clear()
    A, B = so.settings_a_and_b(name)
    settings = {"A": {**A, "reverse_io": False}, "B": {**B, "reverse_io": False}}
    c = _Lstm(name, features=settings["A"])
    ins = {k: {"fwd": {**c.fwd_in, "x": c._n(*c.x_shape(f))}, "bwd": c.bwd_in} for k, f in settings.items()}

    def sequence(stream, a, sync, probe=lambda: None):
        def after():
            if sync:
                torch.cuda.synchronize()
        out = {}
        with torch.cuda.stream(stream):
            for step, f in settings.items():
                c.apply(f)
                o = c.forward(a[step]["fwd"])
                if step == "A":
                    probe()
                after()
                out[step] = so.snapshot_then_poison(stream, o, a[step]["fwd"])
                after()
                b = c.backward(a[step]["bwd"], c.grads_for("overwrite"))
                after()
                out[step].update(so.snapshot_then_poison(stream, b, a[step]["bwd"]))
                after()
        return out
    d = torch.cuda.default_stream()
    want = _synced(lambda: sequence(d, _clone(ins), sync=True))
    so.assert_same_bits(_synced(lambda: sequence(d, _clone(ins), sync=True)), want, f"{name}: second synchronised run")
    for (k, a_), (_, b_) in zip(so._named(want["A"]), so._named(want["B"])):
        assert not so.same_bits(a_, b_), f"{name}: {k} of step B has the bits of step A: the settings cannot be told apart"
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        a = _clone(ins)
    sequence(s, a, sync=False)
    with torch.cuda.stream(s):
        a = _clone(ins)
    s.synchronize()
    _, t_host = so.timed(lambda: sequence(s, a, sync=False))
    s.synchronize()
    delay, la = so.late_all(s, ins, so.delay_ms_for(t_host))
    running = []
    out = sequence(s, la, sync=False, probe=lambda: running.append(delay.still_running()))
    s.synchronize()
    _report(f"{name} settings A then B", t_host, delay, t0, running[0])
    assert running == [True]
    so.assert_same_bits(out, want, f"{name} settings A then B")
    assert c.plan.status() == 0


CALLBACK_CASES = [(name, None) for name in LSTM_CASES] + [("p2_nopersist_bwd", "all"), ("streams_b320_h256", "all")]


@pytest.mark.parametrize("mode", ["overwrite", "accumulate"])
@pytest.mark.parametrize("name,features", CALLBACK_CASES, ids=[n if f is None else f"{n}-{f}" for n, f in CALLBACK_CASES])
def test_lstm_grad_ready_callback_marks_complete_gradients(cuda, name, features, mode):
    """The point csn_lstm_plan_set_grad_callback marks, used as the header describes it: inside fn(user, layer) an event is
    recorded on the current stream, a reader stream of the test's waits for it and clones layer's dw_ih, dw_hh, db_ih and
    db_hh -- nothing else, and nothing that calls back into the plan.  The incoming gradients (accumulate: and what the
    gradient tensors hold; overwrite: they hold NaN) arrive behind the Delay.  Every clone must have the bits of the
    synchronised backward's gradient.  A callback fired before a layer's weight-gradient GEMM, bias reduction or
    accumulating add is enqueued -- or fired on the caller's thread while that work sits on the side stream of
    backward_il without a join in front of the callback -- gives a clone of NaN, of the previous values or of a
    half-written tensor."""
    t0 = time.perf_counter()
    c = _lstm(name, features)
    L = c.shape[4]
    what = f"{name} {features or 'plain'} callback {mode}"
    s, reader = torch.cuda.Stream(), torch.cuda.Stream()
    seen = {}

    def hook(grads):
        seen.update(grads=grads, order=[], clones={})

    def ready(layer):
        ev = torch.cuda.Event()
        ev.record()                                   # the current stream: the one the backward was given
        reader.wait_event(ev)
        with torch.cuda.stream(reader):
            seen["clones"][layer] = {k: seen["grads"][k][layer].clone() for k in GROUPS}
        seen["order"].append(layer)
    c.plan.set_grad_callback(ready)
    try:
        _, running = _backward_with_late_inputs(c, s, mode, t0, what, hook)
        reader.synchronize()
    finally:
        c.plan.set_grad_callback(None)
    assert seen["order"] == list(range(L - 1, -1, -1)), seen["order"]
    assert running
    want = c.want_bwd[mode]
    for layer in range(L):
        so.assert_same_bits(seen["clones"][layer], {k: want[k][layer] for k in GROUPS}, f"{what}: layer {layer} at its callback")
    assert c.plan.status() == 0


def test_workspace_init_and_status_word_in_stream_order(cuda):
    """csn_lstm_workspace_init, csn_lstm_status_raise and csn_lstm_status_clear are memsets on `stream`.  Behind a Delay:
    the workspace is filled with 0xff, initialised, and the status raised -- an init or a raise that ran on another
    stream ran BEFORE the fill and leaves another status word than TIMEOUT.  Then raise, clear, forward, backward: a
    clear that overtook the raise leaves the word raised, and the results equal the synchronised run only if the zeros
    of the init are still there (a weight-stationary stateless plan never rewrites them)."""
    t0 = time.perf_counter()
    B, T, I, H, L = st.CASES["t4_l3"][0]
    plan = cabi.LstmPlan(B, T, I, H, L, torch.bfloat16, DEV, training=True)
    assert (plan.path(),) + plan.kernel_names() == st.P3
    g = torch.Generator(device="cpu").manual_seed(6)
    x = torch.randn(B, T, I, generator=g).to(DEV)
    ws = [[(0.2 * torch.randn(4 * H, I if (l == 0 and k == 0) else H, generator=g)).to(DEV) if k < 2
           else (0.2 * torch.randn(4 * H, generator=g)).to(DEV) for l in range(L)] for k in range(4)]
    dy = torch.randn(B, H, generator=g).to(DEV)

    def step():
        y_last, y_all = plan.forward(x, *ws, want_all=True)
        grads = [[torch.full_like(w, NAN) for w in grp] for grp in ws]
        dx = torch.full((B, T, I), NAN, device=DEV)
        plan.backward(dy, None, grads, dx=dx)
        return {"y_last": y_last, "y_all": y_all, "dx": dx, "grads": grads}
    want = _synced(step)
    so.assert_same_bits(_synced(step), want, "second synchronised run")
    s = torch.cuda.Stream()
    lib = cabi.load()
    with torch.cuda.stream(s):
        _, t_host = so.timed(step)
        s.synchronize()
        delay = so.Delay(s, so.delay_ms_for(t_host))
        plan.workspace.fill_(0xff)
        cabi._check(lib.csn_lstm_workspace_init(plan._plan, plan._ws_ptr, cabi._stream()))
        plan.inject_timeout()
        running = delay.still_running()
        s.synchronize()
        _report("workspace_init + status_raise", t_host, delay, t0, running)
        assert running
        assert plan.status() == cabi.STATUS_TIMEOUT
        delay = so.Delay(s, so.delay_ms_for(t_host))
        plan.inject_timeout()
        plan.clear_status()
        out = step()
        running = delay.still_running()
    snaps = so.snapshot_then_poison(s, out, [])
    s.synchronize()
    _report("status_raise + status_clear + forward + backward", t_host, delay, t0, running)
    assert running
    assert plan.status() == 0
    so.assert_same_bits(snaps, want, "after workspace_init in stream order")


# ---------------------------------------------------------------------------------------------------------------------------
# through the Python layer
# ---------------------------------------------------------------------------------------------------------------------------
TRAINER_SHAPES = {"f32_b8_t33_c12_h64_l3": ((8, 33, 12, 64, 3), torch.float32),       # test_trainer_fused_optimizer_matches_the_torch_one
                  "bf16_b8_t40_c16_h128_l2": ((8, 40, 16, 128, 2), torch.bfloat16)}


@pytest.mark.parametrize("optimizer,fused", [("adamw", True), ("rmsprop", False)], ids=["fused_adamw", "rmsprop"])
@pytest.mark.parametrize("shape", list(TRAINER_SHAPES))
def test_trainer_steps_on_a_side_stream_with_a_late_batch(cuda, shape, optimizer, fused):
    """DistillTrainer.train_step three times inside `with torch.cuda.stream(s)`, the batch produced late on s: parameters
    and losses bit-equal to three steps on the default stream with a device synchronisation after each."""
    t0 = time.perf_counter()
    (B, T, C, H, L), dtype = TRAINER_SHAPES[shape]
    rng = np.random.default_rng(B + T)
    batch = {"x": torch.from_numpy(rng.standard_normal((B, C, T)).astype(np.float32)).to(cuda),
             "tgt": torch.from_numpy(rng.standard_normal((B, 24)).astype(np.float32)).to(cuda)}

    def trainer():
        torch.manual_seed(3)
        m = Model(input_size=C, lstm_size=H, lstm_layers=L, output_size=24, include_top=False, compute_dtype=dtype).to(cuda)
        tr = DistillTrainer(m, None, loss="cosine", lr=1e-3, optimizer=optimizer, preprocess=False, fused_optimizer=fused)
        assert tr.grads.flat_params is not None
        torch.cuda.synchronize()
        return tr

    def steps(tr, b, sync):
        losses = []
        for _ in range(3):
            losses.append(tr.train_step(b["x"], b["tgt"]))
            if sync:
                torch.cuda.synchronize()
        return {"losses": losses, "params": tr.grads.flat_params}
    want = _clone(steps(trainer(), batch, sync=True))
    so.assert_same_bits(steps(trainer(), batch, sync=True), want, "second synchronised run")
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        tr = trainer()
        steps(tr, batch, sync=False)          # warm-up: lazy allocations of this process, on a trainer of its own
        s.synchronize()
        _, t_host = so.timed(lambda: steps(tr, batch, sync=False))
        s.synchronize()
        tr = trainer()
    delay, b = so.late_all(s, batch, so.delay_ms_for(t_host))
    with torch.cuda.stream(s):
        out = steps(tr, b, sync=False)
        running = delay.still_running()
    snaps = so.snapshot_then_poison(s, out, b)
    s.synchronize()
    _report(f"trainer {shape} {optimizer}", t_host, delay, t0, running)
    assert running
    so.assert_same_bits(snaps, want, f"trainer {shape} {optimizer}")
    tr.check_device_status()


BILSTM_SHAPES = ("v1_h96", "ks_h256", "f32_h128")          # of test_gpu_bilstm.MODEL_SHAPES


@pytest.mark.parametrize("name", BILSTM_SHAPES)
def test_bilstm_module_on_a_side_stream_with_late_inputs(cuda, name):
    """BiLSTM forward and torch.autograd.backward with lengths inside `with torch.cuda.stream(s)`: x, h0, c0 and the
    output gradients arrive late; out, h_n, c_n are cloned and x, h0, c0 overwritten behind the forward, the parameter and
    input gradients cloned and the output gradients overwritten behind the backward.  The two plans of a layer write the
    halves of one [B, T, 2H] buffer and read the halves of its gradient, and the reverse one adds into the forward one's
    dx: an io kernel or the adding dx store on a wrong stream, or a direction that starts before the layer below has
    finished both halves, changes the bits.  The forward is required to return while the Delay runs; the backward of a
    plan with lengths waits on the host for its own forward's upload (BLOCKING), so the wall time holds one Delay."""
    t0 = time.perf_counter()
    (B, T, I, H, L), dtype = bl.MODEL_SHAPES[name]
    m, args = bl._model(name)
    lengths = bl._lengths(B, T, "random_with_zeros", (31, 32, 33))
    ins = dict(zip(("x", "h0", "c0", "dy", "dh", "dc"), args))
    params = dict(m.named_parameters())

    def run(a, stream, probe=lambda: None):
        with torch.cuda.stream(stream):
            x, h0, c0 = (a[k].detach().requires_grad_(True) for k in ("x", "h0", "c0"))
            for p in params.values():
                p.grad = None
            out, (h_n, c_n) = m(x, (h0, c0), lengths=lengths)
            probe()
            # (.data: the overwrite is not an in-place operation autograd should know of -- nothing may still read them)
            snaps = so.snapshot_then_poison(stream, {"out": out.detach(), "h_n": h_n.detach(), "c_n": c_n.detach()},
                                            [a[k].data for k in ("x", "h0", "c0")])
            torch.autograd.backward([out, h_n, c_n], [a["dy"], a["dh"], a["dc"]])
            grads = {"dx": x.grad, "dh0": h0.grad, "dc0": c0.grad, **{k: p.grad for k, p in params.items()}}
            snaps.update(so.snapshot_then_poison(stream, grads, [a[k] for k in ("dy", "dh", "dc")]))
        return snaps
    d = torch.cuda.default_stream()
    want = _synced(lambda: run(_clone(ins), d))
    so.assert_same_bits(_synced(lambda: run(_clone(ins), d)), want, f"{name}: second synchronised run")
    assert {pl.reverse for pl in m.all_plans()} == {False, True}
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        run(_clone(ins), s)
        a = _clone(ins)
        s.synchronize()
        _, t_host = so.timed(lambda: run(a, s))
        s.synchronize()
        for pl in m.all_plans():
            _forget_workspace(pl)
    delay, la = so.late_all(s, ins, so.delay_ms_for(t_host))
    running = []
    snaps = run(la, s, probe=lambda: running.append(delay.still_running()))
    s.synchronize()
    _report(f"BiLSTM {name}", t_host, delay, t0, running[0])
    assert running == [True]
    so.assert_same_bits(snaps, want, f"BiLSTM {name}")
    for pl in m.all_plans():
        assert pl.status() == 0
