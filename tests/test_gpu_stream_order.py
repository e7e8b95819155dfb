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
plan's path and kernels checked as there.  Each test prints t_host, the Delay and its wall time."""
import os
import time

import numpy as np
import pytest
import torch

import stream_order as so
import test_gpu_lstm_state as st
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
    reference runs."""

    def __init__(self, name, lengths=False):
        shape, dtype, expect, env, state = _case(name)
        self.name, self.shape, self.dtype, self.state = name, shape, dtype, state
        B, T, I, H, L = shape
        old = {k: os.environ.get(k) for k in env}
        os.environ.update(env)          # the switches are read once, at plan creation
        try:
            self.plan = cabi.LstmPlan(B, T, I, H, L, dtype, DEV, training=True, state=state)
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
        g = torch.Generator(device="cpu").manual_seed(5)
        k = 1.0 / np.sqrt(H)

        def u(*s):
            return ((2 * torch.rand(*s, generator=g) - 1) * k).to(DEV)

        def n(*s, scale=1.0):
            return (scale * torch.randn(*s, generator=g)).to(DEV)
        self.fwd_in = {"x": n(B, T, I), "w_ih": [u(4 * H, I if l == 0 else H) for l in range(L)],
                       "w_hh": [u(4 * H, H) for _ in range(L)], "b_ih": [u(4 * H) for _ in range(L)],
                       "b_hh": [u(4 * H) for _ in range(L)], "h0": n(L, B, H, scale=0.5), "c0": n(L, B, H)}
        self.bwd_in = {"dy_last": n(B, H), "dy_all": n(B, T, H), "dh_n": n(L, B, H), "dc_n": n(L, B, H)}
        if not state:
            for k_ in ("h0", "c0"):
                self.fwd_in[k_] = None
            for k_ in ("dh_n", "dc_n"):
                self.bwd_in[k_] = None
        self.grads0 = {k_: [n(*w.shape, scale=0.25) for w in self.fwd_in[k_]] for k_ in GROUPS}     # accumulate mode: what is there before
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
        assert self.plan.status() == 0

    def forward(self, a):
        if not self.state:
            y_last, y_all = self.plan.forward(a["x"], a["w_ih"], a["w_hh"], a["b_ih"], a["b_hh"], want_all=True)
            return {"y_last": y_last, "y_all": y_all}
        y_last, y_all, h_n, c_n = self.plan.forward(a["x"], a["w_ih"], a["w_hh"], a["b_ih"], a["b_hh"], want_all=True,
                                                    h0=a["h0"], c0=a["c0"], want_state=True)
        return {"y_last": y_last, "y_all": y_all, "h_n": h_n, "c_n": c_n}

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
        dx = torch.full((B, T, I), NAN, device=DEV)
        dh0 = None if tail or not self.state else torch.full((L, B, H), NAN, device=DEV)
        dc0 = None if tail or not self.state else torch.full((L, B, H), NAN, device=DEV)
        self.plan.set_grad_mode(mode == "accumulate")
        try:
            self.plan.backward(g["dy_last"], g["dy_all"], [grads[k] for k in GROUPS], dx=dx, dh_n=g["dh_n"], dc_n=g["dc_n"],
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


def _lstm(name):
    if name not in _LSTMS:
        _LSTMS.clear()                  # one case's plan and references at a time
        _LSTMS[name] = _Lstm(name)
    return _LSTMS[name]


def _warm(s, fn):
    """fn() once on `s` to warm it up, once more for its host time."""
    with torch.cuda.stream(s):
        fn()
        s.synchronize()
        _, t_host = so.timed(fn)
        s.synchronize()
    return t_host


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
