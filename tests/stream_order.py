"""Helpers of the stream-order tests (tests/test_gpu_stream_order.py, tests/test_stream_order_cpu.py); not a test module.

The contract under test (include/csn_hip.h, "Stream contract"): everything an entry point enqueues is ordered behind what
the caller enqueued earlier on `stream` and before what the caller enqueues later on it, whatever other streams the
library uses inside.  A test can only see a violation if, at the moment of the call, the inputs are NOT yet there and,
right behind the call, they are gone again:

    Delay                  keeps `stream` busy with ordinary torch work while the host runs ahead
    late                   an argument that holds poison until a copy enqueued on `stream` behind the Delay
    snapshot_then_poison   clones the outputs on `stream` directly behind the call, then overwrites the inputs

A launch or memset that the library left on another stream reads poison (it runs while the Delay still holds `stream`) or
is read too early by the snapshot; a missing join lets the poison that follows the call overtake a reader.

What a pass does NOT prove.  A process has a few hardware queues (4 by default) and HIP spreads its streams over them: a
plan's nine streams, the stream under test and this module's fill stream share them.  Work that the library left on a
wrong stream can land in the hardware queue the Delay occupies and is then serialised behind the Delay by accident, and a
side stream whose join is missing can simply finish first.  The tests are therefore one-sided evidence: a failure shows
a broken order, a pass shows that none was seen in this run's assignment of streams to queues.  (The snapshot order of
_Lstm.backward's "overwrite_tail" mode exists because the closing join of the per-diagonal backward, when removed, was
only seen by a reader directly behind the call's last launch.)

CASE_TABLE names every entry point of include/csn_hip.h that takes a csnStream_t (tests/test_stream_order_cpu.py holds
the two against each other) with its stream-order cases: single calls here, or the tests that run it through a plan.
PLAN_SETTERS does the same for the csn_lstm_plan_set_* functions, which take no stream themselves: what they set --
gradient mode and callback, lengths, input windows, the y_all / dy_all pitch and the adding dx, dropout -- adds launches,
copies and host staging to the forward and backward that follow, and the table names the tests that run those in stream
order (FEATURE_SETS and the draws below them are their host side)."""
import math
import time

import numpy as np
import torch

NAN = float("nan")
INT_POISON = 0          # integers: a value that is in range wherever it might be used as an index or a count


# ---------------------------------------------------------------------------------------------------------------------------
# Delay
# ---------------------------------------------------------------------------------------------------------------------------
class Delay:
    """`ms` milliseconds (at least) of ordinary work on `stream`: a chain of float32 matmuls on buffers of its own.  No
    spin kernel, no sleep: every launch is a finite GEMM.  The time of one link is measured once per process and device
    with events (calibrate); the chain is made SAFETY times longer than that asks for, and the tests assert
    still_running() where it matters, so a chain that came out too short fails the test instead of weakening it."""
    N = 2048                 # one link: a 2048^3 float32 matmul
    SAFETY = 2.0
    MAX_LINKS = 20000
    _ms_per_link = {}

    @staticmethod
    def _chain(n_links, stream):
        with torch.cuda.stream(stream):
            a = torch.full((Delay.N, Delay.N), 1.0 / Delay.N, dtype=torch.float32, device=stream.device)
            b, c = a.clone(), torch.empty_like(a)       # (a b has every element 1 / N again: the values never grow)
            for _ in range(n_links):
                torch.mm(a, b, out=c)
                a, c = c, a
        return a

    @classmethod
    def calibrate(cls, device):
        """ms per link on `device`, measured once per process: warm links first, then a timed chain between two events on a
        stream of its own (only that stream is waited for)."""
        key = torch.device(device).index or 0
        if key not in cls._ms_per_link:
            s = torch.cuda.Stream(device=device)
            cls._chain(30, s)
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(s)
            cls._chain(60, s)
            e1.record(s)
            e1.synchronize()
            cls._ms_per_link[key] = max(e0.elapsed_time(e1) / 60.0, 1e-3)
        return cls._ms_per_link[key]

    def __init__(self, stream, ms):
        self.ms = float(ms)
        self.links = min(self.MAX_LINKS, int(math.ceil(self.SAFETY * self.ms / self.calibrate(stream.device))) + 1)
        self._begin, self._end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        self._begin.record(stream)
        self._keep = self._chain(self.links, stream)
        self._end.record(stream)

    def still_running(self):
        return not self._end.query()

    def measured_ms(self):
        """Length of the chain on the device (call after the stream has been synchronised)."""
        return self._begin.elapsed_time(self._end)


def delay_ms_for(t_host_s):
    """The Delay a call of host time t_host needs: at least 3 t_host + 20 ms."""
    return 3e3 * t_host_s + 20.0


# ---------------------------------------------------------------------------------------------------------------------------
# late arguments, snapshots
# ---------------------------------------------------------------------------------------------------------------------------
def poison_value(t, poison=NAN):
    return poison if t.is_floating_point() else INT_POISON


_fill_streams = {}


def poisoned_like(real, poison=NAN):
    """A tensor of real's shape and dtype that holds poison (NaN; INT_POISON for integers), finished before this returns.
    On a GPU the fill runs on a stream of this module's own, and only that stream is waited for: the stream under test
    and the default stream are neither used nor synchronised.  Call it IN FRONT of a Delay, never behind one: streams share
    a few hardware queues, and a fill that lands in the queue the Delay occupies would make this wait for the Delay."""
    if not real.is_cuda:
        return torch.full_like(real, poison_value(real, poison))
    key = real.device.index or 0
    if key not in _fill_streams:
        _fill_streams[key] = torch.cuda.Stream(device=real.device)
    fs = _fill_streams[key]
    with torch.cuda.stream(fs):
        arg = torch.full_like(real, poison_value(real, poison))
    fs.synchronize()
    return arg


def copy_late(stream, arg, real):
    """arg.copy_(real) enqueued on `stream` (CPU tensors: done at once): the only ordering between real's values and
    whatever reads arg."""
    if arg.is_cuda:
        arg.record_stream(stream)
        with torch.cuda.stream(stream):
            arg.copy_(real, non_blocking=True)
    else:
        arg.copy_(real)
    return arg


def late(stream, real, poison=NAN, before_copy=None):
    """The argument `real` as the stream-order tests pass it: allocated full of poison, the real values arriving through a
    copy enqueued on `stream` -- behind the Delay the caller has put there.  before_copy(arg), if given, sees the
    poisoned argument first (tests/test_stream_order_cpu.py).  Host-side arguments (lengths, sos, segment ends) are not
    made late: the library reads them during the call."""
    arg = poisoned_like(real, poison)
    if before_copy is not None:
        before_copy(arg)
    return copy_late(stream, arg, real)


def _map(tree, fn):
    """fn over the tensors of a dict / list / tuple tree; None stays None."""
    if tree is None:
        return None
    if isinstance(tree, dict):
        return {k: _map(v, fn) for k, v in tree.items()}
    if isinstance(tree, (list, tuple)):
        return [_map(v, fn) for v in tree]
    return fn(tree)


def _leaves(tree):
    out = []
    _map(tree, out.append)
    return out


def late_all(stream, reals, ms, poison=NAN):
    """Every tensor of the tree `reals` late behind ONE Delay of `ms`: the poisoned arguments first (all finished), then
    the Delay on `stream`, then the copies.  -> (delay, arguments in the shape of `reals`)."""
    args = _map(reals, lambda t: poisoned_like(t, poison))
    delay = Delay(stream, ms)
    for a, r in zip(_leaves(args), _leaves(reals)):
        copy_late(stream, a, r)
    return delay, args


def snapshot_then_poison(stream, outputs, overwritable_inputs, poison=NAN):
    """Directly behind a call, on the same stream, without a host synchronisation: clone() of every output (tree of
    tensors -> tree of clones), then poison into every input the header says may be overwritten at that point.  An
    output that is also an input (updated in place) is cloned first and poisoned after."""
    def run():
        snaps = _map(outputs, lambda t: t.clone())
        for t in _leaves(overwritable_inputs):
            t.fill_(poison_value(t, poison))
        return snaps
    if stream is None:
        return run()
    with torch.cuda.stream(stream):
        return run()


def same_bits(a, b):
    """Bit-for-bit equality (NaN payloads included)."""
    if a.shape != b.shape or a.dtype != b.dtype:
        return False
    return torch.equal(a.contiguous().reshape(-1).view(torch.uint8), b.contiguous().reshape(-1).view(torch.uint8))


def assert_same_bits(got, want, what):
    """Every tensor of the tree `got` has the bits of the tensor at the same place in `want`; the two trees hold tensors at
    the same places (an output that came back None where the reference has one is a failure, not a shorter comparison)."""
    names, want_names = [k for k, _ in _named(got)], [k for k, _ in _named(want)]
    assert names == want_names and names, f"{what}: outputs {names} against the synchronised run's {want_names}"
    for (k, g), w in zip(_named(got), _leaves(want)):
        if not same_bits(g, w):
            bad = g.double().sub(w.double()).abs()
            raise AssertionError(f"{what}: {k} differs from the synchronised run "
                                 f"(non-finite: {int((~torch.isfinite(g.double())).sum())} of {g.numel()}, "
                                 f"largest finite difference {float(torch.nan_to_num(bad, nan=0.0, posinf=0.0).max()):.3e})")


def _named(tree, prefix=""):
    if tree is None:
        return []
    if isinstance(tree, dict):
        return [kv for k, v in tree.items() for kv in _named(v, f"{prefix}{k}")]
    if isinstance(tree, (list, tuple)):
        return [kv for i, v in enumerate(tree) for kv in _named(v, f"{prefix}[{i}]")]
    return [(prefix, tree)]


# ---------------------------------------------------------------------------------------------------------------------------
# stateless entry points: one small shape each (the smallest that takes the route named in the label)
# ---------------------------------------------------------------------------------------------------------------------------
class Stateless:
    """One stream-order case of a stateless entry point.  build(device) -> (inputs, call): `inputs` a dict of device
    tensors with the real values (ready), call(args) -> dict of outputs, enqueued on the CURRENT stream; an argument the
    entry point updates in place is returned among the outputs.  Every input may be overwritten behind the call."""

    def __init__(self, entry, label, build):
        self.entry, self.label, self.build = entry, label, build

    @property
    def id(self):
        return f"{self.entry[4:]}-{self.label}"


class InTest:
    """An entry point whose cases are the named tests of tests/test_gpu_stream_order.py (plans, not single calls)."""

    def __init__(self, *tests):
        self.tests = tests


def _rng(seed):
    return np.random.default_rng(seed)


def _dev(a, device, dtype=None):
    t = torch.from_numpy(np.ascontiguousarray(a)).to(device)
    return t.to(dtype) if dtype is not None else t


def _sos(nsec):
    from oracle import eeg_filter
    return eeg_filter.design_bandpass_sos(1000, nsec)


def _znorm(shape, nsec, scan):
    def build(device):
        from cerebralsignalnetworks_amd import cabi
        B, C, T = shape
        assert (T <= 512 and T % 4 == 0 and C % 4 == 0 and nsec <= 5) == scan      # the dispatch rule of the entry point
        x = _dev(_rng(11).standard_normal(shape).astype(np.float32), device)
        sos = _sos(nsec)
        return {"x": x}, lambda a: {"y": cabi.eeg_bandpass_znorm(a["x"], sos, ddof=1)}
    return build


def _bandpass_stream(shape, nsec, scan):
    def build(device):
        from cerebralsignalnetworks_amd import cabi
        B, C, T = shape
        r = _rng(12)
        ins = {"x": _dev(r.standard_normal(shape).astype(np.float32), device),
               "state_in": _dev(0.1 * r.standard_normal((B, C, nsec, 2)), device),
               "mean": _dev(r.standard_normal(C).astype(np.float32), device),
               "inv_std": _dev((0.5 + r.random(C)).astype(np.float32), device)}
        assert cabi.eeg_bandpass_stream_path(ins["x"], nsec) == int(scan)
        sos = _sos(nsec)

        def call(a):
            y, state_out = cabi.eeg_bandpass_stream(a["x"], sos, state_in=a["state_in"], mean=a["mean"], inv_std=a["inv_std"])
            return {"y": y, "state_out": state_out}
        return ins, call
    return build


def _filtfilt(device):
    from cerebralsignalnetworks_amd import cabi
    x = _dev(_rng(13).standard_normal((2, 64, 5)).astype(np.float32), device)
    sos = _sos(4)
    return {"x": x}, lambda a: {"y": cabi.eeg_filtfilt(a["x"], sos)}


def gemm_nt_route(M, N, K, dtype, aligned16=True, generic=False, no_dma=False, no_256=False, no_192=False, no_w4=False):
    """Mirror of nt_route() in csrc/gemm_nt.hip: the kernel family a shape takes.  The keywords are the operands'
    16-byte alignment and the switches CSN_GEMM_GENERIC, CSN_GEMM_NO_DMA, CSN_GEMM_NO_256, CSN_GEMM_NO_192 and
    CSN_NT_NO_W4 (which picks between the two forms of the 192 tile: both are "wide192" here).  The cases below assert
    the route their label names, so a change of the thresholds there shows up here instead of quietly moving a case;
    tests/test_stream_order_cpu.py holds this mirror against the library's own answer (cabi.gemm_nt_route)."""
    if not (dtype == torch.bfloat16 and K % 8 == 0 and N % 4 == 0 and aligned16 and not generic):
        return "generic"
    if K % 64 == 0 and K >= 128 and M >= 256 and not (no_dma or no_256 or no_192):
        def fills(bn):          # whole tiles for every CU: at least 256 tiles, at most 10 % of the last round empty
            t = (N // bn) * -(-M // 256)
            return N % bn == 0 and t >= 256 and t * 10 >= -(-t // 256) * 256 * 9
        if fills(256):
            return "wide256"
        if fills(192):
            return "wide192"
    if K % 64 == 0 and K >= 256 and M >= 256 and N >= 1024 and not (no_dma or no_256):
        return "tile256x128"
    return "dma" if K % 64 == 0 and not no_dma else "bf16"


def gemm_tn_route(M, N, K, no_256=False, no_dma=False):
    """Mirror of tn_route() in csrc/gemm_tn.hip for aligned bf16 operands with M and N multiples of 8; the keywords are
    the switches CSN_GEMM_NO_256 and CSN_GEMM_NO_DMA."""
    assert M % 8 == 0 and N % 8 == 0
    return "tile256" if M >= 256 and N >= 128 and K % 64 == 0 and K >= 8192 and not (no_256 or no_dma) else "tile128"


def _gemm_nt(route, M, N, K, dtype, out_dtype, accumulate=False):
    def build(device):
        from cerebralsignalnetworks_amd import cabi
        assert gemm_nt_route(M, N, K, dtype) == route, (gemm_nt_route(M, N, K, dtype), route)
        r = _rng(M + N + K)
        ins = {"a": _dev(r.standard_normal((M, K)).astype(np.float32), device, dtype),
               "bt": _dev(r.standard_normal((N, K)).astype(np.float32), device, dtype),
               "bias": _dev(r.standard_normal(N).astype(np.float32), device)}
        if accumulate:
            ins["c"] = _dev(r.standard_normal((M, N)).astype(np.float32), device)
            return ins, lambda a: {"c": cabi.gemm_nt(a["a"], a["bt"], a["bias"], out=a["c"], accumulate=True)}
        return ins, lambda a: {"c": cabi.gemm_nt(a["a"], a["bt"], a["bias"], out_dtype=out_dtype)}
    return build


def _gemm_tn(route, M, N, K):
    def build(device):
        from cerebralsignalnetworks_amd import cabi
        assert gemm_tn_route(M, N, K) == route
        r = _rng(M + N + K)
        ins = {"a": _dev(r.standard_normal((K, M)).astype(np.float32), device, torch.bfloat16),
               "b": _dev(r.standard_normal((K, N)).astype(np.float32), device, torch.bfloat16)}
        return ins, lambda a: {"c": cabi.gemm_tn(a["a"], a["b"])}
    return build


def _cell_inputs(B, H, dtype, device):
    r = _rng(B + H)
    k = 1.0 / math.sqrt(H)
    return {"h_prev": _dev(r.uniform(-1, 1, (B, H)).astype(np.float32), device, dtype),
            "w_hh": _dev(r.uniform(-k, k, (4 * H, H)).astype(np.float32), device, dtype),
            "xproj": _dev(r.standard_normal((B, 4 * H)).astype(np.float32), device),
            "c_prev": _dev(r.standard_normal((B, H)).astype(np.float32), device)}


def _cell_forward(B, H, dtype):
    def build(device):
        from cerebralsignalnetworks_amd import cabi
        ins = _cell_inputs(B, H, dtype, device)

        def call(a):
            h, c, gates = cabi.lstm_cell_forward(a["h_prev"], a["w_hh"], a["xproj"], a["c_prev"])
            return {"h": h, "c": c, "gates": gates}
        return ins, call
    return build


def _cell_backward(B, H, dtype):
    def build(device):
        from cerebralsignalnetworks_amd import cabi
        f = _cell_inputs(B, H, dtype, device)
        _, c, gates = cabi.lstm_cell_forward(f["h_prev"], f["w_hh"], f["xproj"], f["c_prev"])
        torch.cuda.synchronize()
        r = _rng(B * H)
        ins = {"dgates_next": _dev(0.1 * r.standard_normal((B, 4 * H)).astype(np.float32), device, dtype),
               "w_hh_t": f["w_hh"].t().contiguous(),
               "dy": _dev(r.standard_normal((B, H)).astype(np.float32), device),
               "gates": gates, "c": c, "c_prev": f["c_prev"],
               "dc_carry": _dev(r.standard_normal((B, H)).astype(np.float32), device)}

        def call(a):
            dg = cabi.lstm_cell_backward(a["dgates_next"], a["w_hh_t"], a["dy"], a["gates"], a["c"], a["c_prev"], a["dc_carry"])
            return {"dgates": dg, "dc_carry": a["dc_carry"]}
        return ins, call
    return build


def _cosine(device):
    from cerebralsignalnetworks_amd import cabi
    r = _rng(14)
    ins = {"student": _dev(r.standard_normal((6, 33)).astype(np.float32), device),
           "teacher": _dev(r.standard_normal((6, 33)).astype(np.float32), device)}

    def call(a):
        loss, ds = cabi.cosine_loss(a["student"], a["teacher"], grad_scale=0.5)
        return {"loss": loss, "dstudent": ds}
    return ins, call


def _barlow(device):
    from cerebralsignalnetworks_amd import cabi
    c = _dev(_rng(15).standard_normal((65, 65)).astype(np.float32), device)
    return {"c": c}, lambda a: {"out": cabi.barlow_offdiag_sqsum(a["c"])}


FLAT_N, FLAT_ENDS, FLAT_FLAGS = 5000, (7, 2050, 5000), (3, 1, 2)      # segment ends off every 2048-element chunk edge


def _flat_buffers(device, names, seed):
    r = _rng(seed)
    return {k: _dev((np.abs(r.standard_normal(FLAT_N)) if k in ("square_avg", "exp_avg_sq") else r.standard_normal(FLAT_N))
                    .astype(np.float32), device) for k in names}


def _rmsprop(device):
    from cerebralsignalnetworks_amd import cabi
    ins = _flat_buffers(device, ("params", "grads", "square_avg"), 16)

    def call(a):
        cabi.rmsprop_step(a["params"], a["grads"], a["square_avg"], 1e-2)
        return {"params": a["params"], "square_avg": a["square_avg"]}
    return ins, call


def _table(device):
    """A prepared segment table (ready) of the flat-buffer cases."""
    from cerebralsignalnetworks_amd import cabi
    t = cabi.SegmentTable(FLAT_ENDS, FLAT_FLAGS, device)
    torch.cuda.synchronize()
    return t


def _segments_prepare(device):
    """The table's bytes are the output; its previous contents (0xff in every byte, late) the only device input."""
    import ctypes
    from cerebralsignalnetworks_amd import cabi
    t = _table(device)
    ends, flags = (ctypes.c_int64 * t.nseg)(*t.seg_end), (ctypes.c_int32 * t.nseg)(*t.flags)
    ins = {"table": torch.full_like(t.buf.view(torch.uint8), 0xff).view(torch.float64)}

    def call(a):
        cabi._check(cabi.load().csn_flat_segments_prepare(ends, flags, t.nseg, t.n, cabi._ptr(a["table"]), cabi._stream()))
        return {"table": a["table"]}
    return ins, call


def _segment_norms(device):
    from cerebralsignalnetworks_amd import cabi
    t = _table(device)
    ins = _flat_buffers(device, ("a", "b"), 17)
    return ins, lambda a: {"norms": cabi.flat_segment_norms(t, a["a"], a["b"], weight_decay=0.1)}


def _flat_clip(device):
    from cerebralsignalnetworks_amd import cabi
    t = _table(device)
    ins = _flat_buffers(device, ("grads",), 18)
    return ins, lambda a: {"norms": cabi.flat_clip(t, a["grads"], 3.0), "grads": a["grads"]}


def _adam(device):
    from cerebralsignalnetworks_amd import cabi
    t = _table(device)
    ins = _flat_buffers(device, ("params", "grads", "exp_avg", "exp_avg_sq"), 19)

    def call(a):
        norms = torch.empty(t.nseg, dtype=torch.float32, device=device)
        cabi.adam_step(t, a["params"], a["grads"], a["exp_avg"], a["exp_avg_sq"], 3, 1e-3, 0.9, 0.999, 1e-8, 0.01, True,
                       clip=3.0, norms_out=norms)
        return {"params": a["params"], "exp_avg": a["exp_avg"], "exp_avg_sq": a["exp_avg_sq"], "norms": norms}
    return ins, call


def _lars(device):
    from cerebralsignalnetworks_amd import cabi
    t = _table(device)
    ins = _flat_buffers(device, ("params", "grads", "mu"), 20)

    def call(a):
        cabi.lars_step(t, a["params"], a["grads"], a["mu"], 0.2, 1e-6, 0.9, 0.001)
        return {"params": a["params"], "mu": a["mu"]}
    return ins, call


def _topk_inputs(Ng, Nq, D, device, seed):
    r = _rng(seed)
    return {"gallery": _dev(r.standard_normal((Ng, D)).astype(np.float32), device),
            "query": _dev(r.standard_normal((Nq, D)).astype(np.float32), device)}


def _l2_topk(device):
    from cerebralsignalnetworks_amd import cabi

    def call(a):
        dist, idx = cabi.l2_topk(a["gallery"], a["query"], 64)
        return {"dist": dist, "idx": idx}
    return _topk_inputs(100, 7, 33, device, 21), call


def _l2_topk_tiled(splits):
    def build(device):
        from cerebralsignalnetworks_amd import cabi
        Ng, Nq, D, k = 500, 7, 33, 70          # 8 gallery tiles of 64 rows: 7 ranges exist; k beyond csn_l2_topk's 64
        lib = cabi.load()

        def call(a):
            # the scratch is poisoned as well (on the stream of the call, in front of it)
            scratch = torch.full((lib.csn_l2_topk_tiled_scratch_bytes(Ng, Nq, k),), 0xff, dtype=torch.uint8, device=device)
            idx = torch.empty((Nq, k), dtype=torch.int64, device=device)
            dist = torch.empty((Nq, k), dtype=torch.float32, device=device)
            d64 = torch.empty((Nq, k), dtype=torch.float64, device=device)
            cabi._check(lib.csn_l2_topk_tiled(cabi._ptr(a["gallery"]), cabi._ptr(a["query"]), Ng, Nq, D, k, splits,
                                              cabi._ptr(idx), cabi._ptr(dist), cabi._ptr(d64), cabi._ptr(scratch), cabi._stream()))
            return {"dist": dist, "idx": idx, "dist64": d64}
        return _topk_inputs(Ng, Nq, D, device, 22), call
    return build


BF16, F32 = torch.bfloat16, torch.float32
_LSTM_TESTS = ("test_lstm_forward_with_late_inputs", "test_lstm_backward_with_late_inputs", "test_lstm_two_steps_back_to_back",
               "test_lstm_lengths_with_late_inputs", "test_lstm_feature_forward_with_late_inputs",
               "test_lstm_feature_backward_with_late_inputs", "test_lstm_settings_change_between_unsynchronised_calls",
               "test_bilstm_module_on_a_side_stream_with_late_inputs", "test_lstm_grad_ready_callback_marks_complete_gradients")
_LSTM_FORWARD_TESTS = tuple(t for t in _LSTM_TESTS if t != "test_lstm_grad_ready_callback_marks_complete_gradients")

# every csn_lstm_plan_set_* function of include/csn_hip.h (host only: none takes a stream; what it sets is read by the
# following csn_lstm_forward / csn_lstm_backward) -> the tests of tests/test_gpu_stream_order.py that run a call under that
# setting in stream order (tests/test_stream_order_cpu.py holds this table against the header too)
PLAN_SETTERS = {
    "csn_lstm_plan_set_grad_callback": ("test_lstm_grad_ready_callback_marks_complete_gradients",),
    "csn_lstm_plan_set_grad_mode": ("test_lstm_backward_with_late_inputs", "test_lstm_lengths_with_late_inputs",
                                    "test_lstm_feature_backward_with_late_inputs",
                                    "test_lstm_grad_ready_callback_marks_complete_gradients"),
    "csn_lstm_plan_set_lengths": ("test_lstm_lengths_with_late_inputs", "test_lstm_feature_forward_with_late_inputs",
                                  "test_lstm_feature_backward_with_late_inputs",
                                  "test_lstm_settings_change_between_unsynchronised_calls",
                                  "test_bilstm_module_on_a_side_stream_with_late_inputs"),
    "csn_lstm_plan_set_views": ("test_lstm_feature_forward_with_late_inputs", "test_lstm_feature_backward_with_late_inputs",
                                "test_lstm_settings_change_between_unsynchronised_calls"),
    "csn_lstm_plan_set_io": ("test_lstm_feature_forward_with_late_inputs", "test_lstm_feature_backward_with_late_inputs",
                             "test_bilstm_module_on_a_side_stream_with_late_inputs"),
    "csn_lstm_plan_set_dropout": ("test_lstm_feature_forward_with_late_inputs", "test_lstm_feature_backward_with_late_inputs",
                                  "test_lstm_settings_change_between_unsynchronised_calls"),
}


# ---------------------------------------------------------------------------------------------------------------------------
# LSTM plans with features: the host-side draws (no GPU needed: tests/test_stream_order_cpu.py checks them)
# ---------------------------------------------------------------------------------------------------------------------------
# feature set -> what the plan carries.  "lengths" only ever on a CSN_LSTM_STATE plan (the stateless path 4 case runs
# its windows over T steps)
FEATURE_SETS = {"dropout": ("dropout",), "reverse_io": ("reverse_io",), "windows": ("windows", "lengths"),
                "all": ("dropout", "reverse_io", "windows", "lengths")}
# name -> ((B, T, I, H, L), CSN_LSTM_STATE plan?) of the cases the feature tests run (tests/test_gpu_stream_order.py holds
# each against the case of that name)
FEATURE_CASES = {
    "v1_h96": ((8, 40, 24, 96, 2), True),
    "p1_l5": ((8, 30, 16, 128, 5), True),
    "p2_nopersist_bwd": ((64, 40, 128, 768, 2), True),
    "ks_fused_h768_t32": ((256, 32, 128, 768, 2), True),
    "f32_h128": ((70, 37, 24, 128, 2), True),
    "ns_fused_h1024_t33": ((65, 33, 128, 1024, 2), True),
    "streams_b320_h256": ((320, 40, 32, 256, 2), True),
    "p4_f32_h128": ((70, 37, 24, 128, 2), False),
}
DROPOUT = (0.5, 1234, 1)            # (p, seed, subsequence) of every feature plan with dropout
SETTINGS_CASES = ("v1_h96", "ks_fused_h768_t32", "f32_h128")


def two_mixed_lengths(B, T):
    """The "two_mixed" pattern of tests/test_gpu_lstm_views.py: the first third of the rows T, the rest 2T/3."""
    return [T if b < max(1, B // 3) else (2 * T) // 3 for b in range(B)]


def random_windows(B, Tsrc, lengths, seed=0):
    """-> (S, src_row[B], t0[B]): the draw of tests/test_gpu_lstm_views.py::_windows("random", ...)."""
    rng = np.random.default_rng(500 + seed)
    S = max(1, B // 3)
    rows = rng.integers(0, S, B).tolist()
    return S, rows, rng.integers(0, Tsrc - np.asarray(lengths) + 1).tolist()


def feature_settings(name, feature_set):
    """The sticky host settings of the plan of (name, feature set): dict(dropout = (p, seed, subsequence) or None,
    reverse_io, lengths = [B] or None, views = (rows, starts, S, Tsrc) or None)."""
    (B, T, I, H, L), state = FEATURE_CASES[name]
    f = FEATURE_SETS[feature_set]
    out = {"dropout": DROPOUT if "dropout" in f else None, "reverse_io": "reverse_io" in f, "lengths": None, "views": None}
    if "lengths" in f and state:
        out["lengths"] = two_mixed_lengths(B, T)
    if "windows" in f:
        Tsrc = T + 7
        S, rows, starts = random_windows(B, Tsrc, out["lengths"] or [T] * B)
        out["views"] = (rows, starts, S, Tsrc)
    return out


def settings_a_and_b(name):
    """The two settings of test_lstm_settings_change_between_unsynchronised_calls: lengths, windows (rows, starts, S,
    Tsrc) and dropout triple.  B's differ from A's in every row -- length, source row and start --, in seed, subsequence
    and p, and in Tsrc."""
    (B, T, I, H, L), _ = FEATURE_CASES[name]
    a = {"lengths": two_mixed_lengths(B, T), "dropout": DROPOUT}
    S, rows, starts = random_windows(B, T + 7, a["lengths"])
    a["views"] = (rows, starts, S, T + 7)
    assert S >= 2
    rng = np.random.default_rng(77)
    lb = [int(v) if int(v) != n else (int(v) + 1) % (T + 1) for v, n in zip(rng.integers(0, T + 1, B), a["lengths"])]
    Tsrc = T + 11
    sb = [int(v) if int(v) != t else (t + 1 if t + 1 + n <= Tsrc else t - 1)
          for v, t, n in zip(rng.integers(0, Tsrc - np.asarray(lb) + 1), starts, lb)]
    b = {"lengths": lb, "dropout": (0.25, 99, 3), "views": ([(r + 1) % S for r in rows], sb, S, Tsrc)}
    return a, b

# every extern "C" function of include/csn_hip.h with a csnStream_t parameter
CASE_TABLE = {
    "csn_eeg_bandpass_znorm": [Stateless("csn_eeg_bandpass_znorm", "rows", _znorm((3, 5, 37), 3, scan=False)),
                               Stateless("csn_eeg_bandpass_znorm", "scan", _znorm((2, 8, 64), 3, scan=True))],
    "csn_eeg_filtfilt": [Stateless("csn_eeg_filtfilt", "s2_t64_c5", _filtfilt)],
    "csn_eeg_bandpass_stream": [Stateless("csn_eeg_bandpass_stream", "rows", _bandpass_stream((3, 5, 37), 3, scan=False)),
                                Stateless("csn_eeg_bandpass_stream", "scan", _bandpass_stream((2, 8, 64), 3, scan=True))],
    "csn_lstm_workspace_init": InTest("test_workspace_init_and_status_word_in_stream_order"),
    "csn_lstm_forward": InTest(*_LSTM_FORWARD_TESTS),
    "csn_lstm_backward": InTest(*(t for t in _LSTM_TESTS if "_forward_with_late_inputs" not in t)),
    "csn_lstm_status_clear": InTest("test_workspace_init_and_status_word_in_stream_order"),
    "csn_lstm_status_raise": InTest("test_workspace_init_and_status_word_in_stream_order"),
    # the five routes of gemm_nt() in csrc/gemm_nt.hip in the order it tries them (the wide one in both tile widths: 16 x 16
    # tiles of 256 x 256, 64 x 4 tiles of 256 x 192 where 64 x 3 tiles of 256 do not fill the chip), and one accumulating call
    "csn_gemm_nt": [Stateless("csn_gemm_nt", "wide256", _gemm_nt("wide256", 4096, 4096, 128, BF16, BF16)),
                    Stateless("csn_gemm_nt", "wide192", _gemm_nt("wide192", 16384, 768, 128, BF16, BF16)),
                    Stateless("csn_gemm_nt", "tile256x128", _gemm_nt("tile256x128", 256, 1024, 256, BF16, F32)),
                    Stateless("csn_gemm_nt", "dma", _gemm_nt("dma", 130, 132, 64, BF16, F32)),
                    Stateless("csn_gemm_nt", "bf16_k40", _gemm_nt("bf16", 70, 132, 40, BF16, F32)),
                    Stateless("csn_gemm_nt", "generic_f32", _gemm_nt("generic", 33, 20, 7, F32, F32)),
                    Stateless("csn_gemm_nt", "dma_accumulate", _gemm_nt("dma", 130, 132, 64, BF16, F32, accumulate=True))],
    "csn_gemm_tn": [Stateless("csn_gemm_tn", "tile128", _gemm_tn("tile128", 136, 72, 600)),
                    Stateless("csn_gemm_tn", "tile256", _gemm_tn("tile256", 256, 256, 8192))],
    "csn_lstm_cell_forward": [Stateless("csn_lstm_cell_forward", "f32_b70_h96", _cell_forward(70, 96, F32)),
                              Stateless("csn_lstm_cell_forward", "bf16_b70_h256", _cell_forward(70, 256, BF16))],
    "csn_lstm_cell_backward": [Stateless("csn_lstm_cell_backward", "f32_b70_h96", _cell_backward(70, 96, F32)),
                               Stateless("csn_lstm_cell_backward", "bf16_b70_h256", _cell_backward(70, 256, BF16))],
    "csn_cosine_loss": [Stateless("csn_cosine_loss", "b6_d33", _cosine)],
    "csn_rmsprop_step": [Stateless("csn_rmsprop_step", "n5000", _rmsprop)],
    "csn_flat_segments_prepare": [Stateless("csn_flat_segments_prepare", "3seg", _segments_prepare)],
    "csn_flat_segment_norms": [Stateless("csn_flat_segment_norms", "3seg", _segment_norms)],
    "csn_flat_clip": [Stateless("csn_flat_clip", "3seg", _flat_clip)],
    "csn_adam_step": [Stateless("csn_adam_step", "adamw_clip", _adam)],
    "csn_lars_step": [Stateless("csn_lars_step", "3seg", _lars)],
    "csn_barlow_offdiag_sqsum": [Stateless("csn_barlow_offdiag_sqsum", "d65", _barlow)],
    "csn_l2_topk": [Stateless("csn_l2_topk", "ng100_k64", _l2_topk)],
    "csn_l2_topk_tiled": [Stateless("csn_l2_topk_tiled", "splits1", _l2_topk_tiled(1)),
                          Stateless("csn_l2_topk_tiled", "splits7", _l2_topk_tiled(7))],
}

STATELESS_CASES = [c for v in CASE_TABLE.values() if isinstance(v, list) for c in v]


def timed(fn):
    """-> (result, host seconds of the call alone)."""
    t0 = time.perf_counter()
    out = fn()
    return out, time.perf_counter() - t0
