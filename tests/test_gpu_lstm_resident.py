"""GPU: the CU-resident LSTM recurrence (CSN_LSTM_RESIDENT plans, path 5; csrc/lstm_resident.hip) against path 0.

The contract is bit identity: every output (y_last, y_all, h_n, c_n) and every gradient (all dw_*, all db_*, dx, dh0, dc0)
of a resident plan equals, with torch.equal, that of the same plan on the per-step cell kernels (path 0), with every plan
feature.  No tolerance appears anywhere: path 0 is held against the float64 and bf16-faithful oracles elsewhere in the
suite, and identity with it carries those results over.  The baseline plan is created under CSN_CELL_V1=1 (read at plan
creation), which is what puts bf16 H = 128 -- and float32 H = 128 without state -- on path 0.

The featured runs go through the runner of tests/test_gpu_lstm_feature_fuzz.py (_featured: one forward + backward with
exactly the arguments a case record names) on hand-written case records; input windows, two accumulating forwards, the
inference plan, chaining through the state and the stream-order procedure have small drivers here.

Float32 at H = 128 is NOT refused: the K-split summation order of path 0 there (4 / 8 partial sums from 0.0, added in k
order) is formed inside the resident kernels without scratch, and its cases below assert identity like the others."""
import contextlib
import os

import numpy as np
import pytest
import torch
from torch.nn.utils.rnn import pack_padded_sequence

import lstm_feature_fuzz as fz
import stream_order as so
import test_gpu_lstm_feature_fuzz as ff
import test_gpu_lstm_state as st
import test_gpu_stream_order as stream_tests
from cerebralsignalnetworks_amd import cabi, BiLSTM, LSTM, Model, EEGFilters
from cerebralsignalnetworks_amd.trainer import DistillTrainer

pytestmark = pytest.mark.gpu

DEV, BF16, F32 = st.DEV, st.BF16, st.F32
NAN = float("nan")
RESIDENT = (5, "lstm_resident_fwd_kernel", "lstm_resident_bwd_kernel")
DTYPES = {"bf16": BF16, "f32": F32}


@contextlib.contextmanager
def _env(**kv):
    """The switches are read once, at plan creation."""
    old = {k: os.environ.get(k) for k in kv}
    os.environ.update(kv)
    try:
        yield
    finally:
        for k, v in old.items():
            os.environ.pop(k, None) if v is None else os.environ.__setitem__(k, v)


def _cell_kernels(H, dtype):
    ks = H % 128 == 0 if dtype == "f32" else H % 256 == 0
    return (0, "lstm_cell_fwd_ks_kernel", "lstm_cell_bwd_ks_kernel") if ks else (0, "lstm_cell_fwd_kernel", "lstm_cell_bwd_kernel")


def _pair(c, chunk="4", training=True):
    """(the resident plan, the path-0 plan) of a case record, both under CSN_LSTM_CHUNK = chunk."""
    args = (c["B"], c["T"], c["I"], c["H"], c["L"], DTYPES[c["dtype"]], DEV)
    kw = dict(training=training, state=c["state"], dropout=c["dropout_plan"], reverse=c["reverse"])
    with _env(CSN_LSTM_CHUNK=chunk):
        res = cabi.LstmPlan(*args, resident=True, **kw)
        with _env(CSN_CELL_V1="1"):
            base = cabi.LstmPlan(*args, **kw)
    assert ff._triple(res) == RESIDENT, ff._triple(res)
    assert ff._triple(base) == _cell_kernels(c["H"], c["dtype"]), ff._triple(base)
    lib = cabi.load()
    assert lib.csn_lstm_plan_workspace_bytes(res._plan) == lib.csn_lstm_plan_workspace_bytes(base._plan) > 0
    assert res.resident and not base.resident
    return res, base


def _record(B, T, I, H, L, dtype, seed=7, **over):
    """A case record as tests/lstm_feature_fuzz.py draws them: a CSN_LSTM_STATE plan, every output and every incoming
    gradient, the state arguments and their gradients, nothing else on."""
    c = dict(B=B, T=T, I=I, H=H, L=L, dtype=dtype, env={}, state=True, reverse=False, dropout_plan=False, dropout=None,
             pattern=None, lengths=None, outputs=st._OUT_KEYS, grads_in=st._BWD_IN, state_in=("h0", "c0"),
             state_grads_out=("dh0", "dc0"), want_dx=True, y_pitch=False, dy_pitch=False, y_half=1, dy_half=0, dx_add=False,
             x_view=None, accumulate=False, callback=False, data_seed=seed)
    c.update(over)
    c["id"] = f"b{B}t{T}i{I}h{H}l{L}-{dtype}"
    return c


def _lengths(B, T):
    """0 and T among them, the rest spread over 1 .. T-1."""
    n = [(3 * b + 1) % T for b in range(B)]
    n[0], n[1 % B], n[B - 1] = T, 0, max(1, T // 2)
    return n


def _finish(plans):
    torch.cuda.synchronize()
    for p in plans:
        assert p.status() == 0
        assert p.dgates_copies() == 0 and p.half_tile_launches(0) == 0 and p.half_tile_launches(1) == 0


def _identical(c, what, poison=False, chunk="4"):
    a = fz.make_inputs(c)
    w = ff._weights(a, c["L"])
    res, base = _pair(c, chunk)
    got = ff._featured(res, c, w, a)
    want = ff._featured(base, c, w, a)
    ff._same_bits(got, want, what)
    for k in c["outputs"] + c["state_grads_out"] + (("dx",) if c["want_dx"] else ()) + tuple(a["lp"]):
        assert k in got and bool(torch.isfinite(got[k]).all()), (what, k)
    if c["callback"]:
        assert got["fired"] == list(range(c["L"] - 1, -1, -1))
    if poison:                  # NaN / Inf in the padding of x and dy_all changes nothing
        ff._same_bits(ff._featured(res, c, w, a, poison=True), want, what + " NaN / Inf padding")
    _finish([res, base])
    return got


# ---- identity over shapes ---------------------------------------------------------------------------------------------------
# CSN_LSTM_CHUNK = 4: T = 11 is chunks of 4, 4 and 3 with boundaries inside the sequence.  B: a partial tile, a full
# tile, several tiles with a partial last one; H: workgroups of two, six and eight waves, one per unit tile of 16 (and 64:
# four).  Thinned product: every value of every axis with both dtypes, (B 37, H 128, L 5) and (B 5, H 96, L 3)
# whole.  A diagonal holds min(L, chunks) problems, so at three chunks L = 5 stays within one launch per diagonal: the
# second launch of a diagonal (more than four problems) is reached under CSN_LSTM_CHUNK = 2, six chunks.
SHAPES = [(37, 11, 20, 128, 5), (5, 11, 8, 96, 3), (16, 11, 8, 32, 1), (16, 1, 20, 96, 1), (37, 1, 8, 32, 3), (5, 11, 20, 128, 1),
          (16, 11, 8, 128, 3), (5, 11, 8, 64, 5), (37, 11, 20, 96, 5)]


@pytest.mark.parametrize("dtype", ["bf16", "f32"])
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "b%dt%di%dh%dl%d" % s)
def test_identity_over_shapes(shape, dtype):
    c = _record(*shape, dtype)
    _identical(c, c["id"])


@pytest.mark.parametrize("dtype", ["bf16", "f32"])
@pytest.mark.parametrize("shape", [(37, 11, 20, 128, 5), (5, 11, 8, 96, 5)], ids=lambda s: "b%dt%di%dh%dl%d" % s)
def test_identity_with_a_second_launch_per_diagonal(shape, dtype):
    c = _record(*shape, dtype)
    _identical(c, c["id"] + " chunk 2", chunk="2")


def test_the_shapes_cover_every_value_of_every_axis():
    for axis, values in ((0, {5, 16, 37}), (1, {1, 11}), (2, {8, 20}), (3, {32, 96, 128}), (4, {1, 3, 5})):
        assert values <= {s[axis] for s in SHAPES}, axis
    assert {(37, 128, 5), (5, 96, 3)} <= {(s[0], s[3], s[4]) for s in SHAPES}


@pytest.mark.parametrize("dtype", ["bf16", "f32"])
def test_inference_plan(dtype):
    """training = 0: no gates are saved (the kernel's gates pointer is null), the outputs are those of path 0."""
    c = _record(37, 11, 20, 96, 3, dtype)
    a = fz.make_inputs(c)
    w = ff._weights(a, c["L"])
    res, base = _pair(c, training=False)
    x, h0, c0 = (a[k].to(DEV) for k in ("x", "h0", "c0"))
    got = res.forward(x, *w, want_all=True, h0=h0, c0=c0, want_state=True)
    want = base.forward(x, *w, want_all=True, h0=h0, c0=c0, want_state=True)
    for k, g, b in zip(st._OUT_KEYS, got, want):
        assert torch.equal(g, b) and bool(torch.isfinite(g).all()), (dtype, k)
    _finish([res, base])


# ---- identity with features -----------------------------------------------------------------------------------------------------
FEATURE_SHAPES = [(6, 9, 12, 96, 3), (19, 9, 8, 128, 2)]
PLAIN = dict(state_in=(), grads_in=("dy_last", "dy_all"), state_grads_out=())


def _feature_record(shape, dtype, feature):
    B, T = shape[0], shape[1]
    on = lambda f: feature in (f, "all")      # noqa: E731
    over = dict(PLAIN)
    if on("state"):
        over.update(state_in=("h0", "c0"), grads_in=st._BWD_IN, state_grads_out=("dh0", "dc0"))
    if on("lengths"):
        over.update(lengths=_lengths(B, T), pattern="hand")
    if on("reverse"):
        over.update(reverse=True)
    if on("dropout"):
        over.update(dropout_plan=True, dropout=(0.5, 1234, 1))
    if on("io"):
        over.update(y_pitch=True, dy_pitch=True, dx_add=True)
    if on("accumulate"):
        over.update(accumulate=True)
    if on("callback"):
        over.update(callback=True)
    c = _record(*shape, dtype, **over)
    c["id"] += "-" + feature
    return c


@pytest.mark.parametrize("feature", ["none", "state", "lengths", "reverse", "dropout", "io", "accumulate", "callback", "all"])
@pytest.mark.parametrize("dtype", ["bf16", "f32"])
@pytest.mark.parametrize("shape", FEATURE_SHAPES, ids=lambda s: "b%dt%di%dh%dl%d" % s)
def test_identity_with_features(shape, dtype, feature):
    c = _feature_record(shape, dtype, feature)
    got = _identical(c, c["id"], poison=c["lengths"] is not None)
    if feature == "dropout":                   # the mask really is applied
        off = _identical(dict(c, dropout=(0.0, 0, 0)), c["id"] + " p = 0")
        assert not torch.equal(off["y_all"], got["y_all"])


def _windowed(plan, c, w, a, src, views, second=None):
    """Forward on input windows of `src` + backward; with `second`, another forward + backward on that source whose
    weight gradients are ADDED to the first's (CSN_GRAD_ACCUMULATE over two forwards)."""
    B, T, I, H, L = (c[k] for k in "BTIHL")
    d = {k: v.to(DEV) for k, v in a.items() if torch.is_tensor(v)}
    ff._settings(plan, c)
    fired, res = [], {}
    plan.set_grad_callback(fired.append)
    grads = [[torch.full_like(p, NAN) for p in group] for group in w]
    for n, x in enumerate([src] + ([second] if second is not None else [])):
        if views is not None:
            plan.set_views(*views)
        try:
            outs = plan.forward(x, *w, want_all=True, h0=d["h0"], c0=d["c0"], want_state=True)
        finally:
            plan.set_views(None)
        res.update({f"{k}{n}": v for k, v in zip(st._OUT_KEYS, outs)})
        res[f"dh0{n}"], res[f"dc0{n}"] = torch.full((L, B, H), NAN, device=DEV), torch.full((L, B, H), NAN, device=DEV)
        res[f"dx{n}"] = torch.full((B, T, I), NAN, device=DEV) if views is None else None
        plan.set_grad_mode(n > 0)
        plan.backward(d["dy_last"], d["dy_all"], grads, dx=res[f"dx{n}"], dh_n=d["dh_n"], dc_n=d["dc_n"], dh0=res[f"dh0{n}"],
                      dc0=res[f"dc0{n}"])
    plan.set_grad_mode(False)
    plan.set_grad_callback(None)
    for n, group in zip(fz.NAMES, grads):
        res.update({f"{n}_l{k}": t for k, t in enumerate(group)})
    return {k: v for k, v in res.items() if v is not None}, fired


def _equal_runs(got, want, what):
    (g, gf), (b, bf) = got, want
    assert list(g) == list(b) and gf == bf, what
    for k in g:
        assert torch.equal(g[k], b[k]) and bool(torch.isfinite(g[k]).all()), (what, k)


@pytest.mark.parametrize("everything", [False, True], ids=["alone", "with_reverse_dropout_lengths"])
@pytest.mark.parametrize("dtype", ["bf16", "f32"])
@pytest.mark.parametrize("shape", FEATURE_SHAPES, ids=lambda s: "b%dt%di%dh%dl%d" % s)
def test_identity_with_input_windows(shape, dtype, everything):
    """Rows of the batch are windows of a source [S, Tsrc, I] with NaN wherever no window reaches."""
    B, T, I, H, L = shape
    lengths = _lengths(B, T) if everything else [T] * B
    over = dict(lengths=lengths, pattern="hand")
    if everything:
        over.update(reverse=True, dropout_plan=True, dropout=(0.5, 1234, 1))
    c = _record(*shape, dtype, **over)
    a = fz.make_inputs(c)
    w = ff._weights(a, L)
    rng = np.random.default_rng(3)
    S, Tsrc = 4, T + 5
    rows = rng.integers(0, S, B).tolist()
    starts = [int(rng.integers(0, Tsrc - max(n, 1) + 1)) for n in lengths]
    g = torch.Generator().manual_seed(11)
    src = torch.randn(S, Tsrc, I, generator=g)
    reached = torch.zeros(S, Tsrc, dtype=torch.bool)
    for r, t0, n in zip(rows, starts, lengths):
        reached[r, t0:t0 + n] = True
    src[~reached] = NAN
    src = src.to(DEV)
    res, base = _pair(c)
    views = (rows, starts, S, Tsrc)
    _equal_runs(_windowed(res, c, w, a, src, views), _windowed(base, c, w, a, src, views), c["id"] + " windows")
    _finish([res, base])


@pytest.mark.parametrize("dtype", ["bf16", "f32"])
@pytest.mark.parametrize("shape", FEATURE_SHAPES, ids=lambda s: "b%dt%di%dh%dl%d" % s)
def test_identity_accumulating_over_two_forwards(shape, dtype):
    c = _record(*shape, dtype)
    a = fz.make_inputs(c)
    w = ff._weights(a, c["L"])
    x = a["x"].to(DEV)
    res, base = _pair(c)
    got = _windowed(res, c, w, a, x, None, second=x.flip(0).contiguous())
    _equal_runs(got, _windowed(base, c, w, a, x, None, second=x.flip(0).contiguous()), c["id"] + " two forwards")
    assert got[1] == 2 * list(range(c["L"] - 1, -1, -1))          # the callback: top layer first, once per backward
    once = _windowed(res, c, w, a, x, None)
    assert not torch.equal(once[0]["weight_hh_l0"], got[0]["weight_hh_l0"])
    _finish([res, base])


# ---- chunks chained through the state ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", ["bf16", "f32"])
def test_chunks_chained_through_the_state(dtype):
    """T = 9 as consecutive calls of T = 4, 4 and 1, (h_n, c_n) of one the (h0, c0) of the next: the outputs of one call."""
    B, I, H, L = 19, 8, 128, 2
    c = _record(B, 9, I, H, L, dtype)
    a = fz.make_inputs(c)
    w = ff._weights(a, L)
    x, h, cc = (a[k].to(DEV) for k in ("x", "h0", "c0"))
    whole, base = _pair(c)
    want = whole.forward(x, *w, want_all=True, h0=h, c0=cc, want_state=True)
    on_cells = base.forward(x, *w, want_all=True, h0=h, c0=cc, want_state=True)
    pieces, t0, plans = [], 0, {}
    for n in (4, 4, 1):
        if n not in plans:
            plans[n] = _pair(_record(B, n, I, H, L, dtype))[0]
        _, y, h, cc = plans[n].forward(x[:, t0:t0 + n].contiguous(), *w, want_all=True, h0=h, c0=cc, want_state=True)
        pieces.append(y)
        t0 += n
    got = (pieces[-1][:, -1], torch.cat(pieces, dim=1), h, cc)
    for k, g, b, v1 in zip(st._OUT_KEYS, got, want, on_cells):
        assert torch.equal(g, b) and torch.equal(b, v1), (dtype, k)
    _finish([whole, base] + list(plans.values()))


# ---- launch counts -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("L,chunk,launches", [(3, "4", 3 + 3 - 1), (5, "4", 3 + 5 - 1), (5, "2", 6 + 5 - 1 + 2)],
                         ids=["l3", "l5", "l5_chunk2_second_launches"])
def test_launch_counts(L, chunk, launches):
    """T 11: ceil(11 / chunk) + L - 1 chunk diagonals, one launch each up to four problems; at chunk 2 (six chunks) the two
    diagonals of L = 5 that hold five problems take a second launch.  (Path 0 launches once per STEP diagonal.)"""
    c = _record(16, 11, 8, 96, L, "bf16")
    a = fz.make_inputs(c)
    w = ff._weights(a, L)
    res, base = _pair(c, chunk)
    res.profile_enable(True)
    ff._featured(res, c, w, a)
    torch.cuda.synchronize()
    p = res.profile_read()
    assert (p["fwd_launches"], p["fwd_cells"]) == (launches, 11 * L), p
    assert (p["bwd_launches"], p["bwd_cells"]) == (launches, 11 * L), p
    assert p["fwd_ms"] > 0 and p["bwd_ms"] > 0
    _finish([res, base])


# ---- stream order ------------------------------------------------------------------------------------------------------------------
def test_stream_order_with_late_inputs_and_early_readers(cuda):
    """The procedure of tests/test_gpu_stream_order.py (late inputs behind a Delay, outputs snapshotted and inputs poisoned
    directly behind the call) on a resident plan, forward and backward on a side stream."""
    B, T, I, H, L = 19, 9, 8, 128, 2
    c = _record(B, T, I, H, L, "bf16")
    a = fz.make_inputs(c)
    plan, _ = _pair(c)
    groups = ("w_ih", "w_hh", "b_ih", "b_hh")
    fwd_in = {"x": a["x"].to(DEV), "h0": a["h0"].to(DEV), "c0": a["c0"].to(DEV),
              **{g: list(ws) for g, ws in zip(groups, ff._weights(a, L))}}
    bwd_in = {k: a[k].to(DEV) for k in st._BWD_IN}

    def forward(f):
        outs = plan.forward(f["x"], *[f[g] for g in groups], want_all=True, h0=f["h0"], c0=f["c0"], want_state=True)
        return dict(zip(st._OUT_KEYS, outs))

    def backward(g):
        grads = {k: [torch.full_like(t, NAN) for t in fwd_in[k]] for k in groups}
        out = {"dx": torch.full((B, T, I), NAN, device=DEV), "dh0": torch.full((L, B, H), NAN, device=DEV),
               "dc0": torch.full((L, B, H), NAN, device=DEV)}
        plan.backward(g["dy_last"], g["dy_all"], [grads[k] for k in groups], dx=out["dx"], dh_n=g["dh_n"], dc_n=g["dc_n"],
                      dh0=out["dh0"], dc0=out["dc0"])
        return {**out, **grads}

    want_f = stream_tests._synced(lambda: forward(fwd_in))
    want_b = stream_tests._synced(lambda: backward(bwd_in))
    s = torch.cuda.Stream()
    t_f = stream_tests._warm(s, lambda: forward(fwd_in))
    t_b = stream_tests._warm(s, lambda: backward(bwd_in))
    with torch.cuda.stream(s):
        stream_tests._forget_workspace(plan)
    s.synchronize()
    delay, la = so.late_all(s, fwd_in, so.delay_ms_for(t_f))
    with torch.cuda.stream(s):
        out = forward(la)
    running_f = delay.still_running()
    snap_f = so.snapshot_then_poison(s, out, la)          # x, weights, h0, c0 are gone before the backward runs
    s.synchronize()
    delay, lg = so.late_all(s, bwd_in, so.delay_ms_for(t_b))
    with torch.cuda.stream(s):
        out = backward(lg)
    running_b = delay.still_running()
    snap_b = so.snapshot_then_poison(s, out, lg)
    s.synchronize()
    assert running_f and running_b
    so.assert_same_bits(snap_f, want_f, "resident forward")
    so.assert_same_bits(snap_b, want_b, "resident backward")
    assert plan.status() == 0


# ---- module surface ---------------------------------------------------------------------------------------------------------------
def _module_run(m, x, hx, lengths, dy, dh, dc):
    hx = None if hx is None else tuple(t.clone().requires_grad_(True) for t in hx)
    for p in m.parameters():
        p.grad = None
    out, (h_n, c_n) = m(x, hx) if lengths is None else m(x, hx, lengths=lengths)
    data = out.data if isinstance(out, torch.nn.utils.rnn.PackedSequence) else out
    torch.autograd.backward([data, h_n, c_n], [dy[:data.shape[0]] if data.dim() == 2 else dy, dh, dc])
    res = dict(out=data.detach(), h_n=h_n.detach(), c_n=c_n.detach(), **{k: p.grad.clone() for k, p in m.named_parameters()})
    if hx is not None:
        res.update(dh0=hx[0].grad, dc0=hx[1].grad)
    return res


@pytest.mark.parametrize("dtype", ["bf16", "f32"])
@pytest.mark.parametrize("cls", [LSTM, BiLSTM], ids=["LSTM", "BiLSTM"])
def test_module_with_and_without_the_flag(cls, dtype):
    B, T, I, H, L = 6, 9, 96, 96, 2
    D = 2 if cls is BiLSTM else 1
    torch.manual_seed(5)
    plain = cls(I, H, L, compute_dtype=DTYPES[dtype]).to(DEV)
    res = cls(I, H, L, compute_dtype=DTYPES[dtype], resident=True).to(DEV)
    res.load_state_dict(plain.state_dict(), strict=True)
    g = torch.Generator().manual_seed(6)
    r = lambda *s: torch.randn(*s, generator=g).to(DEV)      # noqa: E731
    x, hx = r(B, T, I), (0.5 * r(D * L, B, H), r(D * L, B, H))
    dy, dh, dc = 0.1 * r(B, T, D * H), r(D * L, B, H), r(D * L, B, H)
    lengths = [9, 4, 0, 1, 9, 6]
    order = sorted(range(B), key=lambda b: -max(lengths[b], 1))
    packed = pack_padded_sequence(x[order], torch.tensor([max(lengths[b], 1) for b in order]), batch_first=True)
    dy_packed = 0.1 * r(packed.data.shape[0], D * H)
    calls = {"plain": (x, None, None, dy), "hx": (x, hx, None, dy), "lengths": (x, hx, lengths, dy),
             "packed": (packed, hx, None, dy_packed)}
    for what, (inp, state, lens, grad) in calls.items():
        got = _module_run(res, inp, state, lens, grad, dh, dc)
        want = _module_run(plain, inp, state, lens, grad, dh, dc)
        assert list(got) == list(want)
        for k in got:
            assert torch.equal(got[k], want[k]) and bool(torch.isfinite(got[k]).all()), (cls.__name__, dtype, what, k)
    torch.cuda.synchronize()
    assert res.all_plans() and all(pl.path() == 5 and pl.resident and pl.status() == 0 for pl in res.all_plans())
    assert plain.all_plans() and all(pl.path() == 0 and pl.status() == 0 for pl in plain.all_plans())


def test_trainer_step_leaves_the_same_loss_and_parameters(cuda):
    """Model(96, 96, 2, 384, True) through one DistillTrainer.train_step (featdist, rmsprop) at B 16, T 32."""
    B, T, C, D = 16, 32, 96, 384
    torch.manual_seed(7)
    plain = Model(C, 96, 2, D, True).to(cuda)
    res = Model(C, 96, 2, D, True, resident=True).to(cuda)
    res.load_state_dict(plain.state_dict(), strict=True)
    g = torch.Generator().manual_seed(8)
    eeg, tgt = torch.randn(B, C, T, generator=g).to(cuda), torch.randn(B, D, generator=g).to(cuda)
    lab = torch.randint(0, 40, (B,), generator=g).to(cuda)
    sos = EEGFilters(1000, order=3).sos
    start = {k: v.clone() for k, v in plain.state_dict().items()}
    losses = []
    for m in (plain, res):
        tr = DistillTrainer(m, sos, loss="featdist", lr=1e-3, optimizer="rmsprop", nepochs=100)
        losses.append(tr.train_step(eeg, tgt, lab, epoch=25))
        tr.check_device_status()
    torch.cuda.synchronize()
    assert torch.equal(losses[0], losses[1]) and bool(torch.isfinite(losses[0]).all())
    for (k, p), (_, q) in zip(plain.state_dict().items(), res.state_dict().items()):
        assert torch.equal(p, q), k
    assert not torch.equal(res.state_dict()["lstm.weight_hh_l0"], start["lstm.weight_hh_l0"])      # the step moved the LSTM
    assert all(pl.path() == 5 for pl in res.lstm.all_plans()) and all(pl.path() == 0 for pl in plain.lstm.all_plans())


# ---- command line -----------------------------------------------------------------------------------------------------------------
def test_cli_prints_the_epoch_line_of_the_run_without_the_flag(cuda, tmp_path, capsys, monkeypatch):
    import LstmDistillFromDinoV2Train as train
    paths = []
    init = cabi.LstmPlan.__init__

    def recording_init(self, *a, **kw):
        init(self, *a, **kw)
        paths.append(self.path())
    monkeypatch.setattr(cabi.LstmPlan, "__init__", recording_init)
    lines, hists = [], []
    for flag in ([], ["--resident_lstm"]):
        capsys.readouterr()
        hists.append(train.main(["--synthetic", "64", "--num_epochs", "1", "--batch_size", "16", "--log_dir", str(tmp_path)] + flag))
        torch.cuda.synchronize()
        lines.append([ln for ln in capsys.readouterr().out.splitlines() if ln.startswith("EPOCH 0 ")])
        hists[-1] = (hists[-1], sorted(set(paths)))
        paths.clear()
    assert len(lines[0]) == 1 and lines[0] == lines[1], lines
    assert hists[0][0] == hists[1][0] and np.isfinite(hists[0][0][0])
    assert hists[0][1] == [0] and hists[1][1] == [5]
