"""GPU: the attention readout of the LSTM (csn_lstm_plan_set_attention), through the C ABI and the modules.

1. forward      y_last against the SAME call's y_all and q in float64 (tests/lstm_attn_reference.py): within ulp32(y_last) +
                2^-40 (derived there); attn_out within ulp32 + 2^-40 a, summing to 1, zero in the padding; two calls the same
                bits; y_all, h_n, c_n with the bits of the call with attention off; an inference plan.
2. saturation   q = 3000 x a sign pattern: everything finite, the bound holds, one-hot weights where the restatement's are.
3. q = 0        the float64 mean within the same bound, attn_out = fl32(1 / n) exactly.
4. backward     THE IDENTITY: every LSTM gradient of an attention call has the bits of the same plan with attention off under
                "last", fed dy_last = NULL and dy_all' = fl32(dy_all + G), G built on the host from the library's own attn_out
                and dscore_out; x and dy_all hold NaN past each row's length in both calls.  dscore_out and dq against the
                restatement within their bounds; dq = NULL changes no other bit; an empty row gets nothing from dy_last.
5. features     lengths, input windows, inter-layer dropout and pitched y_all / dy_all together, plain and reverse; output
                dropout leaves y_last alone.
6. hygiene      refusals on real plans keep the setting; off after on is a fresh plan's call, launches included; the readout
                mode underneath comes back.
7. modules      HipLSTM(readout="attn"), LSTM.pooled, BiLSTM.pooled, Model(readout="attn"), direct_grads, a CLI round trip.
8. stream order the attention forward and backward on a side stream with late inputs (tests/lstm_attn_stream_cases.py).

Regimes of 1 to 4: those of tests/test_gpu_lstm_readout.py -- B 5, T 37, I 24, L 2 (ragged, a resident chunk boundary at 32 with
a 5-step tail) at H 32 and 96 in bf16 and float32 on path 0 and path 5, and one regime of tests/lstm_width_matrix.py (B 65,
T 9) per path 1, 2, 3, 4."""
import os
import time

import numpy as np
import pytest
import torch

import lstm_attn_reference as aref
import lstm_attn_stream_cases as stream_cases
import stream_order as so
import test_gpu_lstm_readout as rt
import test_lstm_attn_cpu as cpu_checks
from cerebralsignalnetworks_amd import cabi
from cerebralsignalnetworks_amd.lstm_model import BiLSTM, HipLSTM, LSTM, Model

pytestmark = pytest.mark.gpu

DEV, BF16, F32, NAN = rt.DEV, rt.BF16, rt.F32, rt.NAN
GROUPS, GRAD_KEYS, REGIMES = rt.GROUPS, rt.GRAD_KEYS, rt.REGIMES


def _query(H, seed=31, amp=4.0):
    """|q_h| <= amp."""
    q = (2 * torch.rand(H, generator=torch.Generator().manual_seed(seed)) - 1) * amp
    assert float(q.abs().max()) <= amp
    return q.to(DEV)


def _call(plan, w, a, q, lengths=None, dy_last=None, dy_all=None, state_grads=False, accumulate=False, backward=True, want_dq=True,
          readout="last", scale=None, prev_dq=None):
    """forward (every output) + backward of one plan, with the attention readout under query ``q`` (None: attention off, and
    ``readout`` governs); x and dy_all hold NaN past each row's length.  With q: attn_fwd / attn_bwd (the weights after each
    call), dscore and dq (None without want_dq) come back too.  Attention is off on the plan afterwards."""
    d = plan.desc
    pad = rt._pad(lengths, d.B, d.T)
    if plan.state:
        plan.set_lengths(lengths)
    else:
        assert lengths is None
    plan.set_readout(readout)
    out = {}
    try:
        if q is not None:
            attn_out, dscore = (torch.full((d.B, d.T), NAN, device=DEV) for _ in range(2))
            dq = None
            if want_dq and backward:
                dq = prev_dq.clone() if accumulate else torch.full((d.H,), NAN, device=DEV)
            plan.set_attention(q, scale, dq, attn_out, dscore)
        else:
            plan.set_attention()
        kw = dict(h0=a["h0"], c0=a["c0"]) if plan.state else {}
        x = torch.where(pad, torch.full_like(a["x"], NAN), a["x"])
        outs = plan.forward(x, *w, want_all=True, want_state=plan.state, **kw)
        out.update(zip(("y_last", "y_all", "h_n", "c_n"), outs))
        if q is not None:
            out["attn_fwd"] = attn_out.clone()
            attn_out.fill_(NAN)
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
        out.update({f"d{n}": g for n, g in zip(GROUPS, grads)})
        if q is not None:
            out.update(attn_bwd=attn_out, dscore=dscore, dq=dq)
        return out
    finally:
        plan.set_attention()


def _check_forward(got, q, scale, lengths, T, what):
    """y_last and attn_out against the same call's y_all and q in float64."""
    v, y, a32 = got["y_all"].cpu().numpy(), got["y_last"].cpu().numpy(), got["attn_fwd"].cpu().numpy()
    assert np.abs(v).max() < 1.0                                       # (the premise of the bound: |h| < 1)
    exact, a64 = aref.forward(v, q.cpu().numpy(), scale, lengths)
    err, bound = np.abs(y.astype(np.float64) - exact), aref.value_bound(y)
    print(f"{what}: y_last error {err.max():.3e}, largest error / bound {float((err / bound).max()):.3f}")
    assert np.isfinite(y).all() and (err <= bound).all(), (what, float((err / bound).max()))
    aerr, abound = np.abs(a32.astype(np.float64) - a64), aref.attn_bound(a32)
    assert (aerr <= abound).all(), (what, "attn_out", float((aerr / abound).max()))
    for b, n in enumerate(aref.rows(lengths, *v.shape[:2])):
        assert not a32[b, n:].any() and not np.signbit(a32[b, n:]).any(), (what, "weights past the row's length")
        if n == 0:
            assert not y[b].any() and not np.signbit(y[b]).any(), (what, "a row of length 0 gives zeros")
        else:
            assert abs(float(a32[b].astype(np.float64).sum()) - 1.0) <= T * 2.0 ** -24, (what, "weights sum to 1")
    return a64


def _scale(H):
    return float(np.float32(H ** -0.5))


# ---- 1. forward -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(REGIMES))
def test_forward_attends_over_the_calls_own_y_all(cuda, name):
    r, plan, w, a = rt._world(name)
    B, T, _, H, _ = r["shape"]
    q = _query(H)
    for lengths in ([None, rt._lengths(B, T)] if r["state"] else [None]):
        what = f"{name} attn lengths {'yes' if lengths else 'no'}"
        got = _call(plan, w, a, q, lengths, backward=False)
        again = _call(plan, w, a, q, lengths, backward=False)
        off = _call(plan, w, a, None, lengths, backward=False)
        _check_forward(got, q, _scale(H), lengths, T, what)
        rt._same(again, got, ("y_last", "attn_fwd", "y_all", "h_n", "c_n"), what + " (second call)")
        rt._same(got, off, ("y_all", "h_n", "c_n"), what + " (against attention off)")
        if lengths is None:
            assert not so.same_bits(got["y_last"], off["y_last"])
    torch.cuda.synchronize()
    assert plan.status() == 0


def test_an_inference_plan_attends_too(cuda):
    r = REGIMES["p0_h32_bf16"]
    plan, (w, a) = rt._plan(r, training=False), rt._inputs(r["shape"])
    B, T, _, H, _ = r["shape"]
    lengths = rt._lengths(B, T)
    got = _call(plan, w, a, _query(H), lengths, backward=False)
    _check_forward(got, _query(H), _scale(H), lengths, T, "inference attn")


def test_a_batch_of_empty_rows_gives_zeros_and_no_query_gradient(cuda):
    """Every row of length 0: no recurrence runs; the readout, the weights, the score gradients and dq are zero, and dq is
    left as it is under accumulation; a backward without dy_last zeroes dq too."""
    r = REGIMES["p0_h32_bf16"]
    B, T, _, H, _ = r["shape"]
    plan, (w, a) = rt._plan(r), rt._inputs(r["shape"])
    q, prev = _query(H), torch.ones(H, device=DEV)
    got = _call(plan, w, a, q, [0] * B, a["dy_last"], None, True)
    for k in ("y_last", "attn_fwd", "attn_bwd", "dscore", "dq"):
        assert not bool(got[k].any()), k
    assert so.same_bits(got["dh0"], a["dh_n"])
    kept = _call(plan, w, a, q, [0] * B, a["dy_last"], None, True, accumulate=True, prev_dq=prev)
    assert so.same_bits(kept["dq"], prev)
    no_dy = _call(plan, w, a, q, rt._lengths(B, T), None, a["dy_all"], True)
    assert not bool(no_dy["dq"].any()) and bool(torch.isfinite(no_dy["dx"]).all())
    assert plan.status() == 0


# ---- 2. a saturated softmax -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["p0_h32_bf16", "p5_h96_f32", "p3_ks384_gemm"])
def test_a_saturated_softmax_stays_finite_and_one_hot(cuda, name):
    r, plan, w, a = rt._world(name)
    B, T, _, H, _ = r["shape"]
    sign = torch.where(torch.rand(H, generator=torch.Generator().manual_seed(5)) < 0.5, -1.0, 1.0)
    q = (3000.0 * sign).to(DEV)
    lengths = rt._lengths(B, T) if r["state"] else None
    got = _call(plan, w, a, q, lengths, a["dy_last"])
    a64 = _check_forward(got, q, _scale(H), lengths, T, f"{name} saturated")
    assert all(bool(torch.isfinite(t).all()) for k in GRAD_KEYS + ("dq", "dscore", "attn_bwd") if k in got for t in so._leaves(got[k]))
    a32 = got["attn_fwd"].cpu().numpy()
    # one-hot in float32: the runner-up lies far below float32's smallest denormal (2^-149), so its rounding is no question
    hot = (a64.max(axis=1) == 1.0) & (np.sort(a64, axis=1)[:, -2] < 2.0 ** -160)
    assert hot.sum() >= 1, "no row of the restatement is one-hot in float32: the fixture proves nothing"
    for b in np.flatnonzero(hot):
        assert np.array_equal(a32[b], (a64[b] == 1.0).astype(np.float32)), (name, b)


# ---- 3. q = 0 is the mean -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["p0_h96_bf16", "p5_h32_f32", "p2_p2_384"])
def test_a_zero_query_is_mean_pooling(cuda, name):
    r, plan, w, a = rt._world(name)
    B, T, _, H, _ = r["shape"]
    lengths = rt._lengths(B, T) if r["state"] else None
    got = _call(plan, w, a, torch.zeros(H, device=DEV), lengths, backward=False)
    v, y, a32 = got["y_all"].cpu().numpy(), got["y_last"].cpu().numpy(), got["attn_fwd"].cpu().numpy()
    n = np.array(aref.rows(lengths, B, T), np.float64)[:, None]
    exact = np.where(n > 0, v.astype(np.float64).sum(axis=1) / np.maximum(n, 1), 0.0)
    err, bound = np.abs(y - exact), aref.value_bound(y)
    print(f"{name} q = 0: mean error {err.max():.3e}, largest error / bound {float((err / bound).max()):.3f}")
    assert (err <= bound).all()
    for b, k in enumerate(aref.rows(lengths, B, T)):
        assert np.array_equal(a32[b, :k], np.full(k, np.float32(1.0 / max(k, 1)))) and not a32[b, k:].any()


# ---- 4. the backward identity ---------------------------------------------------------------------------------------------
def _check_backward_readbacks(got, q, scale, lengths, dy_last, accumulate, prev_dq, what):
    """attn_out again, dscore_out and dq against the restatement."""
    v = got["y_all"].cpu().numpy()
    B, T, _ = v.shape
    assert so.same_bits(got["attn_bwd"], got["attn_fwd"]), what + ": the backward's attn_out has the forward's bits"
    w32 = got["dscore"].cpu().numpy()
    w64, g64 = aref.dscore(v, q.cpu().numpy(), scale, lengths, dy_last.cpu().numpy())
    werr, wbound = np.abs(w32 - w64), aref.dscore_bound(w32, scale, np.abs(g64).max(axis=1, keepdims=True))
    assert (werr <= wbound).all(), (what, "dscore_out", float((werr / wbound).max()))
    for b, n in enumerate(aref.rows(lengths, B, T)):
        assert not w32[b, n:].any(), (what, "score gradients past the row's length")
    if got["dq"] is None:
        return
    dq = got["dq"].cpu().numpy()
    exact = aref.dq(w32, v, lengths)
    bound = aref.dq_bound(dq, B, T, w32)
    if accumulate:
        # fl32(prev + fl32(sum)): the sum's own rounding (an ulp of it) joins the bound of the value stored
        exact, bound = prev_dq.cpu().numpy().astype(np.float64) + exact, bound + aref.ulp32(exact)
    err = np.abs(dq - exact)
    print(f"{what}: dq error {err.max():.3e}, largest error / bound {float((err / bound).max()):.3f}")
    assert np.isfinite(dq).all() and (err <= bound).all(), (what, "dq", float((err / bound).max()))
    assert np.abs(dq).max() > 0


def _identity(plan, w, a, q, lengths, with_dy_all, state_grads, accumulate, what):
    H = plan.desc.H
    prev_dq = 0.25 * torch.randn(H, generator=torch.Generator().manual_seed(41)).to(DEV)
    dy_all = a["dy_all"] if with_dy_all else None
    got = _call(plan, w, a, q, lengths, a["dy_last"], dy_all, state_grads, accumulate, prev_dq=prev_dq)
    G = torch.from_numpy(aref.expand(got["attn_bwd"].cpu().numpy(), got["dscore"].cpu().numpy(), q.cpu().numpy(),
                                     a["dy_last"].cpu().numpy(), lengths)).to(DEV)
    want = _call(plan, w, a, None, lengths, None, a["dy_all"] + G if with_dy_all else G, state_grads, accumulate)
    rt._same(got, want, GRAD_KEYS + ("y_all", "h_n", "c_n"), what)
    assert all(bool(torch.isfinite(t).all()) for k in GRAD_KEYS if k in got for t in so._leaves(got[k])), what
    _check_backward_readbacks(got, q, _scale(H), lengths, a["dy_last"], accumulate, prev_dq, what)
    if lengths is not None and state_grads:
        for b in (b for b, n in enumerate(lengths) if n == 0):       # nothing of dy_last reaches an empty row: dh0 = dh_n
            assert so.same_bits(got["dh0"][:, b], a["dh_n"][:, b]) and so.same_bits(got["dc0"][:, b], a["dc_n"][:, b]), what
    return got


@pytest.mark.parametrize("name", list(REGIMES))
def test_backward_is_the_attention_off_call_on_the_expanded_gradient(cuda, name):
    r, plan, w, a = rt._world(name)
    B, T, _, H, _ = r["shape"]
    q = _query(H)
    cases = [("dy_last", None, False, False, False), ("dy_last + dy_all", None, True, False, False),
             ("dy_last + dy_all, accumulate", None, True, False, True)]
    if r["state"]:
        n = rt._lengths(B, T)
        cases += [("dy_last + dh_n + dc_n", None, False, True, False), ("dy_last, lengths", n, False, False, False),
                  ("everything, lengths", n, True, True, False), ("everything, lengths, accumulate", n, True, True, True)]
    seen = {}
    for label, lengths, with_dy_all, state_grads, accumulate in cases:
        seen[label] = _identity(plan, w, a, q, lengths, with_dy_all, state_grads, accumulate, f"{name} attn {label}")
    assert not so.same_bits(seen["dy_last"]["dweight_hh"][0], seen["dy_last + dy_all"]["dweight_hh"][0])
    # a frozen query (dq = NULL) changes no other bit
    label, lengths, with_dy_all, state_grads, _ = cases[-2 if r["state"] else 1]
    frozen = _call(plan, w, a, q, lengths, a["dy_last"], a["dy_all"] if with_dy_all else None, state_grads, want_dq=False)
    assert frozen["dq"] is None
    rt._same(frozen, seen[label], GRAD_KEYS + ("y_last", "y_all", "h_n", "c_n", "attn_fwd", "attn_bwd", "dscore"), f"{name} dq = NULL")
    torch.cuda.synchronize()
    assert plan.status() == 0


# ---- 5. plan features -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("reverse", [False, True], ids=["plain", "reverse"])
def test_every_plan_feature_at_once(cuda, reverse):
    """Lengths, input windows, inter-layer dropout at p 0.5 and pitched y_all / dy_all on one plan."""
    shape = (5, 37, 24, 32, 2)
    B, T, I, H, L = shape
    GAP, S, TSRC = 4, 3, 50
    w, a = rt._inputs(shape, seed=8)
    q = _query(H, seed=32)
    lengths, rows, starts = rt._lengths(B, T), [2, 0, 1, 2, 0], [13, 50, 49, 1, 7]
    src = torch.randn(S, TSRC, I, generator=torch.Generator().manual_seed(9)).to(DEV)
    plan = cabi.LstmPlan(*shape, BF16, DEV, training=True, state=True, dropout=True, reverse=reverse)
    plan.set_lengths(lengths)
    plan.set_dropout(0.5, 0x1234ABCD5678, 3)
    plan.set_io(H + GAP, H + GAP, False)
    plan.set_views(rows, starts, S, TSRC)
    pad = rt._pad(lengths, B, T)
    attn_out, dscore, dq = torch.full((B, T), NAN, device=DEV), torch.full((B, T), NAN, device=DEV), torch.full((H,), NAN, device=DEV)

    def run(attend, dy_last, dy_all):
        plan.set_attention(*((q, None, dq, attn_out, dscore) if attend else ()))
        y_buf = torch.full((B, T, H + GAP), 7.0, device=DEV)
        y_last, _, h_n, c_n = plan.forward(src, *w, want_state=True, y_all=y_buf[:, :, :H], h0=a["h0"], c0=a["c0"])
        attn_fwd = attn_out.clone()
        dy_buf = torch.full((B, T, H + GAP), NAN, device=DEV)
        dy_buf[:, :, :H] = torch.where(pad, torch.full_like(dy_all, NAN), dy_all)
        grads = [[torch.full_like(p, NAN) for p in group] for group in w]
        out = dict(y_last=y_last, y_buf=y_buf, h_n=h_n, c_n=c_n, dx=torch.full((B, T, I), NAN, device=DEV),
                   dh0=torch.full((L, B, H), NAN, device=DEV), dc0=torch.full((L, B, H), NAN, device=DEV))
        plan.backward(dy_last, dy_buf[:, :, :H], grads, dx=out["dx"], dh_n=a["dh_n"], dc_n=a["dc_n"], dh0=out["dh0"], dc0=out["dc0"])
        out.update({f"d{n}_l{k}": t for n, g in zip(GROUPS, grads) for k, t in enumerate(g)})
        return out, attn_fwd

    got, attn_fwd = run(True, a["dy_last"], a["dy_all"])
    y_all = got["y_buf"][:, :, :H].contiguous()
    assert bool((got["y_buf"][:, :, H:] == 7.0).all())
    what = f"features reverse={reverse} attn"
    _check_forward(dict(y_all=y_all, y_last=got["y_last"], attn_fwd=attn_fwd), q, _scale(H), lengths, T, what)
    assert so.same_bits(attn_out, attn_fwd)
    G = torch.from_numpy(aref.expand(attn_out.cpu().numpy(), dscore.cpu().numpy(), q.cpu().numpy(), a["dy_last"].cpu().numpy(), lengths)).to(DEV)
    _check_backward_readbacks(dict(y_all=y_all, attn_fwd=attn_fwd, attn_bwd=attn_out, dscore=dscore, dq=dq), q, _scale(H), lengths,
                              a["dy_last"], False, None, what)
    want, _ = run(False, None, a["dy_all"] + G)
    keys = [k for k in got if k != "y_last"]
    so.assert_same_bits({k: got[k] for k in keys}, {k: want[k] for k in keys}, what)
    torch.cuda.synchronize()
    assert plan.status() == 0


def test_output_dropout_leaves_the_attention_readout_alone(cuda):
    r = REGIMES["p0_h32_bf16"]
    B, T, I, H, L = r["shape"]
    plan, (w, a) = rt._plan(r), rt._inputs(r["shape"])
    lengths, q = rt._lengths(B, T), _query(H)
    clean = _call(plan, w, a, q, lengths, backward=False)
    plan.set_output_dropout(0.5, 0xFEEDFACE, 1, first=0, index_pitch=H)
    dropped = _call(plan, w, a, q, lengths, backward=False)
    plan.set_output_dropout(0.0)
    assert so.same_bits(dropped["y_last"], clean["y_last"]) and so.same_bits(dropped["attn_fwd"], clean["attn_fwd"])
    kept = dropped["y_all"] != 0
    assert 0.3 < float(kept.float().mean()) / (sum(lengths) / (B * T)) < 0.7         # the mask was on, at p = 0.5
    assert bool((dropped["y_all"][kept] == 2.0 * clean["y_all"][kept]).all())


# ---- 6. the sticky setter -------------------------------------------------------------------------------------------------
def test_setter_refusals_on_real_plans_keep_the_setting(cuda):
    lib = cabi.load()
    r = REGIMES["p0_h32_bf16"]
    B, T, _, H, _ = r["shape"]
    w, a = rt._inputs(r["shape"])
    for bits in (dict(), dict(state=False), dict(reverse=True), dict(dropout=True), dict(resident=True), dict(training=False)):
        plan = rt._plan(r, **bits)
        cpu_checks.check_set_attention_arguments(lib, plan._plan)
    plan = rt._plan(r)
    q, attn_out = _query(H), torch.full((B, T), NAN, device=DEV)
    ws = lib.csn_lstm_plan_workspace_bytes(plan._plan)
    plan.set_attention(q, None, None, attn_out)
    assert lib.csn_lstm_plan_set_attention(plan._plan, cabi._ptr(q), float("nan"), None, None, None) == 1     # refused: the plan still attends
    assert lib.csn_lstm_plan_set_attention(plan._plan, None, 1.0, cabi._ptr(q), None, None) == 1
    plan.set_lengths(None)
    y_last, y_all = plan.forward(a["x"], *w, want_all=True)
    _check_forward(dict(y_last=y_last, y_all=y_all, attn_fwd=attn_out), q, _scale(H), None, T, "kept setting")
    assert lib.csn_lstm_plan_workspace_bytes(plan._plan) == ws
    with pytest.raises(cabi.CsnError):
        plan.set_attention(None, None, q)
    with pytest.raises(cabi.CsnError):
        plan.set_attention(q[:-1])
    # the readout mode underneath comes back when attention is turned off
    plan.set_readout("mean")
    mean, _ = plan.forward(a["x"], *w, want_all=True)
    assert so.same_bits(mean, y_last)                     # (attention governs whatever the mode says)
    plan.set_attention()
    mean, y_all = plan.forward(a["x"], *w, want_all=True)
    rt._check_pooled_value(mean, y_all, None, "mean", T, "mean underneath")


@pytest.mark.parametrize("name", ["p0_h32_bf16", "p5_h96_bf16", "p3_ks384_gemm", "p4_f32p_256"])
def test_attention_off_after_on_is_a_fresh_plans_call(cuda, name):
    r = REGIMES[name]
    w, a = rt._inputs(r["shape"])
    used, fresh = rt._plan(r), rt._plan(r)
    for plan in (used, fresh):
        plan.profile_enable(True)
    lengths = rt._lengths(*r["shape"][:2]) if r["state"] else None
    _call(used, w, a, _query(r["shape"][3]), lengths, a["dy_last"], a["dy_all"], r["state"])
    got = _call(used, w, a, None, lengths, a["dy_last"], a["dy_all"], r["state"])
    want = _call(fresh, w, a, None, lengths, a["dy_last"], a["dy_all"], r["state"])
    torch.cuda.synchronize()
    rt._same(got, want, GRAD_KEYS + ("y_last", "y_all", "h_n", "c_n"), f"{name} off after on")
    if r["state"]:
        assert so.same_bits(got["y_last"], got["h_n"][-1])
    p_used, p_fresh = used.profile_read(), fresh.profile_read()
    for k in ("fwd_launches", "fwd_cells", "bwd_launches", "bwd_cells"):
        assert p_used[k] == p_fresh[k] and (p_used[k] > 0 or r["path"] == 0), (k, p_used, p_fresh)
    assert used.status() == 0 and fresh.status() == 0


# ---- 7. modules -----------------------------------------------------------------------------------------------------------
MB, MT, MI, MH, ML = rt.MB, rt.MT, rt.MI, rt.MH, rt.ML
M_LENGTHS = rt.M_LENGTHS


def _set_queries(m, seed=33):
    with torch.no_grad():
        for i, name in enumerate(n for n in ("attn_query", "attn_query_reverse") if hasattr(m, n)):
            getattr(m, name).copy_(_query(MH, seed + i))


def _check_module_value(y, output, weights, q, lengths, what):
    _check_forward(dict(y_last=y, y_all=output, attn_fwd=weights), q.detach(), _scale(MH), lengths, MT, what)


def test_hiplstm_attention_readout(cuda):
    torch.manual_seed(12)
    m = HipLSTM(MI, MH, ML, readout="attn").to(DEV)
    x = rt._module_x()
    # zeros at the start: mean pooling
    y_all, y = m(x, want_all=True)
    rt._check_pooled_value(y.detach(), y_all.detach(), None, "mean", MT, "HipLSTM attn at q = 0")
    _set_queries(m)
    y_all, y, weights = m(x, want_all=True, return_weights=True)
    assert y.shape == (MB, MH) and weights.shape == (MB, MT) and not weights.requires_grad and so.same_bits(m(x), y)
    _check_module_value(y.detach(), y_all.detach(), weights, m.attn_query, None, "HipLSTM attn")
    dyw = torch.randn(MB, MH, generator=torch.Generator().manual_seed(13)).to(DEV)
    got = rt._param_grads(m, (m(x) * dyw).sum())
    # the twin under "last": fed (y_all G).sum(), G from the library's own weights and score gradients
    plan = cabi.LstmPlan(MB, MT, MI, MH, ML, BF16, DEV, training=True)
    w = [[getattr(m, f"{n}_l{k}").detach() for k in range(ML)] for n in GROUPS]
    attn_out, dscore, dq = torch.empty(MB, MT, device=DEV), torch.empty(MB, MT, device=DEV), torch.empty(MH, device=DEV)
    plan.set_attention(m.attn_query, None, dq, attn_out, dscore)
    plan.forward(x, *w)
    plan.backward(dyw, None, [[torch.empty_like(p) for p in group] for group in w])
    assert so.same_bits(attn_out, weights)
    q = m.attn_query.detach()
    G = torch.from_numpy(aref.expand(attn_out.cpu().numpy(), dscore.cpu().numpy(), q.cpu().numpy(), dyw.cpu().numpy(), None)).to(DEV)
    twin = HipLSTM(MI, MH, ML).to(DEV)
    twin.load_state_dict({k: v for k, v in m.state_dict().items() if k != "attn_query"})
    want = rt._param_grads(twin, (twin(x, want_all=True)[0] * G).sum())
    so.assert_same_bits({k: got[k] for k in want}, want, "HipLSTM attn parameter gradients")
    exact = aref.dq(dscore.cpu().numpy(), y_all.detach().cpu().numpy(), None)
    err, bound = np.abs(got["attn_query"].cpu().numpy() - exact), aref.dq_bound(got["attn_query"].cpu().numpy(), MB, MT, dscore.cpu().numpy())
    assert (err <= bound).all() and so.same_bits(got["attn_query"], dq)
    assert all(pl.status() == 0 for pl in m.all_plans())


@pytest.mark.parametrize("cls", [LSTM, BiLSTM], ids=["LSTM", "BiLSTM"])
def test_drop_in_pooled_attention(cuda, cls):
    torch.manual_seed(14)
    m = cls(MI, MH, ML, attention=True).to(DEV)
    _set_queries(m)
    dirs = 2 if cls is BiLSTM else 1
    queries = [m.attn_query] + ([m.attn_query_reverse] if dirs == 2 else [])
    x = rt._module_x()
    g = torch.Generator().manual_seed(15)
    hx = tuple(t.to(DEV) for t in (0.5 * torch.randn(dirs * ML, MB, MH, generator=g), torch.randn(dirs * ML, MB, MH, generator=g)))
    dyw = torch.randn(MB, dirs * MH, generator=g).to(DEV)
    for lengths in (None, M_LENGTHS):
        what = f"{cls.__name__}.pooled attn lengths {lengths is not None}"
        with torch.no_grad():
            y, weights = m.pooled(x, hx, lengths=lengths, readout="attn", return_weights=True)
            output, _ = m(x, hx, lengths=lengths)
            assert so.same_bits(m.pooled(x, hx, lengths=lengths, readout="attn"), y)
        assert y.shape == (MB, dirs * MH) and weights.shape == ((MB, MT, 2) if dirs == 2 else (MB, MT))
        for d, q in enumerate(queries):      # each direction: its half, its query, its own softmax
            _check_module_value(y[:, d * MH:(d + 1) * MH], output[:, :, d * MH:(d + 1) * MH].contiguous(),
                                weights[:, :, d] if dirs == 2 else weights, q, lengths, f"{what} direction {d}")
        xg = x.clone().requires_grad_(True)
        got = rt._param_grads(m, (m.pooled(xg, hx, lengths=lengths, readout="attn") * dyw).sum())
        assert all(bool(torch.isfinite(t).all()) for t in got.values()) and bool(torch.isfinite(xg.grad).all())
        for d, q in enumerate(queries):      # the query's gradient: the float64 autograd of the same expression on the output
            out64 = output[:, :, d * MH:(d + 1) * MH].double()
            q64 = q.detach().double().requires_grad_(True)
            n = torch.tensor(lengths or [MT] * MB, device=DEV)
            z = _scale(MH) * (out64 @ q64)
            z = z.masked_fill(torch.arange(MT, device=DEV)[None, :] >= n[:, None], -float("inf"))
            z = torch.where(n[:, None] == 0, torch.zeros_like(z), z)          # (an empty row: no weights, and no NaN)
            a = torch.softmax(z, dim=1) * (n[:, None] > 0)
            ((a[:, :, None] * out64).sum(1) * dyw[:, d * MH:(d + 1) * MH].double()).sum().backward()
            name = "attn_query_reverse" if d else "attn_query"
            # (float32 score gradients w32, each within an ulp of its float64 value: relative 2^-23 of sum |w v|, |v| < 1)
            tol = 2.0 ** -22 * float(q64.grad.abs().max()) * MB * MT + 1e-7
            assert float((got[name].double() - q64.grad).abs().max()) <= tol, (what, name)
    packed = torch.nn.utils.rnn.pack_padded_sequence(x[[0, 3, 4]], torch.tensor([37, 36, 20]), batch_first=True)
    hx3 = tuple(t[:, [0, 3, 4]].contiguous() for t in hx)
    with torch.no_grad():
        assert so.same_bits(m.pooled(packed, hx3, readout="attn"), m.pooled(x[[0, 3, 4]], hx3, lengths=[37, 36, 20], readout="attn"))
    assert all(pl.status() == 0 and not pl.busy for pl in m.all_plans())


@pytest.mark.parametrize("bidirectional", [False, True], ids=["uni", "bi"])
def test_model_attention_readout_with_and_without_views(cuda, bidirectional):
    """Model(readout="attn"): fc reads the attention readout.  Held against fc of the drop-in's pooled(readout="attn") on the
    model's parameters: the same kernels on the same values, the same bits."""
    torch.manual_seed(16)
    D = 16
    model = Model(MI, MH, ML, D, include_top=False, bidirectional=bidirectional, readout="attn").to(DEV).eval()
    _set_queries(model.lstm)
    drop_in = (BiLSTM if bidirectional else LSTM)(MI, MH, ML, attention=True).to(DEV)
    drop_in.load_state_dict(model.lstm.state_dict())
    src = torch.randn(3, 50, MI, generator=torch.Generator().manual_seed(17)).to(DEV)
    views, lengths = ([2, 0, 1, 2, 0], [13, 50, 49, 1, 7]), list(M_LENGTHS)
    with torch.no_grad():
        for what, feat, pooled in (("dense", model(src[:, :MT]), drop_in.pooled(src[:, :MT].contiguous(), readout="attn")),
                                   ("views", model(src, views=views, lengths=lengths), drop_in.pooled(src, None, lengths, views, readout="attn"))):
            assert feat.shape == (len(pooled), D)
            assert so.same_bits(feat, model.fc(pooled)), what
    model.train()
    feat = model(src, views=views, lengths=lengths)
    feat.square().sum().backward()
    assert all(p.grad is not None and bool(torch.isfinite(p.grad).all()) for p in model.parameters())
    assert bool(model.lstm.attn_query.grad.any())
    assert all(pl.status() == 0 and not pl.busy for pl in model.lstm.all_plans())


def test_direct_grads_accumulate_sums_the_querys_gradient_over_two_forwards(cuda):
    torch.manual_seed(18)
    m = HipLSTM(MI, MH, ML, readout="attn").to(DEV)
    _set_queries(m)
    xs = [rt._module_x(19), rt._module_x(20)]
    singles = [rt._param_grads(m, m(x).square().sum()) for x in xs]
    for p in m.parameters():
        p.grad = torch.zeros_like(p)
    m.direct_grads = "accumulate"
    for x in xs:
        m(x).square().sum().backward()
    want = singles[0]["attn_query"] + singles[1]["attn_query"]            # fl32(fl32(0 + g1) + g2)
    assert so.same_bits(m.attn_query.grad, want) and bool(want.any())
    assert so.same_bits(m.weight_hh_l1.grad, singles[0]["weight_hh_l1"] + singles[1]["weight_hh_l1"])
    m.direct_grads = True                                                  # one forward per step: .grad is overwritten
    m(xs[0]).square().sum().backward()
    assert so.same_bits(m.attn_query.grad, singles[0]["attn_query"])


def test_cli_train_then_eval_with_attention_readout(cuda, tmp_path, monkeypatch):
    import LstmDistillFromDinoV2Eval as evaluate_cli
    import LstmDistillFromDinoV2Train as train
    from cerebralsignalnetworks_amd.trainer import DistillTrainer
    args = ["--synthetic", "64", "--batch_size", "16", "--num_epochs", "1", "--log_dir", str(tmp_path), "--hidden_size", "32",
            "--lstm_layers", "2", "--loss", "cosine", "--output_size", "24", "--dtype", "bf16", "--readout", "attn"]
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
    assert trainer.model.lstm.readout == "attn"
    query = trainer.model.lstm.attn_query.detach()
    assert bool(query.any()), "the query was trained: the checkpoint holds it, the evaluation loaded it"
    model = Model(input_size=eeg.shape[1], lstm_size=32, lstm_layers=2, output_size=24, include_top=False, compute_dtype=torch.bfloat16,
                  readout="attn").to(DEV)
    evaluate_cli.load_checkpoint_into(model, ckpt)
    assert so.same_bits(model.lstm.attn_query.detach(), query)
    assert so.same_bits(DistillTrainer(model, trainer.sos, loss="cosine").embed_all(eeg, batch), emb)
    with torch.no_grad():
        model.lstm.attn_query.zero_()
    assert not so.same_bits(DistillTrainer(model, trainer.sos, loss="cosine").embed_all(eeg, batch), emb)


# ---- 8. stream order ------------------------------------------------------------------------------------------------------
def test_attention_calls_on_a_side_stream_with_late_inputs(cuda):
    """The procedure of tests/test_gpu_stream_order.py on the case of tests/lstm_attn_stream_cases.py: the score, row and
    weighted-sum kernels behind the recurrence, then the pre-passes, the dq kernels and the attention dy_in, each with its inputs
    -- the query and dy_last among them -- late behind a Delay and overwritten directly behind the call."""
    t0 = time.perf_counter()
    shape, lengths = stream_cases.SHAPE, list(stream_cases.LENGTHS)
    B, T, I, H, L = shape
    plan = cabi.LstmPlan(*shape, BF16, DEV, training=True, state=True)
    w, a = rt._inputs(shape, seed=21)
    fwd_in = {"x": a["x"], "w": w, "h0": a["h0"], "c0": a["c0"], "q": _query(H, 34)}
    bwd_in = {k: a[k] for k in ("dy_last", "dy_all", "dh_n", "dc_n")}
    bwd_in["q"] = fwd_in["q"].clone()
    plan.set_lengths(lengths)

    def forward(f):
        attn_out = torch.full((B, T), NAN, device=DEV)
        plan.set_attention(f["q"], None, None, attn_out)
        out = dict(zip(("y_last", "y_all", "h_n", "c_n"), plan.forward(f["x"], *f["w"], want_all=True, want_state=True, h0=f["h0"], c0=f["c0"])))
        out["attn_out"] = attn_out
        return out

    def backward(g):
        out = dict(dx=torch.full((B, T, I), NAN, device=DEV), dh0=torch.full((L, B, H), NAN, device=DEV), dc0=torch.full((L, B, H), NAN, device=DEV),
                   attn_out=torch.full((B, T), NAN, device=DEV), dscore=torch.full((B, T), NAN, device=DEV), dq=torch.full((H,), NAN, device=DEV))
        grads = [[torch.full_like(p, NAN) for p in group] for group in w]
        plan.set_attention(g["q"], None, out["dq"], out["attn_out"], out["dscore"])
        plan.backward(g["dy_last"], g["dy_all"], grads, dx=out["dx"], dh_n=g["dh_n"], dc_n=g["dc_n"], dh0=out["dh0"], dc0=out["dc0"])
        out["grads"] = grads
        return out

    torch.cuda.synchronize()
    want_fwd = forward(fwd_in)
    want_bwd = backward(bwd_in)
    torch.cuda.synchronize()
    assert bool(want_bwd["dq"].any()) and so.same_bits(want_bwd["attn_out"], want_fwd["attn_out"])
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
    plan.set_attention()
    print(f"stream order attention: t_host {1e3 * t_fwd:.2f} / {1e3 * t_bwd:.2f} ms, delays ran {delay.measured_ms():.1f} / "
          f"{delay2.measured_ms():.1f} ms, still running at return: {running_fwd} / {running_bwd}, wall {time.perf_counter() - t0:.2f} s")
    assert running_fwd and running_bwd
    so.assert_same_bits(snaps_fwd, want_fwd, "attention forward")
    so.assert_same_bits(snaps_bwd, want_bwd, "attention backward")
    assert plan.status() == 0
