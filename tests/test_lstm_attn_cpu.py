"""No GPU: the host side of the LSTM's attention readout -- the new C ABI symbol (csn_lstm_plan_set_attention) and its
refusals, the binding, the modules' refusals and state_dict keys, the order in which a call arms its plan, and the numpy
restatement of tests/lstm_attn_reference.py held against torch's float64 autograd of softmax(scale (y @ q), masked) . y."""
import ctypes
import math
import os
import re

import numpy as np
import pytest
import torch

import bilstm_dropout_stream_cases  # noqa: F401  (these join the stream-order setter table on import)
import lstm_attn_reference as aref
import lstm_attn_stream_cases  # noqa: F401
import lstm_readout_reference as rref
import lstm_readout_stream_cases  # noqa: F401
from cerebralsignalnetworks_amd import cabi, lstm_model
from cerebralsignalnetworks_amd.lstm_model import BiLSTM, HipLSTM, LSTM, LSTMModel, Model

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SOME = ctypes.c_void_p(4096)      # a non-null pointer: the setter is host only and reads nothing through it


# ---- the symbol ---------------------------------------------------------------------------------------------------------
def test_symbol_is_declared_bound_and_checked():
    header = open(os.path.join(ROOT, "include", "csn_hip.h")).read()
    assert re.search(r"int\s+csn_lstm_plan_set_attention\(csnLstmPlan\*\s*\w+,\s*const\s+float\*\s*\w+,\s*float\s+\w+,\s*float\*\s*\w+,"
                     r"\s*float\*\s*\w+,\s*float\*\s*\w+\);", header)
    listed = header[header.index("A symbol added beside the existing ones"):header.index("#define CSN_ABI_VERSION")]
    assert "csn_lstm_plan_set_attention" in listed
    assert re.search(r"#define\s+CSN_ABI_VERSION\s+6\b", header)
    assert not re.search(r"#define\s+CSN_READOUT_\w+\s+3\b", header)          # no fourth mode: attention has its own setter
    vp = ctypes.c_void_p
    assert cabi.SIGNATURES["csn_lstm_plan_set_attention"] == (ctypes.c_int, [vp, vp, ctypes.c_float, vp, vp, vp])
    assert "set_attention" in vars(cabi.LstmPlan)
    lib = cabi.load()
    assert lib.csn_abi_version() == 6 == cabi.ABI_VERSION          # an added symbol does not bump it
    fn = lib.csn_lstm_plan_set_attention
    for args in ((None, 0.0, None, None, None), (SOME, 1.0, None, None, None), (SOME, 0.5, SOME, SOME, SOME)):
        assert fn(None, *args) == 1 and b"null plan" in lib.csn_last_error()
    # the checks that need a plan run where one can be created (and always in tests/test_gpu_lstm_attn.py)
    d = cabi.LstmDesc(3, 5, 8, 32, 1, cabi.CSN_BF16)
    for flags in (0, 1, 1 | cabi.LSTM_STATE | cabi.LSTM_REVERSE | cabi.LSTM_DROPOUT, cabi.LSTM_RESIDENT):
        handle = ctypes.c_void_p()
        if lib.csn_lstm_plan_create(ctypes.byref(d), flags, ctypes.byref(handle)) != 0:
            assert b"hipGetDevice" in lib.csn_last_error()
            continue
        try:
            check_set_attention_arguments(lib, handle)
        finally:
            lib.csn_lstm_plan_destroy(handle)


def check_set_attention_arguments(lib, handle):
    """csn_lstm_plan_set_attention on any plan (nothing is launched): on and off are taken; a non-finite scale and dq,
    attn_out or dscore_out without q are refused.  Leaves attention off."""
    fn = lib.csn_lstm_plan_set_attention
    assert fn(handle, SOME, 0.25, None, None, None) == 0
    assert fn(handle, SOME, -1.0, SOME, SOME, SOME) == 0
    for bad in (float("nan"), float("inf"), -float("inf")):
        assert fn(handle, SOME, bad, None, None, None) == 1 and b"scale" in lib.csn_last_error()
        assert fn(handle, None, bad, None, None, None) == 1 and b"scale" in lib.csn_last_error()
    for args in ((SOME, None, None), (None, SOME, None), (None, None, SOME), (SOME, SOME, SOME)):
        assert fn(handle, None, 1.0, *args) == 1 and b"without q" in lib.csn_last_error()
    assert fn(handle, None, 0.0, None, None, None) == 0


def test_the_readout_setter_and_the_binding_still_refuse_a_fourth_mode():
    lib = cabi.load()
    assert lib.csn_lstm_plan_set_readout(None, 3) == 1
    with pytest.raises(cabi.CsnError, match="readout"):
        cabi.readout_mode(3)
    with pytest.raises(cabi.CsnError, match="readout"):
        cabi.readout_mode("attn")
    assert cabi.READOUTS == {"last": 0, "mean": 1, "max": 2}
    d = cabi.LstmDesc(3, 5, 8, 32, 1, cabi.CSN_BF16)
    handle = ctypes.c_void_p()
    if lib.csn_lstm_plan_create(ctypes.byref(d), 1, ctypes.byref(handle)) == 0:
        try:
            assert lib.csn_lstm_plan_set_readout(handle, 3) == 1 and b"unknown mode" in lib.csn_last_error()
        finally:
            lib.csn_lstm_plan_destroy(handle)


def test_setter_is_in_the_stream_order_table():
    import stream_order as so
    import test_stream_order_cpu as table_checks
    assert so.PLAN_SETTERS["csn_lstm_plan_set_attention"]
    table_checks.test_plan_setters_table_names_exactly_the_setters_of_the_header()


# ---- modules --------------------------------------------------------------------------------------------------------------
def _keys(m):
    return [(k, tuple(v.shape)) for k, v in m.state_dict().items()]


def test_state_dict_keys_appear_only_on_opt_in():
    H = 32
    plain = _keys(HipLSTM(8, H, 2))
    assert _keys(HipLSTM(8, H, 2, readout="mean")) == plain == _keys(LSTM(8, H, 2))
    assert _keys(HipLSTM(8, H, 2, readout="attn")) == plain + [("attn_query", (H,))] == _keys(LSTM(8, H, 2, attention=True))
    assert _keys(HipLSTM(8, H, 2, attention=True)) == plain + [("attn_query", (H,))]
    bi = _keys(BiLSTM(8, H, 2))
    assert _keys(BiLSTM(8, H, 2, attention=True)) == bi + [("attn_query", (H,)), ("attn_query_reverse", (H,))]
    for kw in (dict(), dict(bidirectional=True)):
        base = _keys(Model(8, H, 2, 16, True, **kw))
        got = _keys(Model(8, H, 2, 16, True, readout="attn", **kw))
        extra = [("lstm.attn_query", (H,))] + ([("lstm.attn_query_reverse", (H,))] if kw else [])
        assert sorted(got) == sorted(base + extra) and all(k in got for k in base)
    assert sorted(_keys(LSTMModel(8, H, 2, 16, readout="attn"))) == sorted(_keys(LSTMModel(8, H, 2, 16)) + [("lstm.attn_query", (H,))])
    # zeros at the start: mean pooling
    for m in (HipLSTM(8, H, readout="attn"), BiLSTM(8, H, attention=True)):
        assert all(not p.any() and p.requires_grad for n, p in m.named_parameters() if n.startswith("attn_query"))
    assert Model(8, H, 1, 16, False, readout="attn").lstm.readout == "attn"


def test_module_refusals():
    x = torch.zeros(2, 3, 8)
    for m, name in ((LSTM(8, 32), "LSTM"), (BiLSTM(8, 32), "BiLSTM")):
        with pytest.raises(ValueError, match="built without the attention parameter"):
            m.pooled(x, readout="attn")
        with pytest.raises(ValueError, match="return_weights"):
            m.pooled(x, readout="mean", return_weights=True)
        with pytest.raises(ValueError, match="'mean' or 'max'"):
            m.pooled(x, readout="last")
    for m in (LSTM(8, 32, attention=True), BiLSTM(8, 32, attention=True)):
        with pytest.raises(cabi.CsnError, match="GPU only"):
            m.pooled(x, readout="attn", return_weights=True)       # (past the checks: no CPU fallback)
    with pytest.raises(ValueError, match="return_weights"):
        HipLSTM(8, 32)(x, return_weights=True)
    with pytest.raises(cabi.CsnError, match="GPU only"):
        HipLSTM(8, 32, readout="attn")(x, return_weights=True)
    with pytest.raises(ValueError, match="all_steps"):
        LSTMModel(8, 32, 2, 16, number_of_classes=4, all_steps=True, readout="attn")
    with pytest.raises(ValueError, match="one query per direction"):
        lstm_model._Call(x, True, None, readout="attn")
    with pytest.raises(ValueError, match="one query per direction"):
        lstm_model._Call(x, True, None, readout="attn", attn=[torch.zeros(32)], bi=(2, 32))
    with pytest.raises(ValueError, match="readout must be one of"):
        HipLSTM(8, 32, readout="attention")


def test_the_clis_take_the_attention_readout():
    import LstmDistillFromDinoV2Train as train
    import LstmDistillation as dino
    for p in (train.build_parser(), train.build_parser(train.SPAMPINATO), dino.build_parser()):
        assert p.parse_known_args(["--readout", "attn"])[0].readout == "attn"
        assert p.parse_known_args([])[0].readout == "last"


# ---- a call arms its plan -------------------------------------------------------------------------------------------------
class _RecordingPlan:
    """Takes every setter of cabi.LstmPlan and the two calls, and writes down what it was asked, in order."""

    def __init__(self, state=True):
        self.state, self.log = state, []

    def __getattr__(self, name):
        if not name.startswith("set_") and name not in ("forward", "backward"):
            raise AttributeError(name)
        return lambda *a, **kw: self.log.append((name, a, kw))


def _attention_before_calls(log):
    """For every forward / backward in the log: (readout, attention arguments) last set in front of it (None: not set)."""
    out, readout, attn = [], None, None
    for name, a, _ in log:
        if name == "set_readout":
            readout = a[0]
        elif name == "set_attention":
            attn = a
        elif name in ("forward", "backward"):
            out.append((name, readout, attn))
            readout = attn = None      # (sticky on the library's side, but a pooled plan carries its last user's)
    return out


def test_armed_sets_attention_in_front_of_every_forward_and_backward():
    x, q, dq = torch.zeros(4, 6, 8), torch.zeros(32), torch.ones(32)
    call = lstm_model._Call(x, True, None, lengths=(6, 0, 2, 5), state_plan=True, readout="attn", attn=[q])
    plan = _RecordingPlan()
    lstm_model._armed(plan, call, lambda: plan.forward("x"))
    lstm_model._armed(plan, call, lambda: plan.backward("dy"), grad=(None, False), dq=dq)
    (f, fr, fa), (b, br, ba) = _attention_before_calls(plan.log)
    assert (f, fr, b, br) == ("forward", "last", "backward", "last")
    assert fa[0] is q and fa[2] is None and fa[3] is None and ba[0] is q and ba[2] is dq
    # with the weights asked for, their tensor goes to both calls
    call.attn_out = [torch.zeros(4, 6)]
    lstm_model._armed(plan, call, lambda: plan.backward("dy"), grad=(None, False), dq=dq)
    assert _attention_before_calls(plan.log)[-1][2][3] is call.attn_out[0]
    # every other call turns it off on the plan it was handed
    for readout in ("last", "mean", "max"):
        plan = _RecordingPlan()
        other = lstm_model._Call(x, True, None, readout=readout)
        lstm_model._armed(plan, other, lambda: plan.forward("x"))
        lstm_model._armed(plan, other, lambda: plan.backward("dy"), grad=(None, False))
        assert _attention_before_calls(plan.log) == [("forward", readout, ()), ("backward", readout, ())]


def test_armed_attends_on_the_top_layer_plans_of_a_bidirectional_stack_only():
    L, H = 3, 32
    qs = [torch.zeros(H), torch.ones(H)]
    call = lstm_model._Call(torch.zeros(4, 6, 8), True, None, bi=(L, H), readout="attn", attn=qs)
    for k in range(2 * L):
        plan = _RecordingPlan()
        lstm_model._armed(plan, call, lambda: plan.forward("x"), k=k)
        lstm_model._armed(plan, call, lambda: plan.backward("dy"), grad=(None, False), k=k, dq="dq" if k // 2 == L - 1 else None)
        seen = _attention_before_calls(plan.log)
        assert [s[1] for s in seen] == ["last", "last"]
        if k // 2 == L - 1:
            assert seen[0][2][0] is qs[k % 2] and seen[1][2][0] is qs[k % 2] and seen[1][2][2] == "dq"
        else:
            assert seen[0][2] == () == seen[1][2], k


def test_the_autograd_function_takes_the_query_and_returns_its_gradient(monkeypatch):
    """HipLSTM(readout="attn").forward through _LstmFunction with a recording plan: the query reaches the plan before both
    calls, and what the backward wrote as dq comes back as attn_query.grad."""
    m = HipLSTM(8, 32, 2, readout="attn")
    B, T = 3, 5
    plan = _RecordingPlan(state=False)
    plan.desc = cabi.LstmDesc(B, T, 8, 32, 2, cabi.CSN_BF16)
    plan.busy = False
    seen = {}

    def forward(x, *groups, **kw):
        plan.log.append(("forward", (), kw))
        return torch.zeros(B, 32), None

    def backward(dy_last, dy_all, grads, **kw):
        plan.log.append(("backward", (), kw))
        for group in grads:
            for g in group:
                g.zero_()
        seen["dq"].fill_(7.0)

    def set_attention(*a):
        plan.log.append(("set_attention", a, {}))
        if len(a) > 2 and a[2] is not None:
            seen["dq"] = a[2]
    plan.forward, plan.backward, plan.set_attention = forward, backward, set_attention
    monkeypatch.setattr(m, "_checkout", lambda *a, **kw: plan)
    x = torch.zeros(B, T, 8)
    params = m._flat_params() + [m.attn_query]
    call = lstm_model._Call(x, True, None, readout="attn", attn=[m.attn_query])
    y = lstm_model._LstmFunction.apply(x, None, None, m, call, 2, *params)[0]
    y.sum().backward()
    (f, fr, fa), (b, br, ba) = _attention_before_calls(plan.log)
    assert fa[0] is m.attn_query and ba[0] is m.attn_query and ba[2] is seen["dq"]
    assert bool((m.attn_query.grad == 7.0).all()) and m.weight_hh_l1.grad is not None


# ---- the restatement against torch ----------------------------------------------------------------------------------------
def _values(B, T, H, seed):
    g = np.random.default_rng(seed)
    return (g.uniform(-0.99, 0.99, (B, T, H)).astype(np.float32), g.uniform(-4, 4, H).astype(np.float32),
            g.standard_normal((B, H)).astype(np.float32))


def _torch_attention(v, q, scale, n, dy):
    """float64 autograd of softmax(scale (y @ q) over t < n) . y for one row -> (value, weights, d/dy, d/dq)."""
    y = torch.from_numpy(v[:n]).double().requires_grad_(True)
    qq = torch.from_numpy(q).double().requires_grad_(True)
    a = torch.softmax(float(np.float32(scale)) * (y @ qq), dim=0)
    out = a @ y
    out.backward(torch.from_numpy(dy).double())
    return out.detach().numpy(), a.detach().numpy(), y.grad.numpy(), qq.grad.numpy()


@pytest.mark.parametrize("lengths", [None, (9, 0, 1, 8, 4)], ids=str)
def test_restatement_is_torch_float64_attention(lengths):
    B, T, H = 5, 9, 16
    v, q, dy = _values(B, T, H, 1)
    scale = H ** -0.5
    n = rref.rows(lengths, B, T)
    y64, a64 = aref.forward(v, q, scale, lengths)
    w64, g64 = aref.dscore(v, q, scale, lengths, dy)
    a32, w32 = a64.astype(np.float32), w64.astype(np.float32)
    G = aref.expand(a32, w32, q, dy, lengths)
    assert G.dtype == np.float32 and y64.dtype == np.float64
    dq_t = np.zeros(H)
    for b in range(B):
        if n[b] == 0:
            assert not y64[b].any() and not a64[b].any() and not w64[b].any() and not G[b].any()
            continue
        out, a, dy_dv, dq_b = _torch_attention(v[b], q, scale, n[b], dy[b])
        dq_t += dq_b
        assert np.abs(y64[b] - out).max() <= 2.0 ** -48 and np.abs(a64[b, :n[b]] - a).max() <= 2.0 ** -48
        assert not a64[b, n[b]:].any() and not G[b, n[b]:].any() and abs(a64[b].sum() - 1) <= 2.0 ** -48
        # G against torch's gradient: float32 rounding of its three operations (a32 and w32 are themselves rounded: one
        # more relative 2^-24 on each product), |a dy| + |w q| at most their sum
        size = np.abs(a32[b, :n[b], None] * dy[b][None, :]) + np.abs(w32[b, :n[b], None] * q[None, :])
        assert (np.abs(G[b, :n[b]] - dy_dv) <= 4 * 2.0 ** -24 * size + 2.0 ** -60).all()
    dq = aref.dq(w32, v, lengths)
    size = np.einsum("bt,bth->h", np.abs(w32).astype(np.float64), np.abs(v).astype(np.float64))
    assert (np.abs(dq - dq_t) <= 2.0 ** -24 * size + 2.0 ** -48).all()          # (w32 is w64 rounded to float32)
    assert np.abs(dq_t).max() > 1e-3                                              # the comparison is not of zeros


def test_a_zero_query_is_the_mean():
    B, T, H = 5, 9, 16
    lengths = (9, 0, 1, 8, 4)
    v, _, dy = _values(B, T, H, 2)
    y64, a64 = aref.forward(v, np.zeros(H, np.float32), H ** -0.5, lengths)
    mean = rref.pooled(v, lengths, "mean")
    assert (np.abs(mean - y64) <= aref.value_bound(mean)).all()
    for b, n in enumerate(lengths):
        assert np.array_equal(a64[b, :n], np.full(n, 1.0 / max(n, 1))) and not a64[b, n:].any()
    w64, _ = aref.dscore(v, np.zeros(H, np.float32), H ** -0.5, lengths, dy)
    G = aref.expand(a64.astype(np.float32), w64.astype(np.float32), np.zeros(H, np.float32), dy, lengths)
    # (with q = 0 the score term vanishes from G: what is left is fl32(fl32(1 / n) dy), the mean's dy / n within an ulp)
    assert (np.abs(G - rref.expand(dy, v, lengths, "mean")) <= aref.ulp32(G)).all()


def test_a_saturated_softmax_is_one_hot_and_finite():
    B, T, H = 4, 9, 16
    v, _, dy = _values(B, T, H, 3)
    q = (3000.0 * np.where(np.arange(H) % 2 == 0, 1.0, -1.0)).astype(np.float32)
    y64, a64 = aref.forward(v, q, H ** -0.5, None)
    w64, g64 = aref.dscore(v, q, H ** -0.5, None, dy)
    assert np.isfinite(y64).all() and np.isfinite(a64).all() and np.isfinite(w64).all()
    z = H ** -0.5 * (v.astype(np.float64) @ q.astype(np.float64))
    gaps = np.sort(z, axis=1)
    assert ((gaps[:, -1] - gaps[:, -2]) > 745).any()                  # past the reach of float64's exp
    for b in range(B):
        if gaps[b, -1] - gaps[b, -2] > 745:
            assert np.array_equal(a64[b], (np.arange(T) == z[b].argmax()).astype(np.float64))
            assert np.array_equal(y64[b], v[b, z[b].argmax()].astype(np.float64)) and not w64[b].any()


def test_bounds_have_the_sizes_the_derivation_gives():
    y = np.array([0.75, -0.3, 0.0], np.float32)
    assert np.array_equal(aref.value_bound(y), np.spacing(np.abs(y)).astype(np.float64) + 2.0 ** -40)
    assert (aref.value_bound(y) <= 2.0 ** -24 + 2.0 ** -40).all()      # |y| < 1: at most the ulp of [0.5, 1)
    a = np.array([0.5, 1e-30], np.float32)
    assert aref.attn_bound(a)[0] == 2.0 ** -24 + 2.0 ** -41 and aref.attn_bound(a)[1] < 1e-36
    assert math.isclose(aref.dq_bound(np.float32(1.0), 5, 37, np.ones((5, 37))), 2.0 ** -23 + 5 * 37 * 2.0 ** -53 * 185)
    assert aref.dscore_bound(np.float32(0.5), 0.125, 8.0) == 2.0 ** -24 + 2.0 ** -40
