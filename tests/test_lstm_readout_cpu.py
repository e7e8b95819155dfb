"""No GPU: the host side of the LSTM's pooled readout -- the new C ABI symbol (csn_lstm_plan_set_readout), the refusals of
the modules and the CLIs, the order in which a call arms its plan, and the numpy restatement of
tests/lstm_readout_reference.py held against torch's own mean and max (ties and empty rows included) and against the bf16
oracle for the premise of the GPU tie fixture."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

import bilstm_dropout_stream_cases  # noqa: F401  (joins the stream-order setter table on import, like the cases below)
import lstm_readout_reference as rref
import lstm_readout_stream_cases as stream_cases
from cerebralsignalnetworks_amd import cabi, lstm_model
from cerebralsignalnetworks_amd.lstm_model import BiLSTM, HipLSTM, LSTM, LSTMModel, Model
from oracle import lstm as oracle_lstm

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---- the symbol ---------------------------------------------------------------------------------------------------------
def test_symbol_is_declared_bound_and_checked():
    header = open(os.path.join(ROOT, "include", "csn_hip.h")).read()
    assert re.search(r"int\s+csn_lstm_plan_set_readout\(csnLstmPlan\*\s*\w+,\s*int\s+\w+\);", header)
    for name, value in (("LAST", 0), ("MEAN", 1), ("MAX", 2)):
        assert re.search(rf"#define\s+CSN_READOUT_{name}\s+{value}\b", header)
        assert getattr(cabi, f"READOUT_{name}") == value == cabi.READOUTS[name.lower()]
    listed = header[header.index("A symbol added beside the existing ones"):header.index("#define CSN_ABI_VERSION")]
    assert "csn_lstm_plan_set_readout" in listed
    assert re.search(r"#define\s+CSN_ABI_VERSION\s+6\b", header)
    assert "under CSN_READOUT_LAST h_n[L-1] == y_last" in header
    assert cabi.SIGNATURES["csn_lstm_plan_set_readout"] == (ctypes.c_int, [ctypes.c_void_p, ctypes.c_int])
    assert "set_readout" in vars(cabi.LstmPlan)
    lib = cabi.load()
    assert lib.csn_abi_version() == 6 == cabi.ABI_VERSION          # an added symbol does not bump it
    fn = lib.csn_lstm_plan_set_readout
    for mode in (0, 1, 2, 7):
        assert fn(None, mode) == 1 and b"null plan" in lib.csn_last_error()
    # the checks that need a plan run where one can be created (and always in tests/test_gpu_lstm_readout.py)
    d = cabi.LstmDesc(3, 5, 8, 32, 1, cabi.CSN_BF16)
    for flags in (0, 1, 1 | cabi.LSTM_STATE | cabi.LSTM_REVERSE | cabi.LSTM_DROPOUT, cabi.LSTM_RESIDENT):
        handle = ctypes.c_void_p()
        if lib.csn_lstm_plan_create(ctypes.byref(d), flags, ctypes.byref(handle)) != 0:
            assert b"hipGetDevice" in lib.csn_last_error()
            continue
        try:
            check_set_readout_arguments(lib, handle)
        finally:
            lib.csn_lstm_plan_destroy(handle)


def check_set_readout_arguments(lib, handle):
    """csn_lstm_plan_set_readout on any plan: the three modes are taken, anything else is refused."""
    fn = lib.csn_lstm_plan_set_readout
    for mode in (1, 2, 0):
        assert fn(handle, mode) == 0
    for bad in (-1, 3, 2 ** 20):
        assert fn(handle, bad) == 1 and b"unknown mode" in lib.csn_last_error()


def test_readout_mode_of_the_binding():
    assert [cabi.readout_mode(m) for m in ("last", "mean", "max", 0, 1, 2)] == [0, 1, 2, 0, 1, 2]
    for bad in ("avg", "MEAN", 3, -1, None, True, 1.0):
        with pytest.raises(cabi.CsnError, match="readout"):
            cabi.readout_mode(bad)


def test_setter_is_in_the_stream_order_table():
    import stream_order as so
    import test_stream_order_cpu as table_checks
    assert so.PLAN_SETTERS["csn_lstm_plan_set_readout"]
    assert stream_cases.MODES == rref.MODES
    table_checks.test_plan_setters_table_names_exactly_the_setters_of_the_header()


# ---- refusals -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("bad", ["avg", "MEAN", "", None, 1])
def test_an_unknown_readout_is_refused_by_every_constructor(bad):
    for make in (lambda: HipLSTM(8, 32, 2, readout=bad), lambda: Model(8, 32, 2, 16, False, readout=bad),
                 lambda: Model(8, 32, 2, 16, False, bidirectional=True, readout=bad),
                 lambda: LSTMModel(8, 32, 2, 16, readout=bad)):
        with pytest.raises(ValueError, match="readout must be one of"):
            make()
    x = torch.zeros(2, 3, 8)
    for m in (LSTM(8, 32), BiLSTM(8, 32)):
        with pytest.raises(ValueError, match="readout must be one of"):
            m.pooled(x, readout=bad)


def test_pooled_takes_mean_or_max_and_the_constructors_keep_the_readout():
    x = torch.zeros(2, 3, 8)
    for m in (LSTM(8, 32), BiLSTM(8, 32)):
        with pytest.raises(ValueError, match="'mean' or 'max'"):
            m.pooled(x, readout="last")
        with pytest.raises(cabi.CsnError, match="GPU only"):
            m.pooled(x)                                   # (the default readout is "mean": past the checks, no CPU fallback)
    with pytest.raises(ValueError, match="all_steps"):
        LSTMModel(8, 32, 2, 16, number_of_classes=4, all_steps=True, readout="mean")
    assert LSTMModel(8, 32, 2, 16, number_of_classes=4, all_steps=True).lstm.readout == "last"
    assert HipLSTM(8, 32).readout == "last" == LSTM(8, 32).readout == Model(8, 32, 1, 16, False).lstm.readout
    for r in ("mean", "max"):
        assert HipLSTM(8, 32, readout=r).readout == r == Model(8, 32, 1, 16, False, readout=r).lstm.readout
        assert LSTMModel(8, 32, 2, 16, readout=r).lstm.readout == r
        # no parameter depends on it: checkpoints are unchanged
        a, b = Model(8, 32, 2, 16, True, readout=r), Model(8, 32, 2, 16, True)
        assert [(k, tuple(v.shape)) for k, v in a.state_dict().items()] == [(k, tuple(v.shape)) for k, v in b.state_dict().items()]
        a, b = Model(8, 32, 2, 16, True, bidirectional=True, readout=r), Model(8, 32, 2, 16, True, bidirectional=True)
        assert [(k, tuple(v.shape)) for k, v in a.state_dict().items()] == [(k, tuple(v.shape)) for k, v in b.state_dict().items()]


def test_the_clis_take_the_three_readouts_and_refuse_others(capsys):
    import LstmDistillFromDinoV2Train as train
    import LstmDistillation as dino
    parsers = [train.build_parser(), train.build_parser(train.SPAMPINATO), dino.build_parser()]
    # (LstmDistillFromDinoV2Eval.py and LstmDistillFromDinoV2TrainSpampinato.py parse with the first two)
    eval_src = open(os.path.join(ROOT, "LstmDistillFromDinoV2Eval.py")).read()
    assert "from LstmDistillFromDinoV2Train import build_parser" in eval_src and "readout=FLAGS.readout" in eval_src
    for p in parsers:
        assert p.parse_known_args([])[0].readout == "last"
        for r in ("last", "mean", "max"):
            assert p.parse_known_args(["--readout", r])[0].readout == r
        with pytest.raises(SystemExit):
            p.parse_known_args(["--readout", "avg"])
    assert "invalid choice: 'avg'" in capsys.readouterr().err
    for name in ("LstmDistillFromDinoV2Train.py", "LstmDistillation.py"):
        assert "readout=FLAGS.readout" in open(os.path.join(ROOT, name)).read(), name


# ---- a call arms its plan -------------------------------------------------------------------------------------------------
class _RecordingPlan:
    """Takes every setter of cabi.LstmPlan and the two calls, and writes down what it was asked, in order."""

    def __init__(self, state=True):
        self.state, self.log = state, []

    def __getattr__(self, name):
        if not name.startswith("set_") and name not in ("forward", "backward"):
            raise AttributeError(name)
        return lambda *a, **kw: self.log.append((name, a, kw))


def _readouts_before_calls(log):
    """For every forward / backward in the log: the argument of the last set_readout in front of it (None: none)."""
    out, seen = [], None
    for name, a, _ in log:
        if name == "set_readout":
            seen = a[0]
        elif name in ("forward", "backward"):
            out.append((name, seen))
            seen = None         # (sticky on the library's side, but a pooled plan carries its last user's: set again every time)
    return out


@pytest.mark.parametrize("readout", ["last", "mean", "max"])
def test_armed_sets_the_readout_in_front_of_every_forward_and_backward(readout):
    x = torch.zeros(4, 6, 8)
    call = lstm_model._Call(x, True, None, lengths=(6, 0, 2, 5), state_plan=True, readout=readout)
    assert call.readout == readout and lstm_model._Call(x, True, None).readout == "last"
    plan = _RecordingPlan()
    lstm_model._armed(plan, call, lambda: plan.forward("x"))
    lstm_model._armed(plan, call, lambda: plan.backward("dy"), grad=(None, False))
    assert _readouts_before_calls(plan.log) == [("forward", readout), ("backward", readout)]
    # a plan without CSN_LSTM_STATE takes no lengths, and still the readout
    plan = _RecordingPlan(state=False)
    lstm_model._armed(plan, lstm_model._Call(x, True, None, readout=readout), lambda: plan.forward("x"))
    assert _readouts_before_calls(plan.log) == [("forward", readout)] and "set_lengths" not in [n for n, _, _ in plan.log]
    with pytest.raises(ValueError, match="readout must be one of"):
        lstm_model._Call(x, True, None, readout="avg")


@pytest.mark.parametrize("readout", ["last", "mean", "max"])
def test_armed_pools_on_the_top_layer_plans_of_a_bidirectional_stack_only(readout):
    L, H = 3, 32
    call = lstm_model._Call(torch.zeros(4, 6, 8), True, None, bi=(L, H), readout=readout)
    for k in range(2 * L):
        plan = _RecordingPlan()
        lstm_model._armed(plan, call, lambda: plan.forward("x"), k=k)
        lstm_model._armed(plan, call, lambda: plan.backward("dy"), grad=(None, False), k=k)
        want = readout if k // 2 == L - 1 else "last"
        assert _readouts_before_calls(plan.log) == [("forward", want), ("backward", want)], k


def test_the_autograd_function_arms_the_plan_it_checked_out(monkeypatch):
    """HipLSTM.forward through _LstmFunction with a recording plan in place of a checked-out one: the readout of the module
    reaches the plan before the forward and, from the call kept on ctx, before the backward."""
    m = HipLSTM(8, 32, 2, readout="max")
    B, T = 3, 5
    plan = _RecordingPlan(state=False)
    plan.desc = cabi.LstmDesc(B, T, 8, 32, 2, cabi.CSN_BF16)
    plan.busy = False

    def forward(x, *groups, **kw):
        plan.log.append(("forward", (), kw))
        return torch.zeros(B, 32), None
    plan.forward = forward
    monkeypatch.setattr(m, "_checkout", lambda *a, **kw: plan)
    x = torch.zeros(B, T, 8)
    x.is_cuda                                       # (a CPU tensor: the entry point refuses it, the Function below does not)
    params = m._flat_params()
    call = lstm_model._Call(x, True, None, readout=m.readout)
    y = lstm_model._LstmFunction.apply(x, None, None, m, call, 2, *params)[0]
    y.sum().backward()
    assert _readouts_before_calls(plan.log) == [("forward", "max"), ("backward", "max")]


# ---- the restatement against torch ----------------------------------------------------------------------------------------
def _tied_values(B, T, H, seed):
    """Values on a coarse grid, so that most columns attain their maximum more than once."""
    g = torch.Generator().manual_seed(seed)
    return (torch.randint(-1, 2, (B, T, H), generator=g).float() / 4).numpy()


@pytest.mark.parametrize("lengths", [None, (9, 0, 1, 8, 4)], ids=str)
def test_restatement_is_torch_mean_and_max_with_the_first_maximum(lengths):
    B, T, H = 5, 9, 16
    v = _tied_values(B, T, H, 1)
    dy = torch.randn(B, H, generator=torch.Generator().manual_seed(2))
    n = rref.rows(lengths, B, T)
    assert rref.tied_columns(v, lengths)[[b for b in range(B) if n[b] >= 4]].mean() > 0.5      # (the rows long enough to tie)
    for mode in rref.MODES:
        got, G = rref.pooled(v, lengths, mode), rref.expand(dy.numpy(), v, lengths, mode)
        assert got.dtype == np.float32 == G.dtype
        for b in range(B):
            if n[b] == 0:
                assert not got[b].any() and not G[b].any()
                continue
            vb = torch.from_numpy(v[b, :n[b]]).clone().requires_grad_(True)
            if mode == "mean":
                want = vb.double().mean(0).float()
                (vb.sum(0) / n[b]).backward(dy[b])      # torch's backward of this expression: the float32 division dy / n
            else:
                want, idx = vb.max(0)
                want.backward(dy[b])
                assert np.array_equal(rref.first_max(v, lengths)[b], idx.numpy())
            assert np.array_equal(got[b], want.detach().numpy()), (mode, b)
            assert np.array_equal(G[b, :n[b]], vb.grad.numpy()), (mode, b)
            assert not G[b, n[b]:].any()


def test_restatement_lets_a_nan_win_and_takes_the_first():
    v = _tied_values(2, 6, 4, 3)
    v[0, 2, 1] = v[0, 4, 1] = np.nan
    got, at = rref.pooled(v, None, "max"), rref.first_max(v, None)
    want, idx = torch.from_numpy(v).max(1)
    assert np.isnan(got[0, 1]) and at[0, 1] == 2 == int(idx[0, 1])
    assert np.array_equal(np.isnan(got), torch.isnan(want).numpy())
    G = rref.expand(np.ones((2, 4), np.float32), v, None, "max")
    assert G[0, 2, 1] == 1 and G[0, :, 1].sum() == 1


def test_mean_bound_covers_the_rounding_of_the_float64_mean():
    g = np.random.default_rng(4)
    v = g.uniform(-1, 1, (3, 37, 8)).astype(np.float32)
    exact = v.astype(np.float64).mean(axis=1)
    got = rref.pooled(v, None, "mean")
    assert (np.abs(got - exact) <= rref.mean_bound(got, 37)).all()
    assert (rref.mean_bound(got, 37) <= 2.0 ** -23).all()       # |mean| < 1: at most the ulp of [0.5, 1), 2^-24, plus T 2^-50


# ---- the premise of the GPU tie fixture -----------------------------------------------------------------------------------
def test_saturated_fixture_ties_in_the_bf16_oracle():
    B, T, I, H = 5, 24, 8, 32
    params = rref.saturated_params(I, H)
    x = np.random.default_rng(6).standard_normal((B, T, I)).astype(np.float32)
    y, _ = oracle_lstm.lstm_forward_bf16(x, params, 1)
    y = y.astype(np.float32)
    assert (y[:, 10:] == 1.0).all() and (y[:, 0] < 1.0).all()      # exactly bf16 1.0 from the tenth step on at the latest
    assert rref.tied_columns(y).mean() >= 0.5
    first = rref.first_max(y)
    assert (first > 0).all() and (first <= 10).all()
    # the rows walked backwards (a CSN_LSTM_REVERSE plan on the same x): the maximum is then reached at the END of the
    # caller's time axis and held to its beginning, so the first caller time is step 0 of the caller = the last of the recurrence
    yr, _ = oracle_lstm.lstm_forward_bf16(x[:, ::-1], params, 1)
    yr = yr.astype(np.float32)[:, ::-1]
    assert rref.tied_columns(yr).mean() >= 0.5 and (rref.first_max(yr) == 0).all()
