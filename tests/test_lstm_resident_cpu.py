"""No GPU: the host side of CSN_LSTM_RESIDENT (the CU-resident recurrence, path 5) -- the flag in the header and the
binding, the workspace of a resident plan (that of the same descriptor on path 0, nothing added), the refusal of
H > 128, the `resident` keyword of the plan and the modules, unchanged state-dict keys, and --resident_lstm on the CLIs."""
import ctypes
import inspect
import os
import re

import pytest
import torch

from cerebralsignalnetworks_amd import cabi, BiLSTM, LSTM, LSTMModel, Model
from cerebralsignalnetworks_amd.lstm_model import HipLSTM

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BITS = (0, cabi.LSTM_STATE, cabi.LSTM_DROPOUT, cabi.LSTM_REVERSE, cabi.LSTM_STATE | cabi.LSTM_DROPOUT | cabi.LSTM_REVERSE)


def test_flag_is_declared_and_bound_without_an_abi_bump():
    header = open(os.path.join(ROOT, "include", "csn_hip.h")).read()
    assert re.search(r"#define\s+CSN_LSTM_RESIDENT\s+0x800\b", header) and cabi.LSTM_RESIDENT == 0x800
    assert re.search(r"#define\s+CSN_ABI_VERSION\s+6\b", header)
    assert cabi.load().csn_abi_version() == 6 == cabi.ABI_VERSION
    assert not cabi.LSTM_RESIDENT & (cabi.LSTM_STATE | cabi.LSTM_DROPOUT | cabi.LSTM_REVERSE | 0xff)


@pytest.mark.parametrize("dtype", [cabi.CSN_BF16, cabi.CSN_F32], ids=["bf16", "f32"])
@pytest.mark.parametrize("training", [0, 1])
def test_workspace_is_that_of_the_plan_without_the_bit(dtype, training):
    """LstmDesc(16, 460, 96, 96, 2): without the bit the plan is path 0 (H % 128 != 0), so the sizes are equal."""
    ws = cabi.load().csn_lstm_workspace_bytes
    d = cabi.LstmDesc(16, 460, 96, 96, 2, dtype)
    for bits in BITS:
        plain = ws(ctypes.byref(d), training | bits)
        assert ws(ctypes.byref(d), training | bits | cabi.LSTM_RESIDENT) == plain > 0, (training, bits)


@pytest.mark.parametrize("dtype", [cabi.CSN_BF16, cabi.CSN_F32], ids=["bf16", "f32"])
def test_resident_workspace_at_128_is_the_per_step_cells(dtype, monkeypatch):
    """H = 128: with the bit the layout is the one CSN_CELL_V1=1 selects (path 0), whatever the plain plan would take."""
    ws = cabi.load().csn_lstm_workspace_bytes
    d = cabi.LstmDesc(16, 460, 128, 128, 4, dtype)
    got = ws(ctypes.byref(d), 1 | cabi.LSTM_RESIDENT)
    monkeypatch.setenv("CSN_CELL_V1", "1")
    assert got == ws(ctypes.byref(d), 1) > 0
    assert ws(ctypes.byref(d), 1 | cabi.LSTM_RESIDENT) == got


@pytest.mark.parametrize("H", [160, 256])
@pytest.mark.parametrize("dtype", [cabi.CSN_BF16, cabi.CSN_F32], ids=["bf16", "f32"])
def test_wider_layers_are_refused_with_the_bit_only(H, dtype):
    lib = cabi.load()
    d = cabi.LstmDesc(16, 20, 96, H, 2, dtype)
    for bits in BITS:
        assert lib.csn_lstm_workspace_bytes(ctypes.byref(d), 1 | bits) > 0
        assert lib.csn_lstm_workspace_bytes(ctypes.byref(d), 1 | bits | cabi.LSTM_RESIDENT) == 0
        msg = lib.csn_last_error()
        assert b"CSN_LSTM_RESIDENT" in msg and b"128" in msg, msg
    # plan creation refuses before it asks for a device: CSN_ERR_UNSUPPORTED, the flag and the limit in the message
    handle = ctypes.c_void_p()
    assert lib.csn_lstm_plan_create(ctypes.byref(d), 1 | cabi.LSTM_RESIDENT, ctypes.byref(handle)) == 3
    msg = lib.csn_last_error()
    assert b"CSN_LSTM_RESIDENT" in msg and b"128" in msg and not handle.value
    for ok in (32, 64, 96, 128):
        d = cabi.LstmDesc(16, 20, 96, ok, 2, dtype)
        assert lib.csn_lstm_workspace_bytes(ctypes.byref(d), 1 | cabi.LSTM_RESIDENT) > 0


def test_binding_passes_resident_and_keys_it():
    sig = inspect.signature(cabi.LstmPlan.__init__)
    assert sig.parameters["resident"].default is False
    plan = object.__new__(cabi.LstmPlan)
    plan.desc, plan.training, plan.state, plan.dropout, plan.reverse = cabi.LstmDesc(2, 3, 8, 32, 1, 1), True, True, False, False
    plan.resident = False
    plain = plan.key()
    plan.resident = True
    assert plan.key() != plain and plan.key()[:len(plain)] == plain
    plan._plan = None       # (never created: nothing to destroy)
    assert "5" in cabi.LstmPlan.path.__doc__


def test_modules_take_resident_up_to_128():
    for cls in (HipLSTM, LSTM, BiLSTM):
        assert inspect.signature(cls.__init__).parameters["resident"].default is False
        assert cls(24, 96, 2, resident=True).resident is True and cls(24, 96, 2).resident is False
        assert cls(24, 128, 1, resident=True).resident is True
        with pytest.raises(ValueError, match="resident=True takes hidden_size <= 128"):
            cls(24, 256, 2, resident=True)
        cls(24, 256, 2)
    assert Model(24, 96, 2, 16, True, resident=True).lstm.resident and not Model(24, 96, 2, 16, True).lstm.resident
    assert Model(24, 96, 2, 16, bidirectional=True, resident=True).lstm.resident
    assert LSTMModel(24, 96, 2, 16, resident=True).lstm.resident and not LSTMModel(24, 96, 2, 16).lstm.resident
    for make in (lambda: Model(24, 256, 2, 16, True, resident=True), lambda: LSTMModel(24, 256, 2, 16, resident=True),
                 lambda: Model(24, 256, 2, 16, bidirectional=True, resident=True)):
        with pytest.raises(ValueError, match="resident=True"):
            make()


def test_resident_enters_the_plan_pool_key_and_reaches_the_plan(monkeypatch):
    made = []

    class _Plan:
        busy = False

        def __init__(self, *args, **kw):
            made.append(kw)

    monkeypatch.setattr(cabi, "LstmPlan", _Plan)
    for cls, args in ((HipLSTM, (4, 9, "cpu", True)), (LSTM, (4, 9, "cpu", True)), (BiLSTM, (4, 9, 24, "cpu", True, True))):
        on, off = cls(24, 96, 1, resident=True), cls(24, 96, 1)
        on._checkout(*args)
        off._checkout(*args)
        assert made[-2]["resident"] is True and made[-1]["resident"] is False, cls
        (k_on,), (k_off,) = on._plans, off._plans
        assert k_on != k_off and k_on[:len(k_off)] == k_off, cls


def test_state_dict_keys_are_unchanged():
    torch.manual_seed(0)
    plain, res = Model(24, 96, 2, 16, True), Model(24, 96, 2, 16, True, resident=True)
    assert list(plain.state_dict()) == list(res.state_dict())
    res.load_state_dict(plain.state_dict(), strict=True)
    assert list(BiLSTM(24, 96, 2).state_dict()) == list(BiLSTM(24, 96, 2, resident=True).state_dict())
    assert list(LSTM(24, 96, 2).state_dict()) == list(LSTM(24, 96, 2, resident=True).state_dict())


def test_every_cli_that_builds_a_model_has_the_switch_off_by_default():
    """(DiscoverChannels.py builds no model: it has no such switch)"""
    import LstmDistillFromDinoV2Eval as evaluate_cli
    import LstmDistillFromDinoV2Train as train
    import LstmDistillFromDinoV2TrainSpampinato as spamp
    import LstmDistillation as dino_cli
    parsers = [train.build_parser(train.PERILS), train.build_parser(train.SPAMPINATO), spamp._loop.build_parser(spamp._loop.SPAMPINATO),
               evaluate_cli.build_parser(), dino_cli.build_parser()]
    for p in parsers:
        assert p.parse_args([]).resident_lstm is False
        assert p.parse_args(["--resident_lstm"]).resident_lstm is True
        assert "--resident_lstm" in p.format_help()
