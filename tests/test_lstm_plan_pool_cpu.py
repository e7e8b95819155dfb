"""No GPU: the plan pool of HipLSTM / LSTM / BiLSTM (lstm_model._PlanPool behind ``_checkout``, ``_plans`` and
``all_plans()``), with cabi.LstmPlan replaced by a stand-in as in tests/test_lstm_resident_cpu.py: reuse of an idle plan, a
second plan beside a busy one, the eviction rule (idle plans of OTHER keys, oldest first, while at least MAX_IDLE_PLANS of
them are idle; never a busy plan, never one of the requested key) and the key tuples, written out as literals."""
import pytest
import torch

from cerebralsignalnetworks_amd import cabi, BiLSTM, LSTM
from cerebralsignalnetworks_amd.lstm_model import HipLSTM

BF16 = torch.bfloat16


class _Plan:
    def __init__(self, *args, **kw):
        self.args, self.kw, self.busy = args, kw, False


@pytest.fixture(autouse=True)
def _stand_in(monkeypatch):
    monkeypatch.setattr(cabi, "LstmPlan", _Plan)


def _checkout(m, B, training=True):
    """A plan of the key that batch size B selects, through the module's own positional signature."""
    if isinstance(m, BiLSTM):
        return m._checkout(B, 9, 24, "cpu", training, False)
    return m._checkout(B, 9, "cpu", training)


MODULES = [HipLSTM, LSTM, BiLSTM]


@pytest.mark.parametrize("cls", MODULES)
def test_an_idle_plan_is_reused_and_a_busy_one_is_not(cls):
    m = cls(24, 96, 2)
    assert m.all_plans() == [] and m._plans == {}
    a = _checkout(m, 4)
    assert _checkout(m, 4) is a and m.all_plans() == [a]
    a.busy = True
    b = _checkout(m, 4)
    assert b is not a and m.all_plans() == [a, b] and len(m._plans) == 1
    b.busy = True
    a.busy = False
    assert _checkout(m, 4) is a and m.all_plans() == [a, b]


@pytest.mark.parametrize("cls", MODULES)
def test_the_oldest_idle_plan_of_another_key_goes_when_a_new_key_is_created(cls):
    m = cls(24, 96, 2)
    n = m.MAX_IDLE_PLANS
    assert n == 4
    plans = [_checkout(m, B) for B in range(1, n + 1)]         # n idle plans under n other keys: nothing dropped so far
    assert m.all_plans() == plans
    new = _checkout(m, 100)
    assert m.all_plans() == plans[1:] + [new]                   # the oldest went, the n - 1 younger ones stay
    assert _checkout(m, 1) not in plans                         # (its key is still there, with an empty list: a new plan)
    assert plans[1] not in m.all_plans() and len(m.all_plans()) == n


@pytest.mark.parametrize("cls", MODULES)
def test_busy_plans_and_plans_of_the_requested_key_are_never_dropped(cls):
    m = cls(24, 96, 2)
    n = m.MAX_IDLE_PLANS
    busy = []
    for B in range(1, n + 3):
        busy.append(_checkout(m, B))
        busy[-1].busy = True
    own = _checkout(m, 50)
    own.busy = True
    idle = [_checkout(m, B) for B in range(60, 60 + n - 1)]    # n - 1 idle plans of other keys: below the threshold
    second = _checkout(m, 50)                                   # beside its busy first plan; 3 idle others: nothing goes
    assert second is not own and m.all_plans() == busy + [own, second] + idle
    second.busy = True
    extra = _checkout(m, 63)                                    # a new key with 3 idle others: nothing goes; now n are idle
    assert m.all_plans() == busy + [own, second] + idle + [extra]
    third = _checkout(m, 50)                                    # n idle plans of other keys: the oldest of THEM goes, no more
    assert m.all_plans() == busy + [own, second, third] + idle[1:] + [extra]
    assert m.all_plans() == [pl for lst in m._plans.values() for pl in lst]


@pytest.mark.parametrize("cls", MODULES)
def test_max_idle_plans_is_read_from_the_module_at_every_checkout(cls):
    m = cls(24, 96, 2)
    m.MAX_IDLE_PLANS = 1
    a, b = _checkout(m, 1), _checkout(m, 2)
    assert m.all_plans() == [b] and a is not b


def test_key_tuples_are_the_parents():
    hip, lstm, bi = HipLSTM(24, 96, 2), LSTM(24, 96, 2), BiLSTM(24, 96, 2)
    res_hip, res_bi = HipLSTM(24, 96, 2, resident=True, compute_dtype=torch.float32), BiLSTM(24, 96, 2, resident=True)
    hip._checkout(4, 9, "cpu", True)
    hip._checkout(4, 9, "cpu", 0, dropout=True)
    hip._checkout(4, 9, "cpu", True, state=True)
    hip._checkout(4, 9, "cpu", True, True, True)
    assert list(hip._plans) == [(4, 9, "cpu", True, BF16), (4, 9, "cpu", False, BF16, "dropout plan"),
                                (4, 9, "cpu", True, BF16, "state plan"), (4, 9, "cpu", True, BF16, "dropout plan", "state plan")]
    lstm._checkout(4, 9, "cpu", True)
    lstm._checkout(4, 9, "cpu", True, state=True)                # the class's own kind: the same key
    lstm._checkout(4, 9, "cpu", True, dropout=True, state=False)
    assert list(lstm._plans) == [(4, 9, "cpu", True, BF16), (4, 9, "cpu", True, BF16, "dropout plan", "state plan")]
    res_hip._checkout(4, 9, torch.device("cpu"), True, dropout=True, state=True)
    assert list(res_hip._plans) == [(4, 9, "cpu", True, torch.float32, "dropout plan", "state plan", "resident plan")]
    bi._checkout(4, 9, 24, "cpu", True, False)
    bi._checkout(4, 9, 192, "cpu", False, True)
    res_bi._checkout(4, 9, 24, "cpu", 1, 1)
    assert list(bi._plans) == [(4, 9, 24, "cpu", True, BF16, False), (4, 9, 192, "cpu", False, BF16, True)]
    assert list(res_bi._plans) == [(4, 9, 24, "cpu", True, BF16, True, "resident plan")]


def test_the_constructor_arguments_reach_the_plan():
    hip, lstm, bi = HipLSTM(24, 96, 2), LSTM(24, 96, 3, resident=True), BiLSTM(24, 96, 2)
    pl = hip._checkout(4, 9, "cpu", True, dropout=True, state=True)
    assert pl.args == (4, 9, 24, 96, 2, BF16, "cpu") and pl.kw == dict(training=True, state=True, dropout=True, resident=False)
    pl = lstm._checkout(4, 9, "cpu", False)
    assert pl.args == (4, 9, 24, 96, 3, BF16, "cpu") and pl.kw == dict(training=False, state=True, dropout=False, resident=True)
    pl = bi._checkout(4, 9, 192, "cpu", True, True)
    assert pl.args == (4, 9, 192, 96, 1, BF16, "cpu") and pl.kw == dict(training=True, state=True, reverse=True, resident=False)
