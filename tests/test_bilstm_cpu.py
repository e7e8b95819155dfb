"""No GPU: the bidirectional LSTM's host side -- BiLSTM's parameters and argument checks, the new C ABI symbols, and the
reference of tests/test_gpu_bilstm.py validating itself (the stack composed from single-layer modules on explicitly
reversed tensors against float64 nn.LSTM(bidirectional=True))."""
import ctypes
import os
import re

import pytest
import torch
from torch.nn.utils.rnn import pack_padded_sequence

import bilstm_reference as bref
from cerebralsignalnetworks_amd import cabi, BiLSTM, LSTM, Model

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_parameters_are_nn_lstms():
    torch.manual_seed(0)
    I, H, L = 24, 32, 3
    m = BiLSTM(I, H, L)
    ref = torch.nn.LSTM(I, H, L, batch_first=True, bidirectional=True)
    got = [(k, tuple(p.shape)) for k, p in m.named_parameters()]
    assert got == [(k, tuple(p.shape)) for k, p in ref.named_parameters()]
    assert got[4][0] == "weight_ih_l0_reverse" and dict(got)["weight_ih_l1"] == (4 * H, 2 * H)
    bound = H ** -0.5                                   # nn.LSTM's init: U(-1/sqrt(H), 1/sqrt(H))
    for k, p in m.named_parameters():
        assert 0.8 * bound < float(p.detach().abs().max()) <= bound, k
    # state_dict round trip, both ways, strict
    ref.load_state_dict(m.state_dict(), strict=True)
    m2 = BiLSTM(I, H, L)
    m2.load_state_dict(ref.state_dict(), strict=True)
    for (k, p), (_, q) in zip(m.named_parameters(), m2.named_parameters()):
        assert torch.equal(p, q), k
    assert m.bidirectional and m.batch_first and m.all_plans() == []


def test_arguments_are_checked_before_any_launch():
    B, T, I, H, L = 3, 5, 8, 32, 2
    m = BiLSTM(I, H, L)
    x = torch.zeros(B, T, I)
    with pytest.raises(ValueError, match=r"h0 must be \[2 \* num_layers, B, hidden_size\]"):
        m(x, (torch.zeros(L, B, H), torch.zeros(L, B, H)))
    with pytest.raises(ValueError, match="c0 must be"):
        m(x, (torch.zeros(2 * L, B, H), torch.zeros(2 * L, B + 1, H)))
    with pytest.raises(ValueError, match="2 lengths for a batch of 3"):
        m(x, lengths=[1, 2])
    with pytest.raises(ValueError, match=r"length 6 outside \[0, T = 5\]"):
        m(x, lengths=[1, 6, 2])
    with pytest.raises(ValueError, match="1-d int tensor"):
        m(x, lengths=torch.tensor([1.0, 2.0, 3.0]))
    with pytest.raises(ValueError, match="9 features, expected 8"):
        m(torch.zeros(B, T, I + 1))
    with pytest.raises(ValueError, match="batched"):
        m(torch.zeros(T, I))
    packed = pack_padded_sequence(x, torch.tensor([5, 3, 1]), batch_first=True)
    with pytest.raises(ValueError, match="lengths given together with a PackedSequence"):
        m(packed, lengths=[5, 3, 1])
    with pytest.raises(ValueError, match="dropout != 0 is not supported"):
        BiLSTM(I, H, L, dropout=0.1)
    # valid arguments on CPU tensors reach the refusal to run without a GPU
    for args in ((x,), (x, (torch.zeros(2 * L, B, H), torch.zeros(2 * L, B, H))), (x, None, [5, 0, 1]), (packed,)):
        with pytest.raises(cabi.CsnError, match="GPU only"):
            m(*args)
    assert m.all_plans() == []


def test_lstm_still_refuses_bidirectional_and_points_at_bilstm():
    with pytest.raises(ValueError, match="not supported") as e:
        LSTM(8, 32, 2, bidirectional=True)
    assert "bidirectional=True" in str(e.value) and "BiLSTM" in str(e.value)


def test_new_symbols_are_declared_bound_and_checked():
    header = open(os.path.join(ROOT, "include", "csn_hip.h")).read()
    assert re.search(r"#define\s+CSN_LSTM_REVERSE\s+0x400\b", header) and cabi.LSTM_REVERSE == 0x400
    assert re.search(r"int\s+csn_lstm_plan_set_io\(csnLstmPlan\*\s*\w+,\s*int64_t\s+\w+,\s*int64_t\s+\w+,\s*int\s+\w+\);", header)
    assert "csn_lstm_plan_set_io" in cabi.SIGNATURES
    assert re.search(r"#define\s+CSN_ABI_VERSION\s+6\b", header)
    lib = cabi.load()
    assert lib.csn_abi_version() == 6 == cabi.ABI_VERSION          # an added symbol / flag bit does not bump it
    fn = lib.csn_lstm_plan_set_io
    assert fn(None, 0, 0, 0) == 1 and b"null plan" in lib.csn_last_error()
    # the workspace of a reverse plan is that of a plan without the bit (host only)
    d = cabi.LstmDesc(256, 500, 128, 768, 1, cabi.CSN_BF16)
    ws = lib.csn_lstm_workspace_bytes
    assert ws(ctypes.byref(d), 1 | cabi.LSTM_STATE | cabi.LSTM_REVERSE) == ws(ctypes.byref(d), 1 | cabi.LSTM_STATE) > 0
    # the checks that need a plan: a plan is bound to a device, so they run where one can be created (and always in
    # tests/test_gpu_bilstm.py::test_pitch_and_add)
    H = 32
    d = cabi.LstmDesc(3, 5, 8, H, 1, cabi.CSN_BF16)
    for flags in (1, 1 | cabi.LSTM_STATE | cabi.LSTM_REVERSE):
        handle = ctypes.c_void_p()
        if lib.csn_lstm_plan_create(ctypes.byref(d), flags, ctypes.byref(handle)) != 0:
            assert b"hipGetDevice" in lib.csn_last_error()
            continue
        try:
            check_set_io_arguments(lib, handle, H)
        finally:
            lib.csn_lstm_plan_destroy(handle)


def check_set_io_arguments(lib, handle, H):
    """csn_lstm_plan_set_io on a plan of hidden size H: a pitch below H or no multiple of 4 is refused, 0 and 2H accepted."""
    fn = lib.csn_lstm_plan_set_io
    for bad in (H - 4, H + 2, -4):
        assert fn(handle, bad, 0, 0) == 1 and b"y_all_pitch = %d" % bad in lib.csn_last_error()
        assert fn(handle, 0, bad, 1) == 1 and b"dy_all_pitch = %d" % bad in lib.csn_last_error()
    for ok in (0, H, H + 4, 2 * H):
        assert fn(handle, ok, ok, 0) == 0 and fn(handle, ok, 0, 1) == 0
    assert fn(handle, 0, 0, 0) == 0


def test_binding_passes_reverse_and_keys_it():
    import inspect
    sig = inspect.signature(cabi.LstmPlan.__init__)
    assert sig.parameters["reverse"].default is False
    assert "set_io" in vars(cabi.LstmPlan)
    plan = object.__new__(cabi.LstmPlan)
    plan.desc, plan.training, plan.state, plan.dropout = cabi.LstmDesc(2, 3, 8, 32, 1, 1), True, True, False
    plan.reverse = False
    plain = plan.key()
    plan.reverse = True
    assert plan.key() != plain and plan.key()[:len(plain)] == plain
    plan._plan = None       # (never created: nothing to destroy)


# ---- the reference validates itself ------------------------------------------------------------------------------------
@pytest.mark.parametrize("lengths", [(9, 3, 1, 6, 9), (9, 0, 1, 0, 4), None], ids=str)
def test_composed_stack_is_float64_bidirectional_nn_lstm(lengths):
    B, T, I, H, L = 5, 9, 7, 8, 3
    torch.manual_seed(2)
    ref = torch.nn.LSTM(I, H, L, batch_first=True, bidirectional=True).double()
    layers = bref.single_layer_modules(ref, lambda i, h: torch.nn.LSTM(i, h, 1, batch_first=True).double())
    g = torch.Generator().manual_seed(3)
    x = torch.randn(B, T, I, generator=g, dtype=torch.float64)
    h0, c0, dh, dc = (torch.randn(2 * L, B, H, generator=g, dtype=torch.float64) for _ in range(4))
    dy = torch.randn(B, T, 2 * H, generator=g, dtype=torch.float64)
    want = bref.nn_bilstm_f64(ref, x, lengths, h0, c0, dy, dh, dc)
    got = bref.run(lambda xx, hx: bref.composed(layers, bref.call_packed, xx, hx, lengths),
                   bref.composed_named_params(layers), x, h0, c0, dy, dh, dc)
    assert set(got) == set(want) and len(want) == 6 + 8 * L
    for k, w in want.items():
        err = float((got[k] - w).abs().max())
        assert err <= 1e-12 * float(w.abs().max()), (k, err)
    if lengths is not None:
        for b, n in enumerate(lengths):
            assert not want["out"][b, n:].any() and not want["dx"][b, n:].any()
    # R is an involution that leaves the padding alone
    assert torch.equal(bref.R(bref.R(x, lengths), lengths), x)
    if lengths is not None:
        assert torch.equal(bref.R(x, lengths)[1, lengths[1]:], x[1, lengths[1]:])
        assert torch.equal(bref.R(x, lengths)[0, 0], x[0, lengths[0] - 1])


def test_model_bidirectional_head_and_keys():
    torch.manual_seed(4)
    C, H, L, D = 16, 32, 2, 8
    m = Model(input_size=C, lstm_size=H, lstm_layers=L, output_size=D, include_top=True, n_classes=5, bidirectional=True)
    assert isinstance(m.lstm, BiLSTM) and m.fc.in_features == 2 * H and m.fc.out_features == D

    class Twin(torch.nn.Module):            # the same network from stock torch modules
        def __init__(self):
            super().__init__()
            self.lstm = torch.nn.LSTM(C, H, L, batch_first=True, bidirectional=True)
            self.fc = torch.nn.Linear(2 * H, D)
            self.class_pred = torch.nn.Linear(D, 5)

        def forward(self, x):
            _, (h_n, _) = self.lstm(x)
            feat = self.fc(torch.cat((h_n[-2], h_n[-1]), dim=1))
            return feat, self.class_pred(feat)
    twin = Twin()
    twin.load_state_dict(m.state_dict(), strict=True)
    m.load_state_dict(twin.state_dict(), strict=True)
    assert twin(torch.zeros(2, 3, C))[0].shape == (2, D)
    assert not Model(input_size=C, lstm_size=H, lstm_layers=L, output_size=D).bidirectional
    with pytest.raises(cabi.CsnError, match="GPU only"):
        m(torch.zeros(2, 3, C))


def test_cli_flag_is_on_both_parsers():
    import LstmDistillFromDinoV2Train as train
    for flavour in (train.PERILS, train.SPAMPINATO):
        p = train.build_parser(flavour)
        assert p.parse_args([]).bidirectional is False
        assert p.parse_args(["--bidirectional"]).bidirectional is True
