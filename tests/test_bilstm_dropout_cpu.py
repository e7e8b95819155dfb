"""No GPU: the host side of the bidirectional LSTM's inter-layer dropout and input windows -- the new C ABI symbol
(csn_lstm_plan_set_output_dropout), the reference of tests/test_gpu_bilstm_dropout.py validating itself, and BiLSTM's /
Model's / the CLIs' host logic."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

import bilstm_dropout_reference as bdref
import bilstm_dropout_stream_cases  # noqa: F401  (joins the stream-order setter table on import)
import bilstm_reference as bref
import dropout_reference as dref
from cerebralsignalnetworks_amd import cabi, BiLSTM, Model
from cerebralsignalnetworks_amd import lstm_model

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---- the symbol ---------------------------------------------------------------------------------------------------------
def test_symbol_is_declared_bound_and_checked():
    header = open(os.path.join(ROOT, "include", "csn_hip.h")).read()
    assert re.search(r"int\s+csn_lstm_plan_set_output_dropout\(csnLstmPlan\*\s*\w+,\s*float\s+\w+,\s*uint64_t\s+\w+,\s*uint32_t\s+\w+,"
                     r"\s*uint64_t\s+\w+,\s*int64_t\s+\w+\);", header)
    assert "csn_lstm_plan_set_output_dropout" in cabi.SIGNATURES
    assert "set_output_dropout" in vars(cabi.LstmPlan)
    assert re.search(r"#define\s+CSN_ABI_VERSION\s+6\b", header)
    lib = cabi.load()
    assert lib.csn_abi_version() == 6 == cabi.ABI_VERSION          # an added symbol does not bump it
    fn = lib.csn_lstm_plan_set_output_dropout
    assert fn(None, 0.0, 0, 0, 0, 0) == 1 and b"null plan" in lib.csn_last_error()
    # the checks that need a plan: a plan is bound to a device, so they run where one can be created (and always in
    # tests/test_gpu_bilstm_dropout.py)
    H = 32
    d = cabi.LstmDesc(3, 5, 8, H, 1, cabi.CSN_BF16)
    for flags in (1, 1 | cabi.LSTM_STATE | cabi.LSTM_REVERSE):
        handle = ctypes.c_void_p()
        if lib.csn_lstm_plan_create(ctypes.byref(d), flags, ctypes.byref(handle)) != 0:
            assert b"hipGetDevice" in lib.csn_last_error()
            continue
        try:
            check_set_output_dropout_arguments(lib, handle, H)
        finally:
            lib.csn_lstm_plan_destroy(handle)


def check_set_output_dropout_arguments(lib, handle, H):
    """csn_lstm_plan_set_output_dropout on a plan of hidden size H: p outside [0, 1] or NaN is refused; with p > 0 a first or
    an index_pitch that is no multiple of 4, or an index_pitch below H; with p = 0 anything goes."""
    fn = lib.csn_lstm_plan_set_output_dropout
    for bad in (-0.1, 1.5, float("nan")):
        assert fn(handle, bad, 0, 0, 0, 2 * H) == 1 and b"outside [0, 1]" in lib.csn_last_error()
    for first, pitch in ((2, 2 * H), (0, 2 * H + 2), (0, H - 4), (0, 0), (0, -4)):
        assert fn(handle, 0.5, 1, 0, first, pitch) == 1 and b"index_pitch" in lib.csn_last_error(), (first, pitch)
        assert fn(handle, 0.0, 1, 0, first, pitch) == 0
    for first, pitch in ((0, H), (H, 2 * H), (2 ** 32 - 64, 2 * H + 4), (2 ** 40 + 4, H)):
        for p in (0.5, 1.0):
            assert fn(handle, p, 2 ** 63 + 5, 7, first, pitch) == 0
    assert fn(handle, 0.0, 0, 0, 0, 0) == 0


def test_setter_is_in_the_stream_order_table():
    import stream_order as so
    import test_stream_order_cpu as table_checks
    assert "test_bilstm_module_on_a_side_stream_with_late_inputs" in so.PLAN_SETTERS["csn_lstm_plan_set_output_dropout"]
    table_checks.test_plan_setters_table_names_exactly_the_setters_of_the_header()


# ---- the reference validates itself -------------------------------------------------------------------------------------
def _f64_layers(I, H, L, seed):
    torch.manual_seed(seed)
    ref = torch.nn.LSTM(I, H, L, batch_first=True, bidirectional=True).double()
    return ref, bref.single_layer_modules(ref, lambda i, h: torch.nn.LSTM(i, h, 1, batch_first=True).double())


def _f64_args(B, T, I, H, L, seed):
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(B, T, I, generator=g, dtype=torch.float64)
    h0, c0, dh, dc = (torch.randn(2 * L, B, H, generator=g, dtype=torch.float64) for _ in range(4))
    return x, h0, c0, torch.randn(B, T, 2 * H, generator=g, dtype=torch.float64), dh, dc


@pytest.mark.parametrize("lengths", [None, (9, 0, 1, 6, 4)], ids=str)
def test_composition_with_an_all_ones_mask_is_float64_bidirectional_nn_lstm(lengths):
    B, T, I, H, L = 5, 9, 7, 8, 3
    ref, layers = _f64_layers(I, H, L, 2)
    args = _f64_args(B, T, I, H, L, 3)
    ones = [torch.ones(B, T, 2 * H, dtype=torch.bool)] * (L - 1)
    want = bref.nn_bilstm_f64(ref, args[0], lengths, *args[1:])
    got = bref.run(lambda xx, hx: bdref.composed(layers, bref.call_packed, xx, hx, lengths, ones, 1.0),
                   bref.composed_named_params(layers), *args)
    assert set(got) == set(want) and len(want) == 6 + 8 * L
    for k, w in want.items():
        assert float((got[k] - w).abs().max()) <= 1e-12 * float(w.abs().max()), k


def test_composition_with_a_mask_passes_gradcheck():
    B, T, I, H, L, p = 2, 4, 3, 4, 2, 0.5
    _, layers = _f64_layers(I, H, L, 4)
    x, h0, c0, _, _, _ = _f64_args(B, T, I, H, L, 5)
    masks = bdref.interface_masks(11, 0, p, L, B, T, H)
    assert 0 < int(masks[0].sum()) < masks[0].numel()
    params = [q for _, q in bref.composed_named_params(layers)]

    def fn(xx, hh, cc, *_params):
        out, (h_n, c_n) = bdref.composed(layers, bref.call_packed, xx, (hh, cc), None, masks, dref.scale(p))
        return out, h_n, c_n
    inputs = [t.clone().requires_grad_(True) for t in (x, h0, c0)] + params
    assert torch.autograd.gradcheck(fn, inputs, eps=1e-6, atol=1e-6, rtol=1e-4)


def test_plan_masks_of_the_two_directions_tile_the_interface_stream():
    """first = l B T 2H + d H, index_pitch = 2H: the two plans of layer l draw the halves of the interface's one stream; and
    the library's host keep rule is the numpy one."""
    B, T, H, L, p, seed, sub = 3, 5, 32, 3, 0.5, 2 ** 40 + 3, 2
    for l, mask in enumerate(bdref.interface_masks(seed, sub, p, L, B, T, H)):
        for d in range(2):
            first = l * B * T * 2 * H + d * H
            half = bdref.plan_keep(seed, sub, p, first, 2 * H, B, T, H)
            assert torch.equal(half, mask[:, :, d * H:(d + 1) * H]), (l, d)
            e = bdref.element_index(first, 2 * H, B, T, H)
            assert int(e[1, 2, 3]) == first + (1 * T + 2) * 2 * H + 3
        lib_keep = cabi.lstm_dropout_keep(seed, sub, p, l * B * T * 2 * H, B * T * 2 * H).astype(bool)
        assert np.array_equal(lib_keep, mask.numpy().reshape(-1))


# ---- host logic ---------------------------------------------------------------------------------------------------------
def test_constructor_refusal_is_unchanged_and_the_attribute_is_read_on_every_call():
    with pytest.raises(ValueError, match="dropout != 0 is not supported"):
        BiLSTM(8, 32, 2, dropout=0.1)
    m = BiLSTM(8, 32, 2)
    assert m.dropout == 0.0 and m.dropout_subsequence is None
    m.dropout = 0.25                                   # accepted, as on the LSTM drop-in
    x = torch.zeros(3, 5, 8)
    with pytest.raises(cabi.CsnError, match="GPU only"):
        m(x)
    for bad in (1.5, -0.1, "0.5", True):
        m.dropout = bad
        with pytest.raises(ValueError, match=r"dropout should be a number in range \[0, 1\]"):
            m(x)
    assert m.all_plans() == []


def test_draw_dropout_follows_mode_layers_and_seed():
    m = BiLSTM(8, 32, 2)
    m.dropout = 0.5
    m.eval()
    assert lstm_model._draw_dropout(m) is None
    m.train()
    m.dropout = 0.0
    assert lstm_model._draw_dropout(m) is None
    one = BiLSTM(8, 32, 1)
    one.dropout = 0.5
    assert lstm_model._draw_dropout(one) is None
    m.dropout = 0.5
    torch.manual_seed(5)
    a, b = lstm_model._draw_dropout(m), lstm_model._draw_dropout(m)
    torch.manual_seed(5)
    with torch.no_grad():                              # grad mode does not enter
        c = lstm_model._draw_dropout(m)
    assert a == c and a != b and a[0] == 0.5 and a[2] == 0 and 0 <= a[1] < 2 ** 64
    m.dropout_subsequence = 3
    assert lstm_model._draw_dropout(m)[2] == 3


def test_model_bidirectional_takes_dropout_and_views():
    C, H, L, D = 16, 32, 2, 8
    m = Model(input_size=C, lstm_size=H, lstm_layers=L, output_size=D, include_top=False, bidirectional=True, dropout=0.25)
    assert isinstance(m.lstm, BiLSTM) and m.lstm.dropout == 0.25
    with pytest.raises(ValueError, match="dropout should be a number"):
        Model(input_size=C, lstm_size=H, lstm_layers=L, output_size=D, bidirectional=True, dropout=2.0)
    src = torch.zeros(2, 12, C)
    views, lengths = ([0, 1, 1], [0, 2, 4]), [5, 0, 8]
    with pytest.raises(cabi.CsnError, match="GPU only"):            # (no longer "views are not supported")
        m(src, views=views, lengths=lengths)
    # the refusals of _check_views apply to BiLSTM as to LSTM
    with pytest.raises(ValueError, match="views need lengths"):
        m.lstm(src, views=views)
    with pytest.raises(ValueError, match="requires grad"):
        m.lstm(src.clone().requires_grad_(True), lengths=lengths, views=views)
    with pytest.raises(ValueError, match="with views the input is the source tensor"):
        m.lstm(torch.zeros(2, 12, C + 1), lengths=lengths, views=views)
    with pytest.raises(ValueError, match="with views the input is the source tensor"):
        m.lstm(torch.nn.utils.rnn.pack_padded_sequence(src, torch.tensor([12, 3]), batch_first=True), lengths=lengths, views=views)
    # (the counts of rows / starts / lengths are checked behind the device check: tests/test_gpu_bilstm_views.py)
    with pytest.raises(ValueError, match="Model: lengths are taken with views only"):
        m(src, lengths=lengths)
    assert m.lstm.all_plans() == []


def test_cli_flags():
    import LstmDistillation as dino_cli
    import LstmDistillFromDinoV2Train as train
    p = dino_cli.build_parser()
    assert p.parse_args([]).bidirectional is False
    a = p.parse_args(["--bidirectional", "--fused_views", "--lstm_dropout", "0.2"])
    assert a.bidirectional is True and a.fused_views is True and a.lstm_dropout == 0.2
    for flavour in (train.PERILS, train.SPAMPINATO):
        text = train.build_parser(flavour).format_help()
        assert "--bidirectional" in text and "not with --lstm_dropout" not in " ".join(text.split())
