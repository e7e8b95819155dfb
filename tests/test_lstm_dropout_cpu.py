"""CPU: the LSTM's inter-layer dropout without a GPU -- the Philox known answers, csn_lstm_dropout_keep (the library's host
definition of the mask) against the numpy one of tests/dropout_reference.py bit for bit, the keep rate, the
layer-by-layer composition of the emulator against its own L-layer run (exactly) and against a float64 nn.LSTM chain
with the same mask, and the host checks of csn_lstm_plan_set_dropout / HipLSTM(dropout=...) / LSTM(dropout=...)."""
import ctypes
import math
import os
import warnings

import numpy as np
import pytest
import torch

import dropout_reference as dref
from cerebralsignalnetworks_amd import cabi, LSTM, LSTMModel, Model
from cerebralsignalnetworks_amd.lstm_model import HipLSTM
from oracle import lstm as olstm

SEED = 0x0123456789ABCDEF


def _hex(words):
    return " ".join(f"{int(w[0]):08x}" for w in words)


def test_philox_known_answers():
    assert _hex(dref.philox4x32_10((0, 0, 0, 0), (0, 0))) == "6627e8d5 e169c58d bc57ac4c 9b00dbd8"
    got = dref.philox4x32_10((0x243F6A88, 0x85A308D3, 0x13198A2E, 0x03707344), (0xA4093822, 0x299F31D0))
    assert _hex(got) == "d16cfe09 94fdcceb 5001e420 24126ea1"


def test_library_words_are_the_known_answers():
    """The library's generator through its host window, the keep function: at p = 0.5 (thr = 2^31) an element is kept iff
    the top bit of its word is set.  Counter 0 / key 0 pins the order of words and elements; the comparison with the numpy
    mask below carries every other counter and key."""
    want = [int(w, 16) >> 31 for w in "6627e8d5 e169c58d bc57ac4c 9b00dbd8".split()]
    assert cabi.lstm_dropout_keep(0, 0, 0.5, 0, 4).tolist() == want
    assert cabi.lstm_dropout_keep(0, 0, 0.5, 1, 3).tolist() == want[1:]


@pytest.mark.parametrize("p", [0.0, 0.1, 0.5, 0.9, 1.0])
@pytest.mark.parametrize("first,n,sub", [(0, 4099, 0), (5, 4099, 0), (7, 1, 3), ((1 << 32) - 6, 64, 1), ((1 << 40) + 3, 1001, 0xFFFFFFFF),
                                         (5, 0, 0)])
def test_keep_equals_the_numpy_mask(p, first, n, sub):
    got = cabi.lstm_dropout_keep(SEED, sub, p, first, n)
    want = dref.keep(SEED, sub, p, first, n)
    assert got.dtype == np.uint8 and got.shape == (n,)
    assert np.array_equal(got.astype(bool), want)
    if p == 0.0:
        assert got.all()
    if p == 1.0:
        assert not got.any()


def test_keep_depends_on_seed_and_subsequence():
    base = cabi.lstm_dropout_keep(SEED, 0, 0.5, 0, 4096)
    assert np.array_equal(base, cabi.lstm_dropout_keep(SEED, 0, 0.5, 0, 4096))
    for seed, sub in ((SEED + 1, 0), (SEED ^ (1 << 32), 0), (SEED, 1)):       # low word, high word, subsequence
        other = cabi.lstm_dropout_keep(seed, sub, 0.5, 0, 4096)
        assert 0.4 < float((other != base).mean()) < 0.6
        assert np.array_equal(other.astype(bool), dref.keep(seed, sub, 0.5, 0, 4096))


@pytest.mark.parametrize("p", [0.1, 0.5, 0.9])
def test_keep_rate(p):
    n = 1 << 20
    kept = int(cabi.lstm_dropout_keep(SEED, 0, p, 5, n).sum())
    q = 1.0 - float(np.float32(p))
    z = (kept - n * q) / math.sqrt(n * q * (1 - q))
    print(f"keep rate p = {p}: {kept / n:.6f}, z = {z:+.2f}")
    assert abs(z) < 5.0, (p, kept, z)


def test_keep_refuses_bad_arguments():
    lib = cabi.load()
    buf = (ctypes.c_uint8 * 4)()
    for p in (-0.1, 1.5, float("nan")):
        assert lib.csn_lstm_dropout_keep(1, 0, p, 0, 4, buf) == 1 and b"outside [0, 1]" in lib.csn_last_error()
    assert lib.csn_lstm_dropout_keep(1, 0, 0.5, -1, 4, buf) == 1
    assert lib.csn_lstm_dropout_keep(1, 0, 0.5, 0, 4, None) == 1 and b"null" in lib.csn_last_error()


def _case(L, B=3, T=7, I=5, H=8, seed=0):
    torch.manual_seed(seed)
    lp = {k: v.detach().numpy() for k, v in torch.nn.LSTM(I, H, L, batch_first=True).state_dict().items()}
    rng = np.random.default_rng(seed + 1)
    x = rng.standard_normal((B, T, I)).astype(np.float32)
    h0 = (0.5 * rng.standard_normal((L, B, H))).astype(np.float32)
    c0 = rng.standard_normal((L, B, H)).astype(np.float32)
    dy = rng.standard_normal((B, T, H)).astype(np.float32)
    dh = rng.standard_normal((L, B, H)).astype(np.float32)
    dc = rng.standard_normal((L, B, H)).astype(np.float32)
    return lp, (x, h0, c0, dy, dh, dc)


@pytest.mark.parametrize("L", [2, 3])
@pytest.mark.parametrize("rounding", [True, False])
def test_composition_with_an_all_ones_mask_is_the_emulators_own_run(L, rounding):
    lp, (x, h0, c0, dy, dh, dc) = _case(L)
    y, saved = olstm.lstm_forward_bf16(x, lp, L, rounding=rounding, h0=h0, c0=c0)
    h_n, c_n = olstm.final_state(saved)
    dx, g, _, dh0, dc0 = olstm.lstm_backward_bf16(dy, saved, L, rounding=rounding, dh_n=dh, dc_n=dc, return_state=True)
    want = dict(out=y, h_n=h_n, c_n=c_n, dx=dx, dh0=dh0, dc0=dc0, **g)
    B, T, H = dy.shape
    ones = dref.interface_masks(SEED, 0, 0.0, L, T, B, H)
    assert ones.all() and ones.shape == (L - 1, B, T, H)
    for masks, s in ((ones, dref.scale(0.0)), (None, 1.0)):
        got = dref.composed_emulator(lp, L, x, h0, c0, dy, dh, dc, masks, s, rounding=rounding)
        assert set(got) == set(want)
        for k, w in want.items():
            assert np.array_equal(got[k], w), (L, rounding, k, float(np.abs(got[k] - w).max()))


@pytest.mark.parametrize("L", [2, 3])
@pytest.mark.parametrize("p", [0.1, 0.5, 1.0])
def test_unrounded_composition_is_the_float64_nn_lstm_chain(L, p):
    lp, (x, h0, c0, dy, dh, dc) = _case(L, seed=3)
    B, T, H = dy.shape
    masks, s = dref.interface_masks(SEED, 2, p, L, T, B, H), dref.scale(p)
    assert not masks.all() and (p < 1.0) == bool(masks.any())
    got = dref.composed_emulator(lp, L, x, h0, c0, dy, dh, dc, masks, s, rounding=False)
    want = dref.nn_lstm_chain(lp, L, x, h0, c0, dy, dh, dc, masks, s)
    assert set(got) == set(want)
    for k, w in want.items():
        err = float(np.abs(got[k] - w).max())
        assert err < 1e-10, (L, p, k, err)
    # the rounded composition stays a bf16 rounding away from it, and the mask does reach the result
    plain = dref.composed_emulator(lp, L, x, h0, c0, dy, dh, dc, None, 1.0, rounding=False)
    assert float(np.abs(plain["out"] - want["out"]).max()) > 1e-3
    # rows of a ragged batch: the rows' own slices of the mask (all rows at full length = the dense run)
    rows = dref.rows_composed_emulator(lp, L, x, [T] * B, h0, c0, dy, dh, dc, masks, s, rounding=False)
    for k, w in got.items():
        assert np.allclose(rows[k], w, rtol=0, atol=1e-12), k


def test_dropout_is_in_the_abi_and_checked_on_the_host():
    lib = cabi.load()
    assert lib.csn_abi_version() == 6 == cabi.ABI_VERSION          # added symbols do not bump it
    assert cabi.LSTM_DROPOUT == 0x200
    text = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "csn_hip.h")).read()
    assert "#define CSN_LSTM_DROPOUT 0x200" in text
    fn = lib.csn_lstm_plan_set_dropout
    assert fn(None, 0.5, 1, 0) == 1 and b"null plan" in lib.csn_last_error()
    # the workspace gains h_drop[l], T B H in the compute dtype, for every layer below the top -- and nothing without the bit
    for shape, dt, es, training in (((256, 500, 128, 768, 2), cabi.CSN_BF16, 2, 1), ((8, 30, 16, 128, 5), cabi.CSN_BF16, 2, 0),
                                    ((70, 37, 24, 128, 3), cabi.CSN_F32, 4, 1 | cabi.LSTM_STATE), ((4, 9, 8, 32, 1), cabi.CSN_F32, 4, 1)):
        d = cabi.LstmDesc(*shape, dt)
        B, T, _, H, L = shape
        plain = lib.csn_lstm_workspace_bytes(ctypes.byref(d), training)
        with_bit = lib.csn_lstm_workspace_bytes(ctypes.byref(d), training | cabi.LSTM_DROPOUT)
        per = -(-(T * B * H * es) // 256) * 256
        assert plain > 0 and with_bit - plain == (L - 1) * per, (shape, plain, with_bit)
    # the checks that need a plan: a plan is bound to a device, so they run where one can be created (and always in
    # tests/test_gpu_lstm_dropout.py::test_set_dropout_host_checks)
    d = cabi.LstmDesc(3, 5, 8, 32, 2, cabi.CSN_BF16)
    for flags, has_bit in ((1, False), (1 | cabi.LSTM_DROPOUT, True), (cabi.LSTM_DROPOUT | cabi.LSTM_STATE, True)):
        handle = ctypes.c_void_p()
        if lib.csn_lstm_plan_create(ctypes.byref(d), flags, ctypes.byref(handle)) != 0:
            assert b"hipGetDevice" in lib.csn_last_error()
            continue
        try:
            check_plan_arguments(lib, handle, has_bit)
        finally:
            lib.csn_lstm_plan_destroy(handle)


def check_plan_arguments(lib, handle, has_bit):
    """csn_lstm_plan_set_dropout: p outside [0, 1] and NaN refused; p > 0 refused without CSN_LSTM_DROPOUT; p = 0 always taken."""
    fn = lib.csn_lstm_plan_set_dropout
    for p in (-0.01, 1.01, float("nan"), float("inf")):
        assert fn(handle, p, 1, 0) == 1 and b"outside [0, 1]" in lib.csn_last_error(), p
    assert fn(handle, 0.0, 0, 0) == 0 and fn(handle, 0.0, 2 ** 64 - 1, 2 ** 32 - 1) == 0
    for p in (0.5, 1.0, 1e-30):
        if has_bit:
            assert fn(handle, p, 7, 1) == 0
        else:
            assert fn(handle, p, 7, 1) == 1 and b"without CSN_LSTM_DROPOUT" in lib.csn_last_error()
    assert fn(handle, 0.0, 0, 0) == 0


def test_modules_store_the_value():
    m = HipLSTM(8, 32, 2, dropout=0.25)
    assert m.dropout == 0.25 and m.dropout_subsequence is None
    assert HipLSTM(8, 32, 2).dropout == 0.0
    assert set(m.state_dict()) == set(torch.nn.LSTM(8, 32, 2, dropout=0.25).state_dict())      # no new state
    assert Model(8, 32, 2, 16, dropout=0.3).lstm.dropout == pytest.approx(0.3) and Model(8, 32, 2, 16).lstm.dropout == 0.0
    assert LSTMModel(8, 32, 2, 16, dropout=0.4).lstm.dropout == pytest.approx(0.4) and LSTMModel(8, 32, 2, 16).lstm.dropout == 0.0
    for bad in (-0.1, 1.1, "0.5", True):
        with pytest.raises(ValueError, match="dropout should be a number in range"):
            HipLSTM(8, 32, 2, dropout=bad)
    with pytest.warns(UserWarning, match="non-zero dropout expects num_layers greater than 1"):
        HipLSTM(8, 32, 1, dropout=0.5)
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        HipLSTM(8, 32, 2, dropout=0.5)
        HipLSTM(8, 32, 1, dropout=0.0)


def test_lstm_constructor_still_refuses_dropout_and_takes_the_attribute():
    with pytest.raises(ValueError, match="dropout != 0"):
        LSTM(8, 32, 2, dropout=0.1)
    lstm = LSTM(8, 32, 2)
    assert lstm.dropout == 0.0
    lstm.dropout = 0.1
    assert lstm.dropout == 0.1
    # a bad value set as the attribute is refused when it is read, before any launch (a CPU tensor would be refused next)
    lstm.dropout = 1.5
    with pytest.raises(ValueError, match="dropout should be a number in range"):
        lstm(torch.zeros(2, 3, 8))


def test_seed_draw_follows_the_cpu_generator_and_the_mode():
    from cerebralsignalnetworks_amd import lstm_model
    m = HipLSTM(8, 32, 2, dropout=0.5)
    torch.manual_seed(11)
    a = lstm_model._draw_dropout(m)
    b = lstm_model._draw_dropout(m)
    torch.manual_seed(11)
    assert lstm_model._draw_dropout(m) == a and a != b
    p, seed, sub = a
    assert p == 0.5 and 0 <= seed < 2 ** 64 and sub == 0
    m.dropout_subsequence = 3
    assert lstm_model._draw_dropout(m)[2] == 3
    one = HipLSTM(8, 32, 1)
    one.dropout = 0.5
    state = torch.get_rng_state()
    m.eval()
    assert lstm_model._draw_dropout(m) is None                       # eval(): off, and nothing is drawn
    m.train()
    m.dropout = 0.0
    assert lstm_model._draw_dropout(m) is None
    assert lstm_model._draw_dropout(one) is None                     # a single layer has no interface
    assert torch.equal(torch.get_rng_state(), state)
    with torch.no_grad():                                            # as in torch: grad mode does not enter
        m.dropout = 0.5
        assert lstm_model._draw_dropout(m) is not None
