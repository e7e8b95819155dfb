"""CPU: the initial / final LSTM state (h0, c0 -> h_n, c_n).  The float64 reference the GPU tests use
(torch.nn.LSTM in float64 with an explicit state) is checked against the oracle; lstm_model.LSTM has nn.LSTM's
parameters and rejects what it does not implement; the library checks the new plan flag on the host."""
import ctypes
import os

import numpy as np
import pytest
import torch

import __graft_entry__ as graft
from cerebralsignalnetworks_amd import cabi, LSTM
from oracle import lstm as olstm


def reference_lstm(params, I, H, L):
    """float64 nn.LSTM(batch_first=True) carrying `params` (numpy, nn.LSTM key names)."""
    ref = torch.nn.LSTM(I, H, num_layers=L, batch_first=True).double()
    ref.load_state_dict({k: torch.from_numpy(np.asarray(v, np.float64)) for k, v in params.items()})
    return ref


def test_float64_reference_with_zero_state_matches_oracle():
    B, T, I, H, L = 3, 7, 5, 8, 2
    rng = np.random.default_rng(0)
    src = torch.nn.LSTM(I, H, num_layers=L, batch_first=True)
    params = {k: v.detach().numpy().astype(np.float64) for k, v in src.state_dict().items()}
    x = rng.standard_normal((B, T, I))
    dy = rng.standard_normal((B, T, H))
    ref = reference_lstm(params, I, H, L)
    xt = torch.from_numpy(x).requires_grad_(True)
    h0 = torch.zeros(L, B, H, dtype=torch.float64, requires_grad=True)
    c0 = torch.zeros(L, B, H, dtype=torch.float64, requires_grad=True)
    y, (h_n, c_n) = ref(xt, (h0, c0))
    (y * torch.from_numpy(dy)).sum().backward()
    y_o, saved = olstm.lstm_forward(x, params, L, return_saved=True)
    dx_o, g_o = olstm.lstm_backward(dy, params, saved, L)
    np.testing.assert_allclose(y.detach().numpy(), y_o, rtol=0, atol=1e-12)
    for l in range(L):
        np.testing.assert_allclose(h_n[l].detach().numpy(), saved[l]["hs"][:, -1], rtol=0, atol=1e-12)
        np.testing.assert_allclose(c_n[l].detach().numpy(), saved[l]["cs"][:, -1], rtol=0, atol=1e-12)
    np.testing.assert_allclose(xt.grad.numpy(), dx_o, rtol=0, atol=1e-12)
    for k, p in ref.named_parameters():
        np.testing.assert_allclose(p.grad.numpy(), g_o[k], rtol=0, atol=1e-12)


def test_lstm_has_nn_lstm_parameters_and_state_dicts_load_both_ways():
    torch.manual_seed(3)
    m = LSTM(12, 64, 3)
    ref = torch.nn.LSTM(12, 64, num_layers=3, batch_first=True)
    assert [(k, tuple(v.shape)) for k, v in m.named_parameters()] == \
        [(k, tuple(v.shape)) for k, v in ref.named_parameters()]
    m.load_state_dict(ref.state_dict())
    for k, v in ref.state_dict().items():
        assert torch.equal(m.state_dict()[k], v)
    ref2 = torch.nn.LSTM(12, 64, num_layers=3, batch_first=True)
    ref2.load_state_dict(m.state_dict())
    for k, v in m.state_dict().items():
        assert torch.equal(ref2.state_dict()[k], v)
    # nn.LSTM's init: U(-1/sqrt(H), 1/sqrt(H))
    bound = 1.0 / np.sqrt(64)
    assert all(float(p.detach().abs().max()) <= bound for p in LSTM(12, 64, 3).parameters())


@pytest.mark.parametrize("kw", [dict(bias=False), dict(dropout=0.1), dict(bidirectional=True), dict(proj_size=16),
                                dict(batch_first=False)])
def test_lstm_rejects_unsupported_options(kw):
    with pytest.raises(ValueError, match="not supported"):
        LSTM(8, 32, 2, **kw)


def test_lstm_rejects_bad_input_and_state_before_any_launch():
    m = LSTM(8, 32, 2)
    with pytest.raises(ValueError, match="unbatched"):
        m(torch.zeros(5, 8))
    with pytest.raises(ValueError, match="features"):
        m(torch.zeros(2, 5, 7))
    with pytest.raises(ValueError, match="h0 must be"):
        m(torch.zeros(2, 5, 8), (torch.zeros(1, 2, 32), torch.zeros(2, 2, 32)))
    with pytest.raises(ValueError, match="c0 must be"):
        m(torch.zeros(2, 5, 8), (torch.zeros(2, 2, 32), torch.zeros(2, 3, 32)))
    with pytest.raises(cabi.CsnError):          # GPU only, no CPU fallback
        m(torch.zeros(2, 5, 8), (torch.zeros(2, 2, 32), torch.zeros(2, 2, 32)))


@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(cabi.LIB_PATH):
        graft.build()
    return cabi.load()


def test_state_flag_is_checked_on_the_host(lib):
    assert lib.csn_abi_version() == 6 == cabi.ABI_VERSION
    d = cabi.LstmDesc(4, 8, 16, 48, 2, cabi.CSN_F32)        # H not a multiple of 32: still refused with the flag
    assert lib.csn_lstm_workspace_bytes(ctypes.byref(d), 1 | cabi.LSTM_STATE) == 0
    assert b"multiple of 32" in lib.csn_last_error()
    # a state plan runs the per-step cell paths: its workspace is never larger than the stateless plan's
    for shape in [(256, 500, 128, 768, 2), (16, 460, 128, 128, 4), (16, 460, 96, 96, 2), (70, 37, 24, 128, 2),
                  (8, 30, 16, 128, 5)]:
        for dt in (cabi.CSN_BF16, cabi.CSN_F32):
            d = cabi.LstmDesc(*shape, dt)
            for training in (0, 1):
                plain = lib.csn_lstm_workspace_bytes(ctypes.byref(d), training)
                state = lib.csn_lstm_workspace_bytes(ctypes.byref(d), training | cabi.LSTM_STATE)
                assert 0 < state <= plain, (shape, dt, training, state, plain)
    # null plan: refused before anything else, for the stateful entry points as for the others
    rc = lib.csn_lstm_forward(None, None, 0, 0, None, None, None, None, None, None, None, None, None, None, None, None)
    assert rc == 1 and b"null plan" in lib.csn_last_error()
    rc = lib.csn_lstm_backward(None, None, None, None, None, None, None, None, None, None, None, None, None, None)
    assert rc == 1 and b"null plan" in lib.csn_last_error()
