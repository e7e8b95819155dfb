"""CPU: the initial / final LSTM state (h0, c0 -> h_n, c_n).  The float64 reference the GPU tests use
(torch.nn.LSTM in float64 with an explicit state) is checked against the oracle; the bf16-faithful emulator with state
is that reference without rounding for every subset of the state arguments and incoming gradients, chains through its
state and rounds h0 as torch does; lstm_model.LSTM has nn.LSTM's parameters and rejects what it does not implement; the
library checks the new plan flag on the host."""
import ctypes
import itertools
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


# ---- the bf16-faithful emulator with state (oracle.lstm.lstm_forward_bf16 / lstm_backward_bf16) ------------------------
_FWD_IN = ("h0", "c0")
_BWD_IN = ("dy_last", "dy_all", "dh_n", "dc_n")
_FWD_SUBSETS = [s for n in range(3) for s in itertools.combinations(_FWD_IN, n)]
_BWD_SUBSETS = [s for n in range(1, 5) for s in itertools.combinations(_BWD_IN, n)]


def _state_case(B, T, I, H, L, seed=0):
    p = olstm.init_params(I, H, L, 4, seed=seed)
    lp = {k[len("lstm."):]: v for k, v in p.items() if k.startswith("lstm.")}
    rng = np.random.default_rng(seed)
    f32 = lambda *s: rng.standard_normal(s).astype(np.float32)      # noqa: E731
    a = dict(x=f32(B, T, I), h0=0.5 * f32(L, B, H), c0=f32(L, B, H), dy_last=f32(B, H), dy_all=0.1 * f32(B, T, H),
             dh_n=f32(L, B, H), dc_n=f32(L, B, H))
    return lp, a


def _emu(lp, a, L, fwd, bwd, rounding):
    """Emulator forward with the state arguments in `fwd`, backward with the incoming gradients in `bwd` (others None)."""
    y, saved = olstm.lstm_forward_bf16(a["x"], lp, L, rounding=rounding, h0=a["h0"] if "h0" in fwd else None,
                                       c0=a["c0"] if "c0" in fwd else None)
    h_n, c_n = olstm.final_state(saved)
    dt = np.float32 if rounding else np.float64       # the library adds dy_last to dy_all in float32
    dy = a["dy_all"].astype(dt) if "dy_all" in bwd else np.zeros(y.shape, dt)
    if "dy_last" in bwd:
        dy[:, -1] += a["dy_last"]
    dx, g, _, dh0, dc0 = olstm.lstm_backward_bf16(dy, saved, L, rounding=rounding,
                                                 dh_n=a["dh_n"] if "dh_n" in bwd else None,
                                                 dc_n=a["dc_n"] if "dc_n" in bwd else None, return_state=True)
    return dict(y=y, h_n=h_n, c_n=c_n, dx=dx, dh0=dh0, dc0=dc0, **g)


@pytest.mark.parametrize("bwd", _BWD_SUBSETS, ids="+".join)
@pytest.mark.parametrize("fwd", _FWD_SUBSETS, ids=lambda s: "+".join(s) or "no_state")
def test_emulator_without_rounding_is_nn_lstm_with_state(fwd, bwd):
    """Every subset of (h0, c0) x every non-empty subset of the incoming gradients: the emulator without rounding against
    float64 torch.nn.LSTM given an explicit state (a missing argument is zeros there)."""
    B, T, I, H, L = 5, 6, 7, 8, 3
    lp, a = _state_case(B, T, I, H, L)
    got = _emu(lp, a, L, fwd, bwd, rounding=False)
    ref = reference_lstm(lp, I, H, L)
    t = {k: torch.from_numpy(v.astype(np.float64) if k in ("x",) + fwd + bwd else np.zeros(v.shape)) for k, v in a.items()}
    x, h0, c0 = (t[k].requires_grad_(True) for k in ("x", "h0", "c0"))
    y, (h_n, c_n) = ref(x, (h0, c0))
    ((y * t["dy_all"]).sum() + (y[:, -1] * t["dy_last"]).sum() + (h_n * t["dh_n"]).sum() + (c_n * t["dc_n"]).sum()).backward()
    want = dict(y=y, h_n=h_n, c_n=c_n, dx=x.grad, dh0=h0.grad, dc0=c0.grad, **{k: p.grad for k, p in ref.named_parameters()})
    assert set(got) == set(want)
    for k, v in want.items():
        np.testing.assert_allclose(got[k], v.detach().numpy(), rtol=0, atol=1e-12, err_msg=k)


def test_emulator_chains_through_the_state():
    """Two chunks carried through (h_n, c_n): with rounding the forward is the whole run's bit for bit; without rounding
    the first chunk's backward fed (dh_n, dc_n) = the second chunk's (dh0, dc0) is the whole backward."""
    B, T, I, H, L, k = 5, 9, 7, 32, 3, 4
    lp, a = _state_case(B, T, I, H, L, seed=1)
    x, dy = a["x"], a["dy_all"]
    for rounding in (True, False):
        y, saved = olstm.lstm_forward_bf16(x, lp, L, rounding=rounding, h0=a["h0"], c0=a["c0"])
        y1, s1 = olstm.lstm_forward_bf16(x[:, :k], lp, L, rounding=rounding, h0=a["h0"], c0=a["c0"])
        h_n1, c_n1 = olstm.final_state(s1)
        y2, s2 = olstm.lstm_forward_bf16(x[:, k:], lp, L, rounding=rounding, h0=h_n1, c0=c_n1)
        if rounding:
            assert np.array_equal(np.concatenate([y1, y2], axis=1), y)
            for got, want in zip(olstm.final_state(s2), olstm.final_state(saved)):
                assert np.array_equal(got, want)
            continue
        dx, g, _, dh0, dc0 = olstm.lstm_backward_bf16(dy, saved, L, rounding=False, dh_n=a["dh_n"], dc_n=a["dc_n"],
                                                     return_state=True)
        dx2, g2, _, dh0_2, dc0_2 = olstm.lstm_backward_bf16(dy[:, k:], s2, L, rounding=False, dh_n=a["dh_n"],
                                                           dc_n=a["dc_n"], return_state=True)
        dx1, g1, _, dh0_1, dc0_1 = olstm.lstm_backward_bf16(dy[:, :k], s1, L, rounding=False, dh_n=dh0_2, dc_n=dc0_2,
                                                           return_state=True)
        pairs = [(np.concatenate([dx1, dx2], axis=1), dx), (dh0_1, dh0), (dc0_1, dc0)] + [(g1[n] + g2[n], g[n]) for n in g]
        for got, want in pairs:
            np.testing.assert_allclose(got, want, rtol=0, atol=1e-12 * np.abs(want).max())


def test_emulator_state_rounding_and_null_means_zeros():
    """h0 is rounded as torch's bf16 cast rounds, c0 stays float32; h_n is bf16 values and h_n[L-1] the last output;
    NULL state arguments and gradients are zeros, bit for bit."""
    B, T, I, H, L = 70, 5, 7, 64, 2
    lp, a = _state_case(B, T, I, H, L, seed=2)
    h0 = (a["h0"] * np.float32(3.7)).astype(np.float32)
    y, saved = olstm.lstm_forward_bf16(a["x"], lp, L, h0=h0, c0=a["c0"])
    for l, s in enumerate(saved):
        assert np.array_equal(s["h0"], torch.from_numpy(h0[l]).to(torch.bfloat16).double().numpy())
        assert np.array_equal(s["c0"], a["c0"][l].astype(np.float64))
    h_n, c_n = olstm.final_state(saved)
    assert np.array_equal(h_n, olstm.bf16_round(h_n)) and np.array_equal(c_n, c_n.astype(np.float32))
    assert np.array_equal(h_n[-1], y[:, -1])
    z = {k: np.zeros_like(v) for k, v in a.items()}
    zeros = dict(a, h0=z["h0"], c0=z["c0"], dh_n=z["dh_n"], dc_n=z["dc_n"])
    null = _emu(lp, a, L, (), ("dy_last", "dy_all"), rounding=True)
    explicit = _emu(lp, zeros, L, _FWD_IN, _BWD_IN, rounding=True)
    for k, v in null.items():
        assert np.array_equal(v, explicit[k]), k
