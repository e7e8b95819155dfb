"""CPU: variable-length LSTM batches (csn_lstm_plan_set_lengths, LSTM.forward(lengths=...), PackedSequence input).
The arguments of LSTM.forward are checked before any launch; the library checks csn_lstm_plan_set_lengths on the host
and keeps ABI version 6; and the reference the GPU tests use for bf16 -- the unmodified emulator run on every row's valid
steps alone, parameter gradients summed -- is float64 nn.LSTM on the packed batch when it does not round."""
import ctypes

import numpy as np
import pytest
import torch
from torch.nn.utils.rnn import pack_padded_sequence

import lengths_reference as lref
from cerebralsignalnetworks_amd import cabi, LSTM
from oracle import lstm as olstm


def test_forward_rejects_bad_lengths_before_any_launch():
    m = LSTM(8, 32, 2)
    x = torch.zeros(3, 5, 8)
    with pytest.raises(ValueError, match="2 lengths for a batch of 3"):
        m(x, None, lengths=[5, 4])
    with pytest.raises(ValueError, match="4 lengths for a batch of 3"):
        m(x, None, lengths=torch.tensor([5, 4, 3, 2]))
    with pytest.raises(ValueError, match=r"length 6 outside \[0, T = 5\]"):
        m(x, None, lengths=[5, 6, 1])
    with pytest.raises(ValueError, match=r"length -1 outside \[0, T = 5\]"):
        m(x, None, lengths=torch.tensor([5, -1, 1]))
    with pytest.raises(ValueError, match="1-d int tensor"):
        m(x, None, lengths=torch.tensor([5.0, 4.0, 1.0]))
    packed = pack_padded_sequence(x, torch.tensor([5, 4, 2]), batch_first=True)
    with pytest.raises(ValueError, match="together with a PackedSequence"):
        m(packed, None, lengths=[5, 4, 2])
    # valid lengths (0 included) and a PackedSequence pass the argument checks and reach the "GPU only" refusal
    with pytest.raises(cabi.CsnError, match="GPU only"):
        m(x, None, lengths=[5, 0, 3])
    with pytest.raises(cabi.CsnError, match="GPU only"):
        m(x, None, lengths=torch.tensor([1, 5, 5], dtype=torch.int32))
    with pytest.raises(cabi.CsnError, match="GPU only"):
        m(packed)


def test_set_lengths_is_in_the_abi_and_checked_on_the_host():
    lib = cabi.load()
    assert lib.csn_abi_version() == 6 == cabi.ABI_VERSION          # an added symbol does not bump it
    assert "csn_lstm_plan_set_lengths" in cabi.SIGNATURES
    fn = lib.csn_lstm_plan_set_lengths
    three = (ctypes.c_int32 * 3)(1, 2, 3)
    assert fn(None, three) == 1 and b"null plan" in lib.csn_last_error()
    assert fn(None, None) == 1 and b"null plan" in lib.csn_last_error()
    # the checks that need a plan: a plan is bound to a device, so they run where one can be created (and always in
    # tests/test_gpu_lstm_lengths.py::test_set_lengths_host_checks)
    d = cabi.LstmDesc(3, 5, 8, 32, 2, cabi.CSN_BF16)
    for flags, is_state in ((1, False), (1 | cabi.LSTM_STATE, True)):
        handle = ctypes.c_void_p()
        if lib.csn_lstm_plan_create(ctypes.byref(d), flags, ctypes.byref(handle)) != 0:
            assert b"hipGetDevice" in lib.csn_last_error()
            continue
        try:
            check_plan_arguments(lib, handle, is_state, T=5)
        finally:
            lib.csn_lstm_plan_destroy(handle)


def check_plan_arguments(lib, handle, is_state, T):
    """csn_lstm_plan_set_lengths on a plan of B = 3: refused without CSN_LSTM_STATE; -1 and T + 1 refused; NULL accepted."""
    fn = lib.csn_lstm_plan_set_lengths
    ok = (ctypes.c_int32 * 3)(T, 0, 1)
    if not is_state:
        assert fn(handle, ok) == 1 and b"without CSN_LSTM_STATE" in lib.csn_last_error()
        assert fn(handle, None) == 1 and b"without CSN_LSTM_STATE" in lib.csn_last_error()
        return
    assert fn(handle, ok) == 0
    assert fn(handle, (ctypes.c_int32 * 3)(T, -1, 1)) == 1 and b"lengths[1] = -1 outside [0, %d]" % T in lib.csn_last_error()
    assert fn(handle, (ctypes.c_int32 * 3)(T, 1, T + 1)) == 1 and b"lengths[2] = %d outside" % (T + 1) in lib.csn_last_error()
    assert fn(handle, None) == 0
    assert fn(handle, ok) == 0


@pytest.mark.parametrize("lengths", [(9, 3, 1, 6, 9), (9, 0, 1, 0, 4), (2, 2, 2, 2, 2)], ids=str)
@pytest.mark.parametrize("per_row", [True, False], ids=["row_by_row", "by_length"])
def test_rows_emulator_without_rounding_is_packed_nn_lstm(lengths, per_row):
    """The unmodified emulator on x[b:b+1, :n_b] with that row's state and gradients, parameter gradients summed over
    the rows, against float64 nn.LSTM on the packed batch: random h0, c0, dy, dh_n, dc_n; atol 1e-12 * max |want|."""
    B, T, I, H, L = 5, 9, 7, 8, 3
    p = olstm.init_params(I, H, L, 4, seed=5)
    lp = {k[len("lstm."):]: v for k, v in p.items() if k.startswith("lstm.")}
    rng = np.random.default_rng(6)
    x, dy = rng.standard_normal((B, T, I)), rng.standard_normal((B, T, H))
    h0, c0, dh, dc = (rng.standard_normal((L, B, H)) for _ in range(4))
    ref = torch.nn.LSTM(I, H, num_layers=L, batch_first=True).double()
    ref.load_state_dict({k: torch.from_numpy(np.asarray(v, np.float64)) for k, v in lp.items()})
    want = lref.packed_nn_lstm(ref, *(torch.from_numpy(a) for a in (x,)), lengths,
                               *(torch.from_numpy(a) for a in (h0, c0, dy, dh, dc)))
    got = lref.rows_emulator(lp, L, x, lengths, h0, c0, dy, dh, dc, rounding=False, per_row=per_row)
    assert set(got) == set(want)
    worst = 0.0
    for k, w in want.items():
        w = w.numpy()
        scale = max(float(np.abs(w).max()), 1e-30)
        worst = max(worst, float(np.abs(got[k] - w).max()) / scale)
        np.testing.assert_allclose(got[k], w, rtol=0, atol=1e-12 * scale, err_msg=k)
    print(f"rows emulator vs packed nn.LSTM {lengths}: worst difference {worst:.2e} of max |want|")
    # padding: exactly zero output and input gradient
    for b, n in enumerate(lengths):
        assert not got["out"][b, n:].any() and not got["dx"][b, n:].any()
        assert not want["out"][b, n:].numpy().any() and not want["dx"][b, n:].numpy().any()


def test_rows_emulator_with_rounding_passes_empty_rows_through():
    B, T, I, H, L = 4, 6, 7, 32, 2
    p = olstm.init_params(I, H, L, 4, seed=7)
    lp = {k[len("lstm."):]: v for k, v in p.items() if k.startswith("lstm.")}
    rng = np.random.default_rng(8)
    f32 = lambda *s: rng.standard_normal(s).astype(np.float32)      # noqa: E731
    x, dy, h0, c0, dh, dc = f32(B, T, I), f32(B, T, H), f32(L, B, H), f32(L, B, H), f32(L, B, H), f32(L, B, H)
    got = lref.rows_emulator(lp, L, x, (6, 0, 3, 0), h0, c0, dy, dh, dc)
    for b in (1, 3):
        assert np.array_equal(got["h_n"][:, b], olstm.bf16_round(h0[:, b])) and np.array_equal(got["c_n"][:, b], c0[:, b])
        assert np.array_equal(got["dh0"][:, b], dh[:, b]) and np.array_equal(got["dc0"][:, b], dc[:, b])
        assert not got["out"][b].any() and not got["dx"][b].any()
    # the other rows are the dense run of those rows alone
    alone = lref.rows_emulator(lp, L, x[[0, 2]], (6, 3), h0[:, [0, 2]], c0[:, [0, 2]], dy[[0, 2]], dh[:, [0, 2]], dc[:, [0, 2]])
    for k in lp:
        assert np.array_equal(got[k], alone[k]), k
    assert np.array_equal(got["out"][[0, 2]], alone["out"]) and np.array_equal(got["h_n"][-1, 2], got["out"][2, 2])
    none = lref.rows_emulator(lp, L, x, (0, 0, 0, 0), h0, c0, dy, dh, dc)
    assert all(not none[k].any() for k in lp) and not none["out"].any()
