"""GPU: variable-length LSTM batches -- LSTM.forward(x, hx, lengths=...), PackedSequence input, csn_lstm_plan_set_lengths.

One shape per path (from CASES of tests/test_gpu_lstm_state.py) x a set of length patterns: against float64 nn.LSTM on
the packed batch, against the bf16-faithful emulator run on each row's valid steps alone (tests/lengths_reference.py),
and the bit-exact identities (all T = no lengths, the valid prefix of a ragged call = the dense call, NaN padding = zero
padding, a dense call after a ragged one = a fresh plan, PackedSequence = lengths).  Ragged recordings chained through
their state with accumulating gradients, and the launch / cell counts of a short batch inside a long plan.  Every case
checks the plan's path and kernels and the workspace status word."""
import numpy as np
import pytest
import torch
from torch.nn.utils.rnn import pack_padded_sequence

import lengths_reference as lref
import test_gpu_lstm_state as st
import test_lstm_lengths_cpu as cpu_checks
from cerebralsignalnetworks_amd import cabi, LSTM

pytestmark = pytest.mark.gpu

DEV, BF16, F32 = st.DEV, st.BF16, st.F32

# name: (shape, compute dtype, expected (path, forward kernel, backward kernel), environment, chunk edges): the plan a
# call WITHOUT lengths takes for the shape -- no shape here needs the fall-back of the masked weight-stationary backward
# to lstm_cell_bwd_il_kernel (every masked instantiation builds without scratch)
_KS70 = ((256, 70, 128, 768, 2),) + st.CASES["ks_fused_h768_t32"][1:]      # T raised to 70: three chunks
CASES = {name: (st.CASES[name] if name != "ks_fused_h768" else _KS70) + ((3, 4, 5) if name == "chunk4_l3" else (31, 32, 33),)
         for name in ("v1_h96", "v1_h256_ks", "p1_l5", "p2_nopersist_bwd", "ks_fused_h768", "ns_fused_h1024_t33", "chunk4_l3",
                      "ks_flags", "f32_h128", "ref_h128_l4")}
PATTERNS = ("all_T", "all_1", "random_1_T", "random_with_zeros", "chunk_edges", "single_long", "all_0")
# B T H >= 1e6: the patterns that keep the CPU references affordable (the two the ragged paths depend on most, and the
# two whose references cost nothing)
LARGE_PATTERNS = ("random_with_zeros", "chunk_edges", "all_1", "all_0")


def _patterns(name):
    B, T, _, H, _ = CASES[name][0]
    return PATTERNS if B * T * H < 1e6 else LARGE_PATTERNS


def _lengths(name, pattern, seed=0):
    (B, T, *_), edges = CASES[name][0], CASES[name][4]
    rng = np.random.default_rng(1000 + seed)
    if pattern == "all_T":
        n = [T] * B
    elif pattern == "all_1":
        n = [1] * B
    elif pattern == "all_0":
        n = [0] * B
    elif pattern == "random_1_T":
        n = rng.integers(1, T + 1, B).tolist()
    elif pattern == "random_with_zeros":
        n = rng.integers(0, T + 1, B).tolist()
        n[0], n[1], n[B - 1] = T, 0, 0
    elif pattern == "chunk_edges":
        vals = [e for e in edges if e <= T] + [T, T - 1]
        n = [vals[i % len(vals)] for i in rng.permutation(B)]
    elif pattern == "single_long":
        n = rng.integers(1, 4, B).tolist()
        n[B // 2] = T
    return [int(v) for v in n]


def _bounds(dtype):
    # the values of tests/test_gpu_lstm_state.py::_bounds, used as there: (max |difference| of out, h_n, c_n;
    # relative-norm error of every gradient).  bf16: as test_fast_path_matches_oracle_and_v1; float32: as
    # test_f32_weight_stationary_recurrence
    return (3e-2, 4e-2) if dtype == BF16 else (2e-5, 1e-5)


def _run(m, args, lengths, nan_padding=False):
    """forward with state and lengths + backward of <out,dy> + <h_n,dh> + <c_n,dc>: outputs and every gradient."""
    x, h0, c0, dy, dh, dc = (t.clone() for t in args)
    if nan_padding:
        for b, n in enumerate(lengths):
            x[b, n:] = float("nan") if b % 2 else float("inf")
            dy[b, n:] = float("inf") if b % 2 else float("nan")
    x.requires_grad_(True), h0.requires_grad_(True), c0.requires_grad_(True)
    for p in m.parameters():
        p.grad = None
    out, (h_n, c_n) = m(x, (h0, c0)) if lengths is None else m(x, (h0, c0), lengths=lengths)
    torch.autograd.backward([out, h_n, c_n], [dy, dh, dc])
    grads = {k: p.grad.detach().clone() for k, p in m.named_parameters()}
    return dict(out=out.detach(), h_n=h_n.detach(), c_n=c_n.detach(), dx=x.grad, dh0=h0.grad, dc0=c0.grad, **grads)


def _same_bits(a, b, what):
    for k in a:
        assert torch.equal(a[k], b[k]), (what, k, float((a[k] - b[k]).abs().max()))


def _check_plan(m, expect):
    st._check_plan(m, expect)


def _setup(name, monkeypatch, seed=0):
    shape, dtype, expect, env, _ = CASES[name]
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    m, ref, args = st._make(shape, dtype, seed=seed)
    return shape, dtype, expect, m, ref.cpu(), args


@pytest.mark.parametrize("name,pattern", [(n, p) for n in CASES for p in _patterns(n)])
def test_ragged_matches_packed_nn_lstm_and_row_emulator(name, pattern, monkeypatch):
    shape, dtype, expect, m, ref, args = _setup(name, monkeypatch)
    B, T, I, H, L = shape
    lengths = _lengths(name, pattern)
    got = _run(m, args, lengths)
    torch.cuda.synchronize()
    _check_plan(m, expect)
    # (1) float64 nn.LSTM on the packed batch, on the CPU
    want = lref.packed_nn_lstm(ref, *(t.double().cpu() for t in args[:1]), lengths, *(t.double().cpu() for t in args[1:]))
    elem, rel = _bounds(dtype)
    line = []
    for k, w in want.items():
        g = got[k].double().cpu()
        if k in ("out", "h_n", "c_n"):
            err = float((g - w).abs().max())
            line.append(f"{k} {err:.2e}")
            assert err < elem, (name, pattern, k, err)
        elif float(w.norm()) == 0.0:            # (all rows empty: no gradient reaches x or a parameter)
            assert not g.any(), (name, pattern, k)
        else:
            r = float((g - w).norm() / w.norm())
            line.append(f"{k} {r:.2e}")
            assert r < rel, (name, pattern, k, r)
    print(f"measured vs float64 packed nn.LSTM {name} {pattern}: " + " ".join(line))
    # (3) bit-exact: zeros over the padding, the valid prefix of the dense call, h_n of the top layer = the last output
    dense = _run(m, args, None)
    for b, n in enumerate(lengths):
        assert not got["out"][b, n:].any() and not got["dx"][b, n:].any(), (name, pattern, b)
        assert torch.equal(got["out"][b, :n], dense["out"][b, :n]), (name, pattern, b)
        if n > 0:
            assert torch.equal(got["h_n"][-1, b], got["out"][b, n - 1]), (name, pattern, b)
    # ... NaN / Inf in the padding of x and dy: the same bits as zeros there
    _same_bits(got, _run(m, args, lengths, nan_padding=True), f"{name} {pattern} NaN padding")
    # ... an inference forward with lengths: the training forward's bits
    with torch.no_grad():
        out_i, (h_i, c_i) = m(args[0], (args[1], args[2]), lengths=torch.tensor(lengths))
    assert torch.equal(out_i, got["out"]) and torch.equal(h_i, got["h_n"]) and torch.equal(c_i, got["c_n"])
    assert [pl.status() for pl in m.all_plans() if not pl.training] == [0]
    # (2) bf16: the emulator on each row's valid steps (one run per distinct length, no row left out)
    if dtype == BF16:
        lp = {k: v.detach().cpu().numpy() for k, v in m.state_dict().items()}
        emu = lref.rows_emulator(lp, L, *(st._np(t) for t in args[:1]), lengths, *(st._np(t) for t in args[1:]))
        if not any(lengths):        # nothing ran: every result is exact (compare.errors divides by max |want| = 0)
            for k, w in emu.items():
                assert np.array_equal(st._np(got[k]), w), (name, pattern, k)
        else:
            st._emu_check(f"{name} {pattern}", got, emu)


@pytest.mark.parametrize("name", list(CASES))
def test_all_T_is_no_lengths_and_a_dense_call_after_a_ragged_one_is_a_fresh_plan(name, monkeypatch):
    shape, dtype, expect, m, _, args = _setup(name, monkeypatch, seed=2)
    B, T, I, H, L = shape
    dense = _run(m, args, None)
    _same_bits(dense, _run(m, args, [T] * B), f"{name} all T")
    _run(m, args, _lengths(name, "random_with_zeros", seed=2))
    _run(m, args, [0] * B)
    after = _run(m, args, None)
    fresh = LSTM(I, H, L, compute_dtype=dtype).to(DEV)
    fresh.load_state_dict(m.state_dict())
    _same_bits(after, _run(fresh, args, None), f"{name} fresh plan")
    _same_bits(after, dense, f"{name} before / after")
    assert len(m.all_plans()) == 1           # lengths are per call, not part of the plan key
    _check_plan(m, expect)


@pytest.mark.parametrize("name", ["v1_h96", "p1_l5", "ks_flags", "chunk4_l3", "f32_h128"])
@pytest.mark.parametrize("enforce_sorted", [False, True])
def test_packed_sequence_is_lengths_on_the_padded_tensor(name, enforce_sorted, monkeypatch):
    shape, dtype, expect, m, _, (x, h0, c0, dy, dh, dc) = _setup(name, monkeypatch, seed=3)
    B, T = shape[:2]
    lengths = _lengths(name, "random_1_T", seed=3)
    lengths[B // 3] = lengths[B // 3 + 1] = T           # the longest row (so that the padded tensor has T steps), twice
    if enforce_sorted:
        lengths = sorted(lengths, reverse=True)
    lens = torch.tensor(lengths)

    def run(packed_input):
        xr = x.clone().requires_grad_(True)
        for p in m.parameters():
            p.grad = None
        if packed_input:
            inp = pack_padded_sequence(xr, lens, batch_first=True, enforce_sorted=enforce_sorted)
            out, (h_n, c_n) = m(inp, (h0, c0))
            assert isinstance(out, torch.nn.utils.rnn.PackedSequence)
            assert torch.equal(out.batch_sizes, inp.batch_sizes)
            for a, b in ((out.sorted_indices, inp.sorted_indices), (out.unsorted_indices, inp.unsorted_indices)):
                assert (a is None and b is None) or torch.equal(a, b)
            data = out.data
        else:
            out, (h_n, c_n) = m(xr, (h0, c0), lengths=lens)
            data = pack_padded_sequence(out, lens, batch_first=True, enforce_sorted=enforce_sorted).data
        g = torch.Generator(device="cpu").manual_seed(9)
        w = torch.randn(data.shape, generator=g).to(DEV)
        torch.autograd.backward([data, h_n, c_n], [w, dh, dc])
        return dict(data=data.detach(), h_n=h_n.detach(), c_n=c_n.detach(), dx=xr.grad,
                    **{k: p.grad.detach().clone() for k, p in m.named_parameters()})

    _same_bits(run(True), run(False), f"{name} packed")
    _check_plan(m, expect)


@pytest.mark.parametrize("name", ["v1_h96", "p1_l5", "chunk4_l3", "ks_flags", "f32_h128"])
def test_chained_ragged_recordings_accumulate(name, monkeypatch):
    """Recordings of different duration, three chunks chained through (h_n, c_n), gradients accumulated in place: the rows
    end in chunks 1, 2 and 3, one of them exactly on a chunk end (the next chunk sees n = 0 for it)."""
    (B, Tc, I, H, L), dtype, expect, env, _ = CASES[name]
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    m, ref, (x, h0, c0, dy, dh, dc) = st._make((B, 3 * Tc, I, H, L), dtype, seed=5)
    ref = ref.cpu()
    rng = np.random.default_rng(55)
    full = rng.integers(1, 3 * Tc + 1, B).tolist()
    full[:5] = [Tc, 2 * Tc, 3 * Tc, Tc // 2, Tc + 1]      # ends on both inner chunk ends, at the very end, inside chunks 1 and 2
    m.direct_grads = "accumulate"
    for p in m.parameters():
        p.grad = torch.zeros_like(p)
    xr, h0r, c0r = (t.clone().requires_grad_(True) for t in (x, h0, c0))
    outs, state = [], (h0r, c0r)
    for k in range(3):
        lens = [min(max(n - k * Tc, 0), Tc) for n in full]
        assert k == 0 or 0 in lens
        out, state = m(xr[:, k * Tc:(k + 1) * Tc], state, lengths=lens)
        outs.append(out)
    out = torch.cat(outs, 1)
    torch.autograd.backward([out, state[0], state[1]], [dy, dh, dc])
    torch.cuda.synchronize()
    got = dict(out=out.detach(), h_n=state[0].detach(), c_n=state[1].detach(), dx=xr.grad, dh0=h0r.grad, dc0=c0r.grad,
               **{k: p.grad.detach().clone() for k, p in m.named_parameters()})
    st._check_plans(m.all_plans(), expect, Tc)
    # forward: the bits of one call over the whole length with the full lengths
    m.direct_grads = False
    whole = _run(m, (x, h0, c0, dy, dh, dc), full)
    for k in ("out", "h_n", "c_n"):
        assert torch.equal(got[k], whole[k]), (name, k, float((got[k] - whole[k]).abs().max()))
    # gradients: float64 packed nn.LSTM over the whole length
    want = lref.packed_nn_lstm(ref, x.double().cpu(), full, *(t.double().cpu() for t in (h0, c0, dy, dh, dc)))
    _, rel = _bounds(dtype)
    line = []
    for k, w in want.items():
        if k in ("out", "h_n", "c_n"):
            continue
        r = float((got[k].double().cpu() - w).norm() / w.norm())
        line.append(f"{k} {r:.2e}")
        assert r < rel, (name, k, r)
    print(f"measured chained ragged {name} vs float64 packed nn.LSTM: " + " ".join(line))


@pytest.mark.parametrize("longest", [20, 50])
def test_work_follows_the_longest_row(longest, monkeypatch):
    """ks_fused_h768 (T = 70, chunks of 32): a batch whose longest row has 20 steps (one chunk) or 50 (two) launches and
    computes what a plan created with T = longest does.  Observed on MI355X: the shorter plan takes the same kernels and
    the forward is bit-identical (asserted); the gradients are compared within the bounds of check 1."""
    shape, dtype, expect, m, _, args = _setup("ks_fused_h768", monkeypatch, seed=6)
    B, T, I, H, L = shape
    lengths = np.random.default_rng(66).integers(0, longest + 1, B).tolist()
    lengths[3] = longest
    short = LSTM(I, H, L, compute_dtype=dtype).to(DEV)
    short.load_state_dict(m.state_dict())
    cut = tuple(t[:, :longest].contiguous() if t.dim() == 3 and t.shape[1] == T else t for t in args)
    prof = {}
    for tag, mod, a in (("long", m, args), ("short", short, cut)):
        _run(mod, a, lengths)                      # creates the plan
        (plan,) = mod.all_plans()
        plan.profile_enable(True)
        res = _run(mod, a, lengths)
        torch.cuda.synchronize()
        prof[tag] = (plan.profile_read(), res, plan)
    _check_plan(m, expect)
    assert prof["long"][2].desc.T == T and prof["short"][2].desc.T == longest
    assert prof["short"][2].kernel_names() == prof["long"][2].kernel_names() == expect[1:]
    for k in ("fwd_launches", "fwd_cells", "bwd_launches", "bwd_cells"):
        assert prof["long"][0][k] == prof["short"][0][k] > 0, (k, prof["long"][0], prof["short"][0])
    got, want = prof["long"][1], prof["short"][1]
    assert torch.equal(got["out"][:, :longest], want["out"]) and not got["out"][:, longest:].any()
    assert torch.equal(got["h_n"], want["h_n"]) and torch.equal(got["c_n"], want["c_n"])
    assert not got["dx"][:, longest:].any()
    _, rel = _bounds(dtype)
    for k, w in want.items():
        if k in ("out", "h_n", "c_n"):
            continue
        g = got[k][:, :longest] if k == "dx" else got[k]
        r = float((g.double() - w.double()).norm() / w.double().norm())
        assert r < rel, (k, r)
    # every row empty: no recurrence launch at all
    plan = prof["long"][2]
    _run(m, args, [0] * B)
    torch.cuda.synchronize()
    assert all(v == 0 for v in plan.profile_read().values())


def test_set_lengths_host_checks():
    lib = cabi.load()
    for state in (False, True):
        plan = cabi.LstmPlan(3, 5, 8, 32, 2, BF16, DEV, training=True, state=state)
        cpu_checks.check_plan_arguments(lib, plan._plan, state, T=5)
    plan = cabi.LstmPlan(3, 5, 8, 32, 2, BF16, DEV, training=True, state=True)
    with pytest.raises(cabi.CsnError, match="2 entries for a batch of 3"):
        plan.set_lengths([1, 2])
    with pytest.raises(cabi.CsnError, match="outside"):
        plan.set_lengths(torch.tensor([1, 2, 6]))
    plan.set_lengths(torch.tensor([1, 0, 5]))
    plan.set_lengths(None)
    m = LSTM(8, 32, 2).to(DEV)
    with pytest.raises(ValueError, match="pass CPU lengths"):
        m(torch.zeros(3, 5, 8, device=DEV), None, lengths=torch.tensor([5, 4, 3], device=DEV))
    assert not m.all_plans()                 # refused before any plan or launch
