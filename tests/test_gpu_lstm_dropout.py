"""GPU: the LSTM's inter-layer dropout (csn_lstm_plan_set_dropout, HipLSTM(dropout=p), LSTM.dropout = p) on every path.

One shape per path, from CASES of tests/test_gpu_lstm_state.py, plus a float32 HipLSTM shape on path 4.  The mask is fully
specified, so the references of tests/dropout_reference.py reproduce it on the CPU: bf16 plans against the bf16-faithful
emulator composed layer by layer (the bounds of oracle.compare.BF16_EMU_BOUNDS -- the emulator performs the same
roundings, so they do not depend on p), float32 plans against the unrounded composition (= a float64 nn.LSTM chain with
the same mask) within the float32 bounds of test_gpu_lstm_state.  Then the bit identities (p = 0 on a dropout plan = a
plain plan with the same launch counts, same seed = same bits, other seed or subsequence = other outputs, eval() = p = 0,
train() under no_grad = the training forward), the combinations with state, lengths and accumulating gradients, and one
CLI run.  Every case checks the plan's path and kernels and the workspace status word."""
import os

import numpy as np
import pytest
import torch

import dropout_reference as dref
import test_gpu_lstm_lengths as tl
import test_gpu_lstm_state as st
import test_lstm_dropout_cpu as cpu_checks
from cerebralsignalnetworks_amd import cabi, lstm_model
from cerebralsignalnetworks_amd.lstm_model import HipLSTM
from oracle import compare

pytestmark = pytest.mark.gpu

DEV, BF16, F32 = st.DEV, st.BF16, st.F32
P4 = (4, "lstm_fwd_f32_persist_kernel", "lstm_bwd_f32_persist_kernel")
# the LSTM (state plan) cases: one per path and form -- generic cells, per-diagonal cells with four interfaces, the
# weight-stationary forward with the per-diagonal backward, many chunks in the beside form with L = 3, the same without the
# beside GEMM, T <= chunk (a backward diagonal without a layer in range) with L = 2 and 3, the flag hand-off, the N-split
# forward, float32 cells
STATE_CASES = ("v1_h96", "p1_l5", "p2_nopersist_bwd", "chunk4_l3", "no_beside_l3", "ks_gemm_i24_t31", "t4_l3", "ks_flags",
               "ns_fused_h1024_t33", "f32_h128")
# ... and HipLSTM (a plan without CSN_LSTM_STATE) in float32: path 4, layer after layer, three layers = two interfaces
PLAIN_CASES = {"p4_f32_h128_l3": ((70, 37, 24, 128, 3), F32, P4, {})}
ALL_CASES = STATE_CASES + tuple(PLAIN_CASES)
SEED_A, SEED_B = 0x5EED0123456789AB, 0x0000000100000000 ^ 0x5EED0123456789AB      # differ in the high key word only


def _case(name, monkeypatch):
    """-> shape, dtype, expected (path, kernels), is a state (LSTM) case"""
    shape, dtype, expect, env = PLAIN_CASES[name] if name in PLAIN_CASES else st.CASES[name]
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    return shape, dtype, expect, name not in PLAIN_CASES


def _make(name, monkeypatch, seed=0):
    """The module of the case (LSTM, or HipLSTM for the plain cases), its parameters as numpy, and the arguments of
    st._make (x, h0, c0, dy, dh, dc; a plain case uses x and dy alone)."""
    shape, dtype, expect, state = _case(name, monkeypatch)
    m, _, args = st._make(shape, dtype, seed=seed)
    if not state:
        B, T, I, H, L = shape
        plain = HipLSTM(I, H, L, compute_dtype=dtype).to(DEV)
        plain.load_state_dict(m.state_dict())
        m = plain
    lp = {k: v.detach().cpu().numpy() for k, v in m.state_dict().items()}
    return shape, dtype, expect, state, m.train(), lp, args


def _seeded(m, k):
    """Seeds the CPU generator and returns the (p, seed, subsequence) the module's next forward will draw."""
    torch.manual_seed(k)
    drop = lstm_model._draw_dropout(m)
    torch.manual_seed(k)
    return drop


def _run(m, state, args):
    """State case: st._run.  Plain case: forward for every step + backward of <y_all, dy> + <y_last, dh[-1]>, under st._run's
    keys (out = y_all)."""
    if state:
        return st._run(m, *args)
    x, _, _, dy, dh, _ = args
    x = x.clone().requires_grad_(True)
    for p in m.parameters():
        p.grad = None
    y_all, y_last = m(x, want_all=True)
    ((y_all * dy).sum() + (y_last * dh[-1]).sum()).backward()
    grads = {k: p.grad.detach().clone() for k, p in m.named_parameters()}
    return dict(out=y_all.detach(), y_last=y_last.detach(), dx=x.grad, **grads)


def _reference(lp, shape, dtype, state, args, drop, lengths=None):
    """The composed emulator's answer to _run (tl._run with lengths) for the mask of `drop` = (p, seed, subsequence) or None."""
    B, T, I, H, L = shape
    masks = s = None
    if drop is not None:
        p, seed, sub = drop
        masks, s = dref.interface_masks(seed, sub, p, L, T, B, H), dref.scale(p)
    x, h0, c0, dy, dh, dc = (st._np(t) for t in args)
    rounding = dtype == BF16
    if lengths is not None:
        return dref.rows_composed_emulator(lp, L, x, lengths, h0, c0, dy, dh, dc, masks, s, rounding=rounding)
    if state:
        return dref.composed_emulator(lp, L, x, h0, c0, dy, dh, dc, masks, s, rounding=rounding)
    dy = dy.astype(np.float32).copy()
    dy[:, -1] += dh[-1].astype(np.float32)                # float32, as the library adds dy_last to the last row
    want = dref.composed_emulator(lp, L, x, None, None, dy, None, None, masks, s, rounding=rounding)
    want["y_last"] = want["out"][:, -1]
    return {k: v for k, v in want.items() if k not in ("h_n", "c_n", "dh0", "dc0")}


_F32_OUT, _F32_GRAD = 2e-5, 1e-5        # st._bounds(F32): max |difference| of the outputs, relative norm of every gradient


def _check(case, dtype, got, want):
    if dtype == BF16:
        st._emu_check(case, got, want)
        return
    line, bad = [], []
    for k, w in want.items():
        if k in ("out", "y_last", "h_n", "c_n"):
            err, bound = float(np.abs(st._np(got[k]) - w).max()), _F32_OUT
        else:
            err, bound = compare.errors(st._np(got[k]), w)[0], _F32_GRAD
        line.append(f"{k} {err:.2e}")
        if not err < bound:
            bad.append((k, err, bound))
    print(f"measured float32 vs unrounded composition {case} (outputs max |diff|, gradients rel): " + " ".join(line))
    assert not bad, (case, bad)


def _check_plans(m, expect, state, dropout_plans):
    """Every training plan of the module runs the expected path and kernels (an inference plan has no weight-stationary
    backward to name), every plan is a state plan or not as the case says, and no status word is raised."""
    for plan in m.all_plans():
        assert plan.state == state
        if plan.training:
            assert (plan.path(),) + plan.kernel_names() == expect, (plan.path(), plan.kernel_names(), expect)
        assert plan.status() == 0
    assert sorted(pl.dropout for pl in m.all_plans()) == sorted(dropout_plans), [pl.key() for pl in m.all_plans()]


@pytest.mark.parametrize("p", [0.5, 0.1])
@pytest.mark.parametrize("name", ALL_CASES)
def test_dropout_matches_the_composed_reference(name, p, monkeypatch):
    shape, dtype, expect, state, m, lp, args = _make(name, monkeypatch)
    m.dropout = p
    drop = _seeded(m, 100)
    assert drop[0] == p and drop[2] == 0
    got = _run(m, state, args)
    torch.cuda.synchronize()
    _check_plans(m, expect, state, [True])
    want = _reference(lp, shape, dtype, state, args, drop)
    assert set(want) == set(got)
    _check(f"{name} p={p}", dtype, got, want)
    # not dropped: the top layer's output, so h_n of the top layer / y_last is still the last output, bit for bit
    last = got["h_n"][-1] if state else got["y_last"]
    assert torch.equal(last, got["out"][:, -1])
    # ... and the mask is in the result: the reference WITHOUT it is far outside every bound
    off = _reference(lp, shape, dtype, state, args, None)
    assert compare.errors(st._np(got["out"]), off["out"])[0] > 0.02


# ---- bit identities at the C ABI (cabi.LstmPlan) -----------------------------------------------------------------------
def _plan_inputs(shape, seed=0):
    B, T, I, H, L = shape
    torch.manual_seed(seed)
    sd = torch.nn.LSTM(I, H, L, batch_first=True).state_dict()
    w = [[sd[f"{n}_l{k}"].to(DEV) for k in range(L)] for n in ("weight_ih", "weight_hh", "bias_ih", "bias_hh")]
    g = torch.Generator(device="cpu").manual_seed(seed + 1)
    a = dict(x=torch.randn(B, T, I, generator=g), h0=0.5 * torch.randn(L, B, H, generator=g), c0=torch.randn(L, B, H, generator=g),
             dy_last=torch.randn(B, H, generator=g), dy_all=0.1 * torch.randn(B, T, H, generator=g),
             dh_n=torch.randn(L, B, H, generator=g), dc_n=torch.randn(L, B, H, generator=g))
    return w, {k: v.to(DEV) for k, v in a.items()}


def _plan_call(plan, w, a, drop):
    """set_dropout(*drop), forward for every output, backward for every gradient (the state arguments on a state plan):
    everything on the host, and the launch / cell counts of csn_lstm_profile_read."""
    d = plan.desc
    plan.set_dropout(*drop)
    s = plan.state
    res = plan.forward(a["x"], *w, want_all=True, h0=a["h0"] if s else None, c0=a["c0"] if s else None, want_state=s)
    out = dict(zip(("y_last", "y_all", "h_n", "c_n"), res))
    out["dx"] = torch.empty(d.B, d.T, d.I, device=DEV)
    if s:
        out["dh0"], out["dc0"] = torch.empty(d.L, d.B, d.H, device=DEV), torch.empty(d.L, d.B, d.H, device=DEV)
    grads = [[torch.empty_like(p) for p in group] for group in w]
    if plan.training:
        plan.backward(a["dy_last"], a["dy_all"], grads, dx=out["dx"], dh_n=a["dh_n"] if s else None, dc_n=a["dc_n"] if s else None,
                      dh0=out.get("dh0"), dc0=out.get("dc0"))
        for n, group in zip(("weight_ih", "weight_hh", "bias_ih", "bias_hh"), grads):
            out.update({f"{n}_l{k}": t for k, t in enumerate(group)})
    else:
        out = {k: v for k, v in out.items() if k in ("y_last", "y_all", "h_n", "c_n")}
    torch.cuda.synchronize()
    prof = plan.profile_read()
    counts = tuple(prof[k] for k in ("fwd_launches", "fwd_cells", "bwd_launches", "bwd_cells"))
    return {k: v.cpu() for k, v in out.items()}, counts


def _equal(a, b, what):
    assert set(a) == set(b)
    for k in a:
        assert torch.equal(a[k], b[k]), (what, k, float((a[k] - b[k]).abs().max()))


@pytest.mark.parametrize("name", ALL_CASES)
def test_plan_bit_identities(name, monkeypatch):
    shape, dtype, expect, state = _case(name, monkeypatch)
    B, T, I, H, L = shape
    w, a = _plan_inputs(shape)
    plain = cabi.LstmPlan(B, T, I, H, L, dtype, DEV, training=True, state=state)
    plan = cabi.LstmPlan(B, T, I, H, L, dtype, DEV, training=True, state=state, dropout=True)
    for pl in (plain, plan):
        pl.profile_enable(True)
        assert (pl.path(),) + pl.kernel_names() == expect, (pl.path(), pl.kernel_names())
    per = -(-(T * B * H * (2 if dtype == BF16 else 4)) // 256) * 256
    lib = cabi.load()
    assert lib.csn_lstm_plan_workspace_bytes(plan._plan) - lib.csn_lstm_plan_workspace_bytes(plain._plan) == (L - 1) * per
    assert plan.key() == plain.key() + ("dropout plan",)
    # p = 0 on a dropout plan: a plain plan, in every output and gradient and in what it launches
    base, base_counts = _plan_call(plain, w, a, (0.0, 0, 0))
    off, off_counts = _plan_call(plan, w, a, (0.0, SEED_A, 0))
    _equal(base, off, "p = 0 against a plain plan")
    assert off_counts == base_counts, (off_counts, base_counts)
    assert expect[0] == 0 or (base_counts[0] > 0 and base_counts[2] > 0)      # (the generic cells of path 0 count nothing)
    # the same (seed, subsequence) twice: the same bits; another seed, or another subsequence: another mask
    on, on_counts = _plan_call(plan, w, a, (0.5, SEED_A, 0))
    again, _ = _plan_call(plan, w, a, (0.5, SEED_A, 0))
    _equal(on, again, "the same seed twice")
    assert on_counts == base_counts                         # the recurrence launches are those of a plain plan
    other_seed, _ = _plan_call(plan, w, a, (0.5, SEED_B, 0))
    other_sub, _ = _plan_call(plan, w, a, (0.5, SEED_A, 1))
    for k in ("y_all", "dx", "weight_ih_l1", "weight_hh_l0"):
        for r in (off, other_seed, other_sub):
            assert not torch.equal(on[k], r[k]), k
        assert not torch.equal(other_seed[k], other_sub[k]), k
    # y_all, y_last and h_n[L-1] agree as they do without dropout
    assert torch.equal(on["y_all"][:, -1], on["y_last"])
    if state:
        assert torch.equal(on["h_n"][-1], on["y_last"])
    # p = 1: everything dropped -- the layers above the first see zeros, and no gradient reaches the first through them
    ones, _ = _plan_call(plan, w, a, (1.0, SEED_A, 0))
    assert not ones["weight_ih_l1"].any() and all(torch.isfinite(v).all() for v in ones.values())
    if not state:
        assert not ones["dx"].any() and not ones["weight_hh_l0"].any()
    # the setting is all there is: p = 0 again leaves nothing behind
    _equal(base, _plan_call(plan, w, a, (0.0, 0, 0))[0], "p = 0 after p > 0")
    # an inference plan with the bit: the training forward's outputs
    infer = cabi.LstmPlan(B, T, I, H, L, dtype, DEV, training=False, state=state, dropout=True)
    fwd, _ = _plan_call(infer, w, a, (0.5, SEED_A, 0))
    _equal(fwd, {k: on[k] for k in fwd}, "inference plan")
    assert [pl.status() for pl in (plain, plan, infer)] == [0, 0, 0]


@pytest.mark.parametrize("name", ALL_CASES)
def test_module_modes(name, monkeypatch):
    shape, dtype, expect, state, m, lp, args = _make(name, monkeypatch, seed=2)
    m.dropout = 0.5
    _seeded(m, 7)
    train = _run(m, state, args)
    # train() under no_grad: dropout is active as in torch -- the training forward's output for the same seed
    _seeded(m, 7)
    with torch.no_grad():
        out_ng = m(args[0], (args[1], args[2]))[0] if state else m(args[0], want_all=True)[0]
    assert torch.equal(out_ng, train["out"])
    # eval() = p = 0 = a module that never heard of dropout, and it draws nothing from the generator
    m.eval()
    rng = torch.get_rng_state()
    evaluated = _run(m, state, args)
    assert torch.equal(torch.get_rng_state(), rng)
    m.train()
    m.dropout = 0.0
    zero = _run(m, state, args)
    for k in zero:
        assert torch.equal(evaluated[k], zero[k]), k
    assert not torch.equal(train["out"], zero["out"])
    torch.cuda.synchronize()
    # plans: a training and an inference one with the bit, one plain training plan for eval() and p = 0 together
    _check_plans(m, expect, state, [True, True, False])
    assert sorted(pl.training for pl in m.all_plans() if pl.dropout) == [False, True]


# ---- combinations on LSTM, the value set as the attribute --------------------------------------------------------------
@pytest.mark.parametrize("pattern", ["random_with_zeros", "chunk_edges"])
@pytest.mark.parametrize("name", ["v1_h96", "p1_l5", "chunk4_l3", "no_beside_l3", "f32_h128"])
def test_dropout_with_lengths(name, pattern, monkeypatch):
    shape, dtype, expect, state, m, lp, args = _make(name, monkeypatch, seed=1)
    T = shape[1]
    case = dict(tl.CASES)
    case.setdefault(name, st.CASES[name] + ((31, 32, 33),))
    monkeypatch.setattr(tl, "CASES", case)
    lengths = tl._lengths(name, pattern)
    assert T in lengths and len(set(lengths)) >= 2
    m.dropout = 0.5
    drop = _seeded(m, 31)
    got = tl._run(m, args, lengths)
    torch.cuda.synchronize()
    _check_plans(m, expect, True, [True])
    for b, n in enumerate(lengths):
        assert not got["out"][b, n:].any() and not got["dx"][b, n:].any(), (name, pattern, b)
        if n > 0:
            assert torch.equal(got["h_n"][-1, b], got["out"][b, n - 1]), (name, pattern, b)
    # NaN / Inf in the padding of x and dy: the same bits (the mask is the one of the call without lengths: same seed)
    _seeded(m, 31)
    tl._same_bits(got, tl._run(m, args, lengths, nan_padding=True), f"{name} {pattern} NaN padding")
    # each group of rows of one length against the composed emulator on its valid steps, with its rows of the mask
    _check(f"{name} {pattern} p=0.5", dtype, got, _reference(lp, shape, dtype, True, args, drop, lengths=lengths))


@pytest.mark.parametrize("name", ["v1_h96", "chunk4_l3", "f32_h128"])
def test_accumulating_gradients_over_two_masks(name, monkeypatch):
    """direct_grads = "accumulate": two forwards of one step, each with the mask of its own seed, summed in the library --
    the sum of the two backwards run apart, each with its forward's mask (kept on its autograd node)."""
    shape, dtype, expect, state, m, lp, args = _make(name, monkeypatch, seed=5)
    x, h0, c0, dy, dh, dc = args
    x2 = x.flip(0)
    m.dropout = 0.5

    def one(inp, first):
        torch.manual_seed(9)
        if not first:
            lstm_model._draw_dropout(m)          # the second forward of the step draws the second seed
        out, (h_n, c_n) = m(inp, (h0, c0))
        return (out * dy).sum() + (h_n * dh).sum() + (c_n * dc).sum()

    apart = []
    for inp, first in ((x, True), (x2, False)):
        for p in m.parameters():
            p.grad = None
        one(inp, first).backward()
        apart.append({k: p.grad.clone() for k, p in m.named_parameters()})
    assert not torch.equal(apart[0]["weight_ih_l1"], apart[1]["weight_ih_l1"])
    m.direct_grads = "accumulate"
    for p in m.parameters():
        p.grad = torch.zeros_like(p)
    held = {k: p.grad for k, p in m.named_parameters()}
    torch.manual_seed(9)
    out1, (h1, c1) = m(x, (h0, c0))
    out2, (h2, c2) = m(x2, (h0, c0))
    assert sum(pl.busy for pl in m.all_plans()) == 2
    ((out1 * dy).sum() + (h1 * dh).sum() + (c1 * dc).sum() + (out2 * dy).sum() + (h2 * dh).sum() + (c2 * dc).sum()).backward()
    torch.cuda.synchronize()
    for k, p in m.named_parameters():
        assert p.grad is held[k]                 # added to in place
        assert torch.equal(p.grad, apart[0][k] + apart[1][k]), (name, k)
    _check_plans(m, expect, True, [True, True])


def test_set_dropout_host_checks():
    lib = cabi.load()
    for has_bit, kw in ((False, dict()), (True, dict(dropout=True)), (True, dict(dropout=True, state=True)), (False, dict(state=True))):
        plan = cabi.LstmPlan(3, 5, 8, 32, 2, BF16, DEV, training=True, **kw)
        cpu_checks.check_plan_arguments(lib, plan._plan, has_bit)
        with pytest.raises(cabi.CsnError, match="outside"):
            plan.set_dropout(1.5, 1)
        if not has_bit:
            with pytest.raises(cabi.CsnError, match="without CSN_LSTM_DROPOUT"):
                plan.set_dropout(0.5, 1)
        plan.set_dropout(0.0)
    # a single layer: the bit costs nothing and p > 0 does nothing
    w, a = _plan_inputs((4, 6, 8, 32, 1))
    one = cabi.LstmPlan(4, 6, 8, 32, 1, BF16, DEV, training=True, dropout=True)
    ref = cabi.LstmPlan(4, 6, 8, 32, 1, BF16, DEV, training=True)
    assert lib.csn_lstm_plan_workspace_bytes(one._plan) == lib.csn_lstm_plan_workspace_bytes(ref._plan)
    _equal(_plan_call(one, w, a, (0.5, 1, 0))[0], _plan_call(ref, w, a, (0.0, 0, 0))[0], "L = 1")


def test_cli_train_with_lstm_dropout(tmp_path, monkeypatch):
    import LstmDistillFromDinoV2Train as train
    plans, settings = [], []
    init, set_dropout = cabi.LstmPlan.__init__, cabi.LstmPlan.set_dropout

    def recording_init(self, *a, **kw):
        init(self, *a, **kw)
        plans.append(self)

    def recording_set(self, p, seed=0, subsequence=0):
        settings.append((self.training, p, seed))
        set_dropout(self, p, seed, subsequence)
    monkeypatch.setattr(cabi.LstmPlan, "__init__", recording_init)
    monkeypatch.setattr(cabi.LstmPlan, "set_dropout", recording_set)
    hist = train.main(["--synthetic", "256", "--batch_size", "16", "--num_epochs", "1", "--log_dir", str(tmp_path),
                       "--hidden_size", "128", "--lstm_layers", "2", "--loss", "cosine", "--lstm_dropout", "0.3"])
    torch.cuda.synchronize()
    assert len(hist) == 1 and np.isfinite(hist[0]) and 0.5 < hist[0] < 1.5      # cosine loss vs random targets ~ 1
    assert os.path.exists(os.path.join(str(tmp_path), "lstm_dinov2_best_loss.pth"))
    assert plans and all(pl.dropout and pl.training for pl in plans) and all(pl.status() == 0 for pl in plans)
    on = [s for s in settings if s[1] > 0]
    assert len(on) == len(settings) and all(s[1] == 0.3 for s in on)
    seeds = [s[2] for s in on]
    assert len(set(seeds)) == len(seeds) // 2        # one seed per step, set for the forward and again for its backward
