"""GPU: CSN_GRAD_ACCUMULATE (csn_lstm_plan_set_grad_mode) and what is built on it.

Through the C ABI, one plan per path: in accumulate mode every element of dw_ih / dw_hh / db_ih / db_hh becomes
fl32(prev + g), g being the bits the overwrite mode stores -- torch.equal against torch's own float32 sum; dx, dh0 and dc0
are overwritten in both modes; a second accumulate adds again; back in overwrite mode the bits of g return; the
gradient-ready callback keeps its order.  Then the modules (direct accumulation against autograd's accumulation of
temporaries: two views, micro-batches, chunks of a recording), the trainer's accum_steps, and the CLIs.  Every plan's path,
kernels and status word are checked."""
import contextlib
import os

import numpy as np
import pytest
import torch

from cerebralsignalnetworks_amd import cabi, LSTM, Model, CosineSimilarityLoss
from cerebralsignalnetworks_amd.trainer import DistillTrainer

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda:0")
BF16, F32 = torch.bfloat16, torch.float32
V1 = (0, "lstm_cell_fwd_kernel", "lstm_cell_bwd_kernel")
V1_KS = (0, "lstm_cell_fwd_ks_kernel", "lstm_cell_bwd_ks_kernel")
IL = (1, "lstm_cell_fwd_il_kernel", "lstm_cell_bwd_il_kernel")
_PF, _NSF, _PB, _ILB = "lstm_fwd_persist_kernel", "lstm_fwd_ns_kernel", "lstm_bwd_persist_kernel", "lstm_cell_bwd_il_kernel"
P2 = (2, _PF, _ILB)
P3 = (3, _PF, _PB)
P3_NS = (3, _NSF, _PB)
F32P = (4, "lstm_fwd_f32_persist_kernel", "lstm_bwd_f32_persist_kernel")

# name: ((B, T, I, H, L), compute dtype, (path, forward kernel, backward kernel), environment, CSN_LSTM_STATE plan).
# The state plans are those of test_gpu_lstm_state.CASES; f32_persist is the stateless float32 shape that
# test_gpu_parity.test_f32_weight_stationary_path_is_the_one_that_runs shows on path 4.
CASES = {
    "v1_h96": ((8, 40, 24, 96, 2), BF16, V1, {}, True),
    "f32_cell_v1": ((20, 17, 24, 96, 2), F32, V1, {"CSN_CELL_V1": "1"}, True),
    "f32_h128": ((70, 37, 24, 128, 2), F32, V1_KS, {}, True),
    "p1_env": ((16, 40, 32, 128, 2), BF16, IL, {"CSN_NO_PERSIST": "1"}, True),
    "p1_l5": ((8, 30, 16, 128, 5), BF16, IL, {}, True),
    "p2_nopersist_bwd": ((64, 40, 128, 768, 2), BF16, P2, {"CSN_NO_PERSIST_BWD": "1"}, True),
    "ks_fused_h768_t32": ((256, 32, 128, 768, 2), BF16, P3, {}, True),
    "ks_flags": ((64, 40, 128, 768, 2), BF16, P3, {"CSN_FWD_FLAGS": "1", "CSN_BWD_FLAGS": "1"}, True),
    "ns_fused_h1024_t33": ((65, 33, 128, 1024, 2), BF16, P3_NS, {}, True),
    "t1": ((65, 1, 32, 256, 2), BF16, P3, {}, True),
    "chunk4_l3": ((64, 23, 32, 256, 3), BF16, P3, {"CSN_LSTM_CHUNK": "4"}, True),
    "f32_persist": ((4, 12, 16, 128, 2), F32, F32P, {}, False),
}
_GROUPS = ("weight_ih", "weight_hh", "bias_ih", "bias_hh")


def _rel(got, want):
    return float((got.double() - want).norm() / max(float(want.norm()), 1e-30))


class _Case:
    """One plan of CASES[name], its parameters, random inputs for every argument, seeded `prev` contents for the 4 L
    gradient tensors (db_ih and db_hh different) and garbage for dx / dh0 / dc0."""

    def __init__(self, name, monkeypatch):
        shape, dtype, self.expect, env, self.state = CASES[name]
        for k, v in env.items():
            monkeypatch.setenv(k, v)
        B, T, I, H, L = shape
        self.L = L
        torch.manual_seed(0)
        ref = torch.nn.LSTM(I, H, L, batch_first=True)
        self.w = [[getattr(ref, f"{n}_l{k}").detach().to(DEV) for k in range(L)] for n in _GROUPS]
        g = torch.Generator(device="cpu").manual_seed(1)
        rnd = lambda *s: torch.randn(*s, generator=g).to(DEV)      # noqa: E731
        self.x, self.dy = rnd(B, T, I), rnd(B, T, H)
        self.h0, self.c0, self.dh_n, self.dc_n = 0.5 * rnd(L, B, H), rnd(L, B, H), rnd(L, B, H), rnd(L, B, H)
        self.prev = [[rnd(*p.shape) for p in group] for group in self.w]
        self.shape = shape
        self.plan = cabi.LstmPlan(B, T, I, H, L, dtype, DEV, training=True, state=self.state)

    def run(self, grads):
        """forward + backward into `grads`; -> (dx, dh0, dc0), each pre-filled with garbage (dh0 / dc0: state plans)."""
        B, T, I, H, L = self.shape
        st = dict(h0=self.h0, c0=self.c0, want_state=True) if self.state else {}
        self.plan.forward(self.x, *self.w, want_all=True, **st)
        dx = torch.full((B, T, I), float("nan"), device=DEV)
        dh0 = torch.full((L, B, H), float("nan"), device=DEV) if self.state else None
        dc0 = torch.full((L, B, H), -7.0, device=DEV) if self.state else None
        bw = dict(dh_n=self.dh_n, dc_n=self.dc_n, dh0=dh0, dc0=dc0) if self.state else {}
        self.plan.backward(None, self.dy, grads, dx=dx, **bw)
        torch.cuda.synchronize()
        return [t for t in (dx, dh0, dc0) if t is not None]

    def overwrite(self):
        """-> (g, others): the gradients of overwrite mode, written over garbage."""
        self.plan.set_grad_mode(False)
        g = [[torch.full_like(p, float("nan")) for p in group] for group in self.w]
        return g, self.run(g)

    def check(self):
        got = (self.plan.path(),) + self.plan.kernel_names()
        assert got == self.expect, (got, self.expect)
        assert self.plan.state == self.state
        assert self.plan.status() == 0


def _assert_contract(c, g, others, acc, others_acc, prev):
    for n, gg, ga, gp in zip(_GROUPS, g, acc, prev):
        for l, (a, b, p) in enumerate(zip(gg, ga, gp)):
            assert torch.isfinite(a).all(), (n, l)
            assert torch.equal(b, p + a), (n, l, float((b - (p + a)).abs().max()))
    assert len(others) == (3 if c.state else 1)
    for a, b in zip(others, others_acc):       # dx, dh0, dc0: overwritten in both modes
        assert torch.isfinite(a).all() and torch.equal(a, b)


@pytest.mark.parametrize("name", list(CASES))
def test_accumulate_is_prev_plus_the_overwrite_bits(name, monkeypatch):
    c = _Case(name, monkeypatch)
    g, others = c.overwrite()
    acc = [[p.clone() for p in group] for group in c.prev]
    assert not torch.equal(c.prev[2][0], c.prev[3][0])             # db_ih and db_hh start from different contents
    c.plan.set_grad_mode(True)
    others_acc = c.run(acc)
    _assert_contract(c, g, others, acc, others_acc, c.prev)
    c.check()


@pytest.mark.parametrize("name", list(CASES))
def test_second_accumulate_adds_again_and_overwrite_returns(name, monkeypatch):
    c = _Case(name, monkeypatch)
    g, _ = c.overwrite()
    acc = [[p.clone() for p in group] for group in c.prev]
    c.plan.set_grad_mode(True)
    c.run(acc)
    c.run(acc)                                                     # sticky: no second set_grad_mode
    for n, gg, ga, gp in zip(_GROUPS, g, acc, c.prev):
        for l, (a, b, p) in enumerate(zip(gg, ga, gp)):
            assert torch.equal(b, (p + a) + a), (n, l)
    c.plan.set_grad_mode(False)
    c.run(acc)
    for n, gg, ga in zip(_GROUPS, g, acc):
        for l, (a, b) in enumerate(zip(gg, ga)):
            assert torch.equal(a, b), (n, l)
    c.check()


@pytest.mark.parametrize("name", list(CASES))
def test_accumulate_with_the_gradient_ready_callback(name, monkeypatch):
    c = _Case(name, monkeypatch)
    g, others = c.overwrite()
    calls = []
    c.plan.set_grad_callback(calls.append)
    acc = [[p.clone() for p in group] for group in c.prev]
    c.plan.set_grad_mode(True)
    others_acc = c.run(acc)
    assert calls == list(range(c.L - 1, -1, -1)), calls
    _assert_contract(c, g, others, acc, others_acc, c.prev)
    c.run(acc)
    assert calls == 2 * list(range(c.L - 1, -1, -1)), calls       # once per layer per backward
    c.plan.set_grad_callback(None)
    c.check()


def test_unknown_mode_is_refused():
    plan = cabi.LstmPlan(4, 6, 32, 128, 2, BF16, DEV, training=True)
    lib = cabi.load()
    assert lib.csn_lstm_plan_set_grad_mode(plan._plan, 2) == 1
    assert b"unknown mode" in lib.csn_last_error()
    assert lib.csn_lstm_plan_set_grad_mode(plan._plan, 1) == 0 and lib.csn_lstm_plan_set_grad_mode(plan._plan, 0) == 0


def test_one_buffer_for_both_biases_is_refused_when_accumulating():
    B, T, I, H, L = 4, 6, 32, 128, 2
    plan = cabi.LstmPlan(B, T, I, H, L, BF16, DEV, training=True)
    torch.manual_seed(0)
    ref = torch.nn.LSTM(I, H, L, batch_first=True).to(DEV)
    w = [[getattr(ref, f"{n}_l{k}").detach() for k in range(L)] for n in _GROUPS]
    plan.forward(torch.randn(B, T, I, device=DEV), *w)
    grads = [[torch.zeros_like(p) for p in group] for group in w]
    grads[3] = grads[2]                                    # db_hh is db_ih
    plan.set_grad_mode(True)
    with pytest.raises(cabi.CsnError, match="one buffer"):
        plan.backward(torch.randn(B, H, device=DEV), None, grads)
    torch.cuda.synchronize()
    assert all(float(g.abs().max()) == 0 for group in grads for g in group)     # refused before any launch
    plan.set_grad_mode(False)                              # overwriting, both receive the same bits as they always did
    plan.backward(torch.randn(B, H, device=DEV), None, grads)
    torch.cuda.synchronize()
    assert float(grads[2][0].abs().max()) > 0 and plan.status() == 0


# ---- modules ----------------------------------------------------------------------------------------------------------
# (B, C, H, L): a weight-stationary shape (bf16: path 3, float32: path 4) and H = 96 (generic cells)
_MODEL_SHAPES = {"ws_h128": (12, 16, 128, 2), "h96": (12, 24, 96, 2)}


def _two_models(shape, dtype):
    B, C, H, L = shape
    torch.manual_seed(3)
    a = Model(input_size=C, lstm_size=H, lstm_layers=L, output_size=24, include_top=False, compute_dtype=dtype).to(DEV)
    b = Model(input_size=C, lstm_size=H, lstm_layers=L, output_size=24, include_top=False, compute_dtype=dtype).to(DEV)
    b.load_state_dict(a.state_dict())
    for m in (a, b):
        for p in m.parameters():
            p.grad = torch.zeros_like(p)
    b.lstm.direct_grads = "accumulate"
    return a, b


def _check_model_plans(m, shape, dtype):
    H = shape[2]
    plans = m.lstm.all_plans()
    assert plans
    for pl in plans:
        assert pl.status() == 0
        if H == 128:
            assert pl.path() == (3 if dtype == BF16 else 4), pl.path()
        else:
            assert (pl.path(),) + pl.kernel_names() == V1


def _same_grads(a, b):
    for (k, p), (_, q) in zip(a.named_parameters(), b.named_parameters()):
        assert float(p.grad.abs().max()) > 0, k
        assert torch.equal(p.grad, q.grad), (k, float((p.grad - q.grad).abs().max()))


@pytest.mark.parametrize("dtype", [BF16, F32], ids=["bf16", "f32"])
@pytest.mark.parametrize("shape", list(_MODEL_SHAPES))
def test_two_views_accumulate_directly_as_autograd_does(shape, dtype):
    B, C, H, L = _MODEL_SHAPES[shape]
    a, b = _two_models(_MODEL_SHAPES[shape], dtype)
    g = torch.Generator().manual_seed(5)
    x30, x20, tgt = (torch.randn(*s, generator=g).to(DEV) for s in ((B, 30, C), (B, 20, C), (B, 24)))
    loss = CosineSimilarityLoss()
    for m in (a, b):
        (loss(m(x30), tgt) + loss(m(x20), tgt)).backward()
    torch.cuda.synchronize()
    _same_grads(a, b)
    assert len(b.lstm.all_plans()) == 2
    for m in (a, b):
        _check_model_plans(m, _MODEL_SHAPES[shape], dtype)


@pytest.mark.parametrize("dtype", [BF16, F32], ids=["bf16", "f32"])
@pytest.mark.parametrize("shape", list(_MODEL_SHAPES))
def test_micro_batches_accumulate_directly_as_autograd_does(shape, dtype):
    B, C, H, L = _MODEL_SHAPES[shape]
    a, b = _two_models(_MODEL_SHAPES[shape], dtype)
    g = torch.Generator().manual_seed(6)
    x, tgt = torch.randn(B, 30, C, generator=g).to(DEV), torch.randn(B, 24, generator=g).to(DEV)
    loss = CosineSimilarityLoss()
    for m in (a, b):
        for j in range(3):
            rows = slice(j * B // 3, (j + 1) * B // 3)
            (loss(m(x[rows]), tgt[rows]) / 3).backward()
    torch.cuda.synchronize()
    _same_grads(a, b)
    for m in (a, b):
        _check_model_plans(m, _MODEL_SHAPES[shape], dtype)


@pytest.mark.parametrize("dtype", [BF16, F32], ids=["bf16", "f32"])
@pytest.mark.parametrize("I,H", [(16, 128), (24, 96)], ids=["ws_h128", "h96"])
def test_chunks_of_a_recording_accumulate_directly(I, H, dtype):
    B, L, T = 8, 2, 45
    torch.manual_seed(7)
    a, b = LSTM(I, H, L, compute_dtype=dtype).to(DEV), LSTM(I, H, L, compute_dtype=dtype).to(DEV)
    b.load_state_dict(a.state_dict())
    for m in (a, b):
        for p in m.parameters():
            p.grad = torch.zeros_like(p)
    b.direct_grads = "accumulate"
    g = torch.Generator().manual_seed(8)
    x, dy = torch.randn(B, T, I, generator=g).to(DEV), torch.randn(B, T, H, generator=g).to(DEV)
    for m in (a, b):
        hx = None
        for j in range(3):                      # truncated BPTT: the state is carried, the graph is cut
            t = slice(j * 15, (j + 1) * 15)
            out, (h_n, c_n) = m(x[:, t], hx)
            (out * dy[:, t]).sum().backward()
            hx = (h_n.detach(), c_n.detach())
    torch.cuda.synchronize()
    for (k, p), (_, q) in zip(a.named_parameters(), b.named_parameters()):
        assert float(p.grad.abs().max()) > 0 and torch.equal(p.grad, q.grad), k
    for m in (a, b):
        for pl in m.all_plans():
            assert pl.state and pl.status() == 0
            if dtype == F32:
                assert pl.path() == 0
            else:
                assert pl.path() == (3 if H == 128 else 0)
    # the overwriting form never applies to a state module: direct_grads = True still goes through temporaries
    c = LSTM(I, H, L, compute_dtype=dtype).to(DEV)
    c.load_state_dict(a.state_dict())
    for p in c.parameters():
        p.grad = torch.zeros_like(p)
    c.direct_grads = True
    hx = None
    for j in range(3):
        t = slice(j * 15, (j + 1) * 15)
        out, (h_n, c_n) = c(x[:, t], hx)
        (out * dy[:, t]).sum().backward()
        hx = (h_n.detach(), c_n.detach())
    for (k, p), (_, q) in zip(a.named_parameters(), c.named_parameters()):
        assert torch.equal(p.grad, q.grad), k


@pytest.mark.parametrize("dtype", [BF16, F32], ids=["bf16", "f32"])
def test_plain_direct_grads_still_overwrites(dtype):
    shape = _MODEL_SHAPES["ws_h128"]
    B, C, H, L = shape
    a, b = _two_models(shape, dtype)
    b.lstm.direct_grads = True
    g = torch.Generator().manual_seed(9)
    x30, x20, tgt = (torch.randn(*s, generator=g).to(DEV) for s in ((B, 30, C), (B, 20, C), (B, 24)))
    loss = CosineSimilarityLoss()
    lstm_grads = [p.grad for p in b.lstm.parameters()]
    for p in lstm_grads:
        p.fill_(123.0)                                     # overwritten, not added to
    for m in (a, b):
        loss(m(x30), tgt).backward()
    _same_grads(a, b)
    assert all(p.grad is q for p, q in zip(b.lstm.parameters(), lstm_grads))     # written in place
    # a second forward replaces the LSTM's gradients with its own (the contract of the overwriting form)
    for p in a.parameters():
        p.grad.zero_()
    loss(a(x20), tgt).backward()
    loss(b(x20), tgt).backward()
    torch.cuda.synchronize()
    for (k, p), (_, q) in zip(a.lstm.named_parameters(), b.lstm.named_parameters()):
        assert torch.equal(p.grad, q.grad), k
    _check_model_plans(b, shape, dtype)


# ---- trainer ----------------------------------------------------------------------------------------------------------
def _trainer_pair(B, T, C, H, L, dtype, **kw):
    rng = np.random.default_rng(B + T)
    x = torch.from_numpy(rng.standard_normal((B, C, T)).astype(np.float32)).to(DEV)
    tgt = torch.from_numpy(rng.standard_normal((B, 24)).astype(np.float32)).to(DEV)
    torch.manual_seed(3)
    m_ref = Model(input_size=C, lstm_size=H, lstm_layers=L, output_size=24, include_top=False, compute_dtype=dtype).to(DEV)
    m = Model(input_size=C, lstm_size=H, lstm_layers=L, output_size=24, include_top=False, compute_dtype=dtype).to(DEV)
    m.load_state_dict(m_ref.state_dict())
    tr = DistillTrainer(m, None, loss="cosine", lr=1e-3, preprocess=False, **kw)
    return x, tgt, m_ref, m, tr


_TRAINER_SHAPES = [(8, 40, 16, 128, 2, BF16), (8, 33, 12, 64, 3, F32), (16, 24, 16, 128, 2, F32), (64, 40, 128, 1024, 2, BF16)]


@pytest.mark.parametrize("B,T,C,H,L,dtype", _TRAINER_SHAPES)
def test_trainer_one_step_is_the_one_backward_gradient(B, T, C, H, L, dtype):
    x, tgt, m_ref, m, tr = _trainer_pair(B, T, C, H, L, dtype)
    assert tr.accum_steps == 1 and m.lstm.direct_grads == "accumulate"
    CosineSimilarityLoss()(m_ref(x.transpose(1, 2).contiguous()), tgt).backward()
    want = torch.cat([p.grad.reshape(-1) for p in m_ref.parameters()])
    tr.train_step(x, tgt)
    assert torch.equal(tr.grads.flat, want)
    tr.train_step(x, tgt)                      # the buffer is zeroed per step: nothing of the first step is left in it
    tr.check_device_status()


def _f64_whole_batch_grads(m, x_btc, tgt, L):
    """float64 torch.nn.LSTM + nn.Linear + the cosine loss (1 - mean cos, dim 1, eps 1e-8) on the whole batch, from m's
    weights: {parameter name of Model: gradient}."""
    sd = {k: v.detach().double() for k, v in m.state_dict().items()}
    C, H = m.input_size, m.lstm_size
    ref = torch.nn.LSTM(C, H, num_layers=L, batch_first=True).double().to(DEV)
    ref.load_state_dict({k[len("lstm."):]: v for k, v in sd.items() if k.startswith("lstm.")})
    fc = torch.nn.Linear(H, sd["fc.weight"].shape[0]).double().to(DEV)
    fc.load_state_dict({"weight": sd["fc.weight"], "bias": sd["fc.bias"]})
    feat = fc(ref(x_btc.double())[0][:, -1])
    (1.0 - torch.nn.functional.cosine_similarity(feat, tgt.double(), dim=1, eps=1e-8).mean()).backward()
    out = {f"lstm.{k}": p.grad for k, p in ref.named_parameters()}
    out.update({"fc.weight": fc.weight.grad, "fc.bias": fc.bias.grad})
    return out


@pytest.mark.parametrize("B,T,C,H,L,dtype", _TRAINER_SHAPES)
def test_trainer_accum_steps_4(B, T, C, H, L, dtype):
    k = 4
    x, tgt, m_ref, m, tr = _trainer_pair(B, T, C, H, L, dtype, accum_steps=k)
    x_btc = x.transpose(1, 2).contiguous()
    want64 = _f64_whole_batch_grads(m, x_btc, tgt, L)
    # (a) four manual passes over the same micro-batches, loss / 4, into zeroed .grads through temporaries
    for p in m_ref.parameters():
        p.grad = torch.zeros_like(p)
    mb = B // k
    want_loss = 0
    for j in range(k):
        rows = slice(j * mb, (j + 1) * mb)
        loss = CosineSimilarityLoss()(m_ref(x[rows].transpose(1, 2).contiguous()), tgt[rows]) / k
        loss.backward()
        want_loss = want_loss + loss.detach()
    want = torch.cat([p.grad.reshape(-1) for p in m_ref.parameters()])
    calls = []
    m.lstm.grad_ready_hook = calls.append
    before = torch.cat([p.detach().reshape(-1).clone() for p in m.parameters()])
    got_loss = tr.train_step(x, tgt)
    torch.cuda.synchronize()
    assert torch.equal(tr.grads.flat, want), float((tr.grads.flat - want).abs().max())
    assert torch.equal(got_loss.reshape(()), want_loss.reshape(()))
    # (b) the hook fired once per layer in the whole step, top layer first, and is still installed
    assert calls == list(range(L - 1, -1, -1)), calls
    assert m.lstm.grad_ready_hook == calls.append
    # (c) the whole batch in float64: the project's own relative-norm bounds for the compute type
    #     (test_gpu_lstm_state._bounds: 1e-5 float32, 4e-2 bf16)
    bound = 4e-2 if dtype == BF16 else 1e-5
    for name, p in m.named_parameters():
        r = _rel(p.grad, want64[name])
        print(f"measured accum_steps 4 vs float64 whole batch {name}: {r:.3e} (bound {bound:g})")
    for name, p in m.named_parameters():
        assert _rel(p.grad, want64[name]) < bound, (name, _rel(p.grad, want64[name]))
    # (d) the optimiser stepped once, and the device is healthy
    after = torch.cat([p.detach().reshape(-1) for p in m.parameters()])
    assert not torch.equal(before, after)
    tr.check_device_status()
    for pl in m.lstm.all_plans():
        assert pl.desc.B == mb


def test_trainer_refuses_a_batch_that_does_not_split():
    x, tgt, _, m, tr = _trainer_pair(10, 20, 16, 128, 2, BF16, accum_steps=4)
    tr.grads.flat.fill_(3.0)
    before = torch.cat([p.detach().reshape(-1).clone() for p in m.parameters()])
    with pytest.raises(ValueError, match="accum_steps"):
        tr.train_step(x, tgt)
    torch.cuda.synchronize()
    assert bool((tr.grads.flat == 3.0).all())
    assert torch.equal(before, torch.cat([p.detach().reshape(-1) for p in m.parameters()]))
    assert not m.lstm.all_plans()                          # refused before any launch


# ---- CLIs --------------------------------------------------------------------------------------------------------------
@contextlib.contextmanager
def _status_words_collected():
    """Every plan the block creates, so that their status words can be read after the CLI has returned."""
    plans, init = [], cabi.LstmPlan.__init__

    def recording_init(self, *a, **kw):
        init(self, *a, **kw)
        plans.append(self)
    cabi.LstmPlan.__init__ = recording_init
    try:
        yield plans
    finally:
        cabi.LstmPlan.__init__ = init


def test_cli_train_with_accum_steps(tmp_path):
    import LstmDistillFromDinoV2Train as train
    with _status_words_collected() as plans:
        hist = train.main(["--synthetic", "256", "--batch_size", "16", "--num_epochs", "1", "--log_dir", str(tmp_path),
                           "--hidden_size", "128", "--lstm_layers", "2", "--loss", "cosine", "--accum_steps", "2"])
    torch.cuda.synchronize()
    assert len(hist) == 1 and np.isfinite(hist[0]) and 0.5 < hist[0] < 1.5      # cosine loss vs random targets ~ 1
    sd = torch.load(os.path.join(str(tmp_path), "lstm_dinov2_best_loss.pth"), weights_only=True)
    assert "lstm.weight_hh_l1" in sd and "fc.weight" in sd
    training = [pl for pl in plans if pl.training]
    assert training and all(pl.desc.B <= 8 for pl in training)                  # micro-batches of 16 / 2 rows are what ran
    assert all(pl.status() == 0 for pl in plans)
    with pytest.raises(SystemExit):
        train.main(["--synthetic", "96", "--batch_size", "16", "--accum_steps", "3"])


def test_cli_dino_trainer_accumulates_its_views_directly(tmp_path, monkeypatch):
    import LstmDistillation as dino
    modes, set_grad_mode = [], cabi.LstmPlan.set_grad_mode

    def recording(self, accumulate):
        modes.append(bool(accumulate))
        set_grad_mode(self, accumulate)
    monkeypatch.setattr(cabi.LstmPlan, "set_grad_mode", recording)
    with _status_words_collected() as plans:
        hist = dino.main(["--synthetic", "80", "--batch_size_per_gpu", "16", "--epochs", "1", "--embed_dim", "128",
                          "--lstm_layers", "2", "--out_dim", "64", "--log_dir", str(tmp_path), "--warmup_epochs", "1",
                          "--warmup_teacher_temp_epochs", "1"])
    torch.cuda.synchronize()
    assert len(hist) == 1 and np.isfinite(hist[0])
    assert modes and all(modes) and len(modes) % 6 == 0           # six student views per step, every backward adds in place
    assert plans and all(pl.status() == 0 for pl in plans)
    assert os.path.exists(os.path.join(str(tmp_path), "checkpoint.pth"))
