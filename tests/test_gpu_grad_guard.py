"""GPU: global-norm gradient clipping and the non-finite step skip, decided on the device (csrc/optim.hip: csn_grad_guard,
csn_adam_step_guarded, csn_lars_step_guarded; csrc/loss.hip: csn_rmsprop_step_guarded).

1. the record (norm, scale, finite, skipped) against the float64 restatement flat_optim.guard_restatement, within one
   float32 ulp, on every size at which the guard takes another path; two runs, the same bits; planted Inf / -Inf / NaN.
2. THE ACCEPTANCE TEST, no tolerance: a guarded step has the bits of the unguarded step on the pre-scaled gradient
   g * scale (a torch float32 multiply by the scale read back from the record), parameters and every state buffer, over 8
   steps of the net of tests/test_gpu_flat_optim.py (segments of 1961, 53, 583 and 11 elements: every chunk holds a
   boundary) and one step of a buffer of 2048 * 2048 + 2048 + 5 elements in three unaligned segments (whole chunks, and a
   workgroup that walks more than one).  The unguarded steps themselves stay pinned against torch by
   tests/test_gpu_flat_optim.py.
3. end to end against the torch optimisers, whose gradients are multiplied by the restatement's coefficient: the bound is
   the project's own for a fused step (rtol 2e-6, atol 1e-7) -- the comparison carries the fused step's error only, not
   the rounding of torch's float32 clip_grad_norm_.
4. the skip: parameters, state and the gradient buffer keep their bits, and the run goes on like one that did not call
   step() at that step.
5. DistillTrainer: max_grad_norm, accum_steps, a non-finite gradient under skip_nonfinite, and both options off.
6. stream order: guard plus step on a side stream behind late inputs (tests/grad_guard_stream_cases.py)."""
import statistics

import numpy as np
import pytest
import torch

import grad_guard_stream_cases as stream_cases
import test_gpu_stream_order as stream_tests
from cerebralsignalnetworks_amd import FlatAdamW, FlatLARS, Model, cabi, flat_clip_grad_norm_
from cerebralsignalnetworks_amd.flat_optim import guard_restatement
from cerebralsignalnetworks_amd.losses import LARS
from cerebralsignalnetworks_amd.trainer import DistillTrainer, FlatGrads, FlatRMSprop

pytestmark = pytest.mark.gpu

RTOL, ATOL = 2e-6, 1e-7                 # the project's bound for a fused optimiser step (tests/test_gpu_flat_optim.py)
STEPS = 8
BIG = 2048 * 2048 + 2048 + 5            # kMaxBlocks = 2048 workgroups: the first ones walk a second and a third chunk
SIZES = (1, 7, 2047, 2048, 2049, 2608, 70001, BIG)
INF, NAN = float("inf"), float("nan")


# ---- 1. the record --------------------------------------------------------------------------------------------------------
def _buffers(n, cuda):
    """Seeded normal gradients at scales 1e-3, 1 and 1e3, and an all-zero buffer."""
    g = torch.Generator().manual_seed(n % 9973)
    base = torch.randn(n, generator=g, dtype=torch.float32).to(cuda)
    return [("1e-3", base * 1e-3), ("1", base), ("1e3", base * 1e3), ("zeros", torch.zeros_like(base))]


def _ulps(got, want):
    """|got - want| in units of float32 spacing at want."""
    got, want = np.float32(got), np.float32(want)
    return float(abs(np.float64(got) - np.float64(want)) / np.float64(np.spacing(np.abs(want)))) if got != want else 0.0


@pytest.mark.parametrize("n", SIZES)
def test_record_matches_the_float64_restatement(cuda, n):
    guard = cabi.StepGuard(cuda)
    worst = 0.0
    for label, g in _buffers(n, cuda):
        norm64 = float(g.double().pow(2).sum().sqrt())
        below, above = (0.5 * norm64, 2.0 * norm64) if norm64 > 0 else (1e-7, 1.0)     # (zeros: 1e-7 / (0 + 1e-6) = 0.1)
        for max_norm in (below, above, None):
            want_norm, want_scale, finite = guard_restatement(g, max_norm)
            assert bool(finite)
            before = g.clone()
            guard.measure(g, max_norm)
            first = guard.record.clone()
            guard.measure(g, max_norm)
            assert torch.equal(first.view(torch.int32), guard.record.view(torch.int32)), "a second run gives other bits"
            assert torch.equal(g, before), "the gradient buffer is read, never written"
            norm, scale, fin, skipped = first[0].item(), first[1].item(), *first.view(torch.int32)[2:].tolist()
            assert (fin, skipped) == (1, 0)
            un, us = _ulps(norm, want_norm.item()), _ulps(scale, want_scale.item())
            worst = max(worst, un, us)
            assert un <= 1 and us <= 1, (label, max_norm, norm, want_norm.item(), scale, want_scale.item())
            if max_norm != below:
                assert first.view(torch.int32)[1].item() == 0x3F800000, (label, max_norm, scale)     # exactly 1.0f
            else:
                assert scale < 1.0
            assert guard.norm.is_cuda and guard.norm.dim() == 0 and guard.norm.item() == norm
    print(f"measured n = {n}: largest |record - restatement| = {worst:.2f} float32 ulp (must be <= 1)")


@pytest.mark.parametrize("n", SIZES)
def test_record_of_a_non_finite_buffer(cuda, n):
    guard = cabi.StepGuard(cuda)
    base = _buffers(n, cuda)[1][1]
    calls = 0
    for pos in [p for p in sorted({0, n - 1, 2048}) if p < n]:
        for bad in (INF, -INF, NAN):
            for max_norm in (0.5, None):
                g = base.clone()
                g[pos] = bad
                guard.measure(g, max_norm)
                calls += 1
                rec = guard.record.clone()
                assert rec.view(torch.int32)[2].item() == 0 and rec.view(torch.int32)[1].item() == 0, (pos, bad, rec)   # scale +0
                assert not np.isfinite(rec[0].item())
                assert guard.skipped() == calls
    guard.measure(base, 0.5)                                    # a finite buffer opens the gate again and counts nothing
    assert guard.finite.item() == 1 and guard.skipped() == calls and guard.scale.item() > 0


# ---- 2. guarded == unguarded on the pre-scaled gradient, bit for bit ------------------------------------------------------------
def _make(cuda):
    torch.manual_seed(3)
    net = torch.nn.Sequential(torch.nn.Linear(37, 53), torch.nn.Tanh(), torch.nn.Linear(53, 11)).to(cuda)
    x = torch.randn(29, 37, device=cuda)
    return net, x, FlatGrads(net.parameters(), flatten_params=True)


def _backward(net, x, fg):
    fg.zero()
    net(x).pow(2).mean().backward()


KINDS = {
    "rmsprop": (lambda fg, **kw: FlatRMSprop(fg, lr=1e-3, **kw), ("square_avg",)),
    "adamw": (lambda fg, **kw: FlatAdamW(fg, **kw), ("exp_avg", "exp_avg_sq")),
    "adam_l2": (lambda fg, **kw: FlatAdamW(fg, decoupled=False, weight_decay=0.05, **kw), ("exp_avg", "exp_avg_sq")),
    "adamw_clip": (lambda fg, clip=0.1, **kw: FlatAdamW(fg, clip=clip, **kw), ("exp_avg", "exp_avg_sq", "last_grad_norms")),
    "lars": (lambda fg, **kw: FlatLARS(fg, lr=0.2, weight_decay=1e-6, weight_decay_filter=True, lars_adaptation_filter=True,
                                       **kw), ("mu",)),
}
PROBES = dict(KINDS, adam=(lambda fg, **kw: FlatAdamW(fg, decoupled=False, weight_decay=0, **kw), None))
_medians = {}


def _median_norm(cuda, kind):
    """Median of the run's own unclipped gradient norms (measure-and-gate-only guard): the clip then acts on about half
    of the steps."""
    if kind not in _medians:
        net, x, fg = _make(cuda)
        opt = PROBES[kind][0](fg, max_grad_norm=INF)
        norms = []
        for _ in range(STEPS):
            _backward(net, x, fg)
            opt.step()
            norms.append(opt.last_grad_norm.item())
            assert opt.guard.scale.item() == 1.0
        _medians[kind] = statistics.median(norms)
    return _medians[kind]


def _assert_same_state(a, b, names, what):
    assert torch.equal(a.flat.flat_params, b.flat.flat_params), f"{what}: parameters"
    for name in names:
        assert torch.equal(getattr(a, name), getattr(b, name)), f"{what}: {name}"


@pytest.mark.parametrize("kind", list(KINDS))
def test_guarded_step_is_the_unguarded_step_of_the_scaled_gradient(cuda, kind):
    make, state = KINDS[kind]
    max_norm = _median_norm(cuda, kind)
    net, x, fg = _make(cuda)
    _, _, fg_twin = _make(cuda)
    opt, twin = make(fg, max_grad_norm=max_norm), make(fg_twin)
    assert twin.guard is None and opt.guard is not None
    active = 0
    for step in range(STEPS):
        _backward(net, x, fg)
        g = fg.flat.clone()
        opt.step()
        assert torch.equal(fg.flat, g), "the gradient buffer is read, never written"
        scale = opt.guard.scale.clone()
        active += int(scale.item() < 1.0)
        fg_twin.flat.copy_(g * scale)                           # g' = fl32(scale g): one torch float32 multiply
        twin.step()
        _assert_same_state(opt, twin, state, f"{kind}, step {step + 1}")
    print(f"measured {kind}: max_norm = {max_norm:.6g} (median of the unclipped norms), clip active on {active} of {STEPS} steps")
    assert 0 < active < STEPS, active
    assert opt.skipped_steps() == 0


_big = {}


def _big_case(cuda):
    if not _big:
        g = torch.Generator().manual_seed(41)
        _big["p"] = torch.randn(BIG, generator=g, dtype=torch.float32)
        _big["g"] = torch.randn(BIG, generator=g, dtype=torch.float32)
        _big["v"] = torch.rand(BIG, generator=g, dtype=torch.float32)
    sizes = (1_000_003, 3_000_001, BIG - 4_000_004)              # three segments, no boundary on a multiple of four
    params = [torch.nn.Parameter(t.clone().to(cuda)) for t in torch.split(_big["p"], sizes)]
    fg = FlatGrads(params, flatten_params=True)
    fg.flat.copy_(_big["g"])
    return fg


@pytest.mark.parametrize("kind", list(KINDS))
def test_guarded_step_on_a_large_buffer(cuda, kind):
    make, state = KINDS[kind]
    fg, fg_twin = _big_case(cuda), _big_case(cuda)
    kw = dict(clip=40.0) if kind == "adamw_clip" else {}        # (per-tensor norms of the scaled gradient: about 220 to 850)
    opt, twin = make(fg, max_grad_norm=1000.0, **kw), make(fg_twin, **kw)
    for o in (opt, twin):                                       # second moments that are not zero
        for name in state[:-1] if kind == "adamw_clip" else state:
            getattr(o, name).copy_(_big["v"])
    g = fg.flat.clone()
    opt.step()
    scale = opt.guard.scale.clone()
    want = guard_restatement(g, 1000.0)
    assert 0.4 < scale.item() < 0.6 and _ulps(scale.item(), want[1].item()) <= 1 and _ulps(opt.last_grad_norm.item(), want[0].item()) <= 1
    assert torch.equal(fg.flat, g)
    fg_twin.flat.copy_(g * scale)
    twin.step()
    _assert_same_state(opt, twin, state, f"{kind}, n = {BIG}")
    assert not torch.equal(fg.flat_params, _big["p"].to(cuda))


# ---- 3. end to end against torch ------------------------------------------------------------------------------------------------
def _assert_params_close(net, ref, what):
    worst = 0.0
    for p, q in zip(net.parameters(), ref.parameters()):
        a, b = p.detach().double(), q.detach().double()
        worst = max(worst, float(((a - b).abs() / (ATOL + RTOL * b.abs())).max()))
    print(f"measured {what}: largest |fused - torch| / (atol + rtol |torch|) = {worst:.3f} (must be <= 1)")
    for (n, p), q in zip(net.named_parameters(), ref.parameters()):
        np.testing.assert_allclose(p.detach().cpu().numpy(), q.detach().cpu().numpy(), rtol=RTOL, atol=ATOL, err_msg=n)


@pytest.mark.parametrize("kind", ["adamw", "adam", "lars"])
def test_clipped_run_matches_torch(cuda, kind):
    net, x, fg = _make(cuda)
    ref = torch.nn.Sequential(torch.nn.Linear(37, 53), torch.nn.Tanh(), torch.nn.Linear(53, 11)).to(cuda)
    ref.load_state_dict(net.state_dict())
    lars = dict(lr=0.2, weight_decay=1e-6, weight_decay_filter=True, lars_adaptation_filter=True)
    max_norm = _median_norm(cuda, kind)
    if kind == "adamw":
        opt, ropt = FlatAdamW(fg, max_grad_norm=max_norm), torch.optim.AdamW(ref.parameters(), lr=1e-3)
    elif kind == "adam":
        opt = FlatAdamW(fg, decoupled=False, weight_decay=0, max_grad_norm=max_norm)
        ropt = torch.optim.Adam(ref.parameters(), lr=1e-3)
    else:
        opt, ropt = FlatLARS(fg, max_grad_norm=max_norm, **lars), LARS(ref.parameters(), **lars)
    start = fg.flat_params.clone()
    active = 0
    for _ in range(STEPS):
        _backward(net, x, fg)
        opt.step()
        ropt.zero_grad()
        ref(x).pow(2).mean().backward()
        _, coef, finite = guard_restatement(torch.cat([p.grad.reshape(-1) for p in ref.parameters()]), max_norm)
        assert bool(finite)
        active += int(coef.item() < 1.0)
        for p in ref.parameters():
            p.grad.mul_(coef)
        ropt.step()
    assert 0 < active < STEPS and not torch.equal(start, fg.flat_params)
    _assert_params_close(net, ref, f"{kind} with max_grad_norm, {STEPS} steps, clip active on {active}")


# ---- 4. the skip ----------------------------------------------------------------------------------------------------------------
SKIP_SIZES = (5000, 53, 583, 11)        # chunks 0 and 1 lie inside the first tensor (vector path), chunk 2 holds three boundaries


def _synthetic(cuda, step):
    return torch.randn(sum(SKIP_SIZES), generator=torch.Generator().manual_seed(100 + step), dtype=torch.float32).to(cuda)


def _skip_case(cuda):
    torch.manual_seed(7)
    return FlatGrads([torch.nn.Parameter(torch.randn(n, device=cuda)) for n in SKIP_SIZES], flatten_params=True)


@pytest.mark.parametrize("where,pos", [("vector_chunk", 100), ("boundary_chunk", 5010)])
@pytest.mark.parametrize("kind", list(KINDS))
def test_a_non_finite_step_is_not_taken(cuda, kind, where, pos):
    make, state = KINDS[kind]
    fg, fg_twin = _skip_case(cuda), _skip_case(cuda)
    opt, twin = make(fg, skip_nonfinite=True), make(fg_twin)
    assert opt.param_groups[0]["max_grad_norm"] is None
    for step in range(1, 7):
        g = _synthetic(cuda, step)
        if step == 3:
            g[pos] = INF
        fg.flat.copy_(g)
        before = [fg.flat_params.clone()] + [getattr(opt, name).clone() for name in state]
        opt.step()
        assert torch.equal(fg.flat, g), "the gradient buffer is untouched"
        if step == 3:
            after = [fg.flat_params] + [getattr(opt, name) for name in state]
            assert all(torch.equal(a, b) for a, b in zip(after, before)), "a skipped step wrote something"
            assert opt.skipped_steps() == 1 and not np.isfinite(opt.last_grad_norm.item())
            if hasattr(twin, "steps"):
                twin.steps += 1                                 # Adam's t counts the calls, skipped ones included
        else:
            assert not torch.equal(fg.flat_params, before[0])
            fg_twin.flat.copy_(g)
            twin.step()                                         # (the twin simply does not step at step 3)
            _assert_same_state(opt, twin, state, f"{kind}, step {step}")
    assert opt.skipped_steps() == 1 and twin.skipped_steps() == 0
    if hasattr(opt, "steps"):
        assert opt.steps == twin.steps == 6


def test_a_finite_max_norm_skips_too_and_the_state_dict_keeps_the_count(cuda):
    fg = _skip_case(cuda)
    opt = FlatAdamW(fg, max_grad_norm=2.5)                      # skip_nonfinite=False: 0 * Inf would write NaN
    g = _synthetic(cuda, 1)
    g[7] = NAN
    fg.flat.copy_(g)
    before = fg.flat_params.clone()
    opt.step()
    assert torch.equal(fg.flat_params, before) and opt.skipped_steps() == 1 and opt.skip_nonfinite is False
    sd = opt.state_dict()
    assert sd["max_grad_norm"] == 2.5 and sd["skip_nonfinite"] is False and sd["skipped"] == 1
    other = FlatAdamW(_skip_case(cuda), max_grad_norm=1.0)
    other.load_state_dict(sd)
    assert other.skipped_steps() == 1 and other.param_groups[0]["max_grad_norm"] == 2.5 and other.steps == 1
    # with the guard off nothing is added: the keys of before
    plain = FlatAdamW(_skip_case(cuda))
    assert plain.guard is None and plain.last_grad_norm is None and plain.skipped_steps() == 0
    assert not {"max_grad_norm", "skip_nonfinite", "skipped"} & set(plain.state_dict())
    assert set(FlatRMSprop(_skip_case(cuda)).state_dict()) == {"square_avg", "lr", "alpha", "eps"}
    assert set(FlatRMSprop(_skip_case(cuda), skip_nonfinite=True).state_dict()) == \
        {"square_avg", "lr", "alpha", "eps", "max_grad_norm", "skip_nonfinite", "skipped"}
    plain.param_groups[0]["max_grad_norm"] = 1.0                # cannot be switched on later
    with pytest.raises(ValueError, match="max_grad_norm"):
        plain.step()
    # max_grad_norm is read from param_groups on every step, like lr
    fg.flat.copy_(_synthetic(cuda, 2))
    opt.param_groups[0]["max_grad_norm"] = 1e9
    opt.step()
    assert opt.guard.scale.item() == 1.0
    opt.param_groups[0]["max_grad_norm"] = 1e-3
    opt.step()
    assert 0 < opt.guard.scale.item() < 1e-4


def test_flat_clip_grad_norm_is_clip_grad_norm(cuda):
    net, x, fg = _make(cuda)
    _backward(net, x, fg)
    g = fg.flat.clone()                                         # (a norm of about 0.2)
    norm, coef, _ = guard_restatement(g, 0.1)
    got = flat_clip_grad_norm_(fg, 0.1)
    assert got.is_cuda and got.dim() == 0 and _ulps(got.item(), norm.item()) <= 1 and coef.item() < 1
    np.testing.assert_allclose(fg.flat.cpu().numpy(), (g * coef).cpu().numpy(), rtol=3e-7, atol=0)      # (the two coefficients: one float32 ulp apart at most)
    assert torch.equal(fg.flat, g * fg.step_guard.scale)
    # torch's own clip_grad_norm_ on the same gradient (float32 norm): the same coefficient to float32 rounding
    for p, s in zip(net.parameters(), torch.split(g, [p.numel() for p in net.parameters()])):
        p.grad.copy_(s.view_as(p))
    total = torch.nn.utils.clip_grad_norm_(list(net.parameters()), 0.1)
    np.testing.assert_allclose(got.item(), total.item(), rtol=1e-6)
    # error_if_nonfinite=False: a non-finite buffer stays non-finite
    fg.flat[5] = INF
    flat_clip_grad_norm_(fg, 0.1)
    assert not bool(torch.isfinite(fg.flat).all())


# ---- 5. trainer -----------------------------------------------------------------------------------------------------------------
B, C, T = 4, 8, 12


def _trainer_case(cuda, **kw):
    rng = np.random.default_rng(B + T)
    x = torch.from_numpy(rng.standard_normal((B, C, T)).astype(np.float32)).to(cuda)
    tgt = torch.from_numpy(rng.standard_normal((B, 16)).astype(np.float32)).to(cuda)
    torch.manual_seed(3)
    m = Model(8, 32, 1, 16, include_top=False).to(cuda)
    return x, tgt, m, DistillTrainer(m, None, loss="cosine", optimizer="rmsprop", preprocess=False, **kw)


def _first_norm(cuda, accum_steps=1):
    x, tgt, _, tr = _trainer_case(cuda, max_grad_norm=INF, accum_steps=accum_steps)
    tr.train_step(x, tgt)
    return tr.last_grad_norm.item()


def _manual_step(tr, x, tgt, max_norm, k=1):
    """backward (k micro-batches summed), flat_clip_grad_norm_, the optimiser's plain step"""
    tr.model.train()
    tr.grads.zero()
    mb = x.shape[0] // k
    for j in range(k):
        rows = slice(j * mb, (j + 1) * mb)
        (tr.compute_loss(tr.model(tr.embed(x[rows])), tgt[rows], None, 0) / k).backward()
    norm = flat_clip_grad_norm_(tr.grads, max_norm)
    tr.opt.step()
    return norm


def _assert_trainers_close(tr, ref, what):
    worst = 0.0
    for p, q in zip(tr.model.parameters(), ref.model.parameters()):
        a, b = p.detach().double(), q.detach().double()
        worst = max(worst, float(((a - b).abs() / (ATOL + RTOL * b.abs())).max()))
    print(f"measured {what}: largest |trainer - manual| / (atol + rtol |manual|) = {worst:.3f} (must be <= 1)")
    assert worst <= 1.0


@pytest.mark.parametrize("k", [1, 2])
def test_trainer_clips_the_summed_gradient_once(cuda, k):
    max_norm = 0.5 * _first_norm(cuda, k)
    x, tgt, m, tr = _trainer_case(cuda, max_grad_norm=max_norm, accum_steps=k)
    _, _, m_ref, ref = _trainer_case(cuda)
    assert isinstance(tr.opt, FlatRMSprop) and tr.opt.guard is not None and ref.opt.guard is None
    start = tr.grads.flat_params.clone()
    for step in range(3):
        tr.train_step(x, tgt)
        norm = _manual_step(ref, x, tgt, max_norm, k)
        if step == 0:                                                     # (the same parameters still: the same gradient)
            assert _ulps(tr.last_grad_norm.item(), norm.item()) <= 4
            assert tr.opt.guard.scale.item() < 0.51                       # the clip acted, on the SUM of the micro-batches
    assert not torch.equal(start, tr.grads.flat_params)
    _assert_trainers_close(tr, ref, f"max_grad_norm with accum_steps = {k}, 3 steps")
    tr.check_device_status()
    assert tr.skipped_steps() == 0


def test_trainer_skips_a_non_finite_step(cuda):
    x, tgt, m, tr = _trainer_case(cuda, skip_nonfinite=True)
    poison = {"on": False}

    def hook(p):                        # behind fc.bias's gradient: no LSTM kernel ever sees the value
        if poison["on"]:
            p.grad[3] = INF
    m.fc.bias.register_post_accumulate_grad_hook(hook)
    tr.train_step(x, tgt)
    before = tr.grads.flat_params.clone()
    state = tr.opt.square_avg.clone()
    poison["on"] = True
    tr.train_step(x, tgt)
    poison["on"] = False
    assert torch.equal(tr.grads.flat_params, before) and torch.equal(tr.opt.square_avg, state)
    assert not np.isfinite(tr.last_grad_norm.item())
    tr.check_device_status()            # does not raise: that step was not taken
    assert tr.skipped_steps() == 1
    tr.train_step(x, tgt)               # the next step trains
    assert not torch.equal(tr.grads.flat_params, before) and bool(torch.isfinite(tr.grads.flat_params).all())
    tr.check_device_status()
    assert tr.skipped_steps() == 1
    # without skip_nonfinite a finite max_grad_norm skips the step all the same, and the status check reports the run
    x, tgt, m2, tr2 = _trainer_case(cuda, max_grad_norm=1.0)
    m2.fc.bias.register_post_accumulate_grad_hook(hook)
    tr2.train_step(x, tgt)
    before = tr2.grads.flat_params.clone()
    poison["on"] = True
    tr2.train_step(x, tgt)
    assert torch.equal(tr2.grads.flat_params, before) and tr2.skipped_steps() == 1
    with pytest.raises(FloatingPointError, match="diverged"):
        tr2.check_device_status()


def test_trainer_with_both_options_off_is_the_trainer_of_before(cuda):
    x, tgt, _, tr = _trainer_case(cuda, max_grad_norm=None, skip_nonfinite=False)
    _, _, _, old = _trainer_case(cuda)
    assert tr.opt.guard is None and "max_grad_norm" not in tr.opt.param_groups[0]
    assert torch.equal(tr.train_step(x, tgt), old.train_step(x, tgt))
    assert torch.equal(tr.grads.flat_params, old.grads.flat_params) and torch.equal(tr.opt.square_avg, old.opt.square_avg)
    assert set(tr.opt.state_dict()) == {"square_avg", "lr", "alpha", "eps"} and tr.last_grad_norm is None


def test_trainer_clips_in_front_of_a_torch_optimiser(cuda):
    max_norm = 0.5 * _first_norm(cuda)
    rng = np.random.default_rng(B + T)
    x = torch.from_numpy(rng.standard_normal((B, C, T)).astype(np.float32)).to(cuda)
    tgt = torch.from_numpy(rng.standard_normal((B, 16)).astype(np.float32)).to(cuda)
    torch.manual_seed(3)
    m = Model(8, 32, 1, 16, include_top=False).to(cuda)
    tr = DistillTrainer(m, None, loss="cosine", optimizer="adamw", preprocess=False, max_grad_norm=max_norm)
    assert isinstance(tr.opt, torch.optim.AdamW)
    tr.train_step(x, tgt)
    assert tr.grads.step_guard is not None and 0.49 < tr.grads.step_guard.scale.item() < 0.51
    got = float(tr.grads.flat.double().pow(2).sum().sqrt())      # the buffer was clipped in place
    np.testing.assert_allclose(got, max_norm, rtol=1e-5)
    with pytest.raises(ValueError, match="flat optimiser"):
        DistillTrainer(m, None, loss="cosine", optimizer="adamw", preprocess=False, skip_nonfinite=True)


# ---- 6. stream order --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", [c for v in stream_cases.CASES.values() for c in v], ids=lambda c: c.id)
def test_stream_order(cuda, case):
    """The procedure of tests/test_gpu_stream_order.py on the cases of
    tests/grad_guard_stream_cases.py: guard plus step on a side stream, the gradient arriving late behind a Delay, the
    outputs snapshotted and the inputs poisoned directly behind the call -- the result has the bits of the synchronised run."""
    stream_tests.test_stateless_entry_point_with_late_inputs(cuda, case)
