"""GPU: the fused flat-buffer optimiser steps (csrc/optim.hip through flat_optim.FlatAdamW / FlatLARS /
flat_clip_gradients) against the torch optimisers they replace, on the same device.

The net is the one of test_fused_flat_rmsprop_matches_torch: Linear(37, 53) -> Tanh -> Linear(53, 11), tensors of 1961,
53, 583 and 11 elements, so every segment boundary inside the flat buffer is unaligned.  The parameter tolerance is the
project's own for the fused RMSprop step (rtol 2e-6, atol 1e-7); the arithmetic of csrc/optim.hip (its roundings and fused
multiply-adds) emulated in float32 numpy against the torch optimisers on the CPU stays within 0.40 of it over 8 steps for
AdamW / Adam / clip + AdamW and within 0.05 for LARS; every test prints the ratio it measures."""
import io
import os

import numpy as np
import pytest
import torch

from cerebralsignalnetworks_amd import FlatAdamW, FlatLARS, Model, cabi, flat_clip_gradients
from cerebralsignalnetworks_amd.losses import LARS
from cerebralsignalnetworks_amd.runtime import clip_gradients
from cerebralsignalnetworks_amd.trainer import DistillTrainer, FlatGrads

pytestmark = pytest.mark.gpu

RTOL, ATOL = 2e-6, 1e-7
STEPS = 8


def _make(cuda):
    torch.manual_seed(3)
    net = torch.nn.Sequential(torch.nn.Linear(37, 53), torch.nn.Tanh(), torch.nn.Linear(53, 11)).to(cuda)
    ref = torch.nn.Sequential(torch.nn.Linear(37, 53), torch.nn.Tanh(), torch.nn.Linear(53, 11)).to(cuda)
    ref.load_state_dict(net.state_dict())
    x = torch.randn(29, 37, device=cuda)
    fg = FlatGrads(net.parameters(), flatten_params=True)
    return net, ref, x, fg


def _fused_backward(net, x, fg):
    fg.zero()
    net(x).pow(2).mean().backward()


def _ref_backward(ref, x, ropt):
    ropt.zero_grad()
    ref(x).pow(2).mean().backward()


def _dino_clip(model, clip):
    """the clip loop of the DINO CLI (LstmDistillation.py:141-145 = utils/utils.py:132-141); returns the norms"""
    norms = []
    for p in model.parameters():
        if p.grad is not None:
            norm = p.grad.norm(2)
            norms.append(norm)
            p.grad.mul_(torch.clamp(clip / (norm + 1e-6), max=1.0))
    return torch.stack(norms)


def _assert_params_close(net, ref, fg, what):
    worst = 0.0
    for (n, p), q in zip(net.named_parameters(), ref.parameters()):
        assert fg.flat_params.data_ptr() <= p.data_ptr() < fg.flat_params.data_ptr() + fg.flat_params.numel() * 4
        a, b = p.detach().double(), q.detach().double()
        worst = max(worst, float(((a - b).abs() / (ATOL + RTOL * b.abs())).max()))
    print(f"measured {what}: largest |fused - torch| / (atol + rtol |torch|) = {worst:.3f} (must be <= 1)")
    for (n, p), q in zip(net.named_parameters(), ref.parameters()):
        np.testing.assert_allclose(p.detach().cpu().numpy(), q.detach().cpu().numpy(), rtol=RTOL, atol=ATOL, err_msg=n)
        assert not torch.equal(p.detach(), torch.zeros_like(p))


def _segments(fg, t):
    out, off = [], 0
    for p in fg.params:
        out.append(t[off:off + p.numel()])
        off += p.numel()
    return out


def test_adamw_matches_torch(cuda):
    net, ref, x, fg = _make(cuda)
    opt, ropt = FlatAdamW(fg), torch.optim.AdamW(ref.parameters(), lr=1e-3)
    start = fg.flat_params.clone()
    for _ in range(STEPS):
        _fused_backward(net, x, fg)
        opt.step()
        _ref_backward(ref, x, ropt)
        ropt.step()
    assert opt.steps == STEPS and not torch.equal(start, fg.flat_params)
    _assert_params_close(net, ref, fg, "AdamW, 8 steps")
    assert opt.last_grad_norms is None


def test_adam_matches_torch(cuda):
    net, ref, x, fg = _make(cuda)
    opt, ropt = FlatAdamW(fg, decoupled=False, weight_decay=0), torch.optim.Adam(ref.parameters(), lr=1e-3)
    for _ in range(STEPS):
        _fused_backward(net, x, fg)
        opt.step()
        _ref_backward(ref, x, ropt)
        ropt.step()
    _assert_params_close(net, ref, fg, "Adam, 8 steps")


def test_adam_with_l2_decay_matches_torch(cuda):
    """(the not-decoupled decay path: g <- g + wd p on decayed segments)"""
    net, ref, x, fg = _make(cuda)
    opt = FlatAdamW(fg, decoupled=False, weight_decay=0.05)
    ropt = torch.optim.Adam(ref.parameters(), lr=1e-3, weight_decay=0.05)
    for _ in range(STEPS):
        _fused_backward(net, x, fg)
        opt.step()
        _ref_backward(ref, x, ropt)
        ropt.step()
    _assert_params_close(net, ref, fg, "Adam + L2 decay, 8 steps")


@pytest.mark.parametrize("beta1", [0.5, 0.3])
def test_adamw_with_a_small_beta1_matches_torch(cuda, beta1):
    """(lerp_'s second form, weight = 1 - beta1 >= 0.5: m <- g - (g - m)(1 - weight))"""
    net, ref, x, fg = _make(cuda)
    opt = FlatAdamW(fg, betas=(beta1, 0.99))
    ropt = torch.optim.AdamW(ref.parameters(), lr=1e-3, betas=(beta1, 0.99))
    for _ in range(STEPS):
        _fused_backward(net, x, fg)
        opt.step()
        _ref_backward(ref, x, ropt)
        ropt.step()
    _assert_params_close(net, ref, fg, f"AdamW, beta1 = {beta1}, 8 steps")


def test_clip_cannot_be_switched_on_after_construction(cuda):
    net, ref, x, fg = _make(cuda)
    opt = FlatAdamW(fg)
    _fused_backward(net, x, fg)
    opt.param_groups[0]["clip"] = 0.1            # (the segments carry no clip flag: ignoring it silently would be worse)
    before = fg.flat_params.clone()
    with pytest.raises(ValueError, match="clip"):
        opt.step()
    assert torch.equal(before, fg.flat_params) and opt.steps == 0
    opt.param_groups[0]["clip"] = None
    opt.step()
    assert opt.steps == 1 and not torch.equal(before, fg.flat_params)


def test_adamw_no_decay_group_and_schedules(cuda):
    net, ref, x, fg = _make(cuda)
    biases = [p for p in net.parameters() if p.ndim == 1]
    opt = FlatAdamW(fg, no_decay=biases)
    ropt = torch.optim.AdamW([{"params": [p for p in ref.parameters() if p.ndim > 1]},
                              {"params": [p for p in ref.parameters() if p.ndim == 1], "weight_decay": 0.}])
    for step in range(STEPS):
        lr, wd = 1e-3 * (1 + 0.25 * step), 0.04 * (1 + step)
        opt.param_groups[0]["lr"], opt.param_groups[0]["weight_decay"] = lr, wd
        for i, group in enumerate(ropt.param_groups):
            group["lr"] = lr
            if i == 0:
                group["weight_decay"] = wd
        _fused_backward(net, x, fg)
        opt.step()
        _ref_backward(ref, x, ropt)
        ropt.step()
    _assert_params_close(net, ref, fg, "AdamW, no_decay biases, lr / weight_decay scheduled")
    # the decay did reach the weights and only them: against an optimiser without decay the weights differ, the biases do not
    net2, _, _, fg2 = _make(cuda)
    opt2 = FlatAdamW(fg2, weight_decay=0)
    for step in range(STEPS):
        opt2.param_groups[0]["lr"] = 1e-3 * (1 + 0.25 * step)
        _fused_backward(net2, x, fg2)
        opt2.step()
    assert not torch.equal(net[0].weight, net2[0].weight)


def test_lars_matches_torch(cuda):
    net, ref, x, fg = _make(cuda)
    kw = dict(lr=0.2, weight_decay=1e-6, weight_decay_filter=True, lars_adaptation_filter=True)
    opt, ropt = FlatLARS(fg, **kw), LARS(ref.parameters(), **kw)
    for _ in range(STEPS):
        _fused_backward(net, x, fg)
        opt.step()
        _ref_backward(ref, x, ropt)
        ropt.step()
    _assert_params_close(net, ref, fg, "LARS, 8 steps")


def test_lars_without_filters_and_with_decay_matches_torch(cuda):
    """(1-D tensors decayed and scaled too; a weight decay large enough to matter)"""
    net, ref, x, fg = _make(cuda)
    kw = dict(lr=0.2, weight_decay=1e-2)
    opt, ropt = FlatLARS(fg, **kw), LARS(ref.parameters(), **kw)
    for _ in range(STEPS):
        _fused_backward(net, x, fg)
        opt.step()
        _ref_backward(ref, x, ropt)
        ropt.step()
    _assert_params_close(net, ref, fg, "LARS, no filters, weight decay 1e-2")


def test_adamw_with_the_dino_clip(cuda):
    net, ref, x, fg = _make(cuda)
    opt, ropt = FlatAdamW(fg, clip=0.1), torch.optim.AdamW(ref.parameters(), lr=1e-3)
    for step in range(STEPS):
        _fused_backward(net, x, fg)
        before = fg.flat.clone()
        norms64 = torch.stack([s.double().pow(2).sum().sqrt() for s in _segments(fg, fg.flat)])
        opt.step()
        assert torch.equal(before, fg.flat), "the gradient buffer is read, never written"
        got = opt.last_grad_norms
        assert got.is_cuda and got.dtype == torch.float32 and got.shape == (4,)
        rel = ((got.double() - norms64).abs() / norms64).max().item()
        assert rel <= 1e-6, rel
        _ref_backward(ref, x, ropt)
        ref_norms = _dino_clip(ref, 0.1)
        if step == 0:
            print("measured step-1 gradient norms:", [round(v, 4) for v in ref_norms.tolist()])
            assert (ref_norms > 0.1).tolist() == [True, False, True, False]      # two tensors clipped, two not
        ropt.step()
    _assert_params_close(net, ref, fg, "per-tensor clip 0.1 + AdamW, 8 steps")


def test_flat_clip_gradients_matches_runtime_clip(cuda):
    net, ref, x, fg = _make(cuda)
    _fused_backward(net, x, fg)
    ref(x).pow(2).mean().backward()
    norms64 = torch.stack([s.double().pow(2).sum().sqrt() for s in _segments(fg, fg.flat)])
    before = fg.flat.clone()
    got = flat_clip_gradients(fg, 0.1)
    want = clip_gradients(ref, 0.1)
    assert got.is_cuda and ((got.double() - norms64).abs() / norms64).max().item() <= 1e-6
    np.testing.assert_allclose(got.cpu().numpy(), np.asarray(want, dtype=np.float64), rtol=1e-6, atol=0)
    clipped = [bool(n > 0.1) for n in want]
    assert clipped == [True, False, True, False]
    for p, q, b, c in zip(net.parameters(), ref.parameters(), _segments(fg, before), clipped):
        np.testing.assert_allclose(p.grad.cpu().numpy(), q.grad.cpu().numpy(), rtol=RTOL, atol=ATOL)
        assert torch.equal(p.grad.reshape(-1), b) != c          # an unclipped tensor keeps its bits, a clipped one moved
    # a second call clips the clipped gradients again: they sit at the bound now, the norms say so
    again = flat_clip_gradients(fg, 0.1)
    assert torch.all(again <= 0.1 * (1 + 1e-6))


SIZES = (5, 3 * 2 ** 20 + 5, 1, 4099)


def _big_buffers(cuda, seed):
    g = torch.Generator(device="cpu").manual_seed(seed)
    return torch.randn(sum(SIZES), generator=g, dtype=torch.float32).to(cuda)


def _split(t):
    return list(torch.split(t, SIZES))


def test_segment_norms_across_many_workgroups(cuda):
    ends = list(np.cumsum(SIZES))
    table = cabi.SegmentTable(ends, [3, 3, 3, 3], cuda)
    a, b = _big_buffers(cuda, 11), _big_buffers(cuda, 12)
    _split(a)[3].zero_()                                                        # a segment of zeros
    want_a = torch.stack([s.double().pow(2).sum().sqrt() for s in _split(a)])
    got = cabi.flat_segment_norms(table, a)
    torch.cuda.synchronize()
    assert got.shape == (4,) and got[3].item() == 0.0
    assert ((got.double() - want_a)[:3].abs() / want_a[:3]).max().item() <= 1e-6
    assert torch.equal(got, cabi.flat_segment_norms(table, a))                  # no atomics: the same bits again
    # the LARS pair: |a| and |b + wd a| (every segment decayed here) in one pass
    wd = 0.25
    pair = cabi.flat_segment_norms(table, a, b, weight_decay=wd)
    want_d = torch.stack([torch.add(sb, sa, alpha=wd).double().pow(2).sum().sqrt() for sa, sb in zip(_split(a), _split(b))])
    assert pair.shape == (2, 4) and torch.equal(pair[0], got)
    assert ((pair[1].double() - want_d).abs() / want_d).max().item() <= 1e-6
    assert torch.equal(pair, cabi.flat_segment_norms(table, a, b, weight_decay=wd))
    # segments that are not decayed take d = b
    table0 = cabi.SegmentTable(ends, [2, 3, 2, 3], cuda)
    pair0 = cabi.flat_segment_norms(table0, a, b, weight_decay=wd)
    want_b = torch.stack([s.double().pow(2).sum().sqrt() for s in _split(b)])
    want0 = torch.stack([want_b[0], want_d[1], want_b[2], want_d[3]])
    assert ((pair0[1].double() - want0).abs() / want0).max().item() <= 1e-6


def test_lars_and_adam_on_a_large_buffer_with_a_zero_segment(cuda):
    """Many workgroups, grid-stride, pure and boundary chunks, a tensor whose parameters and gradients are all zero
    (LARS: trust 1, no NaN), a one-element tensor with zero parameter -- against the torch optimisers, and run twice."""
    def build():
        init = _split(_big_buffers(cuda, 21))
        init[2].zero_()
        init[3].zero_()
        params = [torch.nn.Parameter(t.clone()) for t in init]
        fg = FlatGrads(params, flatten_params=True)
        grads = _big_buffers(cuda, 22)
        _split(grads)[3].zero_()
        fg.flat.copy_(grads)
        return params, fg
    results = []
    for _ in range(2):
        params, fg = build()
        refs = [torch.nn.Parameter(p.detach().clone()) for p in params]
        for r, g in zip(refs, _split(fg.flat)):
            r.grad = g.clone()
        opt, ropt = FlatLARS(fg, lr=0.2, weight_decay=1e-3), LARS(refs, lr=0.2, weight_decay=1e-3)
        for _ in range(2):
            opt.step()
            ropt.step()
        torch.cuda.synchronize()
        assert bool(torch.isfinite(fg.flat_params).all()) and bool(torch.isfinite(opt.mu).all())
        assert torch.equal(params[3].detach(), torch.zeros_like(params[3]))
        for p, r in zip(params, refs):
            np.testing.assert_allclose(p.detach().cpu().numpy(), r.detach().cpu().numpy(), rtol=RTOL, atol=ATOL)
        results.append((fg.flat_params.clone(), opt.mu.clone()))
    assert torch.equal(results[0][0], results[1][0]) and torch.equal(results[0][1], results[1][1])
    # AdamW with the clip over the same buffer
    params, fg = build()
    refs = [torch.nn.Parameter(p.detach().clone()) for p in params]
    opt, ropt = FlatAdamW(fg, clip=1.0), torch.optim.AdamW(refs, lr=1e-3)
    for _ in range(2):
        for r, g in zip(refs, _split(fg.flat)):
            r.grad = g.clone()
            r.grad.mul_(torch.clamp(1.0 / (r.grad.norm(2) + 1e-6), max=1.0))
        opt.step()
        ropt.step()
    assert opt.last_grad_norms[3].item() == 0.0
    for p, r in zip(params, refs):
        np.testing.assert_allclose(p.detach().cpu().numpy(), r.detach().cpu().numpy(), rtol=RTOL, atol=ATOL)


def _through_a_file(sd):
    buf = io.BytesIO()
    torch.save(sd, buf)
    buf.seek(0)
    return torch.load(buf, weights_only=True)


@pytest.mark.parametrize("kind", ["adamw", "lars"])
def test_state_dict_round_trip_continues_bit_for_bit(cuda, kind):
    def optimiser(net, fg, other=False):
        biases = [p for p in net.parameters() if p.ndim == 1]
        if kind == "adamw":
            if other:
                return FlatAdamW(fg, lr=5e-2, betas=(0.5, 0.9), eps=1e-3, weight_decay=0.3, decoupled=False)
            return FlatAdamW(fg, lr=2e-3, betas=(0.8, 0.99), weight_decay=0.05, no_decay=biases, clip=0.1)
        if other:
            return FlatLARS(fg, lr=0.01, weight_decay=0.1, momentum=0.5, eta=0.1)
        return FlatLARS(fg, lr=0.2, weight_decay=1e-3, weight_decay_filter=True, lars_adaptation_filter=True)
    state = ("exp_avg", "exp_avg_sq") if kind == "adamw" else ("mu",)

    net_a, _, x, fg_a = _make(cuda)
    opt_a = optimiser(net_a, fg_a)
    for _ in range(6):
        _fused_backward(net_a, x, fg_a)
        opt_a.step()

    net_b, _, _, fg_b = _make(cuda)
    opt_b = optimiser(net_b, fg_b)
    for _ in range(3):
        _fused_backward(net_b, x, fg_b)
        opt_b.step()
    saved = _through_a_file(opt_b.state_dict())
    opt_c = optimiser(net_b, fg_b, other=True)
    assert opt_c.param_groups[0]["lr"] != opt_b.param_groups[0]["lr"]
    opt_c.load_state_dict(saved)
    for k, v in opt_b.param_groups[0].items():
        if k != "params":
            assert opt_c.param_groups[0][k] == v, k
    assert opt_c.flags == opt_b.flags
    if kind == "adamw":
        assert opt_c.steps == 3 and opt_c.decoupled is True
    for _ in range(3):
        _fused_backward(net_b, x, fg_b)
        opt_c.step()
    torch.cuda.synchronize()
    assert torch.equal(fg_a.flat_params, fg_b.flat_params)
    for name in state:
        assert torch.equal(getattr(opt_a, name), getattr(opt_c, name)), name
    if kind == "adamw":
        assert torch.equal(opt_a.last_grad_norms, opt_c.last_grad_norms)


@pytest.mark.parametrize("kind", ["adamw", "lars"])
def test_check_views_catches_a_rehomed_parameter(cuda, kind):
    net, _, x, fg = _make(cuda)
    opt = FlatAdamW(fg) if kind == "adamw" else FlatLARS(fg, lr=0.2)
    _fused_backward(net, x, fg)
    opt.step()
    before = fg.flat_params.clone()
    for p in net.parameters():                      # what net.float() / .to(dtype) / load_state_dict(assign=True) do
        p.data = p.data.clone()
    with pytest.raises(RuntimeError, match="no longer lives in the flat buffer"):
        opt.step()
    torch.cuda.synchronize()
    assert torch.equal(before, fg.flat_params)      # refused before the launch


# ---- trainer and CLI -------------------------------------------------------------------------------------------------------
B, T, C, H, L = 8, 33, 12, 64, 3                   # the small float32 shape of the trainer tests (test_gpu_grad_accumulate)


@pytest.mark.parametrize("name,lr,cls", [("adamw", 1e-3, FlatAdamW), ("adam", 1e-3, FlatAdamW), ("lars", 0.2, FlatLARS)])
def test_trainer_fused_optimizer_matches_the_torch_one(cuda, name, lr, cls):
    rng = np.random.default_rng(B + T)
    x = torch.from_numpy(rng.standard_normal((B, C, T)).astype(np.float32)).to(cuda)
    tgt = torch.from_numpy(rng.standard_normal((B, 24)).astype(np.float32)).to(cuda)
    torch.manual_seed(3)
    m_ref = Model(input_size=C, lstm_size=H, lstm_layers=L, output_size=24, include_top=False, compute_dtype=torch.float32).to(cuda)
    m = Model(input_size=C, lstm_size=H, lstm_layers=L, output_size=24, include_top=False, compute_dtype=torch.float32).to(cuda)
    m.load_state_dict(m_ref.state_dict())
    tr_ref = DistillTrainer(m_ref, None, loss="cosine", lr=lr, optimizer=name, preprocess=False)
    tr = DistillTrainer(m, None, loss="cosine", lr=lr, optimizer=name, preprocess=False, fused_optimizer=True)
    assert type(tr.opt) is cls and isinstance(tr_ref.opt, torch.optim.Optimizer)
    assert tr.grads.flat_params is not None and tr_ref.grads.flat_params is None
    if name == "adam":
        assert tr.opt.decoupled is False and tr.opt.param_groups[0]["weight_decay"] == 0
    if name == "lars":
        assert tr.opt.param_groups[0]["weight_decay"] == 1e-6 and tr.opt.flags.count(3) == 2 * L + 1
    start = tr.grads.flat_params.clone()
    for step in range(3):
        loss, loss_ref = tr.train_step(x, tgt), tr_ref.train_step(x, tgt)
        if step == 0:
            assert torch.equal(loss, loss_ref)
    tr.check_device_status()
    assert not torch.equal(start, tr.grads.flat_params)
    worst = 0.0
    for p, q in zip(m.parameters(), m_ref.parameters()):
        a, b = p.detach().double(), q.detach().double()
        worst = max(worst, float(((a - b).abs() / (ATOL + RTOL * b.abs())).max()))
    print(f"measured trainer {name}, 3 steps: largest |fused - torch| / (atol + rtol |torch|) = {worst:.3f} (must be <= 1)")
    for (n, p), q in zip(m.named_parameters(), m_ref.parameters()):
        np.testing.assert_allclose(p.detach().cpu().numpy(), q.detach().cpu().numpy(), rtol=RTOL, atol=ATOL, err_msg=n)


def test_cli_dino_with_the_fused_optimizer(cuda, tmp_path):
    import LstmDistillation as dino
    from cerebralsignalnetworks_amd.dino import DINOHead, MultiCropWrapper
    hist = dino.main(["--synthetic", "80", "--batch_size_per_gpu", "16", "--epochs", "1", "--embed_dim", "128",
                      "--lstm_layers", "2", "--out_dim", "64", "--log_dir", str(tmp_path), "--warmup_epochs", "1",
                      "--warmup_teacher_temp_epochs", "1", "--fused_optimizer"])
    torch.cuda.synchronize()
    assert len(hist) == 1 and np.isfinite(hist[0])
    ck = torch.load(os.path.join(str(tmp_path), "checkpoint.pth"), weights_only=True)
    sd = ck["optimizer"]
    assert ck["args"]["fused_optimizer"] is True and sd["step"] == 4 and sd["clip"] == 3.0      # 64 training rows / 16
    student = MultiCropWrapper(Model(input_size=96, lstm_size=128, lstm_layers=2, output_size=128, include_top=False),
                               DINOHead(128, 64, False, True)).to(cuda)
    student.load_state_dict(ck["student"])
    fg = FlatGrads(student.parameters(), flatten_params=True)
    opt = FlatAdamW(fg)
    opt.load_state_dict(sd)
    assert opt.steps == 4 and opt.param_groups[0]["clip"] == 3.0 and opt.last_grad_norms is not None
    assert torch.equal(opt.exp_avg, sd["exp_avg"].to(cuda)) and bool(torch.isfinite(opt.exp_avg_sq).all())
    assert float(opt.exp_avg_sq.max()) > 0
    # biases and 1-d tensors do not decay, every tensor is clipped
    for p, f in zip(fg.params, opt.flags):
        assert f == (cabi.SEG_SCALED | (0 if p.ndim == 1 else cabi.SEG_DECAYED))
    # the last layer was frozen during this first epoch: its gradient slice was zeroed, so only the decay moved it
    opt.step()                   # (a reloaded optimiser steps)
    torch.cuda.synchronize()
    assert bool(torch.isfinite(fg.flat_params).all())
