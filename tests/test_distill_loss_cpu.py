"""CPU: the fused distillation losses (csrc/distill_loss.hip) as far as they can be checked without a
GPU -- the numpy restatement of both entry points (tests/distill_loss_reference.py) against the oracle, the reference's
recorded values and gradients, float64 autograd of the unfused classes and F.kl_div; the symbols and their host-side
refusals; and the rule that ``fused=True`` on CPU tensors is the torch form."""
import math
import os
import types

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import __graft_entry__ as graft
import distill_loss_reference as ref
import distill_loss_stream_cases as stream_cases      # joins the stream-order case table on import
import stream_order as so
from cerebralsignalnetworks_amd import cabi
from cerebralsignalnetworks_amd import losses as pl
from cerebralsignalnetworks_amd.dino import DINOLoss
from oracle import losses as oracle_losses

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("csn_distill_loss", "csn_distill_loss_scratch_bytes", "csn_dino_loss", "csn_dino_loss_scratch_bytes")
INVALID = 1                              # CSN_ERR_INVALID_ARGUMENT


@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(cabi.LIB_PATH):
        graft.build()
    return cabi.load()


# ---- 1. the restatement against the oracle and the reference's recorded values ----------------------------------------
def test_restatement_equals_oracle_and_recorded_reference_values(golden):
    g = golden("ref_losses.npz")
    s, t, cls, tcls, lab = g["student"], g["teacher"], g["cls"], g["tcls"], g["labels"]
    sched = oracle_losses.teacher_temp_schedule(100)
    for ep in (0, 25, 50, 99):
        loss, gs, gc = ref.featdist(s, t, sched[ep], lab, cls)
        np.testing.assert_allclose(loss, oracle_losses.feature_distribution_loss(s, t, sched[ep], lab, cls), rtol=1e-12)
        np.testing.assert_allclose(loss, g[f"featdist_ep{ep}"], rtol=1e-12)
        np.testing.assert_allclose(gs, g[f"featdist_ep{ep}_gs"], atol=1e-12)
        np.testing.assert_allclose(gc, g[f"featdist_ep{ep}_gc"], atol=1e-12)
    for alpha, temp in ((1.0, 2.0), (0.5, 4.0), (0.9, 20.0)):
        loss, gs, none = ref.kd(cls, lab, tcls, alpha, temp)
        assert none is None
        np.testing.assert_allclose(loss, oracle_losses.loss_fn_kd(cls, lab, tcls, alpha, temp), rtol=1e-12)
        np.testing.assert_allclose(loss, g[f"kd_a{alpha}_T{temp}"], rtol=1e-12)
        np.testing.assert_allclose(gs, g[f"kd_a{alpha}_T{temp}_g"], atol=1e-12)
    sw, cw, wt, tt, we = g["spamp_weights"]
    sched = oracle_losses.teacher_temp_schedule(100, wt, tt, int(we))
    for ep in (0, 25, 50):
        loss, gs, _ = ref.featdist_kd(cls, tcls, sched[ep], lab, sw, cw)
        np.testing.assert_allclose(loss, oracle_losses.feature_distribution_loss_kd(cls, tcls, sched[ep], lab, sw, cw), rtol=1e-12)
        np.testing.assert_allclose(loss, g[f"featdist_spamp_ep{ep}"], rtol=1e-12)
        np.testing.assert_allclose(gs, g[f"featdist_spamp_ep{ep}_g"], atol=1e-12)
    wt, tt, we = g["eval_temps"]
    sched = oracle_losses.teacher_temp_schedule(100, wt, tt, int(we))
    for ep in (0, 50):
        loss, gs, _ = ref.featdist_soft(s, t, sched[ep])
        np.testing.assert_allclose(loss, oracle_losses.feature_distribution_loss_soft(s, t, sched[ep]), rtol=1e-12)
        np.testing.assert_allclose(loss, g[f"featdist_eval_ep{ep}"], rtol=1e-12)
        np.testing.assert_allclose(gs, g[f"featdist_eval_ep{ep}_g"], atol=1e-12)


def test_dino_restatement_equals_oracle_and_recorded_reference_values(golden):
    g = golden("ref_losses.npz")
    center = np.zeros((1, 32))
    sched = np.concatenate((np.linspace(0.04, 0.07, 3), np.ones(7) * 0.07))
    for step in range(2):
        st, te = g["dino_student"][step], g["dino_teacher"][step]
        loss, ds = ref.dino_loss(st, te, center.reshape(-1, 32), sched[step + 1], 0.1, ref.DINO_SKIP_FIRST)
        want, center = oracle_losses.dino_loss(st, te, center, sched[step + 1])
        np.testing.assert_allclose(loss, want, rtol=1e-12)
        np.testing.assert_allclose(loss, g[f"dino_loss{step}"], rtol=1e-12)
        np.testing.assert_allclose(ds, g[f"dino_grad{step}"], atol=1e-12)
    assert center.shape == (1, 5, 32)            # step 1 ran on the per-sample centre


# ---- 2. the restatement against float64 autograd of the unfused classes ---------------------------------------------------
def _t64(a, grad=False):
    return torch.from_numpy(np.asarray(a, np.float64)).requires_grad_(grad)


@pytest.mark.parametrize("B,D,K", [(3, 5, 2), (5, 65, 40), (9, 384, 40)])
def test_restatement_equals_autograd_of_the_torch_classes(B, D, K):
    r = np.random.default_rng(B * D + K)
    s, t = r.standard_normal((B, D)), r.standard_normal((B, D))
    cls, lab = r.standard_normal((B, K)), r.integers(0, K, B)
    labD = r.integers(0, D, B)
    hp = pl.HyperParams
    fd = pl.FeatureDistributionLoss(100, hp.warmup_teacher_temp, hp.teacher_temp, hp.warmup_teacher_temp_epochs)
    for ep in (0, 30, 99):
        a, c = _t64(s, True), _t64(cls, True)
        loss = fd(a, _t64(t), ep, torch.from_numpy(lab), pred_label=c)
        loss.backward()
        want, gs, gc = ref.featdist(s, t, fd.teacher_temp_schedule[ep], lab, cls, hp.alpha, hp.beta)
        np.testing.assert_allclose(loss.item(), want, rtol=1e-12)
        np.testing.assert_allclose(a.grad.numpy(), gs, atol=1e-14)
        np.testing.assert_allclose(c.grad.numpy(), gc, atol=1e-14)
    for alpha, temp in ((0.5, 2.0), (0.9, 20.0), (0.3, 0.22)):
        a = _t64(s, True)
        loss = pl.loss_fn_kd(a, torch.from_numpy(labD), _t64(t), types.SimpleNamespace(alpha=alpha, temperature=temp))
        loss.backward()
        want, gs, _ = ref.kd(s, labD, t, alpha, temp)
        np.testing.assert_allclose(loss.item(), want, rtol=1e-12)
        np.testing.assert_allclose(a.grad.numpy(), gs, atol=1e-14)
    fk = pl.FeatureDistributionLossKD(100, **pl.FeatureDistributionLossKD.SCHEDULE)
    fs = pl.FeatureDistributionLossSoft(100, **pl.FeatureDistributionLossSoft.SCHEDULE)
    for ep in (0, 60):
        a = _t64(s, True)
        loss = fk(a, _t64(t), ep, torch.from_numpy(labD))
        loss.backward()
        want, gs, _ = ref.featdist_kd(s, t, fk.teacher_temp_schedule[ep], labD, hp.soft_target_loss_weight, hp.ce_loss_weight)
        np.testing.assert_allclose(loss.item(), want, rtol=1e-12)
        np.testing.assert_allclose(a.grad.numpy(), gs, atol=1e-14)
        a = _t64(s, True)
        loss = fs(a, _t64(t), ep)
        loss.backward()
        want, gs, _ = ref.featdist_soft(s, t, fs.teacher_temp_schedule[ep])
        np.testing.assert_allclose(loss.item(), want, rtol=1e-12)
        np.testing.assert_allclose(a.grad.numpy(), gs, atol=1e-14)


@pytest.mark.parametrize("compat", [True, False])
@pytest.mark.parametrize("V,B,D", [(2, 1, 5), (3, 5, 65), (6, 4, 24)])
def test_dino_restatement_equals_autograd_of_the_torch_class(compat, V, B, D):
    r = np.random.default_rng(V * B + D)
    s, t = r.standard_normal((V, B, D)), r.standard_normal((2, B, D))
    crit = DINOLoss(D, V, 0.04, 0.07, 3, 10, compat=compat).double()
    pairing = ref.DINO_SKIP_FIRST if compat else ref.DINO_SKIP_SAME
    for step in range(2):           # the second step runs on the updated centre ([1,B,D] under compat)
        center = crit.center.numpy().copy()
        a = _t64(s if compat else s.reshape(V * B, D), True)
        loss = crit(a, _t64(t if compat else t.reshape(2 * B, D)), step)
        loss.backward()
        want, ds = ref.dino_loss(s, t, center.reshape(-1, D), crit.teacher_temp_schedule[step], 0.1, pairing)
        np.testing.assert_allclose(loss.item(), want, rtol=1e-12)
        np.testing.assert_allclose(a.grad.numpy().reshape(V, B, D), ds, atol=1e-14)
    if V == 2 and compat:
        assert not ds[0].any()          # no pair uses view 0


def test_dino_pairs_and_gradient_scale():
    assert ref.dino_pairs(3, 2, ref.DINO_SKIP_FIRST) == [[1, 2], [1, 2]]
    assert ref.dino_pairs(3, 2, ref.DINO_SKIP_SAME) == [[1, 2], [0, 2]]
    r = np.random.default_rng(3)
    s, t, c = r.standard_normal((3, 2, 7)), r.standard_normal((1, 2, 7)), r.standard_normal(7)
    l1, d1 = ref.dino_loss(s, t, c, 0.05, 0.1, ref.DINO_SKIP_SAME)
    l3, d3 = ref.dino_loss(s, t, c, 0.05, 0.1, ref.DINO_SKIP_SAME, grad_scale=1 / 3)
    assert l1 == l3 and np.allclose(d3 * 3, d1, rtol=1e-15)
    assert not d1[0].any()              # G = 1 under SKIP_SAME: view 0 meets no teacher view


# ---- 3. the zero-probability convention and the label rule ----------------------------------------------------------------
def test_kl_convention_is_kl_divs_where_the_teacher_softmax_underflows():
    r = np.random.default_rng(5)
    s, t = 10 * r.standard_normal((4, 40)), 10 * r.standard_normal((4, 40))
    T = 0.04
    p_t = ref.softmax(t / T)
    assert (p_t == 0).any()
    loss, ds, _ = ref.distill_loss(s, t, ref.SOFT_KL, T, 1.0)
    want = F.kl_div(F.log_softmax(_t64(s) / T, dim=-1), _t64(p_t), reduction="sum") / 4
    np.testing.assert_allclose(loss, want.item(), rtol=1e-13)
    explicit = pl._soft_target_kl(_t64(s), _t64(t), T)
    assert math.isnan(explicit.item()), "the explicit torch formula is NaN on this input: the convention matters here"
    assert np.isfinite(ds).all()
    same, dsame, _ = ref.distill_loss(s, s, ref.SOFT_KL, T, 1.0)
    assert same == 0.0 and not dsame.any()


def test_a_label_out_of_range_is_nan_in_its_row_only():
    r = np.random.default_rng(6)
    s, t, z = r.standard_normal((4, 9)), r.standard_normal((4, 9)), r.standard_normal((4, 3))
    lab = np.array([0, 2, 1, 1])
    _, gs, gc = ref.distill_loss(s, t, ref.SOFT_CE_OF_PROBS, 0.5, 0.5, logits=z, labels=lab, w_ce=0.5)
    for bad in (3, -1):
        lab2 = lab.copy()
        lab2[2] = bad
        loss, gs2, gc2 = ref.distill_loss(s, t, ref.SOFT_CE_OF_PROBS, 0.5, 0.5, logits=z, labels=lab2, w_ce=0.5)
        assert math.isnan(loss) and np.isnan(gc2[2]).all() and np.array_equal(gs2, gs)
        assert np.array_equal(np.delete(gc2, 2, 0), np.delete(gc, 2, 0))
        loss, ga, _ = ref.distill_loss(s, t, ref.SOFT_KL, 0.5, 0.5, labels=np.where(lab2 == bad, 9 if bad > 0 else -1, lab2),
                                       w_ce=0.5, alias=True)
        assert math.isnan(loss) and np.isnan(ga[2]).all() and np.isfinite(np.delete(ga, 2, 0)).all()


# ---- 4. ABI ---------------------------------------------------------------------------------------------------------------
def test_symbols_are_exported_bound_and_declared(lib):
    text = open(os.path.join(ROOT, "include", "csn_hip.h")).read()
    for name in NAMES:
        assert name in cabi.SIGNATURES and hasattr(lib, name)
        assert name + "(" in text
    for name in ("CSN_SOFT_KL = 0", "CSN_SOFT_CE_OF_PROBS = 1", "CSN_DINO_SKIP_FIRST = 0", "CSN_DINO_SKIP_SAME = 1"):
        assert name in text
    assert (cabi.SOFT_KL, cabi.SOFT_CE_OF_PROBS, cabi.DINO_SKIP_FIRST, cabi.DINO_SKIP_SAME) == (0, 1, 0, 1)
    assert (ref.SOFT_KL, ref.SOFT_CE_OF_PROBS, ref.DINO_SKIP_FIRST, ref.DINO_SKIP_SAME) == (0, 1, 0, 1)
    assert hasattr(cabi, "distill_loss") and hasattr(cabi, "dino_loss")
    assert lib.csn_abi_version() == cabi.ABI_VERSION == 6, "added symbols do not bump the ABI"
    assert lib.csn_distill_loss_scratch_bytes(5) == 80 and lib.csn_distill_loss_scratch_bytes(0) == 0
    assert lib.csn_dino_loss_scratch_bytes(5, 1024) == 40 and lib.csn_dino_loss_scratch_bytes(5, 1025) == 8 * (5 + 5 * 1025)
    assert lib.csn_dino_loss_scratch_bytes(0, 8) == 0 and lib.csn_dino_loss_scratch_bytes(8, 0) == 0


def test_stream_order_cases_are_registered():
    for name in ("csn_distill_loss", "csn_dino_loss"):
        cases = so.CASE_TABLE[name]
        assert cases is stream_cases.CASES[name] and cases
        assert all(isinstance(c, so.Stateless) and c.entry == name and callable(c.build) for c in cases)
    ids = [c.id for v in stream_cases.CASES.values() for c in v]
    assert len(set(ids)) == len(ids) and not set(ids) & {c.id for c in so.STATELESS_CASES}
    n = len(so.CASE_TABLE)
    stream_cases.register()
    assert len(so.CASE_TABLE) == n, "registering twice adds nothing"


# ---- 5. refusals ------------------------------------------------------------------------------------------------------
ONE = 1 << 12                            # any non-null, 8-byte aligned address: refused arguments are never dereferenced
TWO = 2 << 12


def _refused(lib, rc, word):
    msg = lib.csn_last_error()
    assert rc == INVALID, (rc, msg)
    assert word in msg, (word, msg)


def test_distill_refusals_happen_on_the_host(lib):
    """No GPU here: every one of these returns before any launch, with a message."""
    def call(s=ONE, t=ONE, B=4, D=8, logits=TWO, K=3, labels=ONE, mode=0, T=0.5, loss=ONE, ds=ONE, dl=ONE, scratch=ONE):
        return lib.csn_distill_loss(s, t, B, D, logits, K, labels, mode, T, 0.5, 0.5, loss, ds, dl, 1.0, scratch, None)

    for null in ("s", "t", "loss", "scratch"):
        _refused(lib, call(**{null: None}), b"null")
    for kw in (dict(B=0), dict(B=-1), dict(D=0), dict(D=-3)):
        _refused(lib, call(**kw), b"shape")
    for T in (0.0, -1.0, float("inf"), float("nan")):
        _refused(lib, call(T=T), b"temperature")
    for mode in (-1, 2):
        _refused(lib, call(mode=mode), b"soft_mode")
    _refused(lib, call(labels=None), b"without labels")
    for K in (0, -2):
        _refused(lib, call(K=K), b"K=")
    _refused(lib, call(logits=ONE, K=3, dl=None), b"!= D")                    # the alias with K != D
    _refused(lib, call(logits=ONE, K=8), b"aliasing")                         # the alias together with dlogits
    _refused(lib, call(logits=None, labels=None), b"dlogits without logits")
    _refused(lib, call(scratch=ONE + 4), b"aligned")


def test_dino_refusals_happen_on_the_host(lib):
    def call(s=ONE, t=ONE, V=3, G=2, B=4, D=8, c=ONE, stride=0, tt=0.04, st=0.1, pairing=0, loss=ONE, scratch=ONE):
        return lib.csn_dino_loss(s, t, V, G, B, D, c, stride, tt, st, pairing, loss, ONE, 1.0, scratch, None)

    for null in ("s", "t", "c", "loss", "scratch"):
        _refused(lib, call(**{null: None}), b"null")
    for kw in (dict(B=0), dict(D=0), dict(B=-2)):
        _refused(lib, call(**kw), b"shape")
    for V in (1, 0):
        _refused(lib, call(V=V, G=1), b"two student views")
    for G in (0, 4, -1):
        _refused(lib, call(G=G), b"outside [1, V=3]")
    _refused(lib, call(stride=4), b"center_stride_b")
    for kw in (dict(tt=0.0), dict(st=-0.1), dict(tt=float("nan")), dict(st=float("inf"))):
        _refused(lib, call(**kw), b"temperatures")
    for pairing in (-1, 2):
        _refused(lib, call(pairing=pairing), b"pairing")
    _refused(lib, call(scratch=ONE + 2), b"aligned")


def test_bindings_refuse_host_tensors():
    x = torch.zeros(2, 4)
    with pytest.raises(cabi.CsnError):
        cabi.distill_loss(x, x, cabi.SOFT_KL, 1.0, 1.0)
    with pytest.raises(cabi.CsnError):
        cabi.dino_loss(torch.zeros(2, 2, 4), torch.zeros(1, 2, 4), torch.zeros(4), 0.04, 0.1, cabi.DINO_SKIP_FIRST)


# ---- 6. fused=True on CPU tensors (and on float64) is the torch form ------------------------------------------------------
def _bits(fn, *grads):
    for g in grads:
        g.grad = None
    loss = fn()
    loss.backward()
    return [loss.detach().clone()] + [g.grad.clone() for g in grads]


@pytest.mark.parametrize("dtype", [torch.float32, torch.float64])
def test_fused_on_cpu_tensors_is_the_torch_form_bit_for_bit(dtype):
    r = np.random.default_rng(8)
    s = torch.from_numpy(r.standard_normal((5, 12))).to(dtype).requires_grad_(True)
    t = torch.from_numpy(r.standard_normal((5, 12))).to(dtype)
    c = torch.from_numpy(r.standard_normal((5, 4))).to(dtype).requires_grad_(True)
    lab, labD = torch.from_numpy(r.integers(0, 4, 5)), torch.from_numpy(r.integers(0, 12, 5))
    hp = pl.HyperParams
    args = (100, hp.warmup_teacher_temp, hp.teacher_temp, hp.warmup_teacher_temp_epochs)
    kd = types.SimpleNamespace(alpha=0.7, temperature=3.0)
    pairs = [
        (lambda f: pl.FeatureDistributionLoss(*args, fused=f)(s, t, 7, lab, pred_label=c), (s, c)),
        (lambda f: pl.FeatureDistributionLossKD(100, **pl.FeatureDistributionLossKD.SCHEDULE, fused=f)(s, t, 7, labD), (s,)),
        (lambda f: pl.FeatureDistributionLossSoft(100, **pl.FeatureDistributionLossSoft.SCHEDULE, fused=f)(s, t, 7), (s,)),
        (lambda f: pl.loss_fn_kd(s, labD, t, kd, fused=f), (s,)),
    ]
    for make, grads in pairs:
        want = _bits(lambda: make(False), *grads)
        got = _bits(lambda: make(True), *grads)
        assert all(so.same_bits(a, b) for a, b in zip(got, want))
    # the HyperParams.T side effect is kept
    pl.HyperParams.T = None
    pl.FeatureDistributionLoss(*args, fused=True)(s, t, 7, lab, pred_label=c)
    assert pl.HyperParams.T == pl.FeatureDistributionLoss(*args).teacher_temp_schedule[7]
    sv = torch.from_numpy(r.standard_normal((3, 5, 12))).to(dtype).requires_grad_(True)
    tv = torch.from_numpy(r.standard_normal((2, 5, 12))).to(dtype)
    for compat in (True, False):
        a = sv if compat else sv.reshape(15, 12)
        b = tv if compat else tv.reshape(10, 12)
        crits = [DINOLoss(12, 3, 0.04, 0.07, 3, 10, compat=compat, fused=f).to(dtype) for f in (False, True)]
        for step in range(2):
            want = _bits(lambda: crits[0](a, b, step), sv)
            got = _bits(lambda: crits[1](a, b, step), sv)
            assert all(so.same_bits(x, y) for x, y in zip(got, want)) and so.same_bits(crits[0].center, crits[1].center)


def test_trainer_and_cli_surface():
    import inspect
    from cerebralsignalnetworks_amd.trainer import DistillTrainer
    import LstmDistillFromDinoV2Train as train_cli
    import LstmDistillation as dino_cli
    assert inspect.signature(DistillTrainer.__init__).parameters["fused_loss"].default is False
    assert inspect.signature(pl.loss_fn_kd).parameters["fused"].default is False
    assert inspect.signature(DINOLoss.__init__).parameters["fused"].default is False
    for flavour in (train_cli.PERILS, train_cli.SPAMPINATO):
        p = train_cli.build_parser(flavour)
        assert p.parse_args([]).fused_loss is False and p.parse_args(["--fused_loss"]).fused_loss is True
        assert "cosine" in p.format_help().split("--fused_loss")[-1].split("--compat_label_bug")[0]
    p = dino_cli.build_parser()
    assert p.parse_args([]).fused_loss is False and p.parse_args(["--fused_loss"]).fused_loss is True
