"""GPU: the fused distillation losses (csrc/distill_loss.hip) -- csn_distill_loss and csn_dino_loss
against their float64 numpy restatements (tests/distill_loss_reference.py) on the float32 inputs upcast, the recorded values
of the reference, canaries around every output, the stream contract, and the wiring into the classes, the trainer and the
command-line tools.

Tolerances (derived, not tuned).  The kernels compute in float64 and round each float32 output once, so
    loss:      |got - ref| <= 2^-23 |ref|                                (one float32 ulp)
    gradient:  |got - ref| <= 2^-23 |ref| + 1e-12 U + 2^-126
with U the natural bound on a gradient element: |grad_scale| (|w_soft| / T + |w_ce|) / B for csn_distill_loss and
|grad_scale| / (student_temp B (V - 1)) for csn_dino_loss.  The float64 error of either side is ~1e-16 of U; 1e-12 U leaves
room for the cancellations (q - p_t, a - sum q a, log Z_s - log Z_t) without admitting a float32 intermediate (6e-8)."""
import types

import numpy as np
import pytest
import torch

import distill_loss_reference as ref
import distill_loss_stream_cases as stream_cases
import test_gpu_stream_order as stream_tests
from cerebralsignalnetworks_amd import cabi, Model, EEGFilters
from cerebralsignalnetworks_amd import losses as pl
from cerebralsignalnetworks_amd.dino import DINOHead, DINOLoss, MultiCropWrapper
from oracle import eeg_filter, losses as oracle_losses, lstm

pytestmark = pytest.mark.gpu

PAD = 96                    # canary elements before and behind every output
CANARY = -7.25
D_SET = (1, 5, 63, 64, 65, 384, 1024, 1025, 2049)       # 1024 is the last register-resident row length
TEMPS = (20.0, 1.65, 0.22, 0.04)


def dev(a, cuda):
    return torch.from_numpy(np.ascontiguousarray(a)).to(cuda)


class Guarded:
    """A dense output inside a larger buffer filled with a canary."""

    def __init__(self, shape, cuda, dtype=torch.float32):
        self.n = int(np.prod(shape))
        self.buf = torch.full((self.n + 2 * PAD,), CANARY, dtype=dtype, device=cuda)
        self.out = self.buf[PAD:PAD + self.n].view(*shape)

    def intact(self):
        return bool((self.buf[:PAD] == CANARY).all()) and bool((self.buf[PAD + self.n:] == CANARY).all())


def raw_distill(cuda, s, t, mode, T, w_soft, logits=None, labels=None, w_ce=0.0, alias=False, gs=1.0, want=("ds", "dl")):
    """The C entry point with every output inside a canary buffer -> (loss, ds | None, dl | None, guards)."""
    lib = cabi.load()
    B, D = s.shape
    lg = s if alias else logits
    K = lg.shape[1] if lg is not None else 0
    g = {"loss": Guarded((1,), cuda), "scratch": Guarded((2 * B,), cuda, torch.float64)}
    if "ds" in want:
        g["ds"] = Guarded((B, D), cuda)
    if "dl" in want and lg is not None and not alias:
        g["dl"] = Guarded((B, K), cuda)
    p = lambda k: cabi._ptr(g[k].out) if k in g else None      # noqa: E731
    cabi._check(lib.csn_distill_loss(cabi._ptr(s), cabi._ptr(t), B, D, cabi._ptr(lg), K, cabi._ptr(labels), mode, T, w_soft,
                                     w_ce, p("loss"), p("ds"), p("dl"), gs, p("scratch"), cabi._stream()))
    return g


def raw_dino(cuda, s, t, c, stride, tt, st, pairing, gs=1.0, want_ds=True):
    lib = cabi.load()
    V, B, D = s.shape
    g = {"loss": Guarded((1,), cuda),
         "scratch": Guarded((lib.csn_dino_loss_scratch_bytes(B, D) // 8,), cuda, torch.float64)}
    if want_ds:
        g["ds"] = Guarded((V, B, D), cuda)
    cabi._check(lib.csn_dino_loss(cabi._ptr(s), cabi._ptr(t), V, t.shape[0], B, D, cabi._ptr(c), stride, tt, st, pairing,
                                  cabi._ptr(g["loss"].out), cabi._ptr(g["ds"].out) if want_ds else None, gs,
                                  cabi._ptr(g["scratch"].out), cabi._stream()))
    return g


def check_loss(got, want, what):
    err = abs(float(got) - want)
    print(f"{what}: loss {float(got)!r} ref {want!r} err {err:.3e} tol {ref.loss_tol(want):.3e}")
    assert err <= ref.loss_tol(want), what


def check_grad(got, want, U, what):
    got = got.double().cpu().numpy() if torch.is_tensor(got) else got
    assert got.shape == want.shape, what
    ratio = np.abs(got - want) / ref.grad_tol(want, U)
    assert np.isfinite(got).all() and ratio.max() <= 1.0, (what, float(ratio.max()))
    return float(ratio.max())


# ---- 1. values and gradients against the restatement ------------------------------------------------------------------
# (mode, logits: None | K | "alias")
CONFIGS = ((ref.SOFT_KL, None), (ref.SOFT_KL, "alias"), (ref.SOFT_KL, 40), (ref.SOFT_CE_OF_PROBS, 2),
           (ref.SOFT_CE_OF_PROBS, 40), (ref.SOFT_CE_OF_PROBS, "alias"))


@pytest.mark.parametrize("D", D_SET)
def test_distill_loss_against_the_restatement(cuda, D):
    r = np.random.default_rng(100 + D)
    worst, n = 0.0, 0
    for B in (1, 3, 5, 9):
        base_s, base_t = r.standard_normal((B, D)).astype(np.float32), r.standard_normal((B, D)).astype(np.float32)
        for scale in (1.0, 10.0):
            s, t = (base_s * np.float32(scale)), (base_t * np.float32(scale))
            sd, td = dev(s, cuda), dev(t, cuda)
            for mode, lg in CONFIGS:
                alias = lg == "alias"
                K = D if alias else lg
                logits = None if (alias or lg is None) else (r.standard_normal((B, K)) * scale).astype(np.float32)
                labels = None if lg is None else r.integers(0, K, B)
                ld = None if logits is None else dev(logits, cuda)
                labd = None if labels is None else dev(labels, cuda)
                for T in TEMPS:
                    n += 1
                    gs = (1.0, 1.0 / 3.0)[(n + n // 4) % 2]            # both scales meet every temperature
                    w_soft, w_ce = (0.25 * T * T, 0.75) if mode == ref.SOFT_KL else (0.5, 0.5)
                    g = raw_distill(cuda, sd, td, mode, T, w_soft, ld, labd, w_ce, alias, gs)
                    gs32 = float(np.float32(gs))            # the entry point takes grad_scale as a float
                    want, ds, dl = ref.distill_loss(s, t, mode, T, w_soft, logits, labels, w_ce, alias, gs32)
                    what = f"B{B} D{D} x{scale:g} mode{mode} logits {lg} T{T} gs{gs:.3f}"
                    assert all(v.intact() for v in g.values()), what
                    err = abs(float(g["loss"].out[0]) - want)
                    assert np.isfinite(want) and err <= ref.loss_tol(want), (what, float(g["loss"].out[0]), want)
                    U = ref.distill_grad_bound(B, T, w_soft, w_ce if lg is not None else 0.0, gs32)
                    worst = max(worst, check_grad(g["ds"].out, ds, U, what))
                    if dl is not None:
                        worst = max(worst, check_grad(g["dl"].out, dl, U, what))
                    else:
                        assert "dl" not in g
    print(f"D {D}: {n} calls, worst gradient error / tolerance {worst:.3f}")
    if D >= 63:
        # x10 at T = 0.04: logits beyond 709 (no row maximum -> overflow) and teacher probabilities that are exactly 0
        assert (10 * np.abs(base_s)).max() / 0.04 > 709 and (ref.softmax(10.0 * base_t.astype(np.float64) / 0.04) == 0).any()


@pytest.mark.parametrize("D", D_SET)
def test_dino_loss_against_the_restatement(cuda, D):
    r = np.random.default_rng(200 + D)
    worst, n = 0.0, 0
    for V in (2, 3, 6):
        for G in (1, 2):
            for B in (1, 5):
                s = r.standard_normal((V, B, D)).astype(np.float32)
                t = r.standard_normal((G, B, D)).astype(np.float32)
                centers = {0: (0.3 * r.standard_normal(D)).astype(np.float32), D: (0.3 * r.standard_normal((B, D))).astype(np.float32)}
                sd, td = dev(s, cuda), dev(t, cuda)
                for stride, c in centers.items():
                    cd = dev(c, cuda)
                    for pairing in (ref.DINO_SKIP_FIRST, ref.DINO_SKIP_SAME):
                        for tt in (0.04, 0.07):
                            n += 1
                            gs = (1.0, 1.0 / 3.0)[(n + n // 2) % 2]
                            gs32 = float(np.float32(gs))
                            g = raw_dino(cuda, sd, td, cd, stride, tt, 0.1, pairing, gs)
                            want, ds = ref.dino_loss(s, t, c, tt, 0.1, pairing, gs32)
                            what = f"V{V} G{G} B{B} D{D} stride {stride} pairing {pairing} tt {tt}"
                            assert all(v.intact() for v in g.values()), what
                            err = abs(float(g["loss"].out[0]) - want)
                            assert err <= ref.loss_tol(want), (what, float(g["loss"].out[0]), want)
                            worst = max(worst, check_grad(g["ds"].out, ds, ref.dino_grad_bound(B, V, 0.1, gs32), what))
                            got = g["ds"].out
                            used = {v for views in ref.dino_pairs(V, G, pairing) for v in views}
                            for v in set(range(V)) - used:          # a view no pair uses: an explicit zero row
                                assert bool((got[v] == 0).all()), (what, v)
                            if V == 2 and G == 2 and pairing == ref.DINO_SKIP_FIRST:
                                assert used == {1} and (D == 1 or bool(got[1].any()))
    print(f"D {D}: {n} calls, worst gradient error / tolerance {worst:.3f}")


# ---- 2. the reference's recorded values --------------------------------------------------------------------------------
def test_fused_classes_give_the_recorded_reference_values(cuda, golden):
    g = golden("ref_losses.npz")
    T32 = lambda a, grad=False: dev(a.astype(np.float32), cuda).requires_grad_(grad)     # noqa: E731
    lab = dev(g["labels"], cuda)
    hp = pl.HyperParams
    B = g["student"].shape[0]
    fd = pl.FeatureDistributionLoss(100, hp.warmup_teacher_temp, hp.teacher_temp, hp.warmup_teacher_temp_epochs, fused=True)
    for ep in (0, 25, 50, 99):
        s, c = T32(g["student"], True), T32(g["cls"], True)
        loss = fd(s, T32(g["teacher"]), ep, lab, pred_label=c)
        loss.backward()
        U = ref.distill_grad_bound(B, fd.teacher_temp_schedule[ep], hp.beta, hp.alpha, 1.0)
        check_loss(loss.item(), float(g[f"featdist_ep{ep}"]), f"featdist ep{ep}")
        check_grad(s.grad, g[f"featdist_ep{ep}_gs"], U, f"featdist ep{ep} gs")
        check_grad(c.grad, g[f"featdist_ep{ep}_gc"], U, f"featdist ep{ep} gc")
    D = g["cls"].shape[1]
    for alpha, temp in ((1.0, 2.0), (0.5, 4.0), (0.9, 20.0)):
        c = T32(g["cls"], True)
        loss = pl.loss_fn_kd(c, lab, T32(g["tcls"]), types.SimpleNamespace(alpha=alpha, temperature=temp), fused=True)
        loss.backward()
        check_loss(loss.item(), float(g[f"kd_a{alpha}_T{temp}"]), f"kd {alpha} {temp}")
        check_grad(c.grad, g[f"kd_a{alpha}_T{temp}_g"], ref.distill_grad_bound(B, temp, alpha * temp * temp / D, 1 - alpha, 1.0),
                   f"kd {alpha} {temp}")
    fk = pl.FeatureDistributionLossKD(100, **pl.FeatureDistributionLossKD.SCHEDULE, fused=True)
    for ep in (0, 25, 50):
        c = T32(g["cls"], True)
        loss = fk(c, T32(g["tcls"]), ep, lab)
        loss.backward()
        T = fk.teacher_temp_schedule[ep]
        check_loss(loss.item(), float(g[f"featdist_spamp_ep{ep}"]), f"spamp ep{ep}")
        check_grad(c.grad, g[f"featdist_spamp_ep{ep}_g"],
                   ref.distill_grad_bound(B, T, hp.soft_target_loss_weight * T * T, hp.ce_loss_weight, 1.0), f"spamp ep{ep}")
    fs = pl.FeatureDistributionLossSoft(100, **pl.FeatureDistributionLossSoft.SCHEDULE, fused=True)
    for ep in (0, 50):
        s = T32(g["student"], True)
        loss = fs(s, T32(g["teacher"]), ep)
        loss.backward()
        T = fs.teacher_temp_schedule[ep]
        check_loss(loss.item(), float(g[f"featdist_eval_ep{ep}"]), f"eval ep{ep}")
        check_grad(s.grad, g[f"featdist_eval_ep{ep}_g"], ref.distill_grad_bound(B, T, T * T, 0.0, 1.0), f"eval ep{ep}")
    assert pl.HyperParams.T == fs.teacher_temp_schedule[50]          # the side effect is kept


def test_fused_dino_class_gives_the_recorded_reference_values(cuda, golden):
    """dino_student / dino_teacher are recorded in float64 and are not float32 numbers, so the class sees their float32
    roundings.  The kernel is held to the restatement ON THOSE ROUNDED INPUTS with the tolerances of this file; against the
    recorded values the bound grows by what the rounding of the inputs itself moves the float64 restatement (computed from
    the restatement alone: |ref(rounded inputs) - ref(recorded inputs)|), and the restatement on the recorded inputs is the
    recorded value to 1e-12 (tests/test_distill_loss_cpu.py)."""
    g = golden("ref_losses.npz")
    crit = DINOLoss(32, 6, 0.04, 0.07, 3, 10, fused=True).to(cuda)
    center64 = np.zeros((1, 32))
    for step in range(2):
        s64, t64 = g["dino_student"][step], g["dino_teacher"][step]
        s32, t32 = s64.astype(np.float32), t64.astype(np.float32)
        c32 = crit.center.cpu().numpy().reshape(-1, 32)
        temp = crit.teacher_temp_schedule[step + 1]
        s = dev(s32, cuda).requires_grad_(True)
        loss = crit(s, dev(t32, cuda), step + 1)
        loss.backward()
        want, ds = ref.dino_loss(s32, t32, c32, temp, 0.1, ref.DINO_SKIP_FIRST)
        U = ref.dino_grad_bound(5, 6, 0.1, 1.0)
        check_loss(loss.item(), want, f"dino step {step} (rounded inputs)")
        check_grad(s.grad, ds, U, f"dino step {step} (rounded inputs)")
        rec, drec = ref.dino_loss(s64, t64, center64.reshape(-1, 32), temp, 0.1, ref.DINO_SKIP_FIRST)
        assert abs(rec - float(g[f"dino_loss{step}"])) <= 1e-12 * abs(rec)
        assert abs(loss.item() - float(g[f"dino_loss{step}"])) <= ref.loss_tol(rec) + abs(want - rec) + 1e-12 * abs(rec)
        got = s.grad.double().cpu().numpy()
        assert (np.abs(got - g[f"dino_grad{step}"]) <= ref.grad_tol(drec, U) + np.abs(ds - drec) + 1e-12).all()
        center64 = g[f"dino_center{step}"]
        np.testing.assert_allclose(crit.center.cpu().numpy(), center64, atol=1e-6)
    assert crit.center.shape == (1, 5, 32)


# ---- 3. identities ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("D", [65, 1025])
def test_kl_of_a_row_with_itself_is_exactly_zero(cuda, D):
    r = np.random.default_rng(D)
    s = (10 * r.standard_normal((5, D))).astype(np.float32)
    for T in (1.65, 0.04):
        g = raw_distill(cuda, dev(s, cuda), dev(s, cuda).clone(), ref.SOFT_KL, T, T * T)
        assert float(g["loss"].out[0]) == 0.0
        check_grad(g["ds"].out, np.zeros_like(s, dtype=np.float64), ref.distill_grad_bound(5, T, T * T, 0.0, 1.0), f"T {T}")


def test_null_outputs_are_not_written_and_two_calls_give_the_same_bits(cuda):
    r = np.random.default_rng(7)
    B, D, K = 9, 384, 40
    s, t, z = (dev(r.standard_normal(sh).astype(np.float32), cuda) for sh in ((B, D), (B, D), (B, K)))
    lab = dev(r.integers(0, K, B), cuda)
    full = raw_distill(cuda, s, t, ref.SOFT_CE_OF_PROBS, 0.22, 0.5, z, lab, 0.5)
    again = raw_distill(cuda, s, t, ref.SOFT_CE_OF_PROBS, 0.22, 0.5, z, lab, 0.5)
    for k in ("loss", "ds", "dl"):
        assert torch.equal(full[k].buf.view(torch.int32), again[k].buf.view(torch.int32)), k
    for want in (("ds",), ("dl",), ()):
        part = raw_distill(cuda, s, t, ref.SOFT_CE_OF_PROBS, 0.22, 0.5, z, lab, 0.5, want=want)
        assert set(part) == {"loss", "scratch", *want} and all(v.intact() for v in part.values())
        for k in ("loss", *want):
            assert torch.equal(part[k].buf.view(torch.int32), full[k].buf.view(torch.int32)), (want, k)
    # the loss alone through the binding; an alias call never has a dlogits
    loss, ds, dl = cabi.distill_loss(s, t, cabi.SOFT_CE_OF_PROBS, 0.22, 0.5, logits=z, labels=lab, w_ce=0.5, want_grad=False)
    assert ds is None and dl is None and torch.equal(loss, full["loss"].out)
    sv, tv, c = (dev(r.standard_normal(sh).astype(np.float32), cuda) for sh in ((3, 5, 1025), (2, 5, 1025), (5, 1025)))
    a = raw_dino(cuda, sv, tv, c, 1025, 0.04, 0.1, ref.DINO_SKIP_SAME)
    b = raw_dino(cuda, sv, tv, c, 1025, 0.04, 0.1, ref.DINO_SKIP_SAME)
    assert torch.equal(a["ds"].buf.view(torch.int32), b["ds"].buf.view(torch.int32)) and torch.equal(a["loss"].buf, b["loss"].buf)
    lo = raw_dino(cuda, sv, tv, c, 1025, 0.04, 0.1, ref.DINO_SKIP_SAME, want_ds=False)
    assert torch.equal(lo["loss"].buf, a["loss"].buf) and all(v.intact() for v in (*a.values(), *lo.values()))


@pytest.mark.parametrize("bad", [None, -1])
def test_a_label_out_of_range_is_nan_in_its_row_only(cuda, bad):
    r = np.random.default_rng(9)
    B, D, K = 6, 65, 7
    s, t, z = (dev(r.standard_normal(sh).astype(np.float32), cuda) for sh in ((B, D), (B, D), (B, K)))
    lab = r.integers(0, K, B)
    good = raw_distill(cuda, s, t, ref.SOFT_CE_OF_PROBS, 0.5, 0.5, z, dev(lab, cuda), 0.5)
    lab2 = lab.copy()
    lab2[4] = K if bad is None else bad
    g = raw_distill(cuda, s, t, ref.SOFT_CE_OF_PROBS, 0.5, 0.5, z, dev(lab2, cuda), 0.5)
    torch.cuda.synchronize()            # the kernel checks the label before it uses it: nothing faulted
    assert all(v.intact() for v in g.values())
    assert bool(torch.isnan(g["loss"].out[0])) and bool(torch.isnan(g["dl"].out[4]).all())
    keep = [i for i in range(B) if i != 4]
    assert torch.equal(g["dl"].out[keep], good["dl"].out[keep]) and torch.equal(g["ds"].out, good["ds"].out)
    # the alias: the row of dstudent
    labD = r.integers(0, D, B)
    good = raw_distill(cuda, s, t, ref.SOFT_KL, 0.5, 0.5, labels=dev(labD, cuda), w_ce=0.5, alias=True)
    labD[1] = D if bad is None else bad
    g = raw_distill(cuda, s, t, ref.SOFT_KL, 0.5, 0.5, labels=dev(labD, cuda), w_ce=0.5, alias=True)
    keep = [i for i in range(B) if i != 1]
    assert bool(torch.isnan(g["loss"].out[0])) and bool(torch.isnan(g["ds"].out[1]).all())
    assert torch.equal(g["ds"].out[keep], good["ds"].out[keep]) and all(v.intact() for v in g.values())


# ---- 4. the stream contract of the two entry points ---------------------------------------------------------------------
@pytest.mark.parametrize("case", [c for v in stream_cases.CASES.values() for c in v], ids=lambda c: c.id)
def test_stream_order(cuda, case):
    """The procedure of tests/test_gpu_stream_order.py on the cases of tests/distill_loss_stream_cases.py."""
    stream_tests.test_stateless_entry_point_with_late_inputs(cuda, case)


# ---- 5. wiring ------------------------------------------------------------------------------------------------------------
def _spy_on_model_outputs(trainer):
    """Keeps what the trainer's next step hands to its loss (the features the step itself computed)."""
    seen, inner = {}, trainer.compute_loss

    def compute_loss(out, targets, labels, epoch):
        seen["out"] = out
        return inner(out, targets, labels, epoch)
    trainer.compute_loss = compute_loss
    return seen


def test_trainer_step_with_the_fused_loss(cuda):
    """One step of DistillTrainer(fused_loss=True) with featdist and with kd at (B 8, T 16, C 8, H 32, L 1): the loss within
    1e-4 of the oracle pipeline (the bound of test_gpu_parity.py::test_end_to_end_step_loss_within_1e4), and equal, bit
    for bit, to the fused class called on the same features."""
    from cerebralsignalnetworks_amd.trainer import DistillTrainer
    B, T, C, H, L, D = 8, 16, 8, 32, 1, 24
    x = eeg_filter.synthetic_eeg(B, C, T, seed=43)
    rng = np.random.default_rng(44)
    tgt = rng.standard_normal((B, D)).astype(np.float32)
    lab = rng.integers(0, 40, B)
    filt = EEGFilters(1000, order=3)

    def model(out, NC):
        p = lstm.init_params(C, H, L, out, NC, seed=43)
        m = Model(input_size=C, lstm_size=H, lstm_layers=L, output_size=out, include_top=bool(NC), n_classes=NC or 40,
                  compute_dtype=torch.float32)
        m.load_state_dict({k: torch.from_numpy(np.asarray(v)) for k, v in p.items()})
        return p, m.to(cuda)

    p, m = model(D, 40)
    tr = DistillTrainer(m, filt.sos, loss="featdist", lr=1e-3, optimizer="rmsprop", nepochs=100, fused_loss=True)
    assert tr.featdist.fused and tr.fused_loss
    seen = _spy_on_model_outputs(tr)
    loss = tr.train_step(dev(x, cuda), dev(tgt, cuda), dev(lab, cuda), epoch=25)
    feat, cls = (o.detach() for o in seen["out"])
    same = tr.featdist(feat, dev(tgt, cuda), 25, dev(lab, cuda), pred_label=cls)
    feat_ref, cls_ref = lstm.model_forward(eeg_filter.eeg_bandpass_znorm(x, filt.sos), p, L, include_top=True)
    want = oracle_losses.feature_distribution_loss(feat_ref, tgt, oracle_losses.teacher_temp_schedule(100)[25], lab, cls_ref)
    print(f"featdist step: fused {loss.item()!r} oracle {want!r}")
    assert abs(loss.item() - want) < 1e-4
    assert loss.item() == same.item()

    kd = types.SimpleNamespace(alpha=0.5, temperature=4.0)
    p2, m2 = model(40, None)
    teacher = rng.standard_normal((B, 40)).astype(np.float32)
    tr2 = DistillTrainer(m2, filt.sos, loss="kd", kd_params=kd, fused_loss=True)
    seen = _spy_on_model_outputs(tr2)
    loss2 = tr2.train_step(dev(x, cuda), dev(teacher, cuda), dev(lab, cuda))
    out = seen["out"][0] if isinstance(seen["out"], tuple) else seen["out"]
    same = pl.loss_fn_kd(out.detach(), dev(lab, cuda), dev(teacher, cuda), kd, fused=True)
    feat2 = lstm.model_forward(eeg_filter.eeg_bandpass_znorm(x, filt.sos), p2, L)
    want2 = oracle_losses.loss_fn_kd(feat2, lab, teacher, 0.5, 4.0)
    print(f"kd step: fused {loss2.item()!r} oracle {want2!r}")
    assert abs(loss2.item() - want2) < 1e-4
    assert loss2.item() == same.item()
    # the step moved the parameters (the saved gradient reached the optimiser)
    assert not np.array_equal(m2.fc.weight.detach().cpu().numpy(), p2["fc.weight"])


@pytest.mark.parametrize("tool", ["featdist", "kd", "dino"])
def test_command_line_tools_run_with_fused_loss(cuda, tmp_path, tool):
    """One --synthetic 64 --fused_loss epoch of LstmDistillFromDinoV2Train.py (featdist, its default loss), of its
    Spampinato flavour (kd) and of LstmDistillation.py (DINO) ends with a finite loss."""
    common = ["--synthetic", "64", "--batch_size", "16", "--num_epochs", "1", "--hidden_size", "32", "--lstm_layers", "1",
              "--dtype", "f32", "--fused_loss", "--log_dir", str(tmp_path)]
    if tool == "featdist":
        import LstmDistillFromDinoV2Train as train
        assert train.build_parser(train.PERILS).parse_args(common).loss == "featdist"
        hist = train.main(common)
    elif tool == "kd":
        import LstmDistillFromDinoV2TrainSpampinato as spamp
        hist = spamp.main(common + ["--hyperprams", "{'alpha': 0.3, 'temperature': 2}"])
    else:
        import LstmDistillation as dino_cli
        hist = dino_cli.main(["--synthetic", "64", "--batch_size_per_gpu", "16", "--epochs", "1", "--embed_dim", "32",
                              "--lstm_layers", "1", "--out_dim", "64", "--log_dir", str(tmp_path), "--warmup_epochs", "1",
                              "--warmup_teacher_temp_epochs", "1", "--dtype", "f32", "--fused_loss"])
    assert len(hist) == 1 and np.isfinite(hist[0])


def test_dino_step_with_the_fused_loss_matches_the_reference_fixture(cuda, golden):
    """The step of tests/test_gpu_fullsize.py::test_dino_self_distillation_step_matches_reference_fixture with fused=True."""
    g = golden("ref_dino_step.npz")
    B, C, H, L, OUT = (int(v) for v in g["dims"])
    p = lstm.init_params(C, H, L, H, None, seed=int(g["seed_params"]))
    head_sd = {k[len("sd__head."):]: torch.from_numpy(g[k]).float() for k in g.files if k.startswith("sd__head.")}

    def build():
        bb = Model(input_size=C, lstm_size=H, lstm_layers=L, output_size=H, include_top=False, compute_dtype=torch.float32)
        bb.load_state_dict({k: torch.from_numpy(np.asarray(v)) for k, v in p.items()})
        head = DINOHead(H, OUT, nlayers=3, hidden_dim=48, bottleneck_dim=16)
        head.load_state_dict(head_sd)
        return MultiCropWrapper(bb, head).to(cuda)

    student, teacher = build(), build()
    crit = DINOLoss(OUT, 6, 0.04, 0.07, 3, 10, fused=True).to(cuda)
    views = [torch.from_numpy(g[f"view{i}"]).to(cuda) for i in range(6)]
    with torch.no_grad():
        teacher_outputs = torch.stack([teacher(v) for v in views[:2]], dim=0)
    student_outputs = torch.stack([student(v) for v in views], dim=0)
    loss = crit(student_outputs, teacher_outputs, 0)
    loss.backward()
    torch.cuda.synchronize()
    print(f"dino step: fused {loss.item()!r} fixture {float(g['loss'])!r}")
    assert abs(loss.item() - float(g["loss"])) < 1e-4
    np.testing.assert_allclose(crit.center.cpu().numpy(), g["center"], atol=1e-6)
    checked = 0
    for name, par in student.named_parameters():
        key = "grad__" + name
        if key in g.files:
            want = g[key]
            np.testing.assert_allclose(par.grad.cpu().numpy(), want, atol=1e-4 * max(1e-3, np.abs(want).max()), err_msg=name)
            checked += 1
    assert checked >= 14
