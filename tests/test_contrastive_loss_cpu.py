"""CPU: the contrastive loss -- the float64 numpy restatement of csn_contrastive_lse and
csn_contrastive_grad (tests/contrastive_loss_reference.py) against float64 autograd of the plain one-process formula, the
decomposition over ranks, the torch form of losses.ContrastiveLoss on one process and on two gloo processes, the trainer and
CLI surface, and the two measured constants the GPU tests read."""
import itertools
import os
import sys

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp
import torch.nn.functional as F

import contrastive_loss_reference as ref
import contrastive_loss_stream_cases  # noqa: F401  (joins the stream-order case table on import)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REL = 1e-12


def plain_formula(s, t, groups, a, w_a=0.5, w_b=0.5):
    """The one-process loss in torch ops, as a user would write it (any float dtype; autograd through everything)."""
    sh, th = F.normalize(s, dim=1, eps=1e-12), F.normalize(t, dim=1, eps=1e-12)
    z = a * (sh @ th.T)
    N = z.shape[0]
    if groups is not None:
        out = (groups[:, None] == groups[None, :]) & ~torch.eye(N, dtype=torch.bool)
        z = z.masked_fill(out, float("-inf"))
    p = torch.diagonal(z)
    return (w_a * (torch.logsumexp(z, 1) - p) + w_b * (torch.logsumexp(z, 0) - p)).sum() / N


def autograd_of_plain(s, t, groups, a, **kw):
    s64 = torch.tensor(np.asarray(s, np.float64), requires_grad=True)
    a64 = torch.tensor(float(a), dtype=torch.float64, requires_grad=True)
    g = None if groups is None else torch.from_numpy(np.asarray(groups))
    loss = plain_formula(s64, torch.tensor(np.asarray(t, np.float64)), g, a64, **kw)
    ds, da = torch.autograd.grad(loss, (s64, a64))
    return loss.item(), ds.numpy(), da.item()


def close(got, want, what, rel=REL, scale=None):
    """Within ``rel`` of the largest element -- of ``scale`` where given: the same formula with absolute values throughout,
    the natural size of a gradient that cancels (with D = 1 the projection leaves exactly 0 of it, and autograd's rounding)."""
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    scale = max(float(np.abs(want if scale is None else scale).max()), 1e-300)
    err = float(np.abs(got - want).max())
    assert err <= rel * scale, (what, err / scale)
    return err / scale


def restated(s, t, groups, a, world=1, **kw):
    return ref.contrastive_sharded(s, t, groups, world, a, **kw)


# ---- 1. the restatement against float64 autograd ----------------------------------------------------------------------------
@pytest.mark.parametrize("N,D", list(itertools.product((1, 2, 5, 12), (1, 7))))
def test_restatement_against_float64_autograd(N, D):
    r = np.random.default_rng(10 * N + D)
    worst = 0.0
    for a, grouped in itertools.product((1.0, 1.0 / 0.07, 1e4), (False, True)):
        s, t = r.standard_normal((N, D)), r.standard_normal((N, D))
        groups = r.integers(0, max(N // 2, 1), size=N).astype(np.int32) if grouped else None
        loss, ds, da = autograd_of_plain(s, t, groups, a)
        got_loss, _, got_ds, got_da, U, Ua = restated(s, t, groups, a)
        what = f"N{N} D{D} a{a:g} groups{grouped}"
        assert abs(got_loss - loss) <= REL * max(abs(loss), 1e-300) or (loss == 0.0 and got_loss == 0.0), (what, got_loss, loss)
        worst = max(worst, close(got_ds, ds, what + " ds", scale=U), close(got_da, da, what + " dscale", scale=Ua))
        if N == 1:
            assert got_loss == 0.0 and not got_ds.any() and got_da == 0.0, what
    print(f"N{N} D{D}: worst relative distance from autograd {worst:.2e}")


def test_special_rows_against_float64_autograd():
    """A row whose every other key is left out (loss term 0, zero gradient), a zero row (no projection, divided by eps), a
    row with 0 < |s| < 1e-12 (likewise), and weights other than one half."""
    r = np.random.default_rng(5)
    N, D, a = 9, 7, 1.0 / 0.07
    s, t = r.standard_normal((N, D)), r.standard_normal((N, D))
    s[2] = 0.0
    s[4] = 1e-14 * r.standard_normal(D)
    assert 0.0 < np.linalg.norm(s[4]) < 1e-12
    groups = np.array([3, 3, 5, 3, 6, 7, 3, -2 ** 31, 2 ** 31 - 1], np.int32)
    everything = np.full(N, 11, np.int32)
    for g, kw in ((groups, {}), (everything, {}), (groups, dict(w_a=0.8, w_b=-0.3)), (None, dict(w_a=1.0, w_b=0.0))):
        loss, ds, da = autograd_of_plain(s, t, g, a, **kw)
        got_loss, rows, got_ds, got_da, U, Ua = restated(s, t, g, a, **kw)
        assert abs(got_loss - loss) <= REL * max(abs(loss), 1e-300) or (loss == 0.0 and got_loss == 0.0)
        close(got_ds, ds, "ds", scale=U)
        close(got_da, da, "dscale", scale=Ua)
        if g is everything:         # every query alone with its positive: lA = lB = p, nothing to learn
            assert got_loss == 0.0 and not got_ds.any() and np.array_equal(rows[0], rows[2]) and np.array_equal(rows[1], rows[2])
    # the tiny and the zero row are divided by eps, not by their norm, and are not projected
    _, _, got_ds, _, _, _ = restated(s, t, None, a)
    assert np.abs(got_ds[2]).max() > 1e9 and np.abs(got_ds[4]).max() > 1e9


# ---- 2. the decomposition over ranks ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("world", [2, 3])
def test_rank_decomposition(world):
    r = np.random.default_rng(world)
    N, D, a = 12, 7, 1.0 / 0.07
    s, t = r.standard_normal((N, D)).astype(np.float32), r.standard_normal((N, D)).astype(np.float32)
    groups = np.array([0, 1, 2, 0, 4, 5, 1, 7, 8, 0, 10, 5], np.int32)          # duplicates inside and across ranks
    for g in (None, groups):
        loss, ds, da = autograd_of_plain(s, t, g, a)
        one = restated(s, t, g, a)
        many = restated(s, t, g, a, world=world, grad_scale=float(world))
        close(many[0], loss, "the partials add up to the global loss", 1e-14)
        close(many[1], one[1], "rows_out", 1e-14)
        close(many[2] / world, one[2], "the ds slices are the global gradient's rows", 1e-14)
        close(many[2] / world, ds, "ds against autograd")
        close(many[3], da, "dscale partials")


# ---- 3. the torch form of the module -------------------------------------------------------------------------------------------
def test_torch_form_module_matches_the_restatement_in_float64():
    from cerebralsignalnetworks_amd.losses import ContrastiveLoss
    r = np.random.default_rng(7)
    N, D = 12, 7
    s, t = r.standard_normal((N, D)), r.standard_normal((N, D))
    groups = np.array([0, 1, 2, 0, 4, 5, 1, 7, 8, 0, 10, 5], np.int32)
    for temperature, g, kw in ((0.07, None, {}), (0.07, groups, {}), (1.0, groups, dict(w_s2t=0.8, w_t2s=0.1)),
                               (1e-4, groups, dict(max_scale=1e4))):
        crit = ContrastiveLoss(temperature=temperature, **kw)
        a = crit.scale()[0]
        assert a == min(1.0 / temperature, kw.get("max_scale", 100.0))
        x = torch.tensor(s, requires_grad=True)
        loss = crit(x, torch.tensor(t), None if g is None else torch.from_numpy(g))
        assert loss.dim() == 0 and loss.dtype == torch.float64
        (2.0 * loss).backward()
        want = restated(s, t, g, a, w_a=kw.get("w_s2t", 0.5), w_b=kw.get("w_t2s", 0.5))
        close(loss.item(), want[0], "loss")
        close(x.grad.numpy(), 2.0 * want[2], "ds")
        with torch.no_grad():               # evaluation: the same value, nothing saved for a backward
            again = crit(x, torch.tensor(t), None if g is None else torch.from_numpy(g))
        assert again.item() == loss.item() and not again.requires_grad
    with pytest.raises(ValueError, match="groups"):
        ContrastiveLoss()(torch.zeros(4, 3), torch.zeros(4, 3), torch.zeros(5, dtype=torch.int64))
    with pytest.raises(ValueError, match="temperature"):
        ContrastiveLoss(temperature=0.0)


def test_learnable_temperature_gradient_matches_autograd():
    from cerebralsignalnetworks_amd.losses import ContrastiveLoss
    r = np.random.default_rng(8)
    N, D = 10, 5
    s, t = torch.tensor(r.standard_normal((N, D))), torch.tensor(r.standard_normal((N, D)))
    groups = torch.from_numpy(r.integers(0, 6, size=N))
    crit = ContrastiveLoss(temperature=0.2, learnable_temperature=True).double()
    assert isinstance(crit.log_scale, torch.nn.Parameter) and abs(crit.scale()[0] - 5.0) < 1e-6
    x = s.clone().requires_grad_(True)
    crit(x, t, groups).backward()
    ls = crit.log_scale.detach().clone().requires_grad_(True)
    x2 = s.clone().requires_grad_(True)
    plain_formula(x2, t, groups, torch.exp(torch.clamp(ls, max=float(np.log(100.0))))).backward()
    close(crit.log_scale.grad.item(), ls.grad.item(), "d loss / d log_scale")
    close(x.grad.numpy(), x2.grad.numpy(), "ds")
    # above the clamp the scale is max_scale and log_scale gets a zero gradient; a fixed temperature is no parameter
    crit = ContrastiveLoss(temperature=0.001, learnable_temperature=True, max_scale=50.0).double()
    crit(s.clone().requires_grad_(True), t, groups).backward()
    assert crit.scale() == (50.0, False) and crit.log_scale.grad.item() == 0.0 and crit.log_scale.grad.dtype == torch.float64
    assert list(ContrastiveLoss().parameters()) == []


# ---- 4. two processes over gloo ----------------------------------------------------------------------------------------------------
def _problem():
    r = np.random.default_rng(21)
    x = torch.tensor(r.standard_normal((8, 6)))
    t = torch.tensor(r.standard_normal((8, 5)))
    groups = torch.tensor([0, 1, 2, 0, 4, 1, 6, 0])            # duplicates inside a rank and across the two
    return x, t, groups


def _encoder():
    torch.manual_seed(3)
    return torch.nn.Linear(6, 5).double()


def _gloo_worker(rank, world, port, out):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world))
    dist.init_process_group("gloo", rank=rank, world_size=world)
    sys.path.insert(0, ROOT)
    from cerebralsignalnetworks_amd.losses import ContrastiveLoss
    x, t, groups = _problem()
    mine = slice(rank * 4, (rank + 1) * 4)
    enc = _encoder()
    loss = ContrastiveLoss()(enc(x[mine]), t[mine], groups[mine])
    loss.backward()
    flat = torch.cat([p.grad.reshape(-1) for p in enc.parameters()])
    dist.all_reduce(flat)           # the mean all-reduce of FlatGrads.all_reduce_mean, in the float64 of this test
    flat /= world
    refused = ""
    try:                        # unequal rows per rank are refused, on every rank, before anything is gathered
        ContrastiveLoss()(enc(x[:3 + rank]), t[:3 + rank])
    except ValueError as e:
        refused = str(e)
    out[rank] = (loss.item(), flat.numpy(), refused)
    dist.barrier()
    dist.destroy_process_group()


def test_two_process_gloo_gives_the_global_loss_and_gradient():
    world, port = 2, 29641
    out = mp.Manager().dict()
    mp.spawn(_gloo_worker, args=(world, port, out), nprocs=world, join=True)
    x, t, groups = _problem()
    enc = _encoder()
    loss = plain_formula(enc(x), t, groups, 1.0 / 0.07)
    loss.backward()
    want = torch.cat([p.grad.reshape(-1) for p in enc.parameters()]).numpy()
    for rank in range(world):
        got_loss, flat, refused = out[rank]
        assert got_loss == out[0][0]
        close(got_loss, loss.item(), "the global loss on every rank")
        close(flat, want, "the averaged parameter gradients are the one-process gradients")
        assert "same number of rows" in refused and "[3, 4]" in refused


# ---- 5. trainer and CLI ------------------------------------------------------------------------------------------------------------
class _CpuModel(torch.nn.Module):
    def __init__(self):
        super().__init__()
        self.fc = torch.nn.Linear(4, 3)

    def forward(self, x):
        return self.fc(x[:, -1])


def test_trainer_takes_the_loss_and_refuses_micro_batches():
    from cerebralsignalnetworks_amd.trainer import DistillTrainer
    from cerebralsignalnetworks_amd.losses import ContrastiveLoss
    with pytest.raises(ValueError, match="contrastive is a batch-level loss"):
        DistillTrainer(_CpuModel(), None, loss="contrastive", optimizer="adam", accum_steps=2)
    tr = DistillTrainer(_CpuModel(), None, loss="contrastive", optimizer="adam", contrastive_temperature=0.2, preprocess=False)
    assert isinstance(tr.contrastive, ContrastiveLoss) and tr.contrastive.scale() == (5.0, False) and not tr.contrastive.fused
    assert DistillTrainer(_CpuModel(), None, loss="cosine", optimizer="adam").contrastive is None
    # one CPU step with group ids: the trainer's loss is the module's loss on the model's output
    r = np.random.default_rng(2)
    x = torch.tensor(r.standard_normal((6, 4, 5)), dtype=torch.float32)          # [B,C,T]
    tgt = torch.tensor(r.standard_normal((6, 3)), dtype=torch.float32)
    groups = torch.tensor([0, 1, 0, 3, 4, 1])
    want = ContrastiveLoss(temperature=0.2)(tr.model(tr.embed(x)), tgt, groups).item()
    assert tr.train_step(x, tgt, groups=groups).item() == want
    assert tr.train_step(x, tgt, groups=groups).item() != want                  # the step moved the parameters


def test_cli_parsers_accept_the_new_flags():
    import LstmDistillFromDinoV2Train as train
    import LstmDistillFromDinoV2Eval as evaluate
    for flavour in (train.PERILS, train.SPAMPINATO):
        p = train.build_parser(flavour)
        d = p.parse_args([])
        assert d.loss == flavour.loss and d.contrastive_temperature == 0.07 and d.contrastive_mask == "image"
        assert d.normalize_embeddings is False
        f = p.parse_args(["--loss", "contrastive", "--contrastive_temperature", "0.05", "--contrastive_mask", "class",
                          "--normalize_embeddings", "--fused_loss"])
        assert (f.loss, f.contrastive_temperature, f.contrastive_mask, f.normalize_embeddings, f.fused_loss) == \
            ("contrastive", 0.05, "class", True, True)
        with pytest.raises(SystemExit):
            p.parse_args(["--contrastive_mask", "subject"])
    assert evaluate.build_parser().parse_args(["--normalize_embeddings"]).normalize_embeddings is True
    rows = train.normalize_rows(torch.tensor([[3.0, 4.0], [0.0, 0.0]]))
    assert torch.equal(rows, torch.tensor([[0.6, 0.8], [0.0, 0.0]]))
    np.testing.assert_allclose(train.normalize_rows([np.array([3.0, 4.0])])[0], [0.6, 0.8])


def test_synthetic_dataset_has_image_ids():
    from cerebralsignalnetworks_amd.dataset import EEGDataset
    d = EEGDataset(synthetic=6, synthetic_channels=4, synthetic_samples=20, time_low=0, time_high=20, feature_dim=3,
                   device=torch.device("cpu"))
    assert torch.equal(d.image_ids_dev, torch.arange(6))


# ---- 6. the measured constants the GPU tests read -------------------------------------------------------------------------------------
def _all_cases():
    return [c for D in ref.D_SET for c in ref.gpu_cases(D)] + [dict(ref.BIG_CASE, row0s=[ref.BIG_CASE["row0"]])]


def test_gpu_cases_cover_every_setting():
    cases = [c for D in ref.D_SET for c in ref.gpu_cases(D)]
    seen = {(c["input_scale"], c["scale"], c["grad_scale"], c["groups"], c["want_dscale"]) for c in cases}
    assert len(seen) == 3 * 4 * 2 * 3 * 2
    assert {(c["B"], c["D"]) for c in cases} == set(itertools.product(ref.B_SET, ref.D_SET))
    for c in cases:
        assert c["N"] in (c["B"], 2 * c["B"], 3 * c["B"] + 1) and c["row0s"][0] == 0 and c["row0s"][-1] == c["N"] - c["B"]


def test_measured_constants_hold():
    """(a) SPREAD: two float64 evaluation orders of the restatement, in units of U, over the cases of the GPU test.
    (b) TORCH_FORM_*: the float32 torch form against the restatement over the same cases at logit scales <= 100, the loss in
    units of ref.loss_scale and the gradient in units of the largest U (a gradient that cancels to nothing, as with D = 1 or
    with every other key left out, has no size of its own).
    Both are measured again here.  The sums run through the host's BLAS, whose blocking and thread count decide the order of
    a float64 or float32 sum, so a measurement on another machine is another sample of the same quantity: it is held to
    twice the recorded value (c = 10 x SPREAD keeps a factor of 5 over such a sample), and c <= 1e-9 is held as it stands."""
    from cerebralsignalnetworks_amd.losses import ContrastiveLoss
    spread, b_loss, b_grad = 0.0, 0.0, 0.0
    for c in _all_cases():
        s, t, g = ref.make_inputs(c)
        N, a = c["N"], c["scale"]
        rows, rows_r = (ref.contrastive_lse(s, t, g, 0, N, a, reverse=rv)[0] for rv in (False, True))
        fwd = ref.contrastive_grad(s, t, g, 0, N, a, rows[0], rows[1], grad_scale=c["grad_scale"])
        rev = ref.contrastive_grad(s, t, g, 0, N, a, rows_r[0], rows_r[1], grad_scale=c["grad_scale"], reverse=True)
        spread = max(spread, float((np.abs(fwd[0] - rev[0]) / np.maximum(fwd[2], 1e-300)).max()))
        if a <= 100.0:
            crit = ContrastiveLoss(temperature=1.0 / a)
            x = torch.from_numpy(s).requires_grad_(True)
            loss = crit(x, torch.from_numpy(t), None if g is None else torch.from_numpy(g))
            loss.backward()
            want = ref.contrastive_lse(s, t, g, 0, N, a)[1]
            b_loss = max(b_loss, abs(loss.item() - want) / ref.loss_scale(rows))
            b_grad = max(b_grad, float(np.abs(x.grad.numpy() * c["grad_scale"] - fwd[0]).max()) / float(fwd[2].max()))
    print(f"(a) spread {spread:.3e} (recorded {ref.SPREAD:g}); (b) torch form: loss {b_loss:.3e} (recorded {ref.TORCH_FORM_LOSS:g}), "
          f"gradient {b_grad:.3e} (recorded {ref.TORCH_FORM_GRAD:g})")
    assert spread <= 2 * ref.SPREAD and ref.C_NOISE == 10 * ref.SPREAD and ref.C_NOISE <= 1e-9
    assert b_loss <= 2 * ref.TORCH_FORM_LOSS and b_grad <= 2 * ref.TORCH_FORM_GRAD
