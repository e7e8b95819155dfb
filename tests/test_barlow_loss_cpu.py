"""CPU: the fused Barlow-Twins loss (csrc/barlow_loss.hip) as far as it can be checked without a GPU
-- the numpy restatement of the two entry points (tests/barlow_loss_reference.py) against the oracle on one and two ranks,
the reference's recorded values, float64 autograd of the torch class and a float64 nn.BatchNorm1d; the symbols and their
host-side refusals; and the rule that ``fused=True`` on CPU tensors, on float64 tensors and in eval() is the torch form."""
import inspect
import os

import numpy as np
import pytest
import torch

import __graft_entry__ as graft
import barlow_loss_reference as ref
import barlow_loss_stream_cases as stream_cases      # joins the stream-order case table on import
import stream_order as so
from cerebralsignalnetworks_amd import cabi
from cerebralsignalnetworks_amd import losses as pl
from oracle import losses as oracle_losses

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("csn_barlow_saved_bytes", "csn_barlow_scratch_bytes", "csn_barlow_corr", "csn_barlow_grad")
INVALID = 1                              # CSN_ERR_INVALID_ARGUMENT


@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(cabi.LIB_PATH):
        graft.build()
    return cabi.load()


def inputs(r, B, D, scale=1.0, shift=0.0, constant_column=True):
    """float32 [B,D] pairs; ``shift``: every column moved by that many column standard deviations."""
    z1, z2 = (r.standard_normal((B, D)) * scale + shift * scale for _ in range(2))
    z1, z2 = z1.astype(np.float32), z2.astype(np.float32)
    if constant_column and D > 1:
        z1[:, 0] = z1[0, 0]              # var = 0 exactly
    return z1, z2


# ---- 1. the restatement against the oracle --------------------------------------------------------------------------------
@pytest.mark.parametrize("world", [1, 2])
def test_restatement_equals_the_oracle(world):
    """Within 1e-12 U: both sides are float64, in different summation orders (the oracle goes through the explicit
    batch-norm backward, mean_b dzn included).  The loss is held to 1e-12 of ITS form with absolute values,
    sum (|c_ii| + 1)^2 + lambd sum c_ij^2: (c_ii - 1)^2 cancels where a column pair correlates perfectly (B 2, D 1)."""
    r = np.random.default_rng(world)
    worst = 0.0
    for B in (2, 3, 5, 64, 65):
        for D in (1, 5, 65, 384):
            for scale, shift in ((1.0, 0.0), (10.0, 0.0), (1e-3, 0.0), (1.0, 100.0)):
                z1, z2 = inputs(r, B * world, D, scale, shift)
                for gs in (1.0, 1.0 / 3.0):
                    want, c, grads = oracle_losses.barlow_loss_sharded(z1, z2, world, ref.LAMBD)
                    loss, c2, got = ref.barlow_sharded(z1, z2, world, ref.LAMBD, gs)
                    labs = ((np.abs(np.diagonal(c)) + 1.0) ** 2).sum() + ref.LAMBD * oracle_losses.off_diagonal_sqsum(c)
                    assert abs(loss - want) <= 1e-12 * labs
                    np.testing.assert_allclose(c2, c, rtol=0, atol=1e-12 * max(1.0, np.abs(c).max()))
                    for (g1, g2), (d1, d2, U1, U2) in zip(grads, got):
                        for g, d, U in ((g1, d1, U1), (g2, d2, U2)):
                            ratio = np.abs(d - gs * g) / (1e-12 * U + ref.F32_TINY)
                            worst = max(worst, float(ratio.max()))
                            assert ratio.max() <= 1.0, (B, D, scale, shift, world, float(ratio.max()))
    print(f"world {world}: worst |restatement - oracle| / (1e-12 U) = {worst:.3f}")


def test_restatement_equals_the_recorded_reference_values(golden):
    """The bounds of tests/test_ref_pinned.py: rtol 1e-12 on the loss, atol 1e-13 on the gradients."""
    g = golden("ref_losses.npz")
    loss, _, got = ref.barlow_sharded(g["barlow_z1"], g["barlow_z2"], 1)
    np.testing.assert_allclose(loss, g["barlow_loss"], rtol=1e-12)
    np.testing.assert_allclose(got[0][0], g["barlow_g1"], atol=1e-13)
    np.testing.assert_allclose(got[0][1], g["barlow_g2"], atol=1e-13)
    g = golden("ref_barlow_2rank.npz")
    loss, _, got = ref.barlow_sharded(g["z1"], g["z2"], 2)
    for r in range(2):
        np.testing.assert_allclose(loss, g[f"loss_r{r}"], rtol=1e-12)
        np.testing.assert_allclose(got[r][0], g[f"g1_r{r}"], atol=1e-13)
        np.testing.assert_allclose(got[r][1], g[f"g2_r{r}"], atol=1e-13)


# ---- 2. the restatement against float64 autograd of the torch class, and its running statistics ----------------------------
@pytest.mark.parametrize("B,D", [(2, 1), (5, 7), (33, 65)])
def test_restatement_equals_autograd_of_the_torch_class(B, D):
    r = np.random.default_rng(B + D)
    z1, z2 = inputs(r, B, D, constant_column=False)
    a = torch.from_numpy(z1.astype(np.float64)).requires_grad_(True)
    b = torch.from_numpy(z2.astype(np.float64)).requires_grad_(True)
    crit = pl.BarlowTwinsLoss(D, B, lambd=0.02).double().train()
    loss = crit(a, b)
    (0.5 * loss).backward()
    want, _, got = ref.barlow_sharded(z1, z2, 1, 0.02, grad_scale=0.5)
    d1, d2, U1, U2 = got[0]
    np.testing.assert_allclose(loss.item(), want, rtol=1e-12)
    assert (np.abs(a.grad.numpy() - d1) <= 1e-12 * U1).all() and (np.abs(b.grad.numpy() - d2) <= 1e-12 * U2).all()


def test_running_statistics_are_those_of_one_batchnorm_called_twice():
    r = np.random.default_rng(11)
    z1, z2 = inputs(r, 9, 13, scale=3.0, shift=2.0, constant_column=False)
    bn = torch.nn.BatchNorm1d(13, affine=False, momentum=0.3).double().train()
    rm0, rv0 = r.standard_normal(13).astype(np.float32), (1 + r.random(13)).astype(np.float32)
    with torch.no_grad():
        bn.running_mean.copy_(torch.from_numpy(rm0))
        bn.running_var.copy_(torch.from_numpy(rv0))
    n1, n2 = bn(torch.from_numpy(z1.astype(np.float64))), bn(torch.from_numpy(z2.astype(np.float64)))
    c, saved, (rm, rv) = ref.barlow_corr(z1, z2, 1.0 / 9, bn.eps, rm0, rv0, 0.3)
    assert rm.dtype == rv.dtype == np.float32 and int(bn.num_batches_tracked) == 2
    # the restatement rounds to float32 after each of the two updates; the float64 module does not
    np.testing.assert_array_less(np.abs(rm - bn.running_mean.numpy()), ref.stats_tol(rm0, saved[0], saved[2]) + 1e-300)
    var1, var2 = z1.astype(np.float64).var(0, ddof=1), z2.astype(np.float64).var(0, ddof=1)
    np.testing.assert_array_less(np.abs(rv - bn.running_var.numpy()), ref.stats_tol(rv0, var1, var2) + 1e-300)
    np.testing.assert_allclose(c, (n1.T @ n2).numpy() / 9, atol=1e-13)
    # without buffers nothing comes back
    assert ref.barlow_corr(z1, z2, 1.0 / 9)[2] is None


# ---- 3. ABI -----------------------------------------------------------------------------------------------------------------
def test_symbols_are_exported_bound_and_declared(lib):
    text = open(os.path.join(ROOT, "include", "csn_hip.h")).read()
    for name in NAMES:
        assert name in cabi.SIGNATURES and hasattr(lib, name)
        assert name + "(" in text
    assert hasattr(cabi, "barlow_corr") and hasattr(cabi, "barlow_grad")
    assert lib.csn_abi_version() == cabi.ABI_VERSION == 6, "added symbols do not bump the ABI"
    assert "#define CSN_ABI_VERSION 6" in text
    assert lib.csn_barlow_saved_bytes(384) == 4 * 384 * 8 and lib.csn_barlow_saved_bytes(0) == 0
    assert lib.csn_barlow_scratch_bytes(0, 8) == 0 and lib.csn_barlow_scratch_bytes(8, 0) == 0
    for D in (1, 16, 17, 384, 1025):
        n = lib.csn_barlow_scratch_bytes(256, D)
        assert n % 8 == 0 and n >= 8 * (2 * D + 2), D                  # k1, k2, the two loss terms at the least
        assert n == lib.csn_barlow_scratch_bytes(2, D), "the scratch layout depends on D only"
    src = open(os.path.join(ROOT, "cerebralsignalnetworks_amd", "csrc", "Makefile")).read()
    assert "barlow_loss.hip" in src


def test_stream_order_cases_are_registered():
    for name in ("csn_barlow_corr", "csn_barlow_grad"):
        cases = so.CASE_TABLE[name]
        assert cases is stream_cases.CASES[name] and cases
        assert all(isinstance(c, so.Stateless) and c.entry == name and callable(c.build) for c in cases)
    ids = [c.id for v in stream_cases.CASES.values() for c in v]
    assert len(set(ids)) == len(ids) and not set(ids) & {c.id for c in so.STATELESS_CASES}
    n = len(so.CASE_TABLE)
    stream_cases.register()
    assert len(so.CASE_TABLE) == n, "registering twice adds nothing"


# ---- 4. refusals ------------------------------------------------------------------------------------------------------------
ONE = 1 << 12                            # any non-null, 8-byte aligned address: refused arguments are never dereferenced
NAN, INF = float("nan"), float("inf")


def _refused(lib, rc, word):
    msg = lib.csn_last_error()
    assert rc == INVALID, (rc, msg)
    assert word in msg, (word, msg)


def test_corr_refusals_happen_on_the_host(lib):
    """No GPU here: every one of these returns before any launch, with a message."""
    def call(z1=ONE, z2=ONE, B=4, D=8, eps=1e-5, inv_batch=0.25, c=ONE, saved=ONE, rm=None, rv=None, momentum=0.1):
        return lib.csn_barlow_corr(z1, z2, B, D, eps, inv_batch, c, saved, rm, rv, momentum, None)

    for null in ("z1", "z2", "c", "saved"):
        _refused(lib, call(**{null: None}), b"null")
    for kw in (dict(B=1), dict(B=0), dict(B=-4), dict(D=0), dict(D=-1)):
        _refused(lib, call(**kw), b"shape")
    for eps in (0.0, -1e-5, NAN, INF):
        _refused(lib, call(eps=eps), b"eps")
    for v in (0.0, -0.25, NAN, INF):
        _refused(lib, call(inv_batch=v), b"inv_batch")
    for m in (-0.1, 1.5, NAN, INF):
        _refused(lib, call(rm=ONE, rv=ONE, momentum=m), b"momentum")
    _refused(lib, call(rm=ONE), b"go together")
    _refused(lib, call(rv=ONE), b"go together")
    _refused(lib, call(c=ONE + 4), b"aligned")
    _refused(lib, call(saved=ONE + 4), b"aligned")


def test_grad_refusals_happen_on_the_host(lib):
    def call(z1=ONE, z2=ONE, B=4, D=8, c=ONE, c_local=ONE, saved=ONE, inv_batch=0.25, lambd=0.0051, loss=ONE, scratch=ONE):
        return lib.csn_barlow_grad(z1, z2, B, D, c, c_local, saved, inv_batch, lambd, 1.0, loss, ONE, ONE, scratch, None)

    for null in ("z1", "z2", "c", "c_local", "saved", "loss", "scratch"):
        _refused(lib, call(**{null: None}), b"null")
    for kw in (dict(B=1), dict(B=0), dict(D=0), dict(D=-3)):
        _refused(lib, call(**kw), b"shape")
    for v in (0.0, -1.0, NAN, INF):
        _refused(lib, call(inv_batch=v), b"inv_batch")
    for v in (NAN, INF, -INF):
        _refused(lib, call(lambd=v), b"lambd")
    for name in ("c", "c_local", "saved", "scratch"):
        _refused(lib, call(**{name: ONE + 4}), b"aligned")


def test_bindings_refuse_host_tensors():
    x = torch.zeros(4, 8)
    with pytest.raises(cabi.CsnError):
        cabi.barlow_corr(x, x, 4)
    with pytest.raises(cabi.CsnError):
        cabi.barlow_grad(x, x, torch.zeros(8, 8, dtype=torch.float64), torch.zeros(8, 8, dtype=torch.float64),
                         torch.zeros(4, 8, dtype=torch.float64), 4, 0.0051)


# ---- 5. fused=True outside its conditions is the torch form ------------------------------------------------------------------
def _run(crit, z1, z2):
    z1, z2 = z1.clone().requires_grad_(True), z2.clone().requires_grad_(True)
    loss = crit(z1, z2)
    loss.backward()
    return [loss.detach(), z1.grad, z2.grad, crit.bn.running_mean.clone(), crit.bn.running_var.clone(),
            crit.bn.num_batches_tracked.clone()]


@pytest.mark.parametrize("dtype,mode", [(torch.float32, "train"), (torch.float64, "train"), (torch.float32, "eval"),
                                        (torch.float32, "bn_eval")])
def test_fused_on_cpu_tensors_float64_and_eval_is_the_torch_form_bit_for_bit(dtype, mode):
    r = np.random.default_rng(12)
    z1, z2 = (torch.from_numpy(r.standard_normal((6, 10))).to(dtype) for _ in range(2))
    crits = [pl.BarlowTwinsLoss(10, 6, fused=f).to(dtype) for f in (False, True)]
    assert crits[1].fused and not crits[0].fused
    for c in crits:
        if mode == "eval":
            c.eval()
        elif mode == "bn_eval":
            c.bn.eval()
    for step in range(2):
        want, got = _run(crits[0], z1, z2), _run(crits[1], z1, z2)
        assert all(so.same_bits(a, b) for a, b in zip(got, want)), (mode, step)


def test_trainer_and_cli_surface():
    from cerebralsignalnetworks_amd.trainer import DistillTrainer
    import LstmDistillFromDinoV2Train as train_cli
    assert inspect.signature(pl.BarlowTwinsLoss.__init__).parameters["fused"].default is False
    assert list(inspect.signature(pl.BarlowTwinsLoss.__init__).parameters)[1:4] == ["dim", "batch_size", "lambd"]
    assert "not affected" not in DistillTrainer.__init__.__doc__ and "csn_barlow_corr" in DistillTrainer.__init__.__doc__
    for flavour in (train_cli.PERILS, train_cli.SPAMPINATO):
        text = " ".join(train_cli.build_parser(flavour).format_help().split("--fused_loss")[-1].split("--compat_label_bug")[0].split())
        assert "barlow" in text and "or --loss barlow" not in text

    class _CpuModel(torch.nn.Module):
        def __init__(self):
            super().__init__()
            self.fc = torch.nn.Linear(4, 6)

        def forward(self, x):
            return self.fc(x)

    for fused in (False, True):
        tr = DistillTrainer(_CpuModel(), None, loss="barlow", optimizer="lars", fused_loss=fused, preprocess=False)
        loss = tr.compute_loss(tr.model(torch.randn(5, 4)), torch.randn(5, 6), None, 0)
        assert tr.barlow.fused is fused and bool(torch.isfinite(loss))
    with pytest.raises(ValueError, match="barlow"):
        DistillTrainer(_CpuModel(), None, loss="barlow", optimizer="lars", accum_steps=2, fused_loss=True)
