"""CPU: the teacher-bank contrastive loss -- the float64 numpy restatement of csn_bank_norms and
csn_bank_contrastive (tests/bank_contrastive_reference.py) against float64 autograd of the plain formula, the torch form of
losses.BankContrastiveLoss, its tie to ContrastiveLoss, micro-batches through the trainer, EEGDataset.image_bank, the header
and the binding with the host-side refusals, and the measured constants the GPU tests read."""
import ctypes
import itertools
import os
import re

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import bank_contrastive_reference as ref
import bank_contrastive_stream_cases  # noqa: F401  (joins the stream-order case table on import)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REL = 1e-12
INVALID = 1                 # CSN_ERR_INVALID_ARGUMENT


def plain_formula(s, bank, group, pos, a):
    """The loss in torch ops, as a user would write it (any float dtype; autograd through everything): the mean."""
    z = a * (F.normalize(s, dim=1, eps=1e-12) @ F.normalize(bank, dim=1, eps=1e-12).T)
    if group is not None:
        out = (group[None, :] == group[pos][:, None]) & (torch.arange(bank.shape[0])[None, :] != pos[:, None])
        z = z.masked_fill(out, float("-inf"))
    return F.cross_entropy(z, pos)


def autograd_of_plain(s, bank, group, pos, a):
    s64 = torch.tensor(np.asarray(s, np.float64), requires_grad=True)
    a64 = torch.tensor(float(a), dtype=torch.float64, requires_grad=True)
    g = None if group is None else torch.from_numpy(np.asarray(group))
    loss = plain_formula(s64, torch.tensor(np.asarray(bank, np.float64)), g, torch.from_numpy(np.asarray(pos)).long(), a64)
    ds, da = torch.autograd.grad(loss, (s64, a64))
    return loss.item(), ds.numpy(), da.item()


def close(got, want, what, rel=REL, scale=None):
    """Within ``rel`` of the largest element -- of ``scale`` where given: the same formula with absolute values throughout,
    the natural size of a gradient that cancels (with D = 1 the projection leaves exactly 0 of it)."""
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    scale = max(float(np.abs(want if scale is None else scale).max()), 1e-300)
    err = float(np.abs(got - want).max())
    assert err <= rel * scale, (what, err / scale)
    return err / scale


def restated(s, bank, group, pos, a, **kw):
    return ref.bank_contrastive(s, bank, ref.bank_norms(bank), group, pos, a, **kw)


def check_against_autograd(s, bank, group, pos, a, what):
    loss, ds, da = autograd_of_plain(s, bank, group, pos, a)
    got = restated(s, bank, group, pos, a)
    assert abs(got["loss"] - loss) <= REL * max(ref.loss_scale(got["rows"]), 1e-300), (what, got["loss"], loss)
    return got, max(close(got["ds"], ds, what + " ds", scale=got["U"]), close(got["dscale"], da, what + " dscale", scale=got["Uscale"]))


# ---- 1. the restatement against float64 autograd ----------------------------------------------------------------------------
@pytest.mark.parametrize("M,D", list(itertools.product((1, 2, 5, 12), (1, 7))))
def test_restatement_against_float64_autograd(M, D):
    r = np.random.default_rng(10 * M + D)
    worst = 0.0
    for a, grouped, B in itertools.product((1.0, 1.0 / 0.07, 1e4), (False, True), (3, 9)):
        s, bank = r.standard_normal((B, D)), r.standard_normal((M, D))
        pos = r.integers(0, M, size=B)                      # B 9 against M <= 5: repeated positives
        group = r.integers(0, max(M // 2, 1), size=M).astype(np.int32) if grouped else None
        what = f"B{B} M{M} D{D} a{a:g} groups{grouped}"
        got, w = check_against_autograd(s, bank, group, pos, a, what)
        worst = max(worst, w)
        if M == 1:          # the positive is the only key: l == p bit for bit, nothing to learn
            assert got["loss"] == 0.0 and not got["ds"].any() and got["dscale"] == 0.0, what
            assert np.array_equal(got["rows"][0], got["rows"][1]), what
    print(f"M{M} D{D}: worst relative distance from autograd {worst:.2e}")


def test_special_rows_against_float64_autograd():
    """A query whose every other key is left out (loss term 0, zero gradient), a zero row (no projection, divided by eps), a
    row with 0 < |s| < 1e-12 (likewise), repeated positives, inv_rows and grad_scale other than 1 / B and 1."""
    r = np.random.default_rng(5)
    B, M, D, a = 9, 11, 7, 1.0 / 0.07
    s, bank = r.standard_normal((B, D)), r.standard_normal((M, D))
    s[2] = 0.0
    s[4] = 1e-14 * r.standard_normal(D)
    assert 0.0 < np.linalg.norm(s[4]) < 1e-12
    pos = np.array([0, 3, 3, 5, 10, 0, 7, 3, 9])
    group = np.array([3, 3, 5, 3, 6, 7, 3, -2 ** 31, 2 ** 31 - 1, 8, 8], np.int32)
    alone = np.full(M, 11, np.int32)            # one group: every query's only key is its positive
    for g in (group, alone, None):
        got, _ = check_against_autograd(s, bank, g, pos, a, "special")
        if g is alone:
            assert np.array_equal(got["rows"][0], got["rows"][1]) and not got["ds"].any() and got["loss"] == 0.0
    # the tiny and the zero row are divided by eps, not by their norm, and are not projected
    got = restated(s, bank, None, pos, a)
    assert np.abs(got["ds"][2]).max() > 1e9 and np.abs(got["ds"][4]).max() > 1e9
    # inv_rows and grad_scale are plain factors; a micro-batch of the rows gives the rows of the full batch
    full = restated(s, bank, group, pos, a, inv_rows=1.0 / B, grad_scale=2.0)
    part = restated(s[3:7], bank, group, pos[3:7], a, inv_rows=1.0 / B, grad_scale=2.0)
    assert np.array_equal(part["rows"], full["rows"][:, 3:7]) and np.array_equal(part["ds"], full["ds"][3:7])
    close(full["ds"], 2.0 * restated(s, bank, group, pos, a)["ds"], "grad_scale", 1e-15)


def test_conventions_of_the_restatement():
    """A NaN in a masked key changes no bit; a NaN in an allowed key and a pos outside [0, M) make that row NaN and no other."""
    r = np.random.default_rng(6)
    B, M, D, a = 6, 10, 5, 1.0 / 0.07
    s, bank = r.standard_normal((B, D)), r.standard_normal((M, D)).astype(np.float32)
    group = np.array([0, 0, 0, 1, 1, 2, 3, 4, 5, 6], np.int32)
    pos = np.array([0, 1, 0, 1, 0, 1])                       # every query's positive is in group 0: key 2 is left out of all
    clean = restated(s, bank, group, pos, a)
    dirty_bank = bank.copy()
    dirty_bank[2, 3] = np.nan
    dirty = restated(s, dirty_bank, group, pos, a)
    assert np.isnan(ref.bank_norms(dirty_bank)[2])
    for k in ("rows", "ds"):
        assert np.array_equal(clean[k], dirty[k]), k
    assert clean["loss"] == dirty["loss"] and clean["dscale"] == dirty["dscale"]
    pos2 = np.array([0, 1, 0, 4, 0, 1])                      # query 3 (group 1) sees key 2
    clean, dirty = restated(s, bank, group, pos2, a), restated(s, dirty_bank, group, pos2, a)
    others = np.arange(B) != 3
    assert np.isnan(dirty["rows"][0, 3]) and np.isnan(dirty["ds"][3]).all() and np.isnan(dirty["loss"])
    assert np.array_equal(clean["rows"][:, others], dirty["rows"][:, others]) and np.array_equal(clean["ds"][others], dirty["ds"][others])
    for bad in (-1, M, 2 ** 31 - 1):
        pos3 = pos2.copy()
        pos3[4] = bad
        got = restated(s, bank, group, pos3, a)
        others = np.arange(B) != 4
        assert np.isnan(got["rows"][:, 4]).all() and np.isnan(got["ds"][4]).all() and np.isnan(got["loss"])
        assert np.array_equal(clean["rows"][:, others], got["rows"][:, others]) and np.array_equal(clean["ds"][others], got["ds"][others])


# ---- 2. the torch form of the module -------------------------------------------------------------------------------------------
def test_torch_form_module_matches_the_restatement_in_float64():
    from cerebralsignalnetworks_amd.losses import BankContrastiveLoss
    r = np.random.default_rng(7)
    B, M, D = 9, 12, 7
    s, bank = r.standard_normal((B, D)), r.standard_normal((M, D))
    pos = r.integers(0, M, size=B)
    group = np.array([0, 1, 2, 0, 4, 5, 1, 7, 8, 0, 10, 5], np.int32)
    for temperature, g, kw in ((0.07, None, {}), (0.07, group, {}), (1.0, group, {}), (1e-4, group, dict(max_scale=1e4))):
        crit = BankContrastiveLoss(temperature=temperature, **kw)
        a = crit.scale()[0]
        assert a == min(1.0 / temperature, kw.get("max_scale", 100.0)) and not crit.fused
        crit.set_bank(torch.tensor(bank), None if g is None else torch.from_numpy(g).long())        # any integer dtype is taken
        x = torch.tensor(s, requires_grad=True)
        loss = crit(x, torch.from_numpy(pos))
        assert loss.dim() == 0 and loss.dtype == torch.float64
        (2.0 * loss).backward()
        want = restated(s, bank, g, pos, a)
        close(loss.item(), want["loss"], "loss", scale=ref.loss_scale(want["rows"]))
        close(x.grad.numpy(), 2.0 * want["ds"], "ds", scale=2.0 * want["U"])
        with torch.no_grad():               # evaluation: the same value
            again = crit(x, torch.from_numpy(pos).int())
        assert again.item() == loss.item() and not again.requires_grad
    with pytest.raises(ValueError, match="set_bank"):
        BankContrastiveLoss()(torch.zeros(4, 3), torch.zeros(4, dtype=torch.int64))
    with pytest.raises(ValueError, match="temperature"):
        BankContrastiveLoss(temperature=0.0)
    crit = BankContrastiveLoss()
    with pytest.raises(ValueError, match="bank_group"):
        crit.set_bank(torch.zeros(5, 3), torch.zeros(4, dtype=torch.int64))
    crit.set_bank(torch.ones(5, 3))
    with pytest.raises(ValueError, match="pos"):
        crit(torch.zeros(4, 3), torch.zeros(5, dtype=torch.int64))
    with pytest.raises(ValueError, match="student"):
        crit(torch.zeros(4, 2), torch.zeros(4, dtype=torch.int64))


def test_set_bank_computes_the_norms_once_per_tensor_and_version():
    from cerebralsignalnetworks_amd.losses import BankContrastiveLoss
    bank = torch.tensor([[3.0, 4.0], [0.0, 0.0], [float("nan"), 1.0]])
    crit = BankContrastiveLoss()
    crit.set_bank(bank)
    inv = crit.bank_inv_norm()
    assert inv.dtype == torch.float64 and inv[0] == 0.2 and inv[1] == 1e12 and torch.isnan(inv[2])
    assert np.array_equal(inv.numpy(), ref.bank_norms(bank.numpy()), equal_nan=True)
    assert crit.bank_inv_norm() is inv                       # the same tensor, the same version: nothing is computed
    bank[0, 0] = 6.0                                         # an in-place write bumps _version
    again = crit.bank_inv_norm()
    assert again is not inv and again[0] == 1.0 / np.sqrt(52.0)
    crit.set_bank(bank[:2].clone())
    assert crit.bank_inv_norm().shape == (2,)


def test_learnable_temperature_gradient_matches_autograd():
    from cerebralsignalnetworks_amd.losses import BankContrastiveLoss
    r = np.random.default_rng(8)
    B, M, D = 10, 7, 5
    s, bank = torch.tensor(r.standard_normal((B, D))), torch.tensor(r.standard_normal((M, D)))
    pos, group = torch.from_numpy(r.integers(0, M, size=B)), torch.from_numpy(r.integers(0, 4, size=M))
    crit = BankContrastiveLoss(temperature=0.2, learnable_temperature=True).double()
    crit.set_bank(bank, group)
    assert isinstance(crit.log_scale, torch.nn.Parameter) and abs(crit.scale()[0] - 5.0) < 1e-6
    x = s.clone().requires_grad_(True)
    crit(x, pos).backward()
    want = restated(s.numpy(), bank.numpy(), group.numpy(), pos.numpy(), crit.scale()[0])
    close(crit.log_scale.grad.item(), crit.scale()[0] * want["dscale"], "d loss / d log_scale = a dscale_part",
          scale=crit.scale()[0] * want["Uscale"])
    close(x.grad.numpy(), want["ds"], "ds", scale=want["U"])
    # above the clamp the scale is max_scale and log_scale gets a zero gradient; a fixed temperature is no parameter
    crit = BankContrastiveLoss(temperature=0.001, learnable_temperature=True, max_scale=50.0).double()
    crit.set_bank(bank, group)
    crit(s.clone().requires_grad_(True), pos).backward()
    assert crit.scale() == (50.0, False) and crit.log_scale.grad.item() == 0.0
    assert list(BankContrastiveLoss().parameters()) == []


def test_tie_to_the_in_batch_loss():
    """With the bank = the batch's teacher rows and pos = arange(B), the loss and gradient are those of
    ContrastiveLoss(w_s2t=1, w_t2s=0): the in-batch student-to-teacher direction."""
    from cerebralsignalnetworks_amd.losses import BankContrastiveLoss, ContrastiveLoss
    r = np.random.default_rng(9)
    B, D = 11, 6
    s, t = torch.tensor(r.standard_normal((B, D))), torch.tensor(r.standard_normal((B, D)))
    groups = torch.tensor([0, 1, 2, 0, 4, 5, 1, 7, 8, 0, 10])
    for g in (None, groups):
        x1, x2 = s.clone().requires_grad_(True), s.clone().requires_grad_(True)
        crit = BankContrastiveLoss()
        crit.set_bank(t, g)
        l1 = crit(x1, torch.arange(B))
        l2 = ContrastiveLoss(w_s2t=1.0, w_t2s=0.0)(x2, t, g)
        l1.backward()
        l2.backward()
        close(l1.item(), l2.item(), "loss")
        close(x1.grad.numpy(), x2.grad.numpy(), "ds")


# ---- 3. the trainer, the dataset and the command line ----------------------------------------------------------------------------
class _CpuModel(torch.nn.Module):
    def __init__(self):
        super().__init__()
        self.fc = torch.nn.Linear(4, 3)

    def forward(self, x):
        return self.fc(x[:, -1])


@pytest.mark.parametrize("k", [2, 3])
def test_micro_batches_through_the_trainer_give_the_full_batch_gradients(k):
    from cerebralsignalnetworks_amd.trainer import DistillTrainer
    from cerebralsignalnetworks_amd.losses import BankContrastiveLoss
    r = np.random.default_rng(k)
    B, M = 12, 9
    x = torch.tensor(r.standard_normal((B, 4, 5)), dtype=torch.float32)          # [B,C,T]
    bank = torch.tensor(r.standard_normal((M, 3)), dtype=torch.float32)
    group = torch.tensor([0, 0, 1, 1, 2, 3, 4, 4, 5])
    pos = torch.from_numpy(r.integers(0, M, size=B))
    tgt = torch.zeros(B, 3)                                                      # not read by this loss
    grads, losses = [], []
    for steps in (1, k):
        torch.manual_seed(3)
        tr = DistillTrainer(_CpuModel(), None, loss="contrastive_bank", optimizer="adam", accum_steps=steps,
                            contrastive_temperature=0.2, preprocess=False)
        assert isinstance(tr.contrastive_bank, BankContrastiveLoss) and tr.contrastive_bank.scale() == (5.0, False)
        assert not tr.contrastive_bank.fused and tr.contrastive is None
        tr.set_bank(bank, group)
        if steps == 1:
            want = tr.contrastive_bank(tr.model(tr.embed(x)), pos).item()
        losses.append(tr.train_step(x, tgt, positives=pos).item())
        grads.append(tr.grads.flat.clone())
    assert losses[0] == want
    # float32 rounding of the sum: each of the k partial gradients is rounded, and so is each of the k - 1 additions
    scale = float(grads[0].abs().max())
    assert float((grads[0] - grads[1]).abs().max()) <= 2 * k * ref.U23 * scale, (grads[0], grads[1])
    assert abs(losses[0] - losses[1]) <= 2 * k * ref.U23 * abs(losses[0])
    with pytest.raises(ValueError, match="positives"):
        tr.train_step(x, tgt)
    with pytest.raises(ValueError, match="contrastive_bank"):
        DistillTrainer(_CpuModel(), None, loss="cosine", optimizer="adam").set_bank(bank)
    # the in-batch loss keeps its refusal
    with pytest.raises(ValueError, match="contrastive is a batch-level loss"):
        DistillTrainer(_CpuModel(), None, loss="contrastive", optimizer="adam", accum_steps=2)


def test_image_bank_of_a_dataset_with_repeated_images():
    from cerebralsignalnetworks_amd.dataset import EEGDataset
    cpu = torch.device("cpu")
    d = EEGDataset(synthetic=8, synthetic_channels=4, synthetic_samples=20, time_low=0, time_high=20, feature_dim=3, device=cpu)
    bank, pos_all, bank_class = d.image_bank()                  # synthetic: every sample its own image
    assert torch.equal(bank, d.features_all) and torch.equal(pos_all, torch.arange(8, dtype=torch.int32))
    assert torch.equal(bank_class, d.labels.to(torch.int32)) and bank.dtype == torch.float32 and pos_all.dtype == torch.int32
    # several samples (subjects) per image, ids neither sorted nor dense
    ids = torch.tensor([40, 7, 40, 19, 7, 7, 3, 19])
    d.image_ids_dev = ids
    feats = torch.arange(24, dtype=torch.float32).reshape(8, 3)
    for i in range(8):
        feats[i] = feats[int((ids == ids[i]).nonzero()[0])]     # an image's samples carry the image's row
    d.set_features(feats.numpy())
    d.labels_dev = torch.tensor([5, 1, 5, 2, 1, 1, 0, 2])
    bank, pos_all, bank_class = d.image_bank()
    assert torch.equal(bank, feats[[6, 1, 3, 0]])               # images 3, 7, 19, 40: the row of the first sample of each
    assert torch.equal(pos_all, torch.tensor([3, 1, 3, 2, 1, 1, 0, 2], dtype=torch.int32))
    assert torch.equal(bank_class, torch.tensor([0, 1, 2, 5], dtype=torch.int32))
    assert torch.equal(bank[pos_all.long()], d.features_all)
    feats[4, 1] += 1.0                                          # sample 4 shows image 7 with another row
    d.set_features(feats.numpy())
    with pytest.raises(ValueError, match="sample 4 and sample 1 show image 7"):
        d.image_bank()
    d.image_features_extracted, d.features_all = False, None
    with pytest.raises(ValueError, match="no teacher features"):
        d.image_bank()


def test_cli_parsers_accept_the_loss():
    import LstmDistillFromDinoV2Train as train
    for flavour in (train.PERILS, train.SPAMPINATO):
        p = train.build_parser(flavour)
        f = p.parse_args(["--loss", "contrastive_bank", "--contrastive_temperature", "0.05", "--contrastive_mask", "class",
                          "--fused_loss", "--accum_steps", "4"])
        assert (f.loss, f.contrastive_temperature, f.contrastive_mask, f.fused_loss, f.accum_steps) == \
            ("contrastive_bank", 0.05, "class", True, 4)
        assert p.parse_args([]).loss == flavour.loss


# ---- 4. the header and the binding -----------------------------------------------------------------------------------------------
NEW_SYMBOLS = ("csn_bank_norms", "csn_bank_contrastive_scratch_bytes", "csn_bank_contrastive")


def test_header_names_the_new_symbols_and_keeps_the_abi():
    from cerebralsignalnetworks_amd import cabi
    with open(os.path.join(ROOT, "include", "csn_hip.h")) as f:
        text = f.read()
    assert re.search(r"#define CSN_ABI_VERSION 6\b", text) and cabi.ABI_VERSION == 6
    added = re.search(r"A symbol added beside the existing ones(.*?)breaks no caller", text, flags=re.S).group(1)
    assert "csn_bank_norms" in added and "csn_bank_contrastive and its _scratch_bytes" in added
    lib = cabi.load()
    assert lib.csn_abi_version() == 6
    for name in NEW_SYMBOLS:
        assert name in cabi.SIGNATURES and hasattr(lib, name) and re.search(rf"\b{name}\(", text), name
    assert "ceil(M / w) B D" in text and "max(64, 32 ceil(M / 2048))" in text        # the scratch formula is in the header
    for B, M, D in ((1, 1, 1), (16, 2000, 384), (256, 4097, 5), (256, 65536, 384)):
        w = max(64, 32 * -(-M // 2048))
        assert lib.csn_bank_contrastive_scratch_bytes(B, M, D) == 8 * (4 * B + B * M + -(-M // w) * B * D)
    for bad in ((0, 5, 5), (5, 0, 5), (5, 5, 0), (-1, 5, 5), (65535 * 16 + 1, 5, 5)):
        assert lib.csn_bank_contrastive_scratch_bytes(*bad) == 0


def test_host_refusals_return_invalid_argument_with_a_message():
    """Every refusal is decided on the host before any launch, so it can be provoked without a device: the pointers are
    host buffers that are never dereferenced."""
    from cerebralsignalnetworks_amd import cabi
    lib = cabi.load()
    buf = (ctypes.c_double * 64)()
    ok = ctypes.c_void_p(ctypes.addressof(buf))
    odd = ctypes.c_void_p(ctypes.addressof(buf) + 4)
    nan, inf = float("nan"), float("inf")

    def norms(**kw):
        v = dict(bank=ok, M=3, D=4, inv=ok)
        v.update(kw)
        return lib.csn_bank_norms(v["bank"], v["M"], v["D"], v["inv"], None)

    def loss(**kw):
        v = dict(s=ok, B=2, D=4, bank=ok, inv=ok, group=ok, M=3, pos=ok, a=2.0, ir=0.5, gs=1.0, rows=ok, loss=ok, ds=ok, dscale=ok,
                 scratch=ok)
        v.update(kw)
        return lib.csn_bank_contrastive(v["s"], v["B"], v["D"], v["bank"], v["inv"], v["group"], v["M"], v["pos"], v["a"], v["ir"],
                                        v["gs"], v["rows"], v["loss"], v["ds"], v["dscale"], v["scratch"], None)

    for kw in (dict(bank=None), dict(inv=None), dict(M=0), dict(D=0), dict(M=-2), dict(inv=odd)):
        assert norms(**kw) == INVALID, kw
        assert "csn_bank_norms" in lib.csn_last_error().decode()
    for kw in (dict(s=None), dict(bank=None), dict(inv=None), dict(pos=None), dict(rows=None), dict(loss=None), dict(scratch=None),
               dict(B=0), dict(M=0), dict(D=0), dict(B=-1), dict(B=65535 * 16 + 1), dict(a=0.0), dict(a=-1.0), dict(a=nan), dict(a=inf),
               dict(ir=nan), dict(ir=inf), dict(gs=nan), dict(gs=-inf), dict(inv=odd), dict(rows=odd), dict(loss=odd),
               dict(dscale=odd), dict(scratch=odd)):
        assert loss(**kw) == INVALID, kw
        assert "csn_bank_contrastive" in lib.csn_last_error().decode()
    # the Python binding refuses host tensors and wrong types before it reaches the library
    with pytest.raises(cabi.CsnError):
        cabi.bank_norms(torch.zeros(3, 4))
    with pytest.raises(cabi.CsnError):
        cabi.bank_contrastive(torch.zeros(2, 4), torch.zeros(3, 4), torch.zeros(3, dtype=torch.float64), torch.zeros(2, dtype=torch.int32), 2.0)


# ---- 5. the measured constants the GPU tests read -------------------------------------------------------------------------------------
def _all_cases():
    return [c for D in ref.D_SET for c in ref.gpu_cases(D)] + ref.EDGE_CASES + [ref.BIG_CASE]


def test_gpu_cases_cover_every_setting():
    cases = [c for D in ref.D_SET for c in ref.gpu_cases(D)]
    seen = {(c["input_scale"], c["scale"], c["grad_scale"], c["inv_rows"], c["groups"], c["want_dscale"]) for c in cases}
    assert len(cases) == 144 and len(seen) == 3 * 4 * 2 * 3 * 2
    for axis, values in (("B", ref.B_SET), ("M", ref.M_SET), ("D", ref.D_SET)):
        count = {v: sum(1 for c in cases if c[axis] == v) for v in values}
        assert min(count.values()) >= 2 and sum(count.values()) == len(cases), (axis, count)
    pairs = {(c["B"], c["M"]) for c in cases}
    assert set(ref.CORNERS) <= pairs                       # the edge values of two axes together
    assert {(c["B"], c["D"]) for c in cases} == set(itertools.product(ref.B_SET, ref.D_SET))


def trainer_step_distance(accum_steps):
    """Measured constant (c): one RMSprop step (the trainer's lr 1e-3 with torch's alpha 0.99 and eps 1e-8, from a zero
    state) of the GPU trainer test's model through the float64 oracle LSTM, with the loss gradient of the
    float32 torch form against the float64 restatement's -> the worst max |p - p_ref| / max |p_ref| over the tensors."""
    from cerebralsignalnetworks_amd.losses import BankContrastiveLoss
    from oracle import eeg_filter, lstm
    B, C, T, H, L, D, M = 8, 16, 24, 32, 1, 48, 40
    r = np.random.default_rng(73)
    k = 1.0 / np.sqrt(H)
    params = {"lstm.weight_ih_l0": r.uniform(-k, k, (4 * H, C)), "lstm.weight_hh_l0": r.uniform(-k, k, (4 * H, H)),
              "lstm.bias_ih_l0": r.uniform(-k, k, 4 * H), "lstm.bias_hh_l0": r.uniform(-k, k, 4 * H),
              "fc.weight": r.uniform(-k, k, (D, H)), "fc.bias": r.uniform(-k, k, D)}
    params = {n: v.astype(np.float32) for n, v in params.items()}
    x = eeg_filter.synthetic_eeg(B, C, T, seed=71).transpose(0, 2, 1)           # [B,T,C]
    x = (x - x.mean(axis=1, keepdims=True)) / x.std(axis=1, keepdims=True)
    bank = r.standard_normal((M, D)).astype(np.float32)
    pos = r.integers(0, M, size=B)
    group = r.integers(0, 10, size=M).astype(np.int32)
    feat, saved = lstm.model_forward(x, params, L, return_saved=True)
    feat32 = feat.astype(np.float32)
    crit = BankContrastiveLoss()
    crit.set_bank(torch.from_numpy(bank), torch.from_numpy(group))
    mb = B // accum_steps
    ds32 = np.zeros((B, D), np.float32)
    for j in range(accum_steps):                        # as DistillTrainer._micro_batches: each mean / k
        rows = slice(j * mb, (j + 1) * mb)
        xs = torch.from_numpy(feat32[rows]).requires_grad_(True)
        (crit(xs, torch.from_numpy(pos[rows])) / accum_steps).backward()
        ds32[rows] = xs.grad.numpy()
    ds64 = ref.bank_contrastive(feat32, bank, ref.bank_norms(bank), group, pos, crit.scale()[0])["ds"]
    worst = 0.0
    stepped = []
    for dfeat in (ds32, ds64):
        _, grads = lstm.model_backward(dfeat, params, saved, L)
        stepped.append({n: params[n] - 1e-3 * grads[n] / (np.sqrt(0.01 * grads[n] ** 2) + 1e-8) for n in params})
    for n in params:
        worst = max(worst, float(np.abs(stepped[0][n] - stepped[1][n]).max() / np.abs(stepped[1][n]).max()))
    return worst


def test_measured_constants_hold():
    """(a) SPREAD: two float64 evaluation orders of the restatement, in units of U, over the cases of the GPU test.
    (b) TORCH_FORM_*: the float32 torch form against the restatement over the same cases at logit scales <= 100, the loss in
    units of ref.loss_scale and the gradient in units of the largest U (a gradient that cancels to nothing, as with D = 1 or
    with every other key left out, has no size of its own).
    (c) TRAINER_STEP: trainer_step_distance above.
    All are measured again here.  The sums run through the host's BLAS, whose blocking and thread count decide the order of
    a float64 or float32 sum, so a measurement on another machine is another sample of the same quantity: it is held to
    twice the recorded value (c = 10 x SPREAD keeps a factor of 5 over such a sample), and c <= 1e-9 is held as it stands."""
    from cerebralsignalnetworks_amd.losses import BankContrastiveLoss
    spread, b_loss, b_grad = 0.0, 0.0, 0.0
    for c in _all_cases():
        s, bank, g, pos = ref.make_inputs(c)
        a = c["scale"]
        fwd = ref.bank_contrastive(s, bank, ref.bank_norms(bank), g, pos, a, c["inv_rows"], c["grad_scale"])
        rev = ref.bank_contrastive(s, bank, ref.bank_norms(bank, reverse=True), g, pos, a, c["inv_rows"], c["grad_scale"], reverse=True)
        spread = max(spread, float((np.abs(fwd["ds"] - rev["ds"]) / np.maximum(fwd["U"], 1e-300)).max()))
        if a <= 100.0:
            crit = BankContrastiveLoss(temperature=1.0 / a)
            crit.set_bank(torch.from_numpy(bank), None if g is None else torch.from_numpy(g))
            x = torch.from_numpy(s).requires_grad_(True)
            loss = crit(x, torch.from_numpy(pos))
            loss.backward()
            plain = ref.bank_contrastive(s, bank, ref.bank_norms(bank), g, pos, a)         # the module's mean: 1 / B, grad_scale 1
            b_loss = max(b_loss, abs(loss.item() - plain["loss"]) / ref.loss_scale(plain["rows"]))
            b_grad = max(b_grad, float(np.abs(x.grad.numpy() - plain["ds"]).max()) / float(plain["U"].max()))
    step = max(trainer_step_distance(1), trainer_step_distance(2))
    print(f"(a) spread {spread:.3e} (recorded {ref.SPREAD:g}); (b) torch form: loss {b_loss:.3e} (recorded {ref.TORCH_FORM_LOSS:g}), "
          f"gradient {b_grad:.3e} (recorded {ref.TORCH_FORM_GRAD:g}); (c) trainer step {step:.3e} (recorded {ref.TRAINER_STEP:g})")
    assert spread <= 2 * ref.SPREAD and ref.C_NOISE == 10 * ref.SPREAD and ref.C_NOISE <= 1e-9
    assert b_loss <= 2 * ref.TORCH_FORM_LOSS and b_grad <= 2 * ref.TORCH_FORM_GRAD
    assert step <= 2 * ref.TRAINER_STEP
