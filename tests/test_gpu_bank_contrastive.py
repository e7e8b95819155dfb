"""GPU: the fused teacher-bank contrastive loss (csrc/bank_contrastive_loss.hip) -- csn_bank_norms and
csn_bank_contrastive against their float64 numpy restatement (tests/bank_contrastive_reference.py) on the float32 inputs
upcast, canaries around every output, the bit-exact conventions of the header, the stream contract, and the wiring into
BankContrastiveLoss(fused=True), DistillTrainer(loss="contrastive_bank") and the command line.

Tolerances (derived, not tuned).  The kernels compute in float64 and round each float32 output once, so
    rows_out:  |got - ref| <= ref.rows_tol: the roundings of a normalised dot product times the logit scale, and of a log-sum-exp
    loss_part: ref.loss_tol: inv_rows times the sum of those row bounds, plus B + 2 roundings of the sum
    ds:        |got - ref| <= 2^-23 |ref| + c U + 2^-126
with U the gradient formula with absolute values throughout (bank_contrastive_reference.bank_contrastive) and c = 10 x the
measured distance of two float64 evaluation orders of the restatement, 5.2e-13 (bank_contrastive_reference.SPREAD; c <= 1e-9,
so a float32 intermediate, 6e-8, is excluded).  dscale_part is a float64 output: c Uscale.
The fused module against the torch form: 2 x the torch form's own measured distance from the restatement
(bank_contrastive_reference.TORCH_FORM_*), the fused form being within half an ulp of it."""
import numpy as np
import pytest
import torch

import bank_contrastive_reference as ref
import bank_contrastive_stream_cases as stream_cases
import test_gpu_stream_order as stream_tests
from cerebralsignalnetworks_amd import cabi, Model, EEGFilters
from cerebralsignalnetworks_amd import losses as pl
from oracle import eeg_filter

pytestmark = pytest.mark.gpu

PAD = 96                    # canary elements before and behind every output
CANARY = -7.25


def dev(a, cuda):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(cuda)


class Guarded:
    """A dense output inside a larger buffer filled with a canary."""

    def __init__(self, shape, cuda, dtype=torch.float64):
        self.n = int(np.prod(shape))
        self.buf = torch.full((self.n + 2 * PAD,), CANARY, dtype=dtype, device=cuda)
        self.out = self.buf[PAD:PAD + self.n].view(*shape)

    def intact(self):
        return bool((self.buf[:PAD] == CANARY).all()) and bool((self.buf[PAD + self.n:] == CANARY).all())

    def untouched(self):
        return bool((self.buf == CANARY).all())

    def np(self):
        return self.out.double().cpu().numpy()


def scratch_for(cuda, B, M, D):
    w = max(64, 32 * -(-M // 2048))
    nbytes = cabi.load().csn_bank_contrastive_scratch_bytes(B, M, D)
    assert nbytes == 8 * (4 * B + B * M + -(-M // w) * B * D)          # the documented formula
    return Guarded((nbytes // 8,), cuda)


def raw_norms(cuda, bank):
    M, D = bank.shape
    out = Guarded((M,), cuda)
    cabi._check(cabi.load().csn_bank_norms(cabi._ptr(bank), M, D, cabi._ptr(out.out), cabi._stream()))
    return out


def raw(cuda, s, bank, inv, g, pos, scale, inv_rows=None, gs=1.0, want_ds=True, want_dscale=True):
    """csn_bank_contrastive with every output inside a canary buffer -> {"rows", "loss", "scratch"[, "ds"][, "dscale"]}."""
    (B, D), M = s.shape, bank.shape[0]
    out = {"rows": Guarded((2, B), cuda), "loss": Guarded((1,), cuda), "scratch": scratch_for(cuda, B, M, D)}
    if want_ds:
        out["ds"] = Guarded((B, D), cuda, torch.float32)
    if want_dscale:
        out["dscale"] = Guarded((1,), cuda)
    cabi._check(cabi.load().csn_bank_contrastive(
        cabi._ptr(s), B, D, cabi._ptr(bank), cabi._ptr(inv), cabi._ptr(g), M, cabi._ptr(pos), scale,
        1.0 / B if inv_rows is None else inv_rows, gs, cabi._ptr(out["rows"].out), cabi._ptr(out["loss"].out),
        cabi._ptr(out["ds"].out) if want_ds else None, cabi._ptr(out["dscale"].out) if want_dscale else None,
        cabi._ptr(out["scratch"].out), cabi._stream()))
    return out


def same_bits(a, b):
    return torch.equal(a.contiguous().view(torch.uint8), b.contiguous().view(torch.uint8))


def check_case(cuda, c, worst):
    """One case: csn_bank_norms and csn_bank_contrastive against the restatement; the value-only call gives the same bits."""
    B, M, D, a, gs, ir = c["B"], c["M"], c["D"], c["scale"], c["grad_scale"], c["inv_rows"]
    what = f"B{B} M{M} D{D} x{c['input_scale']:g} a{a:g} gs{gs:g} ir{ir} {c['groups']} dscale {c['want_dscale']}"
    s, bank, g, pos = ref.make_inputs(c)
    sd, bd, gd, pd = dev(s, cuda), dev(bank, cuda), dev(g, cuda), dev(pos, cuda)
    inv = raw_norms(cuda, bd)
    inv_ref = ref.bank_norms(bank)
    assert inv.intact() and (np.abs(inv.np() - inv_ref) <= ref.U52 * (D + 4) * inv_ref).all(), (what, "bank_norms")
    want = ref.bank_contrastive(s, bank, inv.np(), g, pos, a, ir, gs)
    got = raw(cuda, sd, bd, inv.out, gd, pd, a, ir, gs, want_dscale=c["want_dscale"])
    assert all(v.intact() for v in got.values()), what
    ir = 1.0 / B if ir is None else ir
    rows = got["rows"].np()
    tol = ref.rows_tol(want["rows"], a, M, D)
    err = np.abs(rows - want["rows"])
    assert np.isfinite(rows).all() and (err <= tol).all(), (what, "rows_out", float((err / tol).max()))
    ltol = ref.loss_tol(want["rows"], a, M, D, ir)
    lerr = abs(got["loss"].np()[0] - want["loss"])
    assert lerr <= ltol, (what, "loss_part", lerr / ltol)
    ds = got["ds"].np()
    ratio = np.abs(ds - want["ds"]) / ref.grad_tol(want["ds"], want["U"])
    assert np.isfinite(ds).all() and ratio.max() <= 1.0, (what, "ds", float(ratio.max()))
    worst["rows"] = max(worst["rows"], float((err / tol).max()))
    worst["loss"] = max(worst["loss"], lerr / ltol)
    worst["ds"] = max(worst["ds"], float(ratio.max()))
    if c["groups"] == "one" or M == 1:      # every query alone with its positive: l == p, loss term 0, a ds row of zeros
        assert torch.equal(got["rows"].out[0], got["rows"].out[1]), what
        assert torch.equal(got["loss"].out, torch.zeros_like(got["loss"].out)), what
        assert torch.equal(got["ds"].out, torch.zeros_like(got["ds"].out)), what
    if c["want_dscale"]:
        tol_a = ref.C_NOISE * want["Uscale"] + ref.U52 * abs(want["dscale"])
        assert abs(got["dscale"].np()[0] - want["dscale"]) <= tol_a, (what, "dscale_part", abs(got["dscale"].np()[0] - want["dscale"]) / tol_a)
    # ds == NULL (validation): the value part alone, the same bits; ds does not depend on whether dscale_part is asked for
    value = raw(cuda, sd, bd, inv.out, gd, pd, a, ir, gs, want_ds=False, want_dscale=False)
    assert set(value) == {"rows", "loss", "scratch"} and all(v.intact() for v in value.values()), what
    assert same_bits(value["rows"].buf, got["rows"].buf) and same_bits(value["loss"].buf, got["loss"].buf), what
    other = raw(cuda, sd, bd, inv.out, gd, pd, a, ir, gs, want_dscale=not c["want_dscale"])
    assert same_bits(other["ds"].buf, got["ds"].buf) and same_bits(other["rows"].buf, got["rows"].buf), what


# ---- 1. values and gradients against the restatement ------------------------------------------------------------------------
@pytest.mark.parametrize("D", ref.D_SET)
def test_bank_contrastive_against_the_restatement(cuda, D):
    worst = {"rows": 0.0, "loss": 0.0, "ds": 0.0}
    cases = ref.gpu_cases(D)
    for c in cases:
        check_case(cuda, c, worst)
    print(f"D {D}: {len(cases)} cases; worst error / tolerance: rows_out {worst['rows']:.3f}, loss_part {worst['loss']:.3f}, "
          f"ds {worst['ds']:.3f}")


@pytest.mark.parametrize("case", ref.EDGE_CASES, ids=lambda c: f"b{c['B']}_m{c['M']}_d{c['D']}")
def test_tile_switch_and_split_width_edges(cuda, case):
    """B 65 with M 4032 / 4096: 126 / 128 of the 64 x 64 logit tiles, the last shape of the 16 x 16 tiles and the first of
    the 64 x 64 ones; M 4097: 96-key splits of the ds contraction instead of 64-key ones, with a ragged last split."""
    worst = {"rows": 0.0, "loss": 0.0, "ds": 0.0}
    check_case(cuda, case, worst)
    print(f"worst error / tolerance {worst}")


def test_256_rows_against_a_bank_of_4096(cuda):
    worst = {"rows": 0.0, "loss": 0.0, "ds": 0.0}
    check_case(cuda, ref.BIG_CASE, worst)
    print(f"B 256 M 4096 D 384: worst error / tolerance {worst}")


def test_bank_norms_with_a_zero_row_and_a_nan_row(cuda):
    r = np.random.default_rng(3)
    for M, D in ((1, 1), (5, 63), (70, 65), (257, 384)):
        bank = r.standard_normal((M, D)).astype(np.float32)
        bank[M // 2] = 0.0
        bank[M - 1, D // 2] = np.nan
        got, want = raw_norms(cuda, dev(bank, cuda)), ref.bank_norms(bank)
        assert got.intact()
        out = got.np()
        assert np.array_equal(np.isnan(out), np.isnan(want)) and np.isnan(out[M - 1])
        if M > 1:
            assert out[M // 2] == 1e12                                  # a zero row: 1 / eps
        ok = ~np.isnan(want)
        assert (np.abs(out[ok] - want[ok]) <= ref.U52 * (D + 4) * want[ok]).all()
        assert torch.equal(cabi.bank_norms(dev(bank, cuda)).view(torch.int64), got.out.view(torch.int64))


# ---- 2. the bit-exact conventions ---------------------------------------------------------------------------------------------
def _problem(cuda, B, M, D, seed, kind="class"):
    c = dict(B=B, M=M, D=D, input_scale=1.0, groups=kind, seed=seed)
    s, bank, g, pos = ref.make_inputs(c)
    return s, bank, g, pos


def _run(cuda, s, bank, g, pos, a=1.0 / 0.07, inv_rows=None, **kw):
    bd = dev(bank, cuda)
    return raw(cuda, dev(s, cuda), bd, cabi.bank_norms(bd), dev(g, cuda), dev(pos, cuda), a, inv_rows, **kw)


@pytest.mark.parametrize("B,M,D", [(65, 150, 70), (37, 513, 384)])
def test_two_calls_give_the_same_bits(cuda, B, M, D):
    s, bank, g, pos = _problem(cuda, B, M, D, 11)
    one, two = _run(cuda, s, bank, g, pos), _run(cuda, s, bank, g, pos)
    for k in ("rows", "loss", "ds", "dscale"):
        assert same_bits(one[k].buf, two[k].buf), k


@pytest.mark.parametrize("M,D", [(150, 70), (4097, 5), (513, 384)])
def test_rows_of_a_micro_batch_are_the_rows_of_the_full_batch(cuda, M, D):
    """Rows 3..7 of a B 65 call against a B 5 call on those rows: l, p and ds bit for bit (a row's results depend on (M, D),
    the scalars and the data alone).  With M 4097 the full batch runs on the 64 x 64 logit tiles and the micro-batch on the
    16 x 16 ones."""
    s, bank, g, pos = _problem(cuda, 65, M, D, 12)
    full = _run(cuda, s, bank, g, pos, inv_rows=1.0 / 65)
    part = _run(cuda, s[3:8], bank, g, pos[3:8], inv_rows=1.0 / 65)
    assert torch.equal(part["rows"].out, full["rows"].out[:, 3:8])
    assert torch.equal(part["ds"].out, full["ds"].out[3:8])


@pytest.mark.parametrize("B,M,D", [(5, 65, 63), (65, 257, 64), (64, 513, 5)])
def test_both_logit_tiles_give_the_same_bits(cuda, monkeypatch, B, M, D):
    """CSN_BANK_TILE (a diagnostic switch read per call) forces the 16 x 16 or the 64 x 64 logit tiles on any shape."""
    s, bank, g, pos = _problem(cuda, B, M, D, 13)
    monkeypatch.setenv("CSN_BANK_TILE", "16")
    small = _run(cuda, s, bank, g, pos)
    monkeypatch.setenv("CSN_BANK_TILE", "64")
    wide = _run(cuda, s, bank, g, pos)
    assert all(v.intact() for v in small.values()) and all(v.intact() for v in wide.values())
    for k in ("rows", "loss", "ds", "dscale"):
        assert same_bits(small[k].buf, wide[k].buf), k


def test_a_query_alone_with_its_positive_is_exactly_zero(cuda):
    """M = 1, and a bank where every other key is left out: l == p bit for bit, loss term 0, a ds row of exact zeros."""
    for B, M, D in ((5, 1, 63), (65, 1, 384), (5, 257, 65), (64, 65, 5)):
        s, bank, g, pos = _problem(cuda, B, M, D, 14, "one")
        out = _run(cuda, s, bank, g, pos, a=100.0, gs=3.0)
        assert torch.equal(out["rows"].out[0], out["rows"].out[1])
        assert torch.equal(out["loss"].out, torch.zeros(1, dtype=torch.float64, device=cuda))
        assert torch.equal(out["ds"].out, torch.zeros(B, D, device=cuda))
        assert torch.equal(out["dscale"].out, torch.zeros(1, dtype=torch.float64, device=cuda))


def test_nan_in_a_masked_key_changes_no_bit(cuda):
    B, M, D = 37, 150, 70
    s, bank, _, _ = _problem(cuda, B, M, D, 16, "none")
    r = np.random.default_rng(16)
    g = r.integers(1, 30, size=M).astype(np.int32)
    g[:8] = 0                                               # rows 0..7 are group 0; every positive is one of rows 0..6
    pos = r.integers(0, 7, size=B).astype(np.int32)
    clean = _run(cuda, s, bank, g, pos)
    dirty_bank = bank.copy()
    dirty_bank[7, 5] = np.nan                               # key 7 is left out of every query
    dirty = _run(cuda, s, dirty_bank, g, pos)
    torch.cuda.synchronize()
    assert all(v.intact() for v in dirty.values())
    for k in ("rows", "loss", "ds", "dscale"):
        assert torch.equal(clean[k].out, dirty[k].out) and same_bits(clean[k].buf, dirty[k].buf), k


def test_nan_in_an_allowed_key_and_a_bad_pos_make_that_row_nan_and_no_other(cuda):
    B, M, D = 37, 150, 70
    s, bank, _, _ = _problem(cuda, B, M, D, 17, "none")
    r = np.random.default_rng(17)
    g = r.integers(1, 30, size=M).astype(np.int32)
    g[:8] = 0
    pos = r.integers(0, 7, size=B).astype(np.int32)
    clean = _run(cuda, s, bank, g, pos)
    others = torch.tensor([i for i in range(B) if i != 11], device=cuda)
    # (i) key 7 carries a NaN; query 11 alone (its positive moved to group g[20] != 0) may see it
    pos_a = pos.copy()
    pos_a[11] = 20
    clean_a = _run(cuda, s, bank, g, pos_a)
    dirty_bank = bank.copy()
    dirty_bank[7, 5] = np.nan
    got = _run(cuda, s, dirty_bank, g, pos_a)
    torch.cuda.synchronize()
    assert all(v.intact() for v in got.values())
    assert bool(torch.isnan(got["rows"].out[0, 11])) and bool(torch.isnan(got["ds"].out[11]).all()) and bool(torch.isnan(got["loss"].out).all())
    assert torch.isfinite(clean_a["ds"].out[11]).all()
    assert torch.equal(got["rows"].out[:, others], clean_a["rows"].out[:, others]) and torch.equal(got["ds"].out[others], clean_a["ds"].out[others])
    # (ii) a bad query row of the student: that row alone
    s_bad = s.copy()
    s_bad[11, 3] = np.nan
    got = _run(cuda, s_bad, bank, g, pos)
    assert bool(torch.isnan(got["rows"].out[:, 11]).all()) and bool(torch.isnan(got["ds"].out[11]).all())
    assert torch.equal(got["rows"].out[:, others], clean["rows"].out[:, others]) and torch.equal(got["ds"].out[others], clean["ds"].out[others])
    # (iii) a pos outside [0, M): a NaN l, p and ds row, nothing indexed, no other row touched
    for bad in (-1, M, 2 ** 31 - 1, -2 ** 31):
        pos_b = pos.copy()
        pos_b[11] = bad
        got = _run(cuda, s, bank, g, pos_b)
        torch.cuda.synchronize()
        assert all(v.intact() for v in got.values()), bad
        assert bool(torch.isnan(got["rows"].out[:, 11]).all()) and bool(torch.isnan(got["ds"].out[11]).all()), bad
        assert bool(torch.isnan(got["loss"].out).all()) and bool(torch.isnan(got["dscale"].out).all()), bad
        assert torch.equal(got["rows"].out[:, others], clean["rows"].out[:, others]), bad
        assert torch.equal(got["ds"].out[others], clean["ds"].out[others]), bad


def test_optional_pointers_and_refusals_on_device_buffers(cuda):
    """bank_group, ds and dscale_part may be NULL; a refused call launches nothing (the refusals themselves are listed in
    tests/test_bank_contrastive_cpu.py, which needs no device)."""
    lib = cabi.load()
    s, bank, g, pos = _problem(cuda, 4, 12, 5, 18)
    sd, bd, gd, pd = dev(s, cuda), dev(bank, cuda), dev(g, cuda), dev(pos, cuda)
    inv = cabi.bank_norms(bd)
    rows, loss, ds, dscale, scratch = (Guarded((2, 4), cuda), Guarded((1,), cuda), Guarded((4, 5), cuda, torch.float32),
                                       Guarded((1,), cuda), scratch_for(cuda, 4, 12, 5))
    p, st = cabi._ptr, cabi._stream()

    def call(**kw):
        v = dict(B=4, a=2.0, g=p(gd), ds=p(ds.out), dscale=p(dscale.out), pos=p(pd))
        v.update(kw)
        return lib.csn_bank_contrastive(p(sd), v["B"], 5, p(bd), p(inv), v["g"], 12, v["pos"], v["a"], 0.25, 1.0, p(rows.out),
                                        p(loss.out), v["ds"], v["dscale"], p(scratch.out), st)
    for kw in (dict(B=0), dict(a=float("nan")), dict(a=-1.0), dict(pos=None)):
        assert call(**kw) == 1 and "csn_bank_contrastive" in lib.csn_last_error().decode(), kw
    torch.cuda.synchronize()
    assert all(v.untouched() for v in (rows, loss, ds, dscale, scratch))
    assert call(g=None, ds=None, dscale=None) == 0
    torch.cuda.synchronize()
    assert rows.intact() and not rows.untouched() and ds.untouched() and dscale.untouched()
    assert call() == 0
    torch.cuda.synchronize()
    assert ds.intact() and not ds.untouched() and not dscale.untouched()


# ---- 3. the module -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B,M,D,temperature,kind", [(16, 40, 33, 0.07, "class"), (65, 257, 384, 0.07, "none"), (16, 2000, 384, 0.01, "class")])
def test_fused_module_against_the_restatement_and_the_torch_form(cuda, B, M, D, temperature, kind):
    c = dict(B=B, M=M, D=D, input_scale=2.0, groups=kind, seed=B + D)
    s, bank, g, pos = ref.make_inputs(c)
    a = 1.0 / temperature
    bd, pd = dev(bank, cuda), dev(pos, cuda).long()         # any integer dtype is taken
    gd = None if g is None else dev(g, cuda)
    fused, plain = pl.BankContrastiveLoss(temperature, fused=True), pl.BankContrastiveLoss(temperature)
    fused.set_bank(bd, gd)
    plain.set_bank(bd, gd)
    x = dev(s, cuda).requires_grad_(True)
    loss = fused(x, pd)
    assert loss.dim() == 0 and loss.dtype == torch.float32
    (0.5 * loss).backward()              # an upstream factor: the saved gradient times 0.5 (exact in float32)
    want = ref.bank_contrastive(s, bank, ref.bank_norms(bank), g, pos, a)
    assert abs(loss.item() - want["loss"]) <= ref.U23 * abs(want["loss"]) + ref.loss_tol(want["rows"], a, M, D, 1.0 / B)
    ratio = np.abs(x.grad.double().cpu().numpy() - 0.5 * want["ds"]) / ref.grad_tol(0.5 * want["ds"], 0.5 * want["U"])
    assert ratio.max() <= 1.0, float(ratio.max())
    x2 = dev(s, cuda).requires_grad_(True)
    loss2 = plain(x2, pd)
    (0.5 * loss2).backward()
    d_loss = abs(loss2.item() - loss.item()) / ref.loss_scale(want["rows"])
    d_grad = float((x2.grad - x.grad).abs().max()) / float(0.5 * want["U"].max())
    print(f"B{B} M{M} D{D} T{temperature}: fused {loss.item()!r} torch form {loss2.item()!r} restatement {want['loss']!r}; fused "
          f"gradient error / tolerance {ratio.max():.3f}; torch form - fused: loss {d_loss:.2e} (bound {2 * ref.TORCH_FORM_LOSS:.1e}), "
          f"gradient {d_grad:.2e} (bound {2 * ref.TORCH_FORM_GRAD:.1e})")
    assert d_loss <= 2 * ref.TORCH_FORM_LOSS and d_grad <= 2 * ref.TORCH_FORM_GRAD
    with torch.no_grad():                # validation: the value part alone gives the same loss
        assert fused(x, pd).item() == loss.item()
    # a strided student is made contiguous
    wide = dev(np.concatenate([s, s], axis=1), cuda)
    assert fused(wide[:, :D], pd).item() == loss.item()


def test_fused_module_with_a_learnable_temperature(cuda):
    c = dict(B=37, M=50, D=20, input_scale=1.0, groups="class", seed=4)
    s, bank, g, pos = ref.make_inputs(c)
    crit = pl.BankContrastiveLoss(temperature=0.1, learnable_temperature=True, fused=True).to(cuda)
    crit.set_bank(dev(bank, cuda), dev(g, cuda))
    a = crit.scale()[0]
    x = dev(s, cuda).requires_grad_(True)
    crit(x, dev(pos, cuda)).backward()
    want = ref.bank_contrastive(s, bank, ref.bank_norms(bank), g, pos, a)
    assert abs(crit.log_scale.grad.item() - a * want["dscale"]) <= ref.U23 * abs(a * want["dscale"]) + a * ref.C_NOISE * want["Uscale"]


# ---- 4. the trainer ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("accum_steps", [1, 2])
def test_trainer_step_fused_against_the_torch_form(cuda, accum_steps):
    """One step of two DistillTrainer(loss="contrastive_bank") at B 8, C 16, T 24, H 32, L 1, D 48 against a bank of 40 rows
    with RMSprop from the same parameters, with and without fused_loss: every parameter tensor agrees within
    2 x ref.TRAINER_STEP of its largest element -- the distance the float32 torch form itself shows on the CPU at this shape
    from the float64 restatement (measured 1.133e-06; tests/test_bank_contrastive_cpu.py::trainer_step_distance), doubled."""
    from cerebralsignalnetworks_amd.trainer import DistillTrainer
    B, C, T, H, L, D, M = 8, 16, 24, 32, 1, 48, 40
    r = np.random.default_rng(72)
    x = dev(eeg_filter.synthetic_eeg(B, C, T, seed=71), cuda)
    bank = dev(r.standard_normal((M, D)).astype(np.float32), cuda)
    group = dev(r.integers(0, 10, size=M).astype(np.int32), cuda)
    pos = dev(r.integers(0, M, size=B).astype(np.int32), cuda)
    tgt = bank[pos.long()]
    filt = EEGFilters(1000, order=3)
    torch.manual_seed(73)
    models = [Model(input_size=C, lstm_size=H, lstm_layers=L, output_size=D, include_top=False, compute_dtype=torch.float32)
              for _ in range(2)]
    models[1].load_state_dict(models[0].state_dict())
    before = {n: p.detach().clone().cpu().numpy() for n, p in models[0].named_parameters()}
    trainers = [DistillTrainer(m.to(cuda), filt.sos, loss="contrastive_bank", optimizer="rmsprop", fused_loss=f, accum_steps=accum_steps)
                for m, f in zip(models, (True, False))]
    for tr in trainers:
        tr.set_bank(bank, group)
    assert trainers[0].contrastive_bank.fused and not trainers[1].contrastive_bank.fused
    losses = [tr.train_step(x, tgt, positives=pos) for tr in trainers]
    for tr in trainers:
        tr.check_device_status()
    print(f"contrastive_bank step, accum_steps {accum_steps}: fused {losses[0].item()!r} torch form {losses[1].item()!r}")
    # the loss: 2 x the torch form's measured distance, in units of the loss with absolute values, |l| + |p| <= 2 a + log M
    assert abs(losses[0].item() - losses[1].item()) <= 2 * ref.TORCH_FORM_LOSS * (2.0 / 0.07 + np.log(M))
    moved = 0
    for (n, p), (_, q) in zip(models[0].named_parameters(), models[1].named_parameters()):
        p, q = p.detach().cpu().numpy(), q.detach().cpu().numpy()
        err, bound = float(np.abs(p - q).max()), 2 * ref.TRAINER_STEP * float(np.abs(q).max())
        print(f"{n}: max |fused - torch form| {err:.3e} bound {bound:.3e}; moved by {float(np.abs(p - before[n]).max()):.3e}")
        assert err <= bound, (n, err, bound)
        moved += int(not np.array_equal(p, before[n]))
    assert moved > 0


# ---- 5. the stream contract of the two entry points ---------------------------------------------------------------------------------
@pytest.mark.parametrize("case", [c for v in stream_cases.CASES.values() for c in v], ids=lambda c: c.id)
def test_stream_order(cuda, case):
    """The procedure of tests/test_gpu_stream_order.py on the cases of tests/bank_contrastive_stream_cases.py."""
    stream_tests.test_stateless_entry_point_with_late_inputs(cuda, case)


# ---- 6. the command line --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("extra", [("--accum_steps", "2"), ("--contrastive_mask", "class", "--num_epochs", "2", "--validation_frequency", "1")],
                         ids=["micro_batches", "class_mask_validation"])
def test_command_line_trains_with_the_fused_bank_loss(cuda, tmp_path, capsys, monkeypatch, extra):
    import LstmDistillFromDinoV2Train as train
    seen, inner = [], cabi.bank_contrastive

    def spy(*args, **kw):
        seen.append((args[0].shape[0], args[1].shape[0], kw.get("bank_group", args[5] if len(args) > 5 else None) is not None,
                     kw["want_grad"]))
        return inner(*args, **kw)
    monkeypatch.setattr(cabi, "bank_contrastive", spy)
    hist = train.main(["--synthetic", "64", "--batch_size", "16", "--num_epochs", "1", "--hidden_size", "32", "--loss", "contrastive_bank",
                       "--fused_loss", "--log_dir", str(tmp_path), *extra])
    printed = capsys.readouterr().out
    assert np.isfinite(hist).all() and "contrastive_bank: 64 images in the bank" in printed and "EPOCH 0 train_loss:" in printed
    train_calls = [c for c in seen if c[3]]
    assert all(c[1] == 64 for c in seen)                    # every image of the dataset is a key, whatever the batch
    if "--accum_steps" in extra:                            # 52 training rows in batches of 16 and a last one of 4, each as two micro-batches
        assert len(hist) == 1 and [c[0] for c in train_calls] == [8, 8, 8, 8, 8, 8, 2, 2] and not any(c[2] for c in seen)
    else:
        assert len(hist) == 2 and [c[0] for c in train_calls] == [16, 16, 16, 4] * 2 and all(c[2] for c in seen)
        assert "val_loss" in printed and any(not c[3] for c in seen)        # the validation loss went through the same module
