"""GPU: the fused contrastive loss (csrc/contrastive_loss.hip) -- csn_contrastive_lse and
csn_contrastive_grad against their float64 numpy restatement (tests/contrastive_loss_reference.py) on the float32 inputs upcast,
canaries around every output, the same bits twice and on any split into ranks, NaN / Inf, the host refusals, the stream
contract, and the wiring into ContrastiveLoss(fused=True), DistillTrainer(loss="contrastive") and the command line.

Tolerances (derived, not tuned).  The kernels compute in float64 and round each float32 output once, so
    rows_out:  |got - ref| <= ref.rows_tol: the roundings of a normalised dot product times the logit scale, and of a log-sum-exp
    loss_part: the weighted mean of those row bounds over the local rows, plus B roundings of the sum
    module loss (float32): |got - ref| <= 2^-23 |ref|
    ds:        |got - ref| <= 2^-23 |ref| + c U + 2^-126
with U the gradient formula with absolute values throughout (contrastive_loss_reference.contrastive_grad) and c = 10 x the
measured distance of two float64 evaluation orders of the restatement, 3.1e-12 (contrastive_loss_reference.SPREAD; c <= 1e-9,
so a float32 intermediate, 6e-8, is excluded).  dscale_part is a float64 output: c Uscale.
The fused module against the torch form: 2 x the torch form's own measured distance from the restatement
(contrastive_loss_reference.TORCH_FORM_*), the fused form being within half an ulp of it."""
import ctypes

import numpy as np
import pytest
import torch

import contrastive_loss_reference as ref
import contrastive_loss_stream_cases as stream_cases
import test_gpu_stream_order as stream_tests
from cerebralsignalnetworks_amd import cabi, Model, EEGFilters
from cerebralsignalnetworks_amd import losses as pl
from oracle import eeg_filter

pytestmark = pytest.mark.gpu

PAD = 96                    # canary elements before and behind every output
CANARY = -7.25
INVALID = 1                 # CSN_ERR_INVALID_ARGUMENT


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


def scratch_for(cuda, B, N, D):
    lib = cabi.load()
    kt, sp = (N + 63) // 64, (N + 255) // 256
    nbytes = lib.csn_contrastive_scratch_bytes(B, N, D)
    assert nbytes == 8 * (3 * N + 4 * kt * B + B + B * N + sp * B * D)          # the documented formula
    return Guarded((nbytes // 8,), cuda)


def raw_lse(cuda, s, t, g, row0, B, scale, w_a=0.5, w_b=0.5):
    """csn_contrastive_lse with every output inside a canary buffer -> {"rows", "loss", "scratch"}."""
    N, D = s.shape
    out = {"rows": Guarded((3, B), cuda), "loss": Guarded((1,), cuda), "scratch": scratch_for(cuda, B, N, D)}
    cabi._check(cabi.load().csn_contrastive_lse(cabi._ptr(s), cabi._ptr(t), cabi._ptr(g), N, D, row0, B, scale, w_a, w_b,
                                                cabi._ptr(out["rows"].out), cabi._ptr(out["loss"].out),
                                                cabi._ptr(out["scratch"].out), cabi._stream()))
    return out


def raw_grad(cuda, s, t, g, row0, B, scale, lse_a, lse_b_all, gs=1.0, want_dscale=True, w_a=0.5, w_b=0.5):
    N, D = s.shape
    out = {"ds": Guarded((B, D), cuda, torch.float32), "scratch": scratch_for(cuda, B, N, D)}
    if want_dscale:
        out["dscale"] = Guarded((1,), cuda)
    cabi._check(cabi.load().csn_contrastive_grad(cabi._ptr(s), cabi._ptr(t), cabi._ptr(g), N, D, row0, B, scale, cabi._ptr(lse_a),
                                                 cabi._ptr(lse_b_all), w_a, w_b, gs, cabi._ptr(out["ds"].out),
                                                 cabi._ptr(out["dscale"].out) if want_dscale else None,
                                                 cabi._ptr(out["scratch"].out), cabi._stream()))
    return out


def check_case(cuda, c, s, t, g, row0, lse_b_all_dev, worst):
    """One (case, row0): both calls against the restatement; the second call takes lA from the first on the device."""
    B, N, D, a, gs = c["B"], c["N"], c["D"], c["scale"], c["grad_scale"]
    what = f"B{B} N{N} D{D} row0 {row0} x{c['input_scale']:g} a{a:g} gs{gs:g} {c['groups']} dscale {c['want_dscale']}"
    sd, td, gd = dev(s, cuda), dev(t, cuda), dev(g, cuda)
    rows, loss = ref.contrastive_lse(s, t, g, row0, B, a)
    first = raw_lse(cuda, sd, td, gd, row0, B, a)
    assert all(v.intact() for v in first.values()), what
    tol = ref.rows_tol(rows, a, N, D)
    err = np.abs(first["rows"].np() - rows)
    assert np.isfinite(first["rows"].np()).all() and (err <= tol).all(), (what, "rows_out", float((err / tol).max()))
    loss_tol = (0.5 * (tol[0] + tol[2]) + 0.5 * (tol[1] + tol[2])).sum() / N + ref.U52 * (B + 2) * ref.loss_scale(rows) * B / N
    assert abs(first["loss"].np()[0] - loss) <= loss_tol, (what, "loss_part", abs(first["loss"].np()[0] - loss) / loss_tol)
    worst["rows"] = max(worst["rows"], float((err / tol).max()))
    worst["loss"] = max(worst["loss"], abs(first["loss"].np()[0] - loss) / loss_tol)

    lse_b_ref = ref.contrastive_lse(s, t, g, 0, N, a)[0][1] if B < N else rows[1]
    ds, dscale, U, Uscale = ref.contrastive_grad(s, t, g, row0, B, a, rows[0], lse_b_ref, grad_scale=gs)
    lse_a_dev = first["rows"].out[0]
    second = raw_grad(cuda, sd, td, gd, row0, B, a, lse_a_dev, lse_b_all_dev, gs=gs, want_dscale=c["want_dscale"])
    assert all(v.intact() for v in second.values()), what
    got = second["ds"].np()
    ratio = np.abs(got - ds) / ref.grad_tol(ds, U)
    assert np.isfinite(got).all() and ratio.max() <= 1.0, (what, "ds", float(ratio.max()))
    worst["ds"] = max(worst["ds"], float(ratio.max()))
    if c["groups"] == "masked_row":         # every query alone with its positive: loss term 0, a zero gradient
        assert first["loss"].np()[0] == 0.0 and not got.any(), what
        assert torch.equal(first["rows"].out[0], first["rows"].out[2]) and torch.equal(first["rows"].out[1], first["rows"].out[2])
    if c["want_dscale"]:
        tol_a = ref.C_NOISE * Uscale + ref.U52 * abs(dscale)
        assert abs(second["dscale"].np()[0] - dscale) <= tol_a, (what, "dscale_part", abs(second["dscale"].np()[0] - dscale) / tol_a)
        if row0 == 0:                       # ds does not depend on whether dscale_part is asked for
            plain = raw_grad(cuda, sd, td, gd, row0, B, a, lse_a_dev, lse_b_all_dev, gs=gs, want_dscale=False)
            assert set(plain) == {"ds", "scratch"} and torch.equal(plain["ds"].buf.view(torch.int32), second["ds"].buf.view(torch.int32))


# ---- 1. values and gradients against the restatement ------------------------------------------------------------------------
@pytest.mark.parametrize("D", ref.D_SET)
def test_contrastive_loss_against_the_restatement(cuda, D):
    worst, n = {"rows": 0.0, "loss": 0.0, "ds": 0.0}, 0
    for c in ref.gpu_cases(D):
        s, t, g = ref.make_inputs(c)
        N = c["N"]
        whole = raw_lse(cuda, dev(s, cuda), dev(t, cuda), dev(g, cuda), 0, N, c["scale"])         # lB of all rows, on the device
        for row0 in c["row0s"]:
            check_case(cuda, c, s, t, g, row0, whole["rows"].out[1], worst)
            n += 1
    print(f"D {D}: {n} (case, row0) pairs; worst error / tolerance: rows_out {worst['rows']:.3f}, loss_part {worst['loss']:.3f}, "
          f"ds {worst['ds']:.3f}")


def test_256_local_rows_against_2048_gathered_keys(cuda):
    c = ref.BIG_CASE
    s, t, g = ref.make_inputs(c)
    whole = raw_lse(cuda, dev(s, cuda), dev(t, cuda), dev(g, cuda), 0, c["N"], c["scale"])
    worst = {"rows": 0.0, "loss": 0.0, "ds": 0.0}
    check_case(cuda, c, s, t, g, c["row0"], whole["rows"].out[1], worst)
    print(f"B 256 N 2048 D 384 row0 768: worst error / tolerance {worst}")


# ---- 2. the same bits twice, and on any split into ranks ------------------------------------------------------------------------
def _both_calls(cuda, sd, td, gd, row0, B, a, lse_b_all=None, gs=1.0):
    first = raw_lse(cuda, sd, td, gd, row0, B, a)
    lse_b_all = first["rows"].out[1] if lse_b_all is None else lse_b_all
    second = raw_grad(cuda, sd, td, gd, row0, B, a, first["rows"].out[0], lse_b_all, gs=gs)
    return {"rows": first["rows"], "loss": first["loss"], "ds": second["ds"], "dscale": second["dscale"]}


@pytest.mark.parametrize("N,D", [(198, 70), (522, 384)])
def test_same_bits_on_two_calls_and_on_any_split_into_ranks(cuda, N, D):
    """N rows as one call and as 2 and 3 emulated ranks: rows_out and ds are the same bits (a row's results depend on (N, D)
    and the data alone, not on B or row0), and a repeated call repeats every output."""
    c = dict(N=N, D=D, input_scale=1.0, groups="sparse", seed=N + D)
    s, t, g = ref.make_inputs(c)
    sd, td, gd = dev(s, cuda), dev(t, cuda), dev(g, cuda)
    a = 1.0 / 0.07
    one, again = _both_calls(cuda, sd, td, gd, 0, N, a), _both_calls(cuda, sd, td, gd, 0, N, a)
    for k in one:
        assert torch.equal(one[k].buf.view(torch.uint8), again[k].buf.view(torch.uint8)), k
    for world in (2, 3):
        B = N // world
        assert B * world == N
        parts = [_both_calls(cuda, sd, td, gd, r * B, B, a, lse_b_all=one["rows"].out[1]) for r in range(world)]
        assert torch.equal(torch.cat([p["rows"].out for p in parts], dim=1), one["rows"].out), world
        assert torch.equal(torch.cat([p["ds"].out for p in parts], dim=0), one["ds"].out), world
        total = sum(p["loss"].np()[0] for p in parts)
        assert abs(total - one["loss"].np()[0]) <= ref.U52 * 4 * ref.loss_scale(one["rows"].np())


# ---- 3. NaN and Inf ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("bad", [float("nan"), float("inf"), float("-inf")])
def test_nan_and_inf_inputs_propagate_and_nothing_faults(cuda, bad):
    c = dict(N=70, D=33, input_scale=1.0, groups="none", seed=17)
    s, t, _ = ref.make_inputs(c)
    N, a = c["N"], 1.0 / 0.07
    g = np.arange(N, dtype=np.int32)
    g[3] = g[7]                                   # key 7 is left out of query 3 (and key 3 of query 7)
    # (i) a bad QUERY row of the student
    s1 = s.copy()
    s1[5, 11] = bad
    out = _both_calls(cuda, dev(s1, cuda), dev(t, cuda), dev(g, cuda), 0, N, a)
    torch.cuda.synchronize()
    assert all(v.intact() for v in out.values())
    rows = out["rows"].np()
    assert np.isnan(rows[:, 5]).all() and np.isnan(out["loss"].np()[0])
    assert np.isfinite(np.delete(rows[0], 5)).all() and np.isfinite(np.delete(rows[2], 5)).all()       # the other rows' lA and p
    assert np.isnan(rows[1]).all()                # as a KEY of the image queries it contaminates every lB, as in torch
    want = pl._contrastive_lse_torch(torch.from_numpy(s1).double(), torch.from_numpy(t).double(), torch.from_numpy(g), 0, N, a,
                                     0.5, 0.5)[0].numpy()
    assert np.array_equal(np.isnan(rows), np.isnan(want))
    # (ii) a bad KEY row of the teacher: every lA but the query's that leaves it out
    t1 = t.copy()
    t1[7, 2] = bad
    out = _both_calls(cuda, dev(s, cuda), dev(t1, cuda), dev(g, cuda), 0, N, a)
    torch.cuda.synchronize()
    assert all(v.intact() for v in out.values())
    rows = out["rows"].np()
    want = pl._contrastive_lse_torch(torch.from_numpy(s).double(), torch.from_numpy(t1).double(), torch.from_numpy(g), 0, N, a,
                                     0.5, 0.5)[0].numpy()
    assert np.array_equal(np.isnan(rows), np.isnan(want))
    assert np.isfinite(rows[0, 3]) and np.isnan(np.delete(rows[0], 3)).all()
    assert np.isnan(rows[1, 7]) and np.isfinite(np.delete(rows[1], 7)).all()


# ---- 4. the host refusals ---------------------------------------------------------------------------------------------------------------
def test_host_refusals_launch_nothing(cuda):
    lib = cabi.load()
    N, D, row0, B, a = 12, 5, 4, 4, 2.0
    c = dict(N=N, D=D, input_scale=1.0, groups="sparse", seed=3)
    s, t, g = (dev(x, cuda) for x in ref.make_inputs(c))
    rows, loss, ds, dscale = Guarded((3, B), cuda), Guarded((1,), cuda), Guarded((B, D), cuda, torch.float32), Guarded((1,), cuda)
    scratch = scratch_for(cuda, B, N, D)
    lse = torch.zeros(N, dtype=torch.float64, device=cuda)
    p, st = cabi._ptr, cabi._stream()
    nan, inf = float("nan"), float("inf")

    def lse_call(**kw):
        v = dict(s=p(s), t=p(t), g=p(g), N=N, D=D, row0=row0, B=B, a=a, wa=0.5, wb=0.5, rows=p(rows.out), loss=p(loss.out),
                 scratch=p(scratch.out))
        v.update(kw)
        return lib.csn_contrastive_lse(v["s"], v["t"], v["g"], v["N"], v["D"], v["row0"], v["B"], v["a"], v["wa"], v["wb"], v["rows"],
                                       v["loss"], v["scratch"], st)

    def grad_call(**kw):
        v = dict(s=p(s), t=p(t), g=p(g), N=N, D=D, row0=row0, B=B, a=a, la=p(lse[:B]), lb=p(lse), wa=0.5, wb=0.5, gs=1.0,
                 ds=p(ds.out), dscale=p(dscale.out), scratch=p(scratch.out))
        v.update(kw)
        return lib.csn_contrastive_grad(v["s"], v["t"], v["g"], v["N"], v["D"], v["row0"], v["B"], v["a"], v["la"], v["lb"], v["wa"],
                                        v["wb"], v["gs"], v["ds"], v["dscale"], v["scratch"], st)

    odd = ctypes.c_void_p(scratch.out.data_ptr() + 4)
    shared = [dict(s=None), dict(t=None), dict(scratch=None), dict(N=0), dict(D=0), dict(B=0), dict(N=-1), dict(row0=-1),
              dict(row0=N - B + 1), dict(B=N + 1, row0=0), dict(a=0.0), dict(a=-1.0), dict(a=nan), dict(a=inf), dict(wa=nan),
              dict(wb=inf), dict(scratch=odd)]
    for kw in shared + [dict(rows=None), dict(loss=None), dict(rows=ctypes.c_void_p(rows.out.data_ptr() + 4))]:
        assert lse_call(**kw) == INVALID, kw
        assert "csn_contrastive_lse" in lib.csn_last_error().decode()
    for kw in shared + [dict(la=None), dict(lb=None), dict(ds=None), dict(lb=ctypes.c_void_p(lse.data_ptr() + 4)),
                        dict(dscale=ctypes.c_void_p(dscale.out.data_ptr() + 4))]:
        assert grad_call(**kw) == INVALID, kw
        assert "csn_contrastive_grad" in lib.csn_last_error().decode()
    torch.cuda.synchronize()
    assert all(v.untouched() for v in (rows, loss, ds, dscale, scratch))        # nothing was launched
    assert lib.csn_contrastive_scratch_bytes(0, N, D) == 0 and lib.csn_contrastive_scratch_bytes(B, N, 0) == 0
    assert lib.csn_contrastive_scratch_bytes(N + 1, N, D) == 0
    # the optional pointers may be NULL, and then the calls go through
    assert lse_call(g=None) == 0 and grad_call(g=None, dscale=None) == 0
    torch.cuda.synchronize()
    assert rows.intact() and not rows.untouched() and dscale.untouched()


# ---- 5. the module -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B,D,temperature,kind", [(16, 33, 0.07, "sparse"), (65, 384, 0.07, "none"), (256, 384, 0.01, "sparse")])
def test_fused_module_against_the_restatement_and_the_torch_form(cuda, B, D, temperature, kind):
    c = dict(N=B, D=D, input_scale=2.0, groups=kind, seed=B + D)
    s, t, g = ref.make_inputs(c)
    if temperature < 0.05:
        # make_inputs correlates t_i with s_i; at logit scale 100 every matched pair then saturates its softmax and the loss
        # (2e-10) is the rounding of lA - p, below the restatement's own evaluation-order error: no value to hold a float32
        # loss to.  The teacher rows in another order leave a loss of ordinary size.
        t = np.ascontiguousarray(t[np.random.default_rng(B).permutation(B)])
    a = 1.0 / temperature
    gd = None if g is None else dev(g, cuda).long()          # any integer dtype is taken
    fused, plain = pl.ContrastiveLoss(temperature, fused=True), pl.ContrastiveLoss(temperature)
    x = dev(s, cuda).requires_grad_(True)
    loss = fused(x, dev(t, cuda), gd)
    assert loss.dim() == 0 and loss.dtype == torch.float32
    (0.5 * loss).backward()              # an upstream factor: the saved gradient times 0.5 (exact in float32)
    rows, want = ref.contrastive_lse(s, t, g, 0, B, a)
    ds, _, U, _ = ref.contrastive_grad(s, t, g, 0, B, a, rows[0], rows[1])
    assert abs(loss.item() - want) <= ref.loss_tol(want), ("module loss", loss.item(), want)
    ratio = np.abs(x.grad.double().cpu().numpy() - 0.5 * ds) / ref.grad_tol(0.5 * ds, 0.5 * U)
    assert ratio.max() <= 1.0, float(ratio.max())
    x2 = dev(s, cuda).requires_grad_(True)
    loss2 = plain(x2, dev(t, cuda), gd)
    (0.5 * loss2).backward()
    d_loss = abs(loss2.item() - loss.item()) / ref.loss_scale(rows)
    d_grad = float((x2.grad - x.grad).abs().max()) / float(0.5 * U.max())
    print(f"B{B} D{D} T{temperature}: fused {loss.item()!r} torch form {loss2.item()!r} restatement {want!r}; fused gradient error / "
          f"tolerance {ratio.max():.3f}; torch form - fused: loss {d_loss:.2e} (bound {2 * ref.TORCH_FORM_LOSS:.1e}), gradient "
          f"{d_grad:.2e} (bound {2 * ref.TORCH_FORM_GRAD:.1e})")
    assert d_loss <= 2 * ref.TORCH_FORM_LOSS and d_grad <= 2 * ref.TORCH_FORM_GRAD
    # strided inputs are made contiguous; a teacher that asks for a gradient gets none
    wide = dev(np.concatenate([s, t], axis=1), cuda)
    tt = wide[:, D:].clone().requires_grad_(True)
    again = fused(wide[:, :D].clone().requires_grad_(True), tt, gd)
    again.backward()
    assert again.item() == loss.item() and tt.grad is None
    assert fused(wide[:, :D], wide[:, D:], gd).item() == loss.item()


def test_fused_module_with_a_learnable_temperature(cuda):
    c = dict(N=37, D=20, input_scale=1.0, groups="sparse", seed=4)
    s, t, g = ref.make_inputs(c)
    crit = pl.ContrastiveLoss(temperature=0.1, learnable_temperature=True, fused=True).to(cuda)
    a = crit.scale()[0]
    x = dev(s, cuda).requires_grad_(True)
    crit(x, dev(t, cuda), dev(g, cuda)).backward()
    rows, _ = ref.contrastive_lse(s, t, g, 0, 37, a)
    _, dscale, _, Uscale = ref.contrastive_grad(s, t, g, 0, 37, a, rows[0], rows[1])
    want = a * dscale
    assert abs(crit.log_scale.grad.item() - want) <= ref.U23 * abs(want) + a * ref.C_NOISE * Uscale


def test_module_on_two_ranks_gathers_rows_and_lse(cuda, monkeypatch):
    """The module's multi-rank plumbing without a second process: the world size is patched to 2 and the collectives hand over
    the other rank's rows (and its lB, computed by csn_contrastive_lse on that rank's rows).  Each rank returns the global
    loss and world x its rows of the global gradient."""
    c = dict(N=74, D=33, input_scale=1.0, groups="sparse", seed=6)
    s, t, g = ref.make_inputs(c)
    N, B, a = 74, 37, 1.0 / 0.07
    rows, _ = ref.contrastive_lse(s, t, g, 0, N, a)
    want = ref.contrastive_lse(s, t, g, 0, N, a)[1]
    ds, _, U, _ = ref.contrastive_grad(s, t, g, 0, N, a, rows[0], rows[1], grad_scale=2.0)
    sd, td, gd = dev(s, cuda), dev(t, cuda), dev(g, cuda)
    whole_rows, whole_loss = cabi.contrastive_lse(sd, td, a, gd)
    halves = [slice(0, B), slice(B, N)]

    calls = []

    def all_gather(parts, x):
        """In the module's order: the row counts, student, teacher, groups, lB."""
        if x.dtype == torch.int64:
            src = [x, x]                        # the other rank brings the same number of rows
        else:
            nth = sum(1 for d in calls if d == x.dtype)
            everything = {torch.float32: (sd, td)[min(nth, 1)], torch.int32: gd, torch.float64: whole_rows[1]}[x.dtype]
            assert torch.equal(x, everything[halves[rank]])         # lB of the local rows: the bits of the one-rank call
            src = [everything[h] for h in halves]
        calls.append(x.dtype)
        for r in range(2):
            parts[r].copy_(src[r])

    def all_reduce(x):
        assert x.dtype == torch.float64 and x.shape == (1,)
        x.copy_(whole_loss)

    monkeypatch.setattr(pl, "_dist_world", lambda: 2)
    monkeypatch.setattr(torch.distributed, "all_gather", all_gather)
    monkeypatch.setattr(torch.distributed, "all_reduce", all_reduce)
    for rank in range(2):
        calls.clear()
        monkeypatch.setattr(torch.distributed, "get_rank", lambda: rank)
        x = sd[halves[rank]].clone().requires_grad_(True)
        loss = pl.ContrastiveLoss(fused=True)(x, td[halves[rank]], gd[halves[rank]])
        loss.backward()
        assert calls == [torch.int64, torch.float32, torch.float32, torch.int32, torch.float64]
        assert abs(loss.item() - want) <= ref.loss_tol(want)
        ratio = np.abs(x.grad.double().cpu().numpy() - ds[halves[rank]]) / ref.grad_tol(ds[halves[rank]], U[halves[rank]])
        assert ratio.max() <= 1.0, (rank, float(ratio.max()))


# ---- 6. the trainer ---------------------------------------------------------------------------------------------------------------------------
def test_trainer_step_fused_against_the_torch_form(cuda):
    """One step of two DistillTrainer(loss="contrastive") at B 8, C 16, T 24, H 32, L 1, D 48 with RMSprop from the same
    parameters, with and without fused_loss: every parameter tensor agrees within relative 1e-4 of its largest element, the
    bound tests/test_gpu_barlow_loss.py holds the same comparison to."""
    from cerebralsignalnetworks_amd.trainer import DistillTrainer
    B, C, T, H, L, D = 8, 16, 24, 32, 1, 48
    x = dev(eeg_filter.synthetic_eeg(B, C, T, seed=71), cuda)
    tgt = dev(np.random.default_rng(72).standard_normal((B, D)).astype(np.float32), cuda)
    groups = torch.tensor([0, 1, 2, 0, 4, 5, 6, 1], device=cuda)
    filt = EEGFilters(1000, order=3)
    torch.manual_seed(73)
    models = [Model(input_size=C, lstm_size=H, lstm_layers=L, output_size=D, include_top=False, compute_dtype=torch.float32)
              for _ in range(2)]
    models[1].load_state_dict(models[0].state_dict())
    before = {n: p.detach().clone().cpu().numpy() for n, p in models[0].named_parameters()}
    trainers = [DistillTrainer(m.to(cuda), filt.sos, loss="contrastive", optimizer="rmsprop", fused_loss=f)
                for m, f in zip(models, (True, False))]
    assert trainers[0].contrastive.fused and not trainers[1].contrastive.fused
    losses = [tr.train_step(x, tgt, groups=groups) for tr in trainers]
    for tr in trainers:
        tr.check_device_status()
    print(f"contrastive step: fused {losses[0].item()!r} torch form {losses[1].item()!r}")
    assert abs(losses[0].item() - losses[1].item()) <= 1e-4 * abs(losses[1].item())
    moved = 0
    for (n, p), (_, q) in zip(models[0].named_parameters(), models[1].named_parameters()):
        p, q = p.detach().cpu().numpy(), q.detach().cpu().numpy()
        err, bound = float(np.abs(p - q).max()), 1e-4 * float(np.abs(q).max())
        print(f"{n}: max |fused - torch form| {err:.3e} bound {bound:.3e}; moved by {float(np.abs(p - before[n]).max()):.3e}")
        assert err <= bound, (n, err, bound)
        moved += int(not np.array_equal(p, before[n]))
    assert moved > 0


# ---- 7. the stream contract of the two entry points ---------------------------------------------------------------------------------
@pytest.mark.parametrize("case", [c for v in stream_cases.CASES.values() for c in v], ids=lambda c: c.id)
def test_stream_order(cuda, case):
    """The procedure of tests/test_gpu_stream_order.py on the cases of tests/contrastive_loss_stream_cases.py."""
    stream_tests.test_stateless_entry_point_with_late_inputs(cuda, case)


# ---- 8. the command line --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("extra", [(), ("--contrastive_mask", "class", "--normalize_embeddings", "--num_epochs", "2",
                                         "--validation_frequency", "1")], ids=["image_mask", "class_mask_retrieval"])
def test_command_line_trains_with_the_fused_contrastive_loss(cuda, tmp_path, capsys, monkeypatch, extra):
    import LstmDistillFromDinoV2Train as train
    seen, inner = [], cabi.contrastive_grad

    def spy(*args, **kw):
        seen.append(kw.get("group_all", args[5] if len(args) > 5 else None) is not None)
        return inner(*args, **kw)
    monkeypatch.setattr(cabi, "contrastive_grad", spy)
    hist = train.main(["--synthetic", "64", "--batch_size", "16", "--num_epochs", "1", "--hidden_size", "32", "--loss", "contrastive",
                       "--fused_loss", "--log_dir", str(tmp_path), *extra])
    printed = capsys.readouterr().out
    assert len(hist) == (2 if extra else 1) and np.isfinite(hist).all()
    assert "EPOCH 0 train_loss:" in printed
    assert len(seen) == 4 * len(hist) and all(seen)         # 51 training rows in batches of 16: the HIP calls, with group ids
    if extra:
        assert "Overall Recall" in printed and "val_loss" in printed        # the retrieval leg ran, on normalised embeddings
