"""Numpy float64 restatement of csn_bank_norms and csn_bank_contrastive (include/csn_hip.h): the
contrastive loss of normalised student rows against a fixed bank of normalised teacher rows, with the natural bound U on a
gradient element (the gradient formula with absolute values throughout).  ``reverse=True`` runs every sum over its operands
in reversed order: a second float64 evaluation order, whose distance from the first is the measured constant SPREAD below.
Shared by tests/test_bank_contrastive_cpu.py, which holds it against float64 autograd of the plain formula, and
tests/test_gpu_bank_contrastive.py, which holds the kernels against it.  Not a test module."""
import itertools

import numpy as np

U23 = 2.0 ** -23            # one float32 ulp, relative
U52 = 2.0 ** -52
F32_TINY = 2.0 ** -126
EPS = 1e-12                 # F.normalize

# ---- measured constants (tests/test_bank_contrastive_cpu.py::test_measured_constants_hold measures all of them again) -------
# (a) the worst |ds(ascending) - ds(reversed)| / U of two float64 evaluation orders of this restatement over gpu_cases(),
#     EDGE_CASES and BIG_CASE.  The worst cases are the ones at logit scale 1e4, where a logit carries 1e4 times the rounding
#     of its dot product and exp passes that on as a relative error.
SPREAD = 5.2e-14            # measured 5.097e-14
C_NOISE = 10.0 * SPREAD     # the c of the gradient bound: fma contraction and tile order are further float64 orders
assert C_NOISE <= 1e-9      # a float32 intermediate (6e-8) is still excluded
# (b) the distance of the float32 torch form (BankContrastiveLoss on float32 CPU tensors) from this restatement over the same
#     cases at the logit scales a trainer can reach (max_scale = 100): |loss - ref| / loss_scale and, per gradient tensor,
#     max |ds - ref| / max U.
TORCH_FORM_LOSS = 9.1e-8    # measured 9.000e-08
TORCH_FORM_GRAD = 8.9e-7    # measured 8.856e-07
# (c) one RMSprop step of the trainer test's model (B 8, C 16, T 24, H 32, L 1, D 48, a bank of 40 rows) with the loss
#     gradient of the float32 torch form against the same step with the float64 restatement's, per parameter tensor
#     max |p - p_ref| / max |p_ref|, the worst over the tensors and over accum_steps 1 and 2.
TRAINER_STEP = 1.2e-6       # measured 1.133e-06


def grad_tol(ref, U):
    """One rounding to float32 of a float64 result that is another evaluation order of the restatement."""
    return U23 * np.abs(ref) + C_NOISE * U + F32_TINY


def rows_tol(ref, scale, M, D):
    """l and p are float64 outputs.  A normalised row carries a relative error of (D / 2 + 3) roundings, a dot product of
    two of them D more, the logit one more: (2 D + 8) 2^-53 scale |s^| . |t^| <= (2 D + 8) 2^-53 scale.  A log-sum-exp adds M
    roundings of its sum (relative, so absolute in the logarithm) and a few of its own value.  Twice that: both sides round."""
    return U52 * ((2 * D + 8) * scale + M + 8 + 4 * np.abs(ref))


def loss_tol(rows, scale, M, D, inv_rows):
    """loss_part = inv_rows sum_i (l_i - p_i): the rows' bounds, and B + 2 roundings of the sum and the product."""
    B = rows.shape[1]
    return abs(inv_rows) * (rows_tol(rows, scale, M, D).sum() + U52 * (B + 2) * np.abs(rows).sum())


def loss_scale(rows):
    """The mean loss with absolute values throughout: mean_i (|l_i| + |p_i|)."""
    return float(np.abs(rows).sum(0).mean())


def _sum(x, axis, reverse):
    return np.flip(x, axis).sum(axis) if reverse else x.sum(axis)


def _mm(a, b, reverse):
    """a [M,K] @ b [K,N], the summed index in reversed order if asked."""
    return a[:, ::-1] @ b[::-1, :] if reverse else a @ b


def bank_norms(bank, reverse=False):
    """-> 1 / max(|t_m|, eps) [M] float64; a NaN norm stays NaN."""
    x = np.asarray(bank, np.float64)
    nrm = np.sqrt(_sum(x * x, 1, reverse))
    return 1.0 / np.where(nrm < EPS, EPS, nrm)


def left_out(bank_group, pos, M):
    """[B,M] bool: key m is left out of query i (pos: valid indices)."""
    if bank_group is None:
        return np.zeros((len(pos), M), bool)
    g = np.asarray(bank_group)
    return (g[None, :] == g[pos][:, None]) & (np.arange(M)[None, :] != np.asarray(pos)[:, None])


def bank_contrastive(s, bank, inv_norm, bank_group, pos, scale, inv_rows=None, grad_scale=1.0, reverse=False):
    """-> dict(rows [2,B] = l, p; loss; ds [B,D] holding grad_scale; dscale; U [B,D]; Uscale).  A row whose pos is outside
    [0, M) has NaN l, p and ds (and makes loss and dscale NaN); no other row sees it."""
    s = np.asarray(s, np.float64)
    B, M = s.shape[0], np.asarray(bank).shape[0]
    inv_rows = 1.0 / B if inv_rows is None else inv_rows
    pos = np.asarray(pos, np.int64)
    valid = (pos >= 0) & (pos < M)
    pc = np.where(valid, pos, 0)
    nrm = np.sqrt(_sum(s * s, 1, reverse))
    den = np.where(nrm < EPS, EPS, nrm)
    sh = s / den[:, None]
    with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
        th = np.asarray(bank, np.float64) * np.asarray(inv_norm, np.float64)[:, None]
        # the contraction of the weights with t^ takes a non-finite t^ as 0: a query that may see such a key has NaN weights
        # throughout (NaN x 0 is NaN), a query that leaves it out takes exactly nothing from it
        thc = np.where(np.isfinite(th), th, 0.0)
        out = left_out(bank_group, pc, M)
        d = _mm(sh, th.T, reverse)                      # s^_i . t^_m
        z = scale * d
        zm = np.where(out, -np.inf, z)
        mx = np.nanmax(np.where(np.isnan(zm), -np.inf, zm), axis=1)
        e = np.where(out, 0.0, np.exp(z - mx[:, None]))
        l = np.where(valid, mx + np.log(_sum(e, 1, reverse)), np.nan)
        p = np.where(valid, z[np.arange(B), pc], np.nan)
        loss = inv_rows * _sum(l - p, 0, reverse)
        P = np.where(out, 0.0, np.exp(z - l[:, None]))
        g = (scale * inv_rows) * (_mm(P, thc, reverse) - th[pc])
        gabs = abs(scale * inv_rows) * (np.where(np.isfinite(P), P, 0.0) @ np.abs(thc) + np.abs(thc[pc]))
        proj = (nrm > EPS)[:, None]
        dot = _sum(sh * g, 1, reverse)[:, None]
        ds = grad_scale * (g - np.where(proj, sh * dot, 0.0)) / den[:, None]
        ds = np.where(valid[:, None], ds, np.nan)
        U = abs(grad_scale) * (gabs + np.where(proj, np.abs(sh) * (np.abs(sh) * gabs).sum(1)[:, None], 0.0)) / den[:, None]
        dpos = d[np.arange(B), pc]
        sa = _sum(np.where(out, 0.0, P * d), 1, reverse)
        dscale = inv_rows * _sum(np.where(valid, sa - dpos, np.nan), 0, reverse)
        Uscale = abs(inv_rows) * float(np.nansum(np.where(out, 0.0, P * np.abs(d)).sum(1) + np.abs(dpos)))
    return dict(rows=np.stack([l, p]), loss=loss, ds=ds, dscale=dscale, U=U, Uscale=Uscale)


# ---- the cases of the GPU accuracy test, and of the measured constants ---------------------------------------------------------
# The kernels' edges: 16- and 64-row / key tiles of the two logit kernels, 32-element staging slices of D, the 256 threads of
# a row's sums, 64-key splits of the ds contraction up to M = 4096 and 96-key splits from 4097 on, and the switch from the
# 16 x 16 to the 64 x 64 logit tiles at 128 of the latter (B 65: from M = 4033 on).
B_SET = (1, 2, 5, 63, 64, 65)
M_SET = (1, 2, 63, 64, 65, 257, 513)
D_SET = (1, 5, 63, 64, 65, 384)
INPUT_SCALES = (1.0, 10.0, 1e-3)
LOGIT_SCALES = (1.0, 1.0 / 0.07, 100.0, 1e4)
ROW_SCALES = ((1.0, None), (3.0, 1.0 / 24.0))            # (grad_scale, inv_rows; None: 1 / B)
GROUP_KINDS = ("none", "class", "one")
CORNERS = ((1, 1), (63, 63), (64, 64), (65, 65), (65, 257), (64, 513))
_SETTINGS = list(itertools.product(INPUT_SCALES, LOGIT_SCALES, ROW_SCALES, GROUP_KINDS, (True, False)))         # 144
EDGE_CASES = [dict(B=B, M=M, D=D, input_scale=1.0, scale=1.0 / 0.07, grad_scale=1.0, inv_rows=None, groups=kind, want_dscale=True,
                   seed=7000 + i)
              for i, (B, M, D, kind) in enumerate([(65, 4097, 5, "class"), (64, 4097, 5, "none"), (65, 4032, 1, "class"),
                                                   (65, 4096, 7, "class")])]
BIG_CASE = dict(B=256, M=4096, D=384, input_scale=1.0, scale=1.0 / 0.07, grad_scale=1.0, inv_rows=None, groups="class",
                want_dscale=True, seed=99)


def make_groups(r, M, kind):
    """none; class: about M / 3 classes (at least one), so most positives have other rows of their class to leave out; one:
    all rows share one id, so every query's only key is its positive."""
    if kind == "none":
        return None
    if kind == "one":
        return np.full(M, -7, np.int32)
    ids = r.integers(-2 ** 31, 2 ** 31 - 1, size=max(M // 3, 1), dtype=np.int64).astype(np.int32)
    return ids[r.integers(0, len(ids), size=M)]


def make_inputs(case):
    """-> (s [B,D], bank [M,D] float32, bank_group int32 [M] | None, pos int32 [B]) of a case; the student rows lean towards
    their positives, and positives repeat wherever B > M."""
    r = np.random.default_rng(case["seed"])
    B, M, D = case["B"], case["M"], case["D"]
    bank = (r.standard_normal((M, D)) * case["input_scale"]).astype(np.float32)
    pos = r.integers(0, M, size=B).astype(np.int32)
    s = (0.5 * bank[pos] + r.standard_normal((B, D)) * case["input_scale"]).astype(np.float32)
    return s, bank, make_groups(r, M, case["groups"]), pos


def gpu_cases(D):
    """For one D: every B of B_SET with three M of M_SET taken in turn, and the six corners -- 24 (B, M) problems, each with
    the next of the 144 settings (input scale, logit scale, (grad_scale, inv_rows), groups, dscale_part or NULL), so that the
    144 problems of all D go through every setting, every B 24 times and every M at least 15 times."""
    cases, c = [], D_SET.index(D) * 24
    pairs = [(B, M_SET[(3 * i + j + D_SET.index(D)) % len(M_SET)]) for i, B in enumerate(B_SET) for j in range(3)]
    for B, M in pairs + list(CORNERS):
        x, a, (gs, ir), kind, wd = _SETTINGS[c % len(_SETTINGS)]
        cases.append(dict(B=B, M=M, D=D, input_scale=x, scale=a, grad_scale=gs, inv_rows=ir, groups=kind, want_dscale=wd,
                          seed=1000 * D + c))
        c += 1
    return cases
