"""Numpy float64 restatement of csn_contrastive_lse and csn_contrastive_grad (include/csn_hip.h): the
symmetric in-batch contrastive loss of normalised student rows against normalised teacher rows over the global batch, in the
two calls the ranks make, with the natural bound U on a gradient element (the gradient formula with absolute values
throughout).  ``reverse=True`` runs every sum over its operands in reversed order: a second float64 evaluation order, whose
distance from the first is the measured constant SPREAD below.  Shared by tests/test_contrastive_loss_cpu.py, which holds
it against float64 autograd of the one-process formula, and tests/test_gpu_contrastive_loss.py, which holds the kernels
against it.  Not a test module."""
import itertools

import numpy as np

U23 = 2.0 ** -23            # one float32 ulp, relative
U52 = 2.0 ** -52
F32_TINY = 2.0 ** -126
EPS = 1e-12                 # F.normalize

# ---- measured constants (tests/test_contrastive_loss_cpu.py::test_measured_constants_hold measures both again) ------------
# (a) the worst |ds(ascending) - ds(reversed)| / U of two float64 evaluation orders of this restatement over gpu_cases() and
#     BIG_CASE.  The worst cases are the ones at logit scale 1e4, where a logit carries 1e4 times the rounding of its dot
#     product and exp passes that on as a relative error.
SPREAD = 3.1e-13           # measured 3.024e-13
C_NOISE = 10.0 * SPREAD     # the c of the gradient bound: fma contraction and tile order are further float64 orders
assert C_NOISE <= 1e-9      # a float32 intermediate (6e-8) is still excluded
# (b) the distance of the float32 torch form (ContrastiveLoss on float32 CPU tensors) from this restatement over the same
#     cases at the logit scales a trainer can reach (max_scale = 100): |loss - ref| / loss_scale and, per gradient tensor,
#     max |ds - ref| / max U.
TORCH_FORM_LOSS = 1.3e-7    # measured 1.206e-07
TORCH_FORM_GRAD = 6.6e-7    # measured 6.541e-07


def loss_tol(ref):
    return U23 * abs(ref)


def grad_tol(ref, U):
    """One rounding to float32 of a float64 result that is another evaluation order of the restatement."""
    return U23 * np.abs(ref) + C_NOISE * U + F32_TINY


def rows_tol(ref, scale, N, D):
    """lA, lB, p are float64 outputs.  A normalised row carries a relative error of (D / 2 + 3) roundings, a dot product of
    two of them D more, the logit one more: (2 D + 8) 2^-53 scale |s^| . |t^| <= (2 D + 8) 2^-53 scale.  A log-sum-exp adds N
    roundings of its sum (relative, so absolute in the logarithm) and a few of its own value.  Twice that: both sides round."""
    return U52 * ((2 * D + 8) * scale + N + 8 + 4 * np.abs(ref))


def loss_scale(rows, w_a=0.5, w_b=0.5):
    """The loss with absolute values throughout: mean_i [ |w_a| (|lA_i| + |p_i|) + |w_b| (|lB_i| + |p_i|) ]."""
    lA, lB, p = np.abs(rows)
    return float((abs(w_a) * (lA + p) + abs(w_b) * (lB + p)).mean())


def _sum(x, axis, reverse):
    return np.flip(x, axis).sum(axis) if reverse else x.sum(axis)


def _mm(a, b, reverse):
    """a [M,K] @ b [K,N], the summed index in reversed order if asked."""
    return a[:, ::-1] @ b[::-1, :] if reverse else a @ b


def normalise(x, reverse=False):
    """-> (x^, |x|, max(|x|, eps))."""
    x = np.asarray(x, np.float64)
    nrm = np.sqrt(_sum(x * x, 1, reverse))
    den = np.where(nrm < EPS, EPS, nrm)            # NaN stays NaN
    return x / den[:, None], nrm, den


def left_out(group_all, row0, B, N):
    """[B,N] bool: key j is left out of local query i."""
    if group_all is None:
        return np.zeros((B, N), bool)
    g = np.asarray(group_all)
    rows = np.arange(row0, row0 + B)
    return (g[rows][:, None] == g[None, :]) & (rows[:, None] != np.arange(N)[None, :])


def _lse(z, out, reverse):
    """log sum_{not out} exp(z) per row, the maximum subtracted; a key that is left out adds the constant 0."""
    zm = np.where(out, -np.inf, z)
    with np.errstate(invalid="ignore"):
        m = np.nanmax(np.where(np.isnan(zm), -np.inf, zm), axis=1)
        e = np.where(out, 0.0, np.exp(z - m[:, None]))
        return m + np.log(_sum(e, 1, reverse))


def contrastive_lse(s_all, t_all, group_all, row0, B, scale, w_a=0.5, w_b=0.5, reverse=False):
    """-> (rows_out [3,B] = lA, lB, p of the local rows, loss_part: the local rows' part of the global loss)."""
    sh, _, _ = normalise(s_all, reverse)
    th, _, _ = normalise(t_all, reverse)
    N = sh.shape[0]
    loc = slice(row0, row0 + B)
    out = left_out(group_all, row0, B, N)
    with np.errstate(invalid="ignore", over="ignore"):
        za = scale * _mm(sh[loc], th.T, reverse)
        zb = scale * _mm(th[loc], sh.T, reverse)
        lA, lB = _lse(za, out, reverse), _lse(zb, out, reverse)
        p = za[np.arange(B), np.arange(row0, row0 + B)]
        terms = w_a * (lA - p) + w_b * (lB - p)
    return np.stack([lA, lB, p]), _sum(terms, 0, reverse) / N


def contrastive_grad(s_all, t_all, group_all, row0, B, scale, lse_a_local, lse_b_all, w_a=0.5, w_b=0.5, grad_scale=1.0,
                     reverse=False):
    """-> (ds [B,D], dscale_part, U [B,D], Uscale): the gradient of the global loss for the local student rows, holding
    grad_scale; the local rows' part of dL/d scale; and the two with absolute values throughout."""
    sh, nrm, den = normalise(s_all, reverse)
    th, _, _ = normalise(t_all, reverse)
    N = sh.shape[0]
    loc = slice(row0, row0 + B)
    out = left_out(group_all, row0, B, N)
    lse_a_local, lse_b_all = np.asarray(lse_a_local, np.float64), np.asarray(lse_b_all, np.float64)
    with np.errstate(invalid="ignore", over="ignore"):
        da = _mm(sh[loc], th.T, reverse)               # s^_i . t^_j
        db = _mm(th[loc], sh.T, reverse)               # t^_i . s^_j
        PA = np.where(out, 0.0, np.exp(scale * da - lse_a_local[:, None]))
        PBt = np.where(out, 0.0, np.exp(scale * da - lse_b_all[None, :]))         # PB_ki for local i, all k
        PBq = np.where(out, 0.0, np.exp(scale * db - lse_b_all[loc][:, None]))    # PB_ij for local i as the query
        W, Wabs = w_a * PA + w_b * PBt, abs(w_a) * PA + abs(w_b) * PBt
        g = (scale / N) * (_mm(W, th, reverse) - (w_a + w_b) * th[loc])
        gabs = (scale / N) * (Wabs @ np.abs(th) + (abs(w_a) + abs(w_b)) * np.abs(th[loc]))
        proj = (nrm[loc] > EPS)[:, None]
        shl = sh[loc]
        dot = _sum(shl * g, 1, reverse)[:, None]
        ds = grad_scale * (g - np.where(proj, shl * dot, 0.0)) / den[loc][:, None]
        U = abs(grad_scale) * (gabs + np.where(proj, np.abs(shl) * (np.abs(shl) * gabs).sum(1)[:, None], 0.0)) / den[loc][:, None]
        dii = da[np.arange(B), np.arange(row0, row0 + B)]
        sa = _sum(np.where(out, 0.0, PA * da), 1, reverse)
        sb = _sum(np.where(out, 0.0, PBq * db), 1, reverse)
        dscale = _sum(w_a * (sa - dii) + w_b * (sb - dii), 0, reverse) / N
        Uscale = (abs(w_a) * ((PA * np.abs(da)).sum(1) + np.abs(dii)) + abs(w_b) * ((PBq * np.abs(db)).sum(1) + np.abs(dii))).sum() / N
    return ds, dscale, U, Uscale


def contrastive_sharded(s_all, t_all, group_all, world, scale, w_a=0.5, w_b=0.5, grad_scale=1.0, reverse=False):
    """The two-call protocol on ``world`` equal row shards -> (loss, rows [3,N], ds [N,D], dscale, U [N,D], Uscale): the
    partials summed in rank order, lB gathered in rank order."""
    N = np.asarray(s_all).shape[0]
    B = N // world
    assert B * world == N
    first = [contrastive_lse(s_all, t_all, group_all, r * B, B, scale, w_a, w_b, reverse) for r in range(world)]
    rows = np.concatenate([f[0] for f in first], axis=1)
    loss = sum(f[1] for f in first)
    second = [contrastive_grad(s_all, t_all, group_all, r * B, B, scale, rows[0, r * B:(r + 1) * B], rows[1], w_a, w_b,
                               grad_scale, reverse) for r in range(world)]
    return (loss, rows, np.concatenate([x[0] for x in second]), sum(x[1] for x in second),
            np.concatenate([x[2] for x in second]), sum(x[3] for x in second))


# ---- the cases of the GPU accuracy test, and of the two measured constants ----------------------------------------------------
B_SET = (1, 2, 5, 63, 64, 65)
D_SET = (1, 5, 63, 64, 65, 384)
INPUT_SCALES = (1.0, 10.0, 1e-3)
LOGIT_SCALES = (1.0, 1.0 / 0.07, 100.0, 1e4)
GRAD_SCALES = (1.0, 3.0)
GROUP_KINDS = ("none", "sparse", "masked_row")
BIG_CASE = dict(B=256, N=2048, D=384, row0=768, input_scale=1.0, scale=1.0 / 0.07, grad_scale=1.0, groups="sparse",
                want_dscale=True, seed=99)
_SETTINGS = list(itertools.product(INPUT_SCALES, LOGIT_SCALES, GRAD_SCALES, GROUP_KINDS, (True, False)))       # 144


def make_groups(r, N, kind):
    """none; sparse: a quarter of the rows repeat another row's id (ids of any sign and size); masked_row: all rows share one
    id, so every query's every other key is left out."""
    if kind == "none":
        return None
    if kind == "masked_row":
        return np.full(N, -7, np.int32)
    g = r.integers(-2 ** 31, 2 ** 31 - 1, size=N, dtype=np.int64).astype(np.int32)
    for i in range(0, N, 4):
        g[i] = g[r.integers(0, N)]
    return g


def make_inputs(case):
    """-> (s_all, t_all [N,D] float32, group_all int32 [N] | None) of a case of gpu_cases() / BIG_CASE."""
    r = np.random.default_rng(case["seed"])
    N, D = case["N"], case["D"]
    s = (r.standard_normal((N, D)) * case["input_scale"]).astype(np.float32)
    t = (0.5 * s + r.standard_normal((N, D)) * case["input_scale"]).astype(np.float32)
    return s, t, make_groups(r, N, case["groups"])


def gpu_cases(D):
    """For one D: every B of B_SET with N in {B, 2B, 3B+1}, each with two of the 144 settings (input scale, logit scale,
    grad_scale, groups, dscale_part or NULL) taken in turn, so that the 216 (B, N, D) problems of all D go through every
    setting; ``row0s``: the start, the middle and the end."""
    cases, c = [], D_SET.index(D) * 36
    for B in B_SET:
        for N in (B, 2 * B, 3 * B + 1):
            for _ in range(2):
                x, a, gs, kind, wd = _SETTINGS[c % len(_SETTINGS)]
                cases.append(dict(B=B, N=N, D=D, row0s=sorted({0, (N - B) // 2, N - B}), input_scale=x, scale=a, grad_scale=gs,
                                  groups=kind, want_dscale=wd, seed=1000 * D + c))
                c += 1
    return cases
