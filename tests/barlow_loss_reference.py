"""Numpy float64 restatement of csn_barlow_corr and csn_barlow_grad (include/csn_hip.h): the batch
norm in training mode, the cross-correlation, the loss, and the closed-form gradients through the batch norm, with the
natural bound U on a gradient element (the same closed form with absolute values).  Shared by
tests/test_barlow_loss_cpu.py, which holds it against the oracle (oracle/losses.py:barlow_loss_sharded), the reference's
recorded values on one and two ranks and float64 autograd of the torch class, and tests/test_gpu_barlow_loss.py, which holds
the kernels against it.  Not a test module."""
import numpy as np

U23 = 2.0 ** -23            # one float32 ulp, relative
F32_TINY = 2.0 ** -126
EPS = 1e-5
LAMBD = 0.0051


def loss_tol(ref):
    return U23 * abs(ref)


def grad_tol(ref, U, noise=1e-11):
    """One rounding to float32 of a float64 result whose own error is far below ``noise`` of U."""
    return U23 * np.abs(ref) + noise * U + F32_TINY


def stats_tol(old, mean1, mean2):
    """Running statistics: two float32 roundings of a convex combination of (old, stat1, stat2)."""
    return 2.0 ** -22 * (np.abs(old) + np.abs(mean1) + np.abs(mean2))


def barlow_corr(z1, z2, inv_batch, eps=EPS, running_mean=None, running_var=None, momentum=0.1):
    """-> (c [D,D]: this rank's term, saved [4,D] = mean1, rstd1, mean2, rstd2, (running_mean, running_var) | None).
    The running statistics are updated for z1 and then for z2, rounded to float32 after each, as the kernel and one
    float32 nn.BatchNorm1d called twice do."""
    B = z1.shape[0]
    saved, zn = [], []
    run = None if running_mean is None else [np.asarray(running_mean, np.float32).copy(), np.asarray(running_var, np.float32).copy()]
    for z in (z1, z2):
        z = np.asarray(z, np.float64)
        mean = z.sum(0) / B
        var = ((z - mean) ** 2).sum(0) / B
        rstd = 1.0 / np.sqrt(var + eps)
        saved += [mean, rstd]
        zn.append((z - mean) * rstd)
        if run is not None:
            run[0] = ((1.0 - momentum) * run[0].astype(np.float64) + momentum * mean).astype(np.float32)
            run[1] = ((1.0 - momentum) * run[1].astype(np.float64) + momentum * var * B / (B - 1)).astype(np.float32)
    c = inv_batch * (zn[0].T @ zn[1])
    return c, np.stack(saved), (None if run is None else tuple(run))


def barlow_grad(z1, z2, c, c_local, saved, inv_batch, lambd=LAMBD, grad_scale=1.0):
    """-> (loss, dz1, dz2, U1, U2)."""
    z1, z2 = np.asarray(z1, np.float64), np.asarray(z2, np.float64)
    B = z1.shape[0]
    mean1, rstd1, mean2, rstd2 = saved
    n1, n2 = (z1 - mean1) * rstd1, (z2 - mean2) * rstd2
    diag = np.diagonal(c)
    G = 2.0 * lambd * c
    G[np.diag_indices_from(G)] = 2.0 * (diag - 1.0)
    loss = ((diag - 1.0) ** 2).sum() + lambd * ((c ** 2).sum() - (diag ** 2).sum())
    k1, k2 = (G * c_local).sum(1) / B, (G * c_local).sum(0) / B
    dz1 = grad_scale * rstd1 * (inv_batch * (n2 @ G.T) - n1 * k1)
    dz2 = grad_scale * rstd2 * (inv_batch * (n1 @ G) - n2 * k2)
    A1, A2 = inv_batch * (np.abs(n2) @ np.abs(G).T), inv_batch * (np.abs(n1) @ np.abs(G))
    U1 = abs(grad_scale) * rstd1 * (A1 + A1.mean(0) + np.abs(n1) * (A1 * np.abs(n1)).mean(0))
    U2 = abs(grad_scale) * rstd2 * (A2 + A2.mean(0) + np.abs(n2) * (A2 * np.abs(n2)).mean(0))
    return loss, dz1, dz2, U1, U2


def barlow_sharded(z1, z2, world, lambd=LAMBD, grad_scale=1.0, eps=EPS):
    """The two-call protocol on ``world`` equal row shards -> (loss, c summed, [(dz1, dz2, U1, U2) per rank])."""
    n = z1.shape[0] // world
    parts = [(z1[r * n:(r + 1) * n], z2[r * n:(r + 1) * n]) for r in range(world)]
    inv_batch = 1.0 / z1.shape[0]
    locals_ = [barlow_corr(a, b, inv_batch, eps) for a, b in parts]
    c = sum(cl for cl, _, _ in locals_)
    out, loss = [], None
    for (a, b), (cl, saved, _) in zip(parts, locals_):
        loss, *rest = barlow_grad(a, b, c, cl, saved, inv_batch, lambd, grad_scale)
        out.append(tuple(rest))
    return loss, c, out
