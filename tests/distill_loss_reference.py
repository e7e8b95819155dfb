"""Numpy float64 restatements of csn_distill_loss and csn_dino_loss (include/csn_hip.h): values and
closed-form gradients, with the header's conventions (a KL term with p_t == 0 is 0; a label outside [0, K) makes its row's
CE and CE gradient NaN).  Shared by tests/test_distill_loss_cpu.py, which holds them against the oracle, the reference's
recorded values and float64 autograd of the torch classes, and tests/test_gpu_distill_loss.py, which holds the kernels
against them.  Not a test module."""
import numpy as np

SOFT_KL, SOFT_CE_OF_PROBS = 0, 1
DINO_SKIP_FIRST, DINO_SKIP_SAME = 0, 1
U23 = 2.0 ** -23            # one float32 ulp, relative
F32_TINY = 2.0 ** -126


def softmax(x):
    x = x - x.max(axis=-1, keepdims=True)
    e = np.exp(x)
    return e / e.sum(axis=-1, keepdims=True)


def log_softmax(x):
    x = x - x.max(axis=-1, keepdims=True)
    return x - np.log(np.exp(x).sum(axis=-1, keepdims=True))


def _cross_entropy(logits, labels):
    """-> (ce[B], softmax(logits) - onehot [B,K]); a label outside [0, K): NaN in both for that row."""
    z = np.asarray(logits, np.float64)
    B, K = z.shape
    lab = np.asarray(labels, np.int64)
    ok = (lab >= 0) & (lab < K)
    safe = np.where(ok, lab, 0)
    ce = -log_softmax(z)[np.arange(B), safe]
    g = softmax(z)
    g[np.arange(B), safe] -= 1.0
    ce[~ok] = np.nan
    g[~ok] = np.nan
    return ce, g


def distill_loss(student, teacher, soft_mode, T, w_soft, logits=None, labels=None, w_ce=0.0, alias=False, grad_scale=1.0):
    """-> (loss, dstudent[B,D], dlogits[B,K] | None).  ``alias``: the student is also the logits of the CE term, whose
    gradient is then part of dstudent (dlogits is None)."""
    s, t = np.asarray(student, np.float64), np.asarray(teacher, np.float64)
    B = s.shape[0]
    p_t, q, log_q = softmax(t / T), softmax(s / T), log_softmax(s / T)
    if soft_mode == SOFT_KL:
        # log p_t as log_softmax(t / T): finite where p_t underflows, and equal to log_q bit for bit when s is t
        terms = np.where(p_t > 0, p_t * (log_softmax(t / T) - log_q), 0.0)
        soft = terms.sum(axis=-1)
        ds = w_soft / (B * T) * (q - p_t)
    elif soft_mode == SOFT_CE_OF_PROBS:
        a = log_softmax(p_t)
        soft = -(q * a).sum(axis=-1)
        ds = -w_soft / (B * T) * q * (a - (q * a).sum(axis=-1, keepdims=True))
    else:
        raise ValueError(soft_mode)
    loss = w_soft / B * soft.sum()
    dl = None
    if alias or logits is not None:
        ce, g = _cross_entropy(s if alias else logits, labels)
        loss = loss + w_ce / B * ce.sum()
        if alias:
            ds = ds + w_ce / B * g
        else:
            dl = grad_scale * w_ce / B * g
    return float(loss), grad_scale * ds, dl


def distill_grad_bound(B, T, w_soft, w_ce, grad_scale):
    """U of the issue: the natural bound on any gradient element of csn_distill_loss."""
    return abs(grad_scale) * (abs(w_soft) / T + abs(w_ce)) / B


def dino_pairs(V, G, pairing):
    """S_g for every teacher view g."""
    if pairing == DINO_SKIP_FIRST:
        return [list(range(1, V)) for _ in range(G)]
    if pairing == DINO_SKIP_SAME:
        return [[v for v in range(V) if v != g] for g in range(G)]
    raise ValueError(pairing)


def dino_loss(student, teacher, center, teacher_temp, student_temp, pairing, grad_scale=1.0):
    """student [V,B,D], teacher [G,B,D], center [D] or [B,D] -> (loss, dstudent[V,B,D])."""
    s, t = np.asarray(student, np.float64), np.asarray(teacher, np.float64)
    V, B, D = s.shape
    G = t.shape[0]
    c = np.asarray(center, np.float64).reshape(-1, D)           # [1,D] or [B,D]: broadcasts over the views
    q = softmax((t - c[None]) / teacher_temp)
    logp, p = log_softmax(s / student_temp), softmax(s / student_temp)
    norm = 1.0 / (G * B * (V - 1))
    total, qsum, n = 0.0, np.zeros_like(s), np.zeros(V)
    for g, views in enumerate(dino_pairs(V, G, pairing)):
        for v in views:
            total += (q[g] * logp[v]).sum()
            qsum[v] += q[g]
            n[v] += 1
    ds = -norm / student_temp * (qsum - n[:, None, None] * p)
    ds[n == 0] = 0.0
    return float(-norm * total), grad_scale * ds


def dino_grad_bound(B, V, student_temp, grad_scale):
    return abs(grad_scale) / (student_temp * B * (V - 1))


def loss_tol(ref):
    return U23 * abs(ref)


def grad_tol(ref, U):
    return U23 * np.abs(ref) + 1e-12 * U + F32_TINY


# ---- the library's losses as calls of distill_loss (the table of the header) -------------------------------------------
def featdist(student, teacher, T, labels, pred_label, alpha=0.5, beta=0.5):
    return distill_loss(student, teacher, SOFT_CE_OF_PROBS, T, beta, logits=pred_label, labels=labels, w_ce=alpha)


def kd(outputs, labels, teacher_outputs, alpha, T):
    return distill_loss(outputs, teacher_outputs, SOFT_KL, T, alpha * T * T / np.shape(outputs)[1], labels=labels,
                        w_ce=1.0 - alpha, alias=True)


def featdist_kd(student, teacher, T, labels, soft_w=0.25, ce_w=0.75):
    return distill_loss(student, teacher, SOFT_KL, T, soft_w * T * T, labels=labels, w_ce=ce_w, alias=True)


def featdist_soft(student, teacher, T):
    return distill_loss(student, teacher, SOFT_KL, T, T * T)
