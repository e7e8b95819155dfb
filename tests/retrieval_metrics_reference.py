"""Numpy restatements of the contracts of csn_topk_merge and csn_topk_class_metrics (include/csn_hip.h), the numpy
(search, merge, metrics) engine of retrieval.evaluate_device, and the label sets both retrieval-metrics test files draw;
not a test module."""
import numpy as np

from oracle import retrieval as oracle_retrieval


# ---- the two contracts ---------------------------------------------------------------------------------------------------
def topk_merge(D_parts, I_parts, k):
    """D_parts / I_parts [P, Nq, k_in] -> (D[Nq,k] float64, I[Nq,k] int64): per query the k smallest real entries under
    (distance, index, position), padding (index < 0) behind every real entry; a padding pick comes out as (+inf, -1)."""
    D = np.concatenate([np.asarray(d, dtype=np.float64) for d in D_parts], axis=1)
    I = np.concatenate([np.asarray(i, dtype=np.int64) for i in I_parts], axis=1)
    assert D.shape == I.shape and D.shape[1] >= k
    pad = I < 0
    Dout, Iout = np.empty((len(D), k), np.float64), np.empty((len(D), k), np.int64)
    for r in range(len(D)):
        o = np.lexsort((I[r], D[r], pad[r]))[:k]              # stable: equal pairs stay in order of position
        Dout[r] = np.where(pad[r, o], np.inf, D[r, o])
        Iout[r] = np.where(pad[r, o], -1, I[r, o])
    return Dout, Iout


def class_metrics(idx, gallery_class, query_class, n_classes):
    """-> dict(hits, top1, pred [Nq] int32; class [n_classes,4] int64; top1_correct [1] int64)."""
    idx = np.asarray(idx, dtype=np.int64)
    gc, qc = np.asarray(gallery_class, dtype=np.int32), np.asarray(query_class, dtype=np.int32)
    ok = (idx >= 0) & (idx < len(gc))
    cls = np.where(ok, gc[np.where(ok, idx, 0)], -1)          # an index outside the gallery is a miss, class -1
    hits = ((cls == qc[:, None]) & ok).sum(axis=1).astype(np.int32)
    top1 = cls[:, 0].astype(np.int32)
    pred = np.where(hits > 0, qc, top1).astype(np.int32)
    out = np.zeros((n_classes, 4), dtype=np.int64)
    out[:, 3] = np.iinfo(np.int64).max
    np.add.at(out[:, 0], qc, 1)
    np.add.at(out[:, 1], qc, (hits > 0).astype(np.int64))
    np.add.at(out[:, 2], qc, hits.astype(np.int64))
    np.minimum.at(out[:, 3], qc, np.arange(len(qc), dtype=np.int64))
    out[out[:, 0] == 0, 3] = -1
    correct = np.array([int(((top1 == qc) & ok[:, 0]).sum())], dtype=np.int64)
    return {"hits": hits, "top1": top1, "pred": pred, "class": out, "top1_correct": correct}


# ---- the numpy engine of retrieval.evaluate_device ------------------------------------------------------------------------
def search(gallery, query, k):
    """What retrieval.l2_search returns, from the oracle's brute force: (D float32, I int64)."""
    d, i = oracle_retrieval.l2_topk(np.asarray(gallery, dtype=np.float32).reshape(len(gallery), -1),
                                    np.asarray(query, dtype=np.float32).reshape(len(query), -1), k)
    with np.errstate(over="ignore"):
        return d.astype(np.float32), i.astype(np.int64)


def merge(D_parts, I_parts, k):
    """topk_merge with retrieval.merge_topk_device's check of the result."""
    D, I = topk_merge(D_parts, I_parts, k)
    if (I[:, -1] < 0).any():
        raise ValueError(f"merge_topk: fewer than k={k} candidates for a query")
    return D, I


NUMPY_ENGINE = (search, merge, class_metrics)


# ---- label sets -----------------------------------------------------------------------------------------------------------
class Dataset:
    """The two class maps of dataset.EEGDataset, ids 0 .. n-1."""

    def __init__(self, n_classes, prefix="class_"):
        self.class_id_to_str = {c: f"{prefix}{c}" for c in range(n_classes)}
        self.class_str_to_id = {f"{prefix}{c}": c for c in range(n_classes)}


def label(c, prefix="class_"):
    return {"ClassId": int(c), "ClassName": f"{prefix}{int(c)}", "imagenetClassId": str(int(c))}


def label_set(n_classes, Ng, Nq, seed):
    """Class ids of a gallery and of the queries.  With 3 classes or more, class n-1 occurs in the gallery only and class
    n-2 among the queries only (where there are two queries or more)."""
    rng = np.random.default_rng(seed)
    g = rng.integers(0, n_classes, Ng)
    q = rng.integers(0, n_classes, Nq)
    if n_classes >= 3:
        g[g == n_classes - 2] = 0
        q[q == n_classes - 1] = 1
        g[0] = n_classes - 1
        if Nq >= 2:
            q[-1] = n_classes - 2
    return g.astype(np.int64), q.astype(np.int64)


def neighbour_lists(g_cls, q_cls, k, seed, p_own=0.4):
    """I[Nq,k]: random gallery rows, a share of them drawn from the query's own class where the gallery has it."""
    rng = np.random.default_rng(seed)
    I = rng.integers(0, len(g_cls), (len(q_cls), k))
    for r, c in enumerate(q_cls):
        own = np.nonzero(g_cls == c)[0]
        if len(own):
            take = rng.random(k) < p_own * rng.random()
            I[r, take] = rng.choice(own, int(take.sum()))
    return I.astype(np.int64)


# ---- candidate lists for the merge ----------------------------------------------------------------------------------------
def merge_case(P, Nq, k_in, seed, values=4, pad_parts=(), inf_at=()):
    """D_parts / I_parts [P, Nq, k_in]: every part ascending under (distance, index) like a search result, distances from
    `values` small integers (ties inside and across parts), indices distinct across the parts of a query.  pad_parts:
    {part: real entries kept} -- the rest of that part is (+inf, -1).  inf_at: (part, query) whose last real distance is a
    real +inf."""
    rng = np.random.default_rng(seed)
    D = rng.integers(0, values, (P, Nq, k_in)).astype(np.float64)
    I = np.empty((P, Nq, k_in), dtype=np.int64)
    for q in range(Nq):
        I[:, q, :] = rng.permutation(P * k_in).reshape(P, k_in)
    kept = np.full(P, k_in)
    for p, n in dict(pad_parts).items():
        kept[p] = n
    for p, q in inf_at:
        D[p, q, kept[p] - 1] = np.inf
    for p in range(P):
        for q in range(Nq):
            o = np.lexsort((I[p, q, :kept[p]], D[p, q, :kept[p]]))
            D[p, q, :kept[p]], I[p, q, :kept[p]] = D[p, q, o], I[p, q, o]
        D[p, :, kept[p]:], I[p, :, kept[p]:] = np.inf, -1
    return D, I


def merge_cases():
    """(id, D_parts, I_parts, k) over P in {1, 3, 8}, k_in in {1, 5, 64}, k in {1, 5, k_in, min(P k_in, 100)}, with padding
    in some parts (every query keeps k real candidates), ties across parts, and a real +inf beside padding."""
    cases = []
    for P in (1, 3, 8):
        for k_in in (1, 5, 64):
            for k in sorted({1, 5, k_in, min(P * k_in, 100)}):
                if k > P * k_in:
                    continue
                pad = {}
                if P > 1 and k_in > 1 and (P - 1) * k_in + k_in // 2 >= k:
                    pad = {P - 1: k_in // 2}                   # the last part is half padding
                inf_at = [(P - 1, 0)] if pad and pad[P - 1] >= 1 else []
                D, I = merge_case(P, 3, k_in, 1000 * P + 10 * k_in + k, pad_parts=pad, inf_at=inf_at)
                cases.append((f"P{P}-kin{k_in}-k{k}" + ("-pad-inf" if pad else ""), D, I, k))
    return cases
