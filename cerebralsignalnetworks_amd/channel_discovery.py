"""Greedy forward selection of EEG channels by retrieval recall, on the GPU.

Restates the discovery loop of /root/reference/TestRetrieval_Perils_DiscoverChannels.py:125-351 (and of its two
siblings): one round per accepted channel; a round tries every remaining channel ``ch``, searches the gallery with the
raw window ``eeg[time_low:time_high, fixed + [ch]]`` as the feature at k = topK, folds the neighbours into the per-class
Recall / Precision of ``retrieval._bookkeeping`` and keeps the channel with the best recall.

The reference builds one faiss index per candidate.  The squared L2 distance over a channel subset is the sum of the
per-channel distances, so here the per-channel matrices are computed once (``csn_chan_l2_dist``), a round is one float64
add and one selection per (candidate, query, gallery row) (``csn_chan_l2_select``), and the accepted channel is added to
the running sum (``csn_chan_l2_accumulate``): ((D_s1 + D_s2) + ...) + D_cand in selection order.

There is no CPU path in the product: ``engine`` defaults to the HIP kernels.  Tests inject a numpy triple.
"""
from collections import namedtuple

import numpy as np
import torch

from . import cabi

STOP_NO_IMPROVEMENT = "found no channel better than last iteration"
STOP_MAX_CHANNELS = "max_channels reached"
STOP_EXHAUSTED = "no candidate left"

DiscoveryResult = namedtuple("DiscoveryResult", ["order", "rounds", "stopped", "top1", "best"])
DiscoveryResult.__doc__ = """order: accepted channels, ``start`` first.  rounds: one ``{channel: (Recall_Total,
Precision_Total)}`` dict per round, candidates ascending.  stopped: why discovery ended.  top1: one ``{channel: top-1
accuracy}`` dict per round.  best: per round the leading entry of all rounds so far, ``(channel subset, (Recall_Total,
Precision_Total))`` -- the reference's "best score channel" line -- or None while every recall is 0."""


def _to_nct(x, layout):
    if layout not in ("nct", "ntc"):
        raise ValueError(f"layout must be 'nct' or 'ntc', got {layout!r}")
    if layout == "nct":
        return x
    return x.transpose(1, 2) if isinstance(x, torch.Tensor) else np.transpose(np.asarray(x), (0, 2, 1))


# ---- the HIP engine -----------------------------------------------------------------------------------------------------
def _dev(x, dtype=None):
    t = x if isinstance(x, torch.Tensor) else torch.as_tensor(np.asarray(x))
    if not t.is_cuda:
        t = t.to(torch.device("cuda", torch.cuda.current_device()))
    return t if dtype is None or t.dtype == dtype else t.to(dtype)


def _hip_distances(gallery_nct, query_nct, t0, t1, channels):
    return cabi.chan_l2_dist(_dev(gallery_nct, torch.float32), _dev(query_nct, torch.float32), t0, t1, channels)


def _hip_select(base, Dc, gallery_class, query_class, k):
    out = cabi.chan_l2_select(base, Dc, _dev(gallery_class, torch.int32), _dev(query_class, torch.int32), k,
                              want=("hits", "top1"))
    return out["hits"].cpu().numpy(), out["top1"].cpu().numpy()


def _hip_accumulate(base, D_one, first):
    if base is None:
        base = torch.empty_like(D_one, memory_format=torch.contiguous_format)
    return cabi.chan_l2_accumulate(base, D_one.contiguous(), first)


HIP_ENGINE = (_hip_distances, _hip_select, _hip_accumulate)


def channel_distances(gallery_nct, query_nct, time_low, time_high, channels=None, layout="nct"):
    """Per-channel squared-L2 matrices ``Dc[nch, Nq, Ng]`` (float64, on the device) of the window
    ``[time_low, time_high)``; ``channels=None`` = all, ascending.  ``layout="ntc"``: the recordings are [N, T, C]."""
    return _hip_distances(_to_nct(gallery_nct, layout), _to_nct(query_nct, layout), int(time_low), int(time_high),
                          None if channels is None else [int(c) for c in channels])


# ---- labels and metrics -------------------------------------------------------------------------------------------------
def _class_ids(gallery_labels, query_labels, class_id_to_str):
    """int32 class ids of both sides; ValueError unless the class map is injective and agrees with every ClassName (then
    the bookkeeping's string comparisons are comparisons of class ids)."""
    seen = {}
    for cid, name in class_id_to_str.items():
        if name in seen:
            raise ValueError(f"class_id_to_str is not injective: ids {seen[name]} and {cid} are both {name!r}")
        seen[name] = cid
    out = []
    for side, labels in (("gallery", gallery_labels), ("query", query_labels)):
        ids = np.empty(len(labels), dtype=np.int32)
        for i, lab in enumerate(labels):
            cid = lab["ClassId"]
            if cid not in class_id_to_str:
                raise ValueError(f"{side} label {i}: ClassId {cid} is not in class_id_to_str")
            if class_id_to_str[cid] != lab["ClassName"]:
                raise ValueError(f"{side} label {i}: ClassName {lab['ClassName']!r} is not class_id_to_str[{cid}] = "
                                 f"{class_id_to_str[cid]!r}")
            ids[i] = int(cid)
        out.append(ids)
    return out


def _fold(hits, top1, query_class, class_rows, topK):
    """(Recall_Total, Precision_Total, top-1 accuracy) of one candidate from its per-query hit counts: the floats of
    ``retrieval._bookkeeping`` (TestRetrieval_Perils_DiscoverChannels.py:282-317) -- per-class round(..., 2), classes in
    order of first appearance among the queries, np.array(...).mean()."""
    recalls, precisions = [], []
    for rows in class_rows:
        h = hits[rows]
        tp = int((h > 0).sum())
        retrieved = int(h.sum())            # a query adds its count only when it is a true positive: count > 0
        total = len(rows)
        recalls.append(round((tp * 100) / total, 2))
        precisions.append(round((retrieved * 100) / (total * topK), 2))
    return (float(np.array(recalls).mean()), float(np.array(precisions).mean()),
            int((top1 == query_class).sum()) / max(1, len(query_class)))


# ---- the greedy loop ----------------------------------------------------------------------------------------------------
def discover_channels(gallery_eeg, query_eeg, gallery_labels, query_labels, dataset, topK=5, time_low=20, time_high=480,
                      start=(), max_channels=None, budget_bytes=4 << 30, engine=None, layout="nct"):
    """Greedy channel discovery.  gallery_eeg / query_eeg: [N, C, T] recordings (``layout="ntc"``: [N, T, C]); labels: the
    ``{"ClassId", "ClassName"}`` dicts ``evaluate`` takes; ``dataset.class_id_to_str`` must be injective and agree with
    ``ClassName``.  ``start``: channels fixed from the beginning, in order.  -> DiscoveryResult.

    Rule (the reference script :331-351, whose metrics dict is never reset): a round's winner is its lowest-numbered
    candidate with the round's best recall; it is accepted only if that recall is strictly greater than every recall of
    every earlier round and than 0, otherwise discovery stops.  It also stops once ``max_channels`` are accepted
    (``start`` included) or no candidate is left.

    The per-channel matrices of all C channels take C * Nq * Ng * 8 bytes; beyond ``budget_bytes`` they are computed and
    selected from in blocks of channels, round by round.  The result does not depend on the block size."""
    distances, select, accumulate = engine or HIP_ENGINE
    g_cls, q_cls = _class_ids(gallery_labels, query_labels, dataset.class_id_to_str)
    gal, qry = _to_nct(gallery_eeg, layout), _to_nct(query_eeg, layout)
    if engine is None:                      # upload once, not once per block
        gal, qry = _dev(gal, torch.float32), _dev(qry, torch.float32)
    Ng, C, T = (int(v) for v in gal.shape)
    Nq = int(qry.shape[0])
    if tuple(int(v) for v in qry.shape[1:]) != (C, T):
        raise ValueError(f"gallery recordings are [*, {C}, {T}], query recordings {tuple(qry.shape)}")
    if len(g_cls) != Ng or len(q_cls) != Nq:
        raise ValueError("one label per recording is needed")
    t0, t1 = int(time_low), int(time_high)
    if not 0 <= t0 < t1 <= T:
        raise ValueError(f"window [{t0}, {t1}) is empty or outside [0, {T}]")
    topK = int(topK)
    if not 1 <= topK <= min(64, Ng):
        raise ValueError(f"topK={topK} must be in 1..min(64, {Ng})")
    order = [int(c) for c in start]
    if len(set(order)) != len(order) or any(not 0 <= c < C for c in order):
        raise ValueError(f"start={list(start)} must be distinct channels in [0, {C})")

    class_rows = {}                         # rows of every query class, classes in order of first appearance
    for i, c in enumerate(q_cls.tolist()):
        class_rows.setdefault(c, []).append(i)
    class_rows = [np.array(v) for v in class_rows.values()]

    block = max(1, min(C, int(budget_bytes) // (Nq * Ng * 8)))
    resident = distances(gal, qry, t0, t1, None) if block >= C else None

    def one(ch):
        return resident[ch] if resident is not None else distances(gal, qry, t0, t1, [ch])[0]

    base = None
    for i, ch in enumerate(order):
        base = accumulate(base, one(ch), i == 0)

    rounds, top1s, leaders = [], [], []
    leader = None                           # (subset, (recall, precision)) of the best entry of all rounds so far
    best_so_far = 0                         # the best recall of all rounds so far: the reference never resets its table
    while True:
        if max_channels is not None and len(order) >= max_channels:
            stopped = STOP_MAX_CHANNELS
            break
        cands = [c for c in range(C) if c not in order]
        if not cands:
            stopped = STOP_EXHAUSTED
            break
        metrics, top1 = {}, {}
        if resident is not None:
            blocks = [(list(range(C)), resident)]
        else:
            blocks = ((cands[s:s + block], None) for s in range(0, len(cands), block))
        for chans, Dc in blocks:
            if Dc is None:
                Dc = distances(gal, qry, t0, t1, chans)
            hits, first = select(base, Dc, g_cls, q_cls, topK)
            for j, ch in enumerate(chans):
                if ch not in order:
                    r, p, a = _fold(np.asarray(hits[j]), np.asarray(first[j]), q_cls, class_rows, topK)
                    metrics[ch], top1[ch] = (r, p), a
        rounds.append(metrics)
        top1s.append(top1)
        winner, round_best = None, best_so_far
        for ch, (r, _) in metrics.items():  # first strict maximum in insertion (= ascending channel) order
            if r > round_best:
                winner, round_best = ch, r
        if winner is not None:
            leader = (tuple(order) + (winner,), metrics[winner])
        leaders.append(leader)
        if winner is None:
            stopped = STOP_NO_IMPROVEMENT
            break
        best_so_far = round_best
        base = accumulate(base, one(winner), len(order) == 0)
        order.append(winner)
    return DiscoveryResult(order=order, rounds=rounds, stopped=stopped, top1=top1s, best=leaders)
