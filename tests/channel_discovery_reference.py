"""Numpy restatements for channel discovery (csrc/channel_l2.hip, channel_discovery.py), shared by
tests/test_channel_discovery_cpu.py and tests/test_gpu_channel_discovery.py (not a test module):

* the three kernels' contracts (include/csn_hip.h),
* the numpy engine (distances, select, accumulate) that the tests inject into ``discover_channels``,
* ``naive_discover``: the rule of the reference loop (TestRetrieval_Perils_DiscoverChannels.py:125-351) restated naively
  in this project's own words -- per candidate the feature is gathered [N, Tw, m+1] time-major, flattened, searched with
  ``oracle.retrieval.l2_topk`` and folded with ``oracle.retrieval.evaluate_from_indices``; one table of scores persists
  across rounds and the winner is its first strict maximum in insertion order,
* the planted problems both test files run.
"""
import numpy as np

from oracle import retrieval as oracle_retrieval
from topk_tiled_reference import d2_kernel_order, exact_topk


# ---- kernel contracts ---------------------------------------------------------------------------------------------------
def chan_l2_dist(gallery_nct, query_nct, t0, t1, channels=None):
    """Dc[nch, Nq, Ng] float64: one ascending chain over the window per (channel, pair) (unfused here, as
    ``d2_kernel_order``: equal to the kernel's fused chain wherever every partial sum is exact)."""
    g, q = np.asarray(gallery_nct, np.float32), np.asarray(query_nct, np.float32)
    channels = range(g.shape[1]) if channels is None else channels
    return np.stack([d2_kernel_order(q[:, c, t0:t1], g[:, c, t0:t1]) for c in channels])


def chan_l2_select(base, Dc, gallery_class, query_class, k):
    """-> dict(idx [nc,Nq,k], dist [nc,Nq,k], hits [nc,Nq], top1 [nc,Nq]): the k smallest of base + Dc[j] under (value,
    index); one IEEE add."""
    Dc = np.asarray(Dc, np.float64)
    gc, qc = np.asarray(gallery_class), np.asarray(query_class)
    idx, dist = [], []
    for j in range(Dc.shape[0]):
        v = Dc[j] if base is None else np.asarray(base, np.float64) + Dc[j]
        d, i = exact_topk(v, k)
        idx.append(i)
        dist.append(d)
    idx, dist = np.stack(idx), np.stack(dist)
    return dict(idx=idx.astype(np.int64), dist=dist, hits=(gc[idx] == qc[None, :, None]).sum(axis=-1).astype(np.int32),
                top1=gc[idx[..., 0]].astype(np.int32))


def chan_l2_accumulate(base, D_one, first):
    return np.array(D_one, dtype=np.float64, copy=True) if first else np.asarray(base, np.float64) + np.asarray(D_one)


# ---- the numpy engine ---------------------------------------------------------------------------------------------------
def _np_select(base, Dc, gallery_class, query_class, k):
    out = chan_l2_select(base, Dc, gallery_class, query_class, k)
    return out["hits"], out["top1"]


NUMPY_ENGINE = (chan_l2_dist, _np_select, chan_l2_accumulate)


def counting_engine(calls):
    """The numpy engine, recording the channel list of every distances call in ``calls``."""
    def distances(g, q, t0, t1, channels=None):
        calls.append(None if channels is None else list(channels))
        return chan_l2_dist(g, q, t0, t1, channels)
    return (distances, _np_select, chan_l2_accumulate)


# ---- the reference loop, naively ----------------------------------------------------------------------------------------
def flat_features(eeg_nct, t0, t1, channels):
    """The feature the reference searches with for a channel subset: per recording the window of the chosen channels,
    laid out time-major ([Tw, m+1], channels in the order given) and flattened -> [N, Tw * (m+1)] float64."""
    x = np.asarray(eeg_nct, dtype=np.float64)[:, list(channels), t0:t1]          # [N, m+1, Tw]
    return np.ascontiguousarray(x.transpose(0, 2, 1)).reshape(x.shape[0], -1)


def naive_discover(gallery_nct, query_nct, gallery_labels, query_labels, class_id_to_str, topK=5, time_low=20,
                   time_high=480, start=(), max_channels=None, search=None, fold=None):
    """The reference's greedy loop with nothing shared between candidates or rounds: every candidate gets its own flat
    feature, its own search and its own bookkeeping.  The rule is the reference's: ONE table of scores is carried across
    all rounds, keyed by the whole channel subset; after a round the table is scanned in insertion order for the first
    score strictly above everything before it (starting from 0); if the subset found ends in a channel that is already
    fixed -- an entry of an earlier round still leads -- or nothing is above 0, discovery stops, otherwise that channel
    is fixed.  ``start``, ``max_channels`` and the stop without candidates are the driver's additions.
    -> (order, rounds, stopped, top1) as ``discover_channels`` returns them.  ``search(g, q, k) -> (D, I)`` and
    ``fold(I, gallery_labels, query_labels, topK) -> (recall, precision, _, top1)`` default to the oracle's; the GPU test
    passes the product's own search and bookkeeping for the brute-force form."""
    from cerebralsignalnetworks_amd import channel_discovery as cd
    search = search or oracle_retrieval.l2_topk
    fold = fold or (lambda I, gl, ql, k: oracle_retrieval.evaluate_from_indices(I, gl, ql, class_id_to_str, k))
    n_channels = np.asarray(gallery_nct).shape[1]
    fixed = [int(c) for c in start]
    recall_of_subset = {}                       # subset (tuple, in selection order) -> recall; never cleared
    rounds, top1s = [], []
    while True:
        remaining = [c for c in range(n_channels) if c not in fixed]
        if max_channels is not None and len(fixed) >= max_channels:
            return fixed, rounds, cd.STOP_MAX_CHANNELS, top1s
        if not remaining:
            return fixed, rounds, cd.STOP_EXHAUSTED, top1s
        scores, accuracies = {}, {}
        for cand in remaining:
            subset = tuple(fixed) + (cand,)
            _, neighbours = search(flat_features(gallery_nct, time_low, time_high, subset),
                                   flat_features(query_nct, time_low, time_high, subset), topK)
            recall, precision, _, accuracy = fold(neighbours, gallery_labels, query_labels, topK)
            recall_of_subset[subset] = recall
            scores[cand], accuracies[cand] = (recall, precision), accuracy
        rounds.append(scores)
        top1s.append(accuracies)
        leader, leading = None, 0
        for subset, recall in recall_of_subset.items():
            if recall > leading:
                leader, leading = subset, recall
        if leader is None or leader[-1] in fixed:
            return fixed, rounds, cd.STOP_NO_IMPROVEMENT, top1s
        fixed.append(leader[-1])


# ---- problems -----------------------------------------------------------------------------------------------------------
class DS:
    def __init__(self, ncls):
        self.class_id_to_str = {k: f"class_{k}" for k in range(ncls)}
        self.class_str_to_id = {f"class_{k}": k for k in range(ncls)}


def label(k):
    return {"ClassId": int(k), "ClassName": f"class_{int(k)}", "imagenetClassId": str(int(k))}


PLANTED_TOPK = 2


def planted(seed=3, C=6, ncls=4, per_class=6, T=12, informative=((1, 2), (4, 1)), integer=True, n_gallery=None,
            n_query=None):
    """Channel-first recordings [N, C, T] float32 for both sides + label dicts.  ``informative``: (channel, bit) pairs --
    the channel carries an offset of +-2 according to that bit of the class id, so two such channels are needed to tell
    four classes apart; every other channel is noise.  Integer-valued: noise in [-4, 4], values in [-6, 6] (every partial
    sum of squared differences is exact in float64).  Otherwise standard normal noise.  At PLANTED_TOPK = 2 neighbours
    one informative channel is not enough for full recall, so discovery runs several rounds.  Rows: ``per_class`` per class in
    class order, or ``n_gallery`` / ``n_query`` rows with classes drawn at random."""
    rng = np.random.default_rng(seed)
    sides = []
    for n in (n_gallery, n_query):
        cls = np.repeat(np.arange(ncls), per_class) if n is None else rng.integers(0, ncls, n)
        if integer:
            x = rng.integers(-4, 5, (len(cls), C, T)).astype(np.float32)
        else:
            x = rng.standard_normal((len(cls), C, T)).astype(np.float32)
        for ch, bit in informative:
            x[:, ch, :] += (2.0 * (((cls >> (bit - 1)) & 1) * 2 - 1)).astype(np.float32)[:, None]
        sides.append((x, [label(k) for k in cls]))
    (g, gl), (q, ql) = sides
    return g, q, gl, ql, DS(ncls)


def as_tuple(result):
    """(order, rounds, stopped, top1) of a DiscoveryResult or of naive_discover's tuple, comparable with ==."""
    order, rounds, stopped, top1 = tuple(result)[:4]
    return list(order), [dict(r) for r in rounds], stopped, [dict(t) for t in top1]
