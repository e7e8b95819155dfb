"""Retrieval evaluation: exact L2 top-k on the GPU + the reference's Recall/Precision bookkeeping.

``evaluate`` keeps the signature of /root/reference/utils/Utilities.py:28
(``evaluate(FLAGS, gallery_features, query_features, gallery_labels, query_labels, dataset)``
-> ``(Recall_Total, Precision_Total)``); the ``faiss.IndexFlatL2`` add/search of :45-55 is the
HIP kernel ``csn_l2_topk`` or, for k > 64 and large problems, ``csn_l2_topk_tiled`` (same bits).  ``evaluate_full`` additionally returns top-1 accuracy and (D, I).
``evaluate_device`` is the same evaluation with the search result, the merge of sharded lists (``csn_topk_merge``) and the
class-hit counts (``csn_topk_class_metrics``) kept on the device.
"""
import numpy as np
import torch

from . import cabi


MATRIX_SCRATCH_BUDGET = 1 << 30      # bytes of [Nq,Ng] float64 from which on the matrix form (csn_l2_topk) is not used
MATRIX_MAX_K = 64                    # csn_l2_topk's k limit


def _takes_tiled(Ng, Nq, k):
    """csn_l2_topk_tiled where csn_l2_topk cannot serve (k > 64, or a distance matrix of the budget or more), which is
    also where it was measured to be the faster one (32768 x 4096 x 768: 1.7 x at k = 5, 2.3 x at k = 64); csn_l2_topk
    below, where it was the faster one at the one shape measured (2048 x 512 x 768, k = 5: 0.17 against 0.25 ms) --
    DESIGN.md section 13, profiles/l2_topk_tiled_bench.json.  Both return the same bits, so no caller can tell."""
    return k > MATRIX_MAX_K or Ng * Nq * 8 >= MATRIX_SCRATCH_BUDGET


def l2_search(gallery_features, query_features, k, device=None, dist64=False):
    """-> (D[nq,k] squared distances, I[nq,k] int64) as numpy arrays; D is float32, or with ``dist64=True`` the float64
    values the selection ran on (always the tiled kernel).  1 <= k <= min(1024, Ng)."""
    device = device or torch.device("cuda", torch.cuda.current_device())
    g = torch.as_tensor(np.asarray(gallery_features, dtype=np.float32)).reshape(len(gallery_features), -1).to(device)
    q = torch.as_tensor(np.asarray(query_features, dtype=np.float32)).reshape(len(query_features), -1).to(device)
    if dist64:
        _, I, D = cabi.l2_topk_tiled(g, q, k, dist64=True)
    elif _takes_tiled(g.shape[0], q.shape[0], k):
        D, I = cabi.l2_topk_tiled(g, q, k)
    else:
        D, I = cabi.l2_topk(g, q, k)
    return D.cpu().numpy(), I.cpu().numpy()


def merge_topk(D_parts, I_parts, k):
    """Exact merge of candidate lists: D_parts / I_parts are sequences of [nq, k_p] arrays (float64 distances, int64
    indices into one common numbering); -> (D[nq,k] float64, I[nq,k] int64), the k smallest under (distance, index),
    ascending.  Padding entries (+inf, -1) are dropped; every query must have at least k real candidates."""
    D = np.concatenate([np.asarray(d, dtype=np.float64).reshape(len(d), -1) for d in D_parts], axis=1)
    I = np.concatenate([np.asarray(i, dtype=np.int64).reshape(len(i), -1) for i in I_parts], axis=1)
    if D.shape != I.shape:
        raise ValueError(f"merge_topk: distances {D.shape} and indices {I.shape} differ in shape")
    pad = I < 0
    if D.shape[1] < k or ((~pad).sum(axis=1) < k).any():
        raise ValueError(f"merge_topk: fewer than k={k} candidates for a query")
    Dk = np.where(pad, np.inf, D)
    Ik = np.where(pad, np.iinfo(np.int64).max, I)          # padding sorts behind every real entry, whatever its distance
    Dout, Iout = np.empty((len(D), k), np.float64), np.empty((len(D), k), np.int64)
    for r in range(len(D)):
        o = np.lexsort((Ik[r], Dk[r]))[:k]
        Dout[r], Iout[r] = D[r, o], I[r, o]
    return Dout, Iout


def _bookkeeping(I, gallery_labels, query_labels, class_id_to_str, class_str_to_id, topK):
    class_scores = {}
    top1 = 0
    for query_idx, search_res in enumerate(I):
        test_label = query_labels[query_idx]
        test_strlabel = class_id_to_str[test_label["ClassId"]]
        name = test_label["ClassName"]
        if name not in class_scores:
            class_scores[name] = {"TP": 0, "classIntanceRetrival": 0, "TotalRetrival": 0, "TotalClass": 0,
                                  "GroundTruths": [], "Predicted": [], "Recall": "", "Precision": ""}
        labels_str = [class_id_to_str[gallery_labels[int(g)]["ClassId"]] for g in search_res]
        count = sum(1 for s in labels_str if s == test_strlabel)
        rec = class_scores[name]
        if name in labels_str:
            rec["TP"] += 1
            rec["classIntanceRetrival"] += count
            rec["Predicted"].append(test_label["ClassId"])
        else:
            rec["Predicted"].append(class_str_to_id[labels_str[0]])
        rec["TotalRetrival"] += topK
        rec["TotalClass"] += 1
        rec["GroundTruths"].append(test_label["ClassId"])
        rec["Recall"] = round((rec["TP"] * 100) / rec["TotalClass"], 2)
        rec["Precision"] = round((rec["classIntanceRetrival"] * 100) / rec["TotalRetrival"], 2)
        top1 += int(gallery_labels[int(search_res[0])]["ClassId"] == test_label["ClassId"])
    recall = float(np.array([v["Recall"] for v in class_scores.values()]).mean())
    precision = float(np.array([v["Precision"] for v in class_scores.values()]).mean())
    return recall, precision, class_scores, top1 / max(1, len(I))


def evaluate_full(FLAGS, gallery_features, query_features, gallery_labels, query_labels, dataset):
    topK = FLAGS.topK
    D, I = l2_search(gallery_features, query_features, topK)
    recall, precision, scores, top1 = _bookkeeping(I, gallery_labels, query_labels, dataset.class_id_to_str,
                                                   dataset.class_str_to_id, topK)
    return dict(Recall_Total=recall, Precision_Total=precision, class_scores=scores, top1=top1, D=D, I=I)


def evaluate(FLAGS, gallery_features, query_features, gallery_labels, query_labels, dataset):
    r = evaluate_full(FLAGS, gallery_features, query_features, gallery_labels, query_labels, dataset)
    print(f"Overall Recall :{r['Recall_Total']} Overall Precision: {r['Precision_Total']}")
    return r["Recall_Total"], r["Precision_Total"]


# ---- the device form: search, merge and class hits stay on the GPU; the host folds a few hundred bytes of integers -------
MAX_CLASSES = 65536                  # csn_topk_class_metrics' n_classes limit


def _host(x):
    return x.cpu().numpy() if isinstance(x, torch.Tensor) else np.asarray(x)


def _dev(x, dtype):
    t = x if isinstance(x, torch.Tensor) else torch.as_tensor(np.asarray(x))
    if not t.is_cuda:
        t = t.to(torch.device("cuda", torch.cuda.current_device()))
    return (t if t.dtype == dtype else t.to(dtype)).contiguous()


def _features_dev(x):
    """Device float32 [N, D]: a device tensor is used in place, anything ``l2_search`` takes is uploaded."""
    if isinstance(x, torch.Tensor) and x.is_cuda:
        return x.float().reshape(len(x), -1).contiguous()
    return _dev(np.asarray(x, dtype=np.float32).reshape(len(x), -1), torch.float32)


def l2_search_device(gallery, query, k, dist64=False):
    """``l2_search`` on device float32 tensors [Ng, D] / [Nq, D], without the host round trip: -> (D[nq,k], I[nq,k] int64)
    as device tensors on the inputs' device, the kernel chosen by the same ``_takes_tiled`` rule and D float32, or with
    ``dist64=True`` the float64 values of the tiled kernel."""
    if not (isinstance(gallery, torch.Tensor) and isinstance(query, torch.Tensor) and gallery.is_cuda and query.is_cuda):
        raise cabi.CsnError("l2_search_device needs device tensors (l2_search takes host arrays)")
    g = gallery.float().reshape(len(gallery), -1)
    q = query.float().reshape(len(query), -1)
    if dist64:
        _, I, D = cabi.l2_topk_tiled(g, q, k, dist64=True)
    elif _takes_tiled(g.shape[0], q.shape[0], k):
        D, I = cabi.l2_topk_tiled(g, q, k)
    else:
        D, I = cabi.l2_topk(g, q, k)
    return D, I


def merge_topk_device(D_parts, I_parts, k):
    """``merge_topk`` on the device (``csn_topk_merge``): D_parts / I_parts are [P, nq, k_in] (float64, int64; device
    tensors are used in place, host arrays or sequences of equally wide [nq, k_in] parts are uploaded); -> (D[nq,k]
    float64, I[nq,k] int64) device tensors with ``merge_topk``'s values.  One host check of the result for a query with
    fewer than k real candidates raises ``merge_topk``'s ValueError."""
    def dense(parts, dtype):
        if not isinstance(parts, (torch.Tensor, np.ndarray)):
            parts = torch.stack([torch.as_tensor(p) for p in parts]) if isinstance(parts[0], torch.Tensor) \
                else np.stack([np.asarray(p) for p in parts])
        return _dev(parts, dtype)
    D, I = dense(D_parts, torch.float64), dense(I_parts, torch.int64)
    if D.shape != I.shape or D.dim() != 3:
        raise ValueError(f"merge_topk: distances {tuple(D.shape)} and indices {tuple(I.shape)} differ in shape")
    if D.shape[0] * D.shape[2] < k:
        raise ValueError(f"merge_topk: fewer than k={k} candidates for a query")
    out = cabi.topk_merge(D, I, k, want=("idx", "dist64"))
    if bool((out["idx"][:, -1] < 0).any()):              # padding fills from the back: the last place tells
        raise ValueError(f"merge_topk: fewer than k={k} candidates for a query")
    return out["dist64"], out["idx"]


def _hip_search(gallery_features, query_features, k):
    return l2_search_device(_features_dev(gallery_features), _features_dev(query_features), k)


def _hip_metrics(I, gallery_class, query_class, n_classes):
    out = cabi.topk_class_metrics(_dev(I, torch.int64), _dev(gallery_class, torch.int32), _dev(query_class, torch.int32),
                                  n_classes, want=("pred", "class", "top1_correct"))
    return {name: t.cpu().numpy() for name, t in out.items()}


HIP_ENGINE = (_hip_search, merge_topk_device, _hip_metrics)


def _fold_counts(out_class, k, class_names, query_class=None, pred=None, top1_correct=None):
    """The floats of ``_bookkeeping`` from ``csn_topk_class_metrics``' integers, pure host arithmetic.  out_class
    [n_classes, 4] int64: per class (TotalClass, TP, classIntanceRetrival, first query index or -1); class_names: the
    ClassName of class id c at ``class_names[c]`` (a dict or a sequence).  -> (Recall_Total, Precision_Total, class_scores,
    top1), the tuple ``_bookkeeping`` returns: classes in order of first appearance among the queries (the order of the
    dict, and of the np.array(...).mean() of both totals: numpy sums pairwise, so another order can move the last bit),
    per class round(TP * 100 / TotalClass, 2) and round(classIntanceRetrival * 100 / (TotalClass * k), 2).  GroundTruths /
    Predicted are filled from query_class / pred ([Nq] class ids) when given, top1 is top1_correct / Nq (None without)."""
    oc = np.asarray(out_class, dtype=np.int64).reshape(-1, 4)
    present = np.nonzero(oc[:, 0] > 0)[0]
    order = present[np.argsort(oc[present, 3], kind="stable")]
    class_scores = {}
    for c in order.tolist():
        total, tp, retrieved = int(oc[c, 0]), int(oc[c, 1]), int(oc[c, 2])
        class_scores[class_names[c]] = {
            "TP": tp, "classIntanceRetrival": retrieved, "TotalRetrival": total * k, "TotalClass": total,
            "GroundTruths": [], "Predicted": [],
            "Recall": round((tp * 100) / total, 2), "Precision": round((retrieved * 100) / (total * k), 2)}
    if query_class is not None and pred is not None:
        qc, pr = np.asarray(query_class).reshape(-1), np.asarray(pred).reshape(-1)
        for c in order.tolist():
            rows = np.nonzero(qc == c)[0]
            class_scores[class_names[c]]["GroundTruths"] = [c] * len(rows)
            class_scores[class_names[c]]["Predicted"] = [int(v) for v in pr[rows]]
    recall = float(np.array([v["Recall"] for v in class_scores.values()]).mean())
    precision = float(np.array([v["Precision"] for v in class_scores.values()]).mean())
    n_queries = int(oc[:, 0].sum())
    top1 = None if top1_correct is None else int(np.asarray(top1_correct).reshape(-1)[0]) / max(1, n_queries)
    return recall, precision, class_scores, top1


def _label_classes(gallery_labels, query_labels, dataset):
    """Class ids of both sides as host int32 arrays (+ the object to hand to the metrics engine: a device tensor stays
    one) and the names of the classes, under ``channel_discovery._class_ids``' precondition: ``class_id_to_str`` is
    injective and agrees with every ClassName, so that ``_bookkeeping``'s string comparisons are comparisons of class ids;
    also ``class_str_to_id`` must map the names of the gallery's classes back (``_bookkeeping``'s Predicted), and the ids
    must be in [0, 65536).  Anything else is a ValueError that names the host form."""
    from .channel_discovery import _class_ids
    id_to_str = dataset.class_id_to_str
    try:
        sides, handles = [], []
        tensors = [isinstance(l, (torch.Tensor, np.ndarray)) for l in (gallery_labels, query_labels)]
        dicts = [[] if t else list(l) for t, l in zip(tensors, (gallery_labels, query_labels))]
        from_dicts = _class_ids(dicts[0], dicts[1], id_to_str)           # (runs the injectivity check on empty lists too)
        for is_tensor, labels, ids in zip(tensors, (gallery_labels, query_labels), from_dicts):
            if is_tensor:
                ids = _host(labels).reshape(-1)
                if ids.dtype.kind not in "iu":
                    raise ValueError(f"class ids must be integers, got {ids.dtype}")
                unknown = sorted(set(np.unique(ids).tolist()) - set(id_to_str))
                if unknown:
                    raise ValueError(f"class ids {unknown[:5]} are not in class_id_to_str")
            if len(ids) and not (0 <= int(ids.min()) and int(ids.max()) < MAX_CLASSES):
                raise ValueError(f"class ids must be in [0, {MAX_CLASSES})")
            sides.append(np.ascontiguousarray(ids, dtype=np.int32))
            handles.append(labels if isinstance(labels, torch.Tensor) and labels.is_cuda else sides[-1])
        for c in np.unique(sides[0]).tolist():
            if dataset.class_str_to_id.get(id_to_str[c]) != c:
                raise ValueError(f"class_str_to_id[{id_to_str[c]!r}] is not {c}")
    except ValueError as e:
        raise ValueError(f"evaluate_device: {e}; the host form (evaluate_full) makes no such assumption") from None
    return sides[0], sides[1], handles[0], handles[1], id_to_str


def _device_metrics(I, classes, topK, metrics):
    """(Recall_Total, Precision_Total, class_scores, top1) of neighbour lists I from ``_label_classes``' result."""
    g_cls, q_cls, g_arg, q_arg, names = classes
    n_classes = int(max(g_cls.max(initial=0), q_cls.max(initial=0))) + 1
    out = metrics(I, g_arg, q_arg, n_classes)
    return _fold_counts(out["class"], topK, names, query_class=q_cls, pred=out["pred"], top1_correct=out["top1_correct"])


def evaluate_device(FLAGS, gallery_features, query_features, gallery_labels, query_labels, dataset, engine=None):
    """``evaluate_full`` without the host round trip: the search (``l2_search_device``) and the per-class hit counts
    (``csn_topk_class_metrics``) run on the device, and ``_fold_counts`` turns [n_classes, 4] integers into the floats
    of ``_bookkeeping``, bit for bit.  -> the dict of ``evaluate_full`` (Recall_Total, Precision_Total, class_scores with
    the same keys, top1, D, I), except that D and I are DEVICE tensors here.

    Features: device tensors (used in place, e.g. what ``DistillTrainer.embed_all`` returns) or anything ``l2_search``
    takes.  Labels: the reference's label dicts, or an integer tensor / array of class ids (names from
    ``dataset.class_id_to_str``).  Precondition (``channel_discovery._class_ids``): ``dataset.class_id_to_str`` is
    injective and agrees with every ClassName; otherwise a ValueError names ``evaluate_full`` -- there is no silent
    fall-back.  ``engine``: a (search, merge, metrics) triple, default the HIP one; tests inject a numpy one."""
    search, _, metrics = engine or HIP_ENGINE
    topK = FLAGS.topK
    classes = _label_classes(gallery_labels, query_labels, dataset)            # refuses before any device work
    D, I = search(gallery_features, query_features, topK)
    recall, precision, scores, top1 = _device_metrics(I, classes, topK, metrics)
    return dict(Recall_Total=recall, Precision_Total=precision, class_scores=scores, top1=top1, D=D, I=I)


def _all_gather_rows(local, group=None):
    """Concatenate row blocks of different lengths from all ranks, in rank order (host tensors: the blocks are
    embeddings / label ids computed once per evaluation, a few MB)."""
    import torch.distributed as dist
    world = dist.get_world_size(group)
    # RCCL moves device tensors only; gloo (CPU tests) host tensors
    dev = torch.device("cuda", torch.cuda.current_device()) if dist.get_backend(group) == "nccl" else torch.device("cpu")
    local = torch.as_tensor(np.asarray(local)).contiguous().to(dev)
    n = torch.tensor([local.shape[0]], dtype=torch.long, device=dev)
    sizes = [torch.zeros(1, dtype=torch.long, device=dev) for _ in range(world)]
    dist.all_gather(sizes, n, group=group)
    sizes = [int(v.item()) for v in sizes]
    pad = torch.zeros((max(sizes),) + tuple(local.shape[1:]), dtype=local.dtype, device=dev)
    pad[:local.shape[0]] = local
    parts = [torch.zeros_like(pad) for _ in range(world)]
    dist.all_gather(parts, pad, group=group)
    return torch.cat([p[:k] for p, k in zip(parts, sizes)]).cpu().numpy(), sizes


def evaluate_distributed(FLAGS, gallery_features, query_features, gallery_labels, query_labels, dataset,
                         search_fn=None, group=None, shard_gallery=False, on_device=False, engine=None):
    """Multi-rank evaluation: every rank holds the embeddings of ITS shard of the gallery
    and of the queries (the pattern of PerilsEEGDataset.py:191-215, where shards are gathered to rank 0).  The
    gallery is all-gathered and kept replicated, every rank searches its own queries against it (csn_l2_topk),
    and the per-query neighbour lists are gathered so that every rank reports the same Recall / Precision / top-1
    as a single-process ``evaluate_full`` over the concatenated data.  Labels are the reference's label dicts.
    ``search_fn(gallery, query, k) -> (D, I)`` defaults to the HIP search.

    ``shard_gallery=True`` keeps the gallery where it is: the queries (the small side) are all-gathered, every rank
    searches all of them against its own shard with k_r = min(topK, shard size), adds its base offset (the row's index in
    the rank-ordered concatenation that the replicated form builds), the candidate lists travel as float64 distances +
    int64 indices padded with (+inf, -1), and every rank merges them exactly (``merge_topk``).  The returned dict is the
    replicated form's.  ``search_fn`` must return float64 distances here (default ``l2_search(..., dist64=True)``): two
    distinct float64 distances can collide in float32, and a float32 merge would order them by index.

    ``on_device=True`` (between ranks only; a single process is ``evaluate_full``, as without it): the candidate lists of
    the sharded gallery are merged by ``csn_topk_merge`` instead of ``merge_topk``, and the metrics come from
    ``csn_topk_class_metrics`` + ``_fold_counts`` instead of ``_bookkeeping`` -- the same floats, under the precondition
    of ``evaluate_device``.  The collectives and the returned dict (numpy ``D`` and ``I``) are the same.  ``engine`` is
    ``evaluate_device``'s (search, merge, metrics) triple; only merge and metrics are used here."""
    import torch.distributed as dist
    if not (dist.is_available() and dist.is_initialized()):
        return evaluate_full(FLAGS, gallery_features, query_features, gallery_labels, query_labels, dataset)
    if on_device:
        _, merge_dev, metrics_dev = engine or HIP_ENGINE
    topK = FLAGS.topK
    by_id = {v["ClassId"]: v for v in list(gallery_labels) + list(query_labels)}
    qry = np.asarray(query_features, dtype=np.float32).reshape(len(query_features), -1)
    if shard_gallery:
        gal_ids, shard_sizes = _all_gather_rows(np.array([l["ClassId"] for l in gallery_labels], dtype=np.int64), group)
        search = search_fn or (lambda g, q, k: l2_search(g, q, k, dist64=True))
        gal = np.asarray(gallery_features, dtype=np.float32).reshape(len(gallery_features), qry.shape[1])
        qry_all, _ = _all_gather_rows(qry, group)
        base = sum(shard_sizes[:dist.get_rank(group)])
        k_r = min(topK, len(gal))
        D_loc = np.full((len(qry_all), topK), np.inf, dtype=np.float64)
        I_loc = np.full((len(qry_all), topK), -1, dtype=np.int64)
        if k_r > 0 and len(qry_all):
            D_r, I_r = search(gal, qry_all, k_r)
            if np.asarray(D_r).dtype != np.float64:
                raise TypeError("evaluate_distributed(shard_gallery=True): search_fn must return float64 distances")
            D_loc[:, :k_r], I_loc[:, :k_r] = D_r, np.asarray(I_r, dtype=np.int64) + base
        world = dist.get_world_size(group)
        D_parts, _ = _all_gather_rows(D_loc, group)
        I_parts, _ = _all_gather_rows(I_loc, group)
        I_dev = None
        if on_device:
            D64, I_dev = merge_dev(D_parts.reshape(world, len(qry_all), topK), I_parts.reshape(world, len(qry_all), topK), topK)
            D64, I_all = _host(D64), _host(I_dev)
        else:
            D64, I_all = merge_topk(D_parts.reshape(world, len(qry_all), topK), I_parts.reshape(world, len(qry_all), topK), topK)
        with np.errstate(over="ignore"):
            D_all = D64.astype(np.float32)          # inf where the float64 distance overflows float32, like out_dist
    else:
        search = search_fn or l2_search
        gal, _ = _all_gather_rows(np.asarray(gallery_features, dtype=np.float32).reshape(len(gallery_features), -1), group)
        gal_ids, _ = _all_gather_rows(np.array([l["ClassId"] for l in gallery_labels], dtype=np.int64), group)
        D_loc, I_loc = search(gal, qry, topK) if len(qry) else (np.zeros((0, topK), np.float32), np.zeros((0, topK), np.int64))
        I_all, _ = _all_gather_rows(np.asarray(I_loc, dtype=np.int64), group)
        D_all, _ = _all_gather_rows(np.asarray(D_loc, dtype=np.float32), group)
        I_dev = None
    q_ids, _ = _all_gather_rows(np.array([l["ClassId"] for l in query_labels], dtype=np.int64), group)
    # label dicts by class id: every rank needs the dict of every class that occurs anywhere
    ids_known = sorted(by_id)
    names = [None] * dist.get_world_size(group)
    dist.all_gather_object(names, {k: by_id[k] for k in ids_known}, group=group)
    for d in names:
        by_id.update(d)
    if on_device:
        classes = _label_classes([by_id[int(k)] for k in gal_ids], [by_id[int(k)] for k in q_ids], dataset)
        recall, precision, scores, top1 = _device_metrics(I_all if I_dev is None else I_dev, classes, topK, metrics_dev)
    else:
        recall, precision, scores, top1 = _bookkeeping(I_all, [by_id[int(k)] for k in gal_ids], [by_id[int(k)] for k in q_ids],
                                                       dataset.class_id_to_str, dataset.class_str_to_id, topK)
    return dict(Recall_Total=recall, Precision_Total=precision, class_scores=scores, top1=top1, D=D_all, I=I_all)
