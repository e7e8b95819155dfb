"""Stream-order cases of the two retrieval-metrics entry points (csn_topk_merge, csn_topk_class_metrics;
include/csn_hip.h, "Stream contract"); not a test module.

tests/test_gpu_retrieval_metrics.py runs every case below through the procedure of tests/test_gpu_stream_order.py (late
inputs behind a Delay, a snapshot and poison directly behind the call), whatever else is collected.

The cases are named in stream_order.CASE_TABLE by ``register()``, which runs when this module is imported; both
retrieval-metrics test files import it, and pytest imports every test module of the directory before it runs a test, so in
a run of the suite the table covers the header (see tests/channel_discovery_stream_cases.py for what a run of
tests/test_stream_order_cpu.py alone reports)."""
import numpy as np
import torch

import retrieval_metrics_reference as ref
import stream_order as so


def _dev(a, device):
    return torch.from_numpy(np.ascontiguousarray(a)).to(device)


def _topk_merge(P, k_in, k):
    def build(device):
        from cerebralsignalnetworks_amd import cabi
        D, I = ref.merge_case(P, 9, k_in, 31 + P)
        ins = {"D_parts": _dev(D, device), "I_parts": _dev(I, device)}
        return ins, lambda a: cabi.topk_merge(a["D_parts"], a["I_parts"], k)
    return build


def _topk_class_metrics(device):
    from cerebralsignalnetworks_amd import cabi
    # classes 1 .. 3: the poison of integer inputs is 0, a class (and a gallery row) of its own
    r = np.random.default_rng(32)
    ins = {"idx": _dev(r.integers(1, 300, (70, 5)), device),
           "gallery_class": _dev(r.integers(1, 4, 300).astype(np.int32), device),
           "query_class": _dev(r.integers(1, 4, 70).astype(np.int32), device)}
    return ins, lambda a: cabi.topk_class_metrics(a["idx"], a["gallery_class"], a["query_class"], 4)


CASES = {
    # candidates of a query staged in LDS, and more of them than the 2048 that are
    "csn_topk_merge": [so.Stateless("csn_topk_merge", "staged_p3_kin20", _topk_merge(3, 20, 12)),
                       so.Stateless("csn_topk_merge", "unstaged_p33_kin64", _topk_merge(33, 64, 12))],
    "csn_topk_class_metrics": [so.Stateless("csn_topk_class_metrics", "nq70_k5", _topk_class_metrics)],
}


def register():
    """Names CASES in stream_order.CASE_TABLE; a second call changes nothing."""
    for name, cases in CASES.items():
        so.CASE_TABLE.setdefault(name, cases)


register()
