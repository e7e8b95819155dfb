"""Stream-order cases of the three channel-discovery entry points (csn_chan_l2_dist, csn_chan_l2_select,
csn_chan_l2_accumulate; include/csn_hip.h, "Stream contract"); not a test module.

tests/test_gpu_channel_discovery.py runs every case below through the procedure of tests/test_gpu_stream_order.py (late
inputs behind a Delay, a snapshot and poison directly behind the call), whatever else is collected.

tests/stream_order.py keeps CASE_TABLE, the table of every entry point that takes a csnStream_t, and
tests/test_stream_order_cpu.py holds that table against the header.  The cases here are named in the table by
``register()``, which runs when this module is imported; both channel-discovery test files import it, and pytest imports
every test module of the directory before it runs a test, so in a run of the suite the table covers the header.  The
parametrised cases of tests/test_gpu_stream_order.py are not touched.  A run of tests/test_stream_order_cpu.py ALONE
does not import this module and reports the three entry points as uncovered: name one of the two channel-discovery test
files beside it."""
import numpy as np
import torch

import stream_order as so


def _dev(a, device):
    return torch.from_numpy(np.ascontiguousarray(a)).to(device)


def _chan_l2_dist(device):
    from cerebralsignalnetworks_amd import cabi
    r = np.random.default_rng(23)
    ins = {"gallery": _dev(r.standard_normal((70, 3, 21)).astype(np.float32), device),
           "query": _dev(r.standard_normal((9, 3, 21)).astype(np.float32), device)}
    return ins, lambda a: {"Dc": cabi.chan_l2_dist(a["gallery"], a["query"], 2, 19, [2, 0])}


def _chan_l2_select(Ng):
    def build(device):
        from cerebralsignalnetworks_amd import cabi
        r = np.random.default_rng(24 + Ng)
        # classes 1 .. 3: the poison of integer inputs is 0, a class of its own
        ins = {"base": _dev(r.integers(0, 5, (9, Ng)).astype(np.float64), device),
               "Dc": _dev(r.integers(0, 5, (3, 9, Ng)).astype(np.float64), device),
               "gallery_class": _dev(r.integers(1, 4, Ng).astype(np.int32), device),
               "query_class": _dev(r.integers(1, 4, 9).astype(np.int32), device)}
        return ins, lambda a: cabi.chan_l2_select(a["base"], a["Dc"], a["gallery_class"], a["query_class"], 5)
    return build


def _chan_l2_accumulate(device):
    from cerebralsignalnetworks_amd import cabi
    r = np.random.default_rng(25)
    ins = {"base": _dev(r.standard_normal(5000), device), "one": _dev(r.standard_normal(5000), device)}
    return ins, lambda a: {"base": cabi.chan_l2_accumulate(a["base"], a["one"], False)}


CASES = {
    "csn_chan_l2_dist": [so.Stateless("csn_chan_l2_dist", "ng70_c3_w2-19", _chan_l2_dist)],
    # a row staged in LDS, and one longer than the 2048 entries that are
    "csn_chan_l2_select": [so.Stateless("csn_chan_l2_select", "staged_ng300", _chan_l2_select(300)),
                           so.Stateless("csn_chan_l2_select", "unstaged_ng2100", _chan_l2_select(2100))],
    "csn_chan_l2_accumulate": [so.Stateless("csn_chan_l2_accumulate", "n5000", _chan_l2_accumulate)],
}


def register():
    """Names CASES in stream_order.CASE_TABLE; a second call changes nothing."""
    for name, cases in CASES.items():
        so.CASE_TABLE.setdefault(name, cases)


register()
