"""Stream-order cases of csn_contrastive_lse and csn_contrastive_grad (include/csn_hip.h, "Stream contract"); not a test module.

tests/test_gpu_contrastive_loss.py runs every case below through the procedure of tests/test_gpu_stream_order.py (late
inputs behind a Delay, a snapshot and poison directly behind the call), whatever else is collected.

tests/stream_order.py keeps CASE_TABLE, the table of every entry point that takes a csnStream_t, and
tests/test_stream_order_cpu.py holds that table against the header.  The cases here are named in the table by
``register()``, which runs when this module is imported; both contrastive-loss test files import it, and pytest imports every
test module of the directory before it runs a test, so in a run of the suite the table covers the header.  A run of
tests/test_stream_order_cpu.py ALONE does not import this module and reports the two entry points as uncovered: name one of
the two contrastive-loss test files beside it."""
import numpy as np
import torch

import stream_order as so

N, D, ROW0, B = 150, 70, 37, 76         # the middle rank of uneven emulated shards: three key tiles, two row tiles, a ragged D
SCALE = 1.0 / 0.07


def _dev(a, device):
    return torch.from_numpy(np.ascontiguousarray(a)).to(device)


def _inputs(seed):
    r = np.random.default_rng(seed)
    s = r.standard_normal((N, D)).astype(np.float32)
    t = (0.5 * s + r.standard_normal((N, D))).astype(np.float32)
    g = r.integers(0, N // 2, size=N).astype(np.int32)
    return s, t, g


def _lse(device):
    from cerebralsignalnetworks_amd import cabi
    s, t, g = _inputs(41)
    ins = {"s_all": _dev(s, device), "t_all": _dev(t, device), "group_all": _dev(g, device)}

    def call(a):
        rows, loss = cabi.contrastive_lse(a["s_all"], a["t_all"], SCALE, a["group_all"], ROW0, B)
        return {"rows_out": rows, "loss_part": loss}
    return ins, call


def _grad(device):
    from cerebralsignalnetworks_amd import cabi
    import contrastive_loss_reference as ref
    s, t, g = _inputs(42)
    rows, _ = ref.contrastive_lse(s, t, g, 0, N, SCALE)
    ins = {"s_all": _dev(s, device), "t_all": _dev(t, device), "group_all": _dev(g, device),
           "lse_a_local": _dev(rows[0, ROW0:ROW0 + B], device), "lse_b_all": _dev(rows[1], device)}

    def call(a):
        ds, dscale = cabi.contrastive_grad(a["s_all"], a["t_all"], SCALE, a["lse_a_local"], a["lse_b_all"], a["group_all"], ROW0, B,
                                           grad_scale=3.0, want_dscale=True)
        return {"ds": ds, "dscale_part": dscale}
    return ins, call


CASES = {
    "csn_contrastive_lse": [so.Stateless("csn_contrastive_lse", "n150_d70_groups", _lse)],
    "csn_contrastive_grad": [so.Stateless("csn_contrastive_grad", "n150_d70_dscale", _grad)],
}


def register():
    """Names CASES in stream_order.CASE_TABLE; a second call changes nothing."""
    for name, cases in CASES.items():
        so.CASE_TABLE.setdefault(name, cases)


register()
