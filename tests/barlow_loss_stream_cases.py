"""Stream-order cases of csn_barlow_corr and csn_barlow_grad (include/csn_hip.h, "Stream contract"); not a test module.

tests/test_gpu_barlow_loss.py runs every case below through the procedure of tests/test_gpu_stream_order.py (late inputs
behind a Delay, a snapshot and poison directly behind the call), whatever else is collected.

tests/stream_order.py keeps CASE_TABLE, the table of every entry point that takes a csnStream_t, and
tests/test_stream_order_cpu.py holds that table against the header.  The cases here are named in the table by
``register()``, which runs when this module is imported; both Barlow-loss test files import it, and pytest imports every
test module of the directory before it runs a test, so in a run of the suite the table covers the header.  A run of
tests/test_stream_order_cpu.py ALONE does not import this module and reports the two entry points as uncovered: name one
of the two Barlow-loss test files beside it."""
import numpy as np
import torch

import stream_order as so

B, D, BATCH = 37, 70, 74            # one rank of two: more than one tile column, a ragged slice of the summed dimensions


def _dev(a, device):
    return torch.from_numpy(np.ascontiguousarray(a)).to(device)


def _inputs(seed):
    r = np.random.default_rng(seed)
    return r.standard_normal((B, D)).astype(np.float32), r.standard_normal((B, D)).astype(np.float32)


def _corr(device):
    from cerebralsignalnetworks_amd import cabi
    z1, z2 = _inputs(28)
    r = np.random.default_rng(29)
    ins = {"z1": _dev(z1, device), "z2": _dev(z2, device),
           "running_mean": _dev(r.standard_normal(D).astype(np.float32), device),
           "running_var": _dev((1.0 + r.random(D)).astype(np.float32), device)}

    def call(a):
        c, saved = cabi.barlow_corr(a["z1"], a["z2"], BATCH, running_mean=a["running_mean"], running_var=a["running_var"],
                                    momentum=0.1)
        return {"c": c, "saved": saved, "running_mean": a["running_mean"], "running_var": a["running_var"]}
    return ins, call


def _grad(device):
    from cerebralsignalnetworks_amd import cabi
    import barlow_loss_reference as ref
    z1, z2 = _inputs(30)
    o1, o2 = _inputs(31)            # the other rank's rows
    c_local, saved, _ = ref.barlow_corr(z1, z2, 1.0 / BATCH)
    c = c_local + ref.barlow_corr(o1, o2, 1.0 / BATCH)[0]
    ins = {"z1": _dev(z1, device), "z2": _dev(z2, device), "c": _dev(c, device), "c_local": _dev(c_local, device),
           "saved": _dev(saved, device)}

    def call(a):
        loss, dz1, dz2 = cabi.barlow_grad(a["z1"], a["z2"], a["c"], a["c_local"], a["saved"], BATCH, 0.0051, grad_scale=0.5)
        return {"loss": loss, "dz1": dz1, "dz2": dz2}
    return ins, call


CASES = {
    "csn_barlow_corr": [so.Stateless("csn_barlow_corr", "b37_d70_running", _corr)],
    "csn_barlow_grad": [so.Stateless("csn_barlow_grad", "b37_d70_two_ranks", _grad)],
}


def register():
    """Names CASES in stream_order.CASE_TABLE; a second call changes nothing."""
    for name, cases in CASES.items():
        so.CASE_TABLE.setdefault(name, cases)


register()
