"""Stream-order cases of csn_distill_loss and csn_dino_loss (include/csn_hip.h, "Stream contract"); not a test module.

tests/test_gpu_distill_loss.py runs every case below through the procedure of tests/test_gpu_stream_order.py (late inputs
behind a Delay, a snapshot and poison directly behind the call), whatever else is collected.

tests/stream_order.py keeps CASE_TABLE, the table of every entry point that takes a csnStream_t, and
tests/test_stream_order_cpu.py holds that table against the header.  The cases here are named in the table by
``register()``, which runs when this module is imported; both distillation-loss test files import it, and pytest imports
every test module of the directory before it runs a test, so in a run of the suite the table covers the header.  A run of
tests/test_stream_order_cpu.py ALONE does not import this module and reports the two entry points as uncovered: name one
of the two distillation-loss test files beside it."""
import numpy as np
import torch

import stream_order as so


def _dev(a, device):
    return torch.from_numpy(np.ascontiguousarray(a)).to(device)


def _distill(device):
    from cerebralsignalnetworks_amd import cabi
    r = np.random.default_rng(26)
    # labels 1 .. 6: the poison of integer inputs is 0, a valid label (nothing is read out of range while it is there)
    ins = {"student": _dev(r.standard_normal((6, 33)).astype(np.float32), device),
           "teacher": _dev(r.standard_normal((6, 33)).astype(np.float32), device),
           "logits": _dev(r.standard_normal((6, 7)).astype(np.float32), device),
           "labels": _dev(r.integers(1, 7, 6).astype(np.int64), device)}

    def call(a):
        loss, ds, dl = cabi.distill_loss(a["student"], a["teacher"], cabi.SOFT_CE_OF_PROBS, 0.22, 0.5, logits=a["logits"],
                                         labels=a["labels"], w_ce=0.5, grad_scale=0.5)
        return {"loss": loss, "dstudent": ds, "dlogits": dl}
    return ins, call


def _dino(device):
    from cerebralsignalnetworks_amd import cabi
    r = np.random.default_rng(27)
    ins = {"student": _dev(r.standard_normal((3, 5, 33)).astype(np.float32), device),
           "teacher": _dev(r.standard_normal((2, 5, 33)).astype(np.float32), device),
           "center": _dev(0.1 * r.standard_normal((5, 33)).astype(np.float32), device)}

    def call(a):
        loss, ds = cabi.dino_loss(a["student"], a["teacher"], a["center"], 0.04, 0.1, cabi.DINO_SKIP_SAME, grad_scale=0.5)
        return {"loss": loss, "dstudent": ds}
    return ins, call


CASES = {
    "csn_distill_loss": [so.Stateless("csn_distill_loss", "featdist_b6_d33_k7", _distill)],
    "csn_dino_loss": [so.Stateless("csn_dino_loss", "v3_g2_b5_d33", _dino)],
}


def register():
    """Names CASES in stream_order.CASE_TABLE; a second call changes nothing."""
    for name, cases in CASES.items():
        so.CASE_TABLE.setdefault(name, cases)


register()
