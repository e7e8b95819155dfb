"""Stream-order cases of csn_bank_norms and csn_bank_contrastive (include/csn_hip.h, "Stream contract"); not a test module.

tests/test_gpu_bank_contrastive.py runs every case below through the procedure of tests/test_gpu_stream_order.py (late
inputs behind a Delay, a snapshot and poison directly behind the call), whatever else is collected.

tests/stream_order.py keeps CASE_TABLE, the table of every entry point that takes a csnStream_t, and
tests/test_stream_order_cpu.py holds that table against the header.  The cases here are named in the table by
``register()``, which runs when this module is imported; both bank-contrastive test files import it, and pytest imports every
test module of the directory before it runs a test, so in a run of the suite the table covers the header.  A run of
tests/test_stream_order_cpu.py ALONE does not import this module and reports the two entry points as uncovered: name one of
the two bank-contrastive test files beside it."""
import numpy as np
import torch

import stream_order as so

B, M, D = 76, 150, 70           # two row tiles, three key tiles, three splits of the ds contraction, a ragged D
SCALE = 1.0 / 0.07


def _dev(a, device):
    return torch.from_numpy(np.ascontiguousarray(a)).to(device)


def _inputs(seed):
    r = np.random.default_rng(seed)
    bank = r.standard_normal((M, D)).astype(np.float32)
    pos = r.integers(0, M, size=B).astype(np.int32)
    s = (0.5 * bank[pos] + r.standard_normal((B, D))).astype(np.float32)
    g = r.integers(0, M // 3, size=M).astype(np.int32)
    return s, bank, g, pos


def _norms(device):
    from cerebralsignalnetworks_amd import cabi
    _, bank, _, _ = _inputs(51)
    ins = {"bank": _dev(bank, device)}

    def call(a):
        return {"inv_norm": cabi.bank_norms(a["bank"])}
    return ins, call


def _loss(device):
    from cerebralsignalnetworks_amd import cabi
    import bank_contrastive_reference as ref
    s, bank, g, pos = _inputs(52)
    ins = {"s": _dev(s, device), "bank": _dev(bank, device), "bank_inv_norm": _dev(ref.bank_norms(bank), device),
           "bank_group": _dev(g, device), "pos": _dev(pos, device)}

    def call(a):
        rows, loss, ds, dscale = cabi.bank_contrastive(a["s"], a["bank"], a["bank_inv_norm"], a["pos"], SCALE, a["bank_group"],
                                                       inv_rows=1.0 / 152, grad_scale=3.0, want_dscale=True)
        return {"rows_out": rows, "loss_part": loss, "ds": ds, "dscale_part": dscale}
    return ins, call


CASES = {
    "csn_bank_norms": [so.Stateless("csn_bank_norms", "m150_d70", _norms)],
    "csn_bank_contrastive": [so.Stateless("csn_bank_contrastive", "b76_m150_d70_groups_ds_dscale", _loss)],
}


def register():
    """Names CASES in stream_order.CASE_TABLE; a second call changes nothing."""
    for name, cases in CASES.items():
        so.CASE_TABLE.setdefault(name, cases)


register()
