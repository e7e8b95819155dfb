"""Stream-order cases of csn_grad_guard and of the three guarded optimiser steps (include/csn_hip.h, "Stream contract");
not a test module.

tests/test_gpu_grad_guard.py runs every case below through the procedure of tests/test_gpu_stream_order.py (late inputs
behind a Delay, a snapshot and poison directly behind the call), whatever else is collected.  A guarded step's case is the
pair a caller enqueues -- the guard over the late gradient, then the step behind its record -- so a guard that ran early
would read the poison (NaN), say "non-finite", and the step would write nothing.

tests/stream_order.py keeps CASE_TABLE, the table of every entry point that takes a csnStream_t, and
tests/test_stream_order_cpu.py holds that table against the header.  The cases here are named in the table by
``register()``, which runs when this module is imported; both gradient-guard test files import it, and pytest imports
every test module of the directory before it runs a test, so in a run of the suite the table covers the header.  A run of
tests/test_stream_order_cpu.py ALONE does not import this module and reports the four entry points as uncovered: name one
of the two gradient-guard test files beside it."""
import torch

import stream_order as so

MAX_NORM = 30.0             # the gradient of so._flat_buffers has a norm of about 70: the clip is active


def _guard(device):
    from cerebralsignalnetworks_amd import cabi
    ins = so._flat_buffers(device, ("grads",), 31)

    def call(a):
        guard = cabi.StepGuard(device)
        guard.measure(a["grads"], MAX_NORM)
        return {"record": guard.record}
    return ins, call


def _rmsprop(device):
    from cerebralsignalnetworks_amd import cabi
    ins = so._flat_buffers(device, ("params", "grads", "square_avg"), 32)

    def call(a):
        guard = cabi.StepGuard(device)
        guard.measure(a["grads"], MAX_NORM)
        cabi.rmsprop_step_guarded(guard, a["params"], a["grads"], a["square_avg"], 1e-2)
        return {"params": a["params"], "square_avg": a["square_avg"], "record": guard.record}
    return ins, call


def _adam(device):
    from cerebralsignalnetworks_amd import cabi
    t = so._table(device)
    ins = so._flat_buffers(device, ("params", "grads", "exp_avg", "exp_avg_sq"), 33)

    def call(a):
        guard = cabi.StepGuard(device)
        norms = torch.zeros(t.nseg, dtype=torch.float32, device=device)
        guard.measure(a["grads"], MAX_NORM)
        cabi.adam_step_guarded(guard, t, a["params"], a["grads"], a["exp_avg"], a["exp_avg_sq"], 3, 1e-3, 0.9, 0.999, 1e-8,
                               0.01, True, clip=3.0, norms_out=norms)
        return {"params": a["params"], "exp_avg": a["exp_avg"], "exp_avg_sq": a["exp_avg_sq"], "norms": norms,
                "record": guard.record}
    return ins, call


def _lars(device):
    from cerebralsignalnetworks_amd import cabi
    t = so._table(device)
    ins = so._flat_buffers(device, ("params", "grads", "mu"), 34)

    def call(a):
        guard = cabi.StepGuard(device)
        guard.measure(a["grads"], MAX_NORM)
        cabi.lars_step_guarded(guard, t, a["params"], a["grads"], a["mu"], 0.2, 1e-6, 0.9, 0.001)
        return {"params": a["params"], "mu": a["mu"], "record": guard.record}
    return ins, call


CASES = {
    "csn_grad_guard": [so.Stateless("csn_grad_guard", "n5000", _guard)],
    "csn_rmsprop_step_guarded": [so.Stateless("csn_rmsprop_step_guarded", "guard_then_step_n5000", _rmsprop)],
    "csn_adam_step_guarded": [so.Stateless("csn_adam_step_guarded", "guard_then_adamw_clip", _adam)],
    "csn_lars_step_guarded": [so.Stateless("csn_lars_step_guarded", "guard_then_step_3seg", _lars)],
}


def register():
    """Names CASES in stream_order.CASE_TABLE; a second call changes nothing."""
    for name, cases in CASES.items():
        so.CASE_TABLE.setdefault(name, cases)


register()
