"""GPU: the recurrence launches and cells the library reports for the per-diagonal (path 1) and the CU-resident (path 5)
wavefront are those of tests/wavefront_model.py -- the model tests/test_wavefront_schedule_cpu.py holds
csn::wavefront_schedule (csrc/lstm_schedule.h) to.  T 11 at L 5 under CSN_LSTM_CHUNK = 2 reaches the diagonals with more
than four layers in range, which take a second launch, on both paths."""
import pytest
import torch

import lstm_feature_fuzz as fz
import test_gpu_lstm_feature_fuzz as ff
import test_gpu_lstm_resident as tr
import wavefront_model as wm
from cerebralsignalnetworks_amd import cabi

pytestmark = pytest.mark.gpu

B, T, I, H = 8, 11, 16, 128


@pytest.mark.parametrize("chunk", [2, 4])
@pytest.mark.parametrize("L", [2, 5])
@pytest.mark.parametrize("path", [1, 5])
def test_profile_counts_are_the_models(path, L, chunk):
    c = tr._record(B, T, I, H, L, "bf16")
    a = fz.make_inputs(c)
    w = ff._weights(a, L)
    kw = dict(training=True, state=True)
    with tr._env(CSN_LSTM_CHUNK=str(chunk)):
        if path == 5:
            plan = cabi.LstmPlan(B, T, I, H, L, tr.BF16, tr.DEV, resident=True, **kw)
        else:
            with tr._env(CSN_NO_PERSIST="1"):
                plan = cabi.LstmPlan(B, T, I, H, L, tr.BF16, tr.DEV, **kw)
    assert plan.path() == path, ff._triple(plan)
    plan.profile_enable(True)
    ff._featured(plan, c, w, a)
    torch.cuda.synchronize()
    p = plan.profile_read()
    pair = ("forward_resident", "backward_resident") if path == 5 else ("forward_il", "backward_il")
    want = [n for v in pair for n in wm.counts(v, T, L, chunk)]
    assert [p["fwd_launches"], p["fwd_cells"], p["bwd_launches"], p["bwd_cells"]] == want, (p, want)
    assert plan.status() == 0
