"""CPU: the host side of gradient accumulation -- csn_lstm_plan_set_grad_mode in the header, the library and the
binding (ABI still 6), its host-side argument checks, and DistillTrainer's accum_steps validation."""
import ctypes
import os
import re

import pytest
import torch

from cerebralsignalnetworks_amd import cabi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _header():
    with open(os.path.join(ROOT, "include", "csn_hip.h")) as f:
        return f.read()


def test_set_grad_mode_is_declared_exported_and_bound():
    h = _header()
    assert re.search(r"\bint\s+csn_lstm_plan_set_grad_mode\s*\(\s*csnLstmPlan\s*\*\s*plan\s*,\s*int\s+mode\s*\)\s*;", h)
    assert re.search(r"#define\s+CSN_GRAD_OVERWRITE\s+0\b", h) and re.search(r"#define\s+CSN_GRAD_ACCUMULATE\s+1\b", h)
    assert re.search(r"#define\s+CSN_ABI_VERSION\s+6\b", h)
    assert cabi.SIGNATURES["csn_lstm_plan_set_grad_mode"] == (ctypes.c_int, [ctypes.c_void_p, ctypes.c_int])
    assert (cabi.GRAD_OVERWRITE, cabi.GRAD_ACCUMULATE) == (0, 1)
    lib = cabi.load()                                   # raises if a bound symbol is not exported
    assert lib.csn_abi_version() == 6 == cabi.ABI_VERSION
    assert hasattr(cabi.LstmPlan, "set_grad_mode")


@pytest.mark.parametrize("mode", [0, 1, 7])
def test_null_plan_is_refused_on_the_host(mode):
    lib = cabi.load()
    assert lib.csn_lstm_plan_set_grad_mode(None, mode) == 1         # CSN_ERR_INVALID_ARGUMENT
    assert b"null plan" in lib.csn_last_error()


class _CpuModel(torch.nn.Module):
    def __init__(self):
        super().__init__()
        self.fc = torch.nn.Linear(4, 3)

    def forward(self, x):
        return self.fc(x[:, -1])


def test_trainer_refuses_bad_accum_steps_at_construction():
    from cerebralsignalnetworks_amd.trainer import DistillTrainer
    with pytest.raises(ValueError, match="accum_steps"):
        DistillTrainer(_CpuModel(), None, loss="cosine", optimizer="adam", accum_steps=0)
    with pytest.raises(ValueError, match="barlow"):
        DistillTrainer(_CpuModel(), None, loss="barlow", optimizer="lars", accum_steps=2)
    # the accepted forms build on a CPU model without touching a device
    for loss in ("cosine", "featdist", "kd"):
        assert DistillTrainer(_CpuModel(), None, loss=loss, optimizer="adam", accum_steps=2).accum_steps == 2
    assert DistillTrainer(_CpuModel(), None, loss="barlow", optimizer="lars").accum_steps == 1


def test_cli_has_accum_steps():
    import LstmDistillFromDinoV2Train as train
    for flavour in (train.PERILS, train.SPAMPINATO):
        p = train.build_parser(flavour)
        assert p.parse_args([]).accum_steps == 1
        assert p.parse_args(["--accum_steps", "4"]).accum_steps == 4
