"""CPU: the host side of the device-side gradient guard (global-norm clip and non-finite step skip).
csn_grad_guard, its scratch size and the three guarded steps are declared, exported and bound (ABI still 6); every argument
violation is refused on the host with CSN_ERR_INVALID_ARGUMENT and a message before anything is launched (a launch on a
machine without a GPU would return CSN_ERR_HIP instead); the Python layer refuses CPU tensors for the HIP calls; and a
DistillTrainer on CPU buffers steps with the torch restatement of the guard: the parameters of a hand-written
clip_grad_norm_ loop, and bit-unchanged parameters on a step whose gradient holds an Inf."""
import ctypes
import os
import re
import types

import pytest
import torch

import __graft_entry__ as graft
import grad_guard_stream_cases as stream_cases
import stream_order as so
from cerebralsignalnetworks_amd import cabi
from cerebralsignalnetworks_amd import FlatAdamW, FlatLARS, flat_clip_grad_norm_
from cerebralsignalnetworks_amd.flat_optim import guard_restatement
from cerebralsignalnetworks_amd.losses import loss_fn_kd
from cerebralsignalnetworks_amd.trainer import DistillTrainer, FlatGrads, FlatRMSprop

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("csn_grad_guard_scratch_bytes", "csn_grad_guard", "csn_rmsprop_step_guarded", "csn_adam_step_guarded",
       "csn_lars_step_guarded")
INVALID = 1                 # CSN_ERR_INVALID_ARGUMENT
OK_PTR = 0x10000            # non-null and 16-byte aligned: never dereferenced, every call below is refused before a launch
ODD_PTR = 0x10004           # 4-byte aligned only
INF = float("inf")


@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(cabi.LIB_PATH):
        graft.build()
    return cabi.load()


def test_new_symbols_are_declared_exported_and_bound(lib):
    text = open(os.path.join(ROOT, "include", "csn_hip.h")).read()
    for name in NEW:
        assert re.search(r"\b(?:int|size_t)\s+%s\s*\(" % name, text), f"{name} is not declared in csn_hip.h"
        assert name in cabi.SIGNATURES
        fn = getattr(lib, name)
        res, args = cabi.SIGNATURES[name]
        assert fn.restype is res and list(fn.argtypes) == list(args)
    assert "#define CSN_ABI_VERSION 6" in text and cabi.ABI_VERSION == 6 and lib.csn_abi_version() == 6
    assert re.search(r"typedef\s+struct\s*\{\s*float\s+norm;\s*float\s+scale;\s*uint32_t\s+finite;\s*uint32_t\s+skipped;\s*\}"
                     r"\s*csnStepGuard\s*;", text)
    # a guarded step takes its unguarded twin's arguments, then the record, then the stream
    for name in ("csn_rmsprop_step", "csn_adam_step", "csn_lars_step"):
        plain, guarded = cabi.SIGNATURES[name], cabi.SIGNATURES[name + "_guarded"]
        assert guarded[0] is plain[0] and list(guarded[1]) == list(plain[1][:-1]) + [ctypes.c_void_p, plain[1][-1]]
    # the declarations cite what they replace, and say what Adam's t counts
    block = text[text.index("Global-norm gradient clipping"):text.index("K7  Barlow")]
    for cite in ("torch.nn.utils.clip_grad_norm_", "LstmDistillation.py:606-613", "skipped calls included"):
        assert cite in block, cite


def test_stream_order_cases_are_registered():
    for name in NEW[1:]:                                # (the four that take a csnStream_t)
        cases = so.CASE_TABLE[name]
        assert cases is stream_cases.CASES[name] and cases
        assert all(isinstance(c, so.Stateless) and c.entry == name and callable(c.build) for c in cases)
    ids = [c.id for v in stream_cases.CASES.values() for c in v]
    assert len(set(ids)) == len(ids) and not set(ids) & {c.id for c in so.STATELESS_CASES}
    n = len(so.CASE_TABLE)
    stream_cases.register()
    assert len(so.CASE_TABLE) == n, "registering twice adds nothing"


def _refused(lib, rc, *words):
    msg = lib.csn_last_error().decode()
    assert rc == INVALID, (rc, msg)
    assert msg and all(w in msg for w in words), msg


def test_scratch_bytes(lib):
    size = lib.csn_grad_guard_scratch_bytes
    for n in (1, 7, 2047, 2048, 2049, 2608, 70001, 2048 * 2048 + 2048 + 5):
        chunks = -(-n // 2048)
        assert chunks * 8 <= size(n) <= chunks * 8 + 16 and size(n) % 16 == 0
    assert size(0) == 0 and b"csn_grad_guard_scratch_bytes" in lib.csn_last_error()
    assert size(-5) == 0


def test_grad_guard_refusals(lib):
    def guard(g=OK_PTR, n=2608, max_norm=1.0, scratch=OK_PTR, rec=OK_PTR):
        return lib.csn_grad_guard(g, n, max_norm, scratch, rec, None)
    for k in ("g", "scratch", "rec"):
        _refused(lib, guard(**{k: None}), "csn_grad_guard", "null")
        _refused(lib, guard(**{k: ODD_PTR}), "csn_grad_guard", "aligned")
    for n in (0, -1):
        _refused(lib, guard(n=n), "csn_grad_guard", "n =")
    for m in (0.0, -1.0, -INF, float("nan")):
        _refused(lib, guard(max_norm=m), "csn_grad_guard", "max_norm")


def test_guarded_step_refusals(lib):
    def rms(p=OK_PTR, g=OK_PTR, v=OK_PTR, n=2608, rec=OK_PTR):
        return lib.csn_rmsprop_step_guarded(p, g, v, n, 1e-3, 0.99, 1e-8, rec, None)
    for k in ("p", "g", "v"):
        _refused(lib, rms(**{k: None}), "csn_rmsprop_step_guarded", "null")
        _refused(lib, rms(**{k: ODD_PTR}), "csn_rmsprop_step_guarded", "aligned")
    _refused(lib, rms(n=0), "csn_rmsprop_step_guarded", "empty")
    _refused(lib, rms(n=-4), "csn_rmsprop_step_guarded", "empty")
    _refused(lib, rms(rec=None), "csn_rmsprop_step_guarded", "null guard", "unguarded")
    _refused(lib, rms(rec=ODD_PTR), "csn_rmsprop_step_guarded", "guard record", "aligned")

    def adam(p=OK_PTR, g=OK_PTR, m=OK_PTR, v=OK_PTR, n=2608, nseg=4, table=OK_PTR, t=1, b1=0.9, b2=0.999, rec=OK_PTR):
        return lib.csn_adam_step_guarded(p, g, m, v, n, nseg, table, t, 1e-3, b1, b2, 1e-8, 1e-2, 1, 0.1, None, rec, None)
    for k in ("p", "g", "m", "v", "table"):
        _refused(lib, adam(**{k: None}), "csn_adam_step_guarded", "null")
        _refused(lib, adam(**{k: ODD_PTR}), "csn_adam_step_guarded", "aligned")
    _refused(lib, adam(nseg=0), "csn_adam_step_guarded", "nseg")
    _refused(lib, adam(n=0), "csn_adam_step_guarded", "n = 0")
    _refused(lib, adam(t=0), "csn_adam_step_guarded", "t must be >= 1")
    _refused(lib, adam(b1=1.0), "csn_adam_step_guarded", "betas")
    _refused(lib, adam(rec=None), "csn_adam_step_guarded", "null guard", "unguarded")
    _refused(lib, adam(rec=ODD_PTR), "csn_adam_step_guarded", "guard record", "aligned")

    def lars(p=OK_PTR, g=OK_PTR, mu=OK_PTR, n=2608, nseg=4, table=OK_PTR, rec=OK_PTR):
        return lib.csn_lars_step_guarded(p, g, mu, n, nseg, table, 0.2, 1e-6, 0.9, 1e-3, rec, None)
    for k in ("p", "g", "mu", "table"):
        _refused(lib, lars(**{k: None}), "csn_lars_step_guarded", "null")
        _refused(lib, lars(**{k: ODD_PTR}), "csn_lars_step_guarded", "aligned")
    _refused(lib, lars(nseg=0), "csn_lars_step_guarded", "nseg")
    _refused(lib, lars(n=-1), "csn_lars_step_guarded", "n = -1")
    _refused(lib, lars(rec=None), "csn_lars_step_guarded", "null guard", "unguarded")
    _refused(lib, lars(rec=ODD_PTR), "csn_lars_step_guarded", "guard record", "aligned")
    # the unguarded entry points still speak under their own names
    _refused(lib, lib.csn_lars_step(None, OK_PTR, OK_PTR, 2608, 4, OK_PTR, 0.2, 1e-6, 0.9, 1e-3, None), "csn_lars_step:", "null")
    _refused(lib, lib.csn_rmsprop_step(None, OK_PTR, OK_PTR, 2608, 1e-3, 0.99, 1e-8, None), "csn_rmsprop_step:", "null")


def _net():
    torch.manual_seed(3)
    return torch.nn.Sequential(torch.nn.Linear(37, 53), torch.nn.Tanh(), torch.nn.Linear(53, 11))


def test_python_layer_refuses_cpu_tensors_and_bad_norms():
    fg = FlatGrads(_net().parameters(), flatten_params=True)
    with pytest.raises(cabi.CsnError):
        cabi.StepGuard("cpu")
    with pytest.raises(cabi.CsnError):
        flat_clip_grad_norm_(fg, 1.0)
    with pytest.raises(cabi.CsnError):
        FlatAdamW(fg, max_grad_norm=1.0)
    with pytest.raises(cabi.CsnError):
        FlatLARS(fg, lr=0.2, skip_nonfinite=True)
    with pytest.raises(cabi.CsnError):
        FlatRMSprop(fg, max_grad_norm=1.0)
    with pytest.raises(cabi.CsnError):
        cabi.rmsprop_step_guarded(None, fg.flat_params, fg.flat, torch.zeros_like(fg.flat), 1e-3)
    for bad in (0, -1.0, float("nan"), True):
        with pytest.raises(ValueError, match="max_grad_norm"):
            DistillTrainer(_CpuModel(), None, loss="cosine", optimizer="adam", max_grad_norm=bad)


class _CpuModel(torch.nn.Module):
    def __init__(self):
        super().__init__()
        self.fc = torch.nn.Linear(4, 3)

    def forward(self, x):
        return self.fc(x[:, -1])


@pytest.mark.parametrize("name", ["adamw", "adam", "lars"])
def test_skip_nonfinite_with_a_torch_optimiser_is_refused(name):
    with pytest.raises(ValueError, match="flat optimiser"):
        DistillTrainer(_CpuModel(), None, loss="cosine", optimizer=name, skip_nonfinite=True)
    # the clip alone builds, and so do both with the optimisers that are flat on a GPU
    assert DistillTrainer(_CpuModel(), None, loss="cosine", optimizer=name, max_grad_norm=1.0).max_grad_norm == 1.0
    assert DistillTrainer(_CpuModel(), None, loss="cosine", optimizer="rmsprop", skip_nonfinite=True).skip_nonfinite is True
    assert DistillTrainer(_CpuModel(), None, loss="cosine", optimizer=name, skip_nonfinite=True,
                          fused_optimizer=True).skip_nonfinite is True


def test_restatement_formulas():
    g = torch.tensor([3.0, -4.0, 0.0, 12.0])                                   # |g| = 13
    norm, scale, finite = guard_restatement(g, 6.5)
    assert norm.dtype == scale.dtype == torch.float32 and bool(finite)
    assert norm.item() == 13.0 and scale.item() == torch.tensor(6.5 / (13.0 + 1e-6), dtype=torch.float64).float().item()
    assert guard_restatement(g, 20.0)[1].item() == 1.0 and guard_restatement(g)[1].item() == 1.0
    assert guard_restatement(torch.zeros(5), 1.0)[1].item() == 1.0             # 1 / 1e-6 clamps to 1
    for bad in (INF, -INF, float("nan")):
        g2 = g.clone()
        g2[2] = bad
        for m in (6.5, None):
            norm, scale, finite = guard_restatement(g2, m)
            assert not bool(finite) and scale.item() == 0.0 and not torch.isfinite(norm)
    # a gradient whose float32 squares overflow is finite in float64: measured, not skipped
    big = torch.full((4,), 3e38)
    norm, scale, finite = guard_restatement(big, 1.0)
    assert bool(finite) and torch.isinf(norm) and 0.0 < scale.item() < 1e-37


KD = types.SimpleNamespace(alpha=0.5, temperature=2.0)         # loss="kd": the one trainer loss that is torch ops on a CPU


def _cpu_data():
    g = torch.Generator().manual_seed(5)
    return torch.randn(6, 5, 4, generator=g), torch.randn(6, 3, generator=g), torch.tensor([0, 2, 1, 1, 0, 2])


def _trainer(model, name="rmsprop", lr=1e-2, **kw):
    return DistillTrainer(model, None, loss="kd", kd_params=KD, lr=lr, optimizer=name, preprocess=False, **kw)


@pytest.mark.parametrize("name,cls,lr", [("rmsprop", torch.optim.RMSprop, 1e-2), ("adamw", torch.optim.AdamW, 1e-2),
                                         ("adam", torch.optim.Adam, 1e-2)])
def test_cpu_trainer_steps_with_the_restatement(name, cls, lr):
    x, tgt, labels = _cpu_data()
    torch.manual_seed(11)
    m, ref = _CpuModel(), _CpuModel()
    ref.load_state_dict(m.state_dict())
    # the unclipped norms of this run decide the bound: the clip must act on some steps and not on others
    probe = _CpuModel()
    probe.load_state_dict(m.state_dict())
    tr0 = _trainer(probe, name, lr, max_grad_norm=INF)
    norms = []
    for _ in range(6):
        tr0.train_step(x.transpose(1, 2), tgt, labels)
        norms.append(tr0.last_grad_norm.item())
    bound = sorted(norms)[len(norms) // 2 - 1] * 0.999 + sorted(norms)[len(norms) // 2] * 0.001
    tr = _trainer(m, name, lr, max_grad_norm=bound)
    assert type(tr.opt) is cls and tr.grads.flat_params is None
    ropt = cls(ref.parameters(), lr=lr)
    clipped = 0
    for _ in range(6):
        tr.train_step(x.transpose(1, 2), tgt, labels)
        # the hand-written clip_grad_norm_: float64 total norm, coefficient clamped to 1, every gradient scaled in place
        ropt.zero_grad()
        loss_fn_kd(ref(x), labels, tgt, KD).backward()
        total = torch.sqrt(sum(p.grad.double().pow(2).sum() for p in ref.parameters()))
        coef = torch.clamp(bound / (total + 1e-6), max=1.0).float()
        clipped += int(coef.item() < 1.0)
        assert tr.last_grad_norm.item() == total.float().item()
        for p in ref.parameters():
            p.grad.mul_(coef)
        ropt.step()
    assert 0 < clipped < 6, clipped
    for p, q in zip(m.parameters(), ref.parameters()):
        assert torch.equal(p.detach(), q.detach())
    assert tr.skipped_steps() == 0


@pytest.mark.parametrize("kw", [dict(max_grad_norm=0.05), dict(skip_nonfinite=True), dict(max_grad_norm=0.05, skip_nonfinite=True)])
def test_cpu_trainer_leaves_an_inf_step_untaken(kw):
    x, tgt, labels = _cpu_data()
    torch.manual_seed(11)
    m, twin = _CpuModel(), _CpuModel()
    twin.load_state_dict(m.state_dict())
    tr, tr_twin = _trainer(m, **kw), _trainer(twin, **kw)
    poison = {"on": False}

    def hook(p):
        if poison["on"]:
            p.grad[1] = INF
    m.fc.bias.register_post_accumulate_grad_hook(hook)
    for step in range(5):
        before = [p.detach().clone() for p in m.parameters()]
        state = [v.clone() for st in tr.opt.state.values() for k, v in st.items() if k != "step"]
        poison["on"] = step == 2
        tr.train_step(x.transpose(1, 2), tgt, labels)
        if step == 2:
            for p, b in zip(m.parameters(), before):
                assert torch.equal(p.detach(), b)
            after = [v for st in tr.opt.state.values() for k, v in st.items() if k != "step"]
            assert len(after) == len(state) and all(torch.equal(a, b) for a, b in zip(after, state))
            assert not torch.isfinite(tr.last_grad_norm)
        else:
            tr_twin.train_step(x.transpose(1, 2), tgt, labels)              # the twin simply does not step at step 2
            assert not any(torch.equal(p.detach(), b) for p, b in zip(m.parameters(), before))
    assert tr.skipped_steps() == 1 and tr_twin.skipped_steps() == 0
    for p, q in zip(m.parameters(), twin.parameters()):
        assert torch.equal(p.detach(), q.detach())


def test_cli_flags_are_on_the_three_parsers():
    import LstmDistillFromDinoV2Train as train
    import LstmDistillation as dino
    parsers = [train.build_parser(train.PERILS), train.build_parser(train.SPAMPINATO), dino.build_parser()]
    for p in parsers:
        off = p.parse_args([])
        assert off.clip_grad_norm == 0.0 and off.skip_nonfinite is False
        on = p.parse_args(["--clip_grad_norm", "2.5", "--skip_nonfinite"])
        assert on.clip_grad_norm == 2.5 and on.skip_nonfinite is True
    assert parsers[2].parse_args([]).clip_grad == 3.0                      # (beside the per-tensor clip, whose default stays)


def test_status_check_has_the_new_keyword():
    import inspect
    from cerebralsignalnetworks_amd import trainer
    sig = inspect.signature(trainer.check_device_status)
    assert list(sig.parameters) == ["model", "collective", "tolerate_nonfinite"]
    assert sig.parameters["tolerate_nonfinite"].default is False and sig.parameters["collective"].default is True
