"""CPU: the flat-buffer optimiser entry points (csrc/optim.hip: segment norms, per-tensor clip, Adam / AdamW, LARS) are
declared, exported and bound; every argument violation is refused on the host with CSN_ERR_INVALID_ARGUMENT and a message
before anything is launched (a launch on a machine without a GPU would return CSN_ERR_HIP instead); the Python layer
refuses CPU tensors, derives the per-tensor flags from its arguments, and DistillTrainer without a GPU keeps torch's
optimisers."""
import ctypes
import os
import re

import pytest
import torch

import __graft_entry__ as graft
from cerebralsignalnetworks_amd import cabi
from cerebralsignalnetworks_amd import FlatAdamW, FlatLARS, flat_clip_gradients
from cerebralsignalnetworks_amd.flat_optim import adam_segment_flags, lars_segment_flags, segment_ends
from cerebralsignalnetworks_amd.trainer import DistillTrainer, FlatGrads

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("csn_flat_segments_scratch_bytes", "csn_flat_segments_prepare", "csn_flat_segment_norms", "csn_flat_clip",
       "csn_adam_step", "csn_lars_step")
INVALID = 1                 # CSN_ERR_INVALID_ARGUMENT
OK_PTR = 0x10000            # non-null and 16-byte aligned: never dereferenced, every call below is refused before a launch
ODD_PTR = 0x10004           # 4-byte aligned only


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
    for name, value in (("CSN_SEG_DECAYED", cabi.SEG_DECAYED), ("CSN_SEG_SCALED", cabi.SEG_SCALED)):
        assert re.search(r"#define\s+%s\s+%d\b" % (name, value), text)
    # every new declaration cites the reference call site it replaces
    block = text[text.index("CSN_SEG_DECAYED"):text.index("K7  Barlow")]
    for site in ("utils/utils.py:132-141", "LstmDistillFromDinoV2TrainSpampinato.py:378", "LSTMDistill.py:322",
                 "EEG-BarlowNetworks/optim.py:17-44", "LstmDistillation.py:150"):
        assert site in block, site


def _refused(lib, rc, *words):
    msg = lib.csn_last_error().decode()
    assert rc == INVALID, (rc, msg)
    assert msg and all(w in msg for w in words), msg


def _ends(*v):
    return (ctypes.c_int64 * len(v))(*v)


def test_scratch_bytes_covers_the_table(lib):
    n, nseg = 3 * 2 ** 20 + 4110, 4
    chunks = -(-n // 2048)
    need = chunks * 4 + nseg * (8 + 4 + 4) + 4 + 2 * 8 * (chunks + nseg) + 2 * 8 * nseg
    got = lib.csn_flat_segments_scratch_bytes(nseg, n)
    assert need <= got <= need + 6 * 16
    assert lib.csn_flat_segments_scratch_bytes(0, n) == 0 and b"nseg" in lib.csn_last_error()
    assert lib.csn_flat_segments_scratch_bytes(4, 3) == 0


def test_prepare_refusals(lib):
    prep = lib.csn_flat_segments_prepare
    good = _ends(1961, 2014, 2597, 2608)
    _refused(lib, prep(good, None, 4, 2608, None, None), "null")
    _refused(lib, prep(good, None, 4, 2608, ODD_PTR, None), "aligned")
    _refused(lib, prep(None, None, 4, 2608, OK_PTR, None), "null")
    _refused(lib, prep(good, None, 0, 2608, OK_PTR, None), "nseg")
    _refused(lib, prep(good, None, -2, 2608, OK_PTR, None), "nseg")
    _refused(lib, prep(_ends(1961, 1961, 2597, 2608), None, 4, 2608, OK_PTR, None), "ascend")
    _refused(lib, prep(_ends(1961, 53, 2597, 2608), None, 4, 2608, OK_PTR, None), "ascend")
    _refused(lib, prep(_ends(0, 53, 2597, 2608), None, 4, 2608, OK_PTR, None), "ascend")
    _refused(lib, prep(good, None, 4, 2609, OK_PTR, None), "last segment")
    _refused(lib, prep(_ends(1961, 2014, 2597, 2700), None, 4, 2608, OK_PTR, None), "last segment")
    _refused(lib, prep(good, (ctypes.c_int32 * 4)(1, 2, 3, 4), 4, 2608, OK_PTR, None), "flags")


def test_norm_and_clip_refusals(lib):
    norms, clip = lib.csn_flat_segment_norms, lib.csn_flat_clip
    _refused(lib, norms(None, None, 0.0, 2608, 4, OK_PTR, None, None), "null")
    _refused(lib, norms(OK_PTR, None, 0.0, 2608, 4, None, None, None), "null")
    _refused(lib, norms(ODD_PTR, None, 0.0, 2608, 4, OK_PTR, None, None), "aligned")
    _refused(lib, norms(OK_PTR, ODD_PTR, 0.0, 2608, 4, OK_PTR, None, None), "aligned")
    _refused(lib, norms(OK_PTR, None, 0.0, 2608, 4, ODD_PTR, None, None), "aligned")
    _refused(lib, norms(OK_PTR, None, 0.0, 2608, 0, OK_PTR, None, None), "nseg")
    _refused(lib, clip(None, 2608, 4, OK_PTR, 1.0, None, None), "null")
    _refused(lib, clip(OK_PTR, 2608, 4, None, 1.0, None, None), "null")
    _refused(lib, clip(ODD_PTR, 2608, 4, OK_PTR, 1.0, None, None), "aligned")
    _refused(lib, clip(OK_PTR, 2608, 0, OK_PTR, 1.0, None, None), "nseg")
    _refused(lib, clip(OK_PTR, 2608, 4, OK_PTR, 0.0, None, None), "clip")


def test_adam_and_lars_refusals(lib):
    def adam(p=OK_PTR, g=OK_PTR, m=OK_PTR, v=OK_PTR, n=2608, nseg=4, table=OK_PTR, t=1, b1=0.9, b2=0.999):
        return lib.csn_adam_step(p, g, m, v, n, nseg, table, t, 1e-3, b1, b2, 1e-8, 1e-2, 1, 0.0, None, None)
    for k in ("p", "g", "m", "v", "table"):
        _refused(lib, adam(**{k: None}), "null")
        _refused(lib, adam(**{k: ODD_PTR}), "aligned")
    _refused(lib, adam(nseg=0), "nseg")
    _refused(lib, adam(t=0), "t must be >= 1")
    _refused(lib, adam(t=-3), "t must be >= 1")
    for b in (1.0, -0.1, 1.5, float("nan")):
        _refused(lib, adam(b1=b), "betas")
        _refused(lib, adam(b2=b), "betas")

    def lars(p=OK_PTR, g=OK_PTR, mu=OK_PTR, nseg=4, table=OK_PTR):
        return lib.csn_lars_step(p, g, mu, 2608, nseg, table, 0.2, 1e-6, 0.9, 1e-3, None)
    for k in ("p", "g", "mu", "table"):
        _refused(lib, lars(**{k: None}), "null")
        _refused(lib, lars(**{k: ODD_PTR}), "aligned")
    _refused(lib, lars(nseg=0), "nseg")


def _net():
    torch.manual_seed(3)
    return torch.nn.Sequential(torch.nn.Linear(37, 53), torch.nn.Tanh(), torch.nn.Linear(53, 11))


def test_fused_optimisers_refuse_cpu_tensors():
    fg = FlatGrads(_net().parameters(), flatten_params=True)
    with pytest.raises(cabi.CsnError):
        FlatAdamW(fg)
    with pytest.raises(cabi.CsnError):
        FlatLARS(fg, lr=0.2)
    with pytest.raises(cabi.CsnError):
        flat_clip_gradients(fg, 0.1)
    with pytest.raises(cabi.CsnError):
        cabi.SegmentTable([5, 9], [3, 3], "cpu")
    with pytest.raises(ValueError, match="flatten_params"):
        FlatAdamW(FlatGrads(_net().parameters()))


def test_segment_flags_follow_the_arguments():
    net = _net()
    params = list(net.parameters())                    # weight [53,37], bias [53], weight [11,53], bias [11]
    fg = FlatGrads(params)
    assert segment_ends(fg) == [1961, 2014, 2597, 2608]
    D, S = cabi.SEG_DECAYED, cabi.SEG_SCALED
    assert adam_segment_flags(params) == [D, D, D, D]
    biases = [p for p in params if p.ndim == 1]
    assert adam_segment_flags(params, no_decay=biases) == [D, 0, D, 0]
    assert adam_segment_flags(params, no_decay=biases, clip=0.1) == [D | S, S, D | S, S]
    assert adam_segment_flags(params, clip=3.0) == [D | S] * 4
    # identity, not value: an equal tensor that is not the parameter exempts nothing
    assert adam_segment_flags(params, no_decay=[params[1].detach().clone()]) == [D] * 4
    assert lars_segment_flags(params) == [D | S] * 4
    assert lars_segment_flags(params, weight_decay_filter=True) == [D | S, S, D | S, S]
    assert lars_segment_flags(params, lars_adaptation_filter=True) == [D | S, D, D | S, D]
    assert lars_segment_flags(params, True, True) == [D | S, 0, D | S, 0]


@pytest.mark.parametrize("name,cls", [("adamw", torch.optim.AdamW), ("adam", torch.optim.Adam), ("rmsprop", torch.optim.RMSprop)])
def test_trainer_without_a_gpu_keeps_the_torch_optimisers(name, cls):
    from cerebralsignalnetworks_amd import Model
    m = Model(input_size=16, lstm_size=32, lstm_layers=1, output_size=8, include_top=False)
    tr = DistillTrainer(m, None, loss="cosine", optimizer=name, preprocess=False, fused_optimizer=True)
    assert type(tr.opt) is cls and tr.grads.flat_params is None


def test_trainer_without_a_gpu_keeps_torch_lars():
    from cerebralsignalnetworks_amd import Model
    from cerebralsignalnetworks_amd.losses import LARS
    m = Model(input_size=16, lstm_size=32, lstm_layers=1, output_size=8, include_top=False)
    tr = DistillTrainer(m, None, loss="cosine", optimizer="lars", preprocess=False, fused_optimizer=True)
    assert type(tr.opt) is LARS


def test_cli_flag_is_on_both_parsers():
    import LstmDistillFromDinoV2Train as train
    import LstmDistillation as dino
    for flavour in (train.PERILS, train.SPAMPINATO):
        assert train.build_parser(flavour).parse_args([]).fused_optimizer is False
        assert train.build_parser(flavour).parse_args(["--fused_optimizer"]).fused_optimizer is True
    assert dino.build_parser().parse_args([]).fused_optimizer is False
    assert dino.build_parser().parse_args(["--fused_optimizer"]).fused_optimizer is True


def test_state_dict_holds_plain_numbers_when_a_schedule_wrote_numpy_scalars(tmp_path):
    # the DINO CLI writes cosine_scheduler's numpy.float64 into param_groups; a checkpoint with those inside would be
    # refused by torch.load(weights_only=True)
    import types
    import numpy as np
    from cerebralsignalnetworks_amd.dino import cosine_scheduler
    from cerebralsignalnetworks_amd.flat_optim import _FlatOptimizer
    lr = cosine_scheduler(5e-4, 1e-6, 1, 4, warmup_epochs=1)[3]
    assert type(lr) is not float
    opt = types.SimpleNamespace(flags=[3, 2], param_groups=[dict(lr=lr, betas=(np.float32(0.5), 0.999), eps=1e-8,
                                                                 weight_decay=np.float64(0.04), clip=None, params=[])])
    sd = _FlatOptimizer._state(opt, {"mu": torch.arange(3.)})
    assert type(sd["lr"]) is float and sd["lr"] == float(lr)
    assert type(sd["weight_decay"]) is float and sd["weight_decay"] == 0.04
    assert type(sd["betas"]) is tuple and [type(b) for b in sd["betas"]] == [float, float] and sd["betas"][0] == 0.5
    assert sd["clip"] is None and sd["eps"] == 1e-8 and "params" not in sd
    torch.save({"optimizer": sd}, tmp_path / "ck.pth")
    back = torch.load(tmp_path / "ck.pth", weights_only=True)["optimizer"]
    assert back["lr"] == sd["lr"] and back["flags"] == [3, 2] and torch.equal(back["mu"], sd["mu"])
