"""CPU: LSTM input windows (csn_lstm_plan_set_views) -- what can be checked without a GPU: the declaration and the
binding, the crop bookkeeping of dino.temporal_crops(as_views=True) against its slicing form, the view-major row tables
of MultiCropWrapper.forward_views, and the trainer's flags.  Every test here fails without the feature."""
import os
import re

import numpy as np
import pytest
import torch

import LstmDistillation
from cerebralsignalnetworks_amd import cabi
from cerebralsignalnetworks_amd.dino import temporal_crops, view_rows

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _declaration():
    text = open(os.path.join(ROOT, "include", "csn_hip.h")).read()
    text = re.sub(r"/\*.*?\*/", " ", text, flags=re.S)
    m = re.search(r"\bint\s+csn_lstm_plan_set_views\s*\(([^()]*)\)\s*;", text)
    assert m, "csn_lstm_plan_set_views is not declared in csn_hip.h"
    return [" ".join(a.split()) for a in m.group(1).split(",")]


def test_header_declares_set_views_without_a_stream_and_the_library_exports_it():
    args = _declaration()
    assert args == ["csnLstmPlan* plan", "const int32_t* src_row", "const int32_t* t0", "int32_t src_rows", "int32_t src_T"]
    assert not any("csnStream_t" in a for a in args)
    assert hasattr(cabi.load(), "csn_lstm_plan_set_views")


def test_cabi_binds_set_views_and_the_abi_is_6():
    lib = cabi.load()
    assert "csn_lstm_plan_set_views" in cabi.SIGNATURES
    fn = lib.csn_lstm_plan_set_views
    assert fn.argtypes is not None and len(fn.argtypes) == 5
    assert cabi.ABI_VERSION == 6 and lib.csn_abi_version() == 6
    text = open(os.path.join(ROOT, "include", "csn_hip.h")).read()
    assert re.search(r"#define\s+CSN_ABI_VERSION\s+6\b", text)
    assert callable(getattr(cabi.LstmPlan, "set_views"))
    # a null plan is refused on the host (no device is touched)
    assert fn(None, None, None, 0, 0) == 1
    assert b"null plan" in lib.csn_last_error()


@pytest.mark.parametrize("n_local", [4, 0, 7])
def test_as_views_is_the_slicing_form_call_for_call(n_local):
    g = torch.Generator().manual_seed(3)
    eeg = torch.randn(5, 495, 6, generator=g)
    r1, r2 = np.random.RandomState(17), np.random.RandomState(17)
    for _ in range(3):      # several steps on one generator
        gv, lv = temporal_crops(eeg, 2, n_local, rng=r1)
        starts, lengths = temporal_crops(eeg, 2, n_local, rng=r2, as_views=True)
        assert lengths == [300, 300] + [200] * n_local and len(starts) == 2 + n_local
        for view, s, n in zip(gv + lv, starts, lengths):
            assert 0 <= s <= 495 - n
            assert torch.equal(view, eeg[:, s:s + n])
            for b in range(eeg.shape[0]):
                assert torch.equal(eeg[b, s:s + n], view[b])
        a, b = r1.get_state(), r2.get_state()
        assert a[0] == b[0] and np.array_equal(a[1], b[1]) and a[2:] == b[2:]


def test_as_views_on_the_global_generator_matches_too():
    eeg = torch.zeros(2, 400, 3)
    np.random.seed(5)
    gv, lv = temporal_crops(eeg)
    after = np.random.randint(0, 1 << 30)
    np.random.seed(5)
    starts, lengths = temporal_crops(eeg, as_views=True)
    assert np.random.randint(0, 1 << 30) == after
    assert [v.shape[1] for v in gv + lv] == lengths
    assert [v.storage_offset() // v.stride(1) for v in gv + lv] == list(starts)


def test_per_sample_starts():
    eeg = torch.zeros(7, 330, 2)
    rng = np.random.RandomState(1)
    starts, lengths = temporal_crops(eeg, 2, 4, rng=rng, as_views=True, per_sample=True)
    starts = np.asarray(starts)
    assert starts.shape == (6, 7) and np.issubdtype(starts.dtype, np.integer)
    for v, n in enumerate(lengths):
        assert (starts[v] >= 0).all() and (starts[v] <= 330 - n).all()
    assert len(set(starts[2].tolist())) > 1         # per sample, not one per view
    assert (starts[:2] == 30).any()                 # T - 300 = 30: most draws of a global view are moved left
    with pytest.raises(ValueError, match="as_views"):
        temporal_crops(eeg, rng=rng, per_sample=True)


def test_view_major_rows():
    # V = 3 views of B = 2 samples, one start per view
    rows, t0, n = view_rows([5, 0, 9], [4, 4, 2], 2)
    assert rows == [0, 1, 0, 1, 0, 1]
    assert t0 == [5, 5, 0, 0, 9, 9]
    assert n == [4, 4, 4, 4, 2, 2]
    # one start per (view, sample)
    rows, t0, n = view_rows(np.array([[1, 2, 3], [4, 5, 6]]), [7, 3], 3)
    assert rows == [0, 1, 2, 0, 1, 2]
    assert t0 == [1, 2, 3, 4, 5, 6]
    assert n == [7, 7, 7, 3, 3, 3]
    assert all(type(v) is int for v in rows + t0 + n)
    for v in range(2):
        for b in range(3):
            assert rows[v * 3 + b] == b             # row = v * B + b, src_row = b
    with pytest.raises(ValueError):
        view_rows([1, 2, 3], [4, 4], 2)


def test_trainer_flags_default_off():
    flags = LstmDistillation.build_parser().parse_args([])
    assert flags.fused_views is False and flags.per_sample_crops is False
    flags = LstmDistillation.build_parser().parse_args(["--fused_views", "--per_sample_crops"])
    assert flags.fused_views is True and flags.per_sample_crops is True
    text = LstmDistillation.build_parser().format_help()
    assert "dropout" in text[text.index("--fused_views"):]         # the help says that the masks differ


def test_per_sample_crops_without_fused_views_is_refused(capsys):
    with pytest.raises(SystemExit) as e:
        LstmDistillation.main(["--per_sample_crops", "--synthetic", "8"])
    assert e.value.code == 2
    assert "--per_sample_crops needs --fused_views" in capsys.readouterr().err
