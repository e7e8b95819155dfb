"""The views of tests/lstm_input_views.py on CPU tensors, at the shapes of the GPU matrix: the builder contract, and that
over the matrix every branch predicate of the layout kernels is both true and false -- what makes the claim of
tests/test_gpu_lstm_input_views.py to run both branches of kPrepCastX and kPrepBlockifyX checkable without a GPU."""
import pytest
import torch

import lstm_input_views as lv


def _dense(case):
    B, T, I = lv.MATRIX[case][0][:3]
    g = torch.Generator().manual_seed(3)
    return torch.randn(B, T, I, generator=g)


# name -> (stride_b, stride_t, first element) of the view of a [B,T,I] tensor, in elements
EXPECTED_STRIDES = {
    "time_major": lambda B, T, I: (I, B * I, B * I),
    "chan_slice_aligned": lambda B, T, I: (T * (I + 8), I + 8, 0),
    "chan_slice_off1": lambda B, T, I: (T * (I + 8), I + 8, 1),
    "chan_slice_odd_pitch": lambda B, T, I: (T * (I + 3), I + 3, 0),
    "time_slice": lambda B, T, I: ((T + 5) * I, I, 3 * I),
    "time_step2": lambda B, T, I: (2 * T * I, 2 * I, 0),
    "batch_step2": lambda B, T, I: (2 * T * I, I, 0),
    "batch_broadcast": lambda B, T, I: (0, I, T * I),
}


def test_the_table_keeps_the_views_the_layout_kernels_need():
    assert set(EXPECTED_STRIDES) <= set(lv.VIEWS)


@pytest.mark.parametrize("case", list(lv.MATRIX))
@pytest.mark.parametrize("name", list(lv.VIEWS))
def test_builder_contract(case, name):
    x = _dense(case)
    before = x.clone()
    v, dense = lv.VIEWS[name](x)
    assert torch.equal(x, before)                            # the builder leaves its argument alone
    assert v.shape == x.shape == dense.shape and v.dtype == torch.float32 and v.device == x.device
    assert v.stride(2) == 1
    assert dense.is_contiguous() and not dense.isnan().any()
    assert torch.equal(v, dense)
    if name == "batch_broadcast":
        assert torch.equal(dense, x[:1].expand_as(x))
    else:
        assert torch.equal(dense, x)
    assert dense.untyped_storage().data_ptr() != v.untyped_storage().data_ptr()
    # everything in the backing storage that the view does not address is NaN, and there is some of it
    mask = lv.covered(v)
    flat = lv.backing(v)
    assert int(mask.sum()) == (x.numel() if name != "batch_broadcast" else x[0].numel())
    assert not flat[mask].isnan().any()
    assert flat[~mask].isnan().all() and int((~mask).sum()) > 0
    if name in EXPECTED_STRIDES:
        B, T, I = x.shape
        assert (v.stride(0), v.stride(1), v.storage_offset()) == EXPECTED_STRIDES[name](B, T, I)
    assert not v.is_contiguous()


def _over_matrix(cases):
    for case in cases:
        x = _dense(case)
        for name, build in lv.VIEWS.items():
            yield case, name, build(x)[0]


def test_cast_x_takes_both_branches_over_the_matrix():
    cases = [n for n, c in lv.MATRIX.items() if c[1] == "bf16" and c[2] != "row_major"]     # kPrepCastX runs on these
    seen = {}
    for case, name, v in _over_matrix(cases):
        seen.setdefault(lv.branches(case, v)[0], []).append((case, name))
    assert seen.get(True) and seen.get(False), seen
    # every case with I % 8 == 0 runs both branches on its own; I = 12 runs the scalar one whatever the view
    for case in cases:
        got = {lv.branches(case, v)[0] for c, _, v in _over_matrix([case])}
        assert got == ({True, False} if lv.MATRIX[case][0][2] % 8 == 0 else {False}), (case, got)
    scalar = {name for case, name in seen[False] if case == "ks_gemm_i24"}
    assert scalar == {"chan_slice_off1", "chan_slice_odd_pitch"}         # by the base alone, by the strides alone


def test_blockify_x_takes_both_branches_on_every_fused_case():
    assert len(lv.FUSED) == 3
    for case in lv.FUSED:
        by_view = {name: lv.branches(case, v)[1] for _, name, v in _over_matrix([case])}
        assert by_view["chan_slice_off1"] is False and by_view["chan_slice_odd_pitch"] is False, (case, by_view)
        assert all(b is True for n, b in by_view.items() if n not in ("chan_slice_off1", "chan_slice_odd_pitch")), (case, by_view)
    for case in set(lv.MATRIX) - set(lv.FUSED):
        assert all(lv.branches(case, v)[1] is None for _, _, v in _over_matrix([case]))


def test_fuse_x_is_both_true_and_false_over_the_matrix():
    got = {}
    for case, ((B, T, I, H, L), dtype, kind, env) in lv.MATRIX.items():
        if dtype != "bf16" or kind == "row_major" or "CSN_NO_PERSIST" in env:
            continue                        # (fuse_x is asked of plans on paths 2-3 only)
        fused = lv.fuse_x("CSN_FWD_NSPLIT" in env, I, H) and "CSN_NO_FUSE_X" not in env
        assert fused == kind.endswith("_fused"), case
        got.setdefault(fused, []).append(case)
    assert sorted(got[True]) == sorted(lv.FUSED) and len(got[False]) >= 3, got
    # the N-split forward fuses at I = 128 alone, the K-split one not at H = 512
    assert lv.fuse_x(True, 128, 128) and not lv.fuse_x(True, 96, 128)
    assert lv.fuse_x(False, 96, 256) and not lv.fuse_x(False, 96, 512) and not lv.fuse_x(False, 24, 128)


def test_i12_and_i24_fall_on_different_sides_of_the_width_test():
    I12, I24 = lv.MATRIX["ks_gemm_i12"][0][2], lv.MATRIX["ks_gemm_i24"][0][2]
    assert (I12, I24) == (12, 24) and lv.MATRIX["ks_gemm_i12"][0][:2] == lv.MATRIX["ks_gemm_i24"][0][:2]
    for name in ("time_major", "chan_slice_aligned", "time_slice", "time_step2", "batch_step2", "batch_broadcast"):
        v12, v24 = lv.VIEWS[name](_dense("ks_gemm_i12"))[0], lv.VIEWS[name](_dense("ks_gemm_i24"))[0]
        # the same view: aligned base and strides on both, so I % 8 alone decides
        for v in (v12, v24):
            assert v.stride(0) % 4 == 0 and v.stride(1) % 4 == 0 and lv.byte_offset(v) % 16 == 0, name
        assert lv.branches("ks_gemm_i12", v12)[0] is False and lv.branches("ks_gemm_i24", v24)[0] is True, name


def test_predicate_mirrors_term_by_term():
    assert lv.cast_x_vector(8, 4, 8, 32)
    for args in ((12, 4, 8, 32), (8, 6, 8, 32), (8, 4, 9, 32), (8, 4, 8, 36)):       # each term alone switches it off
        assert not lv.cast_x_vector(*args), args
    assert lv.cast_x_vector(8, 0, 8, 0)                                               # a zero stride is a multiple of 4
    assert lv.blockify_x_vector(4, 8, 16) and lv.blockify_x_vector(0, 8, 0)
    for args in ((5, 8, 16), (4, 10, 16), (4, 8, 20)):
        assert not lv.blockify_x_vector(*args), args
