"""GPU: the 256 x 192 tile body and the XCD-local tile walk of the input-gradient GEMM that runs inside the weight-stationary
backward launches (csrc/gemm_beside.h).

Where the GEMM's width is a multiple of 192 (H = 768, 384) the workers take 256 x 192 tiles, XCD by XCD;
CSN_BESIDE_128=1 keeps the 256 x 128 tiles dealt round-robin, CSN_NO_BESIDE=1 runs the GEMM as a kernel of its own between
two launches.  An output element sees the same 16 x 16 x 32 k-blocks in ascending order in all three, so every output of
forward + backward must be the same BITS: dx, the four gradients of every layer, (dh0, dc0) where a state is given (and
the forward's outputs, which none of the switches touches).  A wrong row clamp or a tile dealt twice or not at all shows
as a difference in the dx rows of a neighbouring timestep or in the layer below's gradients: nothing is compared with a
tolerance.

The kernel names are the same in all three forms.  The launches on 32-row groups are the same with and without
CSN_BESIDE_128; CSN_NO_BESIDE lags the layers one chunk instead of two, so its schedule has L - 1 launches fewer and its
count is checked against that schedule (as tests/test_gpu_half_tiles.py derives it), not against the other two."""
import numpy as np
import pytest

from test_gpu_half_tiles import _expected_half_launches, _run, _same_bits

pytestmark = pytest.mark.gpu

ENVS = (("wide", {}), ("narrow", {"CSN_BESIDE_128": "1"}), ("alone", {"CSN_NO_BESIDE": "1"}))

# name: (B, T, I, H, L), chunk, initial state given
CASES = {
    # chunks of 32 steps and of 1 step: M = 2048 (8 row panels on 208 workers) and M = B = 64 (4 tiles)
    "h768_l2_b64_t33": ((64, 33, 32, 768, 2), 32, False),
    # two GEMMs per launch; M = 96 and M = 24: the only row panel is clamped
    "h768_l3_b24_t9": ((24, 9, 32, 768, 3), 4, True),
    # H = 384: two column tiles, 20 idle workgroups per XCD; B = 130 has padded rows; M = 4160 = 16 panels + 64 rows
    "h384_l2_b130_t33": ((130, 33, 32, 384, 2), 32, False),
    "h384_l3_b64_t9": ((64, 9, 32, 384, 3), 4, True),
    # one chunk, three layers: the diagonals between the layers hold no layer, the GEMMs run stand-alone in every form
    "h768_l3_b24_t4_no_layer_in_range": ((24, 4, 32, 768, 3), 32, False),
    # the cfg2 geometry: 8 groups leave 8 workers per XCD, a 32-step chunk is 128 tiles = two rounds of 64
    "h768_l2_b256_t72_two_rounds": ((256, 72, 32, 768, 2), 32, False),
}


def _three_forms(name, shape, chunk, state, lengths, seed):
    B, T, C, H, L = shape
    got = {}
    for label, env in ENVS:
        out, counts, kernels = _run(shape, chunk, env, state, lengths, seed)       # asserts plan.status() == 0
        want = _expected_half_launches(B, T, H, L, chunk, env, lengths)
        print(f"{name} {label}: 32-row launches (fwd, bwd) {counts}, expected {want}; kernels {kernels}")
        assert counts == want, (name, label, counts, want)
        got[label] = (out, counts, kernels)
    assert got["wide"][1] == got["narrow"][1]
    assert got["wide"][2] == got["narrow"][2] == got["alone"][2]
    assert got["wide"][2][1] == "lstm_bwd_persist_kernel"
    for label in ("narrow", "alone"):
        assert set(got[label][0]) == set(got["wide"][0])
        for k, v in got["wide"][0].items():
            assert np.isfinite(v).all(), k
            _same_bits(v, got[label][0][k], f"{name}: {k}, wide against {label}")
    return got


@pytest.mark.parametrize("name", list(CASES))
def test_wide_tiles_give_the_bits_of_narrow_tiles_and_of_the_standalone_gemm(name):
    shape, chunk, state = CASES[name]
    got = _three_forms(name, shape, chunk, state, None, seed=21)
    want = {"dx"} | ({"dh0", "dc0"} if state else set())
    assert want <= set(got["wide"][0])


def test_wide_tiles_with_lengths():
    """A batch with lengths keeps its backward on 64-row groups: a single layer in range occupies 3 XCDs instead of 6, so
    the workers per XCD and their row-panel ranges are other ones than without lengths."""
    shape, chunk = (130, 9, 32, 768, 2), 4
    B, T = shape[:2]
    rng = np.random.default_rng(5)
    lengths = [int(v) for v in rng.integers(0, T + 1, B)]
    lengths[0], lengths[1], lengths[B - 1] = T, 0, 5
    _three_forms("lengths", shape, chunk, True, lengths, seed=23)


def test_h512_keeps_the_narrow_body():
    """N = 512 is no multiple of 192: the default is the 256 x 128 body, the result that of CSN_BESIDE_128=1."""
    _three_forms("h512", (64, 9, 32, 512, 2), 4, False, None, seed=25)
