"""The four-wave 256 x 256 / 256 x 128 weight-gradient kernel (the default TN path where the 256-tile kernels apply)
against the 8-wave single-phase ring it replaces (CSN_TN_NO_STAGGER=1): same 32-row MFMA k-blocks in the same order
inside the same K splits, hence the same bits -- slabs, reduced gradients and column sums (bias gradients)."""
import numpy as np
import pytest
import torch

from cerebralsignalnetworks_amd import cabi
from gemm_tn_helpers import env as _env, float64_product as _float64_product, plan_gradients as _plan_gradients

pytestmark = pytest.mark.gpu


def _operands(cuda, M, N, K, seed):
    g = torch.Generator(device=cuda).manual_seed(seed)
    a = torch.randn(K, M, device=cuda, generator=g).to(torch.bfloat16)
    b = torch.randn(K, N, device=cuda, generator=g).to(torch.bfloat16)
    return a, b


@pytest.mark.parametrize("M,N,K", [(3072, 768, 128000), (3072, 128, 128000),
                                   (4096, 1024, 112640), (4096, 128, 112640),      # cfg4
                                   (264, 520, 8256),                               # ragged M and N
                                   (512, 768, 8256),                               # K tail of 64
                                   (256, 136, 8192),                               # N just above the narrow body
                                   (512, 256, 8192)])
def test_w4_matches_single_phase_ring_bit_for_bit(cuda, M, N, K):
    a, b = _operands(cuda, M, N, K, M + N + K)
    got = cabi.gemm_tn(a, b)
    again = cabi.gemm_tn(a, b)
    with _env(CSN_TN_NO_STAGGER="1"):
        ring = cabi.gemm_tn(a, b)
    want = _float64_product(a, b)
    err = float((got.double() - want).abs().max())
    print(f"w4 {M}x{N}x{K}: max |err| vs float64 {err:.3e} (bound {2e-4 * np.sqrt(K):.3e}), "
          f"differing from ring {int((got != ring).sum())}, from rerun {int((got != again).sum())}")
    np.testing.assert_array_equal(got.cpu().numpy(), ring.cpu().numpy())
    np.testing.assert_array_equal(got.cpu().numpy(), again.cpu().numpy())
    np.testing.assert_allclose(got.cpu().numpy(), want.cpu().numpy(), rtol=0, atol=2e-4 * np.sqrt(K))


@pytest.mark.parametrize("B,T,C,H,L", [(64, 160, 128, 768, 2), (64, 128, 128, 1024, 2),
                                       (64, 128, 128, 128, 2)])     # N = 128 with column sums: the narrow body's
def test_w4_lstm_weight_and_bias_gradients_bit_for_bit(cuda, B, T, C, H, L):
    """T x B >= 8192 and a multiple of 64, so every weight-gradient GEMM takes a 256-tile kernel; the recurrent one
    carries the column sums (bias gradients)."""
    new = _plan_gradients(cuda, B, T, C, H, L, {})
    ring = _plan_gradients(cuda, B, T, C, H, L, {"CSN_TN_NO_STAGGER": "1"})
    for name, v in new.items():
        assert np.isfinite(v).all(), name
        assert np.abs(v).max() > 0, name
        np.testing.assert_array_equal(v, ring[name], err_msg=name)


def test_w4_race_screen(cuda):
    """The kernel orders its LDS-DMA stages by counted waits and barriers only; a misplaced wait shows as RARE wrong
    tiles that come and go with the memory load.  The shapes and the screen of
    test_gemm_tn_staggered_ring_race_screen: bit for bit against the 8-wave single-phase ring, 25 times per shape,
    with a second stream hammering HBM beside it."""
    rng = np.random.default_rng(11)
    side = torch.cuda.Stream()
    junk = torch.empty(64 << 20, dtype=torch.float32, device=cuda)
    for (M, N, K) in ((3072, 768, 32768), (512, 256, 8192 + 192), (768, 768, 20480),
                      (3072, 128, 32768)):                          # + the 256 x 128 body
        a = torch.from_numpy(rng.standard_normal((K, M)).astype(np.float32)).to(cuda).to(torch.bfloat16)
        b = torch.from_numpy(rng.standard_normal((K, N)).astype(np.float32)).to(cuda).to(torch.bfloat16)
        with _env(CSN_TN_NO_STAGGER="1"):
            want = cabi.gemm_tn(a, b)
        for rep in range(25):
            with torch.cuda.stream(side):
                junk.add_(1.0)
            got = cabi.gemm_tn(a, b)
            assert torch.equal(got, want), (M, N, K, rep, float((got - want).abs().max()))
        torch.cuda.synchronize()
