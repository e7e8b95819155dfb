"""The four-wave 256 x 192 input-projection kernel (gemm_nt_w4_kernel in csrc/gemm_nt.hip, the default wherever the 8-wave
gemm_nt_wide_kernel<.., 192> ran): a ring that wraps, clamped and skipped rows in both wave rows, a last row tile of one
row, an odd number of 64-column blocks, two workgroups on every CU, the LSTM's aspect.

Exact: operands are integers in {-2, ..., 2} and the bias small integers, so every float32 partial sum is exact
(|sum| <= 4 K + 8 < 2^24) and C must have the bits of the float64 product, into a C that holds the NaN pattern 0x7fc00000
and is followed by a guard band.  Random: the same k-blocks in the same order as the 8-wave kernel (CSN_NT_NO_W4) and the
256 x 128 kernel (CSN_GEMM_NO_192), so the three results are bit-equal; against float64 within the limits of
test_gemm_nt_wide_tile_kernel.  Every case asserts through tests/stream_order.py that its shape takes the 256 x 192
route, and through the library's own predicate that its operands lie inside the kernel's 32-bit offset window (what lies
outside is a CPU test: tests/test_gemm_nt_w4_build_cpu.py)."""
import os

import pytest
import torch

import stream_order
from cerebralsignalnetworks_amd import cabi

pytestmark = pytest.mark.gpu

SHAPES = [(256, 49152, 128), (300, 24576, 128), (257, 49152, 128), (1000, 12288, 320), (512, 49152, 128), (2048, 6144, 192)]
GUARD = 1 << 20             # bytes behind C
POISON = 0x7fc00000         # a float32 NaN


@pytest.fixture(autouse=True)
def _only_the_switches_of_the_case(monkeypatch):
    for name in list(os.environ):
        if name.startswith("CSN_GEMM_") or name.startswith("CSN_NT_"):
            monkeypatch.delenv(name, raising=False)
    return monkeypatch


def _route(M, N, K):
    assert stream_order.gemm_nt_route(M, N, K, torch.bfloat16) == "wide192"
    assert cabi.gemm_nt_w4_offsets_fit(M, N, K)


class _PoisonedC:
    """C[M, N] (float32 or bfloat16) as a view of a buffer that holds the NaN pattern and a guard band behind C."""

    def __init__(self, cuda, M, N, dtype=torch.float32):
        self.words = M * N * (4 if dtype == torch.float32 else 2) // 4
        self.buf = torch.full((self.words + GUARD // 4,), POISON, dtype=torch.int32, device=cuda)
        self.c = self.buf[:self.words].view(dtype).view(M, N)

    def check(self):
        torch.cuda.synchronize()
        assert bool((self.buf[self.words:] == POISON).all()), "the guard band behind C was written"
        assert not bool(torch.isnan(self.c).any()), "C holds NaN: an element was not written"
        return self.c


def _ints(cuda, g, lo, hi, *shape):
    return torch.randint(lo, hi + 1, shape, device=cuda, generator=g)


@pytest.mark.parametrize("M,N,K", SHAPES)
def test_exact_product_into_poisoned_c(cuda, M, N, K):
    _route(M, N, K)
    g = torch.Generator(device=cuda).manual_seed(3 * M + 5 * N + 7 * K)
    a, b = _ints(cuda, g, -2, 2, M, K), _ints(cuda, g, -2, 2, N, K)
    bias, c0 = _ints(cuda, g, -8, 8, N), _ints(cuda, g, -64, 64, M, N)
    want64 = a.double() @ b.double().t()
    assert float(want64.abs().max()) + 8 + 64 < 2 ** 24 and float((want64 == 0).double().mean()) < 0.1
    a16, b16, biasf = a.to(torch.bfloat16), b.to(torch.bfloat16), bias.float()

    plain = _PoisonedC(cuda, M, N)
    cabi.gemm_nt(a16, b16, None, out=plain.c)
    got = plain.check()
    print(f"{M}x{N}x{K}: elements differing from the exact product {int((got.double() != want64).sum())}")
    assert torch.equal(got.double(), want64)

    biased = _PoisonedC(cuda, M, N)
    cabi.gemm_nt(a16, b16, biasf, out=biased.c)
    assert torch.equal(biased.check().double(), want64 + bias.double())

    acc = _PoisonedC(cuda, M, N)
    acc.c.copy_(c0.float())
    cabi.gemm_nt(a16, b16, biasf, out=acc.c, accumulate=True)
    assert torch.equal(acc.check().double(), want64 + bias.double() + c0.double())


@pytest.mark.parametrize("M,N,K", SHAPES)
def test_random_operands_bit_equal_to_the_other_kernels(cuda, _only_the_switches_of_the_case, M, N, K):
    _route(M, N, K)
    monkeypatch = _only_the_switches_of_the_case
    g = torch.Generator(device=cuda).manual_seed(M + N + K)
    a = torch.randn(M, K, device=cuda, generator=g).to(torch.bfloat16)
    b = torch.randn(N, K, device=cuda, generator=g).to(torch.bfloat16)
    bias = torch.randn(N, device=cuda, generator=g)
    c0 = torch.randn(M, N, device=cuda, generator=g)
    ref = a.double() @ b.double().t() + bias.double()

    def run():
        f32 = _PoisonedC(cuda, M, N)
        cabi.gemm_nt(a, b, bias, out=f32.c)
        b16 = _PoisonedC(cuda, M, N, torch.bfloat16)
        cabi.gemm_nt(a, b, bias, out=b16.c)
        acc = c0.clone()
        cabi.gemm_nt(a, b, None, out=acc, accumulate=True)
        return f32.check(), b16.check(), acc

    new = run()
    e32, e16 = (float((t.double() - ref).norm() / ref.norm()) for t in new[:2])
    print(f"{M}x{N}x{K}: relative norm error against float64: float32 {e32:.3e}, bfloat16 {e16:.3e}")
    assert e32 < 2e-6 and e16 < 4e-3
    for switch in ("CSN_NT_NO_W4", "CSN_GEMM_NO_192"):
        monkeypatch.setenv(switch, "1")
        old = run()
        monkeypatch.delenv(switch)
        for name, x, y in zip(("float32 with bias", "bfloat16", "accumulate"), new, old):
            assert torch.equal(x, y), f"{name}: default against {switch}"
