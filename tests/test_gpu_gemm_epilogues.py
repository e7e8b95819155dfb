"""The store epilogues of the NT GEMM kernels (nt_store_frag / nt_store4 / nt_store1 in csrc/gemm_tile.h, the epilogue
through LDS of gemm_nt_256_kernel, the generic kernel's own) on every route of csn_gemm_nt: float32 out, float32 out
accumulating into C, bfloat16 out, each with and without a bias.

Exact, no tolerance anywhere: the operands are integers in {-2, ..., 2} (tests/gemm_tn_splits.operands), bias and the old
C small integers, so every partial sum is an integer below 4 K + 8 + 64 < 2^24 and every float32 accumulation order is
exact.  A float32 result must have the bits of the integer product, a bfloat16 result the bits of that float32 result
rounded by torch's .to(torch.bfloat16).  The reference is the numpy product, once per shape: computed through float64
(also exact: integers below 2^53, whatever the summation order), converted to int64 and held against numpy's own int64
matmul on a sample of rows.  C lies between two guard bands and everything holds a NaN pattern before the call: the
guards stay as they were and, unless the call accumulates, no NaN survives inside.  Every case first asserts through
cabi.gemm_nt_route that the library takes the route its id names."""
import functools
import os

import numpy as np
import pytest
import torch

import gemm_tn_splits
from cerebralsignalnetworks_amd import cabi

pytestmark = pytest.mark.gpu

# (route, M, N, K, switches): the smallest shapes that reach each route from both sides of its thresholds
CASES = [("wide192w4", 8192, 3072, 768, {}),
         ("wide192", 8192, 3072, 768, {"CSN_NT_NO_W4": "1"}),
         ("wide256", 8192, 4096, 1024, {}),
         ("dma", 8192, 768, 3072, {}),
         ("tile256x128", 8192, 1024, 768, {}),
         ("wide192w4", 4088, 3072, 128, {}),          # a last row tile of 248 rows
         ("wide256", 4088, 4096, 128, {}),
         ("tile256x128", 264, 1028, 256, {}),         # a column tail of 4, a row tile of 8
         ("dma", 136, 76, 64, {}),                    # column tails in the accumulator layout
         ("bf16", 136, 76, 64, {"CSN_GEMM_NO_DMA": "1"}),
         ("bf16", 136, 76, 72, {}),
         ("generic", 136, 76, 70, {})]
MODES = [(out, acc, bias) for (out, acc) in ((torch.float32, False), (torch.float32, True), (torch.bfloat16, False))
         for bias in (True, False)]
GUARD_ROWS = 8              # rows of N elements in front of and behind C (8 rows keep C 16-byte aligned for every N % 4 == 0)


def _case_id(c):
    return f"{c[0]}-{c[1]}x{c[2]}x{c[3]}" + "".join("-" + k[4:].lower() for k in c[4])


def _mode_id(m):
    return ("f32" if m[0] == torch.float32 else "bf16") + ("-acc" if m[1] else "") + ("-bias" if m[2] else "-nobias")


@pytest.fixture(autouse=True)
def _only_the_switches_of_the_case(monkeypatch):
    for name in list(os.environ):
        if name.startswith("CSN_GEMM_") or name.startswith("CSN_NT_"):
            monkeypatch.delenv(name, raising=False)
    return monkeypatch


@functools.lru_cache(maxsize=2)
def _reference(M, N, K):
    """A[M, K], Bt[N, K] (int8), bias[N], old C[M, N] (small integers) and the int64 product, computed once per shape."""
    a_km, b_kn = gemm_tn_splits.operands(M, N, K)
    a, bt = np.ascontiguousarray(a_km.T), np.ascontiguousarray(b_kn.T)
    rng = np.random.default_rng(gemm_tn_splits.seed_of(M, N, K, salt=1))
    bias = rng.integers(-8, 9, size=N, dtype=np.int64)
    c0 = rng.integers(-64, 65, size=(M, N), dtype=np.int64)
    prod = (a.astype(np.float64) @ bt.astype(np.float64).T).astype(np.int64)
    rows = np.unique(np.concatenate([np.arange(0, M, max(1, M // 16)), [M - 1]]))
    assert np.array_equal(prod[rows], a[rows].astype(np.int64) @ bt.astype(np.int64).T)
    assert int(np.abs(prod).max()) + 8 + 64 < 2 ** 24
    return a, bt, bias, c0, prod


@pytest.mark.parametrize("mode", MODES, ids=_mode_id)
@pytest.mark.parametrize("case", CASES, ids=_case_id)
def test_store_matrix_is_exact_inside_and_leaves_the_guards(cuda, _only_the_switches_of_the_case, case, mode):
    route, M, N, K, env = case
    out_dtype, accumulate, with_bias = mode
    for name, value in env.items():
        _only_the_switches_of_the_case.setenv(name, value)
    a, bt, bias, c0, prod = _reference(M, N, K)

    buf = torch.full((M + 2 * GUARD_ROWS, N), float("nan"), dtype=out_dtype, device=cuda)
    c = buf[GUARD_ROWS:GUARD_ROWS + M]
    a16 = torch.from_numpy(a).to(cuda).to(torch.bfloat16)
    b16 = torch.from_numpy(bt).to(cuda).to(torch.bfloat16)
    biasf = torch.from_numpy(bias).to(cuda).float() if with_bias else None
    aligned = all(t.data_ptr() % 16 == 0 for t in (a16, b16, c) + ((biasf,) if with_bias else ()))
    assert aligned and c.is_contiguous()
    assert cabi.gemm_nt_route(M, N, K, torch.bfloat16, aligned) == route

    want = prod + (bias[None, :] if with_bias else 0)
    if accumulate:
        c.copy_(torch.from_numpy(c0).to(cuda).float())
        want = want + c0
    bits = torch.int32 if out_dtype == torch.float32 else torch.int16
    guards = buf.view(bits).clone()
    cabi.gemm_nt(a16, b16, biasf, out=c, accumulate=accumulate)
    torch.cuda.synchronize()

    after = buf.view(bits)
    assert torch.equal(after[:GUARD_ROWS], guards[:GUARD_ROWS]), "the guard band in front of C was written"
    assert torch.equal(after[GUARD_ROWS + M:], guards[GUARD_ROWS + M:]), "the guard band behind C was written"
    if not accumulate:
        assert not bool(torch.isnan(c).any()), "C holds NaN: an element was not written"
    want_t = torch.from_numpy(want).to(cuda).float()                # exact: |want| < 2^24
    assert torch.equal(want_t.long(), torch.from_numpy(want).to(cuda))
    if out_dtype == torch.bfloat16:
        want_t = want_t.to(torch.bfloat16)
    wrong = int((c.view(bits) != want_t.view(bits)).sum())
    print(f"{_case_id(case)} {_mode_id(mode)}: elements whose bits differ from the exact result: {wrong}")
    assert wrong == 0
