"""Shared by tests/test_gemm_tn_splits_cpu.py and tests/test_gpu_gemm_tn_splits.py (not a test module): a plain-Python
statement of how the weight-gradient GEMM (csn_gemm_tn, launch_gemm_tn_slabs in csrc/gemm_tn.hip) cuts its contraction
K = T * B into S splits of `kper` rows, the cases the two files run, and their exact small-integer operands.

The formulas are WRITTEN OUT here, not imported from the library: the CPU file holds them against
csn_gemm_tn_scratch_bytes (which is S * M * N * 4) and every GPU case asserts through them that it reaches the tail its id
names, so a change of the dispatch turns these tests red instead of letting them test something else.

    256-tile kernels (bf16, M % 8 == N % 8 == 0, K % 64 == 0, K >= 8192, M >= 256, N >= 128, no CSN_GEMM_NO_256):
        S = clamp(min(256 // (ceil(M/256) * ceil(N/256)), K // 2048), 1, 64);  kper = ceil(K / S) rounded up to 64
    128-tile bf16 kernel (M % 8 == N % 8 == 0) and the generic / float32 kernels (everything else):
        S = clamp(min(ceil(1024 / (ceil(M/128) * ceil(N/128))), ceil(K/512)), 1, 64)
        kper = ceil(K / S) rounded up to 64 (bf16 kernel) or to 16 (generic / float32)

Split z covers rows [z * kper, min((z + 1) * kper, K)): rounding kper up leaves the last splits short or EMPTY."""
import collections

import numpy as np

# the environment switches that choose among the weight-gradient kernels: a case sets its own and runs without the others
SWITCHES = ("CSN_GEMM_NO_256", "CSN_GEMM_NO_DMA", "CSN_TN_NO_STAGGER", "CSN_TN_STAGES", "CSN_TN_NO_TR", "CSN_GEMM_GENERIC")

Regime = collections.namedtuple("Regime", "kernel S kper rows")     # rows: the row count of every split, S entries


def _ceil(a, b):
    return -(-a // b)


def _clamp(s):
    return max(1, min(64, s))


def splits_256(M, N, K):
    return _clamp(min(256 // (_ceil(M, 256) * _ceil(N, 256)), K // 2048))


def splits_128(M, N, K):
    return _clamp(min(_ceil(1024, _ceil(M, 128) * _ceil(N, 128)), _ceil(K, 512)))


def uses_256(M, N, K, no_256=False, no_dma=False):
    """The shape part of the dispatch (csn_gemm_tn_scratch_bytes reserves for it whatever the operand type).  no_256 and
    no_dma: CSN_GEMM_NO_256 / CSN_GEMM_NO_DMA are set; either takes the 256-tile kernels away.  The callers pass what
    their case sets and run with every switch in SWITCHES that it does not set removed from the environment."""
    return M >= 256 and N >= 128 and K % 64 == 0 and K >= 8192 and not no_256 and not no_dma


def _rows(S, kper, K):
    return [max(0, min((z + 1) * kper, K) - z * kper) for z in range(S)]


def regime(M, N, K, bf16=True, no_256=False):
    """The kernel family csn_gemm_tn runs for dense 16-byte aligned operands, its S, kper and rows per split."""
    eights = M % 8 == 0 and N % 8 == 0
    if bf16 and eights and uses_256(M, N, K, no_256):
        S, unit, kernel = splits_256(M, N, K), 64, "tn256"
    else:
        S = splits_128(M, N, K)
        if bf16 and eights:
            unit, kernel = 64, "tn128"
        elif not bf16 and M % 128 == 0 and N % 128 == 0 and K % 16 == 0:
            unit, kernel = 16, "f32_128"
        else:
            unit, kernel = 16, "generic"
    kper = _ceil(_ceil(K, S), unit) * unit
    return Regime(kernel, S, kper, _rows(S, kper, K))


def scratch_bytes(M, N, K, no_256=False, no_dma=False):
    """What csn_gemm_tn_scratch_bytes must return: room for the slabs of whichever kernel may run."""
    s256 = splits_256(M, N, K) if uses_256(M, N, K, no_256, no_dma) else 0
    return max(splits_128(M, N, K), s256) * M * N * 4


def tail(r):
    """(rows of the last non-empty split, number of empty splits)."""
    full = [n for n in r.rows if n > 0]
    return full[-1], r.S - len(full)


def describe(r):
    return f"{r.kernel}: S = {r.S}, kper = {r.kper}, last three splits {r.rows[-3:]} rows"


# ---- the cases -------------------------------------------------------------------------------------------------------
# 256-tile kernels: two tiles of 256 each, so S = min(128, K // 2048).  K -> (S, rows of the last non-empty split, empty
# splits); a split of n rows is n / 32 ring stages, and 2 stages is the four-wave kernel's `nh == PF - 1` prologue.
MN_256 = [(512, 128),        # the narrow 256 x 128 body
          (512, 256),        # the 256 x 256 body
          (264, 136)]        # ragged M and N: clamped source columns
K_256 = {63552: (31, 192, 0), 65600: (32, 128, 0), 67648: (33, 64, 0), 69696: (34, 2112, 1), 131136: (64, 192, 1)}
ENVS_256 = [("w4", {}),                                              # the default: the four-wave kernel
            ("ring4", {"CSN_TN_NO_STAGGER": "1"}),                    # 8-wave rings of 4 / 3 / 5 stages
            ("ring3", {"CSN_TN_STAGES": "3"}),
            ("ring5", {"CSN_TN_STAGES": "5"}),
            ("tn128", {"CSN_GEMM_NO_256": "1"}),                      # the 128-tile kernel, S = 64 at these K
            ("tn128-notr", {"CSN_GEMM_NO_256": "1", "CSN_TN_NO_TR": "1"})]

# 128-tile and generic kernels at S = 64: (id, bf16, M, N, K, kernel, kper, rows of the last non-empty split, empty splits)
CASES_128 = [("bf16-128x128-K32769-7empty", True, 128, 128, 32769, "tn128", 576, 513, 7),
             ("bf16-128x128-K32833-last1", True, 128, 128, 32833, "tn128", 576, 1, 6),
             ("bf16-128x128-K35745-1empty", True, 128, 128, 35745, "tn128", 576, 33, 1),
             ("bf16-72x40-K32833-ragged", True, 72, 40, 32833, "tn128", 576, 1, 6),
             ("bf16-70x52-K32833-generic", True, 70, 52, 32833, "generic", 528, 97, 1),
             ("f32-128x128-K32784-last48", False, 128, 128, 32784, "f32_128", 528, 48, 1),
             ("f32-72x40-K32833-generic", False, 72, 40, 32833, "generic", 528, 97, 1)]

# LSTM plans (B, T, C, H, L): the recurrent weight gradient is (4H, H, T * B) and carries the column sums (bias gradients),
# the layer-0 input one is (4H, C, T * B).  -> (S, rows of the last non-empty split, empty splits) of both
LSTM_SHAPES = {(64, 1057, 128, 128, 2): (33, 64, 0),        # the narrow body with column sums, a 64-row last split
               (64, 1089, 128, 128, 2): (34, 2112, 1),      # an empty split
               (64, 1089, 128, 256, 2): (34, 2112, 1)}      # the 256 x 256 body with column sums: 4 tiles, S = 34


def all_shapes():
    """Every (M, N, K) the GPU file hands to the library."""
    out = [(M, N, K) for (M, N) in MN_256 for K in K_256]
    out += [(c[2], c[3], c[4]) for c in CASES_128]
    for (B, T, C, H, L) in LSTM_SHAPES:
        out += [(4 * H, H, T * B), (4 * H, C, T * B)]
    return sorted(set(out))


# ---- exact operands ---------------------------------------------------------------------------------------------------
def seed_of(M, N, K, salt=0):
    return 1000003 * M + 1009 * N + K + 7919 * salt


def operands(M, N, K, salt=0):
    """A[K, M], B[K, N]: integers uniform in {-2, ..., 2} as int8 (exact in bf16 and float32).  Every product is at most 4
    and every partial sum at most 4 K < 2^24, so EVERY float32 accumulation in every kernel, split count and summation
    order is exact and the result must have the bits of the mathematical product."""
    rng = np.random.default_rng(seed_of(M, N, K, salt))
    return rng.integers(-2, 3, size=(K, M), dtype=np.int8), rng.integers(-2, 3, size=(K, N), dtype=np.int8)
