"""CPU: the plain-Python statement of the weight-gradient GEMM's K splits (tests/gemm_tn_splits.py), which
tests/test_gpu_gemm_tn_splits.py uses to assert the tail every case reaches, agrees with the library's host-only
csn_gemm_tn_scratch_bytes at every shape that file runs, and finds the short and empty last splits it is there for."""
import os

import pytest

import gemm_tn_splits as sp
from cerebralsignalnetworks_amd import cabi


@pytest.fixture
def clean_env(monkeypatch):
    for name in sp.SWITCHES:
        monkeypatch.delenv(name, raising=False)
    return monkeypatch


@pytest.mark.parametrize("switch", [None, "CSN_GEMM_NO_256", "CSN_GEMM_NO_DMA"])
def test_scratch_bytes_is_the_mirrors_split_count(clean_env, switch):
    """csn_gemm_tn_scratch_bytes = max(S128, S256 or 0) * M * N * 4, and S128 * M * N * 4 under CSN_GEMM_NO_256 (and
    under CSN_GEMM_NO_DMA, the other switch that takes the 256-tile kernels away)."""
    lib = cabi.load()
    if switch:
        clean_env.setenv(switch, "1")
    off = dict(no_256=switch == "CSN_GEMM_NO_256", no_dma=switch == "CSN_GEMM_NO_DMA")
    shapes = sp.all_shapes()
    assert {(264, 136, 131136), (70, 52, 32833), (128, 128, 32784), (1024, 256, 69696), (1024, 128, 69696)} <= set(shapes)
    for (M, N, K) in shapes:
        s128, s256 = sp.splits_128(M, N, K), sp.splits_256(M, N, K) if sp.uses_256(M, N, K, **off) else 0
        want = max(s128, s256) * M * N * 4
        assert sp.scratch_bytes(M, N, K, **off) == want
        assert lib.csn_gemm_tn_scratch_bytes(M, N, K) == want, (M, N, K, s128, s256)
        if switch:
            assert want == s128 * M * N * 4
    assert os.environ.get("CSN_GEMM_NO_256") == ("1" if switch == "CSN_GEMM_NO_256" else None)


def test_scratch_bytes_along_a_k_sweep(clean_env):
    """The split counts themselves, not only at the chosen K: every multiple of 64 (and the rows next to it, where the
    256-tile kernels do not apply) over the range of the sweep below, at the three (M, N) of the 256-tile cases."""
    lib = cabi.load()
    for (M, N) in sp.MN_256:
        for K in range(8192 - 64, 140000, 64):
            for k in (K, K + 1):
                assert lib.csn_gemm_tn_scratch_bytes(M, N, k) == sp.scratch_bytes(M, N, k), (M, N, k)


def test_sweep_finds_every_tail_of_the_table():
    """(512, 128), K over the multiples of 64 in [8192, 140000]: the 256-tile kernels meet last splits of 64, 128 and 192
    rows and an empty split; and the table of K the GPU file uses is what the formulas give."""
    seen = {}
    for K in range(8192, 140001, 64):
        r = sp.regime(512, 128, K)
        assert r.kernel == "tn256" and sum(r.rows) == K and r.kper % 64 == 0
        seen.setdefault(sp.tail(r), K)
    for want in ((64, 0), (128, 0), (192, 0)):
        assert want in seen, want
    assert any(empty == 1 for (_, empty) in seen), "no K with one empty split"
    assert not any(empty > 1 for (_, empty) in seen)
    print("first K with (last rows, empty splits):", {k: seen[k] for k in ((64, 0), (128, 0), (192, 0))})
    for (M, N) in sp.MN_256:
        for K, (S, last, empty) in sp.K_256.items():
            r = sp.regime(M, N, K)
            assert (r.kernel, r.S, r.kper) == ("tn256", S, 2112) and sp.tail(r) == (last, empty), (M, N, K, sp.describe(r))
            r = sp.regime(M, N, K, no_256=True)
            assert (r.kernel, r.S) == ("tn128", 64), (M, N, K, sp.describe(r))
    assert sp.regime(512, 128, 128000).rows[-2:] == [1280, 0]          # the cfg2 batch (T * B = 500 * 256) at H = 128


def test_cases_at_64_splits_reach_what_their_ids_say():
    for (name, bf16, M, N, K, kernel, kper, last, empty) in sp.CASES_128:
        r = sp.regime(M, N, K, bf16=bf16)
        assert (r.kernel, r.S, r.kper) == (kernel, 64, kper) and sp.tail(r) == (last, empty), (name, sp.describe(r))
        assert sum(r.rows) == K
    assert sp.regime(128, 128, 32784, bf16=False).rows[-2:] == [48, 0]
    for (B, T, C, H, L), (S, last, empty) in sp.LSTM_SHAPES.items():
        for N in (H, C):
            r = sp.regime(4 * H, N, T * B)
            assert (r.kernel, r.S) == ("tn256", S) and sp.tail(r) == (last, empty), (B, T, C, H, sp.describe(r))


def test_operands_are_the_exact_kind():
    a, b = sp.operands(72, 40, 32833)
    assert a.shape == (32833, 72) and b.shape == (32833, 40) and a.dtype == b.dtype == "int8"
    assert set(map(int, set(a.ravel().tolist()))) == {-2, -1, 0, 1, 2} and abs(float(a.mean())) < 0.01
    a2, _ = sp.operands(72, 40, 32833, salt=1)
    assert (a != a2).any()
    assert 4 * max(K for (_, _, K) in sp.all_shapes()) < 2 ** 24
