"""The weight-gradient GEMM (csn_gemm_tn and the LSTM plans, launch_gemm_tn_slabs in csrc/gemm_tn.hip) where rounding the
rows per K split up leaves the last splits SHORT -- 64 / 128 / 192 rows, i.e. 2 / 4 / 6 ring stages against a prefetch
distance of 3, one row, 48 rows -- or EMPTY, in every kernel that has code for it.

Exact: the operands are integers in {-2, ..., 2}, so every float32 partial sum of every kernel, split count and summation
order is exact (|sum| <= 4 K < 2^24) and the result must have the bits of the float64 product.  No tolerance anywhere at
the GEMM level.  Poisoned: the library is called through ctypes with a scratch buffer of exactly the reported size and a C,
both filled with the NaN pattern 0x7fc00000 and followed by a guard band: an unwritten slab shows as NaN in C (or, in the
stale-data cases, as the previous call's values), a store past the end as a changed guard word.  Every case asserts
through tests/gemm_tn_splits.py, a plain-Python statement of the split formulas, that it reaches the tail its id names.

The column sums (bias gradients) exist only inside an LSTM plan: the same tails there, four-wave kernel against the 8-wave
ring bit for bit, a reused workspace against a fresh one bit for bit, and against float64 torch.nn.LSTM no worse than the
128-tile kernels (different split geometry): the relative-norm error of either plan is the bf16 rounding of the recurrence,
the two differ in float32 summation order only, and the test prints both per tensor."""
import ctypes
import os

import numpy as np
import pytest
import torch

import gemm_tn_splits as sp
from cerebralsignalnetworks_amd import cabi
from gemm_tn_helpers import env, float64_product, plan_backward, plan_create, plan_inputs

pytestmark = pytest.mark.gpu


@pytest.fixture(autouse=True)
def _only_the_switches_of_the_case(monkeypatch):
    """The mirror is told the switches a case sets; none of the others may come in from outside."""
    for name in sp.SWITCHES:
        monkeypatch.delenv(name, raising=False)


GUARD = 1 << 20             # bytes behind the scratch and behind C
POISON = 0x7fc00000         # a float32 NaN


def _poisoned(cuda, nbytes):
    assert nbytes % 4 == 0
    return torch.full(((nbytes + GUARD) // 4,), POISON, dtype=torch.int32, device=cuda)


class _RawGemmTn:
    """csn_gemm_tn as cabi.gemm_tn calls it, but into a scratch of exactly csn_gemm_tn_scratch_bytes and a C that both
    hold NaN and are followed by a guard band.  Create it and call it under the switches of the case."""

    def __init__(self, cuda, M, N, K):
        self.M, self.N, self.K = M, N, K
        self.scratch_bytes = cabi.load().csn_gemm_tn_scratch_bytes(M, N, K)
        self.scratch = _poisoned(cuda, self.scratch_bytes)
        self.c = _poisoned(cuda, M * N * 4)

    def poison_c(self):
        self.c.fill_(POISON)

    def __call__(self, a, b, S):
        """-> C[M, N] (a copy).  S: the split count the mirror expects: exactly S slabs are written, all of each."""
        M, N, K = self.M, self.N, self.K
        assert a.shape == (K, M) and b.shape == (K, N) and a.dtype == b.dtype and a.is_contiguous() and b.is_contiguous()
        cabi._check(cabi.load().csn_gemm_tn(cabi._ptr(a), cabi._ptr(b), ctypes.c_void_p(self.c.data_ptr()), M, N, K,
                                            cabi._dt(a.dtype), ctypes.c_void_p(self.scratch.data_ptr()), cabi._stream()))
        torch.cuda.synchronize()
        words = self.scratch_bytes // 4
        assert bool((self.scratch[words:] == POISON).all()), "the guard band behind the scratch was written"
        assert bool((self.c[M * N:] == POISON).all()), "the guard band behind C was written"
        assert S * M * N <= words
        assert not bool(torch.isnan(self.scratch[:S * M * N].view(torch.float32)).any()), "a slab was not (fully) written"
        assert bool((self.scratch[S * M * N:words] == POISON).all()), "more slabs than the mirror's S were written"
        out = self.c[:M * N].view(torch.float32).view(M, N).clone()
        assert not bool(torch.isnan(out).any()), "C holds NaN"
        return out


@pytest.fixture(scope="module")
def exact(cuda):
    """exact(M, N, K, bf16, salt=0) -> (A, B, a^T b as float32) on the device.  The last two cases are kept (the
    parametrisations run the switches of one shape one after another) and freed with the module: the reference is computed
    once per shape, in float64 by row blocks, and its cast to float32 is checked to be exact."""
    cache = {}

    def case(M, N, K, bf16, salt=0):
        key = (M, N, K, bf16, salt)
        if key not in cache:
            while len(cache) >= 2:
                cache.pop(next(iter(cache)))
            dtype = torch.bfloat16 if bf16 else torch.float32
            a8, b8 = sp.operands(M, N, K, salt)
            a, b = torch.from_numpy(a8).to(cuda).to(dtype), torch.from_numpy(b8).to(cuda).to(dtype)
            want64 = float64_product(a, b)
            want = want64.float()
            assert bool((want.double() == want64).all())
            peak, zeros = float(want64.abs().max()), float((want64 == 0).double().mean())
            print(f"reference {M}x{N}x{K} seed {sp.seed_of(M, N, K, salt)}: max |c| = {peak:.0f}, zeros {100 * zeros:.3f} %")
            assert peak < 2 ** 24, "the exactness argument needs |sum| < 2^24"
            assert zeros < 0.01, "an all-zero slab could pass"
            cache[key] = (a, b, want)
        return cache[key]

    yield case
    cache.clear()


def _bits(t):
    return t.view(torch.int32)


def _run_exact(cuda, exact, M, N, K, bf16, switches, r):
    """Two calls into freshly poisoned buffers under `switches`: both the exact product, bit for bit."""
    a, b, want = exact(M, N, K, bf16)
    with env(**switches):
        got = _RawGemmTn(cuda, M, N, K)(a, b, r.S)
        again = _RawGemmTn(cuda, M, N, K)(a, b, r.S)
    wrong = int((got != want).sum())
    print(f"{M}x{N}x{K} {'bf16' if bf16 else 'f32'} {switches}: {sp.describe(r)}; elements differing from the exact "
          f"product {wrong}, from the rerun {int((_bits(got) != _bits(again)).sum())}")
    np.testing.assert_array_equal(got.cpu().numpy(), want.cpu().numpy())
    assert torch.equal(_bits(got), _bits(again))
    return got


def _id_256(M, N, K, envname):
    S, last, empty = sp.K_256[K]
    return f"{M}x{N}-K{K}-S{S}-last{last}-empty{empty}-{envname}"


@pytest.mark.parametrize("M,N,K,envname,switches",
                         [pytest.param(M, N, K, name, switches, id=_id_256(M, N, K, name))
                          for (M, N) in sp.MN_256 for K in sp.K_256 for (name, switches) in sp.ENVS_256])
def test_256_tile_kernels_short_and_empty_last_splits_exact(cuda, exact, M, N, K, envname, switches):
    """Four-wave kernel, 8-wave rings of 4 / 3 / 5 stages and (CSN_GEMM_NO_256) the 128-tile kernel with and without
    transposing reads, where the last non-empty split of the 256-tile kernels has 6 / 4 / 2 ring stages or is followed
    by an empty one: all the exact product, hence all equal."""
    no_256 = "CSN_GEMM_NO_256" in switches
    r = sp.regime(M, N, K, no_256=no_256)
    if no_256:
        assert (r.kernel, r.S) == ("tn128", 64), sp.describe(r)
    else:
        S, last, empty = sp.K_256[K]
        assert (r.kernel, r.S, r.kper) == ("tn256", S, 2112) and sp.tail(r) == (last, empty), sp.describe(r)
        assert last % 32 == 0 and last // 32 in (2, 4, 6, 66)          # ring stages of the last non-empty split
    _run_exact(cuda, exact, M, N, K, True, switches, r)


@pytest.mark.parametrize("name,bf16,M,N,K,kernel,kper,last,empty", [pytest.param(*c, id=c[0]) for c in sp.CASES_128])
def test_128_tile_and_generic_kernels_at_64_splits_exact(cuda, exact, name, bf16, M, N, K, kernel, kper, last, empty):
    """S = 64 with up to seven empty splits, a one-row split, a 48-row split of the float32 128-tile kernel, ragged
    tiles, and the generic kernel (M % 8 != 0, or float32 off the 128-tile grid) with splits."""
    r = sp.regime(M, N, K, bf16=bf16)
    assert (r.kernel, r.S, r.kper) == (kernel, 64, kper) and sp.tail(r) == (last, empty), sp.describe(r)
    _run_exact(cuda, exact, M, N, K, bf16, {}, r)


@pytest.mark.parametrize("M,N,K", [(512, 128, 69696), (512, 256, 131136)])
def test_stale_scratch_does_not_survive_a_second_call(cuda, exact, M, N, K):
    """Default kernel, one empty split: a second product with other operands into the SAME scratch, not poisoned again
    (C is) -- a slab the second call left unwritten would hold the first call's values and go unnoticed by the NaN
    check.  The second result is the second exact product, and so is a third call with the second operands."""
    r = sp.regime(M, N, K)
    assert r.kernel == "tn256" and sp.tail(r)[1] == 1, sp.describe(r)
    a1, b1, want1 = exact(M, N, K, True)
    a2, b2, want2 = exact(M, N, K, True, salt=1)
    assert int((want1 != want2).sum()) > 0.98 * M * N
    raw = _RawGemmTn(cuda, M, N, K)
    np.testing.assert_array_equal(raw(a1, b1, r.S).cpu().numpy(), want1.cpu().numpy())
    raw.poison_c()
    got = raw(a2, b2, r.S)
    raw.poison_c()
    again = raw(a2, b2, r.S)
    print(f"{M}x{N}x{K} second call into the same scratch: {sp.describe(r)}; elements differing from the second exact "
          f"product {int((got != want2).sum())}, from the rerun {int((_bits(got) != _bits(again)).sum())}")
    np.testing.assert_array_equal(got.cpu().numpy(), want2.cpu().numpy())
    assert torch.equal(_bits(got), _bits(again))


# ---- the same tails through an LSTM plan (column sums = bias gradients) -----------------------------------------------
LSTM_IDS = [f"B{s[0]}-T{s[1]}-C{s[2]}-H{s[3]}-L{s[4]}-S{v[0]}-last{v[1]}-empty{v[2]}" for s, v in sp.LSTM_SHAPES.items()]


def _second_dy(cuda, B, T, H):
    g = torch.Generator(device=cuda).manual_seed(7 * (B + T + H) + 1)
    return torch.randn(B, T, H, device=cuda, generator=g) * 0.1, torch.randn(B, H, device=cuda, generator=g)


def _float64_lstm_gradients(params, x, dy_all, dy_last):
    """The gradients of plan_backward from float64 torch.nn.LSTM on the CPU: <y_all, dy_all> + <y_all[:, -1], dy_last>."""
    w_ih = params[0]
    L, H, C = len(w_ih), w_ih[0].shape[0] // 4, w_ih[0].shape[1]
    ref = torch.nn.LSTM(C, H, num_layers=L, batch_first=True).double()
    names = ("weight_ih", "weight_hh", "bias_ih", "bias_hh")
    ref.load_state_dict({f"{n}_l{l}": group[l].double().cpu() for n, group in zip(names, params) for l in range(L)})
    y, _ = ref(x.double().cpu())
    ((y * dy_all.double().cpu()).sum() + (y[:, -1] * dy_last.double().cpu()).sum()).backward()
    short = dict(zip(names, ("dw_ih", "dw_hh", "db_ih", "db_hh")))
    return {f"{short[n]}_l{l}": getattr(ref, f"{n}_l{l}").grad.numpy() for n in names for l in range(L)}


@pytest.fixture(scope="module", params=list(sp.LSTM_SHAPES), ids=LSTM_IDS)
def lstm_runs(request, cuda):
    """(shape, gradients by run and name, as numpy) of one shape, computed once for the tests below and freed after them:
    `w4` the default plan, `w4_second` its second backward with another dy on the same workspace, `ring` a
    CSN_TN_NO_STAGGER plan, `fresh_second` a fresh default plan given only the second dy, `tn128` a CSN_GEMM_NO_256
    plan, `float64` torch.nn.LSTM in float64 on the CPU; plan.status() == 0 after every call (plan_backward).

    The float64 torch.nn.LSTM reference at T above 1000 takes a few seconds on the CPU and is computed once per shape."""
    shape = request.param
    B, T, C, H, L = shape
    outside = {name: os.environ.pop(name) for name in sp.SWITCHES if name in os.environ}     # module scope: this runs
    try:                                                                                     # before the per-test fixture
        params, x, dy_all, dy_last = plan_inputs(cuda, B, T, C, H, L)
        dy_all2, dy_last2 = _second_dy(cuda, B, T, H)
        runs = {}
        plan = plan_create(cuda, B, T, C, H, L, {}, params, x)
        runs["w4"] = plan_backward(plan, params, dy_last, dy_all)
        runs["w4_second"] = plan_backward(plan, params, dy_last2, dy_all2)
        del plan
        runs["ring"] = plan_backward(plan_create(cuda, B, T, C, H, L, {"CSN_TN_NO_STAGGER": "1"}, params, x), params,
                                     dy_last, dy_all)
        runs["fresh_second"] = plan_backward(plan_create(cuda, B, T, C, H, L, {}, params, x), params, dy_last2, dy_all2)
        runs["tn128"] = plan_backward(plan_create(cuda, B, T, C, H, L, {"CSN_GEMM_NO_256": "1"}, params, x), params,
                                      dy_last, dy_all)
    finally:
        os.environ.update(outside)
    runs["float64"] = _float64_lstm_gradients(params, x, dy_all, dy_last)
    return shape, runs


def _assert_lstm_regime(shape):
    B, T, C, H, L = shape
    S, last, empty = sp.LSTM_SHAPES[shape]
    for N in (H, C):                   # (4H, H, T B): recurrent and upper-layer input weights; (4H, C, T B): layer 0's
        r = sp.regime(4 * H, N, T * B)
        assert (r.kernel, r.S) == ("tn256", S) and sp.tail(r) == (last, empty), sp.describe(r)
        print(f"LSTM {shape}: weight gradient {4 * H}x{N}x{T * B}: {sp.describe(r)}")
        r = sp.regime(4 * H, N, T * B, no_256=True)
        assert (r.kernel, r.S) == ("tn128", 64), sp.describe(r)


def test_lstm_tails_four_wave_ring_and_reused_workspace_bit_for_bit(lstm_runs):
    shape, runs = lstm_runs
    _assert_lstm_regime(shape)
    L = shape[4]
    for name, v in runs["w4"].items():
        assert np.isfinite(v).all() and np.abs(v).max() > 0, name
        np.testing.assert_array_equal(v, runs["ring"][name], err_msg=f"{name}: four-wave kernel against the 8-wave ring")
    # db_ih and db_hh are two stores of ONE value: one reduction of one set of column-sum rows writes both (lstm.hip,
    # weight_grads: launch_reduce_slabs_unperm(..., db_ih[l], db_hh[l], ...)).  Their equality is therefore weak by
    # construction -- it holds only that both were stored; what checks the column-sum rows themselves are the
    # comparisons with the ring above and with the fresh plan below, and the float64 test.
    for key in ("w4", "w4_second", "ring", "tn128"):
        for l in range(L):
            np.testing.assert_array_equal(runs[key][f"db_ih_l{l}"], runs[key][f"db_hh_l{l}"], err_msg=f"{key} layer {l}")
    # a second backward on the same plan: whatever the first left in the slabs and column-sum rows must be gone
    changed = 0
    for name, v in runs["w4_second"].items():
        np.testing.assert_array_equal(v, runs["fresh_second"][name], err_msg=f"{name}: reused against fresh workspace")
        changed += int((v != runs["w4"][name]).sum())
    assert changed > 0.9 * sum(v.size for v in runs["w4"].values()), "the second dy must change the gradients"


def _rel(got, want):
    return float(np.linalg.norm(got.astype(np.float64) - want) / np.linalg.norm(want))


def test_lstm_tails_no_worse_against_float64_than_the_128_tile_kernels(lstm_runs):
    """The default plan and a CSN_GEMM_NO_256 plan (128-tile kernels, S = 64, column sums from their own kernel; covered
    by the existing tests) differ in float32 summation order only.  The bound is not chosen in advance: per tensor, the
    relative-norm error of the default plan against float64 nn.LSTM is at most 1.25 x the measured error of the other."""
    shape, runs = lstm_runs
    _assert_lstm_regime(shape)
    want = runs["float64"]
    failed = []
    for name in sorted(want):
        e256, e128 = _rel(runs["w4"][name], want[name]), _rel(runs["tn128"][name], want[name])
        print(f"LSTM {shape} {name}: rel. norm error vs float64 nn.LSTM: default {e256:.6e}, CSN_GEMM_NO_256 {e128:.6e}, "
              f"ratio {e256 / e128:.5f}")
        if not (e128 > 0 and e256 <= 1.25 * e128):
            failed.append((name, e256, e128))
    assert not failed, failed
