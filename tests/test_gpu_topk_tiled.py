"""GPU: csn_l2_topk_tiled (csrc/retrieval_tiled.hip) -- bit equality with csn_l2_topk wherever both
apply, k up to 1024 against an exact oracle on inputs whose distances are exact in float64, ties across every tile and
split border, and the public retrieval interface with topK = 100.  The shapes straddle the kernel's 64-query / 64-row
tiles and the split ranges that tests/topk_tiled_reference.py mirrors from the host code."""
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import topk_tiled_reference as ref
from cerebralsignalnetworks_amd import cabi, retrieval
from oracle import retrieval as oracle_retrieval
from test_gpu_stateless_kernels import _check_topk, _gallery

pytestmark = pytest.mark.gpu
SPLITS = (0, 1, 2, 7)


def dev_t(a, cuda):
    return torch.from_numpy(np.ascontiguousarray(a)).to(cuda)


def _tiled(cuda, g, q, k, splits):
    dist, idx, d64 = cabi.l2_topk_tiled(dev_t(g, cuda), dev_t(q, cuda), k, splits=splits, dist64=True)
    return dist.cpu().numpy(), idx.cpu().numpy(), d64.cpu().numpy()


def _old(cuda, g, q, k):
    dist, idx = cabi.l2_topk(dev_t(g, cuda), dev_t(q, cuda), k)
    return dist.cpu().numpy(), idx.cpu().numpy()


def _assert_same_as_old(cuda, g, q, k, what):
    want_d, want_i = _old(cuda, g, q, k)
    for s in SPLITS:
        dist, idx, d64 = _tiled(cuda, g, q, k, s)
        np.testing.assert_array_equal(idx, want_i, err_msg=f"{what} splits={s}: idx")
        np.testing.assert_array_equal(dist, want_d, err_msg=f"{what} splits={s}: dist")
        with np.errstate(over="ignore"):
            np.testing.assert_array_equal(d64.astype(np.float32), dist, err_msg=f"{what} splits={s}: dist64")
    return want_d, want_i


# ---- 5. bit equality with the old kernel ---------------------------------------------------------------------------------
@pytest.mark.parametrize("Ng,Nq,D,k", [(100, 7, 33, 64), (1, 1, 1, 1), (257, 1, 384, 17), (64, 3, 20, 64), (65, 5, 63, 64),
                                       (257, 17, 65, 64), (5000, 3, 384, 64), (37, 19, 1, 37), (1001, 33, 63, 10),
                                       (250, 50, 65, 5), (523, 21, 384, 9)])
def test_tiled_equals_old_kernel_at_its_edges(cuda, Ng, Nq, D, k):
    """The shapes, seeds and planted duplicates of test_gpu_stateless_kernels.test_l2_topk_at_its_edges."""
    g, q = _gallery(Ng, Nq, D, seed=Ng + Nq + D)
    g[Ng // 2] = g[0]
    q[0] = g[0]
    _, idx = _assert_same_as_old(cuda, g, q, k, f"Ng{Ng} Nq{Nq} D{D} k{k}")
    if Ng > 1 and k >= 2:
        assert idx[0, 0] == 0 and idx[0, 1] == Ng // 2


def test_tiled_equals_old_kernel_on_rows_of_magnitude_1e18(cuda):
    """The inputs of test_l2_topk_rows_of_magnitude_1e18: float32 distances overflow, the selection stays exact."""
    Ng, Nq, D, k = 203, 6, 384, 32
    g, q = _gallery(Ng, Nq, D, seed=18)
    g[::5] *= np.float32(1e18)
    q[1] *= np.float32(1e18)
    q[2] = g[5]
    g[9, :] = 0.0
    g[9, 0] = np.float32(1e18)
    dist, idx = _assert_same_as_old(cuda, g, q, k, "1e18 rows")
    assert np.isinf(dist).any() and idx[2, 0] == 5
    d64 = _tiled(cuda, g, q, k, 0)[2]
    assert np.isfinite(d64).all() and (np.diff(d64, axis=1) >= 0).all()


# ---- 6. k > 64 against an exact oracle ----------------------------------------------------------------------------------
def _exact_inputs(Ng, Nq, D, seed):
    """Integers in [-64, 64] / 16: every difference, square and partial sum up to D = 384 is exact in float64."""
    rng = np.random.default_rng(seed)
    return ((rng.integers(-64, 65, (Ng, D)) / 16).astype(np.float32), (rng.integers(-64, 65, (Nq, D)) / 16).astype(np.float32))


@pytest.mark.parametrize("Ng,Nq,D,k", [(300, 5, 24, 65), (1500, 70, 9, 256), (2049, 3, 130, 1024), (1024, 2, 4, 1024),
                                       (4100, 130, 3, 200)])
def test_tiled_large_k_against_exact_oracle(cuda, Ng, Nq, D, k):
    g, q = _exact_inputs(Ng, Nq, D, seed=Ng + k)
    d2 = ((q.astype(np.float64)[:, None, :] - g.astype(np.float64)[None, :, :]) ** 2).sum(axis=2)
    want_i = np.argsort(d2, axis=1, kind="stable")[:, :k]
    want_d = np.take_along_axis(d2, want_i, axis=1)
    for s in SPLITS:
        dist, idx, d64 = _tiled(cuda, g, q, k, s)
        np.testing.assert_array_equal(idx, want_i, err_msg=f"splits={s}")
        np.testing.assert_array_equal(d64, want_d, err_msg=f"splits={s}")
        np.testing.assert_array_equal(dist, want_d.astype(np.float32), err_msg=f"splits={s}")


# ---- 7. ties by construction --------------------------------------------------------------------------------------------
def test_tiled_all_equal_gallery(cuda):
    Ng, Nq, D, k = 1000, 5, 33, 200
    g, q = _gallery(Ng, Nq, D, seed=Ng)
    g[:] = g[0]
    for s in SPLITS:
        _, idx, _ = _tiled(cuda, g, q, k, s)
        np.testing.assert_array_equal(idx, np.broadcast_to(np.arange(k), (Nq, k)), err_msg=f"splits={s}")


@pytest.mark.parametrize("splits", SPLITS)
def test_tiled_duplicates_across_tile_and_split_borders(cuda, splits):
    """Duplicates of gallery row 0 at the last row of a gallery tile and the first of the next, and at the last row of one
    split range and the first of the next (wherever the call has more than one range): lowest index first, for the query
    equal to row 0 and the one 0.25 beside it, as in test_l2_topk_duplicates_on_both_sides_of_the_selection."""
    Ng, Nq, D, k = 1000, 4, 48, 12
    g, q = _gallery(Ng, Nq, D, seed=77)
    ranges = ref.split_ranges(Ng, Nq, splits)
    assert len(ranges) == {0: 16, 1: 1, 2: 2, 7: 6}[splits]
    dups = {0, ref.TILE - 1, ref.TILE, 5 * ref.TILE - 1, 5 * ref.TILE}
    if len(ranges) > 1:
        border = ranges[len(ranges) // 2][0]
        dups |= {border - 1, border, ranges[1][0] - 1, ranges[1][0]}
    dups = sorted(dups)
    assert len(dups) < k
    g[dups] = g[0]
    q[0] = g[0]
    q[1] = g[0] + np.float32(0.25)
    dist, idx, d64 = _tiled(cuda, g, q, k, splits)
    _check_topk(g, q, k, idx, dist, f"duplicates, splits={splits}")
    np.testing.assert_array_equal(idx[0, :len(dups)], dups)
    np.testing.assert_array_equal(idx[1, :len(dups)], dups)


# ---- 8. random normals ---------------------------------------------------------------------------------------------------
def test_tiled_random_normals_k200(cuda):
    Ng, Nq, D, k = 3000, 9, 96, 200
    g, q = _gallery(Ng, Nq, D, seed=8)
    old_d, old_i = _old(cuda, g, q, 64)
    res = {s: _tiled(cuda, g, q, k, s) for s in (1, 5)}
    for a, b in zip(res[1], res[5]):
        np.testing.assert_array_equal(a, b)
    dist, idx, d64 = res[1]
    np.testing.assert_array_equal(idx[:, :64], old_i)
    np.testing.assert_array_equal(dist[:, :64], old_d)
    dd, di = np.diff(d64, axis=1), np.diff(idx, axis=1)
    assert ((dd > 0) | ((dd == 0) & (di > 0))).all(), "(dist64, idx) not strictly increasing"
    # all terms are non-negative; one rounding per fma in the kernel, two per unfused term in numpy: 2 D 2**-53 relative
    want = np.take_along_axis(ref.d2_kernel_order(q, g), idx, axis=1)
    rel = np.abs(d64 - want) / want
    print(f"max relative difference {rel.max():.3e} (bound {2 * D * 2.0 ** -53:.3e})")
    assert (rel <= 2 * D * 2.0 ** -53).all()


# ---- 9. through the public interface -------------------------------------------------------------------------------------
class _DS:
    def __init__(self, ncls):
        self.class_id_to_str = {k: f"class_{k}" for k in range(ncls)}
        self.class_str_to_id = {f"class_{k}": k for k in range(ncls)}


def test_evaluate_full_with_topk_100(cuda):
    ncls, per, nq, D, topK = 40, 30, 200, 48, 100
    rng = np.random.default_rng(100)
    cents = rng.standard_normal((ncls, D)) * 2.0
    gl = np.repeat(np.arange(ncls), per)
    ql = rng.integers(0, ncls, nq)
    gal = (cents[gl] + rng.standard_normal((len(gl), D))).astype(np.float32)
    qry = (cents[ql] + rng.standard_normal((nq, D))).astype(np.float32)
    lab = lambda c: {"ClassId": int(c), "ClassName": f"class_{int(c)}", "imagenetClassId": str(int(c))}
    g_lab, q_lab = [lab(c) for c in gl], [lab(c) for c in ql]
    ds = _DS(ncls)
    r = retrieval.evaluate_full(SimpleNamespace(topK=topK), gal, qry, g_lab, q_lab, ds)
    rec, prec, _, top1, _, I = oracle_retrieval.evaluate(gal, qry, g_lab, q_lab, ds.class_id_to_str, topK=topK)
    assert (r["Recall_Total"], r["Precision_Total"], r["top1"]) == (rec, prec, top1)
    assert r["I"].shape == (nq, topK) and r["D"].dtype == np.float32
    _check_topk(gal, qry, topK, r["I"], r["D"], "evaluate_full topK=100")     # equal to the sort up to rounding-only swaps
    d2 = ref.d2_kernel_order(qry, gal)
    mism = r["I"] != I
    a, b = d2[np.nonzero(mism)[0], r["I"][mism]], d2[np.nonzero(mism)[0], I[mism]]
    assert (np.abs(a - b) <= 1e-12 * b).all()
    # small k: what l2_search returned before the tiled kernel existed
    D5, I5 = retrieval.l2_search(gal, qry, 5)
    old_d, old_i = _old(cuda, gal, qry, 5)
    np.testing.assert_array_equal(I5, old_i)
    np.testing.assert_array_equal(D5, old_d)
    D64, I64 = retrieval.l2_search(gal, qry, 5, dist64=True)
    assert D64.dtype == np.float64
    np.testing.assert_array_equal(I64, old_i)
    np.testing.assert_array_equal(D64.astype(np.float32), old_d)
