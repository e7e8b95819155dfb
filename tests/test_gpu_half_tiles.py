"""GPU: 32-row hand-off groups in the weight-stationary LSTM launches that have few groups.

A grouped launch with `ns` layers in range runs on 32-row groups, 2 MT per layer, when 2 ns MT <= 8 -- the fill and drain
launches of the (layer, chunk) wavefront at B = 256, every launch of a small batch -- and on 64-row groups otherwise;
CSN_NO_HALF_TILES=1 keeps 64 rows everywhere.  A row's arithmetic does not depend on the rows that share its tile, so
every output of forward + backward must be the same BITS either way: y_all, (h_n, c_n), dx, (dh0, dc0) where a state is
given, and the four gradients of every layer.  csn_lstm_plan_half_tile_launches proves which launches took the new path:
the counts are derived here from the launch geometry and compared, not just "some"."""
import os

import numpy as np
import pytest
import torch

from cerebralsignalnetworks_amd import LSTM

pytestmark = pytest.mark.gpu

BF16 = torch.bfloat16


def _expected_half_launches(B, T, H, L, chunk, env, lengths):
    """(forward, backward) launches on 32-row groups, from the schedule of forward_persist / backward_persist (lstm.hip):
    diagonal dg holds layer l at chunk dg - l (forward) or at reverse chunk dg - lag (L - 1 - l) (backward)."""
    MT = (B + 63) // 64
    nch = (T + chunk - 1) // chunk
    if "CSN_NO_HALF_TILES" in env:
        return 0, 0
    def count(lag):
        n = 0
        for dg in range(nch + lag * (L - 1)):
            ns = sum(1 for l in range(L) if 0 <= dg - lag * l < nch)
            n += 1 if ns > 0 and 2 * ns * MT <= 8 else 0
        return n
    fwd = 0 if H == 1024 else count(1)             # H = 1024: the N-split forward kernel, which has no 32-row groups
    beside = 1 < L <= 4 and H // 32 <= 28 and "CSN_NO_BESIDE" not in env
    bwd = 0 if lengths is not None else count(2 if beside else 1)      # a batch with lengths: the backward stays on 64 rows
    return fwd, bwd


def _run(shape, chunk, env, state, lengths, seed):
    B, T, C, H, L = shape
    env = {"CSN_LSTM_CHUNK": str(chunk), **env}
    old = {k: os.environ.get(k) for k in env}
    os.environ.update(env)
    try:
        dev = torch.device("cuda:0")
        torch.manual_seed(seed)                    # same parameters and inputs in every run of a case
        m = LSTM(C, H, L, compute_dtype=BF16).to(dev)
        g = torch.Generator().manual_seed(seed + 1)
        x = torch.randn(B, T, C, generator=g).to(dev).requires_grad_(True)
        dy = (torch.randn(B, T, H, generator=g) * 0.1).to(dev)
        dh = torch.randn(L, B, H, generator=g).to(dev)
        dc = torch.randn(L, B, H, generator=g).to(dev)
        hx = None
        if state:
            hx = tuple((torch.randn(L, B, H, generator=g) * 0.5).to(dev).requires_grad_(True) for _ in range(2))
        y, (h_n, c_n) = m(x, hx, lengths=lengths)
        ((y * dy).sum() + (h_n * dh).sum() + (c_n * dc).sum()).backward()
        torch.cuda.synchronize()
        plans = m.all_plans()
        assert len(plans) == 1
        plan = plans[0]
        assert plan.status() == 0, "status words not 0: a bounded in-kernel wait timed out, or a non-finite gradient"
        out = dict(y_all=y, h_n=h_n, c_n=c_n, dx=x.grad)
        if state:
            out.update(dh0=hx[0].grad, dc0=hx[1].grad)
        for n, q in m.named_parameters():
            out[n] = q.grad
        assert len([n for n in out if n.startswith(("weight_", "bias_"))]) == 4 * L
        out = {k: v.detach().cpu().numpy() for k, v in out.items()}
        return out, (plan.half_tile_launches(0), plan.half_tile_launches(1)), plan.kernel_names()
    finally:
        for k, v in old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


def _same_bits(a, b, what):
    if np.array_equal(a, b, equal_nan=True):
        return
    bad = np.argwhere(a != b)
    axes = [sorted(set(bad[:, i].tolist()))[:12] for i in range(bad.shape[1])]
    raise AssertionError(f"{what}: {len(bad)} of {a.size} elements differ, max |diff| {np.abs(a - b).max():.3g}; "
                         f"indices per axis (first 12): {axes}")


# name: (B, T, C, H, L), chunk, initial state given, hand-off forms to repeat the comparison under
CASES = {
    # the cfg2 geometry: forward fill and drain, backward launches 0 / 1 (layer 1) and the two drain launches (layer 0), of
    # which launch 1 and the first drain launch carry a pending input-gradient GEMM; the 8-step last chunk is a drain launch
    "cfg2_geometry": ((256, 72, 128, 768, 2), 32, False,
                      ({}, {"CSN_NO_XCD_LOCAL": "1"}, {"CSN_FWD_FLAGS": "1", "CSN_BWD_FLAGS": "1"}, {"CSN_DPOLL_NO_HINT": "1"})),
    # Bpad = 192: tile 4 (rows 128..159) is partly padding, tile 5 (rows 160..191) all padding
    "partly_and_all_padding": ((130, 40, 128, 768, 2), 32, True, ({}, {"CSN_FWD_FLAGS": "1", "CSN_BWD_FLAGS": "1"})),
    "every_launch_half": ((64, 40, 128, 768, 2), 32, False, ({}, {"CSN_DPOLL_NO_HINT": "1"}, {"CSN_NO_BESIDE": "1"})),
    "narrow_h256": ((200, 40, 32, 256, 2), 16, False, ({},)),
    "h1024_backward_only": ((256, 40, 128, 1024, 2), 16, False, ({},)),
    # three layers of two M-tiles: 1 and 2 layers in range run on 32 rows (4 and 8 groups), 3 layers on 64 (6 groups)
    "three_layers": ((128, 40, 64, 768, 3), 8, True, ({}, {"CSN_NO_XCD_LOCAL": "1"})),
}


@pytest.mark.parametrize("name", list(CASES))
def test_half_tiles_give_the_bits_of_64_row_groups(name):
    shape, chunk, state, forms = CASES[name]
    B, T, C, H, L = shape
    for form in forms:
        got = {}
        for label, env in (("half", form), ("full", {**form, "CSN_NO_HALF_TILES": "1"})):
            out, counts, kernels = _run(shape, chunk, env, state, None, seed=7)
            want = _expected_half_launches(B, T, H, L, chunk, env, None)
            print(f"{name} {form or 'default'} {label}: 32-row launches (fwd, bwd) {counts}, expected {want}; kernels {kernels}")
            assert counts == want, (name, form, label, counts, want)
            assert kernels[1] == "lstm_bwd_persist_kernel" and kernels[0] == ("lstm_fwd_ns_kernel" if H == 1024 else "lstm_fwd_persist_kernel")
            got[label] = out
        want_half = _expected_half_launches(B, T, H, L, chunk, form, None)
        assert want_half[1] > 0 and (want_half[0] > 0 or H == 1024), "the case does not reach the 32-row path"
        assert set(got["half"]) == set(got["full"])
        for k in got["half"]:
            assert np.isfinite(got["half"][k]).all(), k
            _same_bits(got["half"][k], got["full"][k], f"{name} {form or 'default'}: {k}")


def test_half_tiles_with_lengths():
    """A batch with lengths: the forward (which has no masked instantiation -- padding is masked outside the recurrence)
    takes 32-row groups, the masked backward stays on 64 rows; same bits as with the switch."""
    shape, chunk = (256, 72, 128, 768, 2), 32
    B, T, C, H, L = shape
    rng = np.random.default_rng(11)
    lengths = [int(v) for v in rng.integers(0, T + 1, B)]
    lengths[0], lengths[1], lengths[B - 1] = T, 0, 33
    got = {}
    for label, env in (("half", {}), ("full", {"CSN_NO_HALF_TILES": "1"})):
        out, counts, _ = _run(shape, chunk, env, True, lengths, seed=9)
        want = _expected_half_launches(B, T, H, L, chunk, env, lengths)
        print(f"lengths {label}: 32-row launches (fwd, bwd) {counts}, expected {want}")
        assert counts == want, (label, counts, want)
        got[label] = out
    assert _expected_half_launches(B, T, H, L, chunk, {}, lengths)[0] > 0
    for k in got["half"]:
        _same_bits(got["half"][k], got["full"][k], f"lengths: {k}")
