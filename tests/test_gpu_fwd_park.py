"""GPU: the H = 768 weight-stationary forward with a short h ring and its waiting registers parked in LDS (DESIGN.md
section 3.4 (i)).

By default lstm_fwd_persist_kernel<6,6> with data polls keeps two k-block groups of a step's h tile in flight and parks
the register set that only waits during the MFMAs in LDS; CSN_NO_FWD_PARK=1 keeps the ring of four with that set in
registers.  Both forms run the same MFMAs in the same order on the same operands and the same epilogue
arithmetic, so every output of forward + backward must be the same BITS either way: y_all (and with it y_last),
(h_n, c_n), dx, (dh0, dc0) where a state is given, and the four gradients of every layer.  The launch schedule does not
change: kernel_names() and half_tile_launches agree, and the plan's status words are 0 after every call."""
import os

import numpy as np
import pytest
import torch

from cerebralsignalnetworks_amd import LSTM

pytestmark = pytest.mark.gpu

BF16 = torch.bfloat16
H = 768           # the only hidden size whose forward is <6,6>


def _run(shape, env, state, train, seed):
    B, T, C, L = shape
    old = {k: os.environ.get(k) for k in env}
    os.environ.update(env)
    try:
        dev = torch.device("cuda:0")
        torch.manual_seed(seed)                    # same parameters and inputs in every run of a case
        m = LSTM(C, H, L, compute_dtype=BF16).to(dev)
        g = torch.Generator().manual_seed(seed + 1)
        x = torch.randn(B, T, C, generator=g).to(dev).requires_grad_(train)
        dy = (torch.randn(B, T, H, generator=g) * 0.1).to(dev)
        dh = torch.randn(L, B, H, generator=g).to(dev)
        dc = torch.randn(L, B, H, generator=g).to(dev)
        hx = None
        if state:
            hx = tuple((torch.randn(L, B, H, generator=g) * 0.5).to(dev).requires_grad_(train) for _ in range(2))
        with torch.enable_grad() if train else torch.no_grad():
            y, (h_n, c_n) = m(x, hx)
            if train:
                ((y * dy).sum() + (h_n * dh).sum() + (c_n * dc).sum()).backward()
        torch.cuda.synchronize()
        plans = m.all_plans()
        assert len(plans) == 1
        plan = plans[0]
        assert plan.status() == 0, "status words not 0: a bounded in-kernel wait timed out, or a non-finite gradient"
        out = dict(y_all=y, y_last=y[:, -1], h_n=h_n, c_n=c_n)
        if train:
            out["dx"] = x.grad
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


def _compare(shape, form, state, train, seed=5):
    got = {}
    for label, env in (("parked", form), ("ring4", {**form, "CSN_NO_FWD_PARK": "1"})):
        got[label] = _run(shape, env, state, train, seed)
    (new, new_half, new_names), (old, old_half, old_names) = got["parked"], got["ring4"]
    what = f"{shape} {form or 'default'} state={state} train={train}"
    assert new_names == old_names, (what, new_names, old_names)
    assert new_names[0] == "lstm_fwd_persist_kernel", (what, new_names)
    assert new_half == old_half, (what, new_half, old_half)
    assert set(new) == set(old)
    for k in new:
        assert np.isfinite(new[k]).all(), (what, k)
        _same_bits(new[k], old[k], f"{what}: {k}")


# B = 130: Bpad = 192, one 32-row tile partly and one all padding; B = 256: the steady 64-row geometry of two layers.
# T = 70 with the default chunk of 32: three chunks -- launch boundaries, the first step without a wait, and the fill,
# steady and drain row heights.  C = 128: the layer-0 projection fused into the recurrence; C = 96: the plain layer 0.
@pytest.mark.parametrize("C", [128, 96])
@pytest.mark.parametrize("L", [1, 2])
@pytest.mark.parametrize("T", [3, 33, 70])
@pytest.mark.parametrize("B", [1, 40, 130, 256])
def test_parked_form_gives_the_bits_of_the_ring_of_four(B, T, L, C):
    for train in (True, False):
        _compare((B, T, C, L), {}, False, train)


@pytest.mark.parametrize("shape", [(130, 70, 128, 2), (256, 33, 96, 2), (40, 70, 96, 1), (1, 3, 128, 1)])
def test_parked_form_with_an_initial_state(shape):
    """h0 / c0 given: step 0 multiplies h0 from slot 0 without a wait, and the cell state starts from c0."""
    for train in (True, False):
        _compare(shape, {}, True, train)


@pytest.mark.parametrize("form", [{"CSN_DPOLL_NO_HINT": "1"}, {"CSN_FWD_HINT": "1"}], ids=["no_hint", "fwd_hint"])
@pytest.mark.parametrize("shape", [(256, 70, 128, 2), (130, 33, 96, 2)])
def test_parked_form_on_both_poll_paths(shape, form):
    """Without hint words every step goes through the re-read path (the forward's default, and with CSN_DPOLL_NO_HINT=1 the
    backward's too); CSN_FWD_HINT=1 makes the forward poll a hint word per producer first."""
    _compare(shape, form, False, True)
    _compare(shape, form, True, True)
