"""No GPU: the case generator of tests/lstm_feature_fuzz.py (determinism, legality, what the committed (seed, n) covers)
and its reference validating itself against float64 torch.nn.LSTM at tiny shapes -- with lengths through
pack_padded_sequence, with state, a reverse plan against the reverse half of nn.LSTM(bidirectional=True), dropout through
a chain of single-layer nn.LSTMs with the library's host mask, and argument subsets against autograd with the omitted
terms left out of the loss."""
import numpy as np
import pytest
import torch

import bilstm_reference as bref
import dropout_reference as dref
import lengths_reference as lref
import lstm_feature_fuzz as fz
import test_gpu_bilstm as tb
import test_gpu_lstm_lengths as tl
import test_gpu_lstm_state as st


def test_cases_are_deterministic_and_legal():
    a, b = fz.cases(fz.SEED, fz.N), fz.cases(fz.SEED, fz.N)
    assert a == b and len(a) == fz.N
    assert fz.cases(fz.SEED, 8) == a[:8] and fz.cases(fz.SEED + 1, fz.N) != a
    assert len({c["id"] for c in a}) == fz.N
    for c in a:
        fz.check_legal(c)
        assert set(fz.features(c)) == set(fz.FEATURES)


def test_the_committed_draw_covers_every_feature_pair_regime_and_path():
    """The condition on (SEED, N).  If it does not hold, another seed or a larger n is the remedy, not a weaker condition."""
    cs = fz.cases(fz.SEED, fz.N)
    on = {f: sum(fz.features(c)[f] for c in cs) for f in fz.FEATURES}
    assert min(on.values()) >= 6, on
    pairs = fz.pair_counts(cs)
    assert len(pairs) == len(fz.FEATURES) * (len(fz.FEATURES) - 1) // 2
    assert min(pairs.values()) >= 2, {k: v for k, v in pairs.items() if v < 2}
    drawn = {r: sum(c["regime"] == r for c in cs) for r in fz.REGIMES}
    assert min(drawn.values()) >= 2, drawn
    # the regimes are the environments and sizes of the two tables, with and without state
    for name, (shape, dtype, _, env) in st.CASES.items():
        assert any((H, d == "bf16", e) == (shape[3], dtype == st.BF16, env) for H, d, e, _ in fz.REGIMES.values()), name
    assert {k for _, _, e, _ in fz.REGIMES.values() for k in e} == {
        "CSN_CELL_V1", "CSN_NO_PERSIST", "CSN_NO_PERSIST_BWD", "CSN_FWD_FLAGS", "CSN_BWD_FLAGS", "CSN_NO_BESIDE", "CSN_FWD_NSPLIT",
        "CSN_LSTM_CHUNK"}
    assert {s for *_, s in fz.REGIMES.values()} == {True, False}
    # every length pattern on a reverse plan
    rev = {c["pattern"] for c in cs if c["reverse"] and c["lengths"] is not None}
    assert rev == set(tl.PATTERNS), set(tl.PATTERNS) - rev
    # stateless float32 plans on the weight-stationary path 4 with set_io or reverse
    p4 = [c for c in cs if fz.expected_plan(c)[0] == 4 and (c["reverse"] or c["y_pitch"] or c["dy_pitch"] or c["dx_add"])]
    assert len(p4) >= 3
    # every (path, kernels) triple the two tables expect, by the mirror of make_layout (the GPU test asks the real plans)
    want = {e for _, _, e, _ in st.CASES.values() if e is not st.PLAIN} | {tb.PLAN_CASES["f32_path4_stateless"][2]}
    taken = [fz.expected_plan(c) for c in cs]
    assert all(taken.count(e) >= 2 for e in want), {e: taken.count(e) for e in want}
    # ... and the shape edges: every B and I value, T on both sides of a chunk edge and of step 32
    assert {c["B"] for c in cs} == set(fz.B_VALUES) and {c["I"] for c in cs} == set(fz.I_VALUES)
    assert {31, 32, 33} <= {c["T"] for c in cs} and {1, 2} <= {c["T"] for c in cs}
    assert {c["L"] for c in cs} == set(range(1, 6))
    assert {c["dropout"][0] for c in cs if c["dropout"]} == set(fz.P_VALUES)


def test_expected_plan_reproduces_the_tables():
    """The mirror of make_layout gives the plan each table entry expects at the entry's own shape."""
    for name, (shape, dtype, expect, env) in st.CASES.items():
        if expect is st.PLAIN:
            continue
        B, T, I, H, L = shape
        c = dict(B=B, T=T, I=I, H=H, L=L, dtype="bf16" if dtype == st.BF16 else "f32", env=env, state=True)
        assert fz.expected_plan(c) == expect, name
    for name, (shape, dtype, expect, env, state) in tb.PLAN_CASES.items():
        B, T, I, H, L = shape
        c = dict(B=B, T=T, I=I, H=H, L=L, dtype="bf16" if dtype == st.BF16 else "f32", env=env, state=state)
        assert fz.expected_plan(c) == expect, name


# ---- the reference against float64 torch.nn.LSTM ------------------------------------------------------------------------
def _tiny(**kw):
    c = dict(regime=None, H=8, dtype="f32", env={}, state=True, B=5, T=6, I=3, L=2, reverse=False, dropout_plan=False,
             dropout=None, pattern=None, lengths=None, edges=(31, 32, 33), outputs=st._OUT_KEYS, grads_in=st._BWD_IN,
             state_in=("h0", "c0"), state_grads_out=("dh0", "dc0"), want_dx=True, y_pitch=False, dy_pitch=False, y_half=0,
             dy_half=0, dx_add=False, x_view=None, accumulate=False, callback=False, data_seed=3)
    c.update(kw)
    return c


def _close(got, want, what):
    for k, w in want.items():
        w = w.detach().numpy() if torch.is_tensor(w) else np.asarray(w)
        assert got[k].shape == w.shape, (what, k)
        # (the inputs are float32 values and dy_last is added in float32, as the library adds it: 1e-6, not 1e-12)
        assert np.abs(got[k] - w).max() <= 1e-6 * max(1.0, np.abs(w).max()), (what, k, float(np.abs(got[k] - w).max()))


def _nn_lstm(c, a):
    ref = torch.nn.LSTM(c["I"], c["H"], c["L"], batch_first=True).double()
    ref.load_state_dict({k: v.double() for k, v in a["lp"].items()})
    return ref


def _nn_want(res, c):
    """The keys of reference() from a dict with the keys of lengths_reference.packed_nn_lstm."""
    want = {k: v for k, v in res.items() if k != "out"}
    want["y_all"], want["y_last"] = res["out"], res["h_n"][c["L"] - 1]
    return want


LENGTHS = [6, 0, 3, 1, 6]


@pytest.mark.parametrize("lengths", [None, LENGTHS], ids=["dense", "ragged"])
def test_reference_is_packed_float64_nn_lstm_with_state(lengths):
    c = _tiny(lengths=lengths, grads_in=("dy_all", "dh_n", "dc_n"))
    a = fz.make_inputs(c)
    d = lambda k: a[k].double()      # noqa: E731
    res = lref.packed_nn_lstm(_nn_lstm(c, a), d("x"), lengths or [c["T"]] * c["B"], d("h0"), d("c0"), d("dy_all"), d("dh_n"), d("dc_n"))
    _close(fz.reference(c, a), _nn_want(res, c), f"lengths={lengths}")


@pytest.mark.parametrize("lengths", [None, LENGTHS], ids=["dense", "ragged"])
def test_reverse_reference_is_the_reverse_half_of_a_bidirectional_nn_lstm(lengths):
    c = _tiny(L=1, reverse=True, lengths=lengths, grads_in=("dy_all", "dh_n", "dc_n"))
    a = fz.make_inputs(c)
    B, T, H = c["B"], c["T"], c["H"]
    torch.manual_seed(1)
    bi = torch.nn.LSTM(c["I"], H, 1, batch_first=True, bidirectional=True).double()
    bi.load_state_dict({**{k: v.detach() for k, v in bi.state_dict().items()}, **{k + "_reverse": v.double() for k, v in a["lp"].items()}})
    g = torch.Generator().manual_seed(2)
    other = lambda t: torch.randn(t.shape, generator=g, dtype=torch.float64)      # noqa: E731
    h0, c0 = (torch.cat([other(a[k]), a[k].double()]) for k in ("h0", "c0"))
    # the forward direction's outputs get no gradient: what reaches x comes through the reverse direction alone
    dy = torch.cat([torch.zeros(B, T, H, dtype=torch.float64), a["dy_all"].double()], dim=2)
    dh, dc = (torch.cat([torch.zeros(1, B, H, dtype=torch.float64), a[k].double()]) for k in ("dh_n", "dc_n"))
    res = bref.nn_bilstm_f64(bi, a["x"].double(), lengths, h0, c0, dy, dh, dc)
    want = dict(y_all=res["out"][:, :, H:], y_last=res["h_n"][1], h_n=res["h_n"][1:], c_n=res["c_n"][1:], dx=res["dx"],
                dh0=res["dh0"][1:], dc0=res["dc0"][1:], **{k: res[k + "_reverse"] for k in a["lp"]})
    _close(fz.reference(c, a), want, f"reverse lengths={lengths}")
    if lengths is None:          # y_last of a reverse plan is its output at time 0
        assert np.array_equal(fz.reference(c, a)["y_last"], fz.reference(c, a)["y_all"][:, 0])


@pytest.mark.parametrize("reverse", [False, True], ids=["plain", "reverse"])
@pytest.mark.parametrize("p", [0.5, 1.0])
def test_dropout_reference_is_the_nn_lstm_chain_with_the_host_mask(p, reverse):
    c = _tiny(L=3, reverse=reverse, dropout_plan=True, dropout=(p, 0x1234567, 2), grads_in=("dy_all", "dh_n", "dc_n"))
    a = fz.make_inputs(c)
    masks = fz.host_masks(c)
    B, T, H, L = c["B"], c["T"], c["H"], c["L"]
    assert masks.shape == (L - 1, B, T, H) and np.array_equal(masks, dref.interface_masks(0x1234567, 2, p, L, T, B, H))
    assert (p < 1.0) == bool(masks.any())
    flip = bref.R if reverse else (lambda t: t)
    # the mask is indexed by recurrence step: the chain runs on reversed data with the mask as it is
    res = dref.nn_lstm_chain({k: v.numpy() for k, v in a["lp"].items()}, L, flip(a["x"]).numpy(), a["h0"].numpy(), a["c0"].numpy(),
                             flip(a["dy_all"]).numpy(), a["dh_n"].numpy(), a["dc_n"].numpy(), masks, dref.scale(p))
    want = _nn_want(res, c)
    want["y_all"], want["dx"] = flip(torch.from_numpy(res["out"])), flip(torch.from_numpy(res["dx"]))
    got = fz.reference(c, a)
    _close(got, want, f"p={p} reverse={reverse}")
    if reverse:                  # ... and a mask indexed by the caller's time is another network
        by_time = fz.reference(c, a, masks=np.ascontiguousarray(masks[:, :, ::-1]))
        assert (p < 1.0) == (np.abs(by_time["y_all"] - got["y_all"]).max() > 1e-3)


@pytest.mark.parametrize("reverse", [False, True], ids=["plain", "reverse"])
def test_argument_subsets_are_the_loss_without_the_omitted_terms(reverse):
    """Every subset of (h0, c0) x every non-empty subset of the incoming gradients, ragged: autograd through float64
    nn.LSTM on R(x) with only the given terms in the loss; y_last = h_n of the top layer, so dy_last of an empty row
    reaches dh0."""
    lengths = LENGTHS
    flip = (lambda t: bref.R(t, lengths)) if reverse else (lambda t: t)
    for state_in in st._FWD_SUBSETS:
        for gin in st._BWD_SUBSETS:
            c = _tiny(reverse=reverse, lengths=lengths, state_in=state_in, grads_in=gin)
            a = fz.make_inputs(c)
            ref = _nn_lstm(c, a)
            x = flip(a["x"].double()).requires_grad_(True)
            h0, c0 = ((a[k].double() if k in state_in else torch.zeros_like(a[k].double())).requires_grad_(True) for k in ("h0", "c0"))
            out, (h_n, c_n) = bref.call_packed(ref, x, (h0, c0), lengths)
            y_last = h_n[-1]
            terms = dict(dy_all=(flip(out), "dy_all"), dy_last=(y_last, "dy_last"), dh_n=(h_n, "dh_n"), dc_n=(c_n, "dc_n"))
            loss = sum((terms[k][0] * a[terms[k][1]].double()).sum() for k in gin)
            grads = torch.autograd.grad(loss, [x, h0, c0] + list(ref.parameters()), allow_unused=True)
            grads = [torch.zeros_like(t) if g is None else g for g, t in zip(grads, [x, h0, c0] + list(ref.parameters()))]
            want = dict(y_all=flip(out.detach()), y_last=y_last.detach(), h_n=h_n.detach(), c_n=c_n.detach(), dx=flip(grads[0]),
                        dh0=grads[1], dc0=grads[2], **{k: g for (k, _), g in zip(ref.named_parameters(), grads[3:])})
            _close(fz.reference(c, a), want, f"reverse={reverse} {state_in} {gin}")


def test_adding_modes_and_padding_of_the_reference():
    c = _tiny(lengths=LENGTHS, reverse=True)
    a = fz.make_inputs(c)
    plain = fz.reference(c, a)
    added = fz.reference(dict(c, dx_add=True, accumulate=True), a)
    for b, n in enumerate(LENGTHS):
        assert not plain["y_all"][b, n:].any() and not plain["dx"][b, n:].any()
        assert np.array_equal(added["dx"][b, n:], a["prev_dx"][b, n:].double().numpy())
    assert np.array_equal(added["dx"], plain["dx"] + a["prev_dx"].double().numpy())
    for k in a["lp"]:
        assert np.array_equal(added[k], plain[k] + a["prev"][k].double().numpy())
    # the bf16-faithful emulator on the same terms: close to, and not equal to, the float64 result
    emu = fz.reference(dict(c, dtype="bf16"), a, rounding=True)
    assert set(emu) == set(plain)
    err = np.abs(emu["y_all"] - plain["y_all"]).max()
    assert 0 < err < 3e-2
