"""GPU: randomised LSTM plans with every plan feature in combination (tests/lstm_feature_fuzz.py), one test per case.

Each case builds the FEATURED plan and a BASELINE plan with the same CSN_LSTM_STATE and CSN_LSTM_DROPOUT bits but no
reverse, default io, dense x, overwriting gradients, every output requested, on data reversed beforehand with R; lengths,
state, dropout setting, incoming gradients (absent ones absent) and weights are the same.  Bit for bit: the featured
results are the baseline's after undoing the layout (R back on y_all and dx; the pitched half is the dense tensor and the
other half is still NaN; dx and the parameter gradients are prev + the baseline's in the adding modes, the padding of dx
untouched under dx_add and zero otherwise; an output left out changes no other; the callback fires once per layer, top
layer first), and NaN / Inf in the padding of x and dy_all changes nothing.  The plans take the path and kernels of a plan
without the dropout and reverse bits, a reverse plan has the workspace size of the plan without the bit, no status word is
raised.  Both results are then held against the float64 reference of the case within st._bounds, and the bf16 ones
against the bf16-faithful emulator within oracle.compare.BF16_EMU_BOUNDS.

Worst measured errors over the 64 committed cases (MI355X, baseline and featured), all under the bounds named above:
bf16 against float64: outputs and states 7.1e-3 (bound 3e-2), gradients 1.25e-2 relative norm (4e-2); bf16 against the
emulator, relative norm: y 1.1e-3, c_n 1.5e-4, dx 2.7e-3, dh0 1.2e-3, dc0 7.1e-4, parameter gradients 2.8e-3; float32:
outputs 1.8e-7 (2e-5), gradients 6.7e-7 (1e-5).  The whole file takes 18 s."""
import numpy as np
import pytest
import torch

import bilstm_reference as bref
import lstm_feature_fuzz as fz
import lstm_input_views as views
import test_gpu_bilstm as tb
import test_gpu_lstm_state as st
from cerebralsignalnetworks_amd import cabi
from oracle import compare

pytestmark = pytest.mark.gpu

DEV, BF16, F32 = st.DEV, st.BF16, st.F32
NAN = float("nan")
CASES = fz.cases(fz.SEED, fz.N)
_OUT_SHAPES = dict(y_last="BH", y_all="BTH", h_n="LBH", c_n="LBH")


def _setenv(c, monkeypatch):
    for k, v in c["env"].items():
        monkeypatch.setenv(k, v)


def _plan(c, **bits):
    kw = dict(state=c["state"], dropout=c["dropout_plan"], reverse=c["reverse"])
    kw.update(bits)
    return cabi.LstmPlan(c["B"], c["T"], c["I"], c["H"], c["L"], BF16 if c["dtype"] == "bf16" else F32, DEV, training=True, **kw)


def _triple(plan):
    return (plan.path(),) + plan.kernel_names()


def _weights(a, L):
    return [[a["lp"][f"{n}_l{k}"].to(DEV) for k in range(L)] for n in fz.NAMES]


def _settings(plan, c):
    if plan.state:
        plan.set_lengths(c["lengths"])
    if plan.dropout:
        plan.set_dropout(*c["dropout"])


def _half(buf, half, H):
    return buf[:, :, half * H:(half + 1) * H]


def _poison(t, lengths, flip):
    """NaN / Inf over the padding t[b, lengths[b]:] of a clone."""
    t = t.clone()
    for b, n in enumerate(lengths):
        t[b, n:] = float("nan") if (b % 2) ^ flip else float("inf")
    return t


def _featured(plan, c, w, a, poison=False):
    """One forward + backward of the featured plan with exactly the arguments the case names.  -> the results by name
    (parameter gradients under their names), with dx / gradients started from the previous contents in the adding modes and
    from NaN otherwise, and 'fired', the layers the callback reported."""
    B, T, I, H, L = (c[k] for k in "BTIHL")
    d = {k: (v.to(DEV) if torch.is_tensor(v) else v) for k, v in a.items()}
    x, dy_all = d["x"], d["dy_all"]
    if poison:
        # (a stride-0 view has one row: every row reads it up to its own length, so only what no row reads is poisoned)
        lens = [max(c["lengths"])] * B if c["x_view"] == "batch_broadcast" else c["lengths"]
        x, dy_all = _poison(x, lens, 0), _poison(dy_all, c["lengths"], 1)
    if c["x_view"] is not None:
        x, dense = views.VIEWS[c["x_view"]](x)
        assert torch.equal(torch.nan_to_num(x), torch.nan_to_num(dense)) and x.stride(2) == 1      # (NaN where poisoned)
    _settings(plan, c)
    plan.set_io(2 * H if c["y_pitch"] else 0, 2 * H if c["dy_pitch"] else 0, c["dx_add"])
    plan.set_grad_mode(c["accumulate"])
    fired = []
    plan.set_grad_callback(fired.append if c["callback"] else None)
    dims = dict(B=B, T=T, H=H, L=L)
    out = {k: torch.full([dims[ch] for ch in _OUT_SHAPES[k]], NAN, device=DEV) for k in c["outputs"]}
    res = dict(out)
    if c["y_pitch"]:
        res["ybuf"] = torch.full((B, T, 2 * H), NAN, device=DEV)
        out["y_all"] = _half(res["ybuf"], c["y_half"], H)
        res["y_all"] = out["y_all"]
    lib = cabi.load()
    cabi._check(lib.csn_lstm_forward(plan._plan, cabi._ptr(x), x.stride(0), x.stride(1), *[cabi._ptr_array(g) for g in w],
                                     cabi._ptr(d["h0"] if "h0" in c["state_in"] else None),
                                     cabi._ptr(d["c0"] if "c0" in c["state_in"] else None), plan._ws_ptr,
                                     *[cabi._ptr(out.get(k)) for k in st._OUT_KEYS], cabi._stream()))
    gin = {k: d[k] if k in c["grads_in"] else None for k in st._BWD_IN}
    if c["dy_pitch"]:
        dybuf = torch.full((B, T, 2 * H), NAN, device=DEV)
        _half(dybuf, c["dy_half"], H).copy_(dy_all)
        gin["dy_all"] = _half(dybuf, c["dy_half"], H)
        res["dybuf"] = dybuf
    elif gin["dy_all"] is not None:
        gin["dy_all"] = dy_all
    grads = [[(d["prev"][f"{n}_l{k}"].to(DEV).clone() if c["accumulate"] else torch.full_like(w[g][k], NAN)) for k in range(L)]
             for g, n in enumerate(fz.NAMES)]
    if c["want_dx"]:
        res["dx"] = d["prev_dx"].clone() if c["dx_add"] else torch.full((B, T, I), NAN, device=DEV)
    for k in c["state_grads_out"]:
        res[k] = torch.full((L, B, H), NAN, device=DEV)
    plan.backward(gin["dy_last"], gin["dy_all"], grads, dx=res.get("dx"), dh_n=gin["dh_n"], dc_n=gin["dc_n"], dh0=res.get("dh0"),
                  dc0=res.get("dc0"))
    for n, group in zip(fz.NAMES, grads):
        res.update({f"{n}_l{k}": t for k, t in enumerate(group)})
    res["fired"] = fired
    return res


def _baseline(plan, c, w, a):
    """The same call on the plan without reverse: default io, dense x, overwrite, every output; x and dy_all reversed."""
    B, T, I, H, L = (c[k] for k in "BTIHL")
    d = {k: (v.to(DEV) if torch.is_tensor(v) else v) for k, v in a.items()}
    flip = (lambda t: bref.R(t, c["lengths"])) if c["reverse"] else (lambda t: t)
    _settings(plan, c)
    s = plan.state
    outs = plan.forward(flip(d["x"]).contiguous(), *w, want_all=True, h0=d["h0"] if "h0" in c["state_in"] else None,
                        c0=d["c0"] if "c0" in c["state_in"] else None, want_state=s)
    res = dict(zip(st._OUT_KEYS, outs))
    gin = {k: d[k] if k in c["grads_in"] else None for k in st._BWD_IN}
    if gin["dy_all"] is not None:
        gin["dy_all"] = flip(gin["dy_all"]).contiguous()
    res["dx"] = torch.full((B, T, I), NAN, device=DEV)
    if s:
        res["dh0"], res["dc0"] = torch.full((L, B, H), NAN, device=DEV), torch.full((L, B, H), NAN, device=DEV)
    grads = [[torch.full_like(p, NAN) for p in group] for group in w]
    plan.backward(gin["dy_last"], gin["dy_all"], grads, dx=res["dx"], dh_n=gin["dh_n"], dc_n=gin["dc_n"], dh0=res.get("dh0"),
                  dc0=res.get("dc0"))
    for n, group in zip(fz.NAMES, grads):
        res.update({f"{n}_l{k}": t for k, t in enumerate(group)})
    # undo the layout: the baseline's y_all and dx in the caller's time
    res["y_all"], res["dx"] = flip(res["y_all"]), flip(res["dx"])
    return res


def _bit_identities(c, a, got, base, what):
    B, T, H, L = c["B"], c["T"], c["H"], c["L"]
    lengths = c["lengths"] if c["lengths"] is not None else [T] * B
    valid = (torch.arange(T)[None, :] < torch.tensor(lengths)[:, None]).to(DEV)              # [B, T]
    for k in c["outputs"] + c["state_grads_out"]:
        assert torch.equal(got[k], base[k]), (what, k, float((got[k] - base[k]).abs().max()))
    if "y_all" in c["outputs"]:
        assert not got["y_all"][~valid].any(), (what, "y_all padding")
    if c["y_pitch"]:
        assert torch.isnan(_half(got["ybuf"], 1 - c["y_half"], H)).all(), (what, "the other half of the y_all buffer")
    if c["dy_pitch"]:
        assert torch.isnan(_half(got["dybuf"], 1 - c["dy_half"], H)).all(), (what, "the other half of the dy_all buffer")
    assert not base["dx"][~valid].any(), (what, "baseline dx padding")
    if c["want_dx"]:
        prev = a["prev_dx"].to(DEV)
        if c["dx_add"]:
            assert torch.equal(got["dx"][valid], (prev + base["dx"])[valid]), (what, "dx += over the valid steps")
            assert torch.equal(got["dx"][~valid], prev[~valid]), (what, "dx padding under dx_add")
        else:
            assert torch.equal(got["dx"], base["dx"]), (what, "dx", float((got["dx"] - base["dx"]).abs().max()))
            assert not got["dx"][~valid].any(), (what, "dx padding")
    for k in a["lp"]:
        want = a["prev"][k].to(DEV) + base[k] if c["accumulate"] else base[k]
        assert torch.equal(got[k], want), (what, k, float((got[k] - want).abs().max()))
    assert got["fired"] == (list(range(L - 1, -1, -1)) if c["callback"] else []), (what, got["fired"])


def _same_bits(got, again, what):
    for k, v in got.items():
        if torch.is_tensor(v) and k not in ("ybuf", "dybuf"):          # (the buffers hold NaN halves; y_all is the view)
            assert torch.equal(v, again[k]), (what, k)
    assert got["fired"] == again["fired"]


def _against_reference(c, res, keys, want, emu, what):
    """`res`[k] for k in keys within st._bounds of the float64 reference (outputs and states: max |difference|; gradients:
    relative norm; a reference that is exactly zero must be met exactly) and, bf16, within the emulator bounds.
    -> (the printed line, the failures)."""
    elem, rel = st._bounds(BF16 if c["dtype"] == "bf16" else F32)
    line, bad = [], []
    for k in keys:
        g, w = st._np(res[k]), want[k]
        if not np.isfinite(g).all():
            bad.append((what, k, "non-finite"))
            continue
        if k in st._OUT_KEYS:
            err, bound = float(np.abs(g - w).max()), elem
        elif not w.any():
            err, bound = float(np.abs(g).max()), 0.0
        else:
            err, bound = float(np.linalg.norm(g - w) / np.linalg.norm(w)), rel
        line.append(f"{k} {err:.2e}")
        if not (err < bound or err == bound == 0.0):
            bad.append((what, k, err, bound))
        if emu is not None:
            r, e = compare.errors(g, emu[k])
            line[-1] += f" (emu {r:.1e}/{e:.1e})"
            try:
                compare.check(f"{what}: {k}", g, emu[k], *compare.bf16_emu_bound(k), layout=compare.layout_of(k))
            except AssertionError as exc:
                bad.append(str(exc))
    return f"measured {what} vs float64 reference" + (" (bf16 emulator rel/elem)" if emu is not None else "") + ": " + " ".join(line), bad


@pytest.mark.parametrize("c", CASES, ids=[c["id"] for c in CASES])
def test_featured_plan_is_the_baseline_and_the_reference(c, monkeypatch):
    _setenv(c, monkeypatch)
    a = fz.make_inputs(c)
    L = c["L"]
    w = _weights(a, L)
    featured, baseline, plain = _plan(c), _plan(c, reverse=False), _plan(c, dropout=False, reverse=False)
    # plan identity: the path and kernels of a plan with none of the feature bits, which are those the mirror expects
    assert _triple(featured) == _triple(baseline) == _triple(plain) == fz.expected_plan(c), (c["id"], _triple(featured))
    if c["state"] and c["dtype"] == "bf16":          # a bf16 state plan takes the stateless plan's path
        assert _triple(featured) == _triple(_plan(c, state=False, dropout=False, reverse=False))
    lib = cabi.load()
    assert lib.csn_lstm_plan_workspace_bytes(featured._plan) == lib.csn_lstm_plan_workspace_bytes(baseline._plan)
    assert featured.reverse == c["reverse"] and not baseline.reverse

    got = _featured(featured, c, w, a)
    base = _baseline(baseline, c, w, a)
    _bit_identities(c, a, got, base, c["id"])
    if c["lengths"] is not None:
        _same_bits(got, _featured(featured, c, w, a, poison=True), c["id"] + " NaN / Inf padding")
    torch.cuda.synchronize()
    assert featured.status() == 0 and baseline.status() == 0

    # both against the float64 reference (and the bf16 emulator) of the case: computed once in plain terms, the featured
    # results against it with the previous contents of the adding modes joined
    plain_terms = dict(c, dx_add=False, accumulate=False)
    want = fz.reference(plain_terms, a)
    emu = fz.reference(plain_terms, a, rounding=True) if c["dtype"] == "bf16" else None
    base_keys = [k for k in base if c["state"] or k not in ("h_n", "c_n")]
    line_b, bad_b = _against_reference(c, base, base_keys, want, emu, c["id"] + " baseline")
    want, emu = fz.add_previous(c, a, want), (fz.add_previous(c, a, emu) if emu is not None else None)
    line_f, bad_f = _against_reference(c, got, [k for k in got if k in want], want, emu, c["id"] + " featured")
    print(line_b)
    print(line_f)
    assert not bad_b + bad_f, (bad_b + bad_f)[:4]


def test_every_expected_path_and_kernel_triple_is_taken_by_two_cases(monkeypatch):
    """Every case's plan, created and not run: each (path, forward kernel, backward kernel) that test_gpu_lstm_state.CASES
    and the stateless float32 path-4 case of test_gpu_bilstm expect is what at least two cases run on."""
    taken = []
    for c in CASES:
        with monkeypatch.context() as m:
            _setenv(c, m)
            plan = _plan(c)
            taken.append(_triple(plan))
            assert taken[-1] == fz.expected_plan(c), (c["id"], taken[-1])
            del plan
    want = {e for _, _, e, _ in st.CASES.values() if e is not st.PLAIN} | {tb.PLAN_CASES["f32_path4_stateless"][2]}
    assert len(want) == 7
    counts = {e: taken.count(e) for e in want}
    assert min(counts.values()) >= 2, counts
