"""Randomised LSTM plan cases with every plan feature in combination, shared by tests/test_lstm_feature_fuzz_cpu.py and
tests/test_gpu_lstm_feature_fuzz.py (not a test module; nothing here touches a GPU).

cases(seed, n) draws case records: a regime -- (H, dtype, environment, state) of tests/test_gpu_lstm_state.py::CASES and
tests/test_gpu_bilstm.py::PLAN_CASES, each with and without CSN_LSTM_STATE -- a small shape around the tile, chunk and
32-step edges, and the plan features, each drawn on its own where the combination is legal: reverse, lengths, state
arguments, dropout, the three settings of csn_lstm_plan_set_io, a strided x view, accumulating gradients, the
gradient-ready callback, subsets of the outputs and of the incoming gradients.  expected_plan(case) mirrors make_layout's
choice of path and kernels (csrc/lstm.hip) so that the coverage of the committed (seed, n) is checkable without a GPU.

reference(case, inputs) is the float64 result of a case in plain terms, from parts the suite already has: the per-row
reversal R (bilstm_reference), the stack composed layer by layer and row group by row group with the mask between the
layers (dropout_reference.rows_composed_emulator without rounding = a float64 nn.LSTM chain), and the host mask
cabi.lstm_dropout_keep.  A reverse plan is the whole stack on R(x, lengths) with y_all and dx reversed back, its dropout
mask indexed by RECURRENCE STEP; an absent incoming gradient is a zero gradient; y_last is h_n of the top layer; the
padding of y_all and dx is zero, under dx_add the padding of dx is left as it was.  With lengths, y_last of an empty row is h0 of the top
layer, so that row's dy_last reaches dh0[L-1] (test_argument_subsets_are_the_loss_without_the_omitted_terms: autograd)."""
import itertools

import numpy as np
import torch

import bilstm_reference as bref
import dropout_reference as dref
import lstm_input_views as views
import test_gpu_bilstm as tb
import test_gpu_lstm_lengths as tl
import test_gpu_lstm_state as st

SEED, N = 1, 64            # the committed draw: tests/test_lstm_feature_fuzz_cpu.py states what it must cover

NAMES = bref.NAMES
FEATURES = ("reverse", "lengths", "state_args", "dropout", "y_pitch", "dy_pitch", "dx_add", "x_view", "accumulate", "callback",
            "out_subset", "grad_subset")
B_VALUES = (1, 31, 32, 33, 63, 64, 65, 129)
I_VALUES = (1, 12, 24, 32, 128, 130)
P_VALUES = (0.0, 0.1, 0.5, 1.0)
T_MAX, L_MAX = 41, 5
_WS_H = (128, 256, 384, 512, 768, 1024)       # hidden sizes of the weight-stationary kernels


def _regimes():
    """name -> (H, 'bf16' | 'f32', environment, state): the distinct (H, dtype, environment) of st.CASES, each as a state
    and as a stateless plan, and the stateless float32 path-4 plan of tb.PLAN_CASES under its own name."""
    table, seen = {}, {}
    for name, (shape, dtype, _, env) in st.CASES.items():
        key = (shape[3], dtype, tuple(sorted(env.items())))
        if key in seen:
            continue
        seen[key] = name
        for state in (True, False):
            table[name + ("" if state else "_stateless")] = (shape[3], "bf16" if dtype == st.BF16 else "f32", dict(env), state)
    shape, dtype, _, env, state = tb.PLAN_CASES["f32_path4_stateless"]
    assert dtype == st.F32 and not state
    table["f32_path4_stateless"] = (shape[3], "f32", dict(env), False)
    return table


REGIMES = _regimes()


def expected_plan(case):
    """(path, forward kernel, backward kernel) a training plan of the case takes on a whole MI355X: make_layout,
    csn_lstm_plan_path and csn_lstm_plan_kernel_name of csrc/lstm.hip with the *_supported predicates behind them."""
    H, B, T, L, env = case["H"], case["B"], case["T"], case["L"], case["env"]
    bf16 = case["dtype"] == "bf16"
    on = lambda k: env.get(k, "0") not in ("", "0")        # noqa: E731
    cell_v1 = on("CSN_CELL_V1")
    no_persist = on("CSN_NO_PERSIST") or (case["state"] and not bf16)
    chunk = max(1, int(env.get("CSN_LSTM_CHUNK", 32)))
    tiles = (B + 63) // 64
    il = bf16 and H % 128 == 0 and not cell_v1
    slabs_fit = (T + 1) * tiles * 64 * H * 8 < 1 << 32
    ns_ok = (bf16 and not no_persist and not on("CSN_FWD_KSPLIT") and H in _WS_H and (H == 1024 or on("CSN_FWD_NSPLIT"))
             and H != 768 and (H // 32) * tiles <= 128)
    fwd_ns = il and ns_ok and L <= 4
    nq, ks = (6 if H % 24 == 0 else 8), H // 128
    ks_shape = (nq == 6 and ks in (6, 3)) or (nq == 8 and ks in (4, 2, 1))
    ks_ok = bf16 and H % 128 == 0 and not no_persist and ks_shape and (H // (4 * nq)) * tiles <= 128
    persist = fwd_ns or (il and slabs_fit and ks_ok and L <= 4)
    persist_bwd = persist and slabs_fit and bf16 and not no_persist and not on("CSN_NO_PERSIST_BWD") and H in _WS_H
    f32_persist = not il and not bf16 and not no_persist and not cell_v1 and H in _WS_H
    if f32_persist:
        return (4, "lstm_fwd_f32_persist_kernel", "lstm_bwd_f32_persist_kernel")
    cell_ks = H % 256 == 0 if bf16 else H % 128 == 0
    fwd = ("lstm_fwd_ns_kernel" if fwd_ns else "lstm_fwd_persist_kernel" if persist else "lstm_cell_fwd_il_kernel" if il
           else "lstm_cell_fwd_ks_kernel" if cell_ks else "lstm_cell_fwd_kernel")
    slots = min(L, -(-T // chunk))
    grouped = persist_bwd and slots <= 4 and slots * tiles <= 8 and not on("CSN_PERSIST_STREAMS")
    bwd = ("lstm_bwd_persist_kernel" if grouped else "lstm_cell_bwd_il_kernel" if il
           else "lstm_cell_bwd_ks_kernel" if cell_ks else "lstm_cell_bwd_kernel")
    return (3 if persist_bwd else 2 if persist else 1 if il else 0, fwd, bwd)


def lengths_for(pattern, B, T, edges, rng):
    """The patterns of tests/test_gpu_lstm_lengths.py::_lengths for any B >= 1."""
    if pattern == "all_T":
        n = [T] * B
    elif pattern == "all_1":
        n = [1] * B
    elif pattern == "all_0":
        n = [0] * B
    elif pattern == "random_1_T":
        n = rng.integers(1, T + 1, B).tolist()
    elif pattern == "random_with_zeros":
        n = rng.integers(0, T + 1, B).tolist()
        n[B - 1] = n[1 % B] = 0
        n[0] = T
    elif pattern == "chunk_edges":
        vals = [e for e in edges if e <= T] + [T, T - 1]
        n = [vals[i % len(vals)] for i in rng.permutation(B)]
    elif pattern == "single_long":
        n = rng.integers(1, min(3, T) + 1, B).tolist()
        n[B // 2] = T
    else:
        raise ValueError(pattern)
    return [int(v) for v in n]


def _subset(rng, keys):
    """A non-empty random subset of `keys`, in their order."""
    while True:
        pick = tuple(k for k in keys if rng.random() < 0.6)
        if pick:
            return pick


def _draw(rng, k, regime):
    H, dtype, env, state = REGIMES[regime]
    chunk = int(env.get("CSN_LSTM_CHUNK", 32))
    big = H >= 768
    c = dict(regime=regime, H=H, dtype=dtype, env=dict(env), state=state)
    c["B"] = int(rng.choice([b for b in B_VALUES if not big or b <= 65]))
    c["I"] = int(rng.choice(I_VALUES))
    t_max, l_max = (33, 2) if big else (T_MAX, L_MAX)
    t_edges = sorted({e + d for e in (1, chunk, 2 * chunk, 32) for d in (-1, 0, 1) if 1 <= e + d <= t_max})
    c["T"] = int(rng.choice(t_edges)) if rng.random() < 0.7 else int(rng.integers(1, t_max + 1))
    c["L"] = int(rng.integers(1, l_max + 1))
    c["reverse"] = bool(rng.random() < 0.5)
    # dropout: a dropout plan with at least two layers; p = 0 on it is the plain plan's bits
    c["dropout_plan"] = bool(rng.random() < 0.55)
    c["dropout"] = None
    if c["dropout_plan"]:
        c["L"] = max(c["L"], 2)
        c["dropout"] = (float(rng.choice(P_VALUES, p=(0.1, 0.3, 0.4, 0.2))), int(rng.integers(0, 1 << 63)), int(rng.integers(0, 4)))
    # lengths (state plans only)
    c["pattern"], c["lengths"] = None, None
    c["edges"] = (3, 4, 5) if chunk == 4 else (31, 32, 33)
    if state and rng.random() < 0.7:
        c["pattern"] = str(rng.choice(tl.PATTERNS))
        c["lengths"] = lengths_for(c["pattern"], c["B"], c["T"], c["edges"], rng)
    # outputs and incoming gradients: non-empty subsets of what the plan has
    c["outputs"] = _subset(rng, st._OUT_KEYS if state else st._OUT_KEYS[:2])
    c["grads_in"] = _subset(rng, st._BWD_IN if state else st._BWD_IN[:2])
    c["state_in"] = tuple(k for k in ("h0", "c0") if state and rng.random() < 0.6)
    c["state_grads_out"] = tuple(k for k in ("dh0", "dc0") if state and rng.random() < 0.6)
    c["want_dx"] = bool(rng.random() < 0.8)
    # csn_lstm_plan_set_io: a pitch where the tensor it describes is there, the left (0) or right (1) half of [B,T,2H]
    c["y_pitch"] = bool("y_all" in c["outputs"] and rng.random() < 0.6)
    c["dy_pitch"] = bool("dy_all" in c["grads_in"] and rng.random() < 0.6)
    c["y_half"], c["dy_half"] = int(rng.integers(0, 2)), int(rng.integers(0, 2))
    c["dx_add"] = bool(c["want_dx"] and rng.random() < 0.5)
    c["x_view"] = str(rng.choice(list(views.VIEWS))) if rng.random() < 0.5 else None
    c["accumulate"] = bool(rng.random() < 0.5)
    c["callback"] = bool(rng.random() < 0.5)
    c["data_seed"] = int(rng.integers(0, 1 << 31))
    f = features(c)
    c["id"] = (f"{k:02d}-{regime}-b{c['B']}t{c['T']}i{c['I']}l{c['L']}" + "".join(
        "-" + tag for tag, on in (("rev", f["reverse"]), (f"len_{c['pattern']}", f["lengths"]), ("st", f["state_args"]),
                                  (f"p{c['dropout'][0] if c['dropout'] else 0}", c["dropout_plan"]),
                                  ("io" + "y" * f["y_pitch"] + "d" * f["dy_pitch"] + "a" * f["dx_add"], f["y_pitch"] or f["dy_pitch"] or f["dx_add"]),
                                  (f"x_{c['x_view']}", f["x_view"]), ("acc", f["accumulate"]), ("cb", f["callback"]),
                                  ("out_" + "+".join(c["outputs"]), f["out_subset"]), ("in_" + "+".join(c["grads_in"]), f["grad_subset"])) if on))
    return c


def features(c):
    """{feature: on} of a case record."""
    n_out, n_in = (4, 4) if c["state"] else (2, 2)
    return dict(reverse=c["reverse"], lengths=c["lengths"] is not None,
                state_args=bool(c["state_in"] or c["state_grads_out"] or set(c["grads_in"]) & {"dh_n", "dc_n"}),
                dropout=c["dropout"] is not None and c["dropout"][0] > 0, y_pitch=c["y_pitch"], dy_pitch=c["dy_pitch"],
                dx_add=c["dx_add"], x_view=c["x_view"] is not None, accumulate=c["accumulate"], callback=c["callback"],
                out_subset=len(c["outputs"]) < n_out, grad_subset=len(c["grads_in"]) < n_in)


def cases(seed=SEED, n=N):
    """n case records, the same for the same (seed, n).  The regimes are dealt round-robin from a shuffled deck, so every
    regime is drawn floor(n / len(REGIMES)) times at least; everything else is drawn per case."""
    rng = np.random.default_rng(seed)
    deck = [list(REGIMES)[i] for i in rng.permutation(len(REGIMES))]
    return [_draw(rng, k, deck[k % len(deck)]) for k in range(n)]


def check_legal(c):
    """Raises AssertionError unless the record is a combination the library accepts and the issue's ranges hold."""
    H, dtype, env, state = REGIMES[c["regime"]]
    assert (c["H"], c["dtype"], c["env"], c["state"]) == (H, dtype, env, state)
    big = H >= 768
    assert c["B"] in B_VALUES and c["I"] in I_VALUES and 1 <= c["T"] <= T_MAX and 1 <= c["L"] <= L_MAX
    assert not big or (c["B"] <= 65 and c["T"] <= 33 and c["L"] <= 2)
    assert c["outputs"] and c["grads_in"]
    if not state:
        assert c["lengths"] is None and not c["state_in"] and not c["state_grads_out"]
        assert set(c["outputs"]) <= {"y_last", "y_all"} and set(c["grads_in"]) <= {"dy_last", "dy_all"}
    assert set(c["outputs"]) <= set(st._OUT_KEYS) and set(c["grads_in"]) <= set(st._BWD_IN)
    if c["lengths"] is not None:
        assert c["pattern"] in tl.PATTERNS and len(c["lengths"]) == c["B"] and all(0 <= v <= c["T"] for v in c["lengths"])
    assert (c["dropout"] is not None) == c["dropout_plan"]
    if c["dropout"] is not None:
        assert c["L"] >= 2 and c["dropout"][0] in P_VALUES
    assert not c["y_pitch"] or "y_all" in c["outputs"]
    assert not c["dy_pitch"] or "dy_all" in c["grads_in"]
    assert not c["dx_add"] or c["want_dx"]
    assert c["x_view"] is None or c["x_view"] in views.VIEWS


# ---- inputs -------------------------------------------------------------------------------------------------------------
def make_inputs(c):
    """Every tensor a case can pass, as float32 CPU tensors, from the case's data seed: lp (the parameters under nn.LSTM's
    names), x (the DENSE equivalent of the case's view), the state, every incoming gradient, and the previous contents of
    dx and of the parameter gradients for the adding modes."""
    B, T, I, H, L = (c[k] for k in "BTIHL")
    torch.manual_seed(c["data_seed"])
    lp = {k: v.detach().clone() for k, v in torch.nn.LSTM(I, H, L, batch_first=True).state_dict().items()}
    g = torch.Generator().manual_seed(c["data_seed"] + 1)
    r = lambda *shape: torch.randn(*shape, generator=g)      # noqa: E731
    a = dict(lp=lp, x=r(B, T, I), h0=0.5 * r(L, B, H), c0=r(L, B, H), dy_last=r(B, H), dy_all=0.1 * r(B, T, H), dh_n=r(L, B, H),
             dc_n=r(L, B, H), prev_dx=r(B, T, I), prev={k: r(*v.shape) for k, v in lp.items()})
    if c["x_view"] == "batch_broadcast":           # a stride-0 view IS its first row, repeated
        a["x"] = a["x"][:1].expand(B, T, I).contiguous()
    return a


def host_masks(c):
    """[L-1, B, T, H] bool from the library's host mask, or None without dropout: element (l, t, b, u) of the PLAN's
    T, B, H has index ((l T + t) B + b) H + u, where t counts the plan's recurrence steps."""
    if c["dropout"] is None or c["dropout"][0] == 0:
        return None
    from cerebralsignalnetworks_amd import cabi
    B, T, H, L = c["B"], c["T"], c["H"], c["L"]
    p, seed, sub = c["dropout"]
    keep = cabi.lstm_dropout_keep(seed, sub, p, 0, (L - 1) * T * B * H).astype(bool).reshape(L - 1, T, B, H)
    return np.ascontiguousarray(keep.transpose(0, 2, 1, 3))


def reference(c, a, rounding=False, masks="host"):
    """The case in plain terms (module docstring).  a = make_inputs(c).  -> float64 numpy under the keys y_last, y_all,
    h_n, c_n, dx, dh0, dc0 and the parameter names: EVERY output, whatever the case asks for; dx and the parameter
    gradients include the previous contents where the case adds (dx_add, accumulate).  rounding=True: the bf16-faithful
    emulator on the same terms (for the bf16 cases)."""
    B, T, H, L = c["B"], c["T"], c["H"], c["L"]
    n64 = lambda t: t.detach().double().numpy()        # noqa: E731
    lengths = c["lengths"] if c["lengths"] is not None else [T] * B
    flip = (lambda t: bref.R(t, lengths)) if c["reverse"] else (lambda t: t)
    gin = set(c["grads_in"])
    zeros = torch.zeros(L, B, H)
    h0 = a["h0"] if "h0" in c["state_in"] else zeros
    c0 = a["c0"] if "c0" in c["state_in"] else zeros
    dh = (a["dh_n"] if "dh_n" in gin else zeros).clone()
    dc = a["dc_n"] if "dc_n" in gin else zeros
    dy = flip(a["dy_all"] if "dy_all" in gin else torch.zeros(B, T, H)).clone()
    if "dy_last" in gin:                           # y_last is h_n of the top layer: its gradient enters where dh_n[L-1] does
        for b, n in enumerate(lengths):
            if n > 0:
                dy[b, n - 1] += a["dy_last"][b]    # (float32, as the library adds them)
            else:
                dh[L - 1, b] += a["dy_last"][b]
    if isinstance(masks, str):
        masks = host_masks(c)
    s = dref.scale(c["dropout"][0]) if masks is not None else None
    lp = {k: n64(v) for k, v in a["lp"].items()}
    res = dref.rows_composed_emulator(lp, L, n64(flip(a["x"])), lengths, n64(h0), n64(c0), n64(dy), n64(dh), n64(dc), masks, s,
                                      rounding=rounding)
    back = lambda v: n64(flip(torch.from_numpy(np.ascontiguousarray(v))))        # noqa: E731
    out = dict(y_last=res["h_n"][L - 1], y_all=back(res["out"]), h_n=res["h_n"], c_n=res["c_n"], dx=back(res["dx"]),
               dh0=res["dh0"], dc0=res["dc0"], **{k: np.asarray(res[k], np.float64) for k in lp})
    return add_previous(c, a, out)


def add_previous(c, a, out):
    """A copy of reference()'s dict with the previous contents joined where the case adds: dx (dx_add; the padding of dx is
    then what it was) and the parameter gradients (accumulate)."""
    out = dict(out)
    if c["dx_add"]:
        out["dx"] = out["dx"] + a["prev_dx"].double().numpy()
    if c["accumulate"]:
        for k in a["lp"]:
            out[k] = out[k] + a["prev"][k].double().numpy()
    return out


def pair_counts(cs):
    """{(feature, feature): cases with both on} over every pair of FEATURES."""
    fs = [features(c) for c in cs]
    return {(p, q): sum(f[p] and f[q] for f in fs) for p, q in itertools.combinations(FEATURES, 2)}
