"""Every LSTM kernel instantiation with state, lengths and plan features: the case records of
tests/test_gpu_lstm_width_matrix.py and the mirror of the template dispatch behind them, shared with
tests/test_lstm_width_matrix_cpu.py (not a test module; nothing here touches a GPU).

The recurrence kernels are compiled once per hidden size, so a defect can live in one instantiation only (DESIGN.md 3.5,
3.8).  REGIMES names one hand-written shape per (kernel, hidden size) that the state / lengths / feature tests did not
reach; records() crosses each with its feature sets, in the record form of tests/lstm_feature_fuzz.py so that the fuzz
runner (make_inputs, reference, expected_plan, _featured, _baseline, _bit_identities, _against_reference) takes them as
they are.

launches(record) mirrors which template instantiation every recurrence launch of a record takes, read off
launch_persist_t / launch_fwd_persist (lstm_fwd_persist.hip), launch_ns_t / launch_fwd_ns (lstm_fwd_ns.hip),
launch_bwd_persist_t (lstm_bwd_persist.hip), launch_*_f32_persist (lstm_f32_persist.hip), launch_cell_fwd_il /
launch_cell_bwd_il (lstm_cell_blk.hip) and the launch schedules of forward_persist / backward_persist / forward_f32p
(lstm.hip):

    ("fwd_persist", NQ, KS, DPOLL, RG, PARK)    ("fwd_ns", KB, FUSE)    ("bwd_persist", KS, DPOLL, MASK, RG)
    ("f32_fwd", KS)    ("f32_bwd", KS)    ("il_fwd", NQ)    ("il_bwd", NUG, NK, MASK)

The per-step cells of path 0 are not templates over the hidden size and have no tuple.  SELECTABLE is every tuple a plan
can select; ledger_records() are the records of this file and of the tables that already ran with state."""
import numpy as np

import lstm_feature_fuzz as fz
import lstm_input_views as views
import test_gpu_bilstm as tb
import test_gpu_half_tiles as ht
import test_gpu_lstm_state as st

CHUNK = "4"          # T = 9: chunks of 4, 4 and 1, both boundaries inside the sequence
P3_IL = (3, st._PF, st._ILB)      # path 3 whose grouped backward does not apply: the per-diagonal backward cells
P4 = (4, "lstm_fwd_f32_persist_kernel", "lstm_bwd_f32_persist_kernel")
STATE_SETS = ("none", "state", "lengths", "state_lengths", "all")
STATELESS_SETS = ("none", "all_stateless")
STRIDED_VIEW = "time_major"


def _regime(shape, dtype, plan, env=None, fuse=None, sets=STATE_SETS):
    """fuse: what the regime's name says about layer 0's projection (True: inside the recurrence, False: a GEMM), or None
    where the name says nothing."""
    return dict(shape=shape, dtype=dtype, plan=plan, env={"CSN_LSTM_CHUNK": CHUNK, **(env or {})}, fuse=fuse, sets=sets)


_FLAGS = {"CSN_FWD_FLAGS": "1", "CSN_BWD_FLAGS": "1"}
_NS = {"CSN_FWD_NSPLIT": "1"}
# name: (B, T, I, H, L).  B = 65: two row tiles, the second holding one row.
REGIMES = {
    # bf16, path 3, K-split forward
    "ks384_fused": _regime((65, 9, 128, 384, 2), "bf16", st.P3, fuse=True),
    "ks384_gemm": _regime((65, 9, 24, 384, 2), "bf16", st.P3, fuse=False),
    "ks512": _regime((65, 9, 32, 512, 2), "bf16", st.P3, fuse=False),              # H 512 never fuses (views.fuse_x)
    "ks384_flags": _regime((65, 9, 32, 384, 2), "bf16", st.P3, _FLAGS),
    "ks512_flags": _regime((65, 9, 32, 512, 2), "bf16", st.P3, _FLAGS),
    "ks384_l4": _regime((65, 17, 32, 384, 4), "bf16", st.P3),                      # launches of 1 .. 4 layers: 32- and 64-row groups
    "ks512_b129": _regime((129, 9, 32, 512, 2), "bf16", st.P3),                    # three tiles, grouped
    "ks512_b129_l3": _regime((129, 9, 32, 512, 3), "bf16", P3_IL),                 # 3 slots x 3 tiles = 9 groups: ungrouped on purpose
    # bf16, path 3, N-split forward
    "ns256_fused": _regime((65, 9, 128, 256, 2), "bf16", st.P3_NS, _NS, fuse=True),
    "ns256_gemm": _regime((65, 9, 24, 256, 2), "bf16", st.P3_NS, _NS, fuse=False),
    "ns384_fused": _regime((65, 9, 128, 384, 2), "bf16", st.P3_NS, _NS, fuse=True),
    "ns384_gemm": _regime((65, 9, 24, 384, 2), "bf16", st.P3_NS, _NS, fuse=False),
    "ns512_fused": _regime((65, 9, 128, 512, 2), "bf16", st.P3_NS, _NS, fuse=True),
    "ns512_gemm": _regime((65, 9, 24, 512, 2), "bf16", st.P3_NS, _NS, fuse=False),
    # bf16, path 2
    "p2_384": _regime((65, 9, 32, 384, 2), "bf16", st.P2, {"CSN_NO_PERSIST_BWD": "1"}),
    "p2_512": _regime((65, 9, 32, 512, 2), "bf16", st.P2, {"CSN_NO_PERSIST_BWD": "1"}),
    # bf16, path 1; 640 and 896 are no weight-stationary widths and need no switch
    "p1_384": _regime((65, 9, 32, 384, 2), "bf16", st.IL, {"CSN_NO_PERSIST": "1"}),
    "p1_512": _regime((65, 9, 32, 512, 2), "bf16", st.IL, {"CSN_NO_PERSIST": "1"}),
    "p1_640": _regime((33, 9, 32, 640, 2), "bf16", st.IL),
    "p1_896": _regime((33, 9, 32, 896, 2), "bf16", st.IL),
    # float32, path 4 (stateless plans only: a float32 state plan takes path 0)
    "f32p_256": _regime((65, 9, 24, 256, 2), "f32", P4, sets=STATELESS_SETS),
    "f32p_384": _regime((65, 9, 24, 384, 2), "f32", P4, sets=STATELESS_SETS),
    "f32p_512": _regime((65, 9, 24, 512, 2), "f32", P4, sets=STATELESS_SETS),
    "f32p_768": _regime((65, 9, 24, 768, 2), "f32", P4, sets=STATELESS_SETS),
    # five row tiles where f32_persist_tiles_per_launch(1024) is four: two launches per layer
    "f32p_1024_b260": _regime((260, 3, 24, 1024, 2), "f32", P4, sets=STATELESS_SETS),
    # float32 state plans: path 0, K-split cells
    "f32_state_384": _regime((33, 9, 24, 384, 2), "f32", st.V1_KS),
    "f32_state_512": _regime((33, 9, 24, 512, 2), "f32", st.V1_KS),
    # the launch forms of the weight-stationary kernels that the regimes above and the older tables leave out, or reach only
    # without state arguments (the ledger of tests/test_lstm_width_matrix_cpu.py): the flag hand-off at H 128 / 256 / 1024
    # with its masked backward, and 64-row groups -- B 129 is three tiles, so a launch of two layers has 6 groups of 64 rows
    # (2 x 2 x 3 > 8) and a launch of one layer 6 groups of 32 -- with flags at every width, with data polls at H 256 / 1024
    "ks128_flags": _regime((65, 9, 32, 128, 2), "bf16", st.P3, _FLAGS, sets=("state", "all")),
    "ks256_flags": _regime((65, 9, 32, 256, 2), "bf16", st.P3, _FLAGS, sets=("state", "all")),
    "ns1024_flags": _regime((65, 9, 128, 1024, 2), "bf16", st.P3_NS, _FLAGS, fuse=True, sets=("state", "all")),
    "ks128_flags_b129": _regime((129, 9, 32, 128, 2), "bf16", st.P3, _FLAGS, sets=("state",)),
    "ks256_flags_b129": _regime((129, 9, 32, 256, 2), "bf16", st.P3, _FLAGS, sets=("state",)),
    "ks384_flags_b129": _regime((129, 9, 32, 384, 2), "bf16", st.P3, _FLAGS, sets=("state",)),
    "ks512_flags_b129": _regime((129, 9, 32, 512, 2), "bf16", st.P3, _FLAGS, sets=("state",)),
    "ns1024_flags_b129": _regime((129, 9, 24, 1024, 2), "bf16", st.P3_NS, _FLAGS, fuse=False, sets=("state",)),
    "ks256_b129": _regime((129, 9, 32, 256, 2), "bf16", st.P3, sets=("state",)),
    "ns1024_b129": _regime((129, 9, 24, 1024, 2), "bf16", st.P3_NS, fuse=False, sets=("state",)),
    "ns128_fused": _regime((65, 9, 128, 128, 2), "bf16", st.P3_NS, _NS, fuse=True, sets=("state", "lengths")),
}

# the three bf16 weight-stationary widths of the two cross-form tests (32- against 64-row groups, weight-stationary against
# per-diagonal): name -> (B, T, I, H, L)
WS_WIDTHS = {"ks384_fused": REGIMES["ks384_fused"]["shape"], "ks512": REGIMES["ks512"]["shape"], "ks128": (65, 9, 32, 128, 2)}
EXACT = {"CSN_NO_ROTATE": "1", "CSN_NO_FUSE_X": "1", "CSN_FWD_KSPLIT": "1"}      # every workgroup walks K in one order


def hand_lengths(B, T):
    """0 and T among them, the rest spread over 1 .. T-1 (tests/test_gpu_lstm_resident.py::_lengths)."""
    n = [(3 * b + 1) % T for b in range(B)]
    n[0], n[1 % B], n[B - 1] = T, 0, max(1, T // 2)
    return n


def copy_rows(B):
    """The rows that are made copies of row 0: row 64 (alone in the second 64-row tile at B = 65) and the last row where it
    is another one (B = 33: row 32, alone in the second 32-row tile of the per-step cells; B = 260: row 259, the second
    launch of a path-4 layer)."""
    return sorted({r for r in (64, B - 1) if 0 < r < B})


def record(B, T, I, H, L, dtype, env, state=True, seed=7, **over):
    """A case record as tests/lstm_feature_fuzz.py draws them (the keys of tests/test_gpu_lstm_resident.py::_record)."""
    c = dict(B=B, T=T, I=I, H=H, L=L, dtype=dtype, env=dict(env), state=state, reverse=False, dropout_plan=False, dropout=None,
             pattern=None, lengths=None, outputs=st._OUT_KEYS if state else st._OUT_KEYS[:2],
             grads_in=st._BWD_IN[:2], state_in=(), state_grads_out=(), want_dx=True, y_pitch=False, dy_pitch=False, y_half=1,
             dy_half=0, dx_add=False, x_view=None, accumulate=False, callback=False, data_seed=seed)
    c.update(over)
    return c


def feature_record(regime, feature):
    """The record of REGIMES[regime] with one feature set (tests/test_gpu_lstm_resident.py::_feature_record):
    none / state / lengths / state_lengths / all on a state plan, none / all_stateless on a stateless one.  `lengths` alone
    passes no dh_n / dc_n, and a row's gradient at its first dead step is then zero whichever side of the `t < length`
    comparison it falls on; state_lengths is what sees that comparison without dropout in the way of the row copies."""
    r = REGIMES[regime]
    B, T, I, H, L = r["shape"]
    stateless = r["sets"] == STATELESS_SETS
    assert feature in r["sets"], (regime, feature)
    over = {}
    if feature in ("state", "state_lengths", "all"):
        over.update(state_in=("h0", "c0"), grads_in=st._BWD_IN, state_grads_out=("dh0", "dc0"))
    if feature in ("lengths", "state_lengths", "all"):
        n = hand_lengths(B, T)
        for row in copy_rows(B):
            n[row] = n[0]
        over.update(lengths=n, pattern="hand")
    if feature in ("all", "all_stateless"):
        over.update(reverse=True, dropout_plan=True, dropout=(0.5, 1234, 1), y_pitch=True, dy_pitch=True, dx_add=True,
                    accumulate=True, callback=True)
    if feature == "all_stateless":
        over.update(x_view=STRIDED_VIEW)
    c = record(B, T, I, H, L, r["dtype"], r["env"], state=not stateless, **over)
    c["regime"], c["feature"], c["id"] = regime, feature, f"{regime}-{feature}"
    return c


def records():
    return [feature_record(name, f) for name, r in REGIMES.items() for f in r["sets"]]


def ws_width_record(name, feature, env):
    """A WS_WIDTHS shape with the `state` or `lengths` feature set under `env` (plus the chunk)."""
    B, T, I, H, L = WS_WIDTHS[name]
    over = dict(lengths=hand_lengths(B, T), pattern="hand") if feature == "lengths" else {}
    c = record(B, T, I, H, L, "bf16", {"CSN_LSTM_CHUNK": CHUNK, **env}, state_in=("h0", "c0"), grads_in=st._BWD_IN,
               state_grads_out=("dh0", "dc0"), **over)
    c["id"] = f"{name}-{feature}-" + ("+".join(k[4:].lower() for k in env) or "default")
    return c


def half_tile_records():
    """32- against 64-row groups: (default, CSN_NO_HALF_TILES=1) per width, on the `state` feature set."""
    return [(ws_width_record(n, "state", {}), ws_width_record(n, "state", {"CSN_NO_HALF_TILES": "1"})) for n in WS_WIDTHS]


def diagonal_records():
    """Weight-stationary against per-diagonal: (path 3, path 1, path 2) under EXACT per width and feature set."""
    return [tuple(ws_width_record(n, f, {**EXACT, **extra}) for extra in ({}, {"CSN_NO_PERSIST": "1"}, {"CSN_NO_PERSIST_BWD": "1"}))
            for n in WS_WIDTHS for f in ("state", "lengths")]


def make_inputs(c):
    """fz.make_inputs with every row of copy_rows a copy of row 0 in every per-row input (the lengths: feature_record)."""
    a = fz.make_inputs(c)
    for row in copy_rows(c["B"]):
        for k in ("x", "dy_last", "dy_all", "prev_dx"):
            a[k][row] = a[k][0]
        for k in ("h0", "c0", "dh_n", "dc_n"):
            a[k][:, row] = a[k][:, 0]
    return a


# ---- the mirror of the template dispatch ----------------------------------------------------------------------------------
def _on(env, k):
    return env.get(k, "0") not in ("", "0")


def launches(c):
    """(forward launches, backward launches) of one forward + backward of the record: the tuple of the module docstring
    per recurrence launch, in launch order ([] where the path's kernels are no templates over H)."""
    B, T, I, H, L, env = c["B"], c["T"], c["I"], c["H"], c["L"], c["env"]
    _, fwd, bwd = fz.expected_plan(c)
    lengths = c["lengths"]
    steps = T if lengths is None else max(lengths)       # a batch with lengths runs steps 0 .. max(lengths) - 1
    if steps == 0:
        return [], []
    chunk = max(1, int(env.get("CSN_LSTM_CHUNK", 32)))
    MT, nch = (B + 63) // 64, -(-steps // chunk)
    slots = min(L, nch)
    half_ok = not _on(env, "CSN_NO_HALF_TILES")

    def diagonals(lag):
        """The layers in range per chunk diagonal: layer l at chunk dg - lag * l (forward; the backward counts from the top)."""
        out = []
        for dg in range(nch + lag * (L - 1)):
            out.append([l for l in range(L) if 0 <= dg - lag * l < nch])
        return out

    f, b = [], []
    if fwd == "lstm_fwd_persist_kernel":
        nq, ks = (6 if H % 24 == 0 else 8), H // 128
        dpoll = not _on(env, "CSN_FWD_FLAGS")
        park = (nq, ks) == (6, 6) and dpoll and not _on(env, "CSN_NO_FWD_PARK")
        grouped = slots <= 4 and slots * MT <= 8 and H // (4 * nq) <= 32 and not _on(env, "CSN_PERSIST_STREAMS")
        if grouped:
            f = [("fwd_persist", nq, ks, dpoll, 2 if half_ok and 2 * len(ls) * MT <= 8 else 4, park) for ls in diagonals(1)]
        else:
            f = [("fwd_persist", nq, ks, dpoll, 4, park)] * (nch * L)
    elif fwd == "lstm_fwd_ns_kernel":
        fuse = views.fuse_x(True, I, H) and not _on(env, "CSN_NO_FUSE_X")
        grouped = slots <= 4 and slots * MT <= 8 and H // 32 <= 32 and not _on(env, "CSN_PERSIST_STREAMS")
        if grouped:
            f = [("fwd_ns", H // 32, fuse and 0 in ls) for ls in diagonals(1)]          # FUSE: a slot of the launch multiplies x_t
        else:
            f = [("fwd_ns", H // 32, fuse and l == 0) for _ in range(nch) for l in range(L)]
    elif fwd == "lstm_cell_fwd_il_kernel":
        f = [("il_fwd", 6 if H % 24 == 0 else 8)]
    elif fwd == "lstm_fwd_f32_persist_kernel":
        per = 256 // (H // 16)                                                          # f32_persist_tiles_per_launch
        f = [("f32_fwd", H // 64)] * (L * -(-MT // per))
    if bwd == "lstm_bwd_persist_kernel":
        beside = 1 < L <= 4 and H // 32 <= 28 and not _on(env, "CSN_NO_BESIDE")
        dpoll, mask = not _on(env, "CSN_BWD_FLAGS"), lengths is not None
        b = [("bwd_persist", H // 32, dpoll, mask, 2 if half_ok and not mask and 2 * len(ls) * MT <= 8 else 4)
             for ls in diagonals(2 if beside else 1) if ls]
    elif bwd == "lstm_cell_bwd_il_kernel":
        b = [("il_bwd", 3 if H % 48 == 0 else 4, 4, lengths is not None)]               # (one entry: every launch is the same)
    elif bwd == "lstm_bwd_f32_persist_kernel":
        b = [("f32_bwd", H // 64)] * (L * -(-MT // (256 // (H // 16))))
    return f, b


def instantiations(c):
    f, b = launches(c)
    return set(f) | set(b)


def half_tile_launches(c):
    """(forward, backward) recurrence launches on 32-row groups: csn_lstm_plan_half_tile_launches(0 / 1)."""
    f, b = launches(c)
    return (sum(t[0] == "fwd_persist" and t[4] == 2 for t in f), sum(t[0] == "bwd_persist" and t[4] == 2 for t in b))


def dgates_copies(c):
    """csn_lstm_plan_dgates_copies after a backward of a fresh plan: 2 behind the grouped weight-stationary backward (hand-off
    slabs and the row-major copy), 0 everywhere else."""
    return 2 if fz.expected_plan(c)[2] == "lstm_bwd_persist_kernel" else 0


# Every instantiation a plan can select.  lstm_fwd_persist_kernel<NQ, KS, DPOLL, RG, PARK>: the five (NQ, KS) of
# launch_fwd_persist, data polls or flags, 32- or 64-row groups; PARK only on <6, 6> with data polls (CSN_NO_FWD_PARK takes
# it off).  lstm_fwd_ns_kernel<KB, FUSE>: H / 32 of fwd_ns_supported's widths (not 768).  lstm_bwd_persist_kernel<2, KS,
# DPOLL, MASK, RG>: the six widths; the masked kernel has no 32-row form.  Path 4: KS = H / 64 of the six widths.
FWD_PERSIST_NQ_KS = ((6, 6), (6, 3), (8, 4), (8, 2), (8, 1))
FWD_NS_KB = (4, 8, 12, 16, 32)
BWD_PERSIST_KS = (4, 8, 12, 16, 24, 32)
F32_KS = (2, 4, 6, 8, 12, 16)
SELECTABLE = (
    {("fwd_persist", nq, ks, dpoll, rg, False) for nq, ks in FWD_PERSIST_NQ_KS for dpoll in (True, False) for rg in (2, 4)
     if (nq, ks, dpoll) != (6, 6, True)}
    | {("fwd_persist", 6, 6, True, rg, park) for rg in (2, 4) for park in (True, False)}
    | {("fwd_ns", kb, fuse) for kb in FWD_NS_KB for fuse in (True, False)}
    | {("bwd_persist", ks, dpoll, False, rg) for ks in BWD_PERSIST_KS for dpoll in (True, False) for rg in (2, 4)}
    | {("bwd_persist", ks, dpoll, True, 4) for ks in BWD_PERSIST_KS for dpoll in (True, False)}
    | {("f32_fwd", ks) for ks in F32_KS} | {("f32_bwd", ks) for ks in F32_KS}
    | {("il_fwd", 6), ("il_fwd", 8)}
    | {("il_bwd", nug, 4, mask) for nug in (3, 4) for mask in (True, False)})
# Built and never selected: the il kernels run only where cell_blk_supported holds, which requires H % 128 == 0.  Then
# H % 32 == 0, so launch_cell_fwd_il's nq is 6 (H % 24 == 0, i.e. 3 | H) or 8 and never 4; H % 64 == 0, so
# launch_cell_bwd_il's nug is 3 (3 | H) or 4 and never 2; and H / 32 is a multiple of 4, so pick_nk(H / 32, 4) is always 4.
UNREACHABLE = ({("il_fwd", 4)} | {("il_bwd", 3, nk, m) for nk in (3, 2, 1) for m in (True, False)}
               | {("il_bwd", 4, nk, m) for nk in (2, 1) for m in (True, False)}
               | {("il_bwd", 2, nk, m) for nk in (4, 2, 1) for m in (True, False)})
# kernels with a MASK template parameter (both values must be held to the emulator)
MASKED_KINDS = ("bwd_persist", "il_bwd")


# ---- the older tables as records ----------------------------------------------------------------------------------------------
def _table_record(shape, dtype, env, state, lengths=None, emu=True, source=""):
    c = record(*shape, "bf16" if dtype in ("bf16", st.BF16) else "f32", env, state=True)
    if state:
        c.update(state_in=("h0", "c0"), grads_in=st._BWD_IN, state_grads_out=("dh0", "dc0"))
    c.update(lengths=lengths, emu=emu, id=source)
    return c


def ledger_records():
    """Every record the ledger counts: those of this file (all held to the emulator, or to float64 on float32), and as
    records the cases of tests/test_gpu_lstm_state.py::CASES, the stateless float32 path-4 case of
    tests/test_gpu_bilstm.py::PLAN_CASES, the committed draw of tests/lstm_feature_fuzz.py (held to the emulator too),
    tests/test_gpu_half_tiles.py::CASES with its lengths case and the shapes of tests/test_gpu_fwd_park.py (bit identities
    between two forms: not held to a reference)."""
    out = [dict(c, emu=True) for c in records()]
    out += [dict(c, emu=False) for pair in half_tile_records() for c in pair]
    out += [dict(c, emu=False) for trio in diagonal_records() for c in trio]
    for name, (shape, dtype, _, env) in st.CASES.items():
        out.append(_table_record(shape, dtype, env, True, source="state:" + name))
    shape, dtype, _, env, state = tb.PLAN_CASES["f32_path4_stateless"]
    c = _table_record(shape, dtype, env, False, source="bilstm:f32_path4_stateless")
    c.update(state=False, outputs=st._OUT_KEYS[:2])
    out.append(c)
    out += [dict(c, emu=True) for c in fz.cases(fz.SEED, fz.N)]
    for name, (shape, chunk, state, forms) in ht.CASES.items():
        for form in forms:
            for extra in ({}, {"CSN_NO_HALF_TILES": "1"}):
                env = {"CSN_LSTM_CHUNK": str(chunk), **form, **extra}
                out.append(_table_record(shape, "bf16", env, state, emu=False, source="half_tiles:" + name))
    # test_half_tiles_with_lengths (its lengths hold 0 and T)
    rng = np.random.default_rng(11)
    n = [int(v) for v in rng.integers(0, 73, 256)]
    n[0], n[1], n[255] = 72, 0, 33
    for extra in ({}, {"CSN_NO_HALF_TILES": "1"}):
        out.append(_table_record((256, 72, 128, 768, 2), "bf16", {"CSN_LSTM_CHUNK": "32", **extra}, True, lengths=n, emu=False,
                                 source="half_tiles:lengths"))
    # tests/test_gpu_fwd_park.py (H = 768): its stateless product of shapes, its four shapes with a state, its two poll forms
    park = [((B, T, C, 768, L), {}, False) for B in (1, 40, 130, 256) for T in (3, 33, 70) for L in (1, 2) for C in (128, 96)]
    park += [((B, T, C, 768, L), {}, True) for B, T, C, L in ((130, 70, 128, 2), (256, 33, 96, 2), (40, 70, 96, 1), (1, 3, 128, 1))]
    park += [((B, T, C, 768, L), form, state) for B, T, C, L in ((256, 70, 128, 2), (130, 33, 96, 2))
             for form in ({"CSN_DPOLL_NO_HINT": "1"}, {"CSN_FWD_HINT": "1"}) for state in (False, True)]
    for shape, form, state in park:
        for extra in ({}, {"CSN_NO_FWD_PARK": "1"}):
            out.append(_table_record(shape, "bf16", {**form, **extra}, state, emu=False, source="fwd_park"))
    return out
