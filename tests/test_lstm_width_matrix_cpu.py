"""No GPU: the case records of tests/lstm_width_matrix.py are legal and take the plans their regimes name; the ledger --
every template instantiation a plan can select is launched by a record, with state arguments, the masked and unmasked
forms by records that are held to a reference; and the hidden-size lists of the mirror are those of the dispatch code, so
that a width added to a kernel fails here until a record exists for it."""
import os
import re

import lstm_feature_fuzz as fz
import lstm_input_views as views
import lstm_schedule_probe as sp
import lstm_width_matrix as wm
import test_gpu_half_tiles as ht
import test_gpu_lstm_state as st
import test_gpu_stream_order as gso

CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "cerebralsignalnetworks_amd", "csrc")
WIDTHS = {128, 256, 384, 512, 768, 1024}
# the regimes the matrix was specified with: removing one fails here even where another record launches the same kernels
NAMED = {"ks384_fused", "ks384_gemm", "ks512", "ks384_flags", "ks512_flags", "ks384_l4", "ks512_b129", "ks512_b129_l3",
         "ns256_fused", "ns256_gemm", "ns384_fused", "ns384_gemm", "ns512_fused", "ns512_gemm", "p2_384", "p2_512", "p1_384",
         "p1_512", "p1_640", "p1_896", "f32p_256", "f32p_384", "f32p_512", "f32p_768", "f32p_1024_b260", "f32_state_384",
         "f32_state_512"}


def _source(name):
    with open(os.path.join(CSRC, name)) as f:
        return f.read()


def test_records_are_legal_and_take_the_plan_their_regime_names():
    """The rules of lstm_feature_fuzz.check_legal without the regime lookup and the fuzz ranges."""
    cs = wm.records()
    assert len({c["id"] for c in cs}) == len(cs) and NAMED <= set(wm.REGIMES)
    for c in cs:
        r = wm.REGIMES[c["regime"]]
        B, T, I, H, L = r["shape"]
        assert (c["B"], c["T"], c["I"], c["H"], c["L"], c["dtype"], c["env"]) == (B, T, I, H, L, r["dtype"], r["env"])
        assert B * T <= 260 * 9 and c["env"]["CSN_LSTM_CHUNK"] == wm.CHUNK
        assert T > 2 * int(wm.CHUNK) or c["regime"] == "f32p_1024_b260"       # both chunk boundaries inside the sequence
        assert c["outputs"] and c["grads_in"]
        if not c["state"]:
            assert c["lengths"] is None and not c["state_in"] and not c["state_grads_out"]
            assert set(c["outputs"]) <= {"y_last", "y_all"} and set(c["grads_in"]) <= {"dy_last", "dy_all"}
        assert set(c["outputs"]) <= set(st._OUT_KEYS) and set(c["grads_in"]) <= set(st._BWD_IN)
        if c["lengths"] is not None:
            assert len(c["lengths"]) == B and all(0 <= v <= T for v in c["lengths"]) and {0, T} <= set(c["lengths"])
            assert all(c["lengths"][row] == c["lengths"][0] for row in wm.copy_rows(B))
        assert (c["dropout"] is not None) == c["dropout_plan"] and (c["dropout"] is None or L >= 2)
        assert (not c["y_pitch"] or "y_all" in c["outputs"]) and (not c["dy_pitch"] or "dy_all" in c["grads_in"])
        assert (not c["dx_add"] or c["want_dx"]) and (c["x_view"] is None or c["x_view"] in views.VIEWS)
        assert fz.expected_plan(c) == r["plan"], (c["id"], fz.expected_plan(c))
        # a bf16 regime is a state plan, a float32 path-4 regime a stateless one
        assert c["state"] == (r["plan"][0] != 4) and (c["dtype"] == "bf16" or r["plan"][0] in (0, 4))
        if r["fuse"] is not None:
            ns = r["plan"][1] == "lstm_fwd_ns_kernel"
            assert r["plan"][0] in (2, 3) and views.fuse_x(ns, I, H) == r["fuse"], c["id"]
        assert wm.copy_rows(B), c["id"]
    # the feature sets: state regimes none / state / lengths / state_lengths / all, path 4 none / all_stateless
    for name in NAMED:
        r = wm.REGIMES[name]
        assert r["sets"] == (wm.STATELESS_SETS if r["plan"][0] == 4 else wm.STATE_SETS), name
    on = fz.features(wm.feature_record("ks384_fused", "all"))
    assert all(on[k] for k in ("reverse", "lengths", "state_args", "dropout", "y_pitch", "dy_pitch", "dx_add", "accumulate", "callback"))
    on = fz.features(wm.feature_record("f32p_512", "all_stateless"))
    assert all(on[k] for k in ("reverse", "dropout", "y_pitch", "dy_pitch", "dx_add", "x_view", "accumulate", "callback"))
    on = fz.features(wm.feature_record("ks512", "none"))      # (no state gradient comes in: that much is a subset)
    assert not any(v for k, v in on.items() if k != "grad_subset")


def test_the_ungrouped_form_and_the_second_launch_are_run_on_purpose():
    c = wm.feature_record("ks512_b129_l3", "state")
    assert fz.expected_plan(c) == (3, "lstm_fwd_persist_kernel", "lstm_cell_bwd_il_kernel")
    f, b = wm.launches(c)
    assert f == [("fwd_persist", 8, 4, True, 4, False)] * 9 and b == [("il_bwd", 4, 4, False)]
    assert wm.half_tile_launches(c) == (0, 0) and wm.dgates_copies(c) == 0
    f, b = wm.launches(wm.feature_record("f32p_1024_b260", "none"))          # five tiles, four per launch, two layers
    assert f == [("f32_fwd", 16)] * 4 and b == [("f32_bwd", 16)] * 4
    # launches of one and two layers at B 65 are all on 32-row groups, of three and four layers on 64
    f, b = wm.launches(wm.feature_record("ks384_l4", "state"))
    assert {t[4] for t in f} == {2, 4} == {t[4] for t in b}
    c = wm.feature_record("ks384_fused", "lengths")
    assert wm.half_tile_launches(c)[0] > 0 and wm.half_tile_launches(c)[1] == 0 and {t[3] for t in wm.launches(c)[1]} == {True}
    # the N-split kernel's fused form only in the launches that hold layer 0
    assert {t[2] for t in wm.launches(wm.feature_record("ns384_fused", "state"))[0]} == {True, False}
    assert {t[2] for t in wm.launches(wm.feature_record("ns384_gemm", "state"))[0]} == {False}


def test_the_mirror_counts_the_32_row_launches_as_the_half_tile_test_does():
    for c in wm.ledger_records():
        if not c["id"].startswith("half_tiles:"):
            continue
        want = ht._expected_half_launches(c["B"], c["T"], c["H"], c["L"], int(c["env"]["CSN_LSTM_CHUNK"]), c["env"], c["lengths"])
        assert wm.half_tile_launches(c) == want, (c["id"], c["env"], wm.half_tile_launches(c), want)
        assert wm.dgates_copies(c) == 2


def test_the_mirror_counts_the_launches_of_the_schedules_the_library_builds(tmp_path):
    """The weight-stationary records of the ledger against fwd_persist_schedule / bwd_persist_schedule (csrc/lstm_schedule.h,
    through the host-only program of tests/lstm_schedule_probe.py): the launches on 32-row groups, the recurrence launches
    (the occupied diagonals of the mirror; a merged launch covers one per round), and the form of the forward."""
    ask = sp.build(tmp_path)
    recs, queries = [], []
    for c in wm.ledger_records():
        _, fwd, bwd = fz.expected_plan(c)
        steps = c["T"] if c["lengths"] is None else max(c["lengths"])
        if steps == 0 or not {fwd, bwd} & {st._PF, st._NSF, "lstm_bwd_persist_kernel"}:
            continue
        env = c["env"]
        shape = (steps, c["B"], c["H"], c["L"], max(1, int(env.get("CSN_LSTM_CHUNK", 32))))
        no_half = wm._on(env, "CSN_NO_HALF_TILES")
        recs.append((c, fwd, bwd))
        queries.append(sp.fwd_query(*shape, fwd_ns=fwd == st._NSF, persist_streams=wm._on(env, "CSN_PERSIST_STREAMS"), no_half=no_half))
        queries.append(sp.bwd_query(*shape, lengths=c["lengths"] is not None, dropout=c["dropout"] is not None,
                                    dh_n="dh_n" in c["grads_in"], flags=wm._on(env, "CSN_BWD_FLAGS"),
                                    no_beside=wm._on(env, "CSN_NO_BESIDE"), no_merge=wm._on(env, "CSN_BWD_NO_MERGE"), no_half=no_half))
    answers = ask(queries)
    assert len(recs) > 100
    seen = set()
    for i, (c, fwd, bwd) in enumerate(recs):
        real_f, real_b = answers[2 * i], answers[2 * i + 1]
        f, b = wm.launches(c)
        half = wm.half_tile_launches(c)
        if fwd in (st._PF, st._NSF):
            assert len(real_f["launches"]) == len(f), (c["id"], c["env"])
            assert sum(q["half"] for q in real_f["launches"]) == half[0], (c["id"], c["env"])
            seen.add(fwd)
        if bwd == "lstm_bwd_persist_kernel":
            assert sum(q["nrounds"] for q in real_b if q["slots"]) == len(b), (c["id"], c["env"])
            assert sum(q["half"] * q["nrounds"] for q in real_b) == half[1], (c["id"], c["env"])
            seen.add(bwd)
    assert seen == {st._PF, st._NSF, "lstm_bwd_persist_kernel"}
    # the form of the forward: the cases of tests/test_gpu_stream_order.py that name theirs
    for name, streams in gso.STREAM_FORM.items():
        shape, dtype, _, env = gso._case(name)[:4]
        B, T, I, H, L = shape
        path, fwd, _ = fz.expected_plan(wm.record(B, T, I, H, L, "bf16", env))
        assert dtype == st.BF16 and path in (2, 3) and fwd in (st._PF, st._NSF), name
        [real] = ask([sp.fwd_query(T, B, H, L, int(env.get("CSN_LSTM_CHUNK", 32)), fwd_ns=fwd == st._NSF,
                                   persist_streams=env.get("CSN_PERSIST_STREAMS") == "1")])
        assert (real["form"] == "layer_streams") == gso._forward_takes_layer_streams(shape, env, fwd) == streams, (name, real["form"])
        assert real["form"] != "caller_stream", name


def test_the_ledger():
    recs = wm.ledger_records()
    union = set().union(*(wm.instantiations(c) for c in recs))
    assert union == wm.SELECTABLE, (sorted(wm.SELECTABLE - union, key=str), sorted(union - wm.SELECTABLE, key=str))
    assert not wm.SELECTABLE & wm.UNREACHABLE
    # ... by a record with state arguments (path 4 takes stateless plans only: a float32 state plan is path 0)
    with_state = set().union(*(wm.instantiations(c) for c in recs if c["state_in"]))
    assert wm.SELECTABLE - with_state == {t for t in wm.SELECTABLE if t[0] in ("f32_fwd", "f32_bwd")}, sorted(
        wm.SELECTABLE - with_state, key=str)
    # ... and every path-4 instantiation by a record of this file, held to float64
    own = set().union(*(wm.instantiations(c) for c in wm.records()))
    assert {t for t in wm.SELECTABLE if t[0] in ("f32_fwd", "f32_bwd") and t[1] != 2} <= own
    # kernels with a MASK parameter: at every width, the masked and the unmasked form by a record held to the emulator
    held = set().union(*(wm.instantiations(c) for c in recs if c["emu"]))
    for kind in wm.MASKED_KINDS:
        for size in {t[1] for t in wm.SELECTABLE if t[0] == kind}:
            masks = {t[3] for t in held if t[0] == kind and t[1] == size}
            assert masks == {True, False}, (kind, size, masks)
    # ... and what this file adds for the widths nothing held to a state before: every form of H 384 and H 512
    for t in wm.SELECTABLE:
        if (t[0] == "fwd_persist" and t[1:3] in ((6, 3), (8, 4))) or (t[0] == "bwd_persist" and t[1] in (12, 16)) or (
                t[0] == "fwd_ns" and t[1] in (8, 12, 16)):
            assert any(t in wm.instantiations(c) and c["state_in"] for c in wm.records()), t


def test_the_unreachable_instantiations_follow_from_the_dispatch():
    """cell_blk_supported requires H % 128 == 0; launch_cell_fwd_il / launch_cell_bwd_il / pick_nk as they stand."""
    src = _source("lstm_cell_blk.hip")
    assert re.search(r"return dtype == CSN_BF16 && H % 128 == 0 && !opt\.cell_v1;", src)
    assert "(H % 24 == 0) ? 6 : ((H % 32 == 0) ? 8 : 4)" in src and "(H % 48 == 0) ? 3 : ((H % 64 == 0) ? 4 : 2)" in src
    assert "pick_nk(steps, 4)" in src and "const int steps = H / 32;" in src
    built_fwd = {("il_fwd", int(nq)) for nq, _ in re.findall(r"CSN_CASE\((\d), (1)\)", src.split("launch_cell_bwd_il")[0])}
    built_bwd = {("il_bwd", int(g), int(k), m) for g, k in re.findall(r"CSN_CASE\((\d), (\d)\);", src.split("int launch_cell_bwd_il")[1])
                 for m in (True, False)}
    taken = set()
    for H in range(128, 4097, 128):
        nq = 6 if H % 24 == 0 else 8 if H % 32 == 0 else 4
        nug = 3 if H % 48 == 0 else 4 if H % 64 == 0 else 2
        nk = next(k for k in (4, 3, 2, 1) if (H // 32) % k == 0)
        taken |= {("il_fwd", nq), ("il_bwd", nug, nk, True), ("il_bwd", nug, nk, False)}
    il = {t for t in wm.SELECTABLE if t[0] in ("il_fwd", "il_bwd")}
    assert taken == il and (built_fwd | built_bwd) - il == wm.UNREACHABLE


def test_the_hidden_sizes_are_those_of_the_dispatch_tables():
    """Read out of the source text: a width added to a kernel fails here (or in the ledger) until a record exists."""
    src = _source("lstm_fwd_persist.hip")
    rows = re.findall(r"if \(nq == (\d+) && ks == (\d+)\) return launch_persist_t<(\d+), (\d+)>\(a, st\);", src)
    assert len(rows) == len(re.findall(r"return launch_persist_t<", src)) == 5 and all(r[:2] == r[2:] for r in rows)
    assert {(int(a), int(b)) for a, b, _, _ in rows} == set(wm.FWD_PERSIST_NQ_KS)
    assert "(nq == 6 && (ks == 6 || ks == 3)) || (nq == 8 && (ks == 4 || ks == 2 || ks == 1))" in src
    # the mirror of fz.expected_plan knows the same widths
    assert {128 * ks for _, ks in wm.FWD_PERSIST_NQ_KS} | {1024} == set(fz._WS_H) == WIDTHS

    src = _source("lstm_fwd_ns.hip")
    assert {int(k) for k in re.findall(r"^\s*CSN_NS_CASE\((\d+)\);", src, re.M)} == set(wm.FWD_NS_KB)
    assert "case KBV * 32:" in src and len(re.findall(r"launch_ns_t<", src)) == 2
    supported = src.split("bool fwd_ns_supported")[1].split("}")[0]
    assert {int(h) for h in re.findall(r"H == (\d+)", supported)} - {768} == {32 * kb for kb in wm.FWD_NS_KB} == WIDTHS - {768}

    src = _source("lstm_bwd_persist.hip")
    rows = re.findall(r"case (\d+): return launch_bwd_persist_t<2, (\d+)>\(a, st, lengths\);", src)
    assert len(rows) == len(re.findall(r"return launch_bwd_persist_t<", src)) and all(int(h) == 32 * int(ks) for h, ks in rows)
    assert {int(ks) for _, ks in rows} == set(wm.BWD_PERSIST_KS)
    supported = src.split("bool bwd_persist_supported")[1].split("}")[0]
    assert {int(h) for h in re.findall(r"H == (\d+)", supported)} == WIDTHS

    src = _source("lstm_f32_persist.hip")
    for which in ("fwd", "bwd"):
        rows = re.findall(rf"case (\d+): return launch_{which}_t<(\d+)>\(a, st\);", src)
        last = re.findall(rf"default: return launch_{which}_t<(\d+)>\(a, st\);", src)
        assert len(rows) + len(last) == len(re.findall(rf"return launch_{which}_t<", src)) and len(last) == 1
        assert all(int(h) == 64 * int(ks) for h, ks in rows)
        assert {int(ks) for _, ks in rows} | {int(last[0])} == set(wm.F32_KS)
    supported = src.split("bool f32_persist_supported")[1].split("}")[0]
    assert {int(h) for h in re.findall(r"H == (\d+)", supported)} == {64 * ks for ks in wm.F32_KS} == WIDTHS
    assert "int f32_persist_tiles_per_launch(int H) { return 256 / (H / 16); }" in src
