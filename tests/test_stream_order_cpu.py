"""CPU: the stream-order case table covers the header, and the helpers of tests/stream_order.py do what the GPU tests
(tests/test_gpu_stream_order.py) rely on."""
import os
import re

import pytest
import torch

import stream_order as so
import channel_discovery_stream_cases  # noqa: F401  (these two join the stream-order case table on import: without them
import distill_loss_stream_cases  # noqa: F401   this module, run on its own, misses their entry points in the table)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _declarations(header_text):
    """(name, parameter text) of every csn_* function include/csn_hip.h declares."""
    text = re.sub(r"/\*.*?\*/", " ", header_text, flags=re.S)
    text = re.sub(r"//[^\n]*", " ", text)
    text = re.sub(r"^\s*#[^\n]*", " ", text, flags=re.M)
    found = []
    for decl in text.split(";"):
        m = re.search(r"\b(csn_\w+)\s*\(([^()]*)\)\s*$", decl, flags=re.S)
        if m:
            found.append((m.group(1), m.group(2)))
    return found


def _entry_points_with_a_stream(header_text):
    """Names of the functions include/csn_hip.h declares with a csnStream_t parameter."""
    return [name for name, params in _declarations(header_text) if re.search(r"\bcsnStream_t\b", params)]


def _plan_setters(header_text):
    """Names of the csn_lstm_plan_set_* functions include/csn_hip.h declares."""
    return [name for name, _ in _declarations(header_text) if name.startswith("csn_lstm_plan_set_")]


def _header():
    with open(os.path.join(ROOT, "include", "csn_hip.h")) as f:
        return f.read()


def test_parser_finds_declarations_and_only_those():
    text = """/* csn_in_comment(csnStream_t s); */
    typedef void* csnStream_t;
    int csn_a(const float* x, int n,
              csnStream_t stream);
    size_t csn_a_scratch_bytes(int n);
    int csn_b(csnStream_t stream, int* out);   // int csn_c(csnStream_t s);
    typedef void (*csnFn)(void* user, int layer);
    int csn_d(csnFn fn, void* user);"""
    assert _entry_points_with_a_stream(text) == ["csn_a", "csn_b"]
    assert [n for n, _ in _declarations(text)] == ["csn_a", "csn_a_scratch_bytes", "csn_b", "csn_d"]
    assert _plan_setters("int csn_lstm_plan_set_x(csnLstmPlan* plan, csnFn fn, void* user); /* csn_lstm_plan_set_y(int a); */\n"
                         "int csn_lstm_plan_path(const csnLstmPlan* plan);") == ["csn_lstm_plan_set_x"]


def test_case_table_names_exactly_the_entry_points_that_take_a_stream():
    declared = _entry_points_with_a_stream(_header())
    assert len(declared) == len(set(declared)) and len(declared) >= 22, declared
    missing = sorted(set(declared) - set(so.CASE_TABLE))
    stale = sorted(set(so.CASE_TABLE) - set(declared))
    assert not missing, f"entry points with a csnStream_t but no stream-order case: {missing}"
    assert not stale, f"CASE_TABLE names functions the header does not declare with a csnStream_t: {stale}"


def test_a_removed_table_entry_is_noticed(monkeypatch):
    table = dict(so.CASE_TABLE)
    del table["csn_gemm_nt"]
    monkeypatch.setattr(so, "CASE_TABLE", table)
    with pytest.raises(AssertionError, match="csn_gemm_nt"):
        test_case_table_names_exactly_the_entry_points_that_take_a_stream()


def test_every_table_entry_is_a_case_or_a_reason():
    gpu_tests = _gpu_tests()
    for name, entry in so.CASE_TABLE.items():
        if isinstance(entry, so.InTest):
            assert entry.tests and set(entry.tests) <= gpu_tests, (name, entry.tests)
        else:
            assert entry and all(isinstance(c, so.Stateless) and c.entry == name and callable(c.build) for c in entry), name
    ids = [c.id for c in so.STATELESS_CASES]
    assert len(ids) == len(set(ids))
    assert "test_stateless_entry_point_with_late_inputs" in gpu_tests


def _gpu_tests():
    with open(os.path.join(ROOT, "tests", "test_gpu_stream_order.py")) as f:
        return set(re.findall(r"^def (test_\w+)\(", f.read(), flags=re.M))


def test_plan_setters_table_names_exactly_the_setters_of_the_header():
    declared = _plan_setters(_header())
    assert len(declared) == len(set(declared)) and len(declared) >= 6, declared
    missing = sorted(set(declared) - set(so.PLAN_SETTERS))
    stale = sorted(set(so.PLAN_SETTERS) - set(declared))
    assert not missing, f"csn_lstm_plan_set_* functions with no stream-order test: {missing}"
    assert not stale, f"PLAN_SETTERS names functions the header does not declare: {stale}"
    gpu_tests = _gpu_tests()
    for name, tests in so.PLAN_SETTERS.items():
        assert tests and set(tests) <= gpu_tests, (name, sorted(set(tests) - gpu_tests))
        # a setter only matters through the calls that follow it: its tests are tests of the forward or the backward
        assert set(tests) <= set(so.CASE_TABLE["csn_lstm_forward"].tests) | set(so.CASE_TABLE["csn_lstm_backward"].tests), name


def test_a_removed_setter_or_a_test_that_does_not_exist_is_noticed(monkeypatch):
    full = dict(so.PLAN_SETTERS)
    table = dict(full)
    del table["csn_lstm_plan_set_views"]
    monkeypatch.setattr(so, "PLAN_SETTERS", table)
    with pytest.raises(AssertionError, match="csn_lstm_plan_set_views"):
        test_plan_setters_table_names_exactly_the_setters_of_the_header()
    table = dict(full, csn_lstm_plan_set_io=("test_that_was_renamed",))
    monkeypatch.setattr(so, "PLAN_SETTERS", table)
    with pytest.raises(AssertionError, match="test_that_was_renamed"):
        test_plan_setters_table_names_exactly_the_setters_of_the_header()
    monkeypatch.setattr(so, "PLAN_SETTERS", dict(full, csn_lstm_plan_set_nothing=("test_lstm_forward_with_late_inputs",)))
    with pytest.raises(AssertionError, match="csn_lstm_plan_set_nothing"):
        test_plan_setters_table_names_exactly_the_setters_of_the_header()


def _check_settings(shape, state, f, S_Tsrc=None):
    B, T, I, H, L = shape
    n = f["lengths"]
    if n is not None:
        assert state and len(n) == B and all(0 <= v <= T for v in n)
    if f["dropout"] is not None:
        assert L >= 2 and 0.0 < f["dropout"][0] < 1.0          # with one layer there is no interface to drop
    if f["views"] is not None:
        rows, starts, S, Tsrc = f["views"]
        assert S == max(1, B // 3) and len(rows) == len(starts) == B
        assert all(0 <= r < S for r in rows)
        assert all(t0 >= 0 and t0 + k <= Tsrc for t0, k in zip(starts, n or [T] * B))


def test_feature_settings_are_legal_for_every_case_and_feature_set():
    for name, (shape, state) in so.FEATURE_CASES.items():
        B, T, I, H, L = shape
        assert L >= 2 and H % 4 == 0                            # (the [B,T,2H] halves start on 16 bytes)
        for fs, parts in so.FEATURE_SETS.items():
            f = so.feature_settings(name, fs)
            _check_settings(shape, state, f)
            assert (f["dropout"] is not None) == ("dropout" in parts) and f["reverse_io"] == ("reverse_io" in parts)
            assert (f["views"] is not None) == ("windows" in parts) and (f["lengths"] is not None) == ("lengths" in parts and state)
            if f["views"] is not None:
                assert f["views"][3] == T + 7
            if f["lengths"] is not None:                        # two_mixed: some rows T (the plan's own T is reached), the rest shorter
                assert max(f["lengths"]) == T and 0 < min(f["lengths"]) < T
    assert so.two_mixed_lengths(8, 40) == [40, 40] + [26] * 6
    assert so.feature_settings("v1_h96", "all") == so.feature_settings("v1_h96", "all")          # fixed seeds


def test_settings_a_and_b_differ_in_every_row():
    for name in so.SETTINGS_CASES:
        shape, state = so.FEATURE_CASES[name]
        a, b = so.settings_a_and_b(name)
        for f in (a, b):
            _check_settings(shape, state, {**f, "reverse_io": False})
        assert all(x != y for x, y in zip(a["lengths"], b["lengths"]))
        (ra, ta, Sa, Tsa), (rb, tb, Sb, Tsb) = a["views"], b["views"]
        assert all(x != y for x, y in zip(ra, rb)) and all(x != y for x, y in zip(ta, tb))
        assert Sa == Sb and Tsa != Tsb
        assert all(x != y for x, y in zip(a["dropout"], b["dropout"]))


def test_late_holds_poison_until_the_copy():
    seen = {}
    real = torch.arange(12, dtype=torch.float32).reshape(3, 4)
    arg = so.late(None, real, before_copy=lambda a: seen.setdefault("before", a.clone()))
    assert bool(torch.isnan(seen["before"]).all()) and seen["before"].shape == real.shape
    assert torch.equal(arg, real) and arg.data_ptr() != real.data_ptr()
    ints = torch.arange(1, 7, dtype=torch.int64)
    arg = so.late(None, ints, before_copy=lambda a: seen.setdefault("ints", a.clone()))
    assert bool((seen["ints"] == so.INT_POISON).all()) and torch.equal(arg, ints)
    d = so.late(None, torch.ones(3, dtype=torch.float64), poison=float("inf"), before_copy=lambda a: seen.setdefault("inf", a.clone()))
    assert bool(torch.isinf(seen["inf"]).all()) and bool((d == 1).all())


def test_snapshot_then_poison_clones_first_and_poisons_every_input():
    x, w = torch.ones(4), [torch.ones(2, 2), torch.ones(3)]
    inout = torch.full((5,), 2.0)
    idx = torch.arange(3)
    outputs = {"y": torch.full((4,), 7.0), "state": inout, "none": None, "idx": idx}
    snaps = so.snapshot_then_poison(None, outputs, {"x": x, "w": w, "state": inout, "none": None})
    assert set(snaps) == set(outputs) and snaps["none"] is None
    assert bool((snaps["y"] == 7).all()) and bool((snaps["state"] == 2).all()) and torch.equal(snaps["idx"], idx)
    assert snaps["state"].data_ptr() != inout.data_ptr()
    for t in (x, inout, *w):
        assert bool(torch.isnan(t).all())
    assert bool((outputs["y"] == 7).all())            # an output that is no input is left alone
    ints = torch.arange(1, 4)
    so.snapshot_then_poison(None, {}, [ints])
    assert bool((ints == so.INT_POISON).all())


def test_same_bits_tells_nan_payloads_and_signed_zeros_apart():
    a = torch.tensor([0.0, float("nan"), 1.0])
    assert so.same_bits(a, a.clone())
    assert not so.same_bits(a, torch.tensor([-0.0, float("nan"), 1.0]))
    b = a.clone()
    b.view(torch.int32)[1] += 1                       # another NaN
    assert not so.same_bits(a, b)
    assert not so.same_bits(a, a.double())
    with pytest.raises(AssertionError, match=r"w\[1\]"):
        so.assert_same_bits({"x": [a, a], "w": [a, b]}, {"x": [a, a], "w": [a, a]}, "case")
    for got in ({"x": [a, a], "w": None}, {"x": [a]}, {}):          # a missing output is no shorter comparison
        with pytest.raises(AssertionError, match="outputs"):
            so.assert_same_bits(got, {"x": [a, a], "w": [a, a]}, "case")
    so.assert_same_bits({"x": [a, a]}, {"x": [a, a.clone()]}, "case")


def test_delay_length_rule():
    assert so.delay_ms_for(0.0) == 20.0 and so.delay_ms_for(0.010) == pytest.approx(50.0)


def test_gemm_route_mirrors_name_the_routes_of_the_cases():
    routes = [so.gemm_nt_route(*a) for a in ((4096, 4096, 128, torch.bfloat16), (16384, 768, 128, torch.bfloat16),
                                             (256, 1024, 256, torch.bfloat16), (130, 132, 64, torch.bfloat16),
                                             (70, 132, 40, torch.bfloat16), (33, 20, 7, torch.float32))]
    assert routes == ["wide256", "wide192", "tile256x128", "dma", "bf16", "generic"]
    # the two shapes csrc/gemm_nt.hip quotes: 16 x 32 tiles of 192 fill two rounds, 128 tiles of 192 do not fill one
    assert so.gemm_nt_route(8192, 3072, 768, torch.bfloat16) == "wide192"
    assert so.gemm_nt_route(8192, 768, 3072, torch.bfloat16) == "dma"
    assert [so.gemm_tn_route(136, 72, 600), so.gemm_tn_route(256, 256, 8192), so.gemm_tn_route(256, 120, 8192)] == ["tile128", "tile256", "tile128"]


_ROUTE_SWITCHES = ("CSN_GEMM_GENERIC", "CSN_GEMM_NO_DMA", "CSN_GEMM_NO_256", "CSN_GEMM_NO_192", "CSN_NT_NO_W4",
                   "CSN_TN_NO_STAGGER", "CSN_TN_STAGES", "CSN_TN_NO_TR")
_SWEEP = [(M, N, K) for M in (8, 136, 255, 256, 264, 4088, 4096, 8192, 16384)
          for N in (4, 72, 76, 128, 192, 768, 1024, 1028, 3072, 4096) for K in (7, 40, 64, 72, 128, 256, 768, 8192)]


def _only(monkeypatch, env):
    for name in _ROUTE_SWITCHES:
        monkeypatch.delenv(name, raising=False)
    for name, value in env.items():
        monkeypatch.setenv(name, value)


def test_gemm_nt_route_mirror_agrees_with_the_library(monkeypatch):
    """The hand-written mirror so.gemm_nt_route against what the library says it launches (cabi.gemm_nt_route), over a
    sweep of shapes, both operand types, every single switch, and misaligned operands.  The mirror calls both forms of the
    192 tile "wide192"; which form it is follows from CSN_NT_NO_W4 alone here (every swept operand is far below the
    4 GiB window of the four-wave kernel)."""
    from cerebralsignalnetworks_amd import cabi
    envs = [({}, {}), ({"CSN_GEMM_GENERIC": "1"}, {"generic": True}), ({"CSN_GEMM_NO_DMA": "1"}, {"no_dma": True}),
            ({"CSN_GEMM_NO_256": "1"}, {"no_256": True}), ({"CSN_GEMM_NO_192": "1"}, {"no_192": True}),
            ({"CSN_NT_NO_W4": "1"}, {"no_w4": True})]
    for env, kw in envs:
        _only(monkeypatch, env)
        for aligned in ((True, False) if not env else (True,)):
            for dtype in (torch.bfloat16, torch.float32):
                for (M, N, K) in _SWEEP:
                    want = so.gemm_nt_route(M, N, K, dtype, aligned16=aligned, **kw)
                    if want == "wide192" and not kw.get("no_w4"):
                        want = "wide192w4"
                    assert cabi.gemm_nt_route(M, N, K, dtype, aligned) == want, (M, N, K, dtype, aligned, env)
    # the routes the parent's ladder gives, read line by line
    _only(monkeypatch, {})
    table = [((8192, 3072, 768), "wide192w4"), ((8192, 4096, 1024), "wide256"), ((8192, 768, 3072), "dma"),
             ((8192, 1024, 768), "tile256x128"), ((4088, 3072, 128), "wide192w4"), ((4088, 4096, 128), "wide256"),
             ((264, 1028, 256), "tile256x128"), ((136, 76, 64), "dma"), ((136, 76, 72), "bf16"), ((136, 76, 70), "generic")]
    for shape, want in table:
        assert cabi.gemm_nt_route(*shape) == want, shape
    _only(monkeypatch, {"CSN_NT_NO_W4": "1"})
    assert cabi.gemm_nt_route(8192, 3072, 768) == "wide192"


def _tn_kernel_behind(route, N, colsum, no_stagger=False, stages=4, no_tr=False):
    """The kernel behind a TN route, as the ladder of launch_gemm_tn_slabs chose it before there was a route function."""
    if route == "tile256":
        if not no_stagger and stages == 4:
            return "w4-128" if N <= 128 else "w4-256"
        if colsum:
            return "ring4"
        return {3: "ring3", 5: "ring5"}.get(stages, "ring4")
    return {"tile128": "tn128-notr" if no_tr else "tn128", "generic": "generic"}[route]


def test_gemm_tn_route_mirrors_agree_with_the_library(monkeypatch):
    """so.gemm_tn_route and gemm_tn_splits.regime against cabi.gemm_tn_route over the same sweep, with and without
    column sums, under every single switch of the 256-tile kernels, and for misaligned operands."""
    import gemm_tn_splits as sp
    from cerebralsignalnetworks_amd import cabi
    envs = [({}, {}, {}), ({"CSN_GEMM_NO_256": "1"}, {"no_256": True}, {}),
            ({"CSN_TN_NO_STAGGER": "1"}, {}, {"no_stagger": True}), ({"CSN_TN_STAGES": "3"}, {}, {"stages": 3}),
            ({"CSN_TN_STAGES": "5"}, {}, {"stages": 5}), ({"CSN_TN_NO_TR": "1"}, {}, {"no_tr": True})]
    family = {"tn256": "tile256", "tn128": "tile128", "f32_128": "generic", "generic": "generic"}
    for env, route_kw, kernel_kw in envs:
        _only(monkeypatch, env)
        for aligned in ((True, False) if not env else (True,)):
            for bf16 in (True, False):
                for (M, N, K) in _SWEEP:
                    if bf16 and aligned and M % 8 == 0 and N % 8 == 0:
                        route = so.gemm_tn_route(M, N, K, **route_kw)
                        assert family[sp.regime(M, N, K, True, **route_kw).kernel] == route, (M, N, K, env)
                    elif aligned:
                        route = family[sp.regime(M, N, K, bf16, **route_kw).kernel]
                        assert route == "generic", (M, N, K, bf16)
                    else:
                        route = "generic"                   # misaligned operands: neither bf16 kernel family
                    for colsum in (False, True):
                        want = (route, _tn_kernel_behind(route, N, colsum, **kernel_kw))
                        got = cabi.gemm_tn_route(M, N, K, torch.bfloat16 if bf16 else torch.float32, aligned, colsum)
                        assert got == want, (M, N, K, bf16, aligned, colsum, env)
