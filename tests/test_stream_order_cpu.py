"""CPU: the stream-order case table covers the header, and the helpers of tests/stream_order.py do what the GPU tests
(tests/test_gpu_stream_order.py) rely on."""
import os
import re

import pytest
import torch

import stream_order as so

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _entry_points_with_a_stream(header_text):
    """Names of the functions include/csn_hip.h declares with a csnStream_t parameter."""
    text = re.sub(r"/\*.*?\*/", " ", header_text, flags=re.S)
    text = re.sub(r"//[^\n]*", " ", text)
    text = re.sub(r"^\s*#[^\n]*", " ", text, flags=re.M)
    names = []
    for decl in text.split(";"):
        m = re.search(r"\b(csn_\w+)\s*\(([^()]*)\)\s*$", decl, flags=re.S)
        if m and re.search(r"\bcsnStream_t\b", m.group(2)):
            names.append(m.group(1))
    return names


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
    with open(os.path.join(ROOT, "tests", "test_gpu_stream_order.py")) as f:
        gpu_tests = set(re.findall(r"^def (test_\w+)\(", f.read(), flags=re.M))
    for name, entry in so.CASE_TABLE.items():
        if isinstance(entry, so.InTest):
            assert entry.tests and set(entry.tests) <= gpu_tests, (name, entry.tests)
        else:
            assert entry and all(isinstance(c, so.Stateless) and c.entry == name and callable(c.build) for c in entry), name
    ids = [c.id for c in so.STATELESS_CASES]
    assert len(ids) == len(set(ids))
    assert "test_stateless_entry_point_with_late_inputs" in gpu_tests


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
    # the two shapes csrc/gemm.hip quotes: 16 x 32 tiles of 192 fill two rounds, 128 tiles of 192 do not fill one
    assert so.gemm_nt_route(8192, 3072, 768, torch.bfloat16) == "wide192"
    assert so.gemm_nt_route(8192, 768, 3072, torch.bfloat16) == "dma"
    assert [so.gemm_tn_route(136, 72, 600), so.gemm_tn_route(256, 256, 8192), so.gemm_tn_route(256, 120, 8192)] == ["tile128", "tile256", "tile128"]
