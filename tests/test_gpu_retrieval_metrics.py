"""GPU: csn_topk_merge against retrieval.merge_topk, csn_topk_class_metrics against its numpy restatement,
retrieval.evaluate_device against retrieval.evaluate_full, their stream order, host refusals and the --device_eval flag of
the evaluation CLI.  Every comparison is exact."""
import json
import os
import re
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import retrieval_metrics_reference as ref
import retrieval_metrics_stream_cases as stream_cases
import test_gpu_stream_order as stream_tests
from cerebralsignalnetworks_amd import cabi, retrieval

pytestmark = pytest.mark.gpu

SENTINEL = -77
GUARD = 64


def _dev(a, device):
    return torch.from_numpy(np.ascontiguousarray(a)).to(device)


# ---- 1. csn_topk_merge against merge_topk ---------------------------------------------------------------------------------
def _staging_cases():
    """The smallest (P, k_in) with one candidate fewer than the staging limit, exactly the limit, and one more; k = 1024 on
    the middle one (P = 2, k_in = 1024)."""
    limit = cabi.TOPK_MERGE_STAGED_MAX
    cases = []
    for n, k in ((limit - 1, 100), (limit, 1024), (limit + 1, 100)):
        P = next(p for p in range(1, 65) if n % p == 0 and n // p <= 1024)
        D, I = ref.merge_case(P, 2, n // P, seed=n, values=6, pad_parts={P - 1: n // P - 3})
        cases.append((f"P{P}-kin{n // P}-k{k}-n{n}", D, I, k))
    return cases


def _row_count_cases():
    return [(f"nq{Nq}", *ref.merge_case(3, Nq, 5, seed=Nq, pad_parts={1: 2}), 5) for Nq in (1, 65, 300)]


def test_staging_cases_stand_on_both_sides_of_the_limit():
    shapes = [(c[1].shape[0], c[1].shape[2], c[3]) for c in _staging_cases()]
    assert cabi.TOPK_MERGE_STAGED_MAX == 2048 and shapes == [(23, 89, 100), (2, 1024, 1024), (3, 683, 100)]
    assert cabi.load().csn_topk_merge_staged_max() == cabi.TOPK_MERGE_STAGED_MAX


@pytest.mark.parametrize("case", ref.merge_cases() + _staging_cases() + _row_count_cases(), ids=lambda c: c[0])
def test_merge_equals_merge_topk(cuda, case):
    _, D, I, k = case
    want_d, want_i = retrieval.merge_topk(list(D), list(I), k)
    out = cabi.topk_merge(_dev(D, cuda), _dev(I, cuda), k)
    assert torch.equal(out["idx"].cpu(), torch.from_numpy(want_i))
    assert torch.equal(out["dist64"].cpu(), torch.from_numpy(want_d))
    assert torch.equal(out["dist"].cpu(), torch.from_numpy(want_d.astype(np.float32)))
    got_d, got_i = retrieval.merge_topk_device(D, I, k)              # the form evaluate_distributed(on_device=True) calls
    assert torch.equal(got_i, out["idx"]) and torch.equal(got_d, out["dist64"])


def test_merge_float32_overflow_equal_pairs_and_too_few_candidates(cuda):
    D = np.array([[[1.0, 1e300, np.inf]], [[1.0, 3.0, np.inf]]])       # part 0 ends in a real +inf, part 1 in padding
    I = np.array([[[4, 5, 9]], [[4, 6, -1]]])                          # (1.0, 4) twice: both stay, part 0's first
    want_d, want_i = retrieval.merge_topk(list(D), list(I), 5)
    out = cabi.topk_merge(_dev(D, cuda), _dev(I, cuda), 5)
    assert out["idx"].cpu().tolist() == [[4, 4, 6, 5, 9]] == want_i.tolist()
    assert out["dist64"].cpu().tolist() == [[1.0, 1.0, 3.0, 1e300, np.inf]] == want_d.tolist()
    assert out["dist"].cpu().tolist() == [[1.0, 1.0, 3.0, np.inf, np.inf]]
    only_idx = cabi.topk_merge(_dev(D, cuda), _dev(I, cuda), 5, want=("idx",))
    assert set(only_idx) == {"idx"} and torch.equal(only_idx["idx"], out["idx"])
    six = cabi.topk_merge(_dev(D, cuda), _dev(I, cuda), 6)              # five real candidates: the sixth place is padding
    assert six["idx"].cpu().tolist() == [[4, 4, 6, 5, 9, -1]] and six["dist64"].cpu().tolist()[0][5] == np.inf
    assert six["dist"].cpu().tolist()[0][5] == np.inf
    with pytest.raises(ValueError, match="fewer than k=6"):
        retrieval.merge_topk_device(D, I, 6)
    with pytest.raises(ValueError, match="fewer than k=7"):            # more than P * k_in: refused before the call
        retrieval.merge_topk_device(D, I, 7)


# ---- 2. csn_topk_class_metrics against the numpy restatement --------------------------------------------------------------
NG = 300
OUTPUTS = (("hits", torch.int32), ("top1", torch.int32), ("pred", torch.int32), ("class", torch.int64),
           ("top1_correct", torch.int64))


def _metrics_case(Nq, k, n_classes):
    g_cls, q_cls = ref.label_set(n_classes, NG, Nq, seed=Nq + k + n_classes)
    I = ref.neighbour_lists(g_cls, q_cls, k, seed=Nq * k)
    I[0, k // 2] = -1                                                 # a miss that must not be dereferenced
    I[Nq - 1, 0] = -1                                                 # ... in the first place: top-1 class -1
    return I, g_cls.astype(np.int32), q_cls.astype(np.int32)


def _guarded_call(cuda, I, g_cls, q_cls, n_classes, skip=()):
    """The raw entry point with every output inside a larger buffer of sentinels; -> {name: (buffer, view)}."""
    Nq = len(q_cls)
    sizes = {"hits": Nq, "top1": Nq, "pred": Nq, "class": n_classes * 4, "top1_correct": 1}
    bufs = {}
    for name, dtype in OUTPUTS:
        buf = torch.full((sizes[name] + 2 * GUARD,), SENTINEL, dtype=dtype, device=cuda)
        bufs[name] = (buf, buf[GUARD:GUARD + sizes[name]])
    idx, gc, qc = _dev(I, cuda), _dev(g_cls, cuda), _dev(q_cls, cuda)
    ptr = lambda name: None if name in skip else cabi._ptr(bufs[name][1])
    cabi._check(cabi.load().csn_topk_class_metrics(cabi._ptr(idx), Nq, I.shape[1], cabi._ptr(gc), len(g_cls), cabi._ptr(qc),
                                                   n_classes, ptr("hits"), ptr("top1"), ptr("pred"), ptr("class"),
                                                   ptr("top1_correct"), cabi._stream()))
    torch.cuda.synchronize()
    return bufs


def _assert_guarded(bufs, want, skip=()):
    for name, (buf, view) in bufs.items():
        assert bool((buf[:GUARD] == SENTINEL).all()) and bool((buf[GUARD + view.numel():] == SENTINEL).all()), name
        if name in skip:
            assert bool((view == SENTINEL).all()), name
        else:
            assert torch.equal(view.cpu(), torch.from_numpy(want[name].reshape(-1))), name


@pytest.mark.parametrize("k", [1, 5, 64, 200])
@pytest.mark.parametrize("Nq", [1, 70, 257])
def test_class_metrics_equal_the_contract(cuda, Nq, k):
    for n_classes in (1, 7, 40, 1000):
        I, g_cls, q_cls = _metrics_case(Nq, k, n_classes)
        want = ref.class_metrics(I, g_cls, q_cls, n_classes)
        assert want["top1"][Nq - 1] == -1 and int(want["class"][:, 0].sum()) == Nq
        _assert_guarded(_guarded_call(cuda, I, g_cls, q_cls, n_classes), want)
        out = cabi.topk_class_metrics(_dev(I, cuda), _dev(g_cls, cuda), _dev(q_cls, cuda), n_classes)
        assert {name: tuple(t.shape) for name, t in out.items()} == \
            {"hits": (Nq,), "top1": (Nq,), "pred": (Nq,), "class": (n_classes, 4), "top1_correct": (1,)}
        for name in want:
            assert torch.equal(out[name].cpu(), torch.from_numpy(want[name])), (name, n_classes)


@pytest.mark.parametrize("skip", [name for name, _ in OUTPUTS])
def test_class_metrics_leave_null_outputs_alone(cuda, skip):
    I, g_cls, q_cls = _metrics_case(70, 5, 7)
    want = ref.class_metrics(I, g_cls, q_cls, 7)
    _assert_guarded(_guarded_call(cuda, I, g_cls, q_cls, 7, skip=(skip,)), want, skip=(skip,))
    names = tuple(name for name, _ in OUTPUTS if name != skip)
    out = cabi.topk_class_metrics(_dev(I, cuda), _dev(g_cls, cuda), _dev(q_cls, cuda), 7, want=names)
    assert set(out) == set(names)


def test_class_metrics_do_not_depend_on_the_order_of_the_queries(cuda):
    """Integer sums and a minimum: a permutation of the queries permutes the per-query outputs and leaves the per-class
    sums alone (the first-query column follows the permutation)."""
    I, g_cls, q_cls = _metrics_case(257, 5, 40)
    perm = np.random.default_rng(3).permutation(257)
    a = cabi.topk_class_metrics(_dev(I, cuda), _dev(g_cls, cuda), _dev(q_cls, cuda), 40)
    b = cabi.topk_class_metrics(_dev(I[perm], cuda), _dev(g_cls, cuda), _dev(q_cls[perm], cuda), 40)
    assert torch.equal(a["class"][:, :3], b["class"][:, :3]) and torch.equal(a["top1_correct"], b["top1_correct"])
    assert torch.equal(a["hits"][torch.from_numpy(perm).to(cuda)], b["hits"])
    assert torch.equal(b["class"][:, 3].cpu(), torch.from_numpy(ref.class_metrics(I[perm], g_cls, q_cls[perm], 40)["class"][:, 3]))


# ---- 3. evaluate_device against evaluate_full, end to end -----------------------------------------------------------------
def _clustered_embeddings(Ng=500, Nq=120, D=32, n_classes=40, seed=7, snr=0.6):
    """Class centres * snr + N(0, 1), the construction of dataset.clustered_eeg on embeddings."""
    rng = np.random.default_rng(seed)
    cents = rng.standard_normal((n_classes, D))
    g_cls, q_cls = rng.integers(0, n_classes, Ng), rng.integers(0, n_classes, Nq)
    gal = (snr * cents[g_cls] + rng.standard_normal((Ng, D))).astype(np.float32)
    qry = (snr * cents[q_cls] + rng.standard_normal((Nq, D))).astype(np.float32)
    return gal, qry, g_cls, q_cls, ref.Dataset(n_classes)


@pytest.fixture(scope="module")
def embeddings():
    return _clustered_embeddings()


@pytest.mark.parametrize("k,tiled", [(5, False), (100, True)])
def test_evaluate_device_equals_evaluate_full(cuda, embeddings, k, tiled):
    gal, qry, g_cls, q_cls, ds = embeddings
    assert retrieval._takes_tiled(len(gal), len(qry), k) == tiled
    glab, qlab = [ref.label(c) for c in g_cls], [ref.label(c) for c in q_cls]
    flags = SimpleNamespace(topK=k)
    want = retrieval.evaluate_full(flags, gal, qry, glab, qlab, ds)
    assert 0.0 < want["Recall_Total"] and want["Precision_Total"] < 100.0          # neither all hits nor none
    g_d, q_d = _dev(gal, cuda), _dev(qry, cuda)
    for gl, ql in ((glab, qlab), (_dev(g_cls, cuda), _dev(q_cls.astype(np.int32), cuda))):
        got = retrieval.evaluate_device(flags, g_d, q_d, gl, ql, ds)
        assert set(got) == set(want) and got["I"].is_cuda and got["D"].is_cuda
        assert (got["Recall_Total"], got["Precision_Total"], got["top1"]) == \
            (want["Recall_Total"], want["Precision_Total"], want["top1"])
        assert got["class_scores"] == want["class_scores"] and list(got["class_scores"]) == list(want["class_scores"])
        assert torch.equal(got["I"].cpu(), torch.from_numpy(want["I"]))
        assert torch.equal(got["D"].cpu(), torch.from_numpy(want["D"]))
    host = retrieval.evaluate_device(flags, gal, list(qry), glab, qlab, ds)        # anything l2_search takes
    assert host["class_scores"] == want["class_scores"] and torch.equal(host["I"].cpu(), torch.from_numpy(want["I"]))


def test_l2_search_device_returns_what_l2_search_returns(cuda, embeddings):
    gal, qry = embeddings[0], embeddings[1]
    for k, dist64 in ((5, False), (100, False), (5, True)):
        want_d, want_i = retrieval.l2_search(gal, qry, k, dist64=dist64)
        got_d, got_i = retrieval.l2_search_device(_dev(gal, cuda), _dev(qry, cuda), k, dist64=dist64)
        assert got_d.is_cuda and torch.equal(got_i.cpu(), torch.from_numpy(want_i))
        assert torch.equal(got_d.cpu(), torch.from_numpy(want_d))


# ---- 4. the stream contract of the two entry points -----------------------------------------------------------------------
@pytest.mark.parametrize("case", [c for v in stream_cases.CASES.values() for c in v], ids=lambda c: c.id)
def test_entry_point_with_late_inputs(cuda, case):
    """The procedure of tests/test_gpu_stream_order.py on the cases of tests/retrieval_metrics_stream_cases.py."""
    stream_tests.test_stateless_entry_point_with_late_inputs(cuda, case)


# ---- 5. host refusals: a status, a message, no launch ---------------------------------------------------------------------
def test_refused_calls_launch_nothing(cuda):
    lib = cabi.load()
    D, I = (_dev(a, cuda) for a in ref.merge_case(2, 3, 4, seed=1))
    outs = [torch.full((3 * 1100,), SENTINEL, dtype=t, device=cuda) for t in (torch.int64, torch.float64, torch.float32)]
    p = cabi._ptr
    for args, text in (((p(D), p(I), 2, 3, 4, 1025, p(outs[0]), p(outs[1]), p(outs[2])), b"at most 1024"),
                       ((p(D), p(I), 2, 3, 4, 9, p(outs[0]), p(outs[1]), p(outs[2])), b"fewer than k"),
                       ((None, p(I), 2, 3, 4, 4, p(outs[0]), p(outs[1]), p(outs[2])), b"null"),
                       ((p(D), None, 2, 3, 4, 4, p(outs[0]), p(outs[1]), p(outs[2])), b"null"),
                       ((p(D), p(I), 2, 3, 4, 4, None, p(outs[1]), p(outs[2])), b"null")):
        assert lib.csn_topk_merge(*args, cabi._stream()) != 0
        assert text in lib.csn_last_error(), lib.csn_last_error()
    idx = _dev(np.zeros((3, 5), dtype=np.int64), cuda)
    cls = _dev(np.zeros(9, dtype=np.int32), cuda)
    mouts = [torch.full((64,), SENTINEL, dtype=t, device=cuda) for t in (torch.int32, torch.int32, torch.int32, torch.int64, torch.int64)]
    mp = [p(t) for t in mouts]
    for args, text in (((None, 3, 5, p(cls), 9, p(cls), 4, *mp), b"null"), ((p(idx), 3, 5, None, 9, p(cls), 4, *mp), b"null"),
                       ((p(idx), 3, 5, p(cls), 9, None, 4, *mp), b"null"), ((p(idx), 3, 1025, p(cls), 9, p(cls), 4, *mp), b"at most 1024"),
                       ((p(idx), 3, 5, p(cls), 9, p(cls), 0, *mp), b"bad shape")):
        assert lib.csn_topk_class_metrics(*args, cabi._stream()) != 0
        assert text in lib.csn_last_error(), lib.csn_last_error()
    torch.cuda.synchronize()
    for t in outs + mouts:
        assert bool((t == SENTINEL).all())
    with pytest.raises(cabi.CsnError, match="at most 1024"):
        cabi.topk_merge(D, I, 1025)
    with pytest.raises(cabi.CsnError, match="dense float64"):
        cabi.topk_merge(D.float(), I, 2)
    with pytest.raises(cabi.CsnError, match="dense int64"):
        cabi.topk_merge(D, I[:, :, :2], 2)
    with pytest.raises(cabi.CsnError, match="dense int32"):
        cabi.topk_class_metrics(idx, cls.long(), cls[:3], 4)


# ---- 6. the evaluation CLI ------------------------------------------------------------------------------------------------
def test_cli_device_eval_writes_the_same_scores(cuda, tmp_path, capsys):
    """LstmDistillFromDinoV2Eval.py with and without --device_eval: the printed line and the score files are the same.
    The .csv is compared byte for byte; the .txt too, after the two fields of its metadata that name the run itself (the
    wall-clock "processing_time", which two runs of ONE form do not share either, and the flag) are taken out."""
    import LstmDistillFromDinoV2Eval as evaluate_cli
    args = ["--synthetic", "32", "--batch_size", "16", "--hidden_size", "128", "--lstm_layers", "1", "--output_size", "16",
            "--dtype", "f32", "--topK", "5", "--log_dir", str(tmp_path)]
    seen = {}
    for tag, extra in (("host", []), ("device", ["--device_eval"])):
        torch.manual_seed(5)                                          # the CLI draws the model's weights: the same ones twice
        r = evaluate_cli.main(args + extra)
        line = [l for l in capsys.readouterr().out.splitlines() if l.startswith("Overall Recall")][-1]
        files = {}
        for suffix in (".txt", "_.csv"):
            with open(os.path.join(str(tmp_path), f"Theperils_sub_1_Scores{suffix}"), "rb") as f:
                files[suffix] = f.read()
            os.remove(os.path.join(str(tmp_path), f"Theperils_sub_1_Scores{suffix}"))
        meta = json.loads(files[".txt"])["metadata"]
        assert meta["flags"]["device_eval"] is (tag == "device")
        files[".txt"] = re.sub(rb'"processing_time": "[0-9.]+s"', b"", files[".txt"], count=1)
        files[".txt"] = re.sub(rb'"device_eval": (true|false)', b"", files[".txt"], count=1)
        seen[tag] = (line, files, torch.as_tensor(r["I"]).cpu())
    assert seen["device"][0] == seen["host"][0]
    assert seen["device"][1]["_.csv"] == seen["host"][1]["_.csv"] and len(seen["host"][1]["_.csv"].splitlines()) > 2
    assert seen["device"][1][".txt"] == seen["host"][1][".txt"]
    assert torch.equal(seen["device"][2], seen["host"][2]) and seen["host"][2].shape[1] == 5
