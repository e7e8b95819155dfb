"""CPU: the XCD-local tile walk of the 256 x 192 body of the input-gradient GEMM inside the backward launches
(beside_xcd_tiles, csrc/gemm_beside.h) and what the build says about the kernel that carries the
body.  The GEMMs are those of the schedule the library builds (bwd_persist_schedule, csrc/lstm_schedule.h) and the walks
those of csn::beside_xcd_tiles itself, both through the host-only program of tests/lstm_schedule_probe.py; the walk and
the choice of the body are modelled in plain Python too, and the models are held to the C++.

The walk: tiles are numbered row panel by row panel; the workers of one XCD take a contiguous range of whole row panels,
proportional to their share of the workers, and deal its tiles round-robin among themselves.  Every tile has to be
visited exactly once whatever the worker counts are -- half-tile launches, launches with XCDs that hold no group, H = 384
with 20 idle workgroups per XCD, chunks of one step, M no multiple of 256 -- and at H = 768 the column tiles of a row
panel must stay on one XCD.  All 36 instantiations of lstm_bwd_persist_kernel carry the body (the width is a run-time
value of the GEMM): none may use scratch, none more than the 512 registers of one wave per SIMD."""
import os
import re

import pytest

import lstm_schedule_probe as sp

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RES =os.path.join(ROOT, "build", "csrc", "lstm_bwd_persist.res")
GRID_SLICES = 32


def xcd_workers(ngroups, nslices):
    """[(xbase, xcount)] of the 8 XCDs: the worker arithmetic of lstm_bwd_persist_kernel.  XCD x < ngroups runs a group on
    nslices of its 32 workgroups and leaves the rest to the GEMM, the other XCDs give all 32."""
    idle = GRID_SLICES - nslices
    out, base = [], 0
    for x in range(8):
        count = idle if x < ngroups else GRID_SLICES
        out.append((base, count))
        base += count
    return out, base


def beside_xcd_tiles(npanels, ntn, xbase, xcount, local, nworkers):
    """Model of csn::beside_xcd_tiles: (first, end, step) of the worker's walk."""
    p0 = npanels * xbase // nworkers
    p1 = npanels * (xbase + xcount) // nworkers
    return p0 * ntn + local, p1 * ntn, xcount


def walk(ngroups, nslices, M, N, tiles=beside_xcd_tiles):
    """{tile: [(xcd, local, round)]} for one GEMM of one launch; tiles: the model, or the C++ function (real_tiles)."""
    assert N % 192 == 0
    npanels, ntn = (M + 255) // 256, N // 192
    xcds, nworkers = xcd_workers(ngroups, nslices)
    assert nworkers > 0
    seen = {}
    for x, (xbase, xcount) in enumerate(xcds):
        for local in range(xcount):
            first, end, step = tiles(npanels, ntn, xbase, xcount, local, nworkers)
            for rnd, lid in enumerate(range(first, end, step)):
                seen.setdefault(lid, []).append((x, local, rnd))
    return seen, npanels, ntn


def takes_wide(ngroups, nslices, M, N):
    """Model of csn::beside_takes_wide: the wide body unless its busiest worker has two or more tiles and 1.3 times its
    rounds exceed the rounds of the 256 x 128 tiles dealt round-robin."""
    if N % 192:
        return False
    seen, npanels, _ = walk(ngroups, nslices, M, N)
    nworkers = xcd_workers(ngroups, nslices)[1]
    wide_rounds = 1 + max(rnd for [(_, _, rnd)] in seen.values())
    narrow_rounds = -(-npanels * ((N + 127) // 128) // nworkers)
    return wide_rounds < 2 or 13 * wide_rounds <= 10 * narrow_rounds


@pytest.fixture(scope="module")
def ask(tmp_path_factory):
    return sp.build(tmp_path_factory.mktemp("beside_wide"))


def launches(ask, B, T, H, L, chunk, lengths=False, no_merge=True):
    """(ngroups, nslices, half, M, N) of every input-gradient GEMM that runs inside a launch, from the schedule the library
    builds (bwd_persist_schedule, csrc/lstm_schedule.h): by default its per-diagonal view, CSN_BWD_NO_MERGE."""
    [real] = ask([sp.bwd_query(T, B, H, L, chunk, lengths=lengths, no_merge=no_merge)])
    return [(len(q["slots"]) * q["MT"], H // 32, bool(q["half"]), (t_hi - t_lo + 1) * B, H)
            for q in real if q["slots"] for _, t_lo, t_hi, _, _ in q["gemms"]]


def real_tiles(ask, gemms):
    """csn::beside_xcd_tiles for every worker of every (ngroups, nslices, M, N) of `gemms`, asked in one process: a
    function that walk() takes in place of the model."""
    args = set()
    for ngroups, nslices, M, N in gemms:
        xcds, nworkers = xcd_workers(ngroups, nslices)
        args |= {((M + 255) // 256, N // 192, xbase, xcount, local, nworkers) for xbase, xcount in xcds for local in range(xcount)}
    args = sorted(args)
    table = dict(zip(args, (tuple(v) for v in ask(["tiles " + " ".join(map(str, a)) for a in args]))))
    return lambda *a: table[a]


# the shapes tests/test_gpu_beside_wide.py runs (B, T, H, L, chunk, lengths), and cfg2
GPU_CASES = [(64, 33, 768, 2, 32, False), (24, 9, 768, 3, 4, False), (130, 33, 384, 2, 32, False), (64, 9, 384, 3, 4, False),
             (24, 4, 768, 3, 32, False), (256, 72, 768, 2, 32, False), (130, 9, 768, 2, 4, True)]
CFG2 = (256, 500, 768, 2, 32, False)
# (ngroups, nslices, M, N) of test_worker_counts_the_host_can_produce
WORKER_COUNTS = [(ngroups, H // 32, npanels * 256 - 255, H) for H in (384, 768) for ngroups in range(1, 9)
                 for npanels in (1, 2, 3, 7, 8, 9, 16, 17, 31, 32, 33, 64, 100, 257)]


def test_the_schedule_mirror_finds_the_launches_of_cfg2(ask):
    found = launches(ask, *CFG2)
    assert len(found) == 16                                   # 18 launches, the first and the last without a GEMM
    assert found[0] == (8, 24, True, 32 * 256, 768)           # launch 1: layer 1 alone, on 32-row groups
    assert found[1] == (8, 24, False, 32 * 256, 768)
    assert found[-1] == (8, 24, True, 20 * 256, 768)          # the last chunk's 20 steps
    assert all(xcd_workers(g, s)[1] == 64 for g, s, *_ in found)
    # 32 row panels: 2 rounds of wide tiles against 3 of narrow ones; the 20 panels of the last chunk: 2 against 2
    assert [takes_wide(g, s, M, N) for g, s, _, M, N in found] == [True] * 15 + [False]


@pytest.mark.parametrize("case", GPU_CASES + [CFG2])
def test_a_merged_launch_holds_the_gemms_of_the_diagonals_it_covers(ask, case):
    """Default schedule against the per-diagonal view: the launches are the same but for one run of diagonals that became
    one launch, whose GEMMs in round r (the host's list moved down r chunks) are those of the r-th diagonal of the run."""
    B, T, H, L, chunk, lengths = case
    merged, apart = ask([sp.bwd_query(T, B, H, L, chunk, lengths=lengths, no_merge=nm) for nm in (False, True)])
    rounds = [r for q in merged for r in sp.bwd_rounds(q, T, chunk)]
    assert rounds == [r for q in apart for r in sp.bwd_rounds(q, T, chunk)], case
    assert all(q["nrounds"] == 1 for q in apart)
    covered = [q["nrounds"] for q in merged if q["nrounds"] > 1]
    nch = -(-T // chunk)
    assert covered == ([nch - 2 * (L - 1)] if not lengths and nch - 2 * (L - 1) >= 2 else []), (case, covered)
    for q in merged:
        if q["nrounds"] > 1:      # one geometry for all its rounds: that of each diagonal's own launch
            same = [a for a in apart if a["slots"] and q["agree"] - q["nrounds"] < a["agree"] <= q["agree"]]
            assert len(same) == q["nrounds"] and all((a["half"], a["MT"], len(a["slots"])) == (q["half"], q["MT"], len(q["slots"])) for a in same)


def test_every_gpu_case_reaches_the_wide_body(ask):
    for case in GPU_CASES:
        found = launches(ask, *case)
        assert (case[3] == 3 and case[1] <= case[4]) or any(takes_wide(g, s, M, N) for g, s, _, M, N in found), case
    # ... the two-round case in its steady-state launch, 8 workers per XCD
    assert (8, 24, False, 8192, 768) in launches(ask, 256, 72, 768, 2, 32) and takes_wide(8, 24, 8192, 768)
    assert not takes_wide(2, 16, 2048, 512)


def test_the_models_are_the_functions_the_kernel_and_its_launcher_call(ask):
    """beside_xcd_tiles and takes_wide above against csn::beside_xcd_tiles and csn::beside_takes_wide (csrc/gemm_beside.h)."""
    tiles = real_tiles(ask, WORKER_COUNTS)
    for ngroups, nslices, M, N in WORKER_COUNTS:
        xcds, nworkers = xcd_workers(ngroups, nslices)
        for xbase, xcount in xcds:
            for local in range(xcount):
                a = ((M + 255) // 256, N // 192, xbase, xcount, local, nworkers)
                assert tiles(*a) == beside_xcd_tiles(*a), a
    gemms = sorted({(g, s, M, N) for case in GPU_CASES + [CFG2] for g, s, _, M, N in launches(ask, *case)})
    assert gemms
    real = ask([f"wide {M} {N} {g} {s} {GRID_SLICES}" for g, s, M, N in gemms] + [f"wide 2048 512 2 16 {GRID_SLICES}"])
    assert real == [int(takes_wide(*g)) for g in gemms] + [0]
    assert {0, 1} <= set(real)


@pytest.mark.parametrize("case", GPU_CASES + [CFG2])
def test_every_tile_is_visited_exactly_once(ask, case):
    found = launches(ask, *case)
    if case[1] <= case[4] and case[3] == 3:
        assert found == []                                    # one chunk, three layers: every GEMM runs stand-alone
    else:
        assert found
    tiles = real_tiles(ask, [(g, s, M, N) for g, s, _, M, N in found])
    for ngroups, nslices, half, M, N in found:
        seen, npanels, ntn = walk(ngroups, nslices, M, N, tiles)
        assert sorted(seen) == list(range(npanels * ntn)), (case, ngroups, M)
        assert all(len(v) == 1 for v in seen.values()), (case, ngroups, M)


def test_worker_counts_the_host_can_produce(ask):
    """Every (groups, slices per group) of a grouped launch at the two widths, against panel counts around the worker counts."""
    tiles = real_tiles(ask, WORKER_COUNTS)
    for H in (384, 768):
        for ngroups in range(1, 9):
            xcds, nworkers = xcd_workers(ngroups, H // 32)
            assert nworkers == ngroups * (32 - H // 32) + (8 - ngroups) * 32
            for npanels in (1, 2, 3, 7, 8, 9, 16, 17, 31, 32, 33, 64, 100, 257):
                assert (ngroups, H // 32, npanels * 256 - 255, H) in WORKER_COUNTS
                seen, _, ntn = walk(ngroups, H // 32, npanels * 256 - 255, H, tiles)
                assert sorted(seen) == list(range(npanels * ntn)) and all(len(v) == 1 for v in seen.values())


def test_a_row_panel_stays_on_one_xcd_at_h768(ask):
    found = launches(ask, *CFG2) + launches(ask, 256, 72, 768, 2, 32) + launches(ask, 130, 33, 768, 2, 32)
    tiles = real_tiles(ask, [(g, s, M, N) for g, s, _, M, N in found] + [(8, 24, 8192, 768)])
    for ngroups, nslices, half, M, N in found:
        seen, npanels, ntn = walk(ngroups, nslices, M, N, tiles)
        assert ntn == 4
        for p in range(npanels):
            assert len({seen[p * ntn + j][0][0] for j in range(ntn)}) == 1, (ngroups, M, p)
    # cfg2's steady state: each XCD takes 4 row panels, two at a time -- the 4 column tiles of panels 2 r and 2 r + 1 of
    # its range in round r
    seen, npanels, ntn = walk(8, 24, 8192, 768, tiles)
    for lid, [(x, local, rnd)] in seen.items():
        assert lid // ntn == 4 * x + 2 * rnd + local // 4 and lid % ntn == local % 4


def _kernels(text, name):
    """{mangled name: {field: int}} of the kernels whose mangled name contains `name`."""
    found = {}
    for block in re.split(r"remark: [^\n]*Function Name: ", text)[1:]:
        mangled = block.split()[0]
        if name in mangled:
            fields = dict(re.findall(r":\s+([A-Za-z][A-Za-z \[\]/]*?): (\d+) \[-Rpass", block))
            found[mangled] = {k.strip(): int(v) for k, v in fields.items()}
    return found


@pytest.mark.skipif(not os.path.exists(RES), reason="no in-tree build: build/csrc/lstm_bwd_persist.res is absent")
def test_no_instantiation_has_scratch_or_more_than_512_registers():
    with open(RES) as f:
        kernels = _kernels(f.read(), "lstm_bwd_persist_kernel")
    assert len(kernels) == 36, sorted(kernels)
    for name, r in kernels.items():
        print(name, r)
        assert r["ScratchSize [bytes/lane]"] == 0, name
        assert r["VGPRs Spill"] == 0 and r["SGPRs Spill"] == 0, name
        assert r["VGPRs"] + r["AGPRs"] <= 512, name
        assert r["Occupancy [waves/SIMD]"] == 1, name
