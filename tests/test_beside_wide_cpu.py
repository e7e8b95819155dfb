"""CPU: the XCD-local tile walk of the 256 x 192 body of the input-gradient GEMM inside the backward launches
(beside_xcd_tiles, csrc/gemm_beside.h), mirrored in plain Python, and what the build says about the
kernel that carries the body.

The walk: tiles are numbered row panel by row panel; the workers of one XCD take a contiguous range of whole row panels,
proportional to their share of the workers, and deal its tiles round-robin among themselves.  Every tile has to be
visited exactly once whatever the worker counts are -- half-tile launches, launches with XCDs that hold no group, H = 384
with 20 idle workgroups per XCD, chunks of one step, M no multiple of 256 -- and at H = 768 the column tiles of a row
panel must stay on one XCD.  All 36 instantiations of lstm_bwd_persist_kernel carry the body (the width is a run-time
value of the GEMM): none may use scratch, none more than the 512 registers of one wave per SIMD."""
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RES = os.path.join(ROOT, "build", "csrc", "lstm_bwd_persist.res")
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
    """Mirror of csn::beside_xcd_tiles: (first, end, step) of the worker's walk."""
    p0 = npanels * xbase // nworkers
    p1 = npanels * (xbase + xcount) // nworkers
    return p0 * ntn + local, p1 * ntn, xcount


def walk(ngroups, nslices, M, N):
    """{tile: [(xcd, local, round)]} for one GEMM of one launch."""
    assert N % 192 == 0
    npanels, ntn = (M + 255) // 256, N // 192
    xcds, nworkers = xcd_workers(ngroups, nslices)
    assert nworkers > 0
    seen = {}
    for x, (xbase, xcount) in enumerate(xcds):
        for local in range(xcount):
            first, end, step = beside_xcd_tiles(npanels, ntn, xbase, xcount, local, nworkers)
            for rnd, lid in enumerate(range(first, end, step)):
                seen.setdefault(lid, []).append((x, local, rnd))
    return seen, npanels, ntn


def takes_wide(ngroups, nslices, M, N):
    """Mirror of csn::beside_takes_wide: the wide body unless its busiest worker has two or more tiles and 1.3 times its
    rounds exceed the rounds of the 256 x 128 tiles dealt round-robin."""
    if N % 192:
        return False
    seen, npanels, _ = walk(ngroups, nslices, M, N)
    nworkers = xcd_workers(ngroups, nslices)[1]
    wide_rounds = 1 + max(rnd for [(_, _, rnd)] in seen.values())
    narrow_rounds = -(-npanels * ((N + 127) // 128) // nworkers)
    return wide_rounds < 2 or 13 * wide_rounds <= 10 * narrow_rounds


def launches(B, T, H, L, chunk, lengths=False):
    """(ngroups, nslices, half, M, N) of every input-gradient GEMM that runs inside a launch of backward_persist (lstm.hip):
    diagonal dg holds layer l at reverse chunk dg - 2 (L - 1 - l); the chunks layer l > 0 finished in one launch are the
    GEMMs of the next one, if that one has a layer in range."""
    MT = (B + 63) // 64
    nch = (T + chunk - 1) // chunk
    steps = [min(chunk, T - c * chunk) for c in range(nch)]
    found, pending = [], []
    for dg in range(nch + 2 * (L - 1)):
        layers = [(l, dg - 2 * (L - 1 - l)) for l in range(L) if 0 <= dg - 2 * (L - 1 - l) < nch]
        if layers:
            half = not lengths and 2 * len(layers) * MT <= 8
            ngroups = len(layers) * MT * (2 if half else 1)
            for M in pending:
                found.append((ngroups, H // 32, half, M, H))
        pending = [steps[c] * B for l, c in layers if l > 0] if layers else []
    return found


# the shapes tests/test_gpu_beside_wide.py runs (B, T, H, L, chunk, lengths), and cfg2
GPU_CASES = [(64, 33, 768, 2, 32, False), (24, 9, 768, 3, 4, False), (130, 33, 384, 2, 32, False), (64, 9, 384, 3, 4, False),
             (24, 4, 768, 3, 32, False), (256, 72, 768, 2, 32, False), (130, 9, 768, 2, 4, True)]
CFG2 = (256, 500, 768, 2, 32, False)


def test_the_schedule_mirror_finds_the_launches_of_cfg2():
    found = launches(*CFG2)
    assert len(found) == 16                                   # 18 launches, the first and the last without a GEMM
    assert found[0] == (8, 24, True, 32 * 256, 768)           # launch 1: layer 1 alone, on 32-row groups
    assert found[1] == (8, 24, False, 32 * 256, 768)
    assert found[-1] == (8, 24, True, 20 * 256, 768)          # the last chunk's 20 steps
    assert all(xcd_workers(g, s)[1] == 64 for g, s, *_ in found)
    # 32 row panels: 2 rounds of wide tiles against 3 of narrow ones; the 20 panels of the last chunk: 2 against 2
    assert [takes_wide(g, s, M, N) for g, s, _, M, N in found] == [True] * 15 + [False]


def test_every_gpu_case_reaches_the_wide_body():
    for case in GPU_CASES:
        found = launches(*case)
        assert (case[3] == 3 and case[1] <= case[4]) or any(takes_wide(g, s, M, N) for g, s, _, M, N in found), case
    # ... the two-round case in its steady-state launch, 8 workers per XCD
    assert (8, 24, False, 8192, 768) in launches(256, 72, 768, 2, 32) and takes_wide(8, 24, 8192, 768)
    assert not takes_wide(2, 16, 2048, 512)


@pytest.mark.parametrize("case", GPU_CASES + [CFG2])
def test_every_tile_is_visited_exactly_once(case):
    found = launches(*case)
    if case[1] <= case[4] and case[3] == 3:
        assert found == []                                    # one chunk, three layers: every GEMM runs stand-alone
    else:
        assert found
    for ngroups, nslices, half, M, N in found:
        seen, npanels, ntn = walk(ngroups, nslices, M, N)
        assert sorted(seen) == list(range(npanels * ntn)), (case, ngroups, M)
        assert all(len(v) == 1 for v in seen.values()), (case, ngroups, M)


def test_worker_counts_the_host_can_produce():
    """Every (groups, slices per group) of a grouped launch at the two widths, against panel counts around the worker counts."""
    for H in (384, 768):
        for ngroups in range(1, 9):
            xcds, nworkers = xcd_workers(ngroups, H // 32)
            assert nworkers == ngroups * (32 - H // 32) + (8 - ngroups) * 32
            for npanels in (1, 2, 3, 7, 8, 9, 16, 17, 31, 32, 33, 64, 100, 257):
                seen, _, ntn = walk(ngroups, H // 32, npanels * 256 - 255, H)
                assert sorted(seen) == list(range(npanels * ntn)) and all(len(v) == 1 for v in seen.values())


def test_a_row_panel_stays_on_one_xcd_at_h768():
    for ngroups, nslices, half, M, N in launches(*CFG2) + launches(256, 72, 768, 2, 32) + launches(130, 33, 768, 2, 32):
        seen, npanels, ntn = walk(ngroups, nslices, M, N)
        assert ntn == 4
        for p in range(npanels):
            assert len({seen[p * ntn + j][0][0] for j in range(ntn)}) == 1, (ngroups, M, p)
    # cfg2's steady state: each XCD takes 4 row panels, two at a time -- the 4 column tiles of panels 2 r and 2 r + 1 of
    # its range in round r
    seen, npanels, ntn = walk(8, 24, 8192, 768)
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
