"""CPU: the launch schedule of the weight-stationary LSTM backward and its merged launch.

The schedule under test is the one the library runs: bwd_persist_schedule (csrc/lstm_schedule.h), which backward_persist
(csrc/lstm.hip) enqueues entry by entry, printed by a host-only program (tests/lstm_schedule_probe.py) and expanded into
rounds as the round loop of lstm_bwd_persist_kernel (csrc/lstm_bwd_persist.hip) moves a merged launch's slots and GEMMs.
schedule() below is an independent model of it in Python (tests/test_gpu_bwd_merged.py takes its launch counts from it);
the two must agree field by field over the sweep.

The diagonals on which every layer is in range run as ONE launch of as many rounds; the two kernel boundaries around each
input-gradient GEMM become the counters rec_done[layer][chunk] (added to by the recurrence workgroups of a layer when they
leave a chunk, waited for by the GEMM workers) and gemm_done[layer][chunk] (added to by the workers, waited for by the
layer below).  Checked over a sweep of plans: every (layer, chunk) and every GEMM runs exactly once and behind its
producer; the words the two sides of a hand-off index are the same word, nobody else's, and inside the zeroed region; the
value a waiter expects is the number of workgroups that add; and CSN_BWD_NO_MERGE is read into Options."""
import itertools
import os
import subprocess

import pytest

import lstm_schedule_probe as sp

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "cerebralsignalnetworks_amd", "csrc")
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
GRID_SLICES = 32


def schedule(T, L, H, B, chunk, dropout=False, lengths=False, flags=False, no_merge=False, dh_n=False, no_half=False,
             no_beside=False):
    """Model of what backward_persist enqueues, in stream order.  A launch is a dict: rounds = [(rec, gemms)] with rec =
    [(layer, chunk)] top layer first and gemms = [(layer, chunk)] (the input-gradient GEMM of `layer`'s `chunk`, written to
    the layer below), half = 32-row groups, plus the counter indices of a merged launch; a stand-alone GEMM (a diagonal
    without a layer in range, or every GEMM where the launches do not carry them) is a launch with rec = []."""
    nch = -(-T // chunk)
    MT = -(-B // 64)
    nslices = H // 32
    beside = 1 < L <= 4 and nslices <= 28 and not no_beside
    lag = 2 if beside else 1
    first, count = lag * (L - 1), nch - lag * (L - 1)
    merge = beside and not (no_merge or flags or lengths or dropout or dh_n) and count >= 2
    out, pending, dg = [], [], 0
    while dg < nch + lag * (L - 1):
        merged = merge and dg == first
        last = dg + count - 1 if merged else dg
        rec = [(l, last - lag * (L - 1 - l)) for l in range(L - 1, -1, -1) if 0 <= last - lag * (L - 1 - l) < nch]
        if not rec:
            out += [dict(rounds=[([], [g])], half=False, merged=0) for g in pending]
            pending, dg = [], dg + 1
            continue
        half = not no_half and not lengths and 2 * len(rec) * MT <= 8
        launch = dict(half=half, merged=count if merged else 0, groups=len(rec) * (2 * MT if half else MT), nslices=nslices)
        if merged:
            assert len(rec) == L and len(pending) == L - 1
            rounds = []
            for r in range(count):
                back = count - 1 - r
                rounds.append(([(l, c - back) for l, c in rec], pending))
                pending = [(l, c - back) for l, c in rec if l > 0]          # what round r leaves for round r + 1
            launch["rounds"] = rounds
            c0 = {l: c - (count - 1) for l, c in rec}
            launch["cnt_pub"] = {l: (l * nch + c0[l] if l > 0 else -1) for l in c0}
            launch["cnt_wait"] = {l: ((L + l + 1) * nch + c0[l] if l < L - 1 else -1) for l in c0}
            launch["wk"] = (launch["cnt_pub"][L - 1] - 1, launch["cnt_wait"][L - 2] + 1, nch + lag)
            launch["words"] = 2 * L * nch
        else:
            launch["rounds"] = [(rec, pending)]
            pending = [(l, c) for l, c in rec if l > 0] if beside else []
            if not beside:      # lag 1: the GEMM runs between two launches
                out.append(launch)
                out += [dict(rounds=[([], [(l, c)])], half=False, merged=0) for l, c in rec if l > 0]
                dg += 1
                continue
        out.append(launch)
        dg = last + 1
    assert not pending                                     # (the last launch holds layer 0 alone: nothing is left over)
    return out


def nworkers(groups, nslices):
    return groups * (GRID_SLICES - nslices) + (8 - groups) * GRID_SLICES


def as_model(real, T, L, H, chunk):
    """A schedule as the library builds it (the probe's JSON) in the form of schedule(): the rounds of a merged launch
    expanded as the kernel does, its counter indices by layer, and the GEMMs that run between two launches (a diagonal
    without a layer in range; dx_chunk_gemm behind the launch where the launches carry no GEMM) as launches with rec = []."""
    nch = -(-T // chunk)
    alone = lambda g: dict(rounds=[([], [g])], half=False, merged=0)
    out = []
    for q in real:
        rounds = sp.bwd_rounds(q, T, chunk)
        if not q["slots"]:
            assert q["nrounds"] == 1 and not q["inline_gemms"] and q["gemms"], q
            out += [alone(g) for g in rounds[0][1]]
            continue
        merged = q["nrounds"] if q["nrounds"] > 1 else 0
        launch = dict(half=bool(q["half"]), merged=merged, groups=len(q["slots"]) * q["MT"], nslices=H // 32, rounds=rounds)
        if merged:
            launch["cnt_pub"] = {layer: pub for layer, _, _, _, pub, _ in q["slots"]}
            launch["cnt_wait"] = {layer: wait for layer, _, _, _, _, wait in q["slots"]}
            launch["wk"] = tuple(q["wk"])
            launch["words"] = 2 * L * nch                  # rec_done[L][nch], then gemm_done[L][nch]
        else:
            assert all(pub == wait == -1 for *_, pub, wait in q["slots"]), q
        out.append(launch)
        if q["inline_gemms"]:
            assert not q["gemms"], q
            out += [alone(cell) for cell in rounds[0][0] if cell[0] > 0]
    return out


# (chunk 4 throughout; no_beside and no_half cross every feature)
SWEEP = [dict(T=T, L=L, H=H, B=B, chunk=4, **feat, **nb, **nh)
         for L in (1, 2, 3, 4) for H in (128, 384, 768, 1024) for B in (64, 130, 256)
         for T in list(range(4, 49, 4)) + [5, 22, 38, 47]
         for feat in ({}, {"dropout": True}, {"lengths": True}, {"flags": True}, {"no_merge": True}, {"dh_n": True})
         for nb in ({}, {"no_beside": True}) for nh in ({}, {"no_half": True})
         if L * -(-B // 64) <= 8]


def _query(p):
    return sp.bwd_query(**p)


@pytest.fixture(scope="module")
def ask(tmp_path_factory):
    return sp.build(tmp_path_factory.mktemp("bwd_schedule"))


@pytest.fixture(scope="module")
def swept(ask):
    """[(plan, the library's schedule in the probe's form, the same in the model's form)] over SWEEP: one process."""
    raw = ask([_query(p) for p in SWEEP])
    return [(p, q, as_model(q, p["T"], p["L"], p["H"], p["chunk"])) for p, q in zip(SWEEP, raw)]


def test_the_model_is_the_schedule_the_library_runs(swept):
    for p, _, real in swept:
        model = schedule(**p)
        assert len(model) == len(real), (p, len(model), len(real))
        for i, (m, r) in enumerate(zip(model, real)):
            assert set(m) == set(r), (p, i, sorted(m), sorted(r))
            for field in m:      # rounds (cells and GEMMs), half, merged, groups, nslices, cnt_pub, cnt_wait, wk, words
                assert m[field] == r[field], (p, i, field, m[field], r[field])


def test_what_follows_a_gemm_and_the_agreement_words(swept):
    """The dropout mask follows every GEMM of a plan with dropout on, the dh_n term the GEMM of reverse chunk 0 (with lengths:
    every GEMM); every launch has agreement words of its own -- those of the last diagonal it covers -- inside the region."""
    for p, raw, _ in swept:
        T, L, chunk = p["T"], p["L"], p["chunk"]
        for q in raw:
            for layer, t_lo, t_hi, mask, add in q["gemms"]:
                assert mask == int(bool(p.get("dropout")) and L > 1), (p, q)
                assert add == int(bool(p.get("dh_n")) and (t_hi == T - 1 or bool(p.get("lengths")))), (p, q)
        agree = [q["agree"] for q in raw if q["slots"]]
        assert agree == sorted(set(agree)) and all(0 <= a < T + 8 for a in agree), (p, agree)
        lag = 2 if (1 < L <= 4 and p["H"] // 32 <= 28 and not p.get("no_beside")) else 1
        for q in raw:
            if q["slots"]:
                layer, c = q["slots"][0][:2]
                assert q["agree"] == c + lag * (L - 1 - layer) + q["nrounds"] - 1, (p, q)


def test_every_cell_and_gemm_runs_once_behind_its_producer(swept):
    for p, _, launches in swept:
        nch, L = -(-p["T"] // p["chunk"]), p["L"]
        when_rec, when_gemm = {}, {}
        for li, launch in enumerate(launches):
            for ri, (rec, gemms) in enumerate(launch["rounds"]):
                for cell in rec:
                    assert cell not in when_rec, (p, cell)
                    when_rec[cell] = (li, ri)
                for g in gemms:
                    assert g not in when_gemm, (p, g)
                    when_gemm[g] = (li, ri)
        assert set(when_rec) == set(itertools.product(range(L), range(nch))), p
        assert set(when_gemm) == set(itertools.product(range(1, L), range(nch))), p
        for (l, c), when in when_rec.items():
            if c > 0:
                assert when_rec[(l, c - 1)] < when, (p, l, c)              # a layer walks its chunks in order
            if l < L - 1:
                assert when_gemm[(l + 1, c)] < when, (p, l, c)             # its dy is the GEMM of the layer above
        for g, when in when_gemm.items():
            assert when_rec[g] < when, (p, g)                              # the GEMM's operand is that chunk's dgates


def test_merge_decision(swept):
    for p, _, launches in swept:
        merged = [x for x in launches if x["merged"]]
        nch, L, H = -(-p["T"] // p["chunk"]), p["L"], p["H"]
        excluded = any(p.get(k) for k in ("dropout", "lengths", "flags", "no_merge", "dh_n", "no_beside"))
        want = 0 if (excluded or L == 1 or H == 1024 or nch - 2 * (L - 1) < 2) else nch - 2 * (L - 1)
        assert sum(x["merged"] for x in merged) == want and len(merged) == (1 if want else 0), (p, want)
        rec_launches = [x for x in launches if x["rounds"][0][0]]
        lag = 2 if (1 < L <= 4 and H // 32 <= 28 and not p.get("no_beside")) else 1
        occupied = sum(1 for dg in range(nch + lag * (L - 1)) if any(0 <= dg - lag * k < nch for k in range(L)))
        assert len(rec_launches) == occupied - max(0, want - 1), p
        for x in merged:      # the GEMMs of a merged launch all have full chunks: the short one is multiplied a launch later
            assert all(c < nch - 1 for _, gemms in x["rounds"] for _, c in gemms), p


def test_counters(swept):
    for p, _, launches in swept:
        nch, L = -(-p["T"] // p["chunk"]), p["L"]
        for x in launches:
            if not x["merged"]:
                continue
            adds, waits = {}, {}                     # word -> [who adds], [(who waits, value expected)]
            wait0, pub0, stride = x["wk"]
            for r, (rec, gemms) in enumerate(x["rounds"]):
                more = r + 1 < x["merged"]
                for l, c in rec:
                    if more and x["cnt_pub"][l] >= 0:
                        adds.setdefault(x["cnt_pub"][l] + r, []).append(("rec", l, c))
                    if r > 0 and x["cnt_wait"][l] >= 0:
                        waits.setdefault(x["cnt_wait"][l] + r, []).append((("rec", l, c), nworkers(x["groups"], x["nslices"])))
                for i, (l, c) in enumerate(gemms):
                    assert l == L - 1 - i
                    if r > 0:
                        waits.setdefault(wait0 + r - i * stride, []).append((("gemm", l, c), x["groups"] // L * x["nslices"]))
                    if more:
                        adds.setdefault(pub0 + r - i * stride, []).append(("gemm", l, c))
            for word, who in adds.items():
                assert 0 <= word < x["words"] <= 2 * L * p["T"] and len(who) == 1, (p, word, who)
                kind, l, c = who[0]
                assert word == (l * nch + c if kind == "rec" else (L + l) * nch + c), (p, word, who)    # [layer][chunk]
            for word, who in waits.items():
                assert len(who) == 1 and word in adds, (p, word, who)
                (kind, l, c), value = who[0]
                # the GEMM of (l, c) waits for the recurrence of (l, c); layer l at chunk c for the GEMM of (l + 1, c)
                assert adds[word][0] == (("rec", l, c) if kind == "gemm" else ("gemm", l + 1, c)), (p, word, who)
                producers = x["groups"] // L * x["nslices"] if kind == "gemm" else nworkers(x["groups"], x["nslices"])
                assert value == producers > 0, (p, word, who)
            # the top layer never waits, layer 0 never publishes: no cycle top layer -> workers -> layer below
            assert x["cnt_wait"][L - 1] == -1 and x["cnt_pub"][0] == -1


def test_both_tile_heights_are_covered(swept):
    heights = {x["half"] for _, _, launches in swept for x in launches if x["merged"]}
    assert heights == {True, False}


PROGRAM = r"""
#include "lstm_cell_blk.h"
int main() {
  const csn::Options o = csn::options_from_env();
  printf("%d %d %d %zu\n", (int)o.bwd_no_merge, (int)o.bwd_flags, (int)o.no_beside, sizeof(csn::PersistBwdArgs));
  return 0;
}
"""


@pytest.fixture(scope="module")
def probe(tmp_path_factory):
    d = tmp_path_factory.mktemp("bwd_merged")
    src, exe = d / "probe.hip", d / "probe"
    src.write_text(PROGRAM)
    subprocess.run([HIPCC, "--cuda-host-only", "-std=c++17", "-O0", "-I", CSRC, str(src), "-o", str(exe)], check=True)

    def run(env):
        clean = {k: v for k, v in os.environ.items() if not k.startswith("CSN_")}
        return [int(v) for v in subprocess.run([str(exe)], env={**clean, **env}, check=True, capture_output=True,
                                               text=True).stdout.split()]
    return run


def test_switch_is_read_into_options(probe):
    assert probe({})[:3] == [0, 0, 0]
    assert probe({"CSN_BWD_NO_MERGE": "1"})[:3] == [1, 0, 0]
    assert probe({"CSN_BWD_FLAGS": "1", "CSN_NO_BESIDE": "1"})[:3] == [0, 1, 1]       # the neighbours do not set it
    assert probe({})[3] <= 4096                                                       # the kernel-argument segment
