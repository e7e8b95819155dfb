"""The launch schedules the library runs, without a GPU (not a test module): a host-only program that includes
csrc/lstm_schedule.h and csrc/gemm_beside.h, reads one query per line on stdin and answers each with one JSON line.

    bwd T B H L chunk lengths dropout dh_n data_polls no_beside no_merge no_half   -> bwd_persist_schedule: [launch]
    fwd T B H L chunk fwd_ns persist_streams no_half                               -> fwd_persist_form and _schedule
    grouped persist_bwd B L steps chunk persist_streams                            -> bwd_grouped: 0 / 1
    wide M N ngroups nslices grid_slices                                           -> beside_takes_wide: 0 / 1
    tiles npanels ntn xbase xcount local nworkers                                  -> beside_xcd_tiles: [first, end, step]
    wave T L chunk by_chunk lag backward                                           -> wavefront_schedule: [launch]

A wave launch is {"cells": [[layer, chunk, t, nsteps, enters, ends, last]], "closes": 0 / 1, "done": [[layer, chunk, last]]}:
the cells of the launch, whether it closes its diagonal, and (closing launches only) the chunks the diagonal finished.

build(dir) compiles it once (a module-scoped fixture per test module); the function it returns takes a list of query
lines and returns the parsed answers, one process per list."""
import json
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "cerebralsignalnetworks_amd", "csrc")
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")

PROGRAM = r"""
#include <cstdio>
#include <cstring>
#include "gemm_beside.h"
#include "lstm_schedule.h"
using namespace csn;

static void print_bwd(const BwdSchedIn& in) {
  const std::vector<BwdLaunch> s = bwd_persist_schedule(in);
  printf("[");
  for (size_t n = 0; n < s.size(); ++n) {
    const BwdLaunch& q = s[n];
    printf("%s{\"slots\": [", n ? ", " : "");
    for (int i = 0; i < q.nslots; ++i) {
      const BwdSlot& S = q.slot[i];
      printf("%s[%d, %d, %d, %d, %d, %d]", i ? ", " : "", S.layer, S.chunk, S.t_hi, S.nsteps, S.cnt_pub, S.cnt_wait);
    }
    printf("], \"gemms\": [");
    for (int i = 0; i < q.ngemm; ++i) {
      const BwdGemm& g = q.gemm[i];
      printf("%s[%d, %d, %d, %d, %d]", i ? ", " : "", g.layer, g.t_lo, g.t_hi, (int)g.mask, (int)g.add);
    }
    printf("], \"inline_gemms\": %d, \"nrounds\": %d, \"half\": %d, \"MT\": %d, \"agree\": %d, \"wk\": [%d, %d, %d]}",
           (int)q.inline_gemms, q.nrounds, (int)q.half, q.MT, q.agree, q.wk_wait, q.wk_pub, q.wk_stride);
  }
  printf("]\n");
}

static void print_fwd(const FwdSchedIn& in) {
  const std::vector<FwdLaunch> s = fwd_persist_schedule(in);
  const FwdForm f = fwd_persist_form(in);
  printf("{\"form\": \"%s\", \"launches\": [", f == FwdForm::grouped ? "grouped" : f == FwdForm::layer_streams ? "layer_streams" : "caller_stream");
  for (size_t n = 0; n < s.size(); ++n) {
    const FwdLaunch& q = s[n];
    printf("%s{\"slots\": [", n ? ", " : "");
    for (int i = 0; i < q.nslots; ++i) {
      const FwdSlot& S = q.slot[i];
      printf("%s[%d, %d, %d, %d, %d]", i ? ", " : "", S.layer, S.chunk, S.t0, S.nsteps, (int)S.feeds_next);
    }
    printf("], \"half\": %d, \"MT\": %d, \"agree\": %d}", (int)q.half, q.MT, q.agree);
  }
  printf("]}\n");
}

static void print_wave(const WaveIn& in) {
  int n = 0;
  printf("[");
  wavefront_schedule(in, [&](const WaveLaunch& q) {
    printf("%s{\"cells\": [", n++ ? ", " : "");
    for (int i = 0; i < q.ncells; ++i) {
      const WaveCell& c = q.cell[i];
      printf("%s[%d, %d, %d, %d, %d, %d, %d]", i ? ", " : "", c.layer, c.chunk, c.t, c.nsteps, (int)c.enters, (int)c.ends, (int)c.last);
    }
    printf("], \"closes\": %d, \"done\": [", (int)q.closes);
    for (int i = 0; i < q.ndone; ++i) printf("%s[%d, %d, %d]", i ? ", " : "", q.done[i].layer, q.done[i].chunk, (int)q.done[i].last);
    printf("]}");
    return 0;
  });
  printf("]\n");
}

int main() {
  char line[256], what[16];
  int v[12];
  while (fgets(line, sizeof line, stdin)) {
    const int n = sscanf(line, "%15s %d %d %d %d %d %d %d %d %d %d %d %d", what, v, v + 1, v + 2, v + 3, v + 4, v + 5, v + 6, v + 7,
                         v + 8, v + 9, v + 10, v + 11) - 1;
    if (!strcmp(what, "bwd") && n == 12)
      print_bwd(BwdSchedIn{v[0], v[1], v[2], v[3], v[4], v[5] != 0, v[6] != 0, v[7] != 0, v[8] != 0, v[9] != 0, v[10] != 0, v[11] != 0});
    else if (!strcmp(what, "fwd") && n == 8)
      print_fwd(FwdSchedIn{v[0], v[1], v[2], v[3], v[4], v[5] != 0, v[6] != 0, v[7] != 0});
    else if (!strcmp(what, "grouped") && n == 6)
      printf("%d\n", (int)bwd_grouped(v[0] != 0, v[1], v[2], v[3], v[4], v[5] != 0));
    else if (!strcmp(what, "wide") && n == 5)
      printf("%d\n", (int)beside_takes_wide(v[0], v[1], v[2], v[3], v[4]));
    else if (!strcmp(what, "tiles") && n == 6) {
      const BesideWalk w = beside_xcd_tiles(v[0], v[1], v[2], v[3], v[4], v[5]);
      printf("[%u, %u, %u]\n", w.first, w.end, w.step);
    } else if (!strcmp(what, "wave") && n == 6 && v[0] >= 1 && v[1] >= 1 && v[1] <= kWaveMaxLayers && v[2] >= 1 && v[4] >= 1) {
      print_wave(WaveIn{v[0], v[1], v[2], v[3] ? WaveUnit::chunk : WaveUnit::step, v[4], v[5] != 0});
    } else {
      fprintf(stderr, "bad query: %s", line);
      return 1;
    }
  }
  return 0;
}
"""


def build(directory, flags=("-O0",)):
    src, exe = os.path.join(str(directory), "schedule_probe.hip"), os.path.join(str(directory), "schedule_probe")
    with open(src, "w") as f:
        f.write(PROGRAM)
    subprocess.run([HIPCC, "--cuda-host-only", "-std=c++17", *flags, "-I", CSRC, src, "-o", exe], check=True)

    def ask(lines):
        done = subprocess.run([exe], input="".join(line + "\n" for line in lines), check=True, capture_output=True, text=True)
        out = [json.loads(line) for line in done.stdout.splitlines()]
        assert len(out) == len(lines), (len(out), len(lines), done.stderr[-2000:])
        return out
    return ask


def bwd_query(T, B, H, L, chunk, lengths=False, dropout=False, dh_n=False, flags=False, no_beside=False, no_merge=False,
              no_half=False):
    """(a plan's dropout bit with one layer is no dropout: drop_on of lstm.hip)"""
    return "bwd " + " ".join(str(int(v)) for v in (T, B, H, L, chunk, lengths, dropout and L > 1, dh_n, not flags, no_beside,
                                                   no_merge, no_half))


def fwd_query(T, B, H, L, chunk, fwd_ns=False, persist_streams=False, no_half=False):
    return "fwd " + " ".join(str(int(v)) for v in (T, B, H, L, chunk, fwd_ns, persist_streams, no_half))


# the six wavefronts of lstm.hip: (unit is a whole chunk, lag in chunks, backward)
WAVE_VARIANTS = {"forward_v1": (False, 1, False), "backward_v1": (False, 1, True),
                 "forward_resident": (True, 1, False), "backward_resident": (True, 1, True),
                 "forward_il": (False, 2, False), "backward_il": (False, 2, True)}


def wave_query(variant, T, L, chunk):
    by_chunk, lag, backward = WAVE_VARIANTS[variant]
    return "wave " + " ".join(str(int(v)) for v in (T, L, chunk, by_chunk, lag, backward))


def bwd_rounds(launch, T, chunk):
    """[(rec, gemms)] per round of a launch of the real schedule, rec = [(layer, chunk)] top layer first and gemms =
    [(layer, chunk)]: round r of a merged launch is the host's round 0 moved down r chunks, as lstm_bwd_persist_kernel
    moves its slots and GEMMs.  Checks on the way that the steps of every slot and GEMM are those of its chunk."""
    def chunk_of(t_lo, t_hi):
        c, rest = divmod(T - 1 - t_hi, chunk)
        assert rest == 0 and t_hi - t_lo + 1 == min(chunk, T - c * chunk), launch
        return c
    rec = [(layer, c) for layer, c, *_ in launch["slots"]]
    for layer, c, t_hi, nsteps, _, _ in launch["slots"]:
        assert chunk_of(t_hi - nsteps + 1, t_hi) == c, launch
    gemms = [(layer, chunk_of(t_lo, t_hi)) for layer, t_lo, t_hi, _, _ in launch["gemms"]]
    return [([(l, c + r) for l, c in rec], [(l, c + r) for l, c in gemms]) for r in range(launch["nrounds"])]
