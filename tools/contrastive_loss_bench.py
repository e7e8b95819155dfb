"""What the fused contrastive loss (csn_contrastive_lse + csn_contrastive_grad, csrc/contrastive_loss.hip)
costs or saves against the plain torch expression a user writes without it: forward plus backward of the LOSS ALONE, on
embeddings that are already there, and two end-to-end legs (a DistillTrainer step with loss="contrastive", with and without
``fused_loss``).

    python tools/contrastive_loss_bench.py          # times every leg, counts launches, writes profiles/contrastive_loss_bench.json
    python tools/contrastive_loss_bench.py time     # the timings alone, in this process: one JSON line per leg
    python tools/contrastive_loss_bench.py trace    # the traced workload (run under rocprofv3 by the driver form)

Legs.  ``contrastive_b256_d384`` / ``_b16_d384``: one rank.  The baseline is the plain expression -- F.normalize twice, one
matmul, two cross_entropy, autograd -- which needs nothing of this library; the fused form is ContrastiveLoss(fused=True).
``contrastive_b256_n2048_d384``: 256 local rows (row0 768) against 2048 gathered keys, no communication in either form: the
baseline is the same expression on the local rows' two [256, 2048] logit blocks, the fused form the two entry points with lB
of all rows at hand.  ``step_*``: DistillTrainer(loss="contrastive") with RMSprop at B 16, C 96, T 460, H 96, L 2 and at cfg2
(B 256, C 128, T 500, H 768, L 2), D 384; there the baseline is the torch form of ContrastiveLoss, the only other form the
trainer has.  No group ids anywhere: the plain expression has none.

Timing and launch counts as tools/distill_loss_bench.py: both forms in one process, after a warm-up of both, alternating CALL
BY CALL, every call between two device events; a window is WINDOW_CALLS calls of each form, the result is the median of
WINDOWS windows with the quartiles.  Launches per call come from one ``rocprofv3 --kernel-trace`` run of the ``trace``
workload of its own, in which every counted block of calls sits between two launches of the library's off-diagonal reduction
(which nothing here uses).  The driver form starts each part as a child under its own time limit, stops at the first that
fails, and never opens the GPU itself."""
import argparse
import csv
import glob
import json
import os
import subprocess
import sys
import tempfile

import numpy as np
import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

CHILD_TIMEOUT_S = 300
WINDOWS, WINDOW_CALLS, WARMUP = 20, 50, 30
STEP_WINDOW_CALLS = 10          # the end-to-end legs: a window of 10 steps of each form
TRACE_CALLS = 10
MARK = "barlow_kernel"
SCALE = 1.0 / 0.07
LEGS = ("contrastive_b256_d384", "contrastive_b16_d384", "contrastive_b256_n2048_d384",
        "step_b16_c96_t460_h96_l2_d384_contrastive", "step_b256_c128_t500_h768_l2_d384_contrastive")


def _rand(shape, dev, seed):
    return torch.randn(shape, device=dev, generator=torch.Generator(device=dev).manual_seed(seed))


def _plain(s, t, s_keys, t_keys, target):
    """The plain expression: queries s against keys t_keys and queries t against keys s_keys."""
    sh, th = F.normalize(s, dim=1), F.normalize(t, dim=1)
    return 0.5 * (F.cross_entropy(SCALE * sh @ F.normalize(t_keys, dim=1).T, target)
                  + F.cross_entropy(SCALE * th @ F.normalize(s_keys, dim=1).T, target))


def _leg(name, dev):
    """-> (baseline call, fused call): each runs forward + backward of the leg once."""
    from cerebralsignalnetworks_amd import cabi, losses as pl
    if name.startswith("contrastive") and "_n" not in name:
        B = int(name.split("_b")[1].split("_")[0])
        s, t = _rand((B, 384), dev, 1).requires_grad_(True), _rand((B, 384), dev, 2)        # the teacher embedding is frozen
        target = torch.arange(B, device=dev)
        crit = pl.ContrastiveLoss(fused=True)

        def call(k):
            s.grad = None
            if k == 0:
                sh, th = F.normalize(s, dim=1), F.normalize(t, dim=1)
                z = SCALE * sh @ th.T
                (0.5 * (F.cross_entropy(z, target) + F.cross_entropy(z.T, target))).backward()
            else:
                crit(s, t).backward()
    elif name.startswith("contrastive"):
        B, N, row0 = 256, 2048, 768
        s_all, t_all = _rand((N, 384), dev, 1), _rand((N, 384), dev, 2)
        s = s_all[row0:row0 + B].clone().requires_grad_(True)
        target = torch.arange(row0, row0 + B, device=dev)
        lse_b_all = cabi.contrastive_lse(s_all, t_all, SCALE)[0][1].clone()       # what the all-gather hands over

        def call(k):
            s.grad = None
            if k == 0:
                s_keys = torch.cat([s_all[:row0], s, s_all[row0 + B:]])
                _plain(s, t_all[row0:row0 + B], s_keys, t_all, target).backward()
            else:
                rows, _ = cabi.contrastive_lse(s_all, t_all, SCALE, None, row0, B)
                cabi.contrastive_grad(s_all, t_all, SCALE, rows[0], lse_b_all, None, row0, B)
    else:
        from cerebralsignalnetworks_amd import EEGFilters, Model
        from cerebralsignalnetworks_amd.trainer import DistillTrainer
        B, C, T, H, L, D = (16, 96, 460, 96, 2, 384) if "_b16_" in name else (256, 128, 500, 768, 2, 384)
        sos = EEGFilters(1000, order=3).sos
        tr = []
        for f in (False, True):
            torch.manual_seed(0)
            m = Model(input_size=C, lstm_size=H, lstm_layers=L, output_size=D, include_top=False).to(dev)
            tr.append(DistillTrainer(m, sos, loss="contrastive", fused_loss=f))
        x, tgt = _rand((B, C, T), dev, 1), _rand((B, D), dev, 3)

        def call(k):
            tr[k].train_step(x, tgt)
    return (lambda: call(0)), (lambda: call(1))


def _window(forms, calls):
    """`calls` calls of each form, alternating call by call, each between two events -> ms per call of each form."""
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(2 * calls + 1)]
    ev[0].record()
    for i in range(calls):
        forms[0]()
        ev[2 * i + 1].record()
        forms[1]()
        ev[2 * i + 2].record()
    ev[-1].synchronize()
    return [sum(ev[2 * i + k].elapsed_time(ev[2 * i + k + 1]) for i in range(calls)) / calls for k in (0, 1)]


def _stats(v):
    q1, med, q3 = (float(x) for x in np.percentile(v, [25, 50, 75]))
    return dict(median_ms=med, q1_ms=q1, q3_ms=q3)


def time_legs():
    dev = torch.device("cuda:0")
    print(json.dumps(dict(leg="device", device=torch.cuda.get_device_name(0))), flush=True)
    for name in LEGS:
        forms = _leg(name, dev)
        calls = STEP_WINDOW_CALLS if name.startswith("step") else WINDOW_CALLS
        for _ in range(WARMUP if calls == WINDOW_CALLS else 5):
            forms[0]()
            forms[1]()
        torch.cuda.synchronize()
        w = np.array([_window(forms, calls) for _ in range(WINDOWS)])
        res = dict(leg=name, windows=WINDOWS, calls_per_window=calls, torch=_stats(w[:, 0]), fused=_stats(w[:, 1]))
        res["torch_over_fused"] = res["torch"]["median_ms"] / res["fused"]["median_ms"]
        print(json.dumps(res), flush=True)
        torch.cuda.empty_cache()


def _mark(c):
    from cerebralsignalnetworks_amd import cabi
    cabi.barlow_offdiag_sqsum(c)


def trace_workload():
    dev = torch.device("cuda:0")
    c = torch.zeros((8, 8), device=dev)
    for name in LEGS:
        forms = _leg(name, dev)
        for _ in range(3):
            forms[0]()
            forms[1]()
        for form in forms:                          # mark, TRACE_CALLS calls, mark
            torch.cuda.synchronize()
            _mark(c)
            for _ in range(TRACE_CALLS):
                form()
            _mark(c)
        torch.cuda.synchronize()


def _short(name):
    words = name.replace("(anonymous namespace)::", "").split("(")[0].split("<")[0].split("::")[-1].split()
    return words[-1] if words else name


def count_launches(trace_csv):
    rows = list(csv.DictReader(open(trace_csv)))
    rows.sort(key=lambda r: int(r["Start_Timestamp"]))
    marks = [i for i, r in enumerate(rows) if MARK in r["Kernel_Name"]]
    assert len(marks) == 4 * len(LEGS), (len(marks), "marks in the trace")
    out = {}
    for k, name in enumerate(LEGS):
        for j, form in enumerate(("torch", "fused")):
            lo, hi = marks[4 * k + 2 * j], marks[4 * k + 2 * j + 1]
            names = [rows[i]["Kernel_Name"] for i in range(lo + 1, hi)]
            per = len(names) / TRACE_CALLS
            out.setdefault(name, {})[f"{form}_launches_per_call"] = int(per) if per == int(per) else per
            if not name.startswith("step"):
                out[name][f"{form}_kernels"] = [_short(n) for n in names[:len(names) // TRACE_CALLS]]
    return out


def _child(args, stdout=None):
    rc = subprocess.run(["timeout", "-k", "10", str(CHILD_TIMEOUT_S), *args], stdout=stdout).returncode
    if rc != 0:
        sys.exit(f"contrastive_loss_bench: {' '.join(args[:6])} ... ended with status {rc}; nothing further was started")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("what", nargs="?", default="all", choices=["all", "time", "trace", "count"])
    ap.add_argument("arg", nargs="?", default=None)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "contrastive_loss_bench.json"))
    args = ap.parse_args()
    me = os.path.abspath(__file__)
    if args.what == "time":
        time_legs()
    elif args.what == "trace":
        trace_workload()
    elif args.what == "count":
        print(json.dumps(count_launches(args.arg)))
    else:
        with tempfile.TemporaryDirectory() as tmp:
            lines = os.path.join(tmp, "time.jsonl")
            with open(lines, "w") as f:
                _child([sys.executable, me, "time"], stdout=f)
            table = {r["leg"]: r for r in map(json.loads, open(lines))}
            _child(["rocprofv3", "--kernel-trace", "--output-format", "csv", "-d", os.path.join(tmp, "trace"), "--",
                    sys.executable, me, "trace"], stdout=subprocess.DEVNULL)
            traces = glob.glob(os.path.join(tmp, "trace", "**", "*kernel_trace.csv"), recursive=True)
            assert traces, "rocprofv3 wrote no kernel trace"
            for name, counts in count_launches(traces[0]).items():
                table[name].update(counts)
        device = table.pop("device")["device"]
        result = dict(tool="tools/contrastive_loss_bench.py", device=device, legs=[table[n] for n in LEGS])
        with open(args.out, "w") as f:
            json.dump(result, f, indent=1)
            f.write("\n")
        print(json.dumps(result))


if __name__ == "__main__":
    main()
