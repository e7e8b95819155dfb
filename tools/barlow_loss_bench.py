"""What the fused Barlow-Twins loss (csn_barlow_corr + csn_barlow_grad, csrc/barlow_loss.hip) costs or
saves against the torch form it replaces: forward plus backward of the LOSS ALONE, on embeddings that are already there, and
one end-to-end leg (the cfg2 DistillTrainer step with the Barlow loss and LARS, with and without ``fused_loss``).

    python tools/barlow_loss_bench.py          # times every leg, counts launches, writes profiles/barlow_loss_bench.json
    python tools/barlow_loss_bench.py time     # the timings alone, in this process: one JSON line per leg
    python tools/barlow_loss_bench.py trace    # the traced workload (run under rocprofv3 by the driver form)

Legs: the loss at 256 x 384 (the cfg2 / cfg5 batch), 16 x 384 and 2048 x 384; ``step``: DistillTrainer at B 256, C 128,
T 500, H 768, L 2, D 384, loss="barlow", optimizer="lars".  The torch form is what BarlowTwinsLoss runs with ``fused=False``
(the default, and the code path ``bench.py --loss barlow`` takes); both forms see the same inputs.

Timing and launch counts as tools/distill_loss_bench.py: both forms in one process, after a warm-up of both, alternating CALL
BY CALL, every call between two device events; a window is WINDOW_CALLS calls of each form, the result is the median of
WINDOWS windows with the quartiles.  Launches per call come from one ``rocprofv3 --kernel-trace`` run of the ``trace``
workload of its own, in which every counted block of calls sits between two launches of the library's RMSprop kernel (which
nothing here uses).  The driver form starts each part as a child under its own time limit, stops at the first that fails, and
never opens the GPU itself."""
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

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

CHILD_TIMEOUT_S = 300
WINDOWS, WINDOW_CALLS, WARMUP = 20, 50, 30
STEP_WINDOW_CALLS = 10          # the end-to-end leg: a window of 10 steps of each form
TRACE_CALLS = 10
MARK = "rmsprop_flat_kernel"
LEGS = ("barlow_b256_d384", "barlow_b16_d384", "barlow_b2048_d384", "step_b256_c128_t500_h768_l2_d384_barlow_lars")


def _rand(shape, dev, seed):
    return torch.randn(shape, device=dev, generator=torch.Generator(device=dev).manual_seed(seed))


def _leg(name, dev):
    """-> (torch call, fused call): each runs forward + backward of the leg once."""
    from cerebralsignalnetworks_amd import losses as pl
    if name.startswith("barlow"):
        B = int(name.split("_b")[1].split("_")[0])
        z1, z2 = _rand((B, 384), dev, 1).requires_grad_(True), _rand((B, 384), dev, 2)       # the target embedding is frozen
        crit = [pl.BarlowTwinsLoss(384, B, fused=f).to(dev) for f in (False, True)]

        def call(k):
            z1.grad = None
            crit[k](z1, z2).backward()
    else:
        from cerebralsignalnetworks_amd import EEGFilters, Model
        from cerebralsignalnetworks_amd.trainer import DistillTrainer
        B, C, T, H, L, D = 256, 128, 500, 768, 2, 384
        sos = EEGFilters(1000, order=3).sos
        tr = []
        for f in (False, True):
            torch.manual_seed(0)
            m = Model(input_size=C, lstm_size=H, lstm_layers=L, output_size=D, include_top=False).to(dev)
            tr.append(DistillTrainer(m, sos, loss="barlow", lr=0.2, optimizer="lars", fused_loss=f))
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


def _mark(bufs):
    from cerebralsignalnetworks_amd import cabi
    cabi.rmsprop_step(bufs[0], bufs[1], bufs[2], 1e-3)


def trace_workload():
    dev = torch.device("cuda:0")
    bufs = [torch.zeros(64, device=dev) for _ in range(3)]
    for name in LEGS:
        forms = _leg(name, dev)
        for _ in range(3):
            forms[0]()
            forms[1]()
        for form in forms:                          # mark, TRACE_CALLS calls, mark
            torch.cuda.synchronize()
            _mark(bufs)
            for _ in range(TRACE_CALLS):
                form()
            _mark(bufs)
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
        sys.exit(f"barlow_loss_bench: {' '.join(args[:6])} ... ended with status {rc}; nothing further was started")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("what", nargs="?", default="all", choices=["all", "time", "trace", "count"])
    ap.add_argument("arg", nargs="?", default=None)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "barlow_loss_bench.json"))
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
        result = dict(tool="tools/barlow_loss_bench.py", device=device, legs=[table[n] for n in LEGS])
        with open(args.out, "w") as f:
            json.dump(result, f, indent=1)
            f.write("\n")
        print(json.dumps(result))


if __name__ == "__main__":
    main()
