"""What the fused distillation losses (csn_distill_loss / csn_dino_loss, csrc/distill_loss.hip) save
over the torch forms they replace: forward plus backward of the LOSS ALONE, on features that are already there, and one
end-to-end leg (the DistillTrainer step at the reference's own shapes with and without ``fused_loss``).

    python tools/distill_loss_bench.py          # times every leg, counts launches, writes profiles/distill_loss_bench.json
    python tools/distill_loss_bench.py time     # the timings alone, in this process: one JSON line per leg
    python tools/distill_loss_bench.py trace    # the traced workload (run under rocprofv3 by the driver form)

Legs: featdist at 256 x 384 and 16 x 384 (K 40); the KD alias at 256 x 384; DINO at V 6, G 2, D 384 with B 8 and B 64;
``step``: DistillTrainer at B 16, C 96, T 460, H 96, L 2, featdist, RMSprop.  The torch form is what the classes run with
``fused=False`` (the default); both forms see the same inputs.

Timing: both forms in one process, after a warm-up of both, alternating CALL BY CALL; every call sits between two device
events, a window is WINDOW_CALLS calls of each form, a window's figure is the sum of its calls' times / WINDOW_CALLS, and
the result is the median of WINDOWS windows with the quartiles.  Launches per call: one ``rocprofv3 --kernel-trace`` run
of the ``trace`` workload, in which every counted block of calls sits between two launches of the library's Barlow
reduction kernel (which no loss here uses); the kernels between two such marks are counted.  The driver form starts each
part as a child under its own time limit, stops at the first that fails, and never opens the GPU itself."""
import argparse
import csv
import glob
import json
import os
import subprocess
import sys
import tempfile
import types

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

CHILD_TIMEOUT_S = 300
WINDOWS, WINDOW_CALLS, WARMUP = 20, 50, 30
STEP_WINDOW_CALLS = 10          # the end-to-end leg: a window of 10 steps of each form
TRACE_CALLS = 10
MARK = "barlow_kernel"
LEGS = ("featdist_b256_d384_k40", "featdist_b16_d384_k40", "kd_alias_b256_d384", "dino_v6_g2_b8_d384", "dino_v6_g2_b64_d384",
        "step_b16_c96_t460_h96_l2_featdist_rmsprop")


def _rand(shape, dev, seed):
    return torch.randn(shape, device=dev, generator=torch.Generator(device=dev).manual_seed(seed))


def _leg(name, dev):
    """-> (torch call, fused call): each runs forward + backward of the leg once."""
    from cerebralsignalnetworks_amd import losses as pl
    from cerebralsignalnetworks_amd.dino import DINOLoss
    hp = pl.HyperParams
    if name.startswith("featdist"):
        B = int(name.split("_b")[1].split("_")[0])
        s, c = _rand((B, 384), dev, 1).requires_grad_(True), _rand((B, 40), dev, 2).requires_grad_(True)
        t, lab = _rand((B, 384), dev, 3), torch.randint(0, 40, (B,), device=dev)
        args = (100, hp.warmup_teacher_temp, hp.teacher_temp, hp.warmup_teacher_temp_epochs)
        crit = [pl.FeatureDistributionLoss(*args, fused=f) for f in (False, True)]

        def call(k):
            s.grad = c.grad = None
            crit[k](s, t, 60, lab, pred_label=c).backward()
    elif name.startswith("kd"):
        s, t = _rand((256, 384), dev, 1).requires_grad_(True), _rand((256, 384), dev, 3)
        lab = torch.randint(0, 384, (256,), device=dev)
        kd = types.SimpleNamespace(alpha=0.5, temperature=4.0)

        def call(k):
            s.grad = None
            pl.loss_fn_kd(s, lab, t, kd, fused=bool(k)).backward()
    elif name.startswith("dino"):
        B = int(name.split("_b")[1].split("_")[0])
        s, t = _rand((6, B, 384), dev, 1).requires_grad_(True), _rand((2, B, 384), dev, 3)
        crit = [DINOLoss(384, 6, 0.04, 0.07, 3, 10, fused=f).to(dev) for f in (False, True)]

        def call(k):
            s.grad = None
            crit[k](s, t, 5).backward()
    else:
        from cerebralsignalnetworks_amd import EEGFilters, Model
        from cerebralsignalnetworks_amd.trainer import DistillTrainer
        B, C, T, H, L = 16, 96, 460, 96, 2
        sos = EEGFilters(1000, order=3).sos
        tr = []
        for f in (False, True):
            torch.manual_seed(0)
            m = Model(input_size=C, lstm_size=H, lstm_layers=L, output_size=384, include_top=True).to(dev)
            tr.append(DistillTrainer(m, sos, loss="featdist", lr=1e-3, optimizer="rmsprop", nepochs=100, fused_loss=f))
        x, tgt, lab = _rand((B, C, T), dev, 1), _rand((B, 384), dev, 3), torch.randint(0, 40, (B,), device=dev)

        def call(k):
            tr[k].train_step(x, tgt, lab, epoch=60)
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


def trace_workload():
    from cerebralsignalnetworks_amd import cabi
    dev = torch.device("cuda:0")
    c = torch.eye(4, device=dev)
    for name in LEGS:
        forms = _leg(name, dev)
        for _ in range(3):
            forms[0]()
            forms[1]()
        for form in forms:                          # mark, TRACE_CALLS calls, mark
            torch.cuda.synchronize()
            cabi.barlow_offdiag_sqsum(c)
            for _ in range(TRACE_CALLS):
                form()
            cabi.barlow_offdiag_sqsum(c)
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
            if form == "fused" and not name.startswith("step"):
                out[name]["fused_kernels"] = [_short(n) for n in names[:len(names) // TRACE_CALLS]]
    return out


def _child(args, stdout=None):
    rc = subprocess.run(["timeout", "-k", "10", str(CHILD_TIMEOUT_S), *args], stdout=stdout).returncode
    if rc != 0:
        sys.exit(f"distill_loss_bench: {' '.join(args[:6])} ... ended with status {rc}; nothing further was started")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("what", nargs="?", default="all", choices=["all", "time", "trace", "count"])
    ap.add_argument("arg", nargs="?", default=None)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "distill_loss_bench.json"))
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
        result = dict(tool="tools/distill_loss_bench.py", device=device, legs=[table[n] for n in LEGS])
        with open(args.out, "w") as f:
            json.dump(result, f, indent=1)
            f.write("\n")
        print(json.dumps(result))


if __name__ == "__main__":
    main()
