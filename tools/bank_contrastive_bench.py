"""What the fused teacher-bank contrastive loss (csn_bank_contrastive, csrc/bank_contrastive_loss.hip)
costs or saves against the torch form of the same module: forward plus backward of the LOSS ALONE on embeddings that are
already there, the two design measurements of section 27, and one end-to-end leg.

    python tools/bank_contrastive_bench.py          # times every leg, counts launches, writes profiles/bank_contrastive_bench.json
    python tools/bank_contrastive_bench.py time     # the timings alone, in this process: one JSON line per leg
    python tools/bank_contrastive_bench.py trace    # the traced workload (run under rocprofv3 by the driver form)

Legs, all at D 384 and temperature 0.07, no group ids.
``bank_b<B>_m<M>``: BankContrastiveLoss, torch form against ``fused=True``, at (B, M) = (16, 2000), (256, 2000), (256, 16384),
(256, 65536).
``tile_b<B>_m2000``: the fused call with the 64 x 64 logit tiles against the 16 x 16 ones (CSN_BANK_TILE), the question of
section 27.2.  ``value_b256_m65536``: the fused call without a gradient (ds NULL: norms, logits, row sums) against the call
with one; the difference is the weight block's second life -- written by the row kernel, read by the ds contraction -- and
what a recomputation of the logits would have to beat (section 27.1).
``step_b16_c96_t460_h96_l2_d384``: a DistillTrainer step with RMSprop, loss="contrastive" (15 negatives) against
loss="contrastive_bank" with a bank of 2000 rows, both with ``fused_loss``.

Timing and launch counts as tools/contrastive_loss_bench.py: both forms in one process, after a
warm-up of both, alternating CALL BY CALL, every call between two device events; a window is WINDOW_CALLS calls of each
form, the result is the median of WINDOWS windows with the quartiles.  Launches per call come from one
``rocprofv3 --kernel-trace`` run of the ``trace`` workload of its own, in which every counted block of calls sits between two
launches of the library's off-diagonal reduction (which nothing here uses).  The driver form starts each part as a child
under its own time limit, stops at the first that fails, and never opens the GPU itself."""
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
BIG_WINDOW_CALLS = 10           # the legs at M 65536 and the end-to-end leg: a window of 10 calls of each form
TRACE_CALLS = 10
MARK = "barlow_kernel"
D = 384
LEGS = {                        # name -> the two forms timed against each other
    "bank_b16_m2000": ("torch", "fused"), "bank_b256_m2000": ("torch", "fused"), "bank_b256_m16384": ("torch", "fused"),
    "bank_b256_m65536": ("torch", "fused"),
    "tile_b16_m2000": ("tile64", "tile16"), "tile_b256_m2000": ("tile64", "tile16"),
    "value_b256_m65536": ("value_only", "with_gradient"),
    "step_b16_c96_t460_h96_l2_d384": ("contrastive", "contrastive_bank"),
}


def _rand(shape, dev, seed):
    return torch.randn(shape, device=dev, generator=torch.Generator(device=dev).manual_seed(seed))


def _shape(name):
    return int(name.split("_b")[1].split("_")[0]), int(name.split("_m")[1].split("_")[0])


def _leg(name, dev):
    """-> (first form, second form): each runs the leg once."""
    from cerebralsignalnetworks_amd import cabi, losses as pl
    if name.startswith("step"):
        from cerebralsignalnetworks_amd import EEGFilters, Model
        from cerebralsignalnetworks_amd.trainer import DistillTrainer
        B, C, T, H, L, M = 16, 96, 460, 96, 2, 2000
        sos = EEGFilters(1000, order=3).sos
        tr = []
        for loss in ("contrastive", "contrastive_bank"):
            torch.manual_seed(0)
            m = Model(input_size=C, lstm_size=H, lstm_layers=L, output_size=D, include_top=False).to(dev)
            tr.append(DistillTrainer(m, sos, loss=loss, fused_loss=True))
        bank = _rand((M, D), dev, 2)
        tr[1].set_bank(bank)
        pos = torch.randint(0, M, (B,), device=dev, generator=torch.Generator(device=dev).manual_seed(4)).int()
        x, tgt = _rand((B, C, T), dev, 1), bank[pos.long()]
        return (lambda: tr[0].train_step(x, tgt)), (lambda: tr[1].train_step(x, tgt, positives=pos))
    B, M = _shape(name)
    bank = _rand((M, D), dev, 2)
    pos = torch.randint(0, M, (B,), device=dev, generator=torch.Generator(device=dev).manual_seed(4)).int()
    s = (0.5 * bank[pos.long()] + _rand((B, D), dev, 1)).requires_grad_(True)
    if name.startswith("bank"):
        crits = [pl.BankContrastiveLoss(fused=f) for f in (False, True)]
        for c in crits:
            c.set_bank(bank)

        def call(k):
            s.grad = None
            crits[k](s, pos).backward()
        return (lambda: call(0)), (lambda: call(1))
    inv = cabi.bank_norms(bank)
    sd = s.detach()
    if name.startswith("tile"):
        def call(k):
            os.environ["CSN_BANK_TILE"] = ("64", "16")[k]
            cabi.bank_contrastive(sd, bank, inv, pos, 1.0 / 0.07)
            del os.environ["CSN_BANK_TILE"]
        return (lambda: call(0)), (lambda: call(1))
    return (lambda: cabi.bank_contrastive(sd, bank, inv, pos, 1.0 / 0.07, want_grad=False)), \
        (lambda: cabi.bank_contrastive(sd, bank, inv, pos, 1.0 / 0.07))


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


def _calls(name):
    return BIG_WINDOW_CALLS if name.startswith("step") or name.endswith("m65536") else WINDOW_CALLS


def time_legs():
    dev = torch.device("cuda:0")
    print(json.dumps(dict(leg="device", device=torch.cuda.get_device_name(0))), flush=True)
    for name, (first, second) in LEGS.items():
        forms = _leg(name, dev)
        calls = _calls(name)
        for _ in range(WARMUP if calls == WINDOW_CALLS else 5):
            forms[0]()
            forms[1]()
        torch.cuda.synchronize()
        w = np.array([_window(forms, calls) for _ in range(WINDOWS)])
        res = {"leg": name, "windows": WINDOWS, "calls_per_window": calls, first: _stats(w[:, 0]), second: _stats(w[:, 1])}
        res[f"{first}_over_{second}"] = res[first]["median_ms"] / res[second]["median_ms"]
        print(json.dumps(res), flush=True)
        del forms
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
        del forms
        torch.cuda.empty_cache()


def _short(name):
    words = name.replace("(anonymous namespace)::", "").split("(")[0].split("<")[0].split("::")[-1].split()
    return words[-1] if words else name


def count_launches(trace_csv):
    rows = list(csv.DictReader(open(trace_csv)))
    rows.sort(key=lambda r: int(r["Start_Timestamp"]))
    marks = [i for i, r in enumerate(rows) if MARK in r["Kernel_Name"]]
    assert len(marks) == 4 * len(LEGS), (len(marks), "marks in the trace")
    out = {}
    for k, (name, labels) in enumerate(LEGS.items()):
        for j, form in enumerate(labels):
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
        sys.exit(f"bank_contrastive_bench: {' '.join(args[:6])} ... ended with status {rc}; nothing further was started")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("what", nargs="?", default="all", choices=["all", "time", "trace", "count"])
    ap.add_argument("arg", nargs="?", default=None)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "bank_contrastive_bench.json"))
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
        result = dict(tool="tools/bank_contrastive_bench.py", device=device, legs=[table[n] for n in LEGS])
        with open(args.out, "w") as f:
            json.dump(result, f, indent=1)
            f.write("\n")
        print(json.dumps(result))


if __name__ == "__main__":
    main()
