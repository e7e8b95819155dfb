"""What the fused flat-buffer optimiser steps (flat_optim.FlatAdamW / FlatLARS, csrc/optim.hip) save over the torch
optimisers they replace: only the step TAIL (clip + optimiser step) is timed, on gradients that are already there.

    python tools/flat_optim_bench.py                  # times every case, counts launches, writes profiles/flat_optim_bench.json
    python tools/flat_optim_bench.py time [--reps N]  # the timings alone, in this process: the device's name, then one JSON line per case
    python tools/flat_optim_bench.py trace            # the traced workload (run under rocprofv3 by the driver form)

Cases: cfg2's model (128 -> 768 x 2 -> 384) with LARS; cfg4's model (128 -> 1024 x 2 -> 384) with AdamW; the reference's
Model(128, 128, 4) with AdamW; a DINO student (Model(96, 128, 4) + DINOHead(128, 384)) with the per-tensor clip loop and
the two-group AdamW of LstmDistillation.py.  The torch form is what DistillTrainer / the DINO CLI run without
--fused_optimizer (gradients are views into one flat buffer, the parameters are torch's own); the fused form is what they
run with it.

Timing: device events around blocks of steps, the two forms alternating block by block in one process, ``--reps`` steps
per form in all after a warm-up; ms per step = total / reps.  Launches per step: one ``rocprofv3 --kernel-trace --stats``
run of the ``trace`` workload, in which every measured block of steps sits between two launches of the library's Barlow
reduction kernel (which no optimiser uses); the kernels between two such marks are counted.  The driver form starts each
part as a child under its own time limit, stops at the first that fails, and never opens the GPU itself."""
import argparse
import csv
import glob
import json
import os
import subprocess
import sys
import tempfile

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

CHILD_TIMEOUT_S = 300
BLOCKS = 5              # alternations per form
TRACE_STEPS = 10
MARK = "barlow_kernel"
CASES = ("cfg2_lars", "cfg4_adamw", "ref128_adamw", "dino_clip_adamw")


def _model(case, dev):
    from cerebralsignalnetworks_amd import Model
    from cerebralsignalnetworks_amd.dino import DINOHead, MultiCropWrapper
    torch.manual_seed(0)
    if case == "cfg2_lars":
        return Model(input_size=128, lstm_size=768, lstm_layers=2, output_size=384, include_top=False).to(dev)
    if case == "cfg4_adamw":
        return Model(input_size=128, lstm_size=1024, lstm_layers=2, output_size=384, include_top=False).to(dev)
    if case == "ref128_adamw":
        return Model(input_size=128, lstm_size=128, lstm_layers=4, output_size=128, include_top=False).to(dev)
    return MultiCropWrapper(Model(input_size=96, lstm_size=128, lstm_layers=4, output_size=128, include_top=False),
                            DINOHead(128, 384, False, True)).to(dev)


def _forms(case, dev):
    """-> (torch step tail, fused step tail, elements, tensors); both on gradients of the same values"""
    from cerebralsignalnetworks_amd.flat_optim import FlatAdamW, FlatLARS
    from cerebralsignalnetworks_amd.losses import LARS
    from cerebralsignalnetworks_amd.trainer import FlatGrads
    m_t, m_f = _model(case, dev), _model(case, dev)
    g_t, g_f = FlatGrads(m_t.parameters()), FlatGrads(m_f.parameters(), flatten_params=True)
    g_t.flat.normal_(generator=torch.Generator(device=dev).manual_seed(1)).mul_(1e-3)
    g_f.flat.copy_(g_t.flat)
    if case == "cfg2_lars":
        kw = dict(lr=0.2, weight_decay=1e-6, weight_decay_filter=True, lars_adaptation_filter=True)
        o_t, o_f = LARS(g_t.params, **kw), FlatLARS(g_f, **kw)
        torch_tail, fused_tail = o_t.step, o_f.step
    elif case in ("cfg4_adamw", "ref128_adamw"):
        o_t, o_f = torch.optim.AdamW(g_t.params, lr=1e-3), FlatAdamW(g_f, lr=1e-3)
        torch_tail, fused_tail = o_t.step, o_f.step
    else:
        clip = 3.0
        named = [(n, p) for n, p in m_t.named_parameters() if p.requires_grad]
        reg = [p for n, p in named if not (n.endswith(".bias") or p.ndim == 1)]
        not_reg = [p for n, p in named if n.endswith(".bias") or p.ndim == 1]
        o_t = torch.optim.AdamW([{"params": reg}, {"params": not_reg, "weight_decay": 0.}])
        no_decay = [p for n, p in m_f.named_parameters() if p.requires_grad and (n.endswith(".bias") or p.ndim == 1)]
        o_f = FlatAdamW(g_f, no_decay=no_decay, clip=clip)

        def torch_tail():                       # LstmDistillation.py:141-150
            for p in m_t.parameters():
                if p.grad is not None:
                    clip_coef = clip / (p.grad.norm(2) + 1e-6)
                    p.grad.mul_(torch.clamp(clip_coef, max=1.0))
            o_t.step()
        fused_tail = o_f.step
    return torch_tail, fused_tail, g_f.flat.numel(), len(g_f.params)


def _block(step, n):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(n):
        step()
    b.record()
    b.synchronize()
    return a.elapsed_time(b)


def time_cases(reps):
    dev = torch.device("cuda:0")
    print(json.dumps(dict(case="device", device=torch.cuda.get_device_name(0))), flush=True)
    out = []
    for case in CASES:
        torch_tail, fused_tail, n, nseg = _forms(case, dev)
        for _ in range(10):
            torch_tail()
            fused_tail()
        torch.cuda.synchronize()
        per = max(1, reps // BLOCKS)
        t_ms = f_ms = 0.0
        for _ in range(BLOCKS):
            t_ms += _block(torch_tail, per)
            f_ms += _block(fused_tail, per)
        res = dict(case=case, elements=n, tensors=nseg, reps=per * BLOCKS, torch_ms_per_step=t_ms / (per * BLOCKS),
                   fused_ms_per_step=f_ms / (per * BLOCKS))
        res["speedup"] = res["torch_ms_per_step"] / res["fused_ms_per_step"]
        print(json.dumps(res), flush=True)
        out.append(res)
        torch.cuda.empty_cache()
    return out


def trace_workload():
    from cerebralsignalnetworks_amd import cabi
    dev = torch.device("cuda:0")
    c = torch.eye(4, device=dev)
    for case in CASES:
        torch_tail, fused_tail, _, _ = _forms(case, dev)
        for _ in range(3):
            torch_tail()
            fused_tail()
        for tail in (torch_tail, fused_tail):       # mark, TRACE_STEPS steps, mark
            torch.cuda.synchronize()
            cabi.barlow_offdiag_sqsum(c)
            for _ in range(TRACE_STEPS):
                tail()
            cabi.barlow_offdiag_sqsum(c)
        torch.cuda.synchronize()


def _short(name):
    """'void csn::(anonymous namespace)::flat_adam_kernel(float*, ...)' -> 'flat_adam_kernel'"""
    words = name.replace("(anonymous namespace)::", "").split("(")[0].split("<")[0].split("::")[-1].split()
    return words[-1] if words else name


def count_launches(trace_csv):
    rows = list(csv.DictReader(open(trace_csv)))
    rows.sort(key=lambda r: int(r["Start_Timestamp"]))
    marks = [i for i, r in enumerate(rows) if MARK in r["Kernel_Name"]]
    assert len(marks) == 4 * len(CASES), (len(marks), "marks in the trace")
    out = {}
    for k, case in enumerate(CASES):
        for j, form in enumerate(("torch", "fused")):
            lo, hi = marks[4 * k + 2 * j], marks[4 * k + 2 * j + 1]
            names = [rows[i]["Kernel_Name"] for i in range(lo + 1, hi)]
            per = len(names) / TRACE_STEPS
            out.setdefault(case, {})[f"{form}_launches_per_step"] = int(per) if per == int(per) else per
            if form == "fused":
                out[case]["fused_kernels"] = [_short(n) for n in names[:len(names) // TRACE_STEPS]]
    return out


def _child(args, stdout=None):
    rc = subprocess.run(["timeout", "-k", "10", str(CHILD_TIMEOUT_S), *args], stdout=stdout).returncode
    if rc != 0:
        sys.exit(f"flat_optim_bench: {' '.join(args[:6])} ... ended with status {rc}; nothing further was started")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("what", nargs="?", default="all", choices=["all", "time", "trace", "count"])
    ap.add_argument("arg", nargs="?", default=None)
    ap.add_argument("--reps", type=int, default=200)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "flat_optim_bench.json"))
    args = ap.parse_args()
    me = os.path.abspath(__file__)
    if args.what == "time":
        time_cases(args.reps)
    elif args.what == "trace":
        trace_workload()
    elif args.what == "count":
        print(json.dumps(count_launches(args.arg)))
    else:
        with tempfile.TemporaryDirectory() as tmp:
            lines = os.path.join(tmp, "time.jsonl")
            with open(lines, "w") as f:
                _child([sys.executable, me, "time", "--reps", str(args.reps)], stdout=f)
            table = {r["case"]: r for r in map(json.loads, open(lines))}
            _child(["rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", os.path.join(tmp, "trace"), "--",
                    sys.executable, me, "trace"], stdout=subprocess.DEVNULL)
            traces = glob.glob(os.path.join(tmp, "trace", "**", "*kernel_trace.csv"), recursive=True)
            assert traces, "rocprofv3 wrote no kernel trace"
            for case, counts in count_launches(traces[0]).items():
                table[case].update(counts)
        device = table.pop("device")["device"]
        result = dict(tool="tools/flat_optim_bench.py", device=device, reps=args.reps, cases=[table[c] for c in CASES])
        with open(args.out, "w") as f:
            json.dump(result, f, indent=1)
            f.write("\n")
        print(json.dumps(result))


if __name__ == "__main__":
    main()
