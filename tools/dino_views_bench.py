"""What one fused pass over all multi-crop views (LstmDistillation.py --fused_views) is worth on the
DINO trainer's step, against the per-view passes:

    python tools/dino_views_bench.py [--out profiles/dino_views_bench.json] [--reps 20]

Shapes: the trainer's CLI defaults (96 channels, 495 samples, embed_dim 128, 4 LSTM layers, 2 global crops of 300 + 4
local crops of 200 samples) at batch 8 and 64, in bf16 and in float32.  Timed: the whole step as the trainer runs it up to
the optimiser -- crops, teacher forward (no_grad), student forward, loss, gradient zeroing, backward (LSTM gradients
accumulated straight into the flat buffer) -- in its two forms, alternating sample by sample in ONE process after a
warm-up of both, a pair of device events around --steps steps and a synchronise behind them.  Per form: median, min / max
and interquartile range per step; the recurrence launches and cells of one step from csn_lstm_profile_read, summed over
every LSTM call of the step; and the kernel launches of one step counted by the torch profiler in a step of its own (null
where the profiler gives no device events).  No ratio is asserted: the file says what was measured.

Every shape runs in a child process of its own under `timeout -k 10`, and the driver stops at the first status that is
not 0.  Needs a GPU: there is no fallback."""
import argparse
import json
import os
import statistics
import subprocess
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from tools.l2_topk_bench import csrc_sha16      # noqa: E402

SHAPE = dict(C=96, T=495, embed_dim=128, layers=4, out_dim=384, n_global=2, n_local=4, global_len=300, local_len=200)
# (name, B, dtype)
CASES = [("b8_bf16", 8, "bf16"), ("b64_bf16", 64, "bf16"), ("b8_f32", 8, "f32"), ("b64_f32", 64, "f32")]
STEP_ARITHMETIC = dict(       # counted from the code (the issue's table), per layer and direction
    student_sequential_steps=dict(per_view=2 * 300 + 4 * 200, fused=300),
    teacher_sequential_steps=dict(per_view=2 * 300, fused=300),
    row_steps_per_sample=dict(per_view=2 * 300 + 4 * 200, fused=6 * 300))


def _stats(ms):
    q = statistics.quantiles(ms, n=4)
    return dict(median_ms=statistics.median(ms), min_ms=min(ms), max_ms=max(ms), iqr_ms=q[2] - q[0])


class _Counter:
    """Sums csn_lstm_profile_read over every LstmPlan.forward / backward between start() and stop()."""

    def __init__(self, cabi):
        self.cabi, self.on = cabi, False
        self.fwd, self.bwd = cabi.LstmPlan.forward, cabi.LstmPlan.backward
        counter = self

        def forward(plan, *a, **k):
            if not counter.on:
                return counter.fwd(plan, *a, **k)
            plan.profile_enable(True)
            out = counter.fwd(plan, *a, **k)
            counter.add(plan.profile_read(), "fwd")
            plan.profile_enable(False)
            return out

        def backward(plan, *a, **k):
            if not counter.on:
                return counter.bwd(plan, *a, **k)
            plan.profile_enable(True)
            out = counter.bwd(plan, *a, **k)
            counter.add(plan.profile_read(), "bwd")
            plan.profile_enable(False)
            return out

        cabi.LstmPlan.forward, cabi.LstmPlan.backward = forward, backward

    def add(self, prof, which):
        self.total[f"{which}_calls"] += 1
        for k in ("launches", "cells"):
            self.total[f"{which}_{k}"] += prof[f"{which}_{k}"]
        self.total[f"{which}_ms"] += prof[f"{which}_ms"]

    def start(self):
        self.total = dict(fwd_calls=0, fwd_launches=0, fwd_cells=0, fwd_ms=0.0, bwd_calls=0, bwd_launches=0, bwd_cells=0, bwd_ms=0.0)
        self.on = True

    def stop(self):
        self.on = False
        return self.total


def _kernel_launches(fn):
    """Device kernel launches of one fn(), from the torch profiler; None where it reports no device events."""
    try:
        from torch.profiler import ProfilerActivity, profile, supported_activities
        if ProfilerActivity.CUDA not in supported_activities():
            return None
        with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as prof:
            fn()
            torch.cuda.synchronize()
        n = sum(1 for e in prof.events() if str(e.device_type).endswith("CUDA"))
        return n or None
    except Exception as exc:      # (counting is an extra: the timings stand without it)
        print(f"dino_views_bench: launch count not available ({type(exc).__name__}: {exc})", file=sys.stderr)
        return None


def run_case(name, reps, steps, out_path):
    from cerebralsignalnetworks_amd import Model, cabi
    from cerebralsignalnetworks_amd.dino import DINOHead, DINOLoss, MultiCropWrapper, temporal_crops
    from cerebralsignalnetworks_amd.lstm_model import HipLSTM
    from cerebralsignalnetworks_amd.trainer import FlatGrads, check_device_status
    if not torch.cuda.is_available():
        sys.exit("dino_views_bench: no GPU is visible (there is no fallback)")
    (B, dt), = [(b, d) for n, b, d in CASES if n == name]
    s = SHAPE
    dev = torch.device("cuda:0")
    dtype = torch.bfloat16 if dt == "bf16" else torch.float32
    torch.manual_seed(43)
    np.random.seed(43)

    def make(bn=False):
        backbone = Model(input_size=s["C"], lstm_size=s["embed_dim"], lstm_layers=s["layers"], output_size=s["embed_dim"],
                         include_top=False, compute_dtype=dtype)
        return MultiCropWrapper(backbone, DINOHead(s["embed_dim"], s["out_dim"], bn)).to(dev)

    student, teacher = make(), make()
    teacher.load_state_dict(student.state_dict())
    for p in teacher.parameters():
        p.requires_grad = False
    student.train()
    grads = FlatGrads(student.parameters(), flatten_params=False)
    for mod in student.modules():
        if isinstance(mod, HipLSTM):
            mod.direct_grads = "accumulate"
    dino_loss = DINOLoss(s["out_dim"], s["n_global"] + s["n_local"], 0.04, 0.04, 0, 1).to(dev)
    eeg = torch.randn(B, s["T"], s["C"], device=dev)

    def per_view():
        gv, lv = temporal_crops(eeg, s["n_global"], s["n_local"], s["global_len"], s["local_len"])
        with torch.no_grad():
            t_out = torch.stack([teacher(v.contiguous()) for v in gv], dim=0)
        s_out = torch.stack([student(v.contiguous()) for v in gv + lv], dim=0)
        loss = dino_loss(s_out, t_out, 0)
        grads.zero()
        loss.backward()
        return loss

    def fused():
        starts, lengths = temporal_crops(eeg, s["n_global"], s["n_local"], s["global_len"], s["local_len"], as_views=True)
        with torch.no_grad():
            t_out = teacher.forward_views(eeg, starts[:s["n_global"]], lengths[:s["n_global"]])
        s_out = student.forward_views(eeg, starts, lengths)
        loss = dino_loss(s_out, t_out, 0)
        grads.zero()
        loss.backward()
        return loss

    forms = {"per_view": per_view, "fused": fused}
    counter = _Counter(cabi)
    for _ in range(3):                              # warm-up of both forms: code objects, plans, streams, the event pool
        for fn in forms.values():
            fn()
    torch.cuda.synchronize()
    ms = {n: [] for n in forms}
    for _ in range(reps):
        for n, fn in forms.items():
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.cuda.synchronize()
            a.record()
            for _k in range(steps):
                loss = fn()
            b.record()
            b.synchronize()
            torch.cuda.synchronize()
            ms[n].append(a.elapsed_time(b) / steps)
    # the same crops in both forms (one seed): the losses agree to the precision of the compute type
    losses = {}
    for n, fn in forms.items():
        np.random.seed(7)
        dino_loss.center.zero_()
        losses[n] = float(fn().item())
    counts = {}
    for n, fn in forms.items():
        counter.start()
        fn()
        torch.cuda.synchronize()
        counts[n] = counter.stop()
    check_device_status(student, collective=False)
    check_device_status(teacher, collective=False)
    res = dict(case=name, B=B, dtype=dt, **s, reps=reps, steps_per_sample=steps,
               student_plans={n: sorted({(pl.desc.B, pl.desc.T, bool(pl.state)) for pl in student.backbone.lstm.all_plans()
                                         if (pl.desc.B == B) == (n == "per_view")}) for n in forms},
               paths=sorted({(pl.desc.B, pl.desc.T, pl.path()) + pl.kernel_names() for pl in student.backbone.lstm.all_plans()}),
               loss_same_crops=losses, **{n: dict(_stats(v), lstm_profile=counts[n], kernel_launches=None)
                                          for n, v in ms.items()})
    pv, fu = res["per_view"], res["fused"]
    res["fused_minus_per_view_ms"] = fu["median_ms"] - pv["median_ms"]
    res["per_view_over_fused"] = pv["median_ms"] / fu["median_ms"]
    res["spread_ms"] = max(pv["iqr_ms"], fu["iqr_ms"])
    res["fused_is_faster_beyond_spread"] = bool(pv["median_ms"] - fu["median_ms"] > res["spread_ms"])
    with open(out_path, "w") as f:
        json.dump(res, f)
    # the launch count last, behind the record of the timings: it is the one part that runs under a profiler
    for n, fn in forms.items():
        res[n]["kernel_launches"] = _kernel_launches(fn)
    check_device_status(student, collective=False)
    with open(out_path, "w") as f:
        json.dump(res, f)
    print(json.dumps(res), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "dino_views_bench.json"))
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--steps", type=int, default=3, help="training steps per timed sample")
    ap.add_argument("--only", default=None, help="substring of the case names to run")
    ap.add_argument("--case", default=None, help="(child) run this one case and write its record to --out")
    ap.add_argument("--timeout", type=int, default=240, help="seconds each case's process may take")
    args = ap.parse_args()
    if args.reps < 20:
        sys.exit("dino_views_bench: at least 20 timed repetitions per shape")
    if args.case:
        run_case(args.case, args.reps, args.steps, args.out)
        return
    out_dir = os.path.dirname(os.path.abspath(args.out))
    os.makedirs(out_dir, exist_ok=True)
    cases = []
    for name, _, _ in CASES:
        if args.only and args.only not in name:
            continue
        part = os.path.join(out_dir, f".dino_views_bench_{name}.json")
        cmd = ["timeout", "-k", "10", str(args.timeout), sys.executable, os.path.abspath(__file__), "--case", name, "--out", part,
               "--reps", str(args.reps), "--steps", str(args.steps)]
        rc = subprocess.run(cmd, cwd=ROOT).returncode
        if rc != 0:             # a fault, an abort or a time limit: nothing more is started on the GPU
            sys.exit(f"dino_views_bench: case {name} ended with status {rc}; stopping")
        with open(part) as f:
            cases.append(json.load(f))
        os.remove(part)
    import torch as _t
    result = dict(tool="tools/dino_views_bench.py", device=_t.cuda.get_device_name(0) if _t.cuda.is_available() else None,
                  csrc_sha16=csrc_sha16(), step_arithmetic=STEP_ARITHMETIC, cases=cases)
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
