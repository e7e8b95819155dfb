"""Speed of the LSTM modules against the parent commit's cerebralsignalnetworks_amd/lstm_model.py (tools/lstm_module_identity.py's
companion: a refactor of the Python layer must cost nothing, on the device or on the host).

    git show <parent>:cerebralsignalnetworks_amd/lstm_model.py > cerebralsignalnetworks_amd/_lstm_model_parent.py
    python tools/lstm_module_bench.py --parent-module cerebralsignalnetworks_amd/_lstm_model_parent.py --parent-commit <hash> \
        [--out profiles/lstm_module_bench.json] [--rounds 2] [--reps 20] [--bench-rounds 4]

Parent and this tree run in fresh child processes in turns; a parent child imports the package with the parent's file in the
place of ``cerebralsignalnetworks_amd.lstm_model`` (a finder in front of sys.meta_path, in that child only), so trainers,
models and bench.py all run on it.  Legs:
  * bench_py: ``bench.py --gpus 1`` at its own configuration, its ms_per_step, one sample per child;
  * bilstm_cfg2 / bilstm_h96_resident: the BiLSTM training steps of profiles/lstm_boundary_bench.json (forward + backward
    with a gradient on every output step and dx asked for), one pair of device events per sample;
  * host_hiplstm / host_lstm_hx_lengths / host_bilstm: what the Python layer itself costs -- enqueue-to-return wall time
    of forward + backward at B=3 T=5 I=4 H=32 L=2, CALLS calls per sample with no synchronisation inside the timed
    region (one after it), in microseconds per call.
Inside a child the five in-process legs alternate sample by sample after a warm-up of all of them.  Per leg and module: the
median, min, max and spread (max - min) over the samples of all rounds.  The bar of every leg: this tree's median is at most
the parent's median plus the parent's own spread.  Needs a GPU: there is no fallback."""
import argparse
import importlib.abc
import importlib.util
import json
import os
import runpy
import statistics
import subprocess
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

BI_CASES = {"bilstm_cfg2": (256, 500, 128, 768, 2, False), "bilstm_h96_resident": (16, 460, 96, 96, 2, True)}     # B T I H L resident
HOST = dict(B=3, T=5, I=4, H=32, L=2)
CALLS = 100
UNITS = dict(bench_py="ms per step", bilstm_cfg2="ms", bilstm_h96_resident="ms", host_hiplstm="us per call",
             host_lstm_hx_lengths="us per call", host_bilstm="us per call")


class _ParentModule(importlib.abc.MetaPathFinder):
    def __init__(self, path):
        self.path = path

    def find_spec(self, name, path, target=None):
        if name == "cerebralsignalnetworks_amd.lstm_model":
            return importlib.util.spec_from_file_location(name, self.path)
        return None


def _bi_step(case, dev):
    from cerebralsignalnetworks_amd import BiLSTM
    B, T, I, H, L, resident = case
    torch.manual_seed(B + T + H)
    bi = BiLSTM(I, H, L, resident=resident).to(dev).train()
    x = torch.randn(B, T, I, device=dev, requires_grad=True)
    dy = torch.randn(B, T, 2 * H, device=dev)

    def step():
        x.grad = None
        y, _ = bi(x)
        y.backward(dy)
    return bi, step


def _host_steps(dev):
    from cerebralsignalnetworks_amd import BiLSTM, LSTM
    from cerebralsignalnetworks_amd.lstm_model import HipLSTM
    B, T, I, H, L = (HOST[k] for k in "BTIHL")
    torch.manual_seed(5)
    hip, lstm, bi = (cls(I, H, L).to(dev).train() for cls in (HipLSTM, LSTM, BiLSTM))
    x = torch.randn(B, T, I, device=dev)
    h0, c0 = torch.randn(L, B, H, device=dev, requires_grad=True), torch.randn(L, B, H, device=dev, requires_grad=True)
    dy_last, dy, dy2 = torch.randn(B, H, device=dev), torch.randn(B, T, H, device=dev), torch.randn(B, T, 2 * H, device=dev)
    lengths = [T, 0, 2]

    def run_hip():
        hip(x).backward(dy_last)

    def run_lstm():
        lstm(x, (h0, c0), lengths=lengths)[0].backward(dy)

    def run_bi():
        bi(x)[0].backward(dy2)
    return (hip, lstm, bi), {"host_hiplstm": run_hip, "host_lstm_hx_lengths": run_lstm, "host_bilstm": run_bi}


def child_legs(args):
    dev = torch.device("cuda:0")
    modules, legs = [], {}
    for name, case in BI_CASES.items():
        bi, step = _bi_step(case, dev)
        modules.append(bi)
        legs[name] = step
    host_modules, host = _host_steps(dev)
    modules += host_modules

    def many(fn):
        def run():
            for _ in range(CALLS):
                fn()
        return run
    legs.update({n: many(fn) for n, fn in host.items()})
    for _ in range(2):
        for fn in legs.values():
            fn()
    torch.cuda.synchronize()
    samples = {n: [] for n in legs}
    for _ in range(args.reps):
        for n, fn in legs.items():
            if n in BI_CASES:
                a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                a.record()
                fn()
                b.record()
                b.synchronize()
                samples[n].append(a.elapsed_time(b))
            else:
                t0 = time.perf_counter()
                fn()
                dt = time.perf_counter() - t0
                torch.cuda.synchronize()
                samples[n].append(1e6 * dt / CALLS)
    status = sorted({pl.status() for m in modules for pl in m.all_plans()})
    import cerebralsignalnetworks_amd.lstm_model as lm
    print(json.dumps(dict(samples=samples, status=status, module_file=os.path.basename(lm.__file__))), flush=True)


def _run_child(kind, module, extra, limit):
    cmd = ["timeout", "-k", "10", str(limit), sys.executable, os.path.abspath(__file__), "--child", kind] + extra
    if module:
        cmd += ["--parent-module", os.path.abspath(module)]
    done = subprocess.run(cmd, cwd=ROOT, stdout=subprocess.PIPE, text=True)
    lines = [ln for ln in done.stdout.splitlines() if ln.startswith("{")]
    if done.returncode != 0 or len(lines) != 1:
        sys.exit(f"lstm_module_bench: the {kind} child on {'the parent module' if module else 'this tree'} exited {done.returncode} "
                 f"with {len(lines)} result line(s); nothing further was started")
    return json.loads(lines[0])


def _stats(v):
    return dict(n=len(v), median=statistics.median(v), min=min(v), max=max(v), spread=max(v) - min(v), samples=[round(t, 3) for t in v])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent-module", default=None, help="the parent commit's lstm_model.py (git show), in a git-ignored place")
    ap.add_argument("--parent-commit", default=None, help="hash of the parent commit")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "lstm_module_bench.json"))
    ap.add_argument("--rounds", type=int, default=2, help="rounds of (parent, this) children for the in-process legs")
    ap.add_argument("--reps", type=int, default=20, help="samples per leg and child")
    ap.add_argument("--bench-rounds", type=int, default=4, help="rounds of (parent, this) runs of bench.py")
    ap.add_argument("--child", default=None, choices=["legs", "bench"], help=argparse.SUPPRESS)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("lstm_module_bench: no GPU is visible (there is no fallback)")
    if args.child:
        if args.parent_module:
            sys.meta_path.insert(0, _ParentModule(args.parent_module))
        if args.child == "legs":
            return child_legs(args)
        sys.argv = [os.path.join(ROOT, "bench.py"), "--gpus", "1"]
        runpy.run_path(sys.argv[0], run_name="__main__")
        return 0
    if not args.parent_module or not os.path.exists(args.parent_module) or not args.parent_commit:
        sys.exit("lstm_module_bench: --parent-module must name the parent commit's lstm_model.py, --parent-commit its hash")
    samples = {who: {n: [] for n in UNITS} for who in ("parent", "this")}
    bench_config = None
    for _ in range(args.rounds):
        for who, module in (("parent", args.parent_module), ("this", None)):
            r = _run_child("legs", module, ["--reps", str(args.reps)], 600)
            assert r["status"] == [0] and r["module_file"] == os.path.basename(module or "lstm_model.py"), r
            for n, v in r["samples"].items():
                samples[who][n] += v
            print(f"legs: {who} done", flush=True)
    for _ in range(args.bench_rounds):
        for who, module in (("parent", args.parent_module), ("this", None)):
            r = _run_child("bench", module, [], 600)
            samples[who]["bench_py"].append(r["ms_per_step"])
            bench_config = {k: r.get(k) for k in ("config", "steps", "warmup", "dtype")}
            print(f"bench.py: {who} {r['ms_per_step']:.3f} ms per step", flush=True)
    legs = {}
    for n, unit in UNITS.items():
        par, new = _stats(samples["parent"][n]), _stats(samples["this"][n])
        legs[n] = dict(unit=unit, parent=par, this=new, this_minus_parent=new["median"] - par["median"],
                       accepted=bool(new["median"] <= par["median"] + par["spread"]))
        print(json.dumps({n: {k: ({q: w for q, w in v.items() if q != "samples"} if isinstance(v, dict) else v) for k, v in legs[n].items()}}), flush=True)
    result = dict(tool="tools/lstm_module_bench.py: the parent commit's lstm_model.py against this tree's, fresh processes in turns; "
                       "accepted: this tree's median <= the parent's median + the parent's own spread (max - min)",
                  device=torch.cuda.get_device_name(0), parent_commit=args.parent_commit, host_shape=HOST, calls_per_host_sample=CALLS,
                  rounds=args.rounds, reps=args.reps, bench_py=dict(command="bench.py --gpus 1 (its defaults)", **(bench_config or {})),
                  legs=legs, all_accepted=all(v["accepted"] for v in legs.values()))
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")
    print(f"all legs accepted: {result['all_accepted']}")
    return 0 if result["all_accepted"] else 1


if __name__ == "__main__":
    sys.exit(main())
