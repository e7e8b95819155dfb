"""What the pooled readout (csn_lstm_plan_set_readout) costs and saves on a training step's forward +
backward of `Model`:

    python tools/lstm_readout_bench.py [--out profiles/lstm_readout_bench.json] [--reps 20] [--parent_lib PATH]

Per shape, on the same inputs and parameter values, one `Model` (include_top=False, bf16) and a gradient on its features:
  (last)        Model(readout="last"): the gather of the last step, dy_last into the last step;
  (mean, max)   Model(readout=...): the pooling reduction behind the recurrence, dy_last expanded inside the dy layout pass;
  (torch_mean,  the same pooling written in torch on the same parameters: y_all asked of the library (a float32 [B,T,H]
   torch_max)   tensor), `y_all.mean(1)` / `y_all.max(1).values`, fc; autograd materialises the [B,T,H] gradient and the
                library's dy layout pass reads it;
  (last against the parent) with --parent_lib, the library built from the parent commit: leg (last) once more in fresh child
                processes, on this tree's library and on the parent's (CSN_LIB_PATH) in turns.  The parent's library has no
                csn_lstm_plan_set_readout: the child drops the symbol from the binding and answers "last" itself.
Timing: one pair of device events around one forward + backward, the legs alternating sample by sample in one process after a
warm-up of all of them; per leg the median over the repetitions, min / max.  Per leg also the peak of torch's allocated
memory over one step above what was allocated before it (the plans' workspaces are allocated before: they are the same in
every leg), and the device kernels of one step as torch.profiler counts them ("not measured" where it gives none).
Needs a GPU: there is no fallback."""
import argparse
import json
import os
import statistics
import subprocess
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from tools.l2_topk_bench import csrc_sha16      # noqa: E402

# (name, B, T, I, H, L, resident): bench.py --config cfg2's LSTM shape, and the reference's H = 96 model on resident plans
CASES = [("cfg2", 256, 500, 128, 768, 2, False), ("ref_h96_resident", 16, 460, 96, 96, 2, True)]
D = 384


def _stats(ms):
    return dict(median_ms=statistics.median(ms), min_ms=min(ms), max_ms=max(ms), spread_ms=max(ms) - min(ms))


def _time_legs(legs, reps):
    """{name: fn} -> {name: [ms] * reps}, the legs in turns after two warm-up rounds of all of them."""
    for _ in range(2):
        for fn in legs.values():
            fn()
    torch.cuda.synchronize()
    ms = {n: [] for n in legs}
    for _ in range(reps):
        for n, fn in legs.items():
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            fn()
            b.record()
            b.synchronize()
            ms[n].append(a.elapsed_time(b))
    return ms


def _peak_bytes(fn):
    torch.cuda.synchronize()
    before = torch.cuda.memory_allocated()
    torch.cuda.reset_peak_memory_stats()
    fn()
    torch.cuda.synchronize()
    return torch.cuda.max_memory_allocated() - before


def _kernels(fn):
    """Device kernels of one fn() as torch.profiler counts them, or None."""
    try:
        from torch.profiler import ProfilerActivity, profile
        with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as prof:
            fn()
            torch.cuda.synchronize()
        n = sum(1 for e in prof.events() if str(e.device_type).endswith("CUDA") and "memcpy" not in e.name.lower()
                and "memset" not in e.name.lower())
        return n or None
    except Exception as e:      # noqa: BLE001  (a profiler that does not start: the timing stands without the count)
        print(f"lstm_readout_bench: no kernel count ({type(e).__name__}: {e})", file=sys.stderr)
        return None


def _case(case, dev, readouts):
    from cerebralsignalnetworks_amd import Model
    name, B, T, I, H, L, resident = case
    torch.manual_seed(B + T + H)
    models = {}
    for r in readouts:
        models[r] = Model(I, H, L, D, include_top=False, resident=resident, readout=r).to(dev).train()
        models[r].load_state_dict(models[readouts[0]].state_dict())
    x = torch.randn(B, T, I, device=dev)
    dy = torch.randn(B, D, device=dev)

    def fused(r):
        def step():
            models[r].zero_grad(set_to_none=True)
            models[r](x).backward(dy)
        return step

    def in_torch(r):
        m = models["last"]

        def step():
            m.zero_grad(set_to_none=True)
            y_all, _ = m.lstm(x, want_all=True)
            m.fc(y_all.mean(1) if r == "mean" else y_all.max(1).values).backward(dy)
        return step
    legs = {r: fused(r) for r in readouts}
    if "mean" in readouts:
        legs.update(torch_mean=in_torch("mean"), torch_max=in_torch("max"))
    return models, legs


def child(args):
    """Leg (last) alone, on whatever library CSN_LIB_PATH names; one JSON line per case."""
    from cerebralsignalnetworks_amd import cabi
    if args.child == "parent":
        cabi.SIGNATURES.pop("csn_lstm_plan_set_readout")

        def last_only(self, mode):
            if cabi.readout_mode(mode) != cabi.READOUT_LAST:
                raise RuntimeError("the parent's library has no pooled readout")
        cabi.LstmPlan.set_readout = last_only
    dev = torch.device("cuda:0")
    for case in CASES:
        models, legs = _case(case, dev, ["last"])
        ms = _time_legs(legs, args.reps)
        print(json.dumps(dict(case=case[0], lib=os.path.basename(cabi.LIB_PATH), ms=ms["last"],
                              status=sorted({pl.status() for pl in models["last"].lstm.all_plans()}))), flush=True)
        del models, legs
        torch.cuda.empty_cache()


def _run_child(which, lib, reps):
    env = dict(os.environ)
    if lib:
        env["CSN_LIB_PATH"] = os.path.abspath(lib)
    else:
        env.pop("CSN_LIB_PATH", None)
    done = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", which, "--reps", str(reps)], env=env, check=True,
                          stdout=subprocess.PIPE, text=True, timeout=900)
    return {r["case"]: r for r in (json.loads(line) for line in done.stdout.splitlines() if line.startswith("{"))}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "lstm_readout_bench.json"))
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--parent_lib", default=None, help="libcsn_hip.so built from the parent commit: adds the last leg")
    ap.add_argument("--child", default=None, choices=["new", "parent"], help=argparse.SUPPRESS)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("lstm_readout_bench: no GPU is visible (there is no fallback)")
    if args.child:
        return child(args)
    if args.reps < 20:
        sys.exit("lstm_readout_bench: at least 20 timed repetitions per shape")
    dev = torch.device("cuda:0")
    out = []
    for case in CASES:
        name, B, T, I, H, L, resident = case
        models, legs = _case(case, dev, ["last", "mean", "max"])
        ms = _time_legs(legs, args.reps)
        torch.cuda.synchronize()
        plans = [pl for m in models.values() for pl in m.lstm.all_plans()]
        res = dict(case=name, B=B, T=T, I=I, H=H, L=L, D=D, dtype="bf16", resident=resident, reps=args.reps,
                   plans=sorted({(pl.path(),) + pl.kernel_names() for pl in plans}), status=sorted({pl.status() for pl in plans}),
                   y_all_bytes=B * T * H * 4, legs={n: _stats(v) for n, v in ms.items()},
                   peak_allocated_bytes_above_start={n: _peak_bytes(fn) for n, fn in legs.items()},
                   device_kernels_per_step={n: _kernels(fn) or "not measured" for n, fn in legs.items()})
        for r in ("mean", "max"):
            res[f"torch_{r}_over_fused_{r}"] = res["legs"][f"torch_{r}"]["median_ms"] / res["legs"][r]["median_ms"]
            res[f"fused_{r}_minus_last_ms"] = res["legs"][r]["median_ms"] - res["legs"]["last"]["median_ms"]
        print(json.dumps(res), flush=True)
        out.append(res)
        del models, legs, plans
        torch.cuda.empty_cache()
    if args.parent_lib:
        # two rounds of (parent, new) child processes: each leg's samples come from two processes, run in turns
        samples = {"parent": {}, "new": {}}
        for _ in range(2):
            for which, lib in (("parent", args.parent_lib), ("new", None)):
                for name, r in _run_child(which, lib, max(10, args.reps // 2)).items():
                    assert r["status"] == [0], r
                    samples[which].setdefault(name, []).extend(r["ms"])
        for res in out:
            new, par = _stats(samples["new"][res["case"]]), _stats(samples["parent"][res["case"]])
            res["last_child_new"], res["last_child_parent"] = new, par
            res["last_new_minus_parent_ms"] = new["median_ms"] - par["median_ms"]
            res["last_new_inside_the_recorded_spread_of_the_parent"] = bool(par["min_ms"] <= new["median_ms"] <= par["max_ms"])
            print(json.dumps({k: res[k] for k in ("case", "last_child_new", "last_child_parent", "last_new_minus_parent_ms",
                                                  "last_new_inside_the_recorded_spread_of_the_parent")}), flush=True)
    result = dict(tool="tools/lstm_readout_bench.py", device=torch.cuda.get_device_name(0), csrc_sha16=csrc_sha16(),
                  parent_leg="measured" if args.parent_lib else "not measured", cases=out)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
