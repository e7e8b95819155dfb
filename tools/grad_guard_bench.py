"""What the device-side gradient guard costs:

    python tools/grad_guard_bench.py [--out profiles/grad_guard_bench.json] [--reps 20] [--parent_lib PATH]

At the flat buffer sizes of bench.py's cfg2 model (Model(128, 768, 2, 384)) and of the reference's Model(96, 96, 2), for
RMSprop, AdamW and LARS, on seeded buffers with the model's own segment cut:
  (a) with --parent_lib, the library built from the parent commit: the UNGUARDED step of this tree against the parent's,
      each in fresh child processes of its own (CSN_LIB_PATH is read at import), two rounds of (parent, new) in turns.  The
      step kernels became templates on the guard; their unguarded instantiations should cost what they cost before.  The
      parent's library has none of the five new symbols: its child drops them from the binding.
  (b) guard + guarded step (csn_grad_guard, csn_*_step_guarded) against torch.nn.utils.clip_grad_norm_ on the same
      gradient views + the unguarded step, in turns in one process, with the number of device launches of each leg
      (torch.profiler's kernel events over one call; null where the profiler gives none).
Timing: one pair of device events around one call, after a warm-up of all legs; per leg the median over the repetitions,
min / max; the spread of a leg is max - min.  The clip is active (max_norm = half the norm).  Needs a GPU: no fallback."""
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

NEW_SYMBOLS = ("csn_grad_guard_scratch_bytes", "csn_grad_guard", "csn_rmsprop_step_guarded", "csn_adam_step_guarded",
               "csn_lars_step_guarded")
MODELS = {"cfg2": dict(input_size=128, lstm_size=768, lstm_layers=2, output_size=384, include_top=False),
          "ref_h96": dict(input_size=96, lstm_size=96, lstm_layers=2)}
OPTIMISERS = ("rmsprop", "adamw", "lars")


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


def _launches(fn):
    """Device kernels of one call, or None where the profiler reports none."""
    try:
        from torch.profiler import ProfilerActivity, profile
        torch.cuda.synchronize()
        with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as prof:
            fn()
            torch.cuda.synchronize()
        n = sum(1 for e in prof.events() if str(getattr(e, "device_type", "")).endswith("CUDA"))
        return n or None
    except Exception:
        return None


def _flat(name, dev):
    """A FlatGrads of the model's parameter tensors (values and gradients seeded normal; the step does not care)."""
    from cerebralsignalnetworks_amd import Model
    from cerebralsignalnetworks_amd.trainer import FlatGrads
    torch.manual_seed(5)
    shapes = [p.shape for p in Model(**MODELS[name]).parameters()]
    params = [torch.nn.Parameter(0.05 * torch.randn(s, device=dev)) for s in shapes]
    fg = FlatGrads(params, flatten_params=True)
    fg.flat.copy_(1e-3 * torch.randn(fg.flat.numel(), device=dev))
    return fg


def _optimiser(kind, fg, **kw):
    from cerebralsignalnetworks_amd import FlatAdamW, FlatLARS
    from cerebralsignalnetworks_amd.trainer import FlatRMSprop
    if kind == "rmsprop":
        return FlatRMSprop(fg, lr=1e-4, **kw)
    if kind == "adamw":
        return FlatAdamW(fg, lr=1e-4, **kw)
    return FlatLARS(fg, lr=1e-3, weight_decay=1e-6, weight_decay_filter=True, lars_adaptation_filter=True, **kw)


def child(args):
    """Leg (a): the unguarded steps alone, on whatever library CSN_LIB_PATH names; one JSON line per (model, optimiser)."""
    from cerebralsignalnetworks_amd import cabi
    if args.child == "parent":
        for name in NEW_SYMBOLS:
            cabi.SIGNATURES.pop(name)
    dev = torch.device("cuda:0")
    for model in MODELS:
        fg = _flat(model, dev)
        opts = {kind: _optimiser(kind, fg) for kind in OPTIMISERS}
        ms = _time_legs({kind: opt.step for kind, opt in opts.items()}, args.reps)
        for kind in OPTIMISERS:
            print(json.dumps(dict(case=f"{model}/{kind}", lib=os.path.abspath(cabi.LIB_PATH), ms=ms[kind])), flush=True)
        del fg, opts
        torch.cuda.empty_cache()


def _run_child(which, lib, reps):
    env = dict(os.environ)
    if lib:
        env["CSN_LIB_PATH"] = os.path.abspath(lib)
    else:
        env.pop("CSN_LIB_PATH", None)
    done = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", which, "--reps", str(reps)], env=env, check=True,
                          stdout=subprocess.PIPE, text=True, timeout=600)
    return {r["case"]: r for r in (json.loads(line) for line in done.stdout.splitlines() if line.startswith("{"))}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "grad_guard_bench.json"))
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--parent_lib", default=None, help="libcsn_hip.so built from the parent commit: adds leg (a)")
    ap.add_argument("--child", default=None, choices=["new", "parent"], help=argparse.SUPPRESS)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("grad_guard_bench: no GPU is visible (there is no fallback)")
    if args.child:
        return child(args)
    if args.reps < 20:
        sys.exit("grad_guard_bench: at least 20 timed repetitions per leg")
    dev = torch.device("cuda:0")
    out, counting = [], []
    for model in MODELS:
        fg = _flat(model, dev)
        n, nseg = fg.flat.numel(), len(fg.params)
        max_norm = 0.5 * float(fg.flat.double().pow(2).sum().sqrt())
        grads = fg.flat.clone()
        for kind in OPTIMISERS:
            guarded, plain = _optimiser(kind, fg, max_grad_norm=max_norm), _optimiser(kind, fg)

            def torch_clip_then_step(fg=fg, plain=plain, max_norm=max_norm):      # (bound now: the launch count calls it later)
                torch.nn.utils.clip_grad_norm_(fg.params, max_norm)
                plain.step()

            def restore():                  # (clip_grad_norm_ scales the buffer in place: every sample starts from the same one)
                fg.flat.copy_(grads)
            legs = {"guard_and_guarded_step": guarded.step, "torch_clip_and_step": torch_clip_then_step, "step_alone": plain.step}
            for _ in range(2):
                for fn in legs.values():
                    restore()
                    fn()
            ms = {k: [] for k in legs}
            for _ in range(args.reps):
                for k, fn in legs.items():
                    restore()
                    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    a.record()
                    fn()
                    b.record()
                    b.synchronize()
                    ms[k].append(a.elapsed_time(b))
            restore()
            res = dict(case=f"{model}/{kind}", n=n, nseg=nseg, bytes=4 * n, reps=args.reps, max_norm=max_norm,
                       scale=float(guarded.guard.scale.item()), **{k: _stats(v) for k, v in ms.items()})
            res["launches"] = None
            counting.append((res, legs))
            res["guard_minus_torch_clip_ms"] = res["guard_and_guarded_step"]["median_ms"] - res["torch_clip_and_step"]["median_ms"]
            res["guard_cost_over_step_alone_ms"] = res["guard_and_guarded_step"]["median_ms"] - res["step_alone"]["median_ms"]
            print(json.dumps(res), flush=True)
            out.append(res)
    if args.parent_lib:
        samples = {"parent": {}, "new": {}}
        for _ in range(2):
            for which, lib in (("parent", args.parent_lib), ("new", None)):
                for name, r in _run_child(which, lib, max(10, args.reps // 2)).items():
                    samples[which].setdefault(name, []).extend(r["ms"])
        for res in out:
            new, par = _stats(samples["new"][res["case"]]), _stats(samples["parent"][res["case"]])
            res["unguarded_child_new"], res["unguarded_child_parent"] = new, par
            res["unguarded_new_minus_parent_ms"] = new["median_ms"] - par["median_ms"]
            res["unguarded_new_minus_parent_inside_the_spread_of_both_legs"] = bool(
                abs(res["unguarded_new_minus_parent_ms"]) <= max(new["spread_ms"], par["spread_ms"]))
            print(json.dumps({k: res[k] for k in ("case", "unguarded_child_new", "unguarded_child_parent",
                                                  "unguarded_new_minus_parent_ms",
                                                  "unguarded_new_minus_parent_inside_the_spread_of_both_legs")}), flush=True)
    result = dict(tool="tools/grad_guard_bench.py", device=torch.cuda.get_device_name(0), csrc_sha16=csrc_sha16(),
                  parent_leg="measured" if args.parent_lib else "not measured", cases=out)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)

    def write():
        with open(args.out, "w") as f:
            json.dump(result, f, indent=1)
            f.write("\n")
    write()                                 # the timings are on disk before the profiler is started
    for res, legs in counting:
        res["launches"] = {k: _launches(fn) for k, fn in legs.items()}
        print(json.dumps(dict(case=res["case"], launches=res["launches"])), flush=True)
    write()


if __name__ == "__main__":
    main()
