"""What the attention readout (csn_lstm_plan_set_attention) costs on a training step's forward + backward
of `Model`:

    python tools/lstm_attn_bench.py [--out profiles/lstm_attn_bench.json] [--reps 20] [--parent_lib PATH]

Per shape of tools/lstm_readout_bench.py, on the same inputs and parameter values, one `Model` (include_top=False, bf16) and a
gradient on its features:
  (last)        Model(readout="last"), attention off: the gather of the last step;
  (mean)        Model(readout="mean"): the fused pooling reduction;
  (attn)        Model(readout="attn") with a non-zero query: the score, row and weighted-sum kernels behind the recurrence, the
                pre-passes, dq and the attention term of the dy layout pass in front of the backward's;
  (torch_attn)  the same attention in torch ops on the same parameters: y_all asked of the library (a float32 [B,T,H] tensor),
                softmax(scale (y_all @ q), dim=1), the weighted sum, fc; autograd materialises the [B,T,H] gradient;
  (last against the parent) with --parent_lib, the library built from the parent commit: leg (last) once more in fresh child
                processes, on this tree's library and on the parent's (CSN_LIB_PATH) in turns.  The parent's library has no
                csn_lstm_plan_set_attention: the child drops the symbol from the binding and takes "off" only.
Timing, peak allocation and kernel counts as in tools/lstm_readout_bench.py: one pair of device events around one forward +
backward, the legs alternating sample by sample after a warm-up of all of them, median of the repetitions with min / max.
Needs a GPU: there is no fallback."""
import argparse
import json
import os
import subprocess
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from tools.l2_topk_bench import csrc_sha16      # noqa: E402
from tools.lstm_readout_bench import CASES, D, _kernels, _peak_bytes, _stats, _time_legs      # noqa: E402


def _case(case, dev, readouts):
    from cerebralsignalnetworks_amd import Model
    name, B, T, I, H, L, resident = case
    torch.manual_seed(B + T + H)
    models = {}
    for r in readouts:
        models[r] = Model(I, H, L, D, include_top=False, resident=resident, readout=r).to(dev).train()
        models[r].load_state_dict(models[readouts[0]].state_dict(), strict=False)
    x = torch.randn(B, T, I, device=dev)
    dy = torch.randn(B, D, device=dev)
    if "attn" in models:
        with torch.no_grad():
            models["attn"].lstm.attn_query.copy_(torch.randn(H, device=dev))

    def fused(r):
        def step():
            models[r].zero_grad(set_to_none=True)
            models[r](x).backward(dy)
        return step

    def in_torch():
        m, q = models["last"], models["attn"].lstm.attn_query.detach().clone().requires_grad_(True)

        def step():
            m.zero_grad(set_to_none=True)
            q.grad = None
            y_all, _ = m.lstm(x, want_all=True)
            a = torch.softmax(H ** -0.5 * (y_all @ q), dim=1)
            m.fc((a[:, :, None] * y_all).sum(1)).backward(dy)
        return step
    legs = {r: fused(r) for r in readouts}
    if "attn" in readouts:
        legs["torch_attn"] = in_torch()
    return models, legs


def child(args):
    """Leg (last) alone, on whatever library CSN_LIB_PATH names; one JSON line per case."""
    from cerebralsignalnetworks_amd import cabi
    if args.child == "parent":
        cabi.SIGNATURES.pop("csn_lstm_plan_set_attention")

        def off_only(self, q=None, *rest, **kw):
            if q is not None:
                raise RuntimeError("the parent's library has no attention readout")
        cabi.LstmPlan.set_attention = off_only
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
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "lstm_attn_bench.json"))
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--parent_lib", default=None, help="libcsn_hip.so built from the parent commit: adds the last leg")
    ap.add_argument("--child", default=None, choices=["new", "parent"], help=argparse.SUPPRESS)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("lstm_attn_bench: no GPU is visible (there is no fallback)")
    if args.child:
        return child(args)
    if args.reps < 20:
        sys.exit("lstm_attn_bench: at least 20 timed repetitions per shape")
    dev = torch.device("cuda:0")
    out = []
    for case in CASES:
        name, B, T, I, H, L, resident = case
        models, legs = _case(case, dev, ["last", "mean", "attn"])
        ms = _time_legs(legs, args.reps)
        torch.cuda.synchronize()
        plans = [pl for m in models.values() for pl in m.lstm.all_plans()]
        res = dict(case=name, B=B, T=T, I=I, H=H, L=L, D=D, dtype="bf16", resident=resident, reps=args.reps,
                   plans=sorted({(pl.path(),) + pl.kernel_names() for pl in plans}), status=sorted({pl.status() for pl in plans}),
                   y_all_bytes=B * T * H * 4, legs={n: _stats(v) for n, v in ms.items()},
                   peak_allocated_bytes_above_start={n: _peak_bytes(fn) for n, fn in legs.items()},
                   device_kernels_per_step={n: _kernels(fn) or "not measured" for n, fn in legs.items()})
        res["torch_attn_over_fused_attn"] = res["legs"]["torch_attn"]["median_ms"] / res["legs"]["attn"]["median_ms"]
        res["fused_attn_minus_last_ms"] = res["legs"]["attn"]["median_ms"] - res["legs"]["last"]["median_ms"]
        res["fused_attn_minus_mean_ms"] = res["legs"]["attn"]["median_ms"] - res["legs"]["mean"]["median_ms"]
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
    result = dict(tool="tools/lstm_attn_bench.py", device=torch.cuda.get_device_name(0), csrc_sha16=csrc_sha16(),
                  parent_leg="measured" if args.parent_lib else "not measured", cases=out)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
