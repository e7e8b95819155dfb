"""What BiLSTM's inter-layer dropout costs on a training step's forward + backward:

    python tools/bilstm_dropout_bench.py [--out profiles/bilstm_dropout_bench.json] [--reps 20] [--parent_lib PATH]

Per shape, on the same inputs and parameter values, a gradient on every output step and the input gradient asked for:
  (p0)  BiLSTM with the attribute at 0: the layout passes the plans ran before csn_lstm_plan_set_output_dropout existed;
  (p05) the attribute at 0.5: the lower layers' plans store y_all and load dy_all through the masked passes
        (y_out<T, true> / dy_in<true> of csrc/lstm_boundary.hip) instead -- no further launch, no further pass;
  (p0 against the parent) with --parent_lib, the library built from the parent commit: leg (p0) once more in two fresh child
        processes, one on this tree's library and one on the parent's (CSN_LIB_PATH), run in turns.  The parent's library
        has no csn_lstm_plan_set_output_dropout: the child drops the symbol from the binding and answers the p = 0
        settings of the module itself (any other value raises).
Timing: one pair of device events around one forward + backward, the legs alternating sample by sample in one process
after a warm-up of all of them; per leg the median over the repetitions, min / max.  The spread of a leg is max - min.
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


def _case(case, dev):
    from cerebralsignalnetworks_amd import BiLSTM
    name, B, T, I, H, L, resident = case
    torch.manual_seed(B + T + H)
    bi = BiLSTM(I, H, L, resident=resident).to(dev).train()
    x = torch.randn(B, T, I, device=dev, requires_grad=True)
    dy = torch.randn(B, T, 2 * H, device=dev)

    def step(p):
        bi.dropout = p
        x.grad = None
        y, _ = bi(x)
        y.backward(dy)
    return bi, step


def child(args):
    """Leg (p0) alone, on whatever library CSN_LIB_PATH names; one JSON line per case."""
    from cerebralsignalnetworks_amd import cabi
    if args.child == "parent":
        cabi.SIGNATURES.pop("csn_lstm_plan_set_output_dropout")

        def p0_only(self, p, *a, **kw):
            if float(p) != 0.0:
                raise RuntimeError("the parent's library has no output dropout")
        cabi.LstmPlan.set_output_dropout = p0_only
    dev = torch.device("cuda:0")
    for case in CASES:
        bi, step = _case(case, dev)
        ms = _time_legs({"p0": lambda: step(0.0)}, args.reps)
        print(json.dumps(dict(case=case[0], lib=os.path.basename(cabi.LIB_PATH), ms=ms["p0"],
                              status=sorted({pl.status() for pl in bi.all_plans()}))), flush=True)
        del bi, step
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
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "bilstm_dropout_bench.json"))
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--parent_lib", default=None, help="libcsn_hip.so built from the parent commit: adds the third leg")
    ap.add_argument("--child", default=None, choices=["new", "parent"], help=argparse.SUPPRESS)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("bilstm_dropout_bench: no GPU is visible (there is no fallback)")
    if args.child:
        return child(args)
    if args.reps < 20:
        sys.exit("bilstm_dropout_bench: at least 20 timed repetitions per shape")
    dev = torch.device("cuda:0")
    out = []
    for case in CASES:
        name, B, T, I, H, L, resident = case
        bi, step = _case(case, dev)
        ms = _time_legs({"p0": lambda: step(0.0), "p05": lambda: step(0.5)}, args.reps)
        torch.cuda.synchronize()
        res = dict(case=name, B=B, T=T, I=I, H=H, L=L, dtype="bf16", resident=resident, reps=args.reps,
                   plans=sorted({(pl.desc.I, pl.reverse, pl.path()) + pl.kernel_names() for pl in bi.all_plans()}),
                   status=sorted({pl.status() for pl in bi.all_plans()}), interface_bytes=B * T * 2 * H * 4,
                   p0=_stats(ms["p0"]), p05=_stats(ms["p05"]))
        res["p05_minus_p0_ms"] = res["p05"]["median_ms"] - res["p0"]["median_ms"]
        res["p05_minus_p0_outside_the_spread_of_both_legs"] = bool(abs(res["p05_minus_p0_ms"]) >
                                                                   max(res["p0"]["spread_ms"], res["p05"]["spread_ms"]))
        print(json.dumps(res), flush=True)
        out.append(res)
        del bi, step
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
            res["p0_child_new"], res["p0_child_parent"] = new, par
            res["p0_new_minus_parent_ms"] = new["median_ms"] - par["median_ms"]
            res["p0_new_minus_parent_inside_the_spread_of_both_legs"] = bool(abs(res["p0_new_minus_parent_ms"]) <=
                                                                             max(new["spread_ms"], par["spread_ms"]))
            print(json.dumps({k: res[k] for k in ("case", "p0_child_new", "p0_child_parent", "p0_new_minus_parent_ms",
                                                  "p0_new_minus_parent_inside_the_spread_of_both_legs")}), flush=True)
    result = dict(tool="tools/bilstm_dropout_bench.py", device=torch.cuda.get_device_name(0), csrc_sha16=csrc_sha16(),
                  parent_leg="measured" if args.parent_lib else "not measured", cases=out)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
