"""What the LSTM's inter-layer dropout (csn_lstm_plan_set_dropout) costs on a training step's
forward + backward at the cfg2 and cfg4 LSTM shapes:

    python tools/lstm_dropout_bench.py [--out profiles/lstm_dropout_bench.json] [--reps 20]

Legs, on the same inputs and parameters: (a) a plain plan -- the path of a library without the feature; (b) a plan created
with CSN_LSTM_DROPOUT at p = 0, which must not differ from (a) beyond the run-to-run spread; (c) the same plan at p = 0.5.
Timing: one pair of device events around --steps forward + backward pairs (5: about 50 ms of work), the legs alternating
sample by sample in one process after a warm-up of all three; reported per leg and per step: the median over the
repetitions, min / max and the interquartile range.  Beside the times: the bytes the two element-wise kernels move per
step (computed from the shapes), the time those bytes take at 4 TB/s (the estimate the feature was planned with), and the
number of dropout launches.  Needs a GPU: there is no fallback."""
import argparse
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from tools.l2_topk_bench import csrc_sha16      # noqa: E402

# (name, B, T, I, H, L): the LSTM of bench.py --config cfg2 / cfg4
CASES = [("cfg2", 256, 500, 128, 768, 2), ("cfg4", 256, 440, 128, 1024, 2)]
PLANNED_BYTES_PER_S = 4e12


def _stats(ms):
    q = statistics.quantiles(ms, n=4)
    return dict(median_ms=statistics.median(ms), min_ms=min(ms), max_ms=max(ms), iqr_ms=q[2] - q[0])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "lstm_dropout_bench.json"))
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--steps", type=int, default=5, help="forward + backward pairs per timed sample")
    ap.add_argument("--only", default=None, help="substring of the case names to run")
    args = ap.parse_args()
    from cerebralsignalnetworks_amd import cabi
    if not torch.cuda.is_available():
        sys.exit("lstm_dropout_bench: no GPU is visible (there is no fallback)")
    if args.reps < 20:
        sys.exit("lstm_dropout_bench: at least 20 timed repetitions per shape")
    dev = torch.device("cuda:0")
    chunk = int(os.environ.get("CSN_LSTM_CHUNK", "32"))
    out = []
    for name, B, T, I, H, L in CASES:
        if args.only and args.only not in name:
            continue
        torch.manual_seed(B + T + H)
        sd = torch.nn.LSTM(I, H, L, batch_first=True).state_dict()
        w = [[sd[f"{n}_l{k}"].to(dev) for k in range(L)] for n in ("weight_ih", "weight_hh", "bias_ih", "bias_hh")]
        grads = [[torch.empty_like(p) for p in group] for group in w]
        x = torch.randn(B, T, I, device=dev)
        dy_last = torch.randn(B, H, device=dev)
        dx = torch.empty(B, T, I, device=dev)
        plain = cabi.LstmPlan(B, T, I, H, L, torch.bfloat16, dev, training=True)
        drop = cabi.LstmPlan(B, T, I, H, L, torch.bfloat16, dev, training=True, dropout=True)

        def step(plan, p, seed):
            plan.set_dropout(p, seed)
            y_last, _ = plan.forward(x, *w)
            plan.backward(dy_last, None, grads, dx=dx)
            return y_last

        legs = {"a_plain_plan": lambda i: step(plain, 0.0, 0), "b_dropout_plan_p0": lambda i: step(drop, 0.0, 0),
                "c_dropout_plan_p0.5": lambda i: step(drop, 0.5, 1000 + i)}
        last = {}
        for i in range(3):                          # warm-up: code objects, side streams, the event pool
            for n, fn in legs.items():
                last[n] = fn(i).clone()
        torch.cuda.synchronize()
        ms = {n: [] for n in legs}
        for i in range(args.reps):
            for n, fn in legs.items():
                a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                a.record()
                for k in range(args.steps):
                    y = fn(i * args.steps + k)
                b.record()
                b.synchronize()
                ms[n].append(a.elapsed_time(b) / args.steps)
                last[n] = y.clone()
        nch = -(-T // chunk)
        es = 2
        fwd_bytes = (L - 1) * 2 * T * B * H * es            # h read, h_drop written
        bwd_bytes = (L - 1) * 2 * T * B * H * 4             # float32 dx read and rewritten
        res = dict(case=name, B=B, T=T, I=I, H=H, L=L, dtype="bf16", reps=args.reps, steps_per_sample=args.steps, path=drop.path(), kernels=drop.kernel_names(),
                   workspace_bytes_plain=cabi.load().csn_lstm_plan_workspace_bytes(plain._plan),
                   workspace_bytes_dropout=cabi.load().csn_lstm_plan_workspace_bytes(drop._plan),
                   dropout_launches_per_step=2 * (L - 1) * nch, dropout_bytes_forward=fwd_bytes, dropout_bytes_backward=bwd_bytes,
                   bytes_bound_estimate_ms=(fwd_bytes + bwd_bytes) / PLANNED_BYTES_PER_S * 1e3,
                   status=[plain.status(), drop.status()], **{n: _stats(v) for n, v in ms.items()})
        res["b_minus_a_ms"] = res["b_dropout_plan_p0"]["median_ms"] - res["a_plain_plan"]["median_ms"]
        res["c_minus_a_ms"] = res["c_dropout_plan_p0.5"]["median_ms"] - res["a_plain_plan"]["median_ms"]
        res["c_cost_over_estimate"] = res["c_minus_a_ms"] / res["bytes_bound_estimate_ms"]
        res["b_bit_equal_a"] = bool(torch.equal(last["a_plain_plan"], last["b_dropout_plan_p0"]))
        res["c_differs_from_a"] = not torch.equal(last["a_plain_plan"], last["c_dropout_plan_p0.5"])
        print(json.dumps(res), flush=True)
        out.append(res)
        del plain, drop, x, dx, last
        torch.cuda.empty_cache()
    result = dict(tool="tools/lstm_dropout_bench.py", device=torch.cuda.get_device_name(0), csrc_sha16=csrc_sha16(), cases=out)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
