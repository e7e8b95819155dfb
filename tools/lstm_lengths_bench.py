"""Cost of variable-length batches: forward + backward of lstm_model.LSTM at cfg2 (B 256, T 500, I 128, H 768, L 2, bf16),
timed warm with HIP events (median and spread over the timed iterations).

    python tools/lstm_lengths_bench.py --case dense|all_T|half|ragged [--iters N] [--T 500] [--B 256]

One case per process, so that a job can give each its own time limit:
  dense   no lengths (runs on a commit without the feature too: the yardstick for "plans without lengths are untouched")
  all_T   lengths all T against no lengths: the price of the masked kernels, the masked transposes and the gathers
  half    lengths with max = T/2 inside a T plan against a plan created with T/2: the overhead of running short
  ragged  lengths uniform in [T/2, T] against the same batch run padded (no lengths): what a user gains
Prints one JSON line."""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from cerebralsignalnetworks_amd import LSTM  # noqa: E402


def _time(step, iters, warmup=3):
    for _ in range(warmup):
        step()
    ms = []
    for _ in range(iters):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        step()
        b.record()
        b.synchronize()
        ms.append(a.elapsed_time(b))
    ms.sort()
    return dict(median_ms=ms[len(ms) // 2], min_ms=ms[0], max_ms=ms[-1])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--case", required=True, choices=["dense", "all_T", "half", "ragged"])
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--B", type=int, default=256)
    ap.add_argument("--T", type=int, default=500)
    args = ap.parse_args()
    B, T, I, H, L = args.B, args.T, 128, 768, 2
    dev = torch.device("cuda:0")
    torch.manual_seed(0)
    m = LSTM(I, H, L).to(dev)
    x = torch.randn(B, T, I, device=dev, requires_grad=True)
    h0 = (0.5 * torch.randn(L, B, H, device=dev)).requires_grad_(True)
    c0 = torch.randn(L, B, H, device=dev).requires_grad_(True)

    def step(xx, lengths=None):
        def run():
            out, (h_n, c_n) = m(xx, (h0, c0)) if lengths is None else m(xx, (h0, c0), lengths=lengths)
            (out.sum() + h_n.sum() + c_n.sum()).backward()
        return run

    res = dict(case=args.case, B=B, T=T, I=I, H=H, L=L, iters=args.iters)
    if args.case == "dense":
        res["dense"] = _time(step(x), args.iters)
    elif args.case == "all_T":
        res["dense"] = _time(step(x), args.iters)
        res["all_T"] = _time(step(x, [T] * B), args.iters)
        res["overhead_pct"] = 100.0 * (res["all_T"]["median_ms"] / res["dense"]["median_ms"] - 1.0)
    elif args.case == "half":
        half = T // 2
        xs = x.detach()[:, :half].contiguous().requires_grad_(True)
        res["plan_T_half"] = _time(step(xs), args.iters)
        res["lengths_half_in_T_plan"] = _time(step(x, [half] * B), args.iters)
        res["overhead_pct"] = 100.0 * (res["lengths_half_in_T_plan"]["median_ms"] / res["plan_T_half"]["median_ms"] - 1.0)
    else:
        g = torch.Generator().manual_seed(1)
        lengths = torch.randint(T // 2, T + 1, (B,), generator=g).tolist()
        res["padded"] = _time(step(x), args.iters)
        res["ragged"] = _time(step(x, lengths), args.iters)
        res["longest"], res["mean_length"] = max(lengths), sum(lengths) / B
        res["gain_pct"] = 100.0 * (1.0 - res["ragged"]["median_ms"] / res["padded"]["median_ms"])
    res["path"] = m.all_plans()[0].path()
    res["status"] = [pl.status() for pl in m.all_plans()]
    print(json.dumps(res), flush=True)


if __name__ == "__main__":
    main()
