"""Cost of the LSTM state: forward + backward of lstm_model.LSTM with and without (h0, c0) -> (h_n, c_n), timed with
HIP events, next to HipLSTM's stateless step on the same shape (the weight-stationary kernels where they apply).

    python tools/lstm_state_bench.py [--iters N]

Shapes: cfg2 (B 256, T 500, I 128, H 768, L 2) and the reference's Model(128, 128, 4) at B 16, T 460; bf16 compute.
Prints one JSON line per shape (median ms over the timed iterations)."""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from cerebralsignalnetworks_amd import LSTM  # noqa: E402
from cerebralsignalnetworks_amd.lstm_model import HipLSTM  # noqa: E402


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
    return sorted(ms)[len(ms) // 2]


def bench(B, T, I, H, L, iters):
    dev = torch.device("cuda:0")
    torch.manual_seed(0)
    m = LSTM(I, H, L).to(dev)
    x = torch.randn(B, T, I, device=dev, requires_grad=True)
    h0 = (0.5 * torch.randn(L, B, H, device=dev)).requires_grad_(True)
    c0 = torch.randn(L, B, H, device=dev).requires_grad_(True)

    def stateless():
        out, (h_n, c_n) = m(x)
        (out.sum() + h_n.sum() + c_n.sum()).backward()

    def stateful():
        out, (h_n, c_n) = m(x, (h0, c0))
        (out.sum() + h_n.sum() + c_n.sum()).backward()

    hip = HipLSTM(I, H, L).to(dev)
    hip.load_state_dict(m.state_dict())

    def hip_step():
        y_all, _ = hip(x, want_all=True)
        y_all.sum().backward()

    res = dict(B=B, T=T, I=I, H=H, L=L, iters=iters, lstm_no_state_ms=_time(stateless, iters),
               lstm_state_ms=_time(stateful, iters), hiplstm_ms=_time(hip_step, iters),
               path=m.all_plans()[0].path(), hiplstm_path=hip.all_plans()[0].path())
    res["state_overhead_pct"] = 100.0 * (res["lstm_state_ms"] / res["lstm_no_state_ms"] - 1.0)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=10)
    args = ap.parse_args()
    for shape in [(256, 500, 128, 768, 2), (16, 460, 128, 128, 4)]:
        print(json.dumps(bench(*shape, args.iters)), flush=True)
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
