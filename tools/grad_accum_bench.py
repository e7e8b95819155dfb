"""What in-place gradient accumulation (CSN_GRAD_ACCUMULATE) costs and saves, timed with HIP events.

    python tools/grad_accum_bench.py [--iters N]            # every measurement below, one child process each
    python tools/grad_accum_bench.py views small|cfg2       # one measurement, in this process
    python tools/grad_accum_bench.py accum 1|2|4

(a) views: forward + backward of six views (2 x T 300, 4 x T 200, the DINO trainer's multi-crop step) through one
    ``Model``, gradients through 4 L temporaries per backward + autograd's adds against ``direct_grads = "accumulate"``:
    ``small`` = Model(128, 128, 4) at B 16, ``cfg2`` = cfg2's encoder (128 -> 768 x 2 -> 384) at B 64.
(b) accum: a cfg2 training step (B 256, 128 x 500, band-pass + z-score, cosine loss, RMSprop) of ``DistillTrainer`` at
    ``accum_steps`` 1, 2, 4, with the bytes of LSTM workspace each setting holds.

Prints one JSON line per measurement (median ms over the timed iterations after 3 warm-up steps).  The driver form runs
each measurement as a child under its own time limit and stops at the first that fails; it never opens the GPU itself."""
import argparse
import json
import os
import subprocess
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

CHILD_TIMEOUT_S = 240


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


def _workspace_bytes(model):
    from cerebralsignalnetworks_amd.lstm_model import HipLSTM
    return sum(pl.workspace.numel() for m in model.modules() if isinstance(m, HipLSTM) for pl in m.all_plans())


def views(which, iters):
    from cerebralsignalnetworks_amd import Model
    from cerebralsignalnetworks_amd.trainer import FlatGrads
    dev = torch.device("cuda:0")
    B, H, L, D = (16, 128, 4, 128) if which == "small" else (64, 768, 2, 384)
    res = dict(measurement="views", shape=which, B=B, H=H, L=L, views=[300, 300, 200, 200, 200, 200], iters=iters)
    torch.manual_seed(0)
    xs = [torch.randn(B, T, 128, device=dev) for T in res["views"]]
    for mode in (False, "accumulate"):
        torch.manual_seed(1)
        m = Model(input_size=128, lstm_size=H, lstm_layers=L, output_size=D, include_top=False).to(dev)
        grads = FlatGrads(m.parameters())
        m.lstm.direct_grads = mode

        def step():
            grads.zero()
            sum(m(x).square().mean() for x in xs).backward()

        key = "direct_accumulate" if mode else "temporaries"
        res[f"{key}_ms"] = _time(step, iters)
        res["path"] = sorted({pl.path() for pl in m.lstm.all_plans()})
        res["workspace_bytes"] = _workspace_bytes(m)
        del m, grads
        torch.cuda.empty_cache()
    res["saved_pct"] = 100.0 * (1.0 - res["direct_accumulate_ms"] / res["temporaries_ms"])
    return res


def accum(k, iters):
    from cerebralsignalnetworks_amd import Model, EEGFilters
    from cerebralsignalnetworks_amd.trainer import DistillTrainer
    dev = torch.device("cuda:0")
    B, C, T, H, L, D = 256, 128, 500, 768, 2, 384
    torch.manual_seed(0)
    m = Model(input_size=C, lstm_size=H, lstm_layers=L, output_size=D, include_top=False).to(dev)
    tr = DistillTrainer(m, EEGFilters(1000, order=3).sos, loss="cosine", lr=1e-3, optimizer="rmsprop", accum_steps=k)
    eeg, tgt = torch.randn(B, C, T, device=dev), torch.randn(B, D, device=dev)
    ms = _time(lambda: tr.train_step(eeg, tgt), iters)
    tr.check_device_status()
    return dict(measurement="accum", accum_steps=k, B=B, micro_batch=B // k, iters=iters, ms_per_step=ms,
                workspace_bytes=_workspace_bytes(m), path=sorted({pl.path() for pl in m.lstm.all_plans()}))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("what", nargs="?", default="all", choices=["all", "views", "accum"])
    ap.add_argument("arg", nargs="?", default=None)
    ap.add_argument("--iters", type=int, default=10)
    args = ap.parse_args()
    if args.what == "views":
        print(json.dumps(views(args.arg or "small", args.iters)), flush=True)
    elif args.what == "accum":
        print(json.dumps(accum(int(args.arg or 1), args.iters)), flush=True)
    else:
        # one fresh process per measurement, each under its own time limit; the first failure ends the run
        for child in (["views", "small"], ["views", "cfg2"], ["accum", "1"], ["accum", "2"], ["accum", "4"]):
            rc = subprocess.run(["timeout", "-k", "10", str(CHILD_TIMEOUT_S), sys.executable, os.path.abspath(__file__), *child,
                                 "--iters", str(args.iters)]).returncode
            if rc != 0:
                sys.exit(f"grad_accum_bench: {' '.join(child)} ended with status {rc}; nothing further was started")


if __name__ == "__main__":
    main()
