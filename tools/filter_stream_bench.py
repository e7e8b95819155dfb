"""What the stateful band-pass (csn_eeg_bandpass_stream, tile-walking scan kernel) costs and saves against the stateless
csn_eeg_bandpass_znorm on the same input:

  (a) 256 x 128 x 500, order 3: both run a chunk scan over one tile per row -- the difference is the price of the carry,
      of left alignment and of one workgroup per 32 rows (against the stateless kernel's two workgroups per CU walking
      row tiles with a prefetch);
  (b) 8 x 128 x 16384 and 1 x 128 x 60000, order 3: T > 512, where the stateless entry point has only its row-walking
      kernel (one lane per row, two passes).  The stream launch has ceil(B C / 32) workgroups: 32 and 4 here.

    python tools/filter_stream_bench.py [--out profiles/eeg_stream_bench.json] [--blocks 9]

Timing: device events around blocks of calls, the two entry points alternating block by block in one process after a
warm-up of both; the calls per block are chosen so that a block lasts about 50 ms; reported: the median over the blocks of
ms per call.  The outputs are not comparable (fixed affine against per-call z-score), so nothing is compared here: the GPU
tests hold both to their references.  Needs a GPU: there is no fallback."""
import argparse
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

CASES = [("a_256x128x500", 256, 128, 500), ("b_8x128x16384", 8, 128, 16384), ("b_1x128x60000", 1, 128, 60000)]
ORDER = 3


def _block(fn, n):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(n):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / n


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "eeg_stream_bench.json"))
    ap.add_argument("--blocks", type=int, default=9)
    args = ap.parse_args()
    from cerebralsignalnetworks_amd import cabi, EEGFilters
    from oracle import eeg_filter
    if not torch.cuda.is_available():
        sys.exit("filter_stream_bench: no GPU is visible (there is no fallback)")
    dev = torch.device("cuda:0")
    sos = EEGFilters(1000, order=ORDER).sos
    out = []
    for name, B, C, T in CASES:
        x = torch.from_numpy(eeg_filter.synthetic_eeg(B, C, T, seed=5)).to(dev)
        state = torch.zeros(B, C, ORDER, 2, dtype=torch.float64, device=dev)
        assert cabi.eeg_bandpass_stream_path(x, ORDER) == 1

        def stream():
            cabi.eeg_bandpass_stream(x, sos, state_in=None, state_out=state)

        def znorm():
            cabi.eeg_bandpass_znorm(x, sos)

        for fn in (stream, znorm):                  # warm-up: code objects, allocator
            for _ in range(3):
                fn()
        torch.cuda.synchronize()
        n = {fn.__name__: max(3, min(400, int(50.0 / max(_block(fn, 2), 1e-3)))) for fn in (stream, znorm)}
        ms = {"stream": [], "znorm": []}
        for _ in range(args.blocks):
            for fn in (stream, znorm):
                ms[fn.__name__].append(_block(fn, n[fn.__name__]))
        res = dict(case=name, B=B, C=C, T=T, order=ORDER, stream_workgroups=-(-B * C // 32),
                   znorm_kernel="scan" if T <= 512 else "rows", calls_per_block=n, blocks=args.blocks,
                   stream_ms=statistics.median(ms["stream"]), znorm_ms=statistics.median(ms["znorm"]),
                   stream_ms_min_max=[min(ms["stream"]), max(ms["stream"])],
                   znorm_ms_min_max=[min(ms["znorm"]), max(ms["znorm"])])
        res["znorm_over_stream"] = res["znorm_ms"] / res["stream_ms"]
        res["stream_gb_per_s"] = B * C * T * 8 / (res["stream_ms"] * 1e-3) / 1e9       # 4 bytes read + 4 written per sample
        print(json.dumps(res), flush=True)
        out.append(res)
    result = dict(tool="tools/filter_stream_bench.py", device=torch.cuda.get_device_name(0), cases=out)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
