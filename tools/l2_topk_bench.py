"""What the tiled exact L2 top-k (csn_l2_topk_tiled: register-tiled distances, selection fused behind the tile, no
distance matrix) costs against csn_l2_topk (the [Nq,Ng] float64 matrix, then k arg-min rounds over every row) on the same
inputs, and what it does where the old entry point cannot run (k > 64, a matrix above the budget):

    python tools/l2_topk_bench.py [--out profiles/l2_topk_tiled_bench.json] [--reps 20]

Timing: one pair of device events around every call, the two entry points alternating call by call in one process after a
warm-up of both at every shape; reported per entry point: the median over the repetitions, min / max and the
interquartile range (the run-to-run spread the comparison is held against).  At every shape both can run, the two results
are compared bit for bit (idx and float32 dist).  Rates are pair-dimensions per second, Ng * Nq * D / time: one float64
subtract and one fma each.  Needs a GPU: there is no fallback."""
import argparse
import glob
import hashlib
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

# (name, Ng, Nq, D, k, old entry point can run)
CASES = [("acceptance_2048x512x768_k5", 2048, 512, 768, 5, True),
         ("32768x4096x768_k5", 32768, 4096, 768, 5, True),
         ("32768x4096x768_k64", 32768, 4096, 768, 64, True),
         ("32768x4096x768_k256", 32768, 4096, 768, 256, False),
         ("262144x2048x384_k10", 262144, 2048, 384, 10, False)]


def csrc_sha16():
    """The kernel-source fingerprint, computed as bench.py computes it."""
    h = hashlib.sha256()
    d = os.path.join(ROOT, "cerebralsignalnetworks_amd", "csrc")
    for f in sorted(glob.glob(os.path.join(d, "*.hip")) + glob.glob(os.path.join(d, "*.h"))):
        h.update(os.path.basename(f).encode())
        h.update(open(f, "rb").read())
    return h.hexdigest()[:16]


def _timed(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    r = fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b), r


def _stats(ms):
    q = statistics.quantiles(ms, n=4)
    return dict(median_ms=statistics.median(ms), min_ms=min(ms), max_ms=max(ms), iqr_ms=q[2] - q[0])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "l2_topk_tiled_bench.json"))
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--only", default=None, help="substring of the case names to run")
    args = ap.parse_args()
    from cerebralsignalnetworks_amd import cabi
    if not torch.cuda.is_available():
        sys.exit("l2_topk_bench: no GPU is visible (there is no fallback)")
    if args.reps < 20:
        sys.exit("l2_topk_bench: at least 20 timed repetitions per shape")
    dev = torch.device("cuda:0")
    lib = cabi.load()
    out = []
    for name, Ng, Nq, D, k, both in CASES:
        if args.only and args.only not in name:
            continue
        gen = torch.Generator(device="cpu").manual_seed(Ng + Nq + k)
        g = torch.randn(Ng, D, generator=gen).to(dev)
        q = torch.randn(Nq, D, generator=gen).to(dev)
        fns = {"tiled": lambda: cabi.l2_topk_tiled(g, q, k)}
        if both:
            fns["old"] = lambda: cabi.l2_topk(g, q, k)
        last = {}
        for _ in range(3):                          # warm-up: code objects, allocator
            for n, fn in fns.items():
                last[n] = fn()
        torch.cuda.synchronize()
        ms = {n: [] for n in fns}
        for _ in range(args.reps):
            for n, fn in fns.items():
                t, last[n] = _timed(fn)
                ms[n].append(t)
        res = dict(case=name, Ng=Ng, Nq=Nq, D=D, k=k, reps=args.reps,
                   tiled=_stats(ms["tiled"]), tiled_scratch_bytes=lib.csn_l2_topk_tiled_scratch_bytes(Ng, Nq, k),
                   matrix_scratch_bytes=lib.csn_l2_topk_scratch_bytes(Ng, Nq))
        res["tiled"]["pair_dims_per_s"] = Ng * Nq * D / (res["tiled"]["median_ms"] * 1e-3)
        if both:
            res["old"] = _stats(ms["old"])
            res["old"]["pair_dims_per_s"] = Ng * Nq * D / (res["old"]["median_ms"] * 1e-3)
            res["old_over_tiled"] = res["old"]["median_ms"] / res["tiled"]["median_ms"]
            res["bit_equal"] = bool(torch.equal(last["tiled"][1], last["old"][1]) and
                                    torch.equal(last["tiled"][0], last["old"][0]))
        else:
            res["old"] = None
            res["bit_equal"] = None                 # the old entry point refuses this shape: nothing to compare
        print(json.dumps(res), flush=True)
        out.append(res)
        del g, q, last
        torch.cuda.empty_cache()
    result = dict(tool="tools/l2_topk_bench.py", device=torch.cuda.get_device_name(0), csrc_sha16=csrc_sha16(), cases=out)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
