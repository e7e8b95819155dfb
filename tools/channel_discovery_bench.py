"""What the per-channel form of greedy channel discovery (csn_chan_l2_dist once, then csn_chan_l2_select /
csn_chan_l2_accumulate per round: DESIGN.md section 17) costs against what the library offered before it for the same job:
per candidate, cabi.l2_topk on a device-resident gathered feature matrix [N, Tw * (m+1)].

    python tools/channel_discovery_bench.py [--out profiles/channel_discovery_bench.json] [--reps 20]

Per shape, reported separately:
  distance pass    new: csn_chan_l2_dist over all C channels.     baseline: its round 0 (m = 0), one search per channel.
  one round at m   new: csn_chan_l2_select over all C channels    baseline: C - m candidates, each a gather of (m+1) channels
                   with the m fixed channels' sum as base.                  and a search.
  two rounds       new: distance pass + select + accumulate +     baseline: round 0 over C candidates + round 1 over C - 1.
                   select.
The baseline's time includes gathering the feature matrix on the device (index_select + reshape) and excludes every host
copy; it stops at the neighbour indices, while the new form also counts the class hits -- so the comparison favours the
baseline.  Outside the timed windows the neighbour indices of both forms are compared for every candidate of the
one-round measurements (same_neighbours: 1.0 = all equal).  Timing: one pair of device events around every form, the two forms alternating call by call in one process
after a warm-up of both at every shape; reported per form: median, min / max and the interquartile range over the
repetitions.  The winner of round 0 is not looked at: round 1 fixes channel 0 in both forms (the work is the same for
every choice).  Needs a GPU: there is no fallback."""
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

# (name, C, Ng, Nq, T, t0, t1, k, fixed-channel counts m of the one-round measurement)
CASES = [("perils_96ch_1200x1200_w20-480_k5", 96, 1200, 1200, 500, 20, 480, 5, (0, 7)),
         ("spampinato_128ch_1600x400_w20-160_k5", 128, 1600, 400, 440, 20, 160, 5, (0,))]


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


def _compare(fns, reps):
    """{name: fn} -> {name: stats}: warm-up of every form, then the forms alternating call by call."""
    for _ in range(2):
        for fn in fns.values():
            fn()
    torch.cuda.synchronize()
    ms = {n: [] for n in fns}
    for _ in range(reps):
        for n, fn in fns.items():
            ms[n].append(_timed(fn)[0])
    return {n: _stats(v) for n, v in ms.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "channel_discovery_bench.json"))
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--only", default=None, help="substring of the case names to run")
    args = ap.parse_args()
    from cerebralsignalnetworks_amd import cabi
    if not torch.cuda.is_available():
        sys.exit("channel_discovery_bench: no GPU is visible (there is no fallback)")
    if args.reps < 20:
        sys.exit("channel_discovery_bench: at least 20 timed repetitions per shape")
    dev = torch.device("cuda:0")
    cabi.load()
    out = []
    for name, C, Ng, Nq, T, t0, t1, k, ms_fixed in CASES:
        if args.only and args.only not in name:
            continue
        gen = torch.Generator(device="cpu").manual_seed(C + Ng + Nq)
        g = torch.randn(Ng, C, T, generator=gen).to(dev)
        q = torch.randn(Nq, C, T, generator=gen).to(dev)
        gc = torch.randint(0, 40, (Ng,), generator=gen).to(torch.int32).to(dev)
        qc = torch.randint(0, 40, (Nq,), generator=gen).to(torch.int32).to(dev)
        Tw = t1 - t0

        def new_dist():
            return cabi.chan_l2_dist(g, q, t0, t1)

        def new_round(base, Dc):
            return cabi.chan_l2_select(base, Dc, gc, qc, k, want=("hits", "top1"))

        sels = {}                                   # channel-index tensors, uploaded before anything is timed

        def base_one(fixed, ch):
            sel = sels.get((fixed, ch))
            if sel is None:
                sel = sels[(fixed, ch)] = torch.tensor(list(fixed) + [ch], device=dev)
            gf = g.index_select(1, sel)[:, :, t0:t1].reshape(Ng, -1)      # the gather is part of the baseline's job
            qf = q.index_select(1, sel)[:, :, t0:t1].reshape(Nq, -1)
            return cabi.l2_topk(gf, qf, k)

        def base_round(fixed):
            res = None
            for ch in range(C):
                if ch not in fixed:
                    res = base_one(fixed, ch)
            return res

        def same_neighbours(base, Dc, fixed):
            """Share of (candidate, query, rank) entries at which both forms name the same gallery row."""
            idx = cabi.chan_l2_select(base, Dc, None, None, k, want=("idx",))["idx"]
            same = [(idx[ch] == base_one(fixed, ch)[1]).float().mean().item() for ch in range(C) if ch not in fixed]
            return sum(same) / len(same)

        def new_two_rounds():
            Dc = new_dist()
            new_round(None, Dc)
            base = cabi.chan_l2_accumulate(torch.empty_like(Dc[0]), Dc[0], True)
            return new_round(base, Dc)

        def base_two_rounds():
            base_round(())
            return base_round((0,))

        res = dict(case=name, C=C, Ng=Ng, Nq=Nq, T=T, window=[t0, t1], k=k, reps=args.reps,
                   dc_bytes=C * Nq * Ng * 8)
        st = _compare({"new": new_dist, "baseline": lambda: base_round(())}, args.reps)
        st["baseline_over_new"] = st["baseline"]["median_ms"] / st["new"]["median_ms"]
        st["new_pair_dims_per_s"] = C * Ng * Nq * Tw / (st["new"]["median_ms"] * 1e-3)
        res["distance_pass"] = st
        print(json.dumps({name: {"distance_pass": st}}), flush=True)
        Dc = new_dist()
        res["one_round"] = {}
        for m in ms_fixed:
            fixed = tuple(range(m))
            base = None
            for i, ch in enumerate(fixed):
                base = cabi.chan_l2_accumulate(torch.empty_like(Dc[0]) if base is None else base, Dc[ch], i == 0)
            st = _compare({"new": lambda: new_round(base, Dc), "baseline": lambda: base_round(fixed)}, args.reps)
            st["baseline_over_new"] = st["baseline"]["median_ms"] / st["new"]["median_ms"]
            # m = 0: the same chain per pair in both forms, so every neighbour must agree; m > 0: the flat feature sums the
            # same squares in another order, and a near-tie within the reordering bound may resolve differently
            st["same_neighbours"] = same_neighbours(base, Dc, fixed)
            res["one_round"][f"m={m}"] = st
            print(json.dumps({name: {f"one_round m={m}": st}}), flush=True)
        del Dc
        st = _compare({"new": new_two_rounds, "baseline": base_two_rounds}, args.reps)
        st["baseline_over_new"] = st["baseline"]["median_ms"] / st["new"]["median_ms"]
        res["two_rounds"] = st
        print(json.dumps({name: {"two_rounds": st}}), flush=True)
        out.append(res)
        del g, q
        torch.cuda.empty_cache()
    result = dict(tool="tools/channel_discovery_bench.py", device=torch.cuda.get_device_name(0), csrc_sha16=csrc_sha16(),
                  cases=out)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
