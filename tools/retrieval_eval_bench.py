"""What the retrieval evaluation leg costs on the host form (retrieval.evaluate_full on host inputs: upload, search,
download, the Python bookkeeping) against the device form (retrieval.evaluate_device on device-resident embeddings: search,
csn_topk_class_metrics, a few hundred bytes back, retrieval._fold_counts), and retrieval.merge_topk against csn_topk_merge
(DESIGN.md section 22).

    python tools/retrieval_eval_bench.py [--out profiles/retrieval_eval_bench.json] [--reps 20]

Per shape three forms alternate call by call, after a warm-up of all of them: "host" (numpy embeddings, label dicts),
"device" (device embeddings, the same label dicts -- what the CLIs pass with --device_eval) and "device_ids" (device
embeddings, device int32 class ids: no per-label Python at all).  Timing is wall clock around the call and a final
synchronise, since the host part is the point; reported per form: median, min / max and the interquartile range over
the repetitions.  The device form's search and metrics kernels are also timed on their own ("split"), each between
synchronisations.  Outside the timed windows the tool checks that all forms return equal floats, class scores and I.
The merge is timed the same way at 8 parts x 4096 queries x 64, k = 64, on host arrays against device tensors.
Labels are random over 40 classes.  Needs a GPU: there is no fallback."""
import argparse
import glob
import hashlib
import json
import os
import statistics
import sys
import time
from types import SimpleNamespace

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

# (name, Ng, Nq, D, k)
CASES = [("32768x4096x768_k5", 32768, 4096, 768, 5), ("32768x4096x768_k64", 32768, 4096, 768, 64),
         ("2048x512x768_k5", 2048, 512, 768, 5)]
MERGE = (8, 4096, 64, 64)            # parts, queries, k_in, k
N_CLASSES = 40


def csrc_sha16():
    """The kernel-source fingerprint, computed as bench.py computes it."""
    h = hashlib.sha256()
    d = os.path.join(ROOT, "cerebralsignalnetworks_amd", "csrc")
    for f in sorted(glob.glob(os.path.join(d, "*.hip")) + glob.glob(os.path.join(d, "*.h"))):
        h.update(os.path.basename(f).encode())
        h.update(open(f, "rb").read())
    return h.hexdigest()[:16]


def _timed(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    r = fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3, r


def _stats(ms):
    q = statistics.quantiles(ms, n=4)
    return dict(median_ms=statistics.median(ms), min_ms=min(ms), max_ms=max(ms), iqr_ms=q[2] - q[0])


def _compare(fns, reps):
    """{name: fn} -> {name: stats}: warm-up of every form, then the forms alternating call by call."""
    for _ in range(2):
        for fn in fns.values():
            fn()
    ms = {n: [] for n in fns}
    for _ in range(reps):
        for n, fn in fns.items():
            ms[n].append(_timed(fn)[0])
    return {n: _stats(v) for n, v in ms.items()}


class _Dataset:
    def __init__(self, n):
        self.class_id_to_str = {c: f"class_{c}" for c in range(n)}
        self.class_str_to_id = {f"class_{c}": c for c in range(n)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "retrieval_eval_bench.json"))
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--only", default=None, help="substring of the case names to run ('merge' for the merge alone)")
    args = ap.parse_args()
    from cerebralsignalnetworks_amd import cabi, retrieval
    if not torch.cuda.is_available():
        sys.exit("retrieval_eval_bench: no GPU is visible (there is no fallback)")
    if args.reps < 20:
        sys.exit("retrieval_eval_bench: at least 20 timed repetitions per shape")
    dev = torch.device("cuda:0")
    cabi.load()
    ds = _Dataset(N_CLASSES)
    out = []
    for name, Ng, Nq, D, k in CASES:
        if args.only and args.only not in name:
            continue
        rng = np.random.default_rng(Ng + Nq + k)
        gal = rng.standard_normal((Ng, D), dtype=np.float32)
        qry = rng.standard_normal((Nq, D), dtype=np.float32)
        g_cls, q_cls = rng.integers(0, N_CLASSES, Ng), rng.integers(0, N_CLASSES, Nq)
        glab = [{"ClassId": int(c), "ClassName": f"class_{int(c)}", "imagenetClassId": str(int(c))} for c in g_cls]
        qlab = [{"ClassId": int(c), "ClassName": f"class_{int(c)}", "imagenetClassId": str(int(c))} for c in q_cls]
        g_d, q_d = torch.from_numpy(gal).to(dev), torch.from_numpy(qry).to(dev)
        gc_d, qc_d = (torch.from_numpy(c.astype(np.int32)).to(dev) for c in (g_cls, q_cls))
        flags = SimpleNamespace(topK=k)
        forms = {"host": lambda: retrieval.evaluate_full(flags, gal, qry, glab, qlab, ds),
                 "device": lambda: retrieval.evaluate_device(flags, g_d, q_d, glab, qlab, ds),
                 "device_ids": lambda: retrieval.evaluate_device(flags, g_d, q_d, gc_d, qc_d, ds)}
        st = _compare(forms, args.reps)
        for n in ("device", "device_ids"):
            st[f"host_over_{n}"] = st["host"]["median_ms"] / st[n]["median_ms"]
        # outside the timed windows: the same floats, class scores and neighbours from every form
        want = forms["host"]()
        same = True
        for n in ("device", "device_ids"):
            got = forms[n]()
            same = same and all(got[key] == want[key] for key in ("Recall_Total", "Precision_Total", "top1", "class_scores"))
            same = same and bool(torch.equal(got["I"].cpu(), torch.from_numpy(want["I"])))
        st["forms_agree"] = same
        I_d = retrieval.l2_search_device(g_d, q_d, k)[1]
        st["split"] = _compare({"search": lambda: retrieval.l2_search_device(g_d, q_d, k),
                                "metrics": lambda: cabi.topk_class_metrics(I_d, gc_d, qc_d, N_CLASSES,
                                                                           want=("pred", "class", "top1_correct"))}, args.reps)
        res = dict(case=name, Ng=Ng, Nq=Nq, D=D, k=k, n_classes=N_CLASSES, reps=args.reps, **st)
        print(json.dumps(res), flush=True)
        out.append(res)
        del g_d, q_d
        torch.cuda.empty_cache()
    merge = None
    if not args.only or args.only in "merge":
        P, Nq, k_in, k = MERGE
        rng = np.random.default_rng(P + Nq + k_in)
        Dp = np.sort(rng.random((P, Nq, k_in)), axis=2)
        Ip = np.argsort(rng.random((P, Nq, k_in)), axis=2) + 1000 * np.arange(P)[:, None, None]
        Dp_d, Ip_d = torch.from_numpy(Dp).to(dev), torch.from_numpy(Ip).to(dev)
        st = _compare({"host": lambda: retrieval.merge_topk(list(Dp), list(Ip), k),
                       "device": lambda: retrieval.merge_topk_device(Dp_d, Ip_d, k)}, args.reps)
        st["host_over_device"] = st["host"]["median_ms"] / st["device"]["median_ms"]
        want_d, want_i = retrieval.merge_topk(list(Dp), list(Ip), k)
        got_d, got_i = retrieval.merge_topk_device(Dp_d, Ip_d, k)
        st["forms_agree"] = bool(torch.equal(got_i.cpu(), torch.from_numpy(want_i))
                                 and torch.equal(got_d.cpu(), torch.from_numpy(want_d)))
        merge = dict(case=f"merge_{P}x{Nq}x{k_in}_k{k}", parts=P, Nq=Nq, k_in=k_in, k=k, reps=args.reps, **st)
        print(json.dumps(merge), flush=True)
    result = dict(tool="tools/retrieval_eval_bench.py", device=torch.cuda.get_device_name(0), csrc_sha16=csrc_sha16(),
                  timing="wall clock around the call and a final synchronise, forms alternating, ms", cases=out, merge=merge)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")
    if not all(c["forms_agree"] for c in out) or (merge and not merge["forms_agree"]):
        sys.exit("retrieval_eval_bench: the forms disagree")


if __name__ == "__main__":
    main()
