"""What the CU-resident LSTM recurrence (CSN_LSTM_RESIDENT plans, path 5) buys at the small shapes
the reference's own scripts build:

    python tools/lstm_resident_bench.py --baseline-lib /path/to/parent/libcsn_hip.so [--out profiles/lstm_resident_bench.json]

Shapes (B, T, C, H, L): Model(96, 96, 2, include_top) and Model(128, 128, 4) at B 16 and at B 256, Model(96, 128, 4) at B 16,
T 460, in bf16 and in float32.  Per shape and dtype, two workloads:
  lstm     forward + backward of the HipLSTM alone (y_last and its gradient), `--inner` of them per sample;
  trainer  one DistillTrainer.train_step (band-pass + z-score, model, loss, optimiser): featdist + rmsprop for the
           include_top shape, kd + adamw for the others.
and three legs:
  plain_parent   the plan without the bit on the PARENT commit's library (--baseline-lib, selected with CSN_LIB_PATH),
  plain          the plan without the bit on this tree's library,
  resident       resident=True on this tree's library.
CSN_LIB_PATH is read when the package is imported, so every library runs in a child process of its own (fresh children,
`--rounds` of them per library, alternating); inside the child of this tree's library the plain and the resident leg
alternate sample by sample.  A sample is one pair of device events around its work, ended by a synchronise; per leg the
median, min, max and interquartile range over all samples of all rounds are kept, and the spread is max - min.  The
recurrence launches and cells of each plan come from csn_lstm_profile_read in one extra, untimed pass; path 0 keeps no
profile, its launches are the count its host loop makes, T + chunk (L - 1) per pass with chunk = 32 (marked "counted").
Needs a GPU: there is no fallback."""
import argparse
import json
import os
import statistics
import subprocess
import sys
import types

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

# (name, B, T, C, H, L, include_top)
SHAPES = [("perils_b16", 16, 460, 96, 96, 2, True), ("spampinato_b16", 16, 460, 128, 128, 4, False),
          ("eval_b16", 16, 460, 96, 128, 4, False), ("perils_b256", 256, 460, 96, 96, 2, True),
          ("spampinato_b256", 256, 460, 128, 128, 4, False)]
DTYPES = {"bf16": torch.bfloat16, "f32": torch.float32}


def _stats(ms):
    q = statistics.quantiles(ms, n=4)
    return dict(n=len(ms), median_ms=statistics.median(ms), min_ms=min(ms), max_ms=max(ms), iqr_ms=q[2] - q[0], spread_ms=max(ms) - min(ms))


def _timed(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b)


def child(args):
    """One library (the one CSN_LIB_PATH names, else this tree's): JSON lines, one per (shape, dtype)."""
    from cerebralsignalnetworks_amd import cabi, Model, EEGFilters
    from cerebralsignalnetworks_amd.lstm_model import HipLSTM
    from cerebralsignalnetworks_amd.trainer import DistillTrainer
    if not torch.cuda.is_available():
        sys.exit("lstm_resident_bench: no GPU is visible (there is no fallback)")
    dev = torch.device("cuda:0")
    leg_names = ["plain"] if args.child == "parent" else ["plain", "resident"]
    sos = EEGFilters(1000, order=3).sos
    for name, B, T, C, H, L, top in SHAPES:
        if args.only and args.only not in name:
            continue
        for dname, dtype in DTYPES.items():
            torch.manual_seed(B + H + L)
            x = torch.randn(B, T, C, device=dev)
            dy = torch.randn(B, H, device=dev)
            eeg, tgt = torch.randn(B, C, T, device=dev), torch.randn(B, 384, device=dev)
            lab = torch.randint(0, 40, (B,), device=dev)
            lstms, trainers = {}, {}
            for leg in leg_names:
                kw = dict(resident=True) if leg == "resident" else {}
                torch.manual_seed(1)
                lstms[leg] = HipLSTM(C, H, L, compute_dtype=dtype, **kw).to(dev)
                torch.manual_seed(2)
                m = Model(C, H, L, 384, top, compute_dtype=dtype, **kw).to(dev)
                trainers[leg] = (DistillTrainer(m, sos, loss="featdist", optimizer="rmsprop") if top else
                                 DistillTrainer(m, sos, loss="kd", optimizer="adamw", lr=1e-4,
                                                kd_params=types.SimpleNamespace(alpha=0.5, temperature=2.0)))

            def lstm_pass(leg):
                for _ in range(args.inner):
                    for p in lstms[leg].parameters():
                        p.grad = None
                    lstms[leg](x).backward(dy)

            def step(leg):
                trainers[leg].train_step(eeg, tgt, lab, 25)

            for _ in range(2):                  # warm-up: code objects, plans and workspaces, optimiser state
                for leg in leg_names:
                    lstm_pass(leg)
                    step(leg)
            torch.cuda.synchronize()
            ms = {(w, leg): [] for w in ("lstm", "trainer") for leg in leg_names}
            for _ in range(args.reps):
                for leg in leg_names:
                    ms["lstm", leg].append(_timed(lambda: lstm_pass(leg)) / args.inner)
                    ms["trainer", leg].append(_timed(lambda: step(leg)))
            res = dict(lib=args.child, shape=name, B=B, T=T, C=C, H=H, L=L, include_top=top, dtype=dname, inner=args.inner)
            for leg in leg_names:
                plans = lstms[leg].all_plans()
                assert len(plans) == 1
                plans[0].profile_enable(True)
                lstm_pass(leg)
                torch.cuda.synchronize()
                prof = plans[0].profile_read()
                plans[0].profile_enable(False)
                tr_plans = trainers[leg].model.lstm.all_plans()
                counted = plans[0].path() == 0
                if counted:
                    n = T + 32 * (L - 1)
                    prof = dict(fwd_launches=n, bwd_launches=n, fwd_cells=T * L, bwd_cells=T * L)
                res[leg] = dict(plan=[plans[0].path()] + list(plans[0].kernel_names()),
                                trainer_plans=sorted({(pl.path(),) + pl.kernel_names() for pl in tr_plans}),
                                recurrence_launches=dict(forward=prof["fwd_launches"], backward=prof["bwd_launches"]),
                                cells=dict(forward=prof["fwd_cells"], backward=prof["bwd_cells"]),
                                launches_from="counted" if counted else "csn_lstm_profile_read",
                                status=sorted({pl.status() for pl in plans + tr_plans}),
                                lstm_ms=ms["lstm", leg], trainer_ms=ms["trainer", leg])
            print("RESULT " + json.dumps(res), flush=True)
            del lstms, trainers
            torch.cuda.empty_cache()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "lstm_resident_bench.json"))
    ap.add_argument("--baseline-lib", default=None, help="libcsn_hip.so built from the parent commit")
    ap.add_argument("--reps", type=int, default=20, help="timed samples per leg and round")
    ap.add_argument("--rounds", type=int, default=2, help="child processes per library, alternating")
    ap.add_argument("--inner", type=int, default=4, help="LSTM forward + backward passes per sample")
    ap.add_argument("--only", default=None, help="substring of the shape names to run")
    ap.add_argument("--child", default=None, choices=["parent", "this"], help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.child:
        return child(args)
    if args.reps < 10 or args.rounds < 1:
        sys.exit("lstm_resident_bench: at least 10 timed samples per round")
    if args.baseline_lib is None or not os.path.exists(args.baseline_lib):
        sys.exit("lstm_resident_bench: --baseline-lib must name the parent commit's library (the comparison is against the "
                 "parent, not against code this tree compiled)")
    from tools.l2_topk_bench import csrc_sha16
    rows = {}
    device = None
    for rnd in range(args.rounds):
        for lib in ("parent", "this"):
            env = dict(os.environ)
            env.pop("CSN_LIB_PATH", None)
            if lib == "parent":
                env["CSN_LIB_PATH"] = os.path.abspath(args.baseline_lib)
            cmd = [sys.executable, os.path.abspath(__file__), "--child", lib, "--reps", str(args.reps), "--inner", str(args.inner)]
            if args.only:
                cmd += ["--only", args.only]
            proc = subprocess.Popen(cmd, env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, cwd=ROOT)
            tail = []
            for ln in proc.stdout:              # (line by line: a long run shows its progress)
                tail = (tail + [ln])[-40:]
                if not ln.startswith("RESULT "):
                    continue
                r = json.loads(ln[7:])
                row = rows.setdefault((r["shape"], r["dtype"]), {k: r[k] for k in ("shape", "B", "T", "C", "H", "L", "include_top", "dtype", "inner")})
                for leg in ("plain", "resident"):
                    if leg not in r:
                        continue
                    key = "plain_parent" if lib == "parent" else leg
                    slot = row.setdefault(key, {k: v for k, v in r[leg].items() if not k.endswith("_ms")})
                    slot.setdefault("lstm_samples", []).extend(r[leg]["lstm_ms"])
                    slot.setdefault("trainer_samples", []).extend(r[leg]["trainer_ms"])
                print(f"round {rnd} {lib}: {r['shape']} {r['dtype']} done", flush=True)
            if proc.wait() != 0:
                sys.exit(f"lstm_resident_bench: the {lib} child failed:\n{''.join(tail)}")
    cases = []
    for row in rows.values():
        for key in ("plain_parent", "plain", "resident"):
            slot = row[key]
            slot["lstm_fwd_bwd"] = _stats(slot.pop("lstm_samples"))
            slot["trainer_step"] = _stats(slot.pop("trainer_samples"))
        for w in ("lstm_fwd_bwd", "trainer_step"):
            base, res = row["plain_parent"][w], row["resident"][w]
            row[f"{w}_parent_over_resident"] = base["median_ms"] / res["median_ms"]
            row[f"{w}_plain_over_parent"] = row["plain"][w]["median_ms"] / base["median_ms"]
            row[f"{w}_resident_faster_beyond_spread"] = bool(base["min_ms"] > res["max_ms"])
        print(json.dumps({k: v for k, v in row.items() if not isinstance(v, dict)}), flush=True)
        cases.append(row)
    if torch.cuda.is_available():
        device = torch.cuda.get_device_name(0)
    result = dict(tool="tools/lstm_resident_bench.py", device=device, csrc_sha16=csrc_sha16(), reps=args.reps, rounds=args.rounds,
                  baseline="parent commit's libcsn_hip.so through CSN_LIB_PATH", cases=cases)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
