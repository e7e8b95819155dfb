"""What a bidirectional LSTM stack costs on a training step's forward + backward:

    python tools/bilstm_bench.py [--out profiles/bilstm_bench.json] [--reps 20]

Legs, per shape, on the same inputs and parameter values, output gradient on every step of the top layer and the input
gradient asked for:
  (a) BiLSTM(I, H, L): a plain and a CSN_LSTM_REVERSE single-layer plan per layer, the halves of each layer's [B,T,2H]
      output written and its gradient read in place, the second direction's dx added to the first's;
  (b) the same network as it has to be composed without BiLSTM: 2L single-layer LSTM modules, torch.flip, torch.cat, and
      autograd's sum of the two input gradients -- this leg runs none of the reverse / pitch / add code, it is the yardstick;
  (c) the unidirectional LSTM(I, H, L), for scale;
  (a_ragged) leg (a) with per-row lengths uniform in [T/2, T] (leg (b) cannot express them: torch.flip reverses the padding
      into the front of a row).
Timing: one pair of device events around one forward + backward, the legs alternating sample by sample in one process
after a warm-up of all of them; per leg the median over the repetitions, min / max and the interquartile range.  The
spread of a leg is max - min.  Needs a GPU: there is no fallback."""
import argparse
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from tools.l2_topk_bench import csrc_sha16      # noqa: E402

# (name, B, T, I, H, L): the LSTM shapes of bench.py --config cfg2 / cfg4
CASES = [("cfg2", 256, 500, 128, 768, 2), ("cfg4", 256, 440, 128, 1024, 2)]
NAMES = ("weight_ih", "weight_hh", "bias_ih", "bias_hh")


def _stats(ms):
    q = statistics.quantiles(ms, n=4)
    return dict(median_ms=statistics.median(ms), min_ms=min(ms), max_ms=max(ms), iqr_ms=q[2] - q[0], spread_ms=max(ms) - min(ms))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "bilstm_bench.json"))
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--only", default=None, help="substring of the case names to run")
    args = ap.parse_args()
    from cerebralsignalnetworks_amd import cabi, BiLSTM, LSTM
    if not torch.cuda.is_available():
        sys.exit("bilstm_bench: no GPU is visible (there is no fallback)")
    if args.reps < 20:
        sys.exit("bilstm_bench: at least 20 timed repetitions per shape")
    dev = torch.device("cuda:0")
    out = []
    for name, B, T, I, H, L in CASES:
        if args.only and args.only not in name:
            continue
        torch.manual_seed(B + T + H)
        bi = BiLSTM(I, H, L).to(dev)
        sd = bi.state_dict()
        parts = []
        for l in range(L):
            pair = []
            for sfx in ("", "_reverse"):
                m = LSTM(I if l == 0 else 2 * H, H, 1).to(dev)
                m.load_state_dict({f"{n}_l0": sd[f"{n}_l{l}{sfx}"] for n in NAMES})
                pair.append(m)
            parts.append(pair)
        uni = LSTM(I, H, L).to(dev)
        x = torch.randn(B, T, I, device=dev, requires_grad=True)
        dy2, dy1 = torch.randn(B, T, 2 * H, device=dev), torch.randn(B, T, H, device=dev)
        g = torch.Generator().manual_seed(T)
        lengths = torch.randint(T // 2, T + 1, (B,), generator=g).tolist()

        def bilstm(lens=None):
            y, _ = bi(x, lengths=lens)
            y.backward(dy2)
            return y

        def composed():
            inp = x
            for fwd, bwd in parts:
                out_f, _ = fwd(inp)
                out_b, _ = bwd(torch.flip(inp, [1]))
                inp = torch.cat([out_f, torch.flip(out_b, [1])], dim=2)
            inp.backward(dy2)
            return inp

        def unidirectional():
            y, _ = uni(x)
            y.backward(dy1)
            return y

        legs = {"a_bilstm": bilstm, "b_composed": composed, "c_unidirectional": unidirectional,
                "a_bilstm_ragged": lambda: bilstm(lengths)}
        last = {}
        for _ in range(2):                          # warm-up: code objects, plans and workspaces, side streams, event pools
            for n, fn in legs.items():
                last[n] = fn().detach()
        torch.cuda.synchronize()
        ms = {n: [] for n in legs}
        for _ in range(args.reps):
            for n, fn in legs.items():
                x.grad = None
                a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                a.record()
                y = fn()
                b.record()
                b.synchronize()
                ms[n].append(a.elapsed_time(b))
                last[n] = y.detach()
        plans = bi.all_plans() + uni.all_plans() + [pl for pair in parts for m in pair for pl in m.all_plans()]
        res = dict(case=name, B=B, T=T, I=I, H=H, L=L, dtype="bf16", reps=args.reps,
                   bilstm_plans=sorted({(pl.desc.I, pl.reverse, pl.path()) + pl.kernel_names() for pl in bi.all_plans()}),
                   unidirectional_plan=[(pl.path(),) + pl.kernel_names() for pl in uni.all_plans()],
                   bilstm_workspace_bytes=sum(cabi.load().csn_lstm_plan_workspace_bytes(pl._plan) for pl in bi.all_plans()
                                              if pl.desc.T == T),
                   ragged_lengths_mean=sum(lengths) / B, status=sorted({pl.status() for pl in plans}),
                   **{n: _stats(v) for n, v in ms.items()})
        res["a_minus_b_ms"] = res["a_bilstm"]["median_ms"] - res["b_composed"]["median_ms"]
        res["a_not_slower_than_b_by_more_than_its_spread"] = bool(res["a_minus_b_ms"] <= res["b_composed"]["spread_ms"])
        res["a_over_c"] = res["a_bilstm"]["median_ms"] / res["c_unidirectional"]["median_ms"]
        res["a_bit_equal_b"] = bool(torch.equal(last["a_bilstm"], last["b_composed"]))
        print(json.dumps(res), flush=True)
        out.append(res)
        del bi, parts, uni, plans, last, x
        torch.cuda.empty_cache()
    result = dict(tool="tools/bilstm_bench.py", device=torch.cuda.get_device_name(0), csrc_sha16=csrc_sha16(), cases=out)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
