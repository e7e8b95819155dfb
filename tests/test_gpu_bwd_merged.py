"""GPU: the merged launch of the weight-stationary LSTM backward against one launch per diagonal.

The chunk diagonals on which every layer is in range run as one launch whose rounds hand the row-major gate gradients and
the input gradients over through chunk-level counters; CSN_BWD_NO_MERGE=1 keeps the kernel boundaries.  The arithmetic of
a step, the hand-off ring and the GEMM tile bodies are the same in both, so every output of the backward must be the same
BITS: dx, (dh0, dc0) and the four gradients of every layer (dw_ih and dw_hh are products of the row-major dgates the
rounds hand over).  Forward + backward run once under each setting, each in a fresh child process (the switch is read when
a plan is created); the status words must read 0 and csn_lstm_plan_bwd_launches must report the launch counts of the
schedule mirrored in tests/test_bwd_merged_cpu.py.  Plans with a final-state gradient, dropout or lengths are never
merged.  Nothing is compared with a tolerance."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CHUNK = 4
I = 32


def _child(case, out_path):
    """Runs in the child process: one forward + backward through the plan API, outputs to an .npz, diagnostics on stdout."""
    sys.path.insert(0, ROOT)
    from cerebralsignalnetworks_amd import cabi
    H, L, B, T = case["H"], case["L"], case["B"], case["T"]
    dev = torch.device("cuda:0")
    g = torch.Generator().manual_seed(case["seed"])
    rnd = lambda *shape, scale=1.0: (torch.randn(*shape, generator=g) * scale).to(dev)
    k = H ** -0.5
    w_ih = [rnd(4 * H, I if l == 0 else H, scale=k) for l in range(L)]
    w_hh = [rnd(4 * H, H, scale=k) for l in range(L)]
    b_ih = [rnd(4 * H, scale=k) for l in range(L)]
    b_hh = [rnd(4 * H, scale=k) for l in range(L)]
    x, dy = rnd(B, T, I), rnd(B, T, H, scale=0.1)
    h0, c0 = rnd(L, B, H, scale=0.5), rnd(L, B, H, scale=0.5)
    dh_n = rnd(L, B, H) if case.get("final_state_grad") else None
    dc_n = rnd(L, B, H) if case.get("final_state_grad") else None
    plan = cabi.LstmPlan(B, T, I, H, L, torch.bfloat16, dev, training=True, state=True, dropout=bool(case.get("dropout")))
    if case.get("dropout"):
        plan.set_dropout(0.25, seed=1234)
    if case.get("lengths"):
        lens = [int(v) for v in np.random.default_rng(case["seed"]).integers(0, T + 1, B)]
        lens[0], lens[1], lens[B - 1] = T, 0, min(T, 5)
        plan.set_lengths(lens)
    plan.forward(x, w_ih, w_hh, b_ih, b_hh, want_all=True, h0=h0, c0=c0, want_state=True)
    grads = [[torch.full_like(p, float("nan")) for p in group] for group in (w_ih, w_hh, b_ih, b_hh)]
    out = dict(dx=torch.full_like(x, float("nan")), dh0=torch.full_like(h0, float("nan")), dc0=torch.full_like(c0, float("nan")))
    plan.backward(None, dy, grads, dx=out["dx"], dh_n=dh_n, dc_n=dc_n, dh0=out["dh0"], dc0=out["dc0"])
    torch.cuda.synchronize()
    for name, group in zip(("dw_ih", "dw_hh", "db_ih", "db_hh"), grads):
        for l, t in enumerate(group):
            out[f"{name}_l{l}"] = t
    np.savez(out_path, **{n: t.cpu().numpy() for n, t in out.items()})
    print(json.dumps(dict(status=plan.status(), launches=plan.bwd_launches(0), merged=plan.bwd_launches(1),
                          kernel=plan.kernel_names()[1])))


def _run(case, env, tmp_path, label):
    out_path = str(tmp_path / f"{label}.npz")
    clean = {k: v for k, v in os.environ.items() if not k.startswith("CSN_") or k == "CSN_LIB_PATH"}
    done = subprocess.run([sys.executable, os.path.abspath(__file__), json.dumps(case), out_path],
                          env={**clean, "CSN_LSTM_CHUNK": str(CHUNK), **env}, capture_output=True, text=True, timeout=300)
    assert done.returncode == 0, (label, done.stdout[-2000:], done.stderr[-4000:])
    info = json.loads(done.stdout.strip().splitlines()[-1])
    with np.load(out_path) as f:
        return {n: torch.from_numpy(f[n]) for n in f.files}, info


def _expected(case, no_merge):
    from test_bwd_merged_cpu import schedule
    launches = schedule(T=case["T"], L=case["L"], H=case["H"], B=case["B"], chunk=CHUNK, no_merge=no_merge,
                        dropout=bool(case.get("dropout")), lengths=bool(case.get("lengths")),
                        dh_n=bool(case.get("final_state_grad")))
    return len([x for x in launches if x["rounds"][0][0]]), sum(x["merged"] for x in launches)


def _both(case, tmp_path):
    got = {}
    for label, env in (("merged", {}), ("apart", {"CSN_BWD_NO_MERGE": "1"})):
        out, info = _run(case, env, tmp_path, label)
        want = _expected(case, no_merge=label == "apart")
        print(f"{case} {label}: {info}, expected (launches, merged diagonals) {want}")
        assert info["status"] == 0, (label, info)
        assert info["kernel"] == "lstm_bwd_persist_kernel", (label, info)
        assert (info["launches"], info["merged"]) == want, (label, info, want)
        got[label] = (out, info)
    assert got["apart"][1]["merged"] == 0
    a, b = got["merged"][0], got["apart"][0]
    assert set(a) == set(b) and len(a) == 3 + 4 * case["L"]
    for n in sorted(a):
        assert torch.isfinite(a[n]).all(), n
        assert torch.equal(a[n], b[n]), (n, int((a[n] != b[n]).sum()), a[n].numel())
    return got["merged"][1]


# H, L, B, T: what the shape covers
CASES = {
    "h768_l2_b256_t22": (768, 2, 256, 22),     # 64-row groups; four merged diagonals; a 2-step tail chunk
    "h768_l2_b64_t22": (768, 2, 64, 22),       # 32-row groups in every launch
    "h384_l3_b128_t30": (384, 3, 128, 30),     # three layers; 20 idle workgroups per XCD
    "h128_l4_b64_t38": (128, 4, 64, 38),       # four layers
    "h768_l2_b130_t22": (768, 2, 130, 22),     # padded tile
}
MERGED_DIAGONALS = {"h768_l2_b256_t22": 4, "h768_l2_b64_t22": 4, "h384_l3_b128_t30": 4, "h128_l4_b64_t38": 4, "h768_l2_b130_t22": 4}


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(CASES))
def test_merged_launch_gives_the_bits_of_one_launch_per_diagonal(name, tmp_path):
    H, L, B, T = CASES[name]
    info = _both(dict(H=H, L=L, B=B, T=T, seed=31), tmp_path)
    nch = -(-T // CHUNK)
    assert info["merged"] == nch - 2 * (L - 1) == MERGED_DIAGONALS[name]
    assert info["launches"] == nch + 2 * (L - 1) - (info["merged"] - 1)


@pytest.mark.gpu
@pytest.mark.parametrize("feature", ["final_state_grad", "dropout", "lengths"])
def test_plans_that_are_never_merged(feature, tmp_path):
    """h0 / c0 with dh_n / dc_n, inter-layer dropout, per-row lengths: something is enqueued between the launches (the dh_n
    term, the mask) or the masked kernel runs -- zero merged diagonals with or without the switch, and equal outputs."""
    info = _both(dict(H=768, L=2, B=130, T=22, seed=33, **{feature: True}), tmp_path)
    assert info["merged"] == 0


if __name__ == "__main__":
    _child(json.loads(sys.argv[1]), sys.argv[2])
