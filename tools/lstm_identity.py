"""A/B identity of the LSTM entry points: the parent commit's library against this tree's, bit for bit.

    python tools/lstm_identity.py --parent-lib cerebralsignalnetworks_amd/lib/libcsn_abl_parent.so --parent-sha16 <sha> \
        [--out profiles/lstm_boundary_identity.json]

For a refactor of host code or of the layout passes that must change no result.  The parent library is built on the build
machine from a `git worktree` of the parent commit and copied to cerebralsignalnetworks_amd/lib/libcsn_abl_parent.so
(git-ignored, as tools/abl_build.sh documents for its libraries); --parent-sha16 is csrc_sha16 of that worktree's sources.

Per case one forward and one backward with every output and gradient the plan gives (y_all, y_last, h_n, c_n, dx, dh0, dc0,
the parameter gradients), once on each library.  Compared: every tensor with torch.equal (and, reported beside it, bit for
bit -- torch.equal does not tell a zero's sign), the four counts of csn_lstm_profile_read, the status word and
(path, kernel names).  Cases:
  * boundary: B=3 T=5 I=4 H=32 L=1, path 0, bf16 and float32, the full product of lengths {none, [T]*B, [T,0,2]}, reverse,
    y_all pitch {dense, H+4}, dy_all pitch {dense, H+4}, dx_add, output dropout p {0, 0.5}: 192 calls, the caller's y_all
    and dx pre-filled (the whole pitched buffers are compared, gaps included);
  * one plan per path 0-5 at a shape of the test tables (tests/test_gpu_lstm_state.py CASES, tests/test_gpu_bilstm.py
    PLAN_CASES, tests/test_gpu_lstm_resident.py), each with and without lengths where the plan takes them.
CSN_LIB_PATH and the diagnostic switches are read when the package is imported / a plan is created, so a library runs the
cases that share an environment in ONE fresh child process (fresh children only: a process that has touched the GPU never
replaces its program), each child under a `timeout` of its own; the parent stops at the first child that does not exit 0.
Needs a GPU: there is no fallback."""
import argparse
import itertools
import json
import os
import subprocess
import sys
import tempfile

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

NAMES = ("weight_ih", "weight_hh", "bias_ih", "bias_hh")
DTYPES = {"bf16": torch.bfloat16, "f32": torch.float32}
GAP = 4


def _ragged(B, T):
    g = torch.Generator().manual_seed(B * 100 + T)
    n = torch.randint(0, T + 1, (B,), generator=g).tolist()
    n[0], n[B - 1] = T, 0
    return n


def cases():
    out = []
    Bb, Tb = 3, 5
    lens = {"none": None, "full": [Tb] * Bb, "ragged": [Tb, 0, 2]}
    for dt, ln, rev, yg, dyg, add, p in itertools.product(DTYPES, lens, (0, 1), (0, GAP), (0, GAP), (0, 1), (0.0, 0.5)):
        out.append(dict(name=f"boundary_{dt}_{ln}_rev{rev}_y{yg}_dy{dyg}_add{add}_p{p}", shape=(Bb, Tb, 4, 32, 1), dtype=dt, env={},
                        state=True, reverse=bool(rev), resident=False, lengths=lens[ln], y_gap=yg, dy_gap=dyg, add=bool(add), p=p))
    paths = [("path0_v1_h96", (8, 40, 24, 96, 2), "bf16", {}, True, False),
             ("path1_p1_l5", (8, 30, 16, 128, 5), "bf16", {}, True, False),
             ("path2_nopersist_bwd", (64, 40, 128, 768, 2), "bf16", {"CSN_NO_PERSIST_BWD": "1"}, True, False),
             ("path3_chunk4_l3", (64, 23, 32, 256, 3), "bf16", {"CSN_LSTM_CHUNK": "4"}, True, False),
             ("path4_f32_stateless", (64, 9, 32, 128, 2), "f32", {}, False, False),
             ("path5_res_l5_chunk2", (5, 11, 8, 96, 5), "bf16", {"CSN_LSTM_CHUNK": "2"}, True, True)]
    for name, shape, dt, env, state, resident in paths:
        for with_len in ((False, True) if state else (False,)):
            out.append(dict(name=name + ("_lengths" if with_len else ""), shape=shape, dtype=dt, env=env, state=state, reverse=False,
                            resident=resident, lengths=_ragged(shape[0], shape[1]) if with_len else None, y_gap=0, dy_gap=0, add=False, p=0.0))
    return out


def _pattern(shape, base, dev):
    n = 1
    for s in shape:
        n *= s
    return (base + 1.0 + torch.arange(n, dtype=torch.float32)).reshape(shape).to(dev)


def run_case(c, plans):
    """One forward + backward of case c on the loaded library -> (tensors on the CPU, meta)."""
    from cerebralsignalnetworks_amd import cabi
    dev = torch.device("cuda:0")
    B, T, I, H, L = c["shape"]
    key = (tuple(c["shape"]), c["dtype"], c["state"], c["reverse"], c["resident"])
    if key not in plans:
        plans[key] = cabi.LstmPlan(B, T, I, H, L, DTYPES[c["dtype"]], dev, training=True, state=c["state"], reverse=c["reverse"],
                                   resident=c["resident"])
    plan = plans[key]
    torch.manual_seed(B + H + L)
    ref = torch.nn.LSTM(I, H, L, batch_first=True)
    w = [[getattr(ref, f"{n}_l{k}").detach().to(dev) for k in range(L)] for n in NAMES]
    g = torch.Generator().manual_seed(B + H + L + 1)
    rnd = lambda *shape: torch.randn(*shape, generator=g).to(dev)      # noqa: E731
    x, dy_all, dy_last = rnd(B, T, I), 0.1 * rnd(B, T, H), rnd(B, H)
    h0, c0, dh_n, dc_n = 0.5 * rnd(L, B, H), rnd(L, B, H), rnd(L, B, H), rnd(L, B, H)
    y_buf, dy_buf, dx = _pattern((B, T, H + c["y_gap"]), 1e3, dev), _pattern((B, T, H + c["dy_gap"]), 2e3, dev), _pattern((B, T, I), 3e3, dev)
    dy_buf[:, :, :H] = dy_all
    if c["state"]:
        plan.set_lengths(c["lengths"])
    plan.set_io(H + c["y_gap"] if c["y_gap"] else 0, H + c["dy_gap"] if c["dy_gap"] else 0, c["add"])
    plan.set_output_dropout(c["p"], 0x0123456789ABCDEF, 2, 8, H + 8)
    plan.profile_enable(True)
    t = dict(y_buf=y_buf, dx=dx)
    if c["state"]:
        t["y_last"], _, t["h_n"], t["c_n"] = plan.forward(x, *w, want_state=True, y_all=y_buf[:, :, :H], h0=h0, c0=c0)
        t["dh0"], t["dc0"] = torch.empty(L, B, H, device=dev), torch.empty(L, B, H, device=dev)
        st = dict(dh_n=dh_n, dc_n=dc_n, dh0=t["dh0"], dc0=t["dc0"])
    else:
        t["y_last"], _ = plan.forward(x, *w, y_all=y_buf[:, :, :H])
        st = {}
    grads = [[torch.empty_like(p) for p in group] for group in w]
    plan.backward(dy_last, dy_buf[:, :, :H], grads, dx=dx, **st)
    torch.cuda.synchronize()
    t.update({f"{n}_l{k}": q for n, group in zip(NAMES, grads) for k, q in enumerate(group)})
    prof = plan.profile_read()
    plan.profile_enable(False)
    meta = dict(plan=[plan.path()] + list(plan.kernel_names()), status=plan.status(),
                profile_counts=[prof[k] for k in ("fwd_launches", "fwd_cells", "bwd_launches", "bwd_cells")])
    return {k: v.cpu() for k, v in t.items()}, meta


def child(args):
    if not torch.cuda.is_available():
        sys.exit("lstm_identity: no GPU is visible (there is no fallback)")
    env = json.loads(args.child)
    plans, res = {}, {}
    for c in cases():
        if c["env"] == env:
            res[c["name"]] = run_case(c, plans)
    torch.save(res, args.out)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "lstm_boundary_identity.json"))
    ap.add_argument("--parent-lib", default=None, help="libcsn_hip.so built from the parent commit")
    ap.add_argument("--parent-sha16", default=None, help="csrc_sha16 of the parent commit's sources")
    ap.add_argument("--child-timeout", type=int, default=240, help="seconds per child process")
    ap.add_argument("--child", default=None, help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.child is not None:
        return child(args)
    if args.parent_lib is None or not os.path.exists(args.parent_lib):
        sys.exit("lstm_identity: --parent-lib must name the parent commit's library")
    from tools.l2_topk_bench import csrc_sha16
    todo = cases()
    envs = []
    for c in todo:
        if c["env"] not in envs:
            envs.append(c["env"])
    got = {"parent": {}, "this": {}}
    with tempfile.TemporaryDirectory() as tmp:
        for i, env in enumerate(envs):
            for lib in ("parent", "this"):
                e = dict(os.environ, **env)
                e.pop("CSN_LIB_PATH", None)
                if lib == "parent":
                    e["CSN_LIB_PATH"] = os.path.abspath(args.parent_lib)
                path = os.path.join(tmp, f"{lib}_{i}.pt")
                cmd = ["timeout", "-k", "10", str(args.child_timeout), sys.executable, os.path.abspath(__file__), "--child", json.dumps(env),
                       "--out", path]
                rc = subprocess.run(cmd, env=e, cwd=ROOT).returncode
                if rc != 0:
                    sys.exit(f"lstm_identity: the {lib} child of environment {env} exited {rc}; nothing further was started")
                got[lib].update(torch.load(path))
                print(f"environment {env}: {lib} done", flush=True)
    rows = []
    for c in todo:
        (tp, mp), (tt, mt) = got["parent"][c["name"]], got["this"][c["name"]]
        differ = [k for k in tp if not torch.equal(tp[k], tt[k])]
        zero_sign = [k for k in tp if k not in differ and not torch.equal(tp[k].view(torch.int32), tt[k].view(torch.int32))]
        row = dict(case=c["name"], shape=list(c["shape"]), dtype=c["dtype"], env=c["env"], state=c["state"], reverse=c["reverse"],
                   resident=c["resident"], lengths=c["lengths"], y_all_pitch=c["shape"][3] + c["y_gap"], dy_all_pitch=c["shape"][3] + c["dy_gap"],
                   dx_add=c["add"], output_dropout_p=c["p"], tensors=len(tp), tensors_differ=differ, equal_but_for_the_sign_of_a_zero=zero_sign,
                   identical=not differ and set(tp) == set(tt) and mp == mt, **mt)
        if mp != mt:
            row["parent"] = mp
        rows.append(row)
        if not row["identical"] or zero_sign:
            print(json.dumps(row), flush=True)
    result = dict(tool="tools/lstm_identity.py: one forward + backward per case on the parent commit's library and on this tree's, fresh "
                       "processes; every output and gradient compared with torch.equal, the four counts of csn_lstm_profile_read, the "
                       "status word and (path, kernel names) compared",
                  device=torch.cuda.get_device_name(0) if torch.cuda.is_available() else None,
                  csrc_sha16=dict(parent=args.parent_sha16, this=csrc_sha16()), all_identical=all(r["identical"] for r in rows),
                  n_cases=len(rows), cases=rows)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")
    print(f"{len(rows)} cases, all identical: {result['all_identical']}")
    return 0 if result["all_identical"] else 1


if __name__ == "__main__":
    sys.exit(main())
