"""A/B identity of the LSTM modules: the parent commit's cerebralsignalnetworks_amd/lstm_model.py against this tree's.

    git show <parent>:cerebralsignalnetworks_amd/lstm_model.py > cerebralsignalnetworks_amd/_lstm_model_parent.py
    python tools/lstm_module_identity.py --parent-module cerebralsignalnetworks_amd/_lstm_model_parent.py \
        --parent-commit <hash> [--out profiles/lstm_module_identity.json]

For a refactor of the Python layer that must change no result and no library call (tools/lstm_identity.py is the same for
the library).  The parent's copy (git-ignored) is imported under a second module name inside the package, so that its
``from . import cabi`` resolves; both modules then run on ONE binding and one library, in one process.  Every case runs once
on each module with equal seeds and equal parameter values; the modules of a kind are reused from case to case, so each
call finds its pooled plans as the case before left them.  The methods of cabi.LstmPlan are wrapped and record, per module:
the plans created (constructor arguments), the order of forward / backward calls over them (a plan is named by its
creation index), per such call the settings in force on that plan (lengths, windows and source shape, dropout triple,
output-dropout tuple, io triple, gradient mode, whether a callback is installed -- whatever order they were set in) and the
shape, dtype, strides and None-ness of every argument (no pointers).  The two records must be equal, and every output and
gradient (outputs, h_n / c_n, dx, dh0 / dc0, every parameter's gradient, the layers the grad_ready_hook saw) equal bit for
bit, compared as integers so that a zero's sign counts.  After every case the status word of every plan the module holds is 0 and none is busy.

Cases (B=3 T=5 I=4 H=32 L=2 in bf16 and float32; B=5 T=11 I=8 H=96 L=2 on resident plans): the entry points of ENTRIES x
{train() with grad, train() under no_grad, eval()} x dropout {0, 0.5} x direct_grads {False, True, "accumulate"} (.grad
pre-filled with a pattern, a hook recording its layers) x inputs requiring grad or not, where each applies; then the
sequences of SEQUENCES.  Needs a GPU: there is no fallback."""
import argparse
import importlib.util
import inspect
import itertools
import json
import os
import sys

import torch
import torch.nn as nn

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

CONFIGS = {"bf16": dict(B=3, T=5, I=4, H=32, L=2, dtype=torch.bfloat16, resident=False),
           "f32": dict(B=3, T=5, I=4, H=32, L=2, dtype=torch.float32, resident=False),
           "resident": dict(B=5, T=11, I=8, H=96, L=2, dtype=torch.bfloat16, resident=True)}
# entry point -> (module kind, form); the forms are the branches of run_entry
ENTRIES = {"hip": ("hip", "last"), "hip_all": ("hip", "all"), "hip_views": ("hip", "views"),
           "lstm": ("lstm", "plain"), "lstm_hx": ("lstm", "hx"), "lstm_ragged": ("lstm", "ragged"), "lstm_views": ("lstm", "views"),
           "lstm_packed": ("lstm", "packed"),
           "bilstm": ("bilstm", "plain"), "bilstm_hx": ("bilstm", "hx"), "bilstm_ragged": ("bilstm", "ragged"),
           "bilstm_views": ("bilstm", "views"), "bilstm_packed": ("bilstm", "packed"),
           "model": ("model", "model"), "model_views": ("model", "model_views"), "model_bi": ("model_bi", "model"),
           "model_bi_views": ("model_bi", "model_views"), "lstmmodel": ("lstmmodel", "model"), "lstmmodel_all": ("lstmmodel_all", "model")}
NO_INPUT_GRAD = ("views", "model_views", "packed")          # forms whose x takes no gradient (or is not a tensor)
DIRECT = ("hip", "lstm", "model", "lstmmodel", "lstmmodel_all")     # kinds whose encoder has direct_grads
SEQUENCES = ("two_outstanding_fifo", "two_outstanding_lifo", "dropped_graph", "refused_then_good", "second_backward")
SETTERS = ("set_lengths", "set_views", "set_dropout", "set_output_dropout", "set_io", "set_grad_mode", "set_grad_callback")


class Recorder:
    """Wraps cabi.LstmPlan for the run; ``log`` is the record of the module under test at the moment."""

    def __init__(self, cabi):
        self.plan_cls, self.log, self.created, self.saved = cabi.LstmPlan, [], {"parent": 0, "this": 0}, {}
        for name in ("__init__", "forward", "backward") + SETTERS:
            self.saved[name] = getattr(self.plan_cls, name)
            setattr(self.plan_cls, name, self._wrap(name, self.saved[name]))

    def restore(self):
        for name, fn in self.saved.items():
            setattr(self.plan_cls, name, fn)

    def start(self, who):
        """Records of ``who`` ("parent" / "this") from here on; plans are numbered per module."""
        self.who, self.log = who, []
        return self.log

    def _wrap(self, name, real):
        sig = inspect.signature(real)
        rec = self

        def call(plan, *a, **kw):
            bound = sig.bind(plan, *a, **kw)
            bound.apply_defaults()
            args = {k: describe(v) for k, v in list(bound.arguments.items())[1:]}
            if name == "__init__":
                real(plan, *a, **kw)
                n = rec.created[rec.who]
                rec.created[rec.who] += 1
                plan._created, plan._settings = n, {}
                rec.log.append(("create", n, args))
                return None
            if name in SETTERS:
                out = real(plan, *a, **kw)
                if name == "set_grad_callback":
                    args = {"installed": bound.arguments["fn"] is not None}
                plan._settings[name] = args
                return out
            rec.log.append((name, plan._created, dict(plan._settings), args))
            return real(plan, *a, **kw)
        return call


def describe(v):
    if isinstance(v, torch.Tensor):
        return ("tensor", tuple(v.shape), str(v.dtype), tuple(v.stride()), bool(v.requires_grad))
    if isinstance(v, (list, tuple)):
        return [describe(u) for u in v]
    if v is None or isinstance(v, (bool, int, float, str)):
        return v
    return str(v)


def bits(t):
    t = t.detach().contiguous().cpu()
    return t.view({1: torch.uint8, 2: torch.int16, 4: torch.int32, 8: torch.int64}[t.element_size()])


def load_parent(path):
    name = "cerebralsignalnetworks_amd._lstm_model_parent"
    spec = importlib.util.spec_from_file_location(name, path)
    mod = importlib.util.module_from_spec(spec)
    sys.modules[name] = mod
    spec.loader.exec_module(mod)
    return mod


def make_module(lm, kind, cfg, dev):
    """One module of ``kind`` from the module file ``lm``; equal seeds give equal parameters on both files."""
    torch.manual_seed(1000 + cfg["H"])
    I, H, L, kw = cfg["I"], cfg["H"], cfg["L"], dict(compute_dtype=cfg["dtype"], resident=cfg["resident"])
    if kind == "hip":
        m = lm.HipLSTM(I, H, L, **kw)
    elif kind == "lstm":
        m = lm.LSTM(I, H, L, **kw)
    elif kind == "bilstm":
        m = lm.BiLSTM(I, H, L, **kw)
    elif kind in ("model", "model_bi"):
        m = lm.Model(I, H, L, 16, True, n_classes=7, bidirectional=kind == "model_bi", **kw)
    else:       # (LSTMModel is given [B, I, T] and reshapes it to [B, T, I])
        m = lm.LSTMModel(I, H, L, 16, number_of_classes=7, all_steps=kind == "lstmmodel_all", **kw)
    return m.to(dev)


def encoder(m):
    return getattr(m, "lstm", m)


def inputs(cfg, form, kind, grad, dev):
    """The tensors of one call, from a generator of their own (the default one draws the dropout seeds)."""
    B, T, I, H, L = (cfg[k] for k in "BTIHL")
    g = torch.Generator().manual_seed(B * 1000 + T)
    rnd = lambda *shape: torch.randn(*shape, generator=g).to(dev)      # noqa: E731
    t = dict(x=rnd(B, I, T) if kind.startswith("lstmmodel") else rnd(B, T, I))
    rows, Bs = 2 * L if kind == "bilstm" else L, B + 1 if form == "views" else B      # (the views forms run B + 1 windows)
    t["h0"], t["c0"] = 0.5 * rnd(rows, Bs, H), rnd(rows, Bs, H)
    for v in t.values():
        v.requires_grad_(grad and form not in NO_INPUT_GRAD)
    return t


def run_entry(m, form, cfg, t):
    """-> the outputs of the entry point, a flat list of tensors."""
    B, T = cfg["B"], cfg["T"]
    x, hx = t["x"], (t["h0"], t["c0"])
    ragged = [T, 0] + [1 + (3 * b) % T for b in range(B - 2)]
    views = ([b % B for b in range(B + 1)], [b % 2 for b in range(B + 1)])
    vlen = [T - 1, 1] + [1 + (2 * b) % (T - 1) for b in range(B - 1)]
    if form == "last":
        return [m(x)]
    if form == "all":
        return list(m(x, want_all=True))
    if form == "model":
        out = m(x)
        return list(out) if isinstance(out, tuple) else [out]
    if form == "model_views":
        return list(m(x, views=views, lengths=vlen))
    if form == "views" and not hasattr(m, "bidirectional"):
        return [m.forward_views(x, views, vlen)]
    if form == "views":
        out, (h_n, c_n) = m(x, hx, vlen, views)
    elif form == "packed":
        packed = nn.utils.rnn.pack_padded_sequence(x, torch.tensor([1 + (3 * b) % T for b in range(B)]), batch_first=True, enforce_sorted=False)
        out, (h_n, c_n) = m(packed, hx)
        out = out.data
    else:
        out, (h_n, c_n) = m(x, hx if form in ("hx", "ragged") else None, lengths=ragged if form == "ragged" else None)
    return [out, h_n, c_n]


def prepare(m, kind, mode, p, direct, hook_log):
    """Module state of one case: train / eval, the dropout attribute, direct_grads with patterned .grad buffers."""
    m.train(mode != "eval")
    enc = encoder(m)
    enc.dropout = p
    if kind in DIRECT:
        enc.direct_grads, enc.grad_ready_hook = direct, hook_log.append
    for i, q in enumerate(m.parameters()):
        q.grad = None
        if direct:
            q.grad = (0.25 + i + torch.arange(q.numel(), dtype=torch.float32, device=q.device) % 7).reshape(q.shape)


def run_case(m, kind, form, cfg, mode, p, direct, grad, seed, dev):
    """One forward (and backward) -> {name: integer view of a tensor, or a list}."""
    hook_log = []
    prepare(m, kind, mode, p, direct, hook_log)
    t = inputs(cfg, form, kind, grad, dev)
    torch.manual_seed(seed)
    got = {}
    with torch.set_grad_enabled(mode != "train_nograd"):
        outs = run_entry(m, form, cfg, t)
    for i, o in enumerate(outs):
        got[f"out{i}"] = bits(o)
    if mode != "train_nograd":
        g = torch.Generator().manual_seed(seed + 1)
        torch.autograd.backward(outs, [torch.randn(o.shape, generator=g).to(dev) for o in outs])
        for k, v in t.items():
            if v.grad is not None:
                got[f"d{k}"] = bits(v.grad)
        for name, q in m.named_parameters():
            got[f"grad.{name}"] = None if q.grad is None else bits(q.grad)
    got["hook_layers"] = list(hook_log)
    return got


def run_sequence(m, kind, name, cfg, dev):
    """The sequences of the module docstring on an LSTM / BiLSTM / HipLSTM module -> comparable results."""
    from cerebralsignalnetworks_amd import cabi
    hook_log = []
    prepare(m, kind, "train", 0.5, False, hook_log)
    torch.manual_seed(77)
    form = "last" if kind == "hip" else "hx"
    got = {}
    if name.startswith("two_outstanding"):
        ta, tb = inputs(cfg, form, kind, True, dev), inputs(cfg, form, kind, True, dev)
        a, b = run_entry(m, form, cfg, ta), run_entry(m, form, cfg, tb)
        assert sum(pl.busy for pl in m.all_plans()) == (4 * cfg["L"] if kind == "bilstm" else 2)
        for tag, outs in ((("a", a), ("b", b)) if name.endswith("fifo") else (("b", b), ("a", a))):
            torch.autograd.backward(outs, [torch.ones_like(o) for o in outs])
            got.update({f"{tag}.out{i}": bits(o) for i, o in enumerate(outs)})
        got.update({f"grad.{n}": bits(q.grad) for n, q in m.named_parameters()})
        got.update({f"{tag}.dx": bits(t["x"].grad) for tag, t in (("a", ta), ("b", tb))})
    elif name == "dropped_graph":
        t = inputs(cfg, form, kind, True, dev)
        outs = run_entry(m, form, cfg, t)
        before = len(m.all_plans())
        got["busy_while_held"] = sum(pl.busy for pl in m.all_plans())
        del outs
        got["busy_after_drop"] = sum(pl.busy for pl in m.all_plans())
        outs = run_entry(m, form, cfg, t)
        torch.autograd.backward(outs, [torch.ones_like(o) for o in outs])
        got["plans_added_by_the_second_forward"] = len(m.all_plans()) - before
        got.update({f"out{i}": bits(o) for i, o in enumerate(outs)})
    elif name == "refused_then_good":
        t = inputs(cfg, "views", kind, False, dev)
        B, T = cfg["B"], cfg["T"]
        rows, starts, lens = list(range(B)), [0] * (B - 1) + [2], [T] * B        # the last window ends 2 past the source
        try:
            m.forward_views(t["x"], (rows, starts), lens) if kind == "hip" else m(t["x"], None, lens, (rows, starts))
            got["refused"] = "not refused"
        except cabi.CsnError as e:
            got["refused"] = str(e)
        got["busy_after_refusal"] = sum(pl.busy for pl in m.all_plans())
        got["windows_left_set"] = sum(pl._views is not None for pl in m.all_plans())
        outs = run_entry(m, "views", cfg, t)
        torch.autograd.backward(outs, [torch.ones_like(o) for o in outs])
        got.update({f"out{i}": bits(o) for i, o in enumerate(outs)})
    else:
        t = inputs(cfg, form, kind, True, dev)
        outs = run_entry(m, form, cfg, t)
        torch.autograd.backward(outs, [torch.ones_like(o) for o in outs], retain_graph=True)
        try:
            torch.autograd.backward(outs, [torch.ones_like(o) for o in outs])
            got["second_backward"] = "no error"
        except RuntimeError as e:
            got["second_backward"] = "RuntimeError" if "second backward through one forward" in str(e) else str(e)
    got["busy_at_end"] = sum(pl.busy for pl in m.all_plans())
    return got


def same(a, b):
    if set(a) != set(b):
        return sorted(set(a) ^ set(b))
    return [k for k in a if not (torch.equal(a[k], b[k]) if isinstance(a[k], torch.Tensor) and isinstance(b[k], torch.Tensor)
                                 else a[k] == b[k])]


def case_list():
    out = []
    for cname, (entry, (kind, form)) in itertools.product(CONFIGS, ENTRIES.items()):
        for mode, p in itertools.product(("train", "train_nograd", "eval"), (0.0, 0.5)):
            with_grad = mode != "train_nograd"
            for direct in ((False, True, "accumulate") if with_grad and kind in DIRECT else (False,)):
                for grad in ((False, True) if with_grad and form not in NO_INPUT_GRAD else (False,)):
                    out.append(dict(name=f"{cname}.{entry}.{mode}.p{p}.direct_{direct}.inputs_grad_{grad}", config=cname, kind=kind,
                                    form=form, mode=mode, p=p, direct=direct, grad=grad))
    for cname, kind, seq in itertools.product(CONFIGS, ("hip", "lstm", "bilstm"), SEQUENCES):
        out.append(dict(name=f"{cname}.{kind}.sequence.{seq}", config=cname, kind=kind, sequence=seq))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent-module", required=True, help="the parent commit's lstm_model.py (git show), in a git-ignored place")
    ap.add_argument("--parent-commit", required=True, help="hash of the parent commit")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "lstm_module_identity.json"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("lstm_module_identity: no GPU is visible (there is no fallback)")
    from cerebralsignalnetworks_amd import cabi, lstm_model as this
    files = {"parent": load_parent(os.path.abspath(args.parent_module)), "this": this}
    dev = torch.device("cuda:0")
    rec = Recorder(cabi)
    modules, rows, status, busy = {}, [], set(), 0
    try:
        for seed, c in enumerate(case_list()):
            cfg = dict(CONFIGS[c["config"]])
            got, logs = {}, {}
            for who, lm in files.items():
                key = (who, c["config"], c["kind"])
                if key not in modules:
                    rec.start(who)
                    modules[key] = make_module(lm, c["kind"], cfg, dev)
                log = rec.start(who)
                m = modules[key]
                try:
                    if "sequence" in c:
                        got[who] = run_sequence(m, c["kind"], c["sequence"], cfg, dev)
                    else:
                        got[who] = run_case(m, c["kind"], c["form"], cfg, c["mode"], c["p"], c["direct"], c["grad"], seed, dev)
                except cabi.CsnError as e:      # (a refusal by the library is a result like any other: it must be the same one)
                    got[who] = {"refused_by_the_library": str(e)}
                logs[who] = list(log)
                status |= {pl.status() for pl in encoder(m).all_plans()}      # (an evicted plan was idle: read after its last case)
                busy += sum(pl.busy for pl in encoder(m).all_plans())
            differ = same(got["parent"], got["this"])
            row = dict(case=c["name"], tensors=sum(isinstance(v, torch.Tensor) for v in got["this"].values()),
                       plan_calls=sum(e[0] in ("forward", "backward") for e in logs["this"]),
                       plans_created=sum(e[0] == "create" for e in logs["this"]), results_differ=differ,
                       records_equal=logs["parent"] == logs["this"], identical=not differ and logs["parent"] == logs["this"])
            if "sequence" in c or "refused_by_the_library" in got["this"]:
                row.update({k: v for k, v in got["this"].items() if not isinstance(v, torch.Tensor) and k != "hook_layers"})
            if not row["identical"]:
                row["first_record_difference"] = next(([repr(a), repr(b)] for a, b in itertools.zip_longest(logs["parent"], logs["this"])
                                                       if a != b), None)
                print(json.dumps(row), flush=True)
            rows.append(row)
        torch.cuda.synchronize()
        status = sorted(status)
    finally:
        rec.restore()
    ok = all(r["identical"] for r in rows) and status == [0] and busy == 0
    result = dict(tool="tools/lstm_module_identity.py: every case once on the parent commit's lstm_model.py and once on this tree's, one "
                       "process, one library; outputs and gradients compared as integers, the recorded plan calls and settings compared",
                  device=torch.cuda.get_device_name(0), parent_commit=args.parent_commit, n_cases=len(rows),
                  n_plan_calls=sum(r["plan_calls"] for r in rows), n_tensors_compared=sum(r["tensors"] for r in rows),
                  plans_created=rec.created, plan_status_words=status, plans_left_busy=busy, all_identical=ok,
                  cases_not_identical=[r["case"] for r in rows if not r["identical"]],
                  sequences=[r for r in rows if ".sequence." in r["case"]])
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")
    print(f"{len(rows)} cases, all identical: {ok} (status words {status}, {busy} plans left busy)")
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
