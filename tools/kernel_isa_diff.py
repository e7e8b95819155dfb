#!/usr/bin/env python3
"""Compare the device code of two builds kernel by kernel, by mangled name.

    kernel_isa_diff.py [--match REGEX] [--rename OLD=NEW ...] [--strict] old.s [old2.s ...] -- new.s [new2.s ...]

The listings are the `*-hip-amdgcn-amd-amdhsa-gfx950.s` files that the Makefile's -save-temps=obj leaves next to the
objects.  A kernel is the text from its label to its `.Lfunc_end`, plus its `.amdhsa_kernel` descriptor (registers, LDS,
scratch).  Before comparing, comments are stripped and the function ordinal is dropped from local labels (`.LBB12_3` ->
`.LBB_3`, `.Lfunc_end12` -> `.Lfunc_end`): the ordinal is the function's position in its file and changes when a file is
split or a function moves.  One line per kernel: SAME or DIFF; for a DIFF the instruction-mnemonic histogram of both
sides (the mnemonics whose counts differ, or `histograms equal` when only registers or the order changed), then the
number of lines that changed (lines only in the old text + lines only in the new one: two instructions that swapped
places are 2) and the `.amdhsa_*` descriptor lines that changed, or `descriptor equal` -- which is what tells a swapped
instruction pair from another register allocation.

Exit status: 1 when a kernel that matches is present on one side only (--rename maps an old name to its new one first),
or with --strict when any kernel differs; 0 otherwise."""
import argparse
import collections
import difflib
import re
import sys

DEFAULT_MATCH = r"gemm_|lstm_bwd_persist_kernel"


def _clean(line):
    line = line.split(";", 1)[0].rstrip()
    line = re.sub(r"\.LBB\d+_", ".LBB_", line)
    return re.sub(r"\.Lfunc_(begin|end)\d+", r".Lfunc_\1", line)


def kernels(path):
    """{mangled name: [cleaned lines of the body and of the descriptor]} of every kernel of a listing."""
    with open(path) as f:
        lines = f.read().splitlines()
    names = {m.group(1) for m in (re.match(r"\s*\.amdhsa_kernel\s+(\S+)", ln) for ln in lines) if m}
    found = collections.defaultdict(list)
    current = None
    for ln in lines:
        label = re.match(r"([A-Za-z_][\w$.]*):", ln)
        desc = re.match(r"\s*\.amdhsa_kernel\s+(\S+)", ln)
        if current is None and label and label.group(1) in names:
            current = label.group(1)                    # body: label .. .Lfunc_end
        elif current is None and desc:
            current = desc.group(1)                     # descriptor: .amdhsa_kernel .. .end_amdhsa_kernel
        if current is None:
            continue
        text = _clean(ln)
        if text.strip():
            found[current].append(text.strip())
        if re.match(r"\.Lfunc_end\d+:", ln) or re.match(r"\s*\.end_amdhsa_kernel", ln):
            current = None
    return dict(found)


def histogram(lines):
    """Mnemonic -> count over the instruction lines (no labels, no directives)."""
    h = collections.Counter()
    for ln in lines:
        word = ln.split()[0]
        if not word.startswith(".") and not word.endswith(":"):
            h[word] += 1
    return h


def changed_lines(old, new):
    """Lines of `old` that are not in `new` at their place + lines of `new` that are not in `old`."""
    ops = difflib.SequenceMatcher(None, old, new, autojunk=False).get_opcodes()
    return sum((i2 - i1) + (j2 - j1) for tag, i1, i2, j1, j2 in ops if tag != "equal")


def descriptor(lines):
    """{.amdhsa_* directive: its operand text} of a kernel."""
    return {ln.split()[0]: " ".join(ln.split()[1:]) for ln in lines if ln.startswith(".amdhsa_") and not ln.startswith(".amdhsa_kernel")}


def _side(paths, match, renames):
    out = {}
    for p in paths:
        for name, body in kernels(p).items():
            if re.search(match, name):
                new = renames.get(name, name)
                out[new] = [ln.replace(name, new) for ln in body]
    return out


def compare(old_paths, new_paths, match=DEFAULT_MATCH, renames=None, out=None):
    """Prints the report; returns (missing, differing) kernel name lists."""
    out = out or sys.stdout
    old, new = _side(old_paths, match, renames or {}), _side(new_paths, match, {})
    missing, differing = [], []
    for name in sorted(set(old) | set(new)):
        if name not in old or name not in new:
            missing.append(name)
            print(f"MISSING in the {'old' if name not in old else 'new'} build  {name}", file=out)
        elif old[name] == new[name]:
            print(f"SAME  {name}  ({len(new[name])} lines)", file=out)
        else:
            differing.append(name)
            ho, hn = histogram(old[name]), histogram(new[name])
            print(f"DIFF  {name}  ({len(old[name])} -> {len(new[name])} lines)", file=out)
            if ho == hn:
                print(f"      histograms equal: {sum(ho.values())} instructions, {len(ho)} mnemonics", file=out)
            for m in sorted(set(ho) | set(hn)):
                if ho[m] != hn[m]:
                    print(f"      {m:40s} {ho[m]:6d} -> {hn[m]:6d}", file=out)
            print(f"      lines changed: {changed_lines(old[name], new[name])}", file=out)
            do, dn = descriptor(old[name]), descriptor(new[name])
            if do == dn:
                print(f"      descriptor equal: {len(dn)} directives", file=out)
            for d in sorted(set(do) | set(dn)):
                if do.get(d) != dn.get(d):
                    print(f"      {d:40s} {do.get(d, '-'):>6s} -> {dn.get(d, '-'):>6s}", file=out)
    print(f"{len(set(old) | set(new))} kernels: {len(missing)} missing, {len(differing)} differ", file=out)
    return missing, differing


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--match", default=DEFAULT_MATCH, help="regex on the mangled name (default: %(default)s)")
    ap.add_argument("--rename", action="append", default=[], metavar="OLD=NEW", help="an old mangled name and its new one")
    ap.add_argument("--strict", action="store_true", help="a DIFF fails too")
    ap.add_argument("listings", nargs="+", help="old.s [...] -- new.s [...]")
    argv = list(sys.argv[1:] if argv is None else argv)
    if "--" not in argv:
        ap.error("expected: old.s [old2.s ...] -- new.s [new2.s ...]")
    cut = argv.index("--")
    args = ap.parse_args(argv[:cut])
    new_paths = argv[cut + 1:]
    if not new_paths:
        ap.error("no new listing behind --")
    renames = dict(r.split("=", 1) for r in args.rename)
    missing, differing = compare(args.listings, new_paths, args.match, renames)
    return 1 if missing or (args.strict and differing) else 0


if __name__ == "__main__":
    sys.exit(main())
