"""CPU: tools/kernel_isa_diff.py on two synthetic listings -- the comparison that shows a refactoring of the kernels'
sources to generate the same device code.  A function that only moved inside its file (another label ordinal, other
comments) is SAME; another register, instruction order or resource descriptor is DIFF, with the histogram saying whether
the instructions themselves changed; a kernel present on one side only fails the run."""
import io
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import kernel_isa_diff as kd      # noqa: E402

BODY_A = "\tv_add_u32_e32 v1, v2, v3\n\ts_cbranch_execz .LBB{n}_2\n\tv_mul_f32_e32 v4, v1, v1\n.LBB{n}_2:\n\ts_endpgm\n"
BODY_B = "\ts_waitcnt lgkmcnt(0)\n\tv_mov_b32_e32 v0, 0\n\ts_endpgm\n"


def _listing(tmp_path, name, functions, vgprs=None):
    """functions: [(mangled name, body template with {n} for the function ordinal)] in file order."""
    text = "\t.text\n"
    for n, (fn, body) in enumerate(functions):
        text += f"\t.globl\t{fn}\n{fn}:                      ; @{fn}\n; %bb.0:\n" + body.format(n=n) + f".Lfunc_end{n}:\n"
        text += f"\t.size\t{fn}, .Lfunc_end{n}-{fn}\n\t.section\t.rodata\n\t.amdhsa_kernel {fn}\n"
        text += f"\t\t.amdhsa_next_free_vgpr {(vgprs or {}).get(fn, 8)}\n\t.end_amdhsa_kernel\n\t.text\n"
    p = tmp_path / name
    p.write_text(text)
    return str(p)


def _run(argv):
    out, saved = io.StringIO(), sys.stdout
    sys.stdout = out
    try:
        rc = kd.main(argv)
    finally:
        sys.stdout = saved
    return rc, out.getvalue()


def test_a_moved_function_is_same_and_a_missing_one_fails(tmp_path):
    old = _listing(tmp_path, "old.s", [("_Z9gemm_nt_av", BODY_A), ("_Z9gemm_tn_bv", BODY_B), ("_Z5otherv", BODY_B)])
    # the same two kernels split over two files: other ordinals, and a comment more
    new1 = _listing(tmp_path, "new1.s", [("_Z9gemm_tn_bv", BODY_B)])
    new2 = _listing(tmp_path, "new2.s", [("_Z4elsev", BODY_B), ("_Z9gemm_nt_av", BODY_A.replace("v1, v1\n", "v1, v1  ; squared\n"))])
    rc, text = _run([old, "--", new1, new2])
    assert rc == 0 and text.count("SAME") == 2 and "DIFF" not in text and "other" not in text, text
    assert "2 kernels: 0 missing, 0 differ" in text
    # a kernel that vanished, and one that appeared
    rc, text = _run([old, "--", new1])
    assert rc == 1 and "MISSING in the new build  _Z9gemm_nt_av" in text
    rc, text = _run([new1, "--", old])
    assert rc == 1 and "MISSING in the old build  _Z9gemm_nt_av" in text
    # ... unless it was renamed on purpose
    renamed = _listing(tmp_path, "renamed.s", [("_Z9gemm_nt_cv", BODY_A), ("_Z9gemm_tn_bv", BODY_B)])
    rc, text = _run(["--rename", "_Z9gemm_nt_av=_Z9gemm_nt_cv", old, "--", renamed])
    assert rc == 0 and "SAME  _Z9gemm_nt_cv" in text, text


def test_a_diff_prints_both_histograms(tmp_path):
    old = _listing(tmp_path, "old.s", [("_Z9gemm_nt_av", BODY_A), ("_Z9gemm_tn_bv", BODY_B)])
    regs = _listing(tmp_path, "regs.s", [("_Z9gemm_nt_av", BODY_A.replace("v4", "v5")), ("_Z9gemm_tn_bv", BODY_B)])
    rc, text = _run([old, "--", regs])
    assert rc == 0 and "DIFF  _Z9gemm_nt_av" in text and "histograms equal: 4 instructions, 4 mnemonics" in text, text
    assert "SAME  _Z9gemm_tn_bv" in text
    assert "lines changed: 2" in text and "descriptor equal: 1 directives" in text, text      # one line out, one line in
    assert _run(["--strict", old, "--", regs])[0] == 1
    # two instructions that swapped places: the histogram cannot tell, the line count and the descriptor can
    swapped = BODY_A.replace("\tv_add_u32_e32 v1, v2, v3\n\ts_cbranch_execz .LBB{n}_2\n", "\ts_cbranch_execz .LBB{n}_2\n\tv_add_u32_e32 v1, v2, v3\n")
    assert swapped != BODY_A
    swap = _listing(tmp_path, "swap.s", [("_Z9gemm_nt_av", swapped), ("_Z9gemm_tn_bv", BODY_B)])
    rc, text = _run([old, "--", swap])
    assert "histograms equal" in text and "lines changed: 2" in text and "descriptor equal" in text, text
    more = _listing(tmp_path, "more.s", [("_Z9gemm_nt_av", BODY_A), ("_Z9gemm_tn_bv", "\ts_nop 0\n" + BODY_B)])
    rc, text = _run([old, "--", more])
    lines = text.splitlines()
    at = lines.index(next(ln for ln in lines if ln.startswith("DIFF  _Z9gemm_tn_bv")))
    assert lines[at + 1].split() == ["s_nop", "0", "->", "1"], text
    assert lines[at + 2].split() == ["lines", "changed:", "1"] and lines[at + 3].split()[:2] == ["descriptor", "equal:"], text
    # the resource descriptor counts: the same instructions on more registers are not the same kernel
    wider = _listing(tmp_path, "wider.s", [("_Z9gemm_nt_av", BODY_A), ("_Z9gemm_tn_bv", BODY_B)], vgprs={"_Z9gemm_tn_bv": 16})
    rc, text = _run([old, "--", wider])
    assert "DIFF  _Z9gemm_tn_bv" in text and "histograms equal" in text
    assert "descriptor equal" not in text, text
    at = text.splitlines().index(next(ln for ln in text.splitlines() if ln.startswith("DIFF  _Z9gemm_tn_bv")))
    assert [ln.split() for ln in text.splitlines()[at + 1:at + 4]] == [
        ["histograms", "equal:", "3", "instructions,", "3", "mnemonics"], ["lines", "changed:", "2"],
        [".amdhsa_next_free_vgpr", "8", "->", "16"]], text
    # --match narrows what is compared
    rc, text = _run(["--match", "gemm_nt", old, "--", more])
    assert rc == 0 and "gemm_tn" not in text and "1 kernels: 0 missing, 0 differ" in text
