"""CPU: what the build says about the four-wave 256 x 192 kernel (gemm_nt_w4_kernel, csrc/gemm_nt.hip) -- the compiler's
resource remarks kept next to the object, the LDS the launcher asks for -- and the launcher's rule for operands outside
the kernel's 32-bit offset window.  Two workgroups per CU need at most 256 registers per lane at two waves per SIMD,
no scratch, and at most half of the CU's 160 KB of LDS each."""
import os
import re

import pytest

from cerebralsignalnetworks_amd import cabi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RES = os.path.join(ROOT, "build", "csrc", "gemm_nt.res")


def _kernels(text, name):
    """{mangled name: {field: int}} of the kernels whose mangled name contains `name`."""
    found = {}
    blocks = re.split(r"remark: [^\n]*Function Name: ", text)[1:]
    for block in blocks:
        mangled = block.split()[0]
        if name in mangled:
            fields = dict(re.findall(r":\s+([A-Za-z][A-Za-z \[\]/]*?): (\d+) \[-Rpass", block))
            found[mangled] = {k.strip(): int(v) for k, v in fields.items()}
    return found


def test_parser_reads_a_resource_block():
    text = ("remark: gemm.hip:1:0: Function Name: _Z1aIfE [-Rpass-analysis=kernel-resource-usage]\n"
            "remark: gemm.hip:1:0:     VGPRs: 7 [-Rpass-analysis=kernel-resource-usage]\n"
            "remark: gemm.hip:1:0:     ScratchSize [bytes/lane]: 0 [-Rpass-analysis=kernel-resource-usage]\n"
            "remark: gemm.hip:1:0:     Occupancy [waves/SIMD]: 2 [-Rpass-analysis=kernel-resource-usage]\n"
            "remark: gemm.hip:9:0: Function Name: _Z1bv [-Rpass-analysis=kernel-resource-usage]\n"
            "remark: gemm.hip:9:0:     VGPRs: 9 [-Rpass-analysis=kernel-resource-usage]\n")
    assert _kernels(text, "1a") == {"_Z1aIfE": {"VGPRs": 7, "ScratchSize [bytes/lane]": 0, "Occupancy [waves/SIMD]": 2}}
    assert _kernels(text, "nothing") == {}


@pytest.mark.skipif(not os.path.exists(RES), reason="no in-tree build: build/csrc/gemm_nt.res is absent")
def test_both_instantiations_fit_two_workgroups_per_cu():
    with open(RES) as f:
        kernels = _kernels(f.read(), "gemm_nt_w4_kernel")
    assert len(kernels) == 2, f"expected the float32 and the bfloat16 instantiation of gemm_nt_w4_kernel, found {sorted(kernels)}"
    assert any("IDF16b" in k for k in kernels) and any("IfLi" in k for k in kernels), sorted(kernels)
    for name, r in kernels.items():
        print(name, r)
        assert r["ScratchSize [bytes/lane]"] == 0, name
        assert r["Occupancy [waves/SIMD]"] == 2, name
        assert r["VGPRs"] + r["AGPRs"] <= 256, name


def test_lds_request_leaves_room_for_a_second_workgroup():
    assert 0 < cabi.gemm_nt_w4_lds_bytes() <= 81920


def test_operands_outside_the_32_bit_window_fall_back():
    """The kernel adds a 32-bit byte offset per lane to the operand base: A[M, K] and Bt[N, K] (2 bytes per element) must
    each end below 4 GiB, else gemm_nt() launches the 8-wave kernel of the same tile."""
    fits = cabi.gemm_nt_w4_offsets_fit
    assert fits(8192, 3072, 768) and fits(256, 49152, 128)
    lim = 1 << 31
    for K in (64, 768, 4096):
        edge = -(-lim // K)                  # the first row count at which rows * K >= 2^31 elements = 4 GiB
        assert fits(edge - 1, 3072, K) and fits(3072, edge - 1, K)
        assert not fits(edge, 3072, K) and not fits(3072, edge, K)
        assert not fits(edge + 1, 192, K) and not fits(256, edge + 191, K)
    assert not fits(1 << 40, 192, 1 << 40) and not fits(256, 1 << 62, 64)      # no overflow of the products
    assert not fits(0, 192, 64) and not fits(256, 192, 0)
