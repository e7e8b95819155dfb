"""CPU: the switch and the LDS request of the parked form of the H = 768 forward, asked of the
library's own headers by a small host program: CSN_NO_FWD_PARK is read into Options like its neighbours, and the
request of the touched instantiations stays above half of a CU's 160 KB of LDS (one workgroup per CU) and within it."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "cerebralsignalnetworks_amd", "csrc")
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")

PROGRAM = r"""
#include "lstm_cell_blk.h"
int main() {
  const csn::Options o = csn::options_from_env();
  printf("no_fwd_park %d no_half_tiles %d\n", (int)o.no_fwd_park, (int)o.no_half_tiles);
  printf("lds %zu %zu %zu\n", csn::fwd_persist_lds_bytes(6, false), csn::fwd_persist_lds_bytes(6, true),
         csn::fwd_persist_lds_bytes(8, false));
  return 0;
}
"""


@pytest.fixture(scope="module")
def probe(tmp_path_factory):
    d = tmp_path_factory.mktemp("fwd_park")
    src, exe = d / "probe.hip", d / "probe"
    src.write_text(PROGRAM)
    subprocess.run([HIPCC, "--cuda-host-only", "-std=c++17", "-O0", "-I", CSRC, str(src), "-o", str(exe)], check=True)

    def run(env):
        clean = {k: v for k, v in os.environ.items() if not k.startswith("CSN_")}
        out = subprocess.run([str(exe)], env={**clean, **env}, check=True, capture_output=True, text=True).stdout.split()
        return {"no_fwd_park": int(out[1]), "no_half_tiles": int(out[3]), "lds": [int(v) for v in out[5:8]]}
    return run


def test_switch_is_read_into_options(probe):
    assert probe({})["no_fwd_park"] == 0
    assert probe({"CSN_NO_FWD_PARK": "1"}) == {**probe({}), "no_fwd_park": 1}
    assert probe({"CSN_NO_HALF_TILES": "1"})["no_fwd_park"] == 0          # a neighbour does not set it


def test_lds_request_of_the_touched_instantiations(probe):
    ring4, parked, nq8 = probe({})["lds"]
    assert ring4 == (4 * 4 * 6 * 71 + 4 * 6) * 16 == 109440                # today's request, unchanged
    assert parked == ring4 + 6 * 256 * 16                                    # + 6 lane-linear 16-byte slots per thread
    for req in (ring4, parked):
        assert 80 * 1024 < req <= 160 * 1024
    assert nq8 == (4 * 4 * 8 * 71 + 4 * 8) * 16                              # <8,*>: untouched
