"""Which form of each switched phase every instantiation of physics_ll_kernel runs (csrc/ll_forms.hpp), without a GPU: a stand-alone
C++ program includes the header alone and prints every switch for both builds x all 16 combinations of TGS, DIAG, BALL, LIMITS.  The
expected table is written out below, by hand, from the expressions as they stood inside the kernel's body before the policy had a header
of its own (the `constexpr bool`s under `#ifdef V2P_LL_REGS_BUILD`): a pull request that moves a kernel to another form has to change
this table, and the change shows in its diff.  The second test holds the kernel's body to reading the policy: no `#ifdef` of the build
between the kernel's signature and the end of its namespace."""
import os
import re
import subprocess
import tempfile

import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(REPO, "vid2player3d_amd", "csrc")

# columns: FASTARG VTAB ROWX UPMASK OPAQUE_H DIAGX | waves per SIMD of (wps, wps_ball, wps_limits) = (3, 4, 5)
# (SETUPX, LIVEM and ROWCNT equal VTAB in every row: asserted below instead of three more columns)
# rows: (TGS, DIAG, BALL, LIMITS)
#   default build:  FASTARG = !BALL && !LIMITS;  VTAB = !LIMITS && !TGS && !BALL;  ROWX = true;  DIAGX = DIAG
#   register build: FASTARG = !BALL && !LIMITS && !TGS && !DIAG;  VTAB = !LIMITS && !TGS && !BALL && !DIAG;  ROWX = VTAB;  DIAGX = false
#   both: UPMASK = !LIMITS && !TGS;  OPAQUE_H = BALL || LIMITS;  waves = DIAG ? 2 : BALL ? wps_ball : LIMITS ? wps_limits : wps
TABLE = {
    "lds": {
        (0, 0, 0, 0): "1 1 1 1 0 0 | 3",
        (0, 0, 0, 1): "0 0 1 0 1 0 | 5",
        (0, 0, 1, 0): "0 0 1 1 1 0 | 4",
        (0, 0, 1, 1): "0 0 1 0 1 0 | 4",
        (0, 1, 0, 0): "1 1 1 1 0 1 | 2",
        (0, 1, 0, 1): "0 0 1 0 1 1 | 2",
        (0, 1, 1, 0): "0 0 1 1 1 1 | 2",
        (0, 1, 1, 1): "0 0 1 0 1 1 | 2",
        (1, 0, 0, 0): "1 0 1 0 0 0 | 3",
        (1, 0, 0, 1): "0 0 1 0 1 0 | 5",
        (1, 0, 1, 0): "0 0 1 0 1 0 | 4",
        (1, 0, 1, 1): "0 0 1 0 1 0 | 4",
        (1, 1, 0, 0): "1 0 1 0 0 1 | 2",
        (1, 1, 0, 1): "0 0 1 0 1 1 | 2",
        (1, 1, 1, 0): "0 0 1 0 1 1 | 2",
        (1, 1, 1, 1): "0 0 1 0 1 1 | 2",
    },
    "regs": {
        (0, 0, 0, 0): "1 1 1 1 0 0 | 3",
        (0, 0, 0, 1): "0 0 0 0 1 0 | 5",
        (0, 0, 1, 0): "0 0 0 1 1 0 | 4",
        (0, 0, 1, 1): "0 0 0 0 1 0 | 4",
        (0, 1, 0, 0): "0 0 0 1 0 0 | 2",
        (0, 1, 0, 1): "0 0 0 0 1 0 | 2",
        (0, 1, 1, 0): "0 0 0 1 1 0 | 2",
        (0, 1, 1, 1): "0 0 0 0 1 0 | 2",
        (1, 0, 0, 0): "0 0 0 0 0 0 | 3",
        (1, 0, 0, 1): "0 0 0 0 1 0 | 5",
        (1, 0, 1, 0): "0 0 0 0 1 0 | 4",
        (1, 0, 1, 1): "0 0 0 0 1 0 | 4",
        (1, 1, 0, 0): "0 0 0 0 0 0 | 2",
        (1, 1, 0, 1): "0 0 0 0 1 0 | 2",
        (1, 1, 1, 0): "0 0 0 0 1 0 | 2",
        (1, 1, 1, 1): "0 0 0 0 1 0 | 2",
    },
}

PROG = r'''
#include "ll_forms.hpp"
#include <stdio.h>
using namespace v2p;
template <LlBuild B, bool TGS, bool DIAG, bool BALL, bool LIMITS>
void row(const char* build) {
    typedef LlForms<B, TGS, DIAG, BALL, LIMITS> F;
    printf("%s %d %d %d %d : %d %d %d %d %d %d | %d : %d %d %d\n", build, (int)TGS, (int)DIAG, (int)BALL, (int)LIMITS, (int)F::FASTARG, (int)F::VTAB,
           (int)F::ROWX, (int)F::UPMASK, (int)F::OPAQUE_H, (int)F::DIAGX, F::waves_per_simd(3, 4, 5), (int)F::SETUPX, (int)F::LIVEM, (int)F::ROWCNT);
}
template <LlBuild B, int I>
void rows(const char* build) {
    if constexpr (I < 16) {
        row<B, (I & 8) != 0, (I & 4) != 0, (I & 2) != 0, (I & 1) != 0>(build);
        rows<B, I + 1>(build);
    }
}
int main() {
    rows<LlBuild::Lds, 0>("lds");
    rows<LlBuild::Regs, 0>("regs");
    return 0;
}
'''


@pytest.fixture(scope="module")
def printed():
    with tempfile.TemporaryDirectory() as d:
        src = os.path.join(d, "s.cpp")
        open(src, "w").write(PROG)
        path = os.path.join(d, "s")
        subprocess.check_call(["g++", "-std=c++17", "-Wall", "-I", CSRC, src, "-o", path])
        out = subprocess.check_output([path]).decode()
    print(out)
    got = {}
    for line in out.splitlines():
        key, row, tied = (part.strip() for part in line.split(":"))
        build, *flags = key.split()
        got[(build, tuple(int(f) for f in flags))] = (row, tied)
    return got


@pytest.mark.parametrize("build", ["lds", "regs"])
def test_forms_table(printed, build):
    assert len(printed) == 32
    for flags, want in TABLE[build].items():
        row, tied = printed[(build, flags)]
        assert row == want, (build, flags)
        vtab = want.split()[1]
        assert tied == " ".join([vtab] * 3), (build, flags)  # SETUPX, LIVEM, ROWCNT


def test_kernel_body_reads_the_policy():
    """no #ifdef of the build between the kernel's signature and the end of its namespace"""
    text = open(os.path.join(CSRC, "physics_ll.hip")).read()
    start = text.index("void physics_ll_kernel(PhysArgs a) {")
    end = text.index("}  // namespace V2P_LL_NS")
    assert start < end
    assert not re.search(r"V2P_LL_REGS_BUILD", text[start:end])
    assert "using F = LlForms<LL_BUILD, TGS, DIAG, BALL, LIMITS>;" in text[start:end]
