"""The switch of csrc/ll_forms.hpp that puts contact generation in front of the tree passes (CGEN_EARLY), over build x TGS x DIAG x BALL x
LIMITS: it is on exactly for the kernels with the visit table
(no joint limits, no TGS, no ball; in the register build not the diagnostic kernel).  The joint-limit kernels activate their rows with v*,
which exists only behind pass 3, so their contact set-up cannot move; the TGS and ball kernels stay with them.  CPU only: a host program
that includes the header alone, as tests/test_ll_forms.py does for the earlier switches (that file's table is unchanged).  And the
fragment with the contact generation is included at exactly two places of the kernel, one per value of the switch."""
import os
import re
import subprocess
import tempfile

import pytest

CSRC = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "vid2player3d_amd", "csrc")

PROG = r'''
#include "ll_forms.hpp"
#include <stdio.h>
using namespace v2p;
template <LlBuild B, bool TGS, bool DIAG, bool BALL, bool LIMITS>
void row(const char* build) {
    typedef LlForms<B, TGS, DIAG, BALL, LIMITS> F;
    printf("%s %d %d %d %d : %d %d\n", build, (int)TGS, (int)DIAG, (int)BALL, (int)LIMITS, (int)F::VTAB, (int)F::CGEN_EARLY);
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


def want(build, tgs, diag, ball, limits):
    """The rule, written out from the flags (not from VTAB)."""
    on = not limits and not tgs and not ball and not (build == "regs" and diag)
    return int(on)


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
        key, row = (part.strip() for part in line.split(":"))
        build, *flags = key.split()
        got[(build, tuple(int(f) for f in flags))] = tuple(int(v) for v in row.split())
    return got


def test_switch_table(printed):
    assert len(printed) == 32
    on = 0
    for (build, flags), (vtab, early) in printed.items():
        w = want(build, *flags)
        assert (vtab, early) == (w, w), (build, flags)
        on += w
    assert on == 3, "lds: the production and the diagnostic kernel; regs: the production kernel"


def test_fragment_is_included_once_per_value_of_the_switch():
    text = open(os.path.join(CSRC, "physics_ll.hip")).read()
    assert len(re.findall(r'^#include "ll_contact_setup.inc"$', text, flags=re.M)) == 2
    first = text.index('#include "ll_contact_setup.inc"')
    second = text.index('#include "ll_contact_setup.inc"', first + 1)
    assert "if constexpr (F::CGEN_EARLY) {" in text[:first] and text.index("pass 2: articulated inertia") > first
    assert text.index("pass 3: accelerations") < second < text.index("Lambda_b, root -> leaves by level")
    frag = open(os.path.join(CSRC, "ll_contact_setup.inc")).read()
    # (what it may touch of the kernel's state: the pose it reads, cnt and the records it leaves - no velocity, no Lambda)
    for name in ("Lam.", "park_vel", "unpark_vel", "PARK_W0", "PARK_XD0", "rootlam"):
        assert name not in frag, name
