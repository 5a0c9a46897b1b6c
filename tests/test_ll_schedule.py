"""The launch policy of the link-per-lane schedule (csrc/ll_schedule.hpp) without a GPU: a stand-alone C++ program includes the header
alone and prints the job plan of a launch and the engine's defaults for a table of cases.  The expected values are worked out by hand
from the formulas as they stood inside the launcher (job_grid) and env.hip (engine_defaults) before the policy had a module of its own,
on an MI355X's 256 CUs: a launch is cut above 8 x CUs = 2048 env pairs under substep_jobs = 1 (above 0 under substep_jobs = 2), jobs are
two substeps long from 32 x CUs = 8192 env pairs.  blocks = ceil(envs / 2).  The sizes at which the engine's own choices switch are
reached by no GPU test (they run 32 - 64 envs)."""
import os
import subprocess
import tempfile

import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

ENGINE = None  # job_len / job_lead left to the engine: stored as 0 / -1
# name: (blocks, nsub, ball, substep_jobs, job_len, job_lead, job_mono_permille) -> (cut, mono, len, lead, jobs per cut pair, grid)
PLANS = {
    "headline, 8192 envs": ((4096, 4, 0, 1, ENGINE, ENGINE, 60), (1, 245, 1, 2, 3, 11798)),
    "4096 envs (not above the threshold)": ((2048, 4, 0, 1, ENGINE, ENGINE, 60), (0, 2048, 1, 1, None, 2048)),
    "16384 envs": ((8192, 4, 0, 1, ENGINE, ENGINE, 250), (1, 2048, 2, 2, 2, 14336)),
    "racket + ball, 8192 envs": ((4096, 4, 1, 1, ENGINE, ENGINE, 250), (1, 1024, 1, 1, 4, 13312)),
    "12 substeps, job_len 5, 64 envs": ((32, 12, 0, 2, 5, ENGINE, 60), (1, 1, 5, 5, 3, 94)),
    "12 substeps, engine's choice, 64 envs": ((32, 12, 0, 2, ENGINE, ENGINE, 60), (1, 1, 1, 2, 11, 342)),
    # (a cfg job_lead < 0 is stored as 0: at 8192 envs that is this row)
    "stored job_lead 0 (jobs of equal length)": ((4096, 4, 0, 1, ENGINE, 0, 60), (1, 245, 1, 1, 4, 15649)),
    "job_lead 3": ((4096, 4, 0, 1, ENGINE, 3, 60), (1, 245, 1, 3, 2, 7947)),
    "job_lead 4 (= nsub, out of range -> job_len)": ((4096, 4, 0, 1, ENGINE, 4, 60), (1, 245, 1, 1, 4, 15649)),
    "one env pair": ((1, 4, 0, 2, ENGINE, ENGINE, 60), (0, 1, 1, 1, None, 1)),
    "jobs off": ((4096, 4, 0, 0, ENGINE, ENGINE, 60), (0, 4096, 1, 1, None, 4096)),
}
# (n, joint_limits, regs_build, ball) -> (pair_mix_permille, job_mono_permille)
DEFAULTS = {
    (8192, 0, 0, 0): (150, 60),
    (1024, 0, 1, 0): (500, 60),
    (16384, 0, 0, 0): (0, 250),
    (16384, 0, 1, 0): (0, 250),
    (64, 1, 0, 0): (0, 250), (1024, 1, 1, 0): (0, 250), (8192, 1, 0, 0): (0, 250), (16384, 1, 0, 0): (0, 250),
    (64, 0, 0, 1): (0, 250), (1024, 0, 1, 1): (0, 250), (8192, 0, 0, 1): (0, 250), (8192, 1, 0, 1): (0, 250),
}

PROG = r'''
#include "ll_schedule.hpp"
#include <stdio.h>
#include <stdlib.h>
int main(int argc, char** argv) {
    if (argc == 8) {  // blocks nsub ball substep_jobs job_len job_lead job_mono_permille
        const unsigned blocks = (unsigned)atoi(argv[1]);
        const int nsub = atoi(argv[2]), ball = atoi(argv[3]), jobs = atoi(argv[4]);
        v2p::JobCfg j = {};
        j.on = jobs ? 1 : 0;
        j.min_blocks = jobs == 1 ? 256 * 8 : 0;
        j.len2_blocks = 256 * 32;
        j.len = atoi(argv[5]);
        j.lead = atoi(argv[6]);
        j.mono_permille = atoi(argv[7]);
        const v2p::JobPlan p = v2p::job_plan(j, blocks, nsub, ball != 0, jobs != 0);  // (progress words exist where substep jobs are on)
        printf("%d %d %d %d %u %u\n", (int)p.cut, p.mono, p.len, p.lead, p.jobs_per_pair, p.grid);
    } else {  // n joint_limits regs_build ball
        const v2p::EngineDefaults d = v2p::engine_defaults(atoll(argv[1]), atoi(argv[2]) != 0, atoi(argv[3]) != 0, atoi(argv[4]) != 0);
        printf("%d %d %d %d %ld\n", d.pair_mix_permille, d.job_mono_permille, d.job_len, d.job_lead, d.job_timeout_spins);
    }
    return 0;
}
'''


@pytest.fixture(scope="module")
def exe():
    with tempfile.TemporaryDirectory() as d:
        src = os.path.join(d, "s.cpp")
        open(src, "w").write(PROG)
        path = os.path.join(d, "s")
        subprocess.check_call(["g++", "-std=c++17", "-Wall", "-I", os.path.join(REPO, "vid2player3d_amd", "csrc"), src, "-o", path])
        yield path


def run(exe, args):
    return [int(x) for x in subprocess.check_output([exe] + [str(a) for a in args]).split()]


@pytest.mark.parametrize("name", list(PLANS))
def test_job_plan(exe, name):
    (blocks, nsub, ball, jobs, job_len, job_lead, mono), want = PLANS[name]
    got = run(exe, [blocks, nsub, ball, jobs, 0 if job_len is ENGINE else job_len, -1 if job_lead is ENGINE else job_lead, mono])
    print(name, got)
    if want[4] is None:  # not cut: no pair has jobs
        got[4] = None
    assert tuple(got) == want


@pytest.mark.parametrize("case", list(DEFAULTS))
def test_engine_defaults(exe, case):
    got = run(exe, case)
    print(case, got)
    assert tuple(got[:2]) == DEFAULTS[case]
    assert got[2:] == [0, -1, 50000]
