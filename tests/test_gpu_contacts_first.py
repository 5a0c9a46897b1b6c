"""Contact generation in front of the tree passes (F::CGEN_EARLY of csrc/ll_forms.hpp: the kernels with the visit table run the hull
scan right behind the kinematics, from the pose in registers, and keep only the number of points and the records in LDS for the sweep).
What the order could break and the phase tests of the scan (tests/test_gpu_contact_scan.py) and of the sweep's set-up
(tests/test_gpu_contact_setup.py, whose poses and batches this file reuses) do not single out:

  the records survive passes 2 and 3   their LDS slots are written before the passes park and unpark velocities and pose around them
  no sweep                             an airborne env, alone and beside a partner: nothing is parked for a sweep, v* is the result
  a sweep that never goes live         an env whose points all separate (the feet on the ground, the body rising at 1.5 m/s): rows run,
                                       no impulse, no closing walk; two substeps later the feet are out of reach and there is no sweep
  the pose of EVERY substep            four substeps in one step: a substep's scan must read the pose its own kinematics produced, not the
                                       parked one of the substep before (contact vertex ids of every substep against the oracle)
  batches of 1, 2, 3 and 34            a full pair, a half-empty wave, a mixed batch; both builds; the launch uncut and cut into jobs

PGS, against the float64 C oracle with the kernel's vertices forced: ids exactly in every substep, the state inside rows_all of
tests/gpu_util.py, every env compared.  Env 0 beside different partners: the same bits.  (The TGS, joint-limit and racket + ball
kernels keep the earlier order and their machine code: their own suites cover them.)"""
import functools

import numpy as np
import pytest

from tests import phys_poses as P
from tests import phys_step as S
from tests.phys_poses import NSUB

MODES = [(build, jobs) for build in (1, 2) for jobs in (0, 2)]   # (kernel_build, substep_jobs)
RISE = 1.5   # m/s: 12.5 mm per substep of 1 / 120 s - the sunk feet (2 - 4 mm) stay within the 20 mm contact offset for two substeps
BATCHES = {
    "one_air": (("air", 0),),
    "one_feet": (("feet", 1),),
    "air_feet": (("air", 0), ("feet", 1)),
    "feet_air": (("feet", 1), ("air", 0)),
    "rising": (("rise", 1),),
    "rising_hands": (("rise", 1), ("hands", 0)),
    "hands_rising_sit": (("hands", 0), ("rise", 1), ("sit", 0)),
}
MIXED = ("feet", "air", "hands", "sit", "rise", "flat", "head", "toe_hand")


def env_state(pose, k):
    if pose != "rise":
        return P.well_conditioned(pose, 0, k)
    root, dpos, dvel, wrench = [a.copy() for a in P.well_conditioned("feet", 0, k)]
    root[9] = RISE
    return root, dpos, dvel, wrench


def mixed_batch():
    return tuple((MIXED[e % len(MIXED)], e // len(MIXED)) for e in range(34))


def states(batch):
    return P.stack(env_state(pose, k) for pose, k in batch)


def oracle_for(batch):
    return P.oracle_for(states(batch), solver_type=0)


@functools.lru_cache(maxsize=None)
def own_selection(batch):
    return oracle_for(batch).step(*P.oracle_inputs(states(batch)), nsub=NSUB, hold=2, want_selection=True)


def test_fixtures_are_what_they_claim():
    """CPU, from the oracle alone: the airborne env never has a point; the rising env has points in its first two substeps, none in the
    last, and no contact force at any time; the mixed batch holds every kind."""
    air = own_selection(BATCHES["one_air"])
    assert (air["own"] < 0).all()
    rise = own_selection(BATCHES["rising"])
    pts = (rise["own"][0] >= 0).any(axis=(-1, -2))
    assert pts[0] and pts[1] and not pts[-1], pts
    assert np.abs(rise["cf"]).max() == 0.0, "the rising env's points all separate"
    feet = own_selection(BATCHES["one_feet"])
    assert np.abs(feet["cf"]).max() > 1.0
    mixed = own_selection(mixed_batch())
    touched = (mixed["own"][:, 0] >= 0).any(axis=-1).sum(axis=1)
    assert (touched == 0).sum() >= 4 and (touched >= P.FLAT_MIN_TOUCHED).sum() >= 4 and len(mixed_batch()) == 34
    for name, batch in list(BATCHES.items()) + [("mixed", mixed_batch())]:
        S.assert_oracle_holds_its_own_bound(oracle_for(batch), P.oracle_inputs(states(batch)), own_selection(batch)["own"], name)


@functools.lru_cache(maxsize=None)
def run_kernel(batch, build, jobs):
    """One control step (four substeps) of the kernel from a batch's states.  Shared by the tests; nothing modifies what it returns."""
    st = states(batch)
    return S.kernel_step(*st[:3], P.actions(st), build=build, substep_jobs=jobs)


def _check(batch, build, jobs, what):
    from tests.gpu_util import _compare

    got = run_kernel(batch, build, jobs)
    ref = S.reference(oracle_for(batch), got)
    assert np.array_equal(got["ids_sub"], ref["own"]), "contact vertex ids, every substep"
    _compare(got, ref, "contacts first, %s build %d jobs %d" % (what, build, jobs))
    return got


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(BATCHES))
@pytest.mark.parametrize("build,jobs", MODES)
def test_batches_match_oracle(name, build, jobs):
    batch = BATCHES[name]
    got = _check(batch, build, jobs, name)
    for e, (pose, _) in enumerate(batch):
        pts = (got["ids_sub"][e] >= 0).any(axis=(-1, -2))
        if pose == "air":
            assert not pts.any() and np.abs(got["cf"][e]).max() == 0.0
        if pose == "rise":
            assert pts[0] and pts[1] and not pts[-1] and np.abs(got["cf"][e]).max() == 0.0, "points, but never an impulse"
        if pose in ("feet", "hands", "sit"):
            assert pts.all() and np.abs(got["cf"][e]).max() > 1.0


@pytest.mark.gpu
@pytest.mark.parametrize("build,jobs", MODES)
def test_mixed_batch_of_34_matches_oracle(build, jobs):
    _check(mixed_batch(), build, jobs, "mixed 34")


@pytest.mark.gpu
@pytest.mark.parametrize("build,jobs", MODES)
def test_env0_bits_do_not_depend_on_the_partner(build, jobs):
    """The rising env and the airborne env alone, beside a deep and beside a shallow partner: the same bits."""
    for a in (("rise", 1), ("air", 0)):
        alone = run_kernel((a,), build, jobs)
        seen = []
        for partner in (("hands", 0), ("sit", 0), ("feet", 1)):
            got = run_kernel((a, partner), build, jobs)
            seen.append(got["dvel"][1])
            for key in S.BITS:
                assert np.array_equal(alone[key][0], got[key][0]), (a, partner, key)
        assert not np.array_equal(seen[0], seen[1]) and not np.array_equal(seen[1], seen[2])
