"""The rows of the contact sweep (the block update of the link the walk stands on, link-per-lane physics kernel): the up to four points of
the two stops of a visit, each with three rows, and which of them run.  A point exists for a lane when the lane's link has that many
points; it is solved when it carries a normal impulse or is not separating.  One control step (4 substeps x 4 sweeps), PGS, both builds
of the kernel, with the launch uncut and cut into substep jobs, batches of 1, 2 and 3 envs (a wave with one env, a wave with two, a lone
env in a second wave) - against the float64 C oracle (oracle/phys) with the bound rows_all of tests/gpu_util.py, and bit for bit
between batches.  Poses, their builder, the states that keep every hull vertex MARGIN away from the contact offset and the oracle set-up
are those of tests/phys_poses.py, the step and its reference those of tests/phys_step.py; `wake` is new here.

An env is (pose, state number); a batch is a list of envs:
  partner   env A's bits are the same alone, beside X (standing: four stops of four points), beside Y (lying on its back: nine stops,
            stops of 1 and 3 points), beside Z (hovering: every point inactive).  A is standing,
            on one foot (ankle + toe), `late` (its left foot hovers: in visits 0 and 1 its points are inactive while X's are solved),
            hovering (the reverse: every point inactive beside partners that solve theirs), fallen (`flat2`), and `wake`
  counts    pairs whose k-th stops have (1, 4), (4, 1), (2, 3), (3, 2), (4, 4), (1, 1), (3, 3) and more points; the standing env has four
            stops and rests in the lying env's surplus visits
  wake      a standing env pitched by 12 mrad: in the first sweep of the first substep the points of its LAST stop (R_Toe) carry no impulse
            and separate, the impulses of the other three links push them in, and from a later sweep on they are solved (the CPU test
            asserts it from one substep of the oracle with one sweep and with four: no load on R_Toe after one, load after four)
  nothing   a wave in which both envs hover: every point of every visit is inactive, the first sweep changes nothing and both are
            struck out; the step is the oracle's and no link carries load
test_fixtures_are_what_they_claim checks on the CPU what the names say."""
import functools

import numpy as np
import pytest

from tests import phys_poses as P
from tests import phys_step as S
from tests.phys_poses import FEET, NSUB, _names, _quat_of, _rot_expmap, _rot_quat, lowest_point

WAKE_STATE, WAKE_PITCH = 2, 0.012   # wake: which `feet` state, and its pitch about the body's left axis, rad (found on the CPU: see the fixture test)
MODES = [(build, jobs) for build in (1, 2) for jobs in (0, 2)]   # (kernel_build, substep_jobs)
X, Y, Z = ("feet", 1), ("flat", 1), ("hover", 1)
A_ENVS = {"standing": ("feet", 0), "one_foot": ("ankle_toe", 0), "late": ("late", 0), "hovering": ("hover", 0), "fallen": ("flat2", 2), "wake": ("wake", 0)}
COUNT_BATCHES = {
    "lying_standing": [("flat", 0), ("feet", 0)],               # (4, 4), (1, 4), then the standing env rests
    "standing_lying": [("feet", 0), ("flat", 0)],               # (4, 1)
    "two_three": [("flat2", 0), ("flat", 0)],                   # (2, 3) in visit 5, (1, 1), (3, 3)
    "three_two_lone": [("flat", 0), ("flat2", 0), ("flat2", 2)],  # (3, 2); a lone env with stops of 1, 2 and 4 points in the second wave
    "fallen_lying": [("flat2", 2), ("flat", 0)],                # (1, 4), (2, 1), (2, 4), (4, 3)
    "lone": [("flat", 0)],
}
WAKE_BATCHES = {"alone": [("wake", 0)], "pair": [("wake", 0), ("feet", 1)], "second_wave": [("feet", 1), ("hover", 1), ("wake", 0)]}
NOTHING_BATCHES = {"one": [("hover", 0)], "two": [("hover", 0), ("hover", 1)], "three": [("hover", 0), ("hover", 1), ("hover", 2)]}
REQUIRED_COUNTS = {(1, 4), (4, 1), (2, 3), (4, 4)}


@functools.lru_cache(maxsize=None)
def wake_state(seed, k):
    """`feet` state WAKE_STATE + k of tests/phys_poses.py, pitched by WAKE_PITCH about the body's left axis and set down again
    (the lowest vertex as deep in the ground as a draw of P.SINK)."""
    root, dpos, dvel, wrench = [a.copy() for a in P.state("feet", seed, WAKE_STATE + k)]
    sink = np.random.default_rng([131, seed, WAKE_STATE + k]).uniform(*P.SINK)
    root[3:7] = _quat_of(_rot_expmap(P.X * WAKE_PITCH) @ _rot_quat(root[3:7])).astype(np.float32)
    root[2] = -lowest_point(root[3:7], dpos).min() - sink
    return root, dpos, dvel, wrench


@functools.lru_cache(maxsize=None)
def env_state(pose, k):
    return wake_state(0, k) if pose == "wake" else P.well_conditioned(pose, 0, k)


def states(batch):
    return P.stack(env_state(pose, k) for pose, k in batch)


def oracle_for(batch, **params):
    return P.oracle_for(states(batch), solver_type=0, **params)


def oracle_inputs(batch):
    return P.oracle_inputs(states(batch))


@functools.lru_cache(maxsize=None)
def first_substep(env, n_iter):
    """One env alone, ONE substep of the oracle with n_iter sweeps: its stops, their numbers of points, the load of every link."""
    batch = (env,)
    out = oracle_for(batch, n_iter=n_iter).step(*oracle_inputs(batch), nsub=1, hold=2, want_selection=True)
    cnt = (out["own"][0, 0] >= 0).sum(axis=-1)
    stops = [int(b) for b in np.nonzero(cnt)[0]]
    return stops, [int(cnt[b]) for b in stops], np.abs(out["cf"][0]).max(axis=-1)


def visit_counts(batch):
    """The numbers of points of the k-th stops of the two envs of every wave of a batch, visit by visit (0: the env rests or is absent)."""
    out = []
    for e in range(0, len(batch), 2):
        c = [first_substep(env, 4)[1] for env in batch[e:e + 2]] + [[]] * (2 - len(batch[e:e + 2]))
        out += [(c[0][k] if k < len(c[0]) else 0, c[1][k] if k < len(c[1]) else 0) for k in range(max(len(c[0]), len(c[1])))]
    return out


def test_fixtures_are_what_they_claim():
    """CPU, from one substep of the oracle per env."""
    names = _names()
    feet = [names.index(c) for c in FEET]
    # partners: X has four stops of four points and solves them all, Y has more stops and stops of 1 - 3 points, Z solves nothing
    sx, cx, fx = first_substep(X, 4)
    sy, cy, fy = first_substep(Y, 4)
    sz, cz, fz = first_substep(Z, 4)
    assert sx == sorted(feet) and cx == [4, 4, 4, 4] and (fx[sx] > 0).all()
    assert len(sy) > 4 and {1, 3} <= set(cy) and (fy > 0).any()
    assert sz == sorted(feet) and fz.max() == 0.0
    # `late`: the points of its first two stops are inactive in every sweep (beside X, which solves its first two stops), the others not
    sl, cl, fl = first_substep(A_ENVS["late"], 4)
    assert sl == sorted(feet) and (fl[sl[:2]] == 0).all() and fl[sl[2:]].max() > 0
    assert first_substep(A_ENVS["hovering"], 4)[2].max() == 0.0
    assert {1, 2, 4} <= set(first_substep(A_ENVS["fallen"], 4)[1])
    # counts: every required combination of the two stops of a visit, and a visit in which one env rests
    seen = set()
    for b in COUNT_BATCHES.values():
        seen |= set(visit_counts(b))
    assert REQUIRED_COUNTS | {(3, 2), (1, 1), (3, 3)} <= seen, sorted(seen)
    assert any(a > 0 and b == 0 for a, b in visit_counts(COUNT_BATCHES["lying_standing"]))
    assert {1, 2, 4} <= {a for a, _ in visit_counts(COUNT_BATCHES["three_two_lone"][2:])}
    # wake: no load on the last stop after one sweep, load after four; the other three carry load after one
    sw, cw, f1 = first_substep(A_ENVS["wake"], 1)
    f4 = first_substep(A_ENVS["wake"], 4)[2]
    assert sw == sorted(feet) and cw == [4, 4, 4, 4]
    assert f1[sw[3]] == 0 and (f1[sw[:3]] > 0).all() and f4[sw[3]] > 1.0, (f1[sw], f4[sw])
    # nothing: no env of these batches ever applies an impulse
    for b in NOTHING_BATCHES.values():
        out = oracle_for(tuple(b)).step(*oracle_inputs(tuple(b)), nsub=NSUB, hold=2)
        assert np.abs(out["cf"]).max() == 0.0


# ---------------------------------------------------------------------------------------------------------------- GPU
@functools.lru_cache(maxsize=None)
def run_kernel(batch, build, jobs):
    """One control step of the kernel from a batch's states.  Shared by the tests; nothing modifies what it returns."""
    st = states(batch)
    return S.kernel_step(*st[:3], P.actions(st), build=build, substep_jobs=jobs)


@functools.lru_cache(maxsize=None)
def _reference(batch, ids_bytes):
    got = run_kernel(batch, 1, 0)
    ids = np.frombuffer(ids_bytes, dtype=got["ids_sub"].dtype).reshape(got["ids_sub"].shape)
    return S.reference(oracle_for(batch), dict(got, ids_sub=ids))


def reference(batch, got):
    """The oracle's step from the same state with the kernel's contact vertices forced: computed once per batch and selection (the
    builds and the cut launch select the same vertices, and their PD targets and wrenches are the same bits)."""
    base = run_kernel(batch, 1, 0)
    for key in ("pd", "force", "torque"):
        assert np.array_equal(got[key], base[key]), key
    return _reference(batch, got["ids_sub"].tobytes())


def compare(batch, build, jobs, what):
    from tests.gpu_util import _compare

    got = run_kernel(batch, build, jobs)
    ref = reference(batch, got)
    assert np.array_equal((got["ids_sub"][:, 0] >= 0).sum(axis=-1), (ref["own"][:, 0] >= 0).sum(axis=-1))
    _compare(got, ref, "%s build %d jobs %d" % (what, build, jobs))
    return got, ref


@pytest.mark.gpu
@pytest.mark.parametrize("a", list(A_ENVS))
@pytest.mark.parametrize("build,jobs", MODES)
def test_env_bits_do_not_depend_on_the_partner(a, build, jobs):
    """Env A alone, beside X, beside Y and beside Z: the same bits.  (As the lone env of a SECOND wave, batch (X, Y, A), its bits are not
    those of the one-env batch, with this change and without it - cause not looked for here; the three-env batches of the other tests
    compare that env against the oracle.)"""
    A = A_ENVS[a]
    alone = run_kernel((A,), build, jobs)
    partners = []
    for batch, e in (((A, X), 0), ((A, Y), 0), ((A, Z), 0)):
        got = run_kernel(batch, build, jobs)
        partners.append(got["dvel"][1])
        for key in S.BITS:
            assert np.array_equal(alone[key][0], got[key][e]), (a, batch, key)
    assert not np.array_equal(partners[0], partners[1]) and not np.array_equal(partners[0], partners[2]), "the partners must differ"
    loaded = np.abs(alone["cf"]).max() > 1.0
    assert loaded == (a != "hovering")


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(COUNT_BATCHES))
@pytest.mark.parametrize("build,jobs", MODES)
def test_point_counts_match_oracle(name, build, jobs):
    """Stops of 1 - 4 points beside stops of 1 - 4 points, and an env that rests: every env's step is the oracle's."""
    batch = tuple(COUNT_BATCHES[name])
    got, _ = compare(batch, build, jobs, "counts " + name)
    assert (np.abs(got["cf"]).reshape(len(batch), -1).max(axis=1) > 1.0).all(), "the contacts must carry load"


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(WAKE_BATCHES))
@pytest.mark.parametrize("build,jobs", MODES)
def test_point_that_wakes_up_matches_oracle(name, build, jobs):
    """The points of the env's last stop are inactive in the first sweep and solved in a later one."""
    batch = tuple(WAKE_BATCHES[name])
    got, _ = compare(batch, build, jobs, "wake " + name)
    e = batch.index(A_ENVS["wake"])
    feet = [_names().index(c) for c in FEET]
    assert (np.abs(got["cf"][e][feet]).max(axis=-1) > 0).all(), "both feet must carry load at the end of the step"


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(NOTHING_BATCHES))
@pytest.mark.parametrize("build,jobs", MODES)
def test_nothing_to_do_matches_oracle(name, build, jobs):
    """Every point of every visit is inactive for both stops: no impulse, no load, the oracle's step."""
    batch = tuple(NOTHING_BATCHES[name])
    got, ref = compare(batch, build, jobs, "nothing " + name)
    assert np.abs(got["cf"]).max() == 0.0 and np.abs(ref["cf"]).max() == 0.0
    assert (got["ids_sub"][:, 0] >= 0).any(axis=-1).sum(axis=-1).tolist() == [4] * len(batch), "every env has its four stops"
