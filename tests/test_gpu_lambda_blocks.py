"""The phases of the link-per-lane physics kernel whose float32 arithmetic was re-formed on 2026-10-20 (csrc/ll_forms.hpp: LAMX, the
Lambda recursion's level by blocks; P2SHIFT, pass 2's shift of cA through cB) and the rows of a contact point, whose `act` test and
normal row a third step of that day formed from one relative velocity (built, not kept: docs/NOTES.md B) - against the float64 C oracle
(oracle/phys).  The tests check the MODEL, not the form: they pass on the library before that change as well.  One control step
(4 substeps x 4 sweeps), builds 1 and 2, the launch uncut and cut into substep jobs, PGS and TGS, batches of 1, 3 and 34 envs; the
bound is rows_all of tests/gpu_util.py with its caps as they are (the air fixture: the flat bound, no conditioning term); env 0 of
every contact fixture keeps its bits beside another partner.

Fixtures (poses, their builder and the oracle set-up: tests/phys_poses.py; the step and its reference: tests/phys_step.py):
  depth d   the deepest touched link of the first substep lies at depth d = 1 .. 8 of the tree, so the recursion runs exactly d levels:
            `sit` 1, `feet` 4, `head` 5, `hands` 8 (poses); 2, 3, 6, 7 from probe bodies whose first link to come near is a knee, an
            ankle, an elbow or a wrist and whose only other link that can come near is the root (as in
            tests/test_gpu_contact_setup.py, rebuilt here; the ankle is new: in the poses a foot's toe comes with it)
  unequal   a depth-8 and a depth-1 env in one wave, both orders: each env's recursion stops at ITS deepest touched link; env 0 also
            beside a standing env instead
  mixed     34 envs: ten poses in turn, the waves pair depths 8 | 1, 4 | 5, 8 | 4, 8 | many stops, none | 4
  air       no contact (tests/test_gpu_tree_passes.py's tumbling body, rebuilt here): pass 2's cA alone decides; flat bound
  rows      `hovering` (every `act` test false), `late` (the left foot's points inactive, the right foot's solved), `wake` (the last stop's
            points turn active within the substep: tests/test_gpu_rows_points.py's, rebuilt here), and `margin`: a standing body set
            MARGIN_GAP above the ground and falling at the speed - found by bisection on the oracle, down to neighbouring float32
            values - at which the normal relative velocity of its first point to be solved is zero with no impulse on it yet: the
            margin at which one rounding of that velocity decides `act`.  Either decision gives that point an impulse of next to
            nothing, so the step stays the oracle's; the CPU test asserts the bisection's two sides.
The CPU tests show that every contact fixture is what it claims and that the float64 oracle, moved by float32 rounding of its inputs,
stays inside the conditioning cap on these inputs on its own (the seeds: SEEDS, chosen on the CPU as tests/test_gpu_tree_passes.py's)."""
import functools

import numpy as np
import pytest

from tests import phys_poses as P
from tests import phys_step as S
from tests.phys_poses import FEET, NB, NSUB, _depths, _names, _quat_of, _rot_expmap, _rot_quat, lowest_point

MODES = [(build, jobs, solver) for build in (1, 2) for jobs in (0, 2) for solver in ("pgs", "tgs")]
SOLVER_TYPE = {"pgs": 0, "tgs": 1}
SEEDS = {"pose": 0, "air": 0, "probe": 1}  # (chosen on the CPU: test_oracle_alone_holds_its_own_bound*; probe seeds 0, 3, 4, 5: the oracle alone
                                               # needs the conditioning term in 2 of 3 envs of one probe)
WAKE_STATE, WAKE_PITCH = 2, 0.012  # (tests/test_gpu_rows_points.py)
MARGIN_GAP = 0.004     # margin: the lowest vertex is this far above the ground, m (contact offset 0.02)
DEPTH_ENVS = {1: ("sit", 0), 4: ("feet", 0), 5: ("head", 0), 8: ("hands", 0)}
ROW_ENVS = {"hovering": ("hover", 0), "late": ("late", 0), "wake": ("wake", 0), "margin": ("margin", 0)}
A_ENVS = dict({"depth%d" % d: e for d, e in DEPTH_ENVS.items()}, **ROW_ENVS)
X, Y = ("feet", 1), ("flat", 1)   # partners: standing (four stops of four points), lying on its back (seven stops or more)
UNEQUAL = {"deep_shallow": (("hands", 0), ("sit", 0)), "shallow_deep": (("sit", 0), ("hands", 0))}
MIXED_POSES = ("hands", "sit", "feet", "head", "toe_hand", "ankle_toe", "head_hand", "flat", "hover", "late")
MIXED = tuple((p, k) for k in range(4) for p in MIXED_POSES)[:34]
GRID = 1024.0
DEEP_LINKS = {2: ("L_Knee", 2), 3: ("L_Ankle", 3), 16: ("L_Elbow", 6), 17: ("L_Wrist", 7)}   # link -> (name, depth): asserted on the CPU
DEEP_COUNTS = (1, 2, 1)  # near links per env: the deep link alone | with the root | alone in the second wave
DEEP_COUNTS_OTHER = (1, 1, 2)  # ... env 0 beside another second env (partner independence)


def batches_of(a):
    """The batches a contact fixture runs in: alone, beside X with Y in a second wave, beside Y with X in a second wave."""
    A = A_ENVS[a]
    return {1: (A,), 3: (A, X, Y), "other": (A, Y, X)}


# ---------------------------------------------------------------------------------------------------------------- states
@functools.lru_cache(maxsize=None)
def wake_state(k):
    root, dpos, dvel, wrench = [a.copy() for a in P.state("feet", SEEDS["pose"], WAKE_STATE + k)]
    sink = np.random.default_rng([131, SEEDS["pose"], WAKE_STATE + k]).uniform(*P.SINK)
    root[3:7] = _quat_of(_rot_expmap(P.X * WAKE_PITCH) @ _rot_quat(root[3:7])).astype(np.float32)
    root[2] = -lowest_point(root[3:7], dpos).min() - sink
    return root, dpos, dvel, wrench


def _lifted(k, vz):
    root, dpos, dvel, wrench = [a.copy() for a in P.well_conditioned("feet", SEEDS["pose"], k)]
    root[2] = -lowest_point(root[3:7], dpos).min() + MARGIN_GAP
    root[9] = np.float32(vz)
    return root, dpos, dvel, wrench


def _first_sweep_load(st):
    """Largest contact force after ONE substep of ONE sweep of the oracle, one env alone."""
    b = P.stack([st])
    return float(np.abs(P.oracle_for(b, solver_type=0, n_iter=1).step(*P.oracle_inputs(b), nsub=1, hold=2)["cf"]).max())


@functools.lru_cache(maxsize=None)
def margin_speeds(k):
    """Neighbouring float32 values of the root's vertical velocity: at the first no point of the lifted standing body is solved in the first
    sweep of the first substep (every point separates, given the bias of its gap), at the second one point is."""
    lo, hi = np.float32(0.0), np.float32(-8.0)
    assert _first_sweep_load(_lifted(k, lo)) == 0.0 and _first_sweep_load(_lifted(k, hi)) > 0.0
    while np.nextafter(lo, hi) != hi:
        mid = np.float32(0.5 * (np.float64(lo) + np.float64(hi)))
        lo, hi = (mid, hi) if _first_sweep_load(_lifted(k, mid)) == 0.0 else (lo, mid)
    return lo, hi


@functools.lru_cache(maxsize=None)
def air_state(k):
    """(tests/test_gpu_tree_passes.py: every joint bent by 0.15 .. 0.45 rad, joint rates of ~1 rad/s, tumbling, 3 m up)"""
    rng = np.random.default_rng([0, SEEDS["air"], k])
    root = np.zeros(13)
    q = np.array([np.sin(np.pi / 4), 0.0, 0.0, np.cos(np.pi / 4)]) + rng.normal(0, 0.3, size=4)
    dpos = rng.uniform(0.15, 0.45, size=69) * rng.choice([-1.0, 1.0], size=69) / np.sqrt(3.0)
    dvel = rng.normal(0, 1.0, size=69)
    root[7:10] = rng.normal(0, 0.5, size=3)
    root[10:13] = rng.normal(0, 1.0, size=3)
    root[3:7] = q / np.linalg.norm(q)
    root[2] = 3.0
    return root.astype(np.float32), dpos.astype(np.float32), dvel.astype(np.float32), rng.normal(0, 0.17, size=6).astype(np.float32)


@functools.lru_cache(maxsize=None)
def env_state(pose, k):
    if pose == "wake":
        return wake_state(k)
    if pose == "margin":
        return _lifted(k, margin_speeds(k)[1])
    if pose == "tumble":
        return air_state(k)
    return P.well_conditioned(pose, SEEDS["pose"], k)


def states(batch):
    return P.stack(env_state(pose, k) for pose, k in batch)


def oracle_for(batch, solver="pgs", **params):
    return P.oracle_for(states(batch), solver_type=SOLVER_TYPE[solver], **params)


def air_batch(n):
    return tuple(("tumble", k) for k in P.STATE_IDS[n]) if n > 1 else (("tumble", 0),)


# ---------------------------------------------------------------------------------------------------------------- the probe bodies
@functools.lru_cache(maxsize=None)
def probe_model(first):
    """The baked body with link origins on a 1/1024 m grid and a plate of candidate vertices under every link (level lv at
    (s + lv) / 1024 m when the root stands at 1 + s / 1024): `first` comes near first, the root second, and no other link ever does."""
    from vid2player3d_amd.model import BodyModel, load_baked_model

    base = load_baked_model()
    rng = np.random.default_rng([31, 9, first, SEEDS["probe"]])
    blob = dict(base.blob)
    local = np.round(np.asarray(base.blob["local_pos"], dtype=np.float64) * GRID) / GRID
    blob["local_pos"] = local
    blob["com"] = np.round(np.asarray(base.blob["com"], dtype=np.float64) * GRID) / GRID
    origin = np.zeros((NB, 3))
    for b in range(1, NB):
        origin[b] = origin[int(base.parents[b])] + local[b]
    rest = [(7 * lv + 3) % NB for lv in range(NB)]
    rest.remove(first)
    rest.remove(0)
    link_of_level = [first, 0] + rest
    sizes = [(6, 64), (1, 3), (3, 7), (5, 12), (4, 9), (2, 2), (8, 33), (1, 1)]
    specs = [(5, 9)] + [sizes[lv % len(sizes)] for lv in range(NB - 1)]
    level_of = {link: lv for lv, link in enumerate(link_of_level)}
    verts, offs = [], [0]
    for b in range(NB):
        lv = level_of[b]
        k, nv = specs[lv]
        hv = np.zeros((nv, 3))
        where = np.sort(rng.permutation(nv)[:k])
        top = np.ones(nv, dtype=bool)
        top[where] = False
        hv[where, :2] = rng.integers(-780, 781, size=(k, 2)) / 4096.0
        dz = rng.permutation(np.arange(8))[:k] / 65536.0
        hv[where, 2] = lv / GRID - 1.0 - origin[b, 2] + dz + (0.125 if lv >= 2 else 0.0)
        nt = int(top.sum())
        hv[top, :2] = rng.integers(-16, 17, size=(nt, 2)) / 64.0
        hv[top, 2] = lv / GRID - 1.0 - origin[b, 2] + 0.25 + rng.integers(0, 32, size=nt) / 64.0
        verts.append(hv)
        offs.append(offs[-1] + nv)
    blob["hull_verts"] = np.concatenate(verts, axis=0)
    blob["hull_offsets"] = np.asarray(offs, dtype=np.int32)
    return BodyModel(blob, **base.model_kw)


def probe_states(counts=DEEP_COUNTS):
    """Upright, identity rotations, the root at the height that brings exactly counts[e] links within the contact offset, falling and
    tumbling slowly."""
    n = len(counts)
    root = np.zeros((n, 13), dtype=np.float32)
    for e, c in enumerate(counts):
        root[e, 2] = 1.0 + (21 - c) / GRID
    root[:, 6] = 1.0
    root[:, 7:10] = [0.0625, -0.03125, -0.5]
    root[:, 10:13] = [0.125, 0.0625, 0.03125]
    return root, np.zeros((n, 69), dtype=np.float32), np.zeros((n, 69), dtype=np.float32)


def probe_oracle(first, solver="pgs"):
    return P.oracle_for(probe_states(), model=probe_model(first), enable_contact=True, solver_type=SOLVER_TYPE[solver])


def deepest(ids_sub):
    """Depth of the deepest touched link of every env in the first substep (-1: none)."""
    touched = (ids_sub[:, 0] >= 0).any(axis=-1)
    return np.where(touched, _depths()[None, :], -1).max(axis=1)


# ---------------------------------------------------------------------------------------------------------------- CPU
def _own(oracle, inputs):
    return oracle.step(*inputs, nsub=NSUB, hold=2, want_selection=True)["own"]


def test_depth_fixtures_reach_every_depth():
    """CPU: the deepest touched link of the first substep is at depth 1, 4, 5, 8 (poses), 2, 3, 6, 7 (probes; the second env's root does
    not change it), 8 | 1 and 1 | 8 in the unequal pairs; the mixed batch holds the pairs its docstring names."""
    for d, env in DEPTH_ENVS.items():
        assert deepest(_own(oracle_for((env,)), P.oracle_inputs(states((env,))))).tolist() == [d]
    dep, names = _depths(), _names()
    z = np.zeros((3, 69))
    for first, (name, d) in DEEP_LINKS.items():
        assert (names[first], int(dep[first])) == (name, d)
        own = probe_oracle(first).step(z, np.zeros((3, 3)), np.zeros((3, 3)), nsub=NSUB, hold=2, want_selection=True)["own"]
        assert deepest(own).tolist() == [d, d, d]
        assert [np.nonzero((own[e, 0] >= 0).any(axis=-1))[0].tolist() for e in range(3)] == [[first], sorted([0, first]), [first]]
        other = P.oracle_for(probe_states(DEEP_COUNTS_OTHER), model=probe_model(first), enable_contact=True, solver_type=0)
        own = other.step(z, np.zeros((3, 3)), np.zeros((3, 3)), nsub=NSUB, hold=2, want_selection=True)["own"]
        assert [np.nonzero((own[e, 0] >= 0).any(axis=-1))[0].tolist() for e in range(3)] == [[first], [first], sorted([0, first])]
    assert sorted(list(DEPTH_ENVS) + [d for _, d in DEEP_LINKS.values()]) == [1, 2, 3, 4, 5, 6, 7, 8] and DEPTH_ENVS[1][0] == "sit"
    for name, batch in UNEQUAL.items():
        assert deepest(_own(oracle_for(batch), P.oracle_inputs(states(batch)))).tolist() == ([8, 1] if name == "deep_shallow" else [1, 8])
    dm = deepest(_own(oracle_for(MIXED), P.oracle_inputs(states(MIXED))))
    assert dm[:7].tolist() == [8, 1, 4, 5, 8, 4, 8] and dm[8:10].tolist() == [4, 4] and len(MIXED) == 34, dm.tolist()


def test_row_fixtures_are_what_they_claim():
    """CPU, from one substep of the oracle per env: hovering solves nothing, late only its right foot, wake its last stop from a later
    sweep on; margin: neighbouring float32 speeds, no point solved at the one, one point - with next to no impulse - at the other."""
    names = _names()
    feet = sorted(names.index(c) for c in FEET)

    def load(env, n_iter):
        b = (env,)
        return np.abs(oracle_for(b, n_iter=n_iter).step(*P.oracle_inputs(states(b)), nsub=1, hold=2)["cf"][0]).max(axis=-1)

    assert load(ROW_ENVS["hovering"], 4).max() == 0.0
    fl = load(ROW_ENVS["late"], 4)
    assert (fl[feet[:2]] == 0).all() and fl[feet[2:]].max() > 0
    f1, f4 = load(ROW_ENVS["wake"], 1), load(ROW_ENVS["wake"], 4)
    assert f1[feet[3]] == 0 and (f1[feet[:3]] > 0).all() and f4[feet[3]] > 1.0
    lo, hi = margin_speeds(0)
    assert np.nextafter(lo, hi) == hi and lo > hi
    f_lo, f_hi = _first_sweep_load(_lifted(0, lo)), _first_sweep_load(_lifted(0, hi))
    print("[lambda blocks] margin: root vz %.9g | %.9g m/s, load after the first sweep %.3g | %.3g N" % (lo, hi, f_lo, f_hi))
    # (a standing body carries ~700 N: the impulse of the point at the margin is the float32 step of the speed through its row)
    assert f_lo == 0.0 and 0.0 < f_hi < 0.05
    b = (ROW_ENVS["margin"],)  # (the body reaches the ground at the end of the first substep: the load comes in the later ones)
    assert np.abs(oracle_for(b).step(*P.oracle_inputs(states(b)), nsub=NSUB, hold=2)["cf"][0][feet]).max() > 1.0


def _contact_batches():
    out = {}
    for a in A_ENVS:
        for size, batch in batches_of(a).items():
            out["%s/%s" % (a, size)] = batch
    out.update(UNEQUAL)
    out["mixed"] = MIXED
    return out


@pytest.mark.parametrize("name", list(_contact_batches()))
@pytest.mark.parametrize("solver", ["pgs", "tgs"])
def test_oracle_alone_holds_its_own_bound(name, solver):
    """CPU: the float64 oracle, its inputs moved by float32 rounding, against itself stays inside the cap of rows_all on every batch."""
    batch = _contact_batches()[name]
    inputs = P.oracle_inputs(states(batch))
    S.assert_oracle_holds_its_own_bound(oracle_for(batch, solver), inputs, _own(oracle_for(batch, solver), inputs), "%s %s" % (name, solver))


@pytest.mark.parametrize("first", list(DEEP_LINKS))
@pytest.mark.parametrize("solver", ["pgs", "tgs"])
def test_oracle_alone_holds_its_own_bound_on_the_probes(first, solver):
    z = (np.zeros((3, 69)), np.zeros((3, 3)), np.zeros((3, 3)))
    S.assert_oracle_holds_its_own_bound(probe_oracle(first, solver), z, _own(probe_oracle(first, solver), z), "probe %d %s" % (first, solver))


# ---------------------------------------------------------------------------------------------------------------- GPU
@functools.lru_cache(maxsize=None)
def run_kernel(batch, build, jobs, solver, contact=True):
    """One control step of the kernel from a batch's states.  Shared by the tests; nothing modifies what it returns."""
    st = states(batch)
    return S.kernel_step(*st[:3], P.actions(st), build=build, solver=solver, contact=contact, substep_jobs=jobs)


@functools.lru_cache(maxsize=None)
def _reference(batch, solver, ids_bytes):
    got = run_kernel(batch, 1, 0, solver)
    ids = np.frombuffer(ids_bytes, dtype=got["ids_sub"].dtype).reshape(got["ids_sub"].shape)
    return S.reference(oracle_for(batch, solver), dict(got, ids_sub=ids))


def compare(batch, build, jobs, solver, what):
    """The oracle's step from the same state with the kernel's contact vertices forced, once per batch, solver and selection."""
    from tests.gpu_util import _compare

    got = run_kernel(batch, build, jobs, solver)
    base = run_kernel(batch, 1, 0, solver)
    for key in ("pd", "force", "torque"):
        assert np.array_equal(got[key], base[key]), key
    ref = _reference(batch, solver, got["ids_sub"].tobytes())
    _compare(got, ref, "%s build %d jobs %d %s" % (what, build, jobs, solver))
    return got, ref


@pytest.mark.gpu
@pytest.mark.parametrize("d", list(DEPTH_ENVS))
@pytest.mark.parametrize("n", [1, 3])
@pytest.mark.parametrize("build,jobs,solver", MODES)
def test_recursion_of_d_levels_matches_oracle(d, n, build, jobs, solver):
    batch = batches_of("depth%d" % d)[n]
    got, _ = compare(batch, build, jobs, solver, "lambda depth %d n=%d" % (d, n))
    assert deepest(got["ids_sub"])[0] == d
    assert np.abs(got["cf"][0]).max() > 1.0, "the contacts must carry load"


@functools.lru_cache(maxsize=None)
def run_probe(first, build, jobs, solver):
    got = S.kernel_step(*probe_states(), np.zeros((3, 75), dtype=np.float32), build=build, solver=solver, body_model=probe_model(first), substep_jobs=jobs)
    return got, S.reference(probe_oracle(first, solver), got)


@pytest.mark.gpu
@pytest.mark.parametrize("first", list(DEEP_LINKS))
@pytest.mark.parametrize("build,jobs,solver", MODES)
def test_recursion_to_a_knee_an_ankle_an_elbow_a_wrist_matches_oracle(first, build, jobs, solver):
    """Depths 2, 3, 6 and 7: three envs, the second with the root beside the deep link, the third alone in its wave."""
    from tests.gpu_util import _compare

    got, ref = run_probe(first, build, jobs, solver)
    assert deepest(got["ids_sub"]).tolist() == [DEEP_LINKS[first][1]] * 3
    assert np.array_equal(got["ids_sub"], ref["own"]), "contact vertex ids, every substep"
    assert np.abs(got["cf"]).max() > 1.0, "the contacts must carry load"
    _compare(got, ref, "lambda depth %d (probe) build %d jobs %d %s" % (DEEP_LINKS[first][1], build, jobs, solver))


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(UNEQUAL))
@pytest.mark.parametrize("build,jobs,solver", MODES)
def test_each_env_stops_at_its_own_depth(name, build, jobs, solver):
    """A depth-8 and a depth-1 env in one wave: each against the oracle, and env 0 with the bits it has alone (the two orders make
    each of them env 0 once; an env in the wave's second half is not held to the bits it has in the first)."""
    batch = UNEQUAL[name]
    got, _ = compare(batch, build, jobs, solver, "lambda " + name)
    assert deepest(got["ids_sub"]).tolist() == ([8, 1] if name == "deep_shallow" else [1, 8])
    alone = run_kernel(batch[:1], build, jobs, solver)
    for key in S.BITS:
        assert np.array_equal(alone[key][0], got[key][0]), (name, key)
    S.assert_env0_ignores_its_partner(got, run_kernel((batch[0], X), build, jobs, solver))


@pytest.mark.gpu
@pytest.mark.parametrize("build,jobs,solver", MODES)
def test_mixed_batch_of_34_matches_oracle(build, jobs, solver):
    got, _ = compare(MIXED, build, jobs, solver, "lambda mixed n=34")
    assert deepest(got["ids_sub"])[:7].tolist() == [8, 1, 4, 5, 8, 4, 8]


@pytest.mark.gpu
@pytest.mark.parametrize("n", [1, 3, 34])
@pytest.mark.parametrize("build", [1, 2])
@pytest.mark.parametrize("jobs", [0, 2])
def test_air_matches_oracle_at_the_flat_bound(n, build, jobs):
    """No contact: pass 2 (with cA's shift), the root solve, pass 3 and the integrator alone; every element of every env within the
    flat bounds of tests/gpu_util.py, no conditioning term."""
    from tests.gpu_util import FORCE_ATOL, FORCE_RTOL, POS_ATOL, VEL_ATOL, VEL_RTOL, assert_none_over, rows_close

    batch = air_batch(n)
    got = run_kernel(batch, build, jobs, "pgs", False)
    ref = _air_reference(batch)
    what = "lambda air n=%d build %d jobs %d" % (n, build, jobs)
    assert np.abs(got["cf"]).max() == 0.0
    qs = np.sign(np.sum(got["rb"][..., 3:7] * ref["rb"][..., 3:7], axis=-1, keepdims=True))  # quaternion sign is arbitrary
    bad = rows_close(got["root"][:, :3], ref["root"][:, :3], POS_ATOL, 0.0, what + " root pos")
    bad |= rows_close(got["dpos"], ref["dpos"], 5e-5, 0.0, what + " dof_pos")
    bad |= rows_close(got["rb"][..., :3], ref["rb"][..., :3], POS_ATOL, 0.0, what + " rb pos")
    bad |= rows_close(got["rb"][..., 3:7] * qs, ref["rb"][..., 3:7], POS_ATOL, 0.0, what + " rb rot")
    bad |= rows_close(got["root"][:, 7:], ref["root"][:, 7:], VEL_ATOL, VEL_RTOL, what + " root vel")
    bad |= rows_close(got["dvel"], ref["dvel"], VEL_ATOL, VEL_RTOL, what + " dof_vel")
    bad |= rows_close(got["rb"][..., 7:], ref["rb"][..., 7:], VEL_ATOL, VEL_RTOL, what + " rb vel")
    bad |= rows_close(got["df"], ref["df"], FORCE_ATOL, FORCE_RTOL, what + " dof force")
    assert_none_over(bad, what)


@functools.lru_cache(maxsize=None)
def _air_reference(batch):
    got = run_kernel(batch, 1, 0, "pgs", False)
    return S.reference(P.oracle_for(states(batch), enable_contact=False), got, contact=False)


@pytest.mark.gpu
@pytest.mark.parametrize("a", list(ROW_ENVS))
@pytest.mark.parametrize("n", [1, 3])
@pytest.mark.parametrize("build,jobs,solver", MODES)
def test_rows_match_oracle(a, n, build, jobs, solver):
    """Points whose `act` test is false, turns true within the substep, or sits at the margin of one float32 rounding."""
    batch = batches_of(a)[n]
    got, ref = compare(batch, build, jobs, solver, "rows %s n=%d" % (a, n))
    loaded = np.abs(got["cf"][0]).max() > 1.0
    assert loaded == (a != "hovering") and (np.abs(ref["cf"][0]).max() > 1.0) == loaded


@pytest.mark.gpu
@pytest.mark.parametrize("a", list(A_ENVS))
@pytest.mark.parametrize("build,jobs,solver", MODES)
def test_env0_ignores_its_partner(a, build, jobs, solver):
    """Env 0 of every contact fixture beside a standing and beside a lying env: the same bits."""
    b = batches_of(a)
    S.assert_env0_ignores_its_partner(run_kernel(b[3], build, jobs, solver), run_kernel(b["other"], build, jobs, solver))


@pytest.mark.gpu
@pytest.mark.parametrize("first", list(DEEP_LINKS))
@pytest.mark.parametrize("build,jobs,solver", MODES)
def test_probe_env0_ignores_its_partner(first, build, jobs, solver):
    """Env 0 of the probe bodies (the deep link alone) beside an env with the root on the ground as well and beside one without."""
    other = S.kernel_step(*probe_states(DEEP_COUNTS_OTHER), np.zeros((3, 75), dtype=np.float32), build=build, solver=solver, body_model=probe_model(first),
                          substep_jobs=jobs)
    S.assert_env0_ignores_its_partner(run_probe(first, build, jobs, solver)[0], other)
