"""What lies between pass 3 and the first visit of the contact sweep in the link-per-lane physics kernel, beside what
tests/test_gpu_contact_scan.py (the hull scan) and tests/test_gpu_sweep_visits.py (the visit table) already pin: the depth of each env's
deepest stop (a reduction over the lanes' own depths), the visit words formed by the stops' own lanes, the hull list at the END of the
vertex table, and the points of a wave with one point / with four points on every link.  One control step (4 substeps x 4 sweeps), PGS,
both builds, the launch uncut and cut into substep jobs, batches of 1 - 3 envs, against the float64 C oracle (oracle/phys): contact
vertex ids exactly in every substep, the state inside rows_all of tests/gpu_util.py; env 0 alone and beside a partner: same bits.

Depths (poses of tests/phys_poses.py; depths of the SMPL tree: Pelvis 0, Torso 1, Toe 4, Head 5, Hand 8):
  deep_shallow / shallow_deep   hands on the ground (deepest stop at depth 8) beside an env sitting on Pelvis and Torso (depth 1), and
                                the reverse: each env's Lambda recursion, its sweep and its closing pass stop at ITS depth
  none_many / many_none         an airborne env (no stop) beside one lying on its back (seven stops or more)
  deepest_last                  L_Toe (4) then R_Hand (8): the deepest stop is the last touched link
  deepest_first_last            both hands (8, 8): the first and the last; beside an env on its head (5)
  deepest_middle                lying on the back: the hands (8) stand between shallower stops on either side
  second_wave                   three envs: the third is alone in its wave
The poses reach deepest stops at depths 1, 4, 5 and 8 (and stops at 0 and 3).  Depths 2, 6 and 7 come from probe bodies (below) whose
first link to come near is a knee, an elbow or a wrist and whose only other link that can come near is the root: `deep`, env 0 with
that link alone, env 1 with the root beside it, env 2 alone in its wave - the deepest stop at every depth 1 .. 8.
The pairing key of the last substep (touched links x 8 + depth of the deepest, capped at 7) is read back through `debug_pairing` from
batches with pairing on: the poses and the `deep` probes, every value 0 .. 7 but 3.

Hull lists (a probe body as in tests/test_gpu_contact_scan.py: every link carries a plate of K candidates at its own level): the LAST
list of the vertex table - link 23's - has 1, 7, 8, 9, 63 or 64 vertices and is the first to come near; 5 + 4 near links pooled in one
wave (a group scans a link of the other env), and a lone env with 9.  The same with PER-ENV SHAPES: three envs, three shapes whose last
lists have 9, 1 and 64 (64, 8 and 7) vertices - two different shapes in one wave with their near links pooled in two rounds, the last
shape of the batch carrying the 64-vertex list - each env against the oracle of its own shape.  Points: `one_point`, a wave whose only
point is the single candidate of one link; `all_four`, every link of both envs with exactly four."""
import functools

import numpy as np
import pytest

from oracle.phys_oracle import BatchOracle, default_params
from tests import phys_poses as P
from tests import phys_step as S
from tests.phys_poses import FLAT_MIN_TOUCHED, NB, NSUB, _depths, _names

MODES = [(build, jobs) for build in (1, 2) for jobs in (0, 2)]   # (kernel_build, substep_jobs)
DEPTH_BATCHES = {
    "deep_shallow": (("hands", 0), ("sit", 0)),
    "shallow_deep": (("sit", 0), ("hands", 0)),
    "none_many": (("air", 0), ("flat", 0)),
    "many_none": (("flat", 0), ("air", 0)),
    "deepest_last": (("toe_hand", 0), ("feet", 1)),
    "deepest_first_last": (("hands", 0), ("head", 0)),
    "deepest_middle": (("flat", 0), ("head_hand", 0)),
    "second_wave": (("feet", 1), ("sit", 0), ("hands", 0)),
}
A_ENVS = {"hands": ("hands", 0), "sit": ("sit", 0), "lying": ("flat", 0), "head": ("head", 0)}
PARTNERS = (("feet", 1), ("flat", 1), ("air", 1))
GRID = 1024.0
HULL_SIZES = (1, 7, 8, 9, 63, 64)
LAST = NB - 1
DEEP_LINKS = {2: ("L_Knee", 2), 16: ("L_Elbow", 6), 17: ("L_Wrist", 7)}   # link -> (name, depth): asserted on the CPU


def states(batch):
    return P.stack(P.well_conditioned(pose, 0, k) for pose, k in batch)


def oracle_for(batch, **params):
    return P.oracle_for(states(batch), solver_type=0, **params)


@functools.lru_cache(maxsize=None)
def first_substep(env):
    """One env alone, one substep of the oracle: its stops in link order and their depths."""
    batch = (env,)
    out = oracle_for(batch).step(*P.oracle_inputs(states(batch)), nsub=1, hold=2, want_selection=True)
    stops = [int(b) for b in np.nonzero((out["own"][0, 0] >= 0).any(axis=-1))[0]]
    dep = _depths()
    return stops, [int(dep[b]) for b in stops]


def test_depth_fixtures_are_what_they_claim():
    """CPU, from one substep of the oracle per env."""
    names = _names()
    deepest = {}
    for env in {e for b in DEPTH_BATCHES.values() for e in b} | set(A_ENVS.values()) | set(PARTNERS):
        stops, deps = first_substep(env)
        deepest[env] = (max(deps) if deps else None, stops, deps)
    assert deepest[("hands", 0)][0] == 8 and deepest[("hands", 0)][2] == [8, 8]
    assert deepest[("sit", 0)][0] == 1 and [names[b] for b in deepest[("sit", 0)][1]] == ["Pelvis", "Torso"]
    assert deepest[("head", 0)][0] == 5 and deepest[("feet", 1)][0] == 4
    assert deepest[("air", 0)][1] == [] and len(deepest[("flat", 0)][1]) >= FLAT_MIN_TOUCHED
    # where the deepest stop stands among the touched links
    assert deepest[("toe_hand", 0)][2] == [4, 8]
    d = deepest[("flat", 0)][2]
    assert d[0] < max(d) and 0 < d.index(max(d)) < len(d) - 1, d
    seen = {x for _, _, deps in deepest.values() for x in deps}
    print("[contact setup] depths of the stops of the poses:", sorted(seen), " lying env:", d)
    assert {0, 1, 3, 4, 5, 8} <= seen, sorted(seen)
    for name, batch in DEPTH_BATCHES.items():
        own = oracle_for(batch).step(*P.oracle_inputs(states(batch)), nsub=NSUB, hold=2, want_selection=True)["own"]
        S.assert_oracle_holds_its_own_bound(oracle_for(batch), P.oracle_inputs(states(batch)), own, name)


# ---------------------------------------------------------------------------------------------------------------- the probe bodies
def _specs(kind, nlast, first):
    """level -> (candidates K, hull vertices), and the link of every level."""
    if kind == "all_four":
        return [(4, 5 + (3 * lv) % 17) for lv in range(NB)], [(7 * lv + 3) % NB for lv in range(NB)]
    # `first` comes near first (edge: the last link of the table); the other levels as scattered as in tests/test_gpu_contact_scan.py
    rest = [(7 * lv + 3) % NB for lv in range(NB)]
    rest.remove(first)
    if kind == "deep":  # (the second link to come near is the root: `first` stays the deepest stop)
        rest.remove(0)
        rest = [0] + rest
    sizes = [(6, 64), (1, 3), (3, 7), (5, 12), (4, 9), (2, 2), (8, 33), (1, 1)]
    return [(min(nlast, 5) if nlast > 1 else 1, nlast)] + [sizes[lv % len(sizes)] for lv in range(NB - 1)], [first] + rest


@functools.lru_cache(maxsize=None)
def probe_model(kind, nlast=0, first=LAST):
    """The baked body with link origins on a 1/1024 m grid and a plate of K candidate vertices under every link: world z of the plate of
    level lv = (s + lv) / 1024 when the root stands at 1 + s / 1024; every other vertex a quarter of a metre or more above it."""
    from vid2player3d_amd.model import BodyModel, load_baked_model

    base = load_baked_model()
    rng = np.random.default_rng([31, nlast, first])
    blob = dict(base.blob)
    local = np.round(np.asarray(base.blob["local_pos"], dtype=np.float64) * GRID) / GRID
    blob["local_pos"] = local
    blob["com"] = np.round(np.asarray(base.blob["com"], dtype=np.float64) * GRID) / GRID
    origin = np.zeros((NB, 3))
    for b in range(1, NB):
        origin[b] = origin[int(base.parents[b])] + local[b]
    specs, link_of_level = _specs(kind, nlast, first)
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
        dz = rng.permutation(np.arange(8))[:k] / 65536.0 if k <= 8 else np.zeros(k)  # (depths all different: no tie for the deepest)
        # (deep: only the first two levels ever come near the ground, however far the body falls within the step)
        hv[where, 2] = lv / GRID - 1.0 - origin[b, 2] + dz + (0.125 if kind == "deep" and lv >= 2 else 0.0)
        nt = int(top.sum())
        hv[top, :2] = rng.integers(-16, 17, size=(nt, 2)) / 64.0
        hv[top, 2] = lv / GRID - 1.0 - origin[b, 2] + 0.25 + rng.integers(0, 32, size=nt) / 64.0
        verts.append(hv)
        offs.append(offs[-1] + nv)
    blob["hull_verts"] = np.concatenate(verts, axis=0)
    blob["hull_offsets"] = np.asarray(offs, dtype=np.int32)
    return BodyModel(blob, **base.model_kw), specs, link_of_level


def probe_states(counts):
    """Upright, identity rotations, the root at the height that brings exactly counts[e] links within the contact offset (the plates of
    levels 0 .. counts[e] - 1: level lv at (21 - c + lv) / 1024 m, the offset is 0.02 m), falling and tumbling slowly."""
    n = len(counts)
    root = np.zeros((n, 13), dtype=np.float32)
    for e, c in enumerate(counts):
        root[e, 2] = 1.0 + (21 - c if c > 0 else 64) / GRID
    root[:, 6] = 1.0
    root[:, 7:10] = [0.0625, -0.03125, -0.5]
    root[:, 10:13] = [0.125, 0.0625, 0.03125]
    return root, np.zeros((n, 69), dtype=np.float32), np.zeros((n, 69), dtype=np.float32)


# probe: (kind, vertices of the first link's list, the first link to come near) -> near links per env
PROBES = {("edge", n, LAST): (5, 4, 9) for n in HULL_SIZES}
PROBES[("one_point", 1, LAST)] = (1, 0)
PROBES[("all_four", 0, LAST)] = (24, 24)
# a knee, an elbow, a wrist on the ground (env 0: the deepest stop at depth 2, 6, 7, alone in the first substep; the only other link that
# can come near in these bodies is the root, depth 0) beside an env with both, and a third alone in its wave
PROBES.update({("deep", 9, link): (1, 2, 1) for link in DEEP_LINKS})
# per-env shapes: the vertices of the last list of the shape of each env.  Envs 0 and 1 share a wave and pool their 5 + 4 near links in
# two rounds (a group scans a link of the other env's shape); the last shape of the batch, alone in its wave, carries the 64-vertex list
# in the first, the 7-vertex one in the second
SHAPE_BATCHES = {"9_1_64": (9, 1, 64), "64_8_7": (64, 8, 7)}
SHAPE_COUNTS = (5, 4, 9)


def _model_of(key):
    kind, nlast, first = key
    return probe_model(kind if kind in ("all_four", "deep") else "edge", nlast, first)


def probe_oracle(key):
    return P.oracle_for(probe_states(PROBES[key]), model=_model_of(key)[0], enable_contact=True)


def shapes_oracle(name):
    n = len(SHAPE_COUNTS)
    oracle = BatchOracle([probe_model("edge", nl)[0] for nl in SHAPE_BATCHES[name]], n, default_params(enable_contact=True), model_of=np.arange(n))
    oracle.set_state(*probe_states(SHAPE_COUNTS))
    return oracle


def _own_first_substep(oracle, n):
    z = np.zeros((n, 69))
    return oracle.step(z, np.zeros((n, 3)), np.zeros((n, 3)), nsub=NSUB, hold=2, want_selection=True)["own"][:, 0]


@pytest.mark.parametrize("key", list(PROBES))
def test_oracle_alone_produces_every_probe_case(key):
    """CPU: the last list of the vertex table has the size asked for and its link is touched in every env that is near the ground; the
    near links per env are the counts; one_point: a single point in the wave; all_four: four on each of the 48 links; deep: the only
    stop of env 0 is the knee, the elbow or the wrist, at depth 2, 6, 7."""
    kind, nlast, first = key
    counts = PROBES[key]
    model, specs, link_of_level = _model_of(key)
    own = _own_first_substep(probe_oracle(key), len(counts))
    npts = (own >= 0).sum(axis=-1)
    assert (npts > 0).sum(axis=1).tolist() == list(counts)
    nverts = np.diff(model.hull_offsets)
    if kind == "edge":
        assert nverts[LAST] == nlast and model.hull_offsets[LAST + 1] == len(model.hull_verts) and link_of_level[0] == LAST
        k = specs[0][0]  # (more than four candidates: the manifold reduction keeps two to four of them)
        assert ((npts[:, LAST] == k) if k <= 4 else (npts[:, LAST] >= 2)).all() and (own[:, LAST][own[:, LAST] >= 0] - 64 * LAST < nlast).all()
        assert counts[0] < 8 <= counts[0] + counts[1] - 1, "the second env's last near link is scanned in the second round"
    if kind == "one_point":
        assert npts.sum() == 1 and npts[0, LAST] == 1
    if kind == "all_four":
        assert (npts == 4).all()
    if kind == "deep":
        dep, names = _depths(), _names()
        assert (names[first], int(dep[first])) == DEEP_LINKS[first]
        assert np.nonzero(npts[0])[0].tolist() == [first]
        assert sorted(np.nonzero(npts[1])[0].tolist()) == sorted([first, link_of_level[1]])


def test_deep_probes_complete_the_depths():
    """CPU: with the poses' 1, 3, 4, 5, 8 the deepest stops of the file's fixtures cover every depth 1 .. 8."""
    assert sorted(d for _, d in DEEP_LINKS.values()) == [2, 6, 7]


@pytest.mark.parametrize("name", list(SHAPE_BATCHES))
def test_oracle_alone_produces_the_shape_batches(name):
    """CPU: every env's shape ends in a list of its own size, that link is touched in every env, and the near links are 5, 4 and 9."""
    nlasts = SHAPE_BATCHES[name]
    assert len(set(nlasts)) == len(nlasts) and 64 in nlasts
    own = _own_first_substep(shapes_oracle(name), len(nlasts))
    npts = (own >= 0).sum(axis=-1)
    assert (npts > 0).sum(axis=1).tolist() == list(SHAPE_COUNTS)
    for e, nl in enumerate(nlasts):
        model = probe_model("edge", nl)[0]
        assert np.diff(model.hull_offsets)[LAST] == nl and model.hull_offsets[LAST + 1] == len(model.hull_verts)
        picks = own[e, LAST][own[e, LAST] >= 0] - 64 * LAST
        assert len(picks) >= 1 and (picks < nl).all()
    a, b = (probe_model("edge", nl)[0] for nl in nlasts[:2])
    assert len(a.hull_verts) != len(b.hull_verts), "two different shapes in one wave"


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


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(DEPTH_BATCHES))
@pytest.mark.parametrize("build,jobs", MODES)
def test_depth_batches_match_oracle(name, build, jobs):
    from tests.gpu_util import _compare

    batch = DEPTH_BATCHES[name]
    got = run_kernel(batch, build, jobs)
    base = run_kernel(batch, 1, 0)
    for key in ("pd", "force", "torque"):
        assert np.array_equal(got[key], base[key]), key
    ref = _reference(batch, got["ids_sub"].tobytes())
    assert np.array_equal(got["ids_sub"], ref["own"]), "contact vertex ids, every substep"
    for e, env in enumerate(batch):
        assert [int(b) for b in np.nonzero((got["ids_sub"][e, 0] >= 0).any(axis=-1))[0]] == first_substep(env)[0], (name, e)
    _compare(got, ref, "contact setup, %s build %d jobs %d" % (name, build, jobs))


@pytest.mark.gpu
@pytest.mark.parametrize("a", list(A_ENVS))
@pytest.mark.parametrize("build,jobs", MODES)
def test_env0_bits_do_not_depend_on_the_partner(a, build, jobs):
    """Env 0 alone, beside a standing, a lying and an airborne env: the same bits (env 0 of two batches only)."""
    A = A_ENVS[a]
    alone = run_kernel((A,), build, jobs)
    seen = []
    for partner in PARTNERS:
        got = run_kernel((A, partner), build, jobs)
        seen.append(got["dvel"][1])
        for key in S.BITS:
            assert np.array_equal(alone[key][0], got[key][0]), (a, partner, key)
    assert not np.array_equal(seen[0], seen[1]) and not np.array_equal(seen[1], seen[2])


def _step(st, act, build, jobs=None, body_model=None, pairing=False, shape_ids=None):
    """One control step of a task set to the state st (as tests/phys_step.kernel_step; with the pairing of envs by load on or off, and
    with one body shape per env): what kernel_step returns, and the pairing keys behind the launch."""
    import torch

    from oracle import task_oracle as O
    from tests.gpu_util import N, T, make_task

    n = len(st[0])
    extra = {k: v for k, v in (("body_model", body_model), ("substep_jobs", jobs), ("motion_shape_ids", shape_ids)) if v is not None}
    if not pairing:
        extra["pair_envs_by_load"] = False
    task = make_task(n, S._mlib(), enable_contact=True, residual_force_hold="first_sim", debug_contacts=2, kernel_build=build, contact_solver="pgs",
                     joint_limits=False, **extra)
    task.reset_with_times(None, T(np.full(n, 0.3)))
    task._humanoid_root_states[:] = T(st[0])
    task._dof_pos[:] = T(st[1])
    task._dof_vel[:] = T(st[2])
    task._reset_env_tensors(None)
    rb0 = N(task._rigid_body_state).reshape(n, NB, 13).copy()
    dpos_before = N(task._dof_pos).copy()
    task.pre_physics_step(T(act))
    task._physics_step()
    keys = N(task.debug_pairing()[1]).astype(int) if pairing else None
    torch.cuda.synchronize()
    _, _, _, force, torque = O.pre_physics(act, N(task.reset_buf), dpos_before, rb0[:, 0, 3:7], P._model().kp.astype(np.float32))
    got = {"root": N(task._humanoid_root_states), "dpos": N(task._dof_pos), "dvel": N(task._dof_vel), "rb": N(task._rigid_body_state).reshape(n, NB, 13),
           "cf": N(task._contact_forces), "df": N(task.dof_force_tensor), "ids": N(task.debug_contacts()), "ids_sub": N(task.debug_contacts_substeps()),
           "pd": N(task._pd_target), "force": force, "torque": torque,
           "shape_of_env": None if task._env_shape_ids is None else np.asarray(task._env_shape_ids).copy()}
    name = task.kernel_build()
    task.close()
    assert name.startswith({1: "lds-parked", 2: "registers"}[build])
    return got, keys


def _assert_keys(keys, ids_sub, what):
    """key = max(touched links, links about to touch) x 8 + min(depth of the deepest touched link of the LAST substep, 7)."""
    dep = _depths()
    for e in range(len(keys)):
        touched = np.nonzero((ids_sub[e, -1] >= 0).any(axis=-1))[0]
        want = min(int(dep[touched].max()), 7) if len(touched) else 0
        assert keys[e] % 8 == want and keys[e] // 8 >= len(touched), (what, e, keys[e], touched.tolist())


@pytest.mark.gpu
@pytest.mark.parametrize("build", [1, 2])
def test_pairing_key_carries_the_depth_of_the_deepest_stop(build):
    """The poses (deepest stops at 1, 8, 5, 4, none, 8) and the knee, elbow and wrist probes (2, 6, 7; env 1: an ankle beside them)."""
    batch = (("sit", 0), ("hands", 0), ("head", 0), ("feet", 1), ("air", 0), ("toe_hand", 0))
    st = states(batch)
    got, keys = _step(st, P.actions(st), build, pairing=True)
    _assert_keys(keys, got["ids_sub"], batch)
    seen = {int(k) % 8 for k in keys}
    for key in PROBES:
        if key[0] == "deep":
            n = len(PROBES[key])
            got, keys = _step(probe_states(PROBES[key]), np.zeros((n, 75), dtype=np.float32), build, body_model=_model_of(key)[0], pairing=True)
            _assert_keys(keys, got["ids_sub"], key)
            assert key[2] in np.nonzero((got["ids_sub"][0, -1] >= 0).any(axis=-1))[0] and keys[0] % 8 == DEEP_LINKS[key[2]][1]
            seen |= {int(k) % 8 for k in keys}
    assert {0, 1, 2, 4, 5, 6, 7} <= seen, sorted(seen)


@functools.lru_cache(maxsize=None)
def run_probe(key, build, jobs):
    counts = PROBES[key]
    n = len(counts)
    got = S.kernel_step(*probe_states(counts), np.zeros((n, 75), dtype=np.float32), build=build, body_model=_model_of(key)[0], substep_jobs=jobs)
    return got, S.reference(probe_oracle(key), got)


@pytest.mark.gpu
@pytest.mark.parametrize("key", list(PROBES))
@pytest.mark.parametrize("build,jobs", MODES)
def test_probe_bodies_match_oracle(key, build, jobs):
    """The hull list at the end of the vertex table (1 .. 64 vertices), one point in a wave, four points on every link, a knee, an elbow
    and a wrist as the deepest stop: the oracle's vertices in every substep, its state within the bounds."""
    from tests.gpu_util import _compare

    got, ref = run_probe(key, build, jobs)
    counts = PROBES[key]
    assert (got["ids_sub"][:, 0] >= 0).any(axis=-1).sum(axis=1).tolist() == list(counts)
    assert np.array_equal(got["ids_sub"], ref["own"]), "contact vertex ids, every substep"
    assert np.abs(got["cf"]).max() > 1.0, "the contacts must carry load"
    _compare(got, ref, "contact setup probes, %s build %d jobs %d" % (key, build, jobs))


@functools.lru_cache(maxsize=None)
def run_shapes(name, build, jobs):
    """One body shape per env (the task takes one per clip: clip k has shape k % 3, env e plays clip e)."""
    nlasts = SHAPE_BATCHES[name]
    n = len(nlasts)
    models = [probe_model("edge", nl)[0] for nl in nlasts]
    got, _ = _step(probe_states(SHAPE_COUNTS), np.zeros((n, 75), dtype=np.float32), build, jobs=jobs, body_model=models, shape_ids=np.arange(S._mlib().num_motions()) % n)
    return got, S.reference(shapes_oracle(name), got)


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(SHAPE_BATCHES))
@pytest.mark.parametrize("build,jobs", MODES)
def test_per_env_shapes_match_oracle(name, build, jobs):
    """Two different shapes in one wave whose near links are pooled, the last shape of the batch with the 64-vertex (7-vertex) list at
    the end of its table: each env against the oracle of ITS shape - vertices in every substep, the state within the bounds."""
    from tests.gpu_util import _compare

    got, ref = run_shapes(name, build, jobs)
    assert got["shape_of_env"].tolist() == [0, 1, 2], "env e simulates shape e"
    assert (got["ids_sub"][:, 0] >= 0).any(axis=-1).sum(axis=1).tolist() == list(SHAPE_COUNTS)
    assert np.array_equal(got["ids_sub"], ref["own"]), "contact vertex ids, every substep"
    assert np.abs(got["cf"]).reshape(3, -1).max(axis=1).min() > 1.0, "the contacts must carry load"
    _compare(got, ref, "contact setup shapes, %s build %d jobs %d" % (name, build, jobs))
