"""The way down of the contact sweep's walk, the closing move and the closing root -> leaves pass, and the head and tail of a visit
(walk_to, walk_close and the visit loop of the link-per-lane physics kernel) - against the float64 C oracle (oracle/phys), one control
step (4 substeps x 4 sweeps), PGS, both builds of the kernel, batches of 2 envs (one full wave), 3 envs (a full wave and a wave with
one env) and 34 envs.  Poses, their builder, the oracle set-up and the bound (rows_all of tests/test_gpu_physics.py with its cap on the
conditioning term) are those of tests/test_gpu_walk_up.py; `hover` is that of tests/test_gpu_sweep_visits.py; `sit` is new here.

Named by what they make the changed loops do (links are lanes in depth-first order; a move goes up from the stop the walk stands on to
the lowest common ancestor and down to the next stop, level by level, for both envs of a wave at once):
  one_level   L_Ankle + L_Toe: the way down ankle -> toe is one level (and the way back has no way down at all)
  full_depth  L_Toe + R_Hand: from a stop in one leg over the root down to a hand, the deepest link (8 levels)
  side_entry  feet / hands / Head + L_Hand: ways down that enter through a link that is not its parent's first child (R_Hip under the
              root, the thoraxes under the chest)
  gap         feet beside hands (beside Head + L_Hand): in their first visit one env goes down levels 1 .. 3 and the other 4 .. 8 (4 .. 5):
              the ranges do not overlap, each env idles through the other's levels
  rest        an env with 2 stops beside one with 4 or with 7 and more: it rests in the surplus visits while the other moves
  single      an env with ONE stop (it stands on its head): it never moves; its closing move and closing pass still run
  close_ends  the last stop is the deepest link (R_Hand, depth 8: `hands`, `toe_hand`) or a child of the root (Torso, depth 1: `sit` -
              sitting on Pelvis and Torso, legs and chest raised): the closing move starts at the deepest and the shallowest stop
  done_early  an env whose four stops hover inside the contact offset (every point separated): its first sweep changes nothing and it is
              struck out, beside a partner whose feet are in the ground and which goes on iterating
  counts      lying on the back: links with 1, 2, 3 and 4 contact points among the stops of the first wave of the small batches (`flat2`: a
              `flat` state that has a link with exactly two; the 34-env batch has 1, 3 and 4), beside envs whose stops all have 4 - the two stops of a visit differ in their number of points
TGS is not run here: its kernels keep the parent's form of everything this file is about (VTAB in physics_ll.hip), and
tests/test_gpu_walk_up.py runs them.
Env 0 holds the same state in the 3-env and in the 34-env batch beside different partners: its bits must not depend on the partner.
test_fixtures_are_what_they_claim checks on the CPU what the names say, that in the state a step starts from EVERY hull vertex of every
link is at least 1e-4 m away from the height at which it would become a contact point or stop being one (the contact offset: these
decisions set which links are stops and how many points each has; an env's state is the first of its numbered states that keeps this
distance) - so that the bound cannot hide a loop that solves other stops or other points -, that a link with up to four vertices below the plane has that
number of points in the oracle's selection, that the partner of the hovering env of done_early still changes something in its fourth
sweep, and that the float64 oracle, perturbed at the level of float32 rounding, stays inside the cap of rows_all on its own."""
import functools

import numpy as np
import pytest

from oracle import task_oracle as O
from oracle.phys_oracle import BatchOracle, default_params
from tests import test_gpu_sweep_visits as V
from tests import test_gpu_walk_up as W
from tests.test_gpu_tree_passes import NB, NSUB, _depths, _mlib, _model, _rot_expmap, _rot_quat, lowest_point

SIZES = (2, 3, 34)
CASES = [(n, build) for n in SIZES for build in (1, 2)]
CONTACT_OFFSET = 0.02   # a hull vertex closer to the ground than this is a contact point, m
MARGIN = 1e-4           # EVERY hull vertex of every link is at least this far from CONTACT_OFFSET in the state a step starts from, m
# nominal state number of every env (env 0 is state 0 in every batch; its partner differs between the 3-env and the 34-env batch).  The state an
# env really gets is the first of k, k + 100, k + 200, ... whose hull vertices all keep MARGIN: well_conditioned()
STATE_IDS = {2: [0, 1], 3: W.STATE_IDS[3], 34: W.STATE_IDS[34]}
STRIDE, TRIES = 100, 200
# sit: the baked body lies on its back; legs raised to the vertical, spine and chest curled up, a tilt of the root levels Pelvis and Torso
SIT = ({"L_Hip": W.X * -np.pi / 2, "R_Hip": W.X * -np.pi / 2, "Spine": W.X * 1.0, "Chest": W.X * 0.5}, ("Pelvis", "Torso"), W.X)
# (the 3-env batch - its first two envs are the 2-env batch -, the first pair of the 34-env batch, the pairs that fill it)
FIXTURES = {
    "one_level": (["ankle_toe", "ankle_toe", "ankle_toe"], ["ankle_toe", "head"], [("ankle_toe", "ankle_toe"), ("ankle_toe", "head"), ("head", "ankle_toe")]),
    "full_depth": (["toe_hand", "toe_hand", "toe_hand"], ["toe_hand", "ankle_toe"], [("toe_hand", "toe_hand"), ("toe_hand", "ankle_toe"), ("hands", "toe_hand")]),
    "side_entry": (["feet", "hands", "head_hand"], ["feet", "head_hand"], [("feet", "feet"), ("hands", "hands"), ("head_hand", "feet"), ("hands", "head_hand")]),
    "gap": (["feet", "hands", "hands"], ["feet", "head_hand"], [("feet", "hands"), ("hands", "feet"), ("feet", "head_hand")]),
    "rest": (["hands", "feet", "ankle_toe"], ["hands", "flat"], [("hands", "flat"), ("ankle_toe", "flat"), ("feet", "hands"), ("flat", "ankle_toe")]),
    "single": (["head", "feet", "head"], ["head", "hands"], [("head", "feet"), ("feet", "head"), ("head", "head"), ("head", "flat")]),
    "close_ends": (["sit", "hands", "sit"], ["sit", "toe_hand"], [("sit", "hands"), ("toe_hand", "sit"), ("sit", "sit"), ("hands", "toe_hand")]),
    "done_early": (["hover", "feet", "hover"], ["hover", "flat"], [("hover", "feet"), ("feet", "hands"), ("feet", "hover"), ("hands", "feet")]),
    "counts": (["flat", "flat2", "feet"], ["flat", "ankle_toe"], [("flat", "feet"), ("feet", "hands"), ("feet", "flat"), ("hands", "feet")]),
}
SEEDS = dict.fromkeys(FIXTURES, 0)
TOUCHING = {"hover": V.FEET, "sit": SIT[1], "flat2": None}


def env_poses(fixture, n):
    three, first, fill = FIXTURES[fixture]
    if n <= 3:
        return three[:n]
    return first + [p for i in range(16) for p in fill[i % len(fill)]]


@functools.lru_cache(maxsize=None)
def sit_state(seed, k):
    """As state() of tests/test_gpu_walk_up.py, for the pose SIT: the tilt of the root about the body's left axis is solved so that
    the lowest vertices of Pelvis and Torso are level; every other link stays more than W.CLEAR above them."""
    names = W._names()
    rng = np.random.default_rng([1009, seed, k])
    joints, chosen, axis = SIT
    fixed = {names.index(j): _rot_expmap(v) for j, v in joints.items()}
    R0 = _rot_expmap(rng.normal(0, 0.002, size=3))
    noise = rng.normal(0, 0.004, size=69)
    dpos = np.concatenate([W._expmap_of(fixed.get(b, np.eye(3)) @ _rot_expmap(noise[3 * (b - 1):3 * b])) for b in range(1, NB)])
    ids = [names.index(c) for c in chosen]

    def resid(a):
        low = lowest_point(W._quat_of(_rot_expmap(axis * a) @ R0), dpos)[ids]
        return low[1] - low[0]

    lo, hi = -0.6, 0.6  # (bisection: the difference of the two lowest vertices is monotonic in the tilt over this range)
    assert resid(lo) * resid(hi) < 0, (resid(lo), resid(hi))
    for _ in range(60):
        mid = 0.5 * (lo + hi)
        lo, hi = (mid, hi) if resid(lo) * resid(mid) > 0 else (lo, mid)
    q = W._quat_of(_rot_expmap(axis * 0.5 * (lo + hi)) @ R0)
    root = np.zeros(13)
    root[3:7] = q
    dvel = rng.normal(0, W.REST_VEL, size=69)
    root[7:10] = rng.normal(0, 0.4 * W.REST_VEL, size=3)
    root[10:13] = rng.normal(0, 0.4 * W.REST_VEL, size=3)
    root, dpos, dvel = root.astype(np.float32), dpos.astype(np.float32), dvel.astype(np.float32)
    low = lowest_point(root[3:7], dpos)
    assert np.ptp(low[ids]) < W.LEVEL and np.delete(low, ids).min() > low[ids].max() + W.CLEAR, (k, np.round(np.sort(low) - low.min(), 4)[:6])
    root[2] = -low.min() - rng.uniform(*W.SINK)
    return root, dpos, dvel, rng.normal(0, 0.02, size=6).astype(np.float32)


def state(pose, seed, k):
    """(flat2: a `flat` state - which of them, well_conditioned() decides)"""
    return sit_state(seed, k) if pose == "sit" else V.state("flat" if pose == "flat2" else pose, seed, k)


def vertex_heights(root, dpos):
    """Height above the ground of every hull vertex of every link (forward kinematics, float64), as one array, and the link of each."""
    m = _model()
    par, lp = np.asarray(m.parents), np.asarray(m.local_pos, dtype=np.float64)
    hv, ho = np.asarray(m.hull_verts, dtype=np.float64), np.asarray(m.hull_offsets)
    R, x = [None] * NB, np.zeros((NB, 3))
    R[0] = _rot_quat(root[3:7])
    out, link = [], []
    for b in range(NB):
        if b:
            q = int(par[b])
            x[b] = x[q] + R[q] @ lp[b]
            R[b] = R[q] @ _rot_expmap(dpos[3 * (b - 1):3 * b])
        out.append((hv[ho[b]:ho[b + 1]] @ R[b].T)[:, 2] + x[b, 2] + float(root[2]))
        link.append(np.full(len(out[-1]), b))
    return np.concatenate(out), np.concatenate(link)


def flip_margin(st):
    """How far the closest hull vertex of a state is from the offset plane: the smallest change of height that would make a vertex a
    contact point or stop it being one (and so change a link's number of points, or whether it is a stop of the walk)."""
    return float(np.abs(vertex_heights(st[0], st[1])[0] - CONTACT_OFFSET).min())


@functools.lru_cache(maxsize=None)
def well_conditioned(pose, seed, k):
    """The first of the states k, k + STRIDE, ... of a pose in which every hull vertex keeps MARGIN from the offset plane."""
    for j in range(TRIES):
        st = state(pose, seed, k + STRIDE * j)
        if flip_margin(st) < MARGIN:
            continue
        if pose in ("flat", "flat2"):  # (lying on the back: seven links or more; flat2: one of them with exactly two vertices below the plane)
            height, link = vertex_heights(st[0], st[1])
            below = np.bincount(link[height < CONTACT_OFFSET], minlength=NB)
            if (below > 0).sum() < W.FLAT_MIN_TOUCHED or (pose == "flat2" and not (below == 2).any()):
                continue
        return st
    raise AssertionError("no state of %s among %d keeps %g m" % (pose, TRIES, MARGIN))


def states(fixture, n):
    parts = [well_conditioned(pose, SEEDS[fixture], k) for pose, k in zip(env_poses(fixture, n), STATE_IDS[n])]
    return [np.stack([p[i] for p in parts]) for i in range(4)]


def actions(fixture, n):
    _, dpos, _, wrench = states(fixture, n)
    return np.concatenate([dpos, wrench], axis=1).astype(np.float32)


def oracle_for(fixture, n):
    root, dpos, dvel, _ = states(fixture, n)
    oracle = BatchOracle(_model(), n, default_params(solver_type=0))
    oracle.set_state(root, dpos, dvel)
    return oracle


def chosen_links(pose):
    return TOUCHING[pose] if pose in TOUCHING else W.POSES[pose][2]


def assert_touched(own, fixture, n):
    """own [n, nsub, NB, 4]: the oracle's contact selection.  In the first substep every env touches the ground with exactly the links
    its pose was built for (flat: seven or more).  Returns the touched links [n, NB] and their numbers of points [n, NB]."""
    names = W._names()
    cnt = (own[:, 0] >= 0).sum(axis=-1)
    touched = cnt > 0
    for e, pose in enumerate(env_poses(fixture, n)):
        got = {names[b] for b in np.nonzero(touched[e])[0]}
        if chosen_links(pose) is None:
            assert len(got) >= W.FLAT_MIN_TOUCHED, (fixture, e, sorted(got))
        else:
            assert got == set(chosen_links(pose)), (fixture, e, pose, sorted(got))
    return touched, cnt


def stops_of(touched_row):
    return [int(b) for b in np.nonzero(touched_row)[0]]  # (the walk takes the touched links in ascending order)


@pytest.mark.parametrize("fixture", list(FIXTURES))
@pytest.mark.parametrize("n", SIZES)
def test_fixtures_are_what_they_claim(fixture, n):
    """CPU.  The envs touch the ground with the links they were built for; every link's lowest vertex is at least MARGIN away from
    the contact offset in the state the step starts from; the walks these stops give are what the fixture's name says (from the tree's
    depths and parents); and the float64 oracle moved by float32 rounding of its inputs (the largest change over 32 perturbed runs, on
    every element) against itself needs the conditioning term in no more envs than rows_close allows - it asserts that cap itself."""
    from tests.gpu_util import N  # noqa: F401  (the helpers import torch; no GPU is touched here)
    from tests.test_gpu_physics import rows_all

    names, dep, par = W._names(), _depths(), [int(p) for p in _model().parents]
    root, dpos, _, _ = states(fixture, n)
    act = actions(fixture, n)
    _, pd, _, force, torque = O.pre_physics(act, np.zeros(n, dtype=np.int64), dpos, root[:, 3:7], _model().kp.astype(np.float32))
    out = oracle_for(fixture, n).step(pd, force, torque, nsub=NSUB, hold=2, want_selection=True)
    own = out["own"]
    touched, cnt = assert_touched(own, fixture, n)
    poses = env_poses(fixture, n)
    for e in range(n):
        height, link = vertex_heights(root[e], dpos[e])
        assert np.abs(height - CONTACT_OFFSET).min() >= MARGIN, (fixture, e, poses[e], np.sort(np.abs(height - CONTACT_OFFSET))[:3])
        below = np.bincount(link[height < CONTACT_OFFSET], minlength=NB)  # (the rule takes every vertex below the plane if they are four at the most)
        assert (cnt[e][below <= 4] == below[below <= 4]).all() and (cnt[e][below > 4] >= 2).all(), (fixture, e, below, cnt[e])
    stops = [stops_of(touched[e]) for e in range(n)]

    def anc(b):  # ancestors or self, root last
        out_ = [b]
        while par[out_[-1]] >= 0:
            out_.append(par[out_[-1]])
        return out_

    def move(a, b):  # (depth of the lowest common ancestor, depth of b, the link through which the way down enters)
        aa, path = set(anc(a)), anc(b)
        lca = next(x for x in path if x in aa)
        return dep[lca], dep[b], (path[path.index(lca) - 1] if lca != b else None)

    def down_range(e, k):  # levels of the way down into stop k of env e (from its stop before, cyclically), or None
        s = stops[e]
        if k >= len(s) or len(s) < 2:
            return None
        dl, dn, _ = move(s[k - 1], s[k])
        return (dl + 1, dn) if dn > dl else None

    pairs = [(e, e + 1) for e in range(0, n - 1, 2)]
    moves = [move(s[k - 1], s[k]) for s in stops if len(s) > 1 for k in range(len(s))]
    if fixture == "one_level":
        assert stops[0] == [names.index("L_Ankle"), names.index("L_Toe")] and down_range(0, 1) == (4, 4) and down_range(0, 0) is None
    if fixture == "full_depth":
        assert move(names.index("L_Toe"), names.index("R_Hand"))[:2] == (0, 8) and dep.max() == 8 and down_range(0, 1) == (1, 8)
    if fixture == "side_entry":
        entries = {m[2] for m in moves if m[2] is not None}
        late_children = {b for b in entries if b != par[b] + 1}
        assert {names.index("R_Hip"), names.index("L_Thorax"), names.index("R_Thorax")} <= late_children, sorted(late_children)
    if fixture == "gap":
        a, b = down_range(0, 0), down_range(1, 0)
        assert a is not None and b is not None and (a[1] < b[0] or b[1] < a[0]), (a, b)
    if fixture == "rest":
        assert len(stops[0]) == 2 and len(stops[1]) >= 4 and any(len(stops[a]) != len(stops[b]) and min(len(stops[a]), len(stops[b])) >= 2 for a, b in pairs)
    if fixture == "single":
        assert len(stops[0]) == 1 and len(stops[1]) > 1 and any(len(stops[a]) == 1 and len(stops[b]) == 1 for a, b in pairs) == (n > 3)
    if fixture == "close_ends":
        last = [dep[s[-1]] for s in stops]
        assert last[0] == 1 and par[stops[0][-1]] == 0 and last[1] == dep.max() and (n < 34 or {1, int(dep.max())} <= set(last[2:]))
    if fixture == "counts":
        seen = set(cnt[:2].ravel().tolist())  # (the first wave, the first substep; flat2 - in the small batches - has a link with two points)
        assert ({1, 2, 3, 4} if n <= 3 else {1, 3, 4}) <= seen, seen
        differ = [k for k in range(min(len(stops[0]), len(stops[1]))) if cnt[0][stops[0][k]] != cnt[1][stops[1][k]]]
        assert differ, "the two stops of a visit must differ in their number of points"
    if fixture == "done_early":
        # ... and the partner of the hovering env 0 still changes something in its FOURTH sweep: the first substep alone with three
        # and with four sweeps gives it other contact forces (an env that is struck out stays struck out, so it ran all four), and
        # the hovering env none with either
        three = BatchOracle(_model(), n, default_params(solver_type=0, n_iter=3))
        three.set_state(*states(fixture, n)[:3])
        cf3 = three.step(pd, force, torque, nsub=1, hold=2)["cf"]
        cf4 = oracle_for(fixture, n).step(pd, force, torque, nsub=1, hold=2)["cf"]
        assert poses[0] == "hover" and poses[1] != "hover"
        assert np.abs(cf4[1] - cf3[1]).max() > 1e-6 * np.abs(cf4[1]).max() > 0.0, (np.abs(cf4[1] - cf3[1]).max(), np.abs(cf4[1]).max())
        assert np.abs(cf4[0]).max() == 0.0 and np.abs(cf3[0]).max() == 0.0
    # done_early: a hovering env carries no load at the end of the step (it never applied an impulse), every other grounded env does
    cf = np.abs(out["cf"]).reshape(n, -1).max(axis=1)
    for e, pose in enumerate(poses):
        assert (cf[e] == 0.0) == (pose == "hover"), (fixture, e, pose, cf[e])
    oracle = oracle_for(fixture, n)
    sens = oracle.sensitivity(pd, force, torque, nsub=NSUB, hold=2, forced_ids=own, seed=n)
    ref = oracle.step(pd, force, torque, nsub=NSUB, hold=2, forced_ids=own)
    ref["sens"] = sens
    moved = {k: ref[k] + sens[k] for k in ("root", "dpos", "dvel", "rb", "cf", "df")}
    bad = rows_all(moved, ref, "oracle at float32 rounding, %s n=%d" % (fixture, n))
    assert not bad.any()


# ---------------------------------------------------------------------------------------------------------------- GPU
@functools.lru_cache(maxsize=None)
def run_case(fixture, n, build):
    """One control step of the kernel from a fixture and the oracle's step from the same state (with the kernel's contact vertices
    forced).  Shared by the tests; nothing modifies what it returns."""
    import torch

    from tests.gpu_util import N, T, close, make_task

    task = make_task(n, _mlib(), enable_contact=True, residual_force_hold="first_sim", debug_contacts=2, pair_envs_by_load=False,
                     kernel_build=build, contact_solver="pgs", joint_limits=False)
    task.reset_with_times(None, T(np.full(n, 0.3)))
    root, dpos, dvel, _ = states(fixture, n)
    task._humanoid_root_states[:] = T(root)
    task._dof_pos[:] = T(dpos)
    task._dof_vel[:] = T(dvel)
    task._reset_env_tensors(None)
    oracle = oracle_for(fixture, n)
    act = actions(fixture, n)
    rb0 = N(task._rigid_body_state).reshape(n, NB, 13).copy()
    dpos_before = N(task._dof_pos).copy()
    task.pre_physics_step(T(act))
    task._physics_step()
    torch.cuda.synchronize()
    pd_tar = N(task._pd_target)
    _, pd_ref, _, force, torque = O.pre_physics(act, N(task.reset_buf), dpos_before, rb0[:, 0, 3:7], task.body_model.kp.astype(np.float32))
    close(pd_tar, pd_ref, 1e-6, "pd target")
    got = {"root": N(task._humanoid_root_states), "dpos": N(task._dof_pos), "dvel": N(task._dof_vel), "rb": N(task._rigid_body_state).reshape(n, NB, 13),
           "cf": N(task._contact_forces), "df": N(task.dof_force_tensor), "ids": N(task.debug_contacts()), "ids_sub": N(task.debug_contacts_substeps())}
    name = task.kernel_build()
    task.close()
    assert name.startswith({1: "lds-parked", 2: "registers"}[build])
    sens = oracle.sensitivity(pd_tar, force, torque, nsub=NSUB, hold=2, forced_ids=got["ids_sub"], seed=n)
    ref = oracle.step(pd_tar, force, torque, nsub=NSUB, hold=2, forced_ids=got["ids_sub"], want_selection=True)
    ref["sens"] = sens
    return got, ref


@pytest.mark.gpu
@pytest.mark.parametrize("fixture", list(FIXTURES))
@pytest.mark.parametrize("n,build", CASES)
def test_way_down_and_close_match_oracle(fixture, n, build):
    """Every env touches the ground with the links its pose was built for (the kernel's selection agrees on which links touch and on
    how many points each has), the envs that stand on something carry load, the hovering ones none, and the step is the oracle's within
    the bounds of rows_all."""
    from tests.test_gpu_physics import _compare

    got, ref = run_case(fixture, n, build)
    assert_touched(ref["own"], fixture, n)
    assert np.array_equal((got["ids_sub"][:, 0] >= 0).sum(axis=-1), (ref["own"][:, 0] >= 0).sum(axis=-1))
    loaded = np.array([p != "hover" for p in env_poses(fixture, n)])
    assert (np.abs(got["cf"]).reshape(n, -1).max(axis=1)[loaded] > 1.0).all(), "the contacts must carry load"
    assert np.abs(got["cf"][~loaded]).max(initial=0.0) == 0.0
    _compare(got, ref, "way down, %s n=%d build %d" % (fixture, n, build))


@pytest.mark.gpu
@pytest.mark.parametrize("fixture", list(FIXTURES))
@pytest.mark.parametrize("build", [1, 2])
def test_env_bits_do_not_depend_on_the_partner(fixture, build):
    """Env 0 holds the same state in the 3-env and in the 34-env batch; the env it shares its wave with is another state, and in most
    fixtures another pose."""
    a, _ = run_case(fixture, 3, build)
    b, _ = run_case(fixture, 34, build)
    assert not np.array_equal(a["dvel"][1], b["dvel"][1]), "the partners must differ"
    for key in ("root", "dpos", "dvel", "rb", "cf", "df", "ids_sub"):
        assert np.array_equal(a[key][0], b[key][0]), key
