"""The way down of the contact sweep's walk, the closing move and the closing root -> leaves pass, and the head and tail of a visit
(walk_to, walk_close and the visit loop of the link-per-lane physics kernel) - against the float64 C oracle (oracle/phys), one control
step (4 substeps x 4 sweeps), PGS, both builds of the kernel, batches of 2 envs (one full wave), 3 envs (a full wave and a wave with
one env) and 34 envs.  Poses, their builder, the oracle set-up and the bound (rows_all of tests/gpu_util.py with its cap on the
conditioning term) are those of tests/phys_poses.py and tests/phys_step.py, `hover` and `sit` among them.

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

from tests import phys_poses as P
from tests import phys_step as S
from tests.phys_poses import CONTACT_OFFSET, FEET, FLAT_MIN_TOUCHED, MARGIN, NB, POSES, SIT, STATE_IDS, _depths, _model, _names, vertex_heights

SIZES = (2, 3, 34)
CASES = [(n, build) for n in SIZES for build in (1, 2)]
# STATE_IDS gives the nominal state number of every env; the state an env really gets is the first of k, k + 100, k + 200, ... whose hull
# vertices all keep MARGIN from the contact offset: phys_poses.well_conditioned()
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
TOUCHING = {"hover": FEET, "sit": SIT[1], "flat2": None}


def env_poses(fixture, n):
    three, first, fill = FIXTURES[fixture]
    if n <= 3:
        return three[:n]
    return first + [p for i in range(16) for p in fill[i % len(fill)]]


def states(fixture, n):
    return P.stack(P.well_conditioned(pose, SEEDS[fixture], k) for pose, k in zip(env_poses(fixture, n), STATE_IDS[n]))


def oracle_for(fixture, n, **params):
    return P.oracle_for(states(fixture, n), solver_type=0, **params)


def chosen_links(pose):
    return TOUCHING[pose] if pose in TOUCHING else POSES[pose][2]


def assert_touched(own, fixture, n):
    """own [n, nsub, NB, 4]: the oracle's contact selection.  In the first substep every env touches the ground with exactly the links
    its pose was built for (flat: seven or more).  Returns the touched links [n, NB] and their numbers of points [n, NB]."""
    names = _names()
    cnt = (own[:, 0] >= 0).sum(axis=-1)
    touched = cnt > 0
    for e, pose in enumerate(env_poses(fixture, n)):
        got = {names[b] for b in np.nonzero(touched[e])[0]}
        if chosen_links(pose) is None:
            assert len(got) >= FLAT_MIN_TOUCHED, (fixture, e, sorted(got))
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
    names, dep, par = _names(), _depths(), [int(p) for p in _model().parents]
    root, dpos, _, _ = states(fixture, n)
    inputs = P.oracle_inputs(states(fixture, n))
    out = oracle_for(fixture, n).step(*inputs, nsub=P.NSUB, hold=2, want_selection=True)
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
        cf3 = oracle_for(fixture, n, n_iter=3).step(*inputs, nsub=1, hold=2)["cf"]
        cf4 = oracle_for(fixture, n).step(*inputs, nsub=1, hold=2)["cf"]
        assert poses[0] == "hover" and poses[1] != "hover"
        assert np.abs(cf4[1] - cf3[1]).max() > 1e-6 * np.abs(cf4[1]).max() > 0.0, (np.abs(cf4[1] - cf3[1]).max(), np.abs(cf4[1]).max())
        assert np.abs(cf4[0]).max() == 0.0 and np.abs(cf3[0]).max() == 0.0
    # done_early: a hovering env carries no load at the end of the step (it never applied an impulse), every other grounded env does
    cf = np.abs(out["cf"]).reshape(n, -1).max(axis=1)
    for e, pose in enumerate(poses):
        assert (cf[e] == 0.0) == (pose == "hover"), (fixture, e, pose, cf[e])
    S.assert_oracle_holds_its_own_bound(oracle_for(fixture, n), inputs, own, "%s n=%d" % (fixture, n))


# ---------------------------------------------------------------------------------------------------------------- GPU
@functools.lru_cache(maxsize=None)
def run_case(fixture, n, build):
    """One control step of the kernel from a fixture and the oracle's step from the same state (with the kernel's contact vertices
    forced).  Shared by the tests; nothing modifies what it returns."""
    st = states(fixture, n)
    got = S.kernel_step(*st[:3], P.actions(st), build=build)
    return got, S.reference(oracle_for(fixture, n), got)


@pytest.mark.gpu
@pytest.mark.parametrize("fixture", list(FIXTURES))
@pytest.mark.parametrize("n,build", CASES)
def test_way_down_and_close_match_oracle(fixture, n, build):
    """Every env touches the ground with the links its pose was built for (the kernel's selection agrees on which links touch and on
    how many points each has), the envs that stand on something carry load, the hovering ones none, and the step is the oracle's within
    the bounds of rows_all."""
    from tests.gpu_util import _compare

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
    S.assert_env0_ignores_its_partner(run_case(fixture, 3, build)[0], run_case(fixture, 34, build)[0])
