"""Contact generation of the link-per-lane physics kernel, case by case: the hull scan by groups of 8 lanes, the manifold reduction
and the contact points of the chosen vertices, against the selection rule of the C oracle (oracle/phys) - vertex ids EXACTLY, in every
substep - and the state after one control step at the bounds of the contact parity tests (rows_all of tests/gpu_util.py).

The fixture is a body whose every link carries a "probe": a hull with a flat plate of K candidate vertices hanging down to a level of
its own, 1/1024 m apart from link to link, under a humanoid that stands upright with identity rotations.  The height of the root then
decides how many links are near the ground (one more per 1/1024 m), the plate of a link decides how many candidates it has and what
its manifold looks like.  All coordinates are multiples of 2^-16 m: float32 (kernel) and float64 (oracle) evaluate the state of the first
substep without any rounding, so exact ties - equal depths, equal distances - are ties in both and the rule "first index attaining the
extreme" decides; from the second substep on the root's angular velocity tilts every plate by far more than float32 rounding.

Cases (ISSUE "contact scan"): no near link; 1, 2, 3, 4 candidates (no reduction); more than 4 with exact ties in depth; collinear
candidates (manifold of 2) and candidates on one side of the base line (manifold of 3); hulls of fewer than 8 and of 64 vertices;
waves with 8, 9 and 17 near links (1, 2, 3 rounds); a link whose rank crosses a round boundary in a wave that pools the near links
of two envs; the same env next to two different partners.  test_oracle_alone_produces_every_case checks on the CPU that the poses
produce them."""
import functools

import numpy as np
import pytest

from tests import phys_poses as P
from tests import phys_step as S
from tests.phys_poses import NB, NSUB

GRID = 1024.0        # link levels and root heights: multiples of 1/1024 m
COFF = 0.02          # contact offset (oracle.default_params)
TOP_LEVEL = 20       # a plate at (s + level) / 1024 m is within the contact offset while s + level <= 20 (21 / 1024 is beyond the box cull too)
# near links per env (the root is put at the height that gives exactly so many), in wave order: envs 2w and 2w + 1 share wave w
COUNTS_34 = [0, 0,   8, 0,   5, 4,   9, 8,   5, 0,   0, 5,   24, 24,   1, 1,   2, 3,   7, 1,   4, 4,   16, 1,   3, 13,   12, 12,   6, 2,   0, 9,   17, 7]
COUNTS_3 = [5, 4, 9]  # wave 0 pools 9 near links (2 rounds); env 2 is alone in its wave with 9 of its own


def _plate(kind, k, rng):
    """Ground-plane coordinates [k, 2] (multiples of 1/4096 m) and depth offsets [k] (multiples of 2^-16 m, 1e-4 m at the most) of a plate."""
    if kind == "line":      # collinear: every signed area is zero, the manifold keeps the deepest and the farthest from it
        t = rng.permutation(np.arange(-8, 8))[:k]
        return np.stack([t * 2, t], axis=1) / 64.0, np.zeros(k)
    if kind == "arc":       # deepest = first index = one end, farthest = the other end, all others on ONE side of that line, no two
        t = np.arange(k)    # of them equally far from it (equal areas stay equal under any rigid motion: rounding would decide later on)
        xy = np.asarray({5: [[0, 0], [4, 3], [9, 7], [13, 4], [17, 0]], 6: [[0, 0], [4, 3], [9, 7], [15, 8], [19, 4], [22, 0]]}[k]) / 64.0
        order = np.concatenate([[0], rng.permutation(np.arange(1, k))])
        return xy[order], np.zeros(k)
    # "flat": equal depths, "tilted": all different; points in general position on a fine grid (no equal distances or areas by accident,
    # and squares of the differences still exact in float32)
    xy = rng.integers(-780, 781, size=(k, 2))
    dz = np.zeros(k) if kind == "flat" else rng.permutation(np.arange(8))[:k] if k <= 8 else rng.integers(0, 8, size=k)
    return xy / 4096.0, dz / 65536.0


# level -> (plate kind, candidates K, hull vertices): the first links to come near carry the named cases
SPECS = [("flat", 6, 64), ("flat", 1, 3), ("flat", 2, 5), ("flat", 3, 7), ("flat", 4, 9), ("line", 5, 12), ("arc", 6, 20), ("tilted", 8, 33),
         ("flat", 40, 64), ("tilted", 5, 8), ("flat", 7, 17), ("tilted", 12, 31), ("flat", 2, 2), ("line", 9, 40), ("flat", 9, 9), ("tilted", 3, 50),
         ("arc", 5, 6), ("flat", 16, 16), ("tilted", 6, 57), ("flat", 5, 5), ("tilted", 4, 23), ("flat", 8, 64), ("tilted", 7, 7), ("flat", 1, 1)]
LINK_OF_LEVEL = [(7 * lv + 3) % NB for lv in range(NB)]  # scattered over the lanes of an env
# Collinear candidates stay collinear under every rigid motion and under the projection onto the ground: the signed areas of such a plate
# are zero in the first substep (exact state) and rounding noise of either sign in all later ones, in float32 and in float64 alike - there
# "a point on either side" is not a property of the rule.  From the second substep on these links are held to the deepest candidate and
# the farthest from it only.
LINE_LINKS = [LINK_OF_LEVEL[lv] for lv, spec in enumerate(SPECS) if spec[0] == "line"]


@functools.lru_cache(maxsize=None)
def probe_model():
    from vid2player3d_amd.model import BodyModel, load_baked_model

    base = load_baked_model()
    rng = np.random.default_rng(20)
    blob = dict(base.blob)
    local = np.round(np.asarray(base.blob["local_pos"], dtype=np.float64) * GRID) / GRID
    blob["local_pos"] = local
    blob["com"] = np.round(np.asarray(base.blob["com"], dtype=np.float64) * GRID) / GRID  # (the kernel places a link by its centre of mass)
    origin = np.zeros((NB, 3))  # link origins relative to the root, identity rotations
    for b in range(1, NB):
        origin[b] = origin[int(base.parents[b])] + local[b]
    verts, offs = [], [0]
    level_of = {link: lv for lv, link in enumerate(LINK_OF_LEVEL)}
    for b in range(NB):
        lv = level_of[b]
        kind, k, nv = SPECS[lv]
        xy, dz = _plate(kind, k, rng)
        hv = np.zeros((nv, 3))
        where = np.sort(rng.permutation(nv)[:k])  # the plate's vertices keep their order, anywhere among the hull's indices
        top = np.ones(nv, dtype=bool)
        top[where] = False
        # plate: world z = (s + lv) / 1024 + dz when the root stands at z = s / 1024 + 1
        hv[where, :2] = xy
        hv[where, 2] = lv / GRID + dz - 1.0 - origin[b, 2]
        nt = int(top.sum())
        hv[top, :2] = rng.integers(-16, 17, size=(nt, 2)) / 64.0
        hv[top, 2] = lv / GRID - 1.0 - origin[b, 2] + 0.25 + rng.integers(0, 32, size=nt) / 64.0
        verts.append(hv)
        offs.append(offs[-1] + nv)
    blob["hull_verts"] = np.concatenate(verts, axis=0)
    blob["hull_offsets"] = np.asarray(offs, dtype=np.int32)
    return BodyModel(blob, **base.model_kw), origin


def probe_states(counts):
    """Root states [n, 13] (xyzw quaternion), dof positions and velocities: upright, identity rotations, root at the height that brings
    exactly counts[e] links within the contact offset (more than 21: the first ones penetrate), falling and tumbling slowly."""
    n = len(counts)
    root = np.zeros((n, 13), dtype=np.float32)
    for e, c in enumerate(counts):
        s = TOP_LEVEL + 1 - c if c > 0 else 64
        root[e, 2] = 1.0 + s / GRID
    root[:, 6] = 1.0
    root[:, 7:10] = [0.0625, -0.03125, -0.5]
    root[:, 10:13] = [0.125, 0.0625, 0.03125]
    return root, np.zeros((n, 69), dtype=np.float32), np.zeros((n, 69), dtype=np.float32)


def expected_structure(counts):
    """What the poses hold, from numpy alone: candidates per (env, link) with their depths, and the near links per wave."""
    model, origin = probe_model()
    root, _, _ = probe_states(counts)
    n = len(counts)
    cands = [[None] * NB for _ in range(n)]
    near = np.zeros((n, NB), dtype=bool)
    for e in range(n):
        for b in range(NB):
            hv = model.hull_verts[model.hull_offsets[b]:model.hull_offsets[b + 1]]
            z = float(root[e, 2]) + origin[b, 2] + hv[:, 2]
            idx = np.nonzero(z < COFF)[0]
            cands[e][b] = (idx, z[idx])
            near[e, b] = z.min() < COFF + 1e-4
            assert near[e, b] == (len(idx) > 0), "a plate sits between the contact offset and the box cull's margin"
    return cands, near


def oracle_for(counts):
    return P.oracle_for(probe_states(counts), model=probe_model()[0], enable_contact=True)


def test_oracle_alone_produces_every_case():
    """CPU: the oracle's own selection in the first substep of the chosen poses shows every case the GPU tests are about."""
    model, _ = probe_model()
    nverts = np.diff(model.hull_offsets)
    for counts in (COUNTS_34, COUNTS_3):
        n = len(counts)
        cands, near = expected_structure(counts)
        assert near.sum(axis=1).tolist() == [min(c, NB) for c in counts]
        z = np.zeros((n, 69))
        own = oracle_for(counts).step(z, np.zeros((n, 3)), np.zeros((n, 3)), nsub=NSUB, hold=2, want_selection=True)["own"][:, 0]
        seen = set()
        for e in range(n):
            for b in range(NB):
                idx, depth = cands[e][b]
                picks = own[e, b][own[e, b] >= 0] - 64 * b
                if len(idx) <= 4:
                    assert picks.tolist() == idx.tolist(), "up to four candidates are the manifold, in index order"
                    seen.add("cand%d" % len(idx))
                else:
                    assert 2 <= len(picks) <= 4 and set(picks) <= set(idx)
                    tie = int((depth == depth.min()).sum())
                    assert picks[0] == idx[np.argmin(depth)], "deepest candidate, first index on a tie"
                    seen.add("manifold%d" % len(picks))
                    if tie > 1:
                        seen.add("depth tie")
                    d2 = ((model.hull_verts[model.hull_offsets[b] + idx, :2] - model.hull_verts[model.hull_offsets[b] + picks[0], :2]) ** 2).sum(axis=1)
                    assert picks[1] == idx[np.argmax(d2)], "farthest from the deepest, first index on a tie"
                    if int((d2 == d2.max()).sum()) > 1:
                        seen.add("distance tie")
                if len(idx):
                    seen.add("hull<8" if nverts[b] < 8 else "hull64" if nverts[b] == 64 else "hull")
        waves = [near[2 * w:2 * w + 2].sum() for w in range((n + 1) // 2)]
        if n == 34:
            assert {"cand0", "cand1", "cand2", "cand3", "cand4", "manifold2", "manifold3", "manifold4", "depth tie", "hull<8", "hull64"} <= seen, seen
            assert {0, 8, 9, 17} <= set(int(w) for w in waves), waves
            # wave 2 pools 5 + 4: the last near link of env 5 has rank 8, first of the second round; wave 3 pools 9 + 8
            assert counts[4] < 8 <= counts[4] + counts[5] - 1 and counts[6] > 8 and counts[6] + counts[7] == 17
            assert counts[4] == counts[8] == counts[11] and counts[5] != counts[9] and counts[10] != counts[5]
        else:
            assert [int(w) for w in waves] == [9, 9]


# ---------------------------------------------------------------------------------------------------------------- GPU
@functools.lru_cache(maxsize=None)
def run_case(n, build):
    """One control step of the kernel from the probe poses and the oracle's step from the same state with the kernel's vertices forced
    (its own picks and their margins beside them).  Shared by the tests; nothing modifies what it returns."""
    counts = {34: COUNTS_34, 3: COUNTS_3}[n]
    # PD targets = the pose the probes stand in (all joints at zero), no residual wrench: the drives hold the pose, what moves the links
    # is gravity, the root's velocity and the contacts
    got = S.kernel_step(*probe_states(counts), np.zeros((n, 75), dtype=np.float32), build=build, body_model=probe_model()[0])
    return got, S.reference(oracle_for(counts), got)


CASES = [(3, 1), (3, 2), (34, 1), (34, 2)]


@pytest.mark.gpu
@pytest.mark.parametrize("n,build", CASES)
def test_contact_vertex_ids_equal_the_oracles_in_every_substep(n, build):
    got, ref = run_case(n, build)  # (it asserts that the build is the one asked for)
    counts = {34: COUNTS_34, 3: COUNTS_3}[n]
    ids, own = got["ids_sub"], ref["own"]
    assert ids.shape == own.shape == (n, NSUB, NB, 4)
    assert np.array_equal(ids[:, -1], got["ids"])
    # the first substep holds exactly the near links the poses were built for
    assert (ids[:, 0] >= 0).any(axis=-1).sum(axis=1).tolist() == [min(c, NB) for c in counts]
    diff = np.any(ids != own, axis=-1)
    big = (ids[:, 1:, LINE_LINKS] >= 0).sum(axis=-1) + (own[:, 1:, LINE_LINKS] >= 0).sum(axis=-1) > 0
    diff[:, 1:, LINE_LINKS] = np.any(ids[:, 1:, LINE_LINKS, :2] != own[:, 1:, LINE_LINKS, :2], axis=-1) & big
    for e, s, b in zip(*np.nonzero(diff)):
        print("[contact scan] env %d substep %d link %d: kernel %s oracle %s (decision margin %.2e m)" % (e, s, b, ids[e, s, b].tolist(), own[e, s, b].tolist(), ref["margin"][e, s, b]))
    assert not diff.any(), "%d (env, substep, link) triples differ from the oracle's selection" % int(diff.sum())


@pytest.mark.gpu
@pytest.mark.parametrize("n,build", CASES)
def test_state_after_one_control_step_matches_oracle(n, build):
    """The drives hold the probe pose (PD targets = the pose), so the step is as well conditioned as the parity fixtures' and the
    parity tests' bounds apply as they are: measured, 2 of 34 envs need the conditioning term (4 may), largest share of a bound 0.03."""
    from tests.gpu_util import _compare

    got, ref = run_case(n, build)
    assert np.abs(got["cf"]).max() > 1.0, "the contacts must carry load"
    _compare(got, ref, "probe poses n=%d build %d" % (n, build))


@pytest.mark.gpu
@pytest.mark.parametrize("build", [1, 2])
def test_same_env_next_to_different_partners_gives_identical_bits(build):
    """Envs 4, 8 and 11 hold the same state beside partners with 4, 0 and 0 near links, in the lower and the upper half of the wave:
    the same vertices in every substep and bit-identical states and forces."""
    got, _ = run_case(34, build)
    for other in (8, 11):
        assert np.array_equal(got["ids_sub"][4], got["ids_sub"][other])
        for key in ("root", "dpos", "dvel", "rb", "cf", "df"):
            assert np.array_equal(got[key][4], got[key][other]), (key, other)
