"""Poses of the baked body for the phase tests of the link-per-lane physics kernel (tests/test_gpu_tree_passes.py, _contact_scan,
_walk_up, _sweep_visits, _walk_down, _rows_points): forward kinematics in numpy, the pose catalogue and its builder, the states derived
from it, and the oracle set to a batch of them.  numpy and the oracle only - no torch, no GPU.

Every pose is built so that a chosen set of links, and only that set, is within reach of the ground: joint angles put the chosen links
lowest, a few free angles (a tilt of the root, one joint) are solved so that their lowest hull vertices are level, and the root height
sinks them 2 .. 4 mm into the ground; every other link stays more than the contact offset (20 mm) above it.

The random streams are seeded by a pose's place in sorted(POSES) and by the literals 97, 1009 and 131 (tests/test_gpu_rows_points.py):
a new key in POSES moves every state, and the seeds of the fixtures were chosen on the CPU to stay inside the conditioning cap."""
import functools

import numpy as np

from oracle import task_oracle as O
from oracle.phys_oracle import BatchOracle, default_params

NSUB = 4
NB = 24
REST_VEL = 0.05          # joint rates, rad/s
SINK = (0.002, 0.004)    # how far the lowest vertex is inside the ground, m
LEVEL = 5e-4            # the lowest vertices of the chosen links are level within this, m
CLEAR = 0.03             # every link outside the chosen set is at least this far above the lowest vertex, m (contact offset: 0.02)
X, Y, Z = np.eye(3)
# pose: rotations of the root (expmaps about world axes, applied in turn; the baked body lies on its back with the identity rotation),
# joint rotations (expmaps, parent axes: x to the body's left, y up the spine, z forward), the links that touch, and the free angles
# that level them ("root": a tilt about a world axis)
POSES = {
    "ankle_toe": ([X * np.pi / 2], {"R_Hip": X * -0.8, "R_Knee": X * 1.2}, ("L_Ankle", "L_Toe"), [("root", X)]),
    "feet": ([X * np.pi / 2], {}, ("L_Ankle", "L_Toe", "R_Ankle", "R_Toe"), [("root", X), ("root", Y), ("R_Ankle", X)]),
    "hands": ([Y * np.pi], {"L_Shoulder": Y * -np.pi / 2, "R_Shoulder": Y * np.pi / 2}, ("L_Hand", "R_Hand"), [("root", Y)]),
    "head_hand": ([X * -np.pi / 2], {"L_Shoulder": Z * 0.6, "R_Shoulder": Z * np.pi / 2}, ("Head", "L_Hand"), [("L_Shoulder", Z)]),
    "toe_hand": ([Y * np.pi], {"R_Shoulder": Y * np.pi / 2, "R_Hip": X * 0.6}, ("L_Toe", "R_Hand"), [("root", X)]),
    "head": ([X * -np.pi / 2], {}, ("Head",), []),
    "air": ([X * np.pi / 2], {}, (), []),
    # (no chosen set: whatever lies within reach, seven links or more)
    "flat": ([], {}, None, [("root", X), ("root", Y), ("L_Shoulder", Y), ("R_Shoulder", Y), ("Neck", X)]),
}
FLAT_LEVEL = ("L_Hand", "R_Hand", "Pelvis", "Chest", "Head")  # flat: the links the free angles bring level
FLAT_MIN_TOUCHED = 7
# state number of every env: env 0 is state 0 in every batch, its partner (env 1) is state 1 in the small ones and state 3 in the large one
STATE_IDS = {2: [0, 1], 3: [0, 1, 2], 34: [0] + list(range(3, 36))}
# states derived from `feet` (hover, late) and the pose `sit`
FEET = ("L_Ankle", "L_Toe", "R_Ankle", "R_Toe")
HOVER = 0.012           # hover: the lowest vertex is this far above the ground, m (contact offset: 0.02; free fall over the step: 5.4 mm)
ROLL = 0.05             # late: roll of the standing body about its forward axis, rad (feet 0.2 m apart: ~1 cm between their soles)
# sit: the baked body lies on its back; legs raised to the vertical, spine and chest curled up, a tilt of the root levels Pelvis and Torso
SIT = ({"L_Hip": X * -np.pi / 2, "R_Hip": X * -np.pi / 2, "Spine": X * 1.0, "Chest": X * 0.5}, ("Pelvis", "Torso"), X)
CONTACT_OFFSET = 0.02   # a hull vertex closer to the ground than this is a contact point, m
MARGIN = 1e-4           # well_conditioned: EVERY hull vertex of every link is at least this far from CONTACT_OFFSET, m
STRIDE, TRIES = 100, 200  # ... in the first of the states k, k + STRIDE, k + 2 STRIDE, ... that is


def _model():
    from vid2player3d_amd.model import load_baked_model

    return load_baked_model()


def _names():
    return list(_model().body_names)


def _depths():
    par = np.asarray(_model().parents)
    dep = np.zeros(NB, dtype=int)
    for b in range(1, NB):
        dep[b] = dep[par[b]] + 1
    return dep


def _rot_expmap(v):
    a = float(np.linalg.norm(v))
    if a < 1e-12:
        return np.eye(3)
    k = np.asarray(v, dtype=np.float64) / a
    K = np.array([[0, -k[2], k[1]], [k[2], 0, -k[0]], [-k[1], k[0], 0]])
    return np.eye(3) + np.sin(a) * K + (1 - np.cos(a)) * (K @ K)


def _rot_quat(q):  # xyzw
    x, y, z, w = [float(c) for c in q]
    return np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - w * z), 2 * (x * z + w * y)],
                     [2 * (x * y + w * z), 1 - 2 * (x * x + z * z), 2 * (y * z - w * x)],
                     [2 * (x * z - w * y), 2 * (y * z + w * x), 1 - 2 * (x * x + y * y)]])


def _quat_of(R):  # xyzw
    w = np.sqrt(max(0.0, 1 + R[0, 0] + R[1, 1] + R[2, 2])) / 2
    x = np.copysign(np.sqrt(max(0.0, 1 + R[0, 0] - R[1, 1] - R[2, 2])) / 2, R[2, 1] - R[1, 2])
    y = np.copysign(np.sqrt(max(0.0, 1 - R[0, 0] + R[1, 1] - R[2, 2])) / 2, R[0, 2] - R[2, 0])
    z = np.copysign(np.sqrt(max(0.0, 1 - R[0, 0] - R[1, 1] + R[2, 2])) / 2, R[1, 0] - R[0, 1])
    q = np.array([x, y, z, w])
    return q / np.linalg.norm(q)


def _expmap_of(R):
    ang = np.arccos(np.clip((np.trace(R) - 1) / 2, -1, 1))
    if ang < 1e-12:
        return np.zeros(3)
    return np.array([R[2, 1] - R[1, 2], R[0, 2] - R[2, 0], R[1, 0] - R[0, 1]]) * (ang / (2 * np.sin(ang)))


def _hull_heights(quat, dpos):
    """Heights of the hull vertices of every link above the root's origin, link by link (forward kinematics, float64)."""
    m = _model()
    par, lp = np.asarray(m.parents), np.asarray(m.local_pos, dtype=np.float64)
    hv, ho = np.asarray(m.hull_verts, dtype=np.float64), np.asarray(m.hull_offsets)
    R, x = [None] * NB, np.zeros((NB, 3))
    R[0] = _rot_quat(quat)
    for b in range(NB):
        if b:
            p = int(par[b])
            x[b] = x[p] + R[p] @ lp[b]
            R[b] = R[p] @ _rot_expmap(dpos[3 * (b - 1):3 * b])
        yield (hv[ho[b]:ho[b + 1]] @ R[b].T)[:, 2] + x[b, 2]


def lowest_point(quat, dpos):
    """Height of the lowest hull vertex of every link above the root's origin."""
    return np.array([z.min() for z in _hull_heights(quat, dpos)])


def vertex_heights(root, dpos):
    """Height above the ground of every hull vertex of every link, as one array, and the link of each."""
    out = [z + float(root[2]) for z in _hull_heights(root[3:7], dpos)]
    return np.concatenate(out), np.concatenate([np.full(len(z), b) for b, z in enumerate(out)])


def posed(pose, rng):
    """Root quaternion (xyzw) and joint angles [69] of a pose, with small random joint angles and a small random tilt under it, the
    free angles solved (Gauss-Newton on the forward kinematics) so that the lowest vertices of the chosen links are level."""
    idx = {nm: i for i, nm in enumerate(_names())}
    rots, joints, chosen, free = POSES[pose]
    R0 = np.eye(3)
    for v in rots:
        R0 = _rot_expmap(v) @ R0
    R0 = _rot_expmap(rng.normal(0, 0.002, size=3)) @ R0
    noise = rng.normal(0, 0.004, size=69)
    fixed = {idx[j]: _rot_expmap(v) for j, v in joints.items()}

    def at(p):
        R, dp = R0, dict(fixed)
        for (what, ax), a in zip(free, p):
            if what == "root":
                R = _rot_expmap(ax * a) @ R
            else:
                dp[idx[what]] = dp.get(idx[what], np.eye(3)) @ _rot_expmap(ax * a)
        dpos = np.concatenate([_expmap_of(dp.get(b, np.eye(3)) @ _rot_expmap(noise[3 * (b - 1):3 * b])) for b in range(1, NB)])
        return _quat_of(R), dpos

    p = np.zeros(len(free))
    if free:
        ids = [idx[c] for c in (FLAT_LEVEL if chosen is None else chosen)]

        def resid(p):
            low = lowest_point(*at(p))[ids]
            return low - low.mean()

        for _ in range(40):  # (damped: the lowest vertex of a hull is a piecewise linear function of the angles)
            r = resid(p)
            if np.abs(r).max() < 1e-7:
                break
            J = np.stack([(resid(p + 1e-5 * e) - r) / 1e-5 for e in np.eye(len(p))], axis=1)
            step, t = np.clip(np.linalg.lstsq(J, r, rcond=None)[0], -0.05, 0.05), 1.0
            while t > 1e-3 and np.abs(resid(p - t * step)).max() >= np.abs(r).max():
                t *= 0.5
            p = p - t * step
    return at(p)


def _resting(q, dpos, chosen, rng, what):
    """A state at rest in a pose: small joint and root rates, the chosen links level and every other link CLEAR above them, the lowest
    vertex SINK inside the ground (no chosen link: 3 m up), a small residual wrench."""
    root = np.zeros(13)
    root[3:7] = q
    dvel = rng.normal(0, REST_VEL, size=69)
    root[7:10] = rng.normal(0, 0.4 * REST_VEL, size=3)
    root[10:13] = rng.normal(0, 0.4 * REST_VEL, size=3)
    root, dpos, dvel = root.astype(np.float32), dpos.astype(np.float32), dvel.astype(np.float32)
    low = lowest_point(root[3:7], dpos)
    if chosen:
        ids = [_names().index(c) for c in chosen]
        assert np.ptp(low[ids]) < LEVEL and np.delete(low, ids).min() > low[ids].max() + CLEAR, (what, np.round(np.sort(low) - low.min(), 4)[:6])
    root[2] = 3.0 if chosen == () else -low.min() - rng.uniform(*SINK)
    return root, dpos, dvel, rng.normal(0, 0.02, size=6).astype(np.float32)


@functools.lru_cache(maxsize=None)
def sit_state(seed, k):
    """State k of the pose SIT: the tilt of the root about the body's left axis is solved so that the lowest vertices of Pelvis and
    Torso are level; every other link stays more than CLEAR above them."""
    names = _names()
    rng = np.random.default_rng([1009, seed, k])
    joints, chosen, axis = SIT
    fixed = {names.index(j): _rot_expmap(v) for j, v in joints.items()}
    R0 = _rot_expmap(rng.normal(0, 0.002, size=3))
    noise = rng.normal(0, 0.004, size=69)
    dpos = np.concatenate([_expmap_of(fixed.get(b, np.eye(3)) @ _rot_expmap(noise[3 * (b - 1):3 * b])) for b in range(1, NB)])
    ids = [names.index(c) for c in chosen]

    def resid(a):
        low = lowest_point(_quat_of(_rot_expmap(axis * a) @ R0), dpos)[ids]
        return low[1] - low[0]

    lo, hi = -0.6, 0.6  # (bisection: the difference of the two lowest vertices is monotonic in the tilt over this range)
    assert resid(lo) * resid(hi) < 0, (resid(lo), resid(hi))
    for _ in range(60):
        mid = 0.5 * (lo + hi)
        lo, hi = (mid, hi) if resid(lo) * resid(mid) > 0 else (lo, mid)
    return _resting(_quat_of(_rot_expmap(axis * 0.5 * (lo + hi)) @ R0), dpos, chosen, rng, ("sit", k))


@functools.lru_cache(maxsize=None)
def state(pose, seed, k):
    """State number k of a pose: root [13] (xyzw quaternion), dof positions [69], dof velocities [69], residual wrench action [6].
    Beside the keys of POSES: `sit`; `flat2`, a `flat` state (which of them, well_conditioned() decides); and `hover` / `late`, the
    `feet` state lifted / rolled so that the left foot is the higher one."""
    if pose == "sit":
        return sit_state(seed, k)
    if pose == "flat2":
        return state("flat", seed, k)
    if pose not in ("hover", "late"):
        rng = np.random.default_rng([sorted(POSES).index(pose), seed, k])
        return _resting(*posed(pose, rng), POSES[pose][2], rng, (pose, k))
    root, dpos, dvel, wrench = [a.copy() for a in state("feet", seed, k)]
    if pose == "hover":
        root[2] = -lowest_point(root[3:7], dpos).min() + HOVER
        return root, dpos, dvel, wrench
    feet = [_names().index(c) for c in FEET]
    rng = np.random.default_rng([97, seed, k])
    for sign in (1.0, -1.0):  # (the forward axis of the standing body is a world axis up to its small random tilt)
        q = _quat_of(_rot_expmap(Y * sign * ROLL) @ _rot_quat(root[3:7])).astype(np.float32)
        low = lowest_point(q, dpos)
        if low[feet[:2]].min() > low[feet[2:]].min():
            break
    root[3:7] = q
    root[2] = -low.min() - rng.uniform(*SINK)
    return root, dpos, dvel, wrench


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
            if (below > 0).sum() < FLAT_MIN_TOUCHED or (pose == "flat2" and not (below == 2).any()):
                continue
        return st
    raise AssertionError("no state of %s among %d keeps %g m" % (pose, TRIES, MARGIN))


# ---------------------------------------------------------------------------------------------------------------- batches
def stack(parts):
    """Per-env states (root, dpos, dvel, wrench) -> the batch's [root [n, 13], dpos [n, 69], dvel [n, 69], wrench [n, 6]]."""
    parts = list(parts)
    return [np.stack([p[i] for p in parts]) for i in range(4)]


def actions(st):
    """PD targets = the pose the batch is in (the drives hold it), plus its residual wrench."""
    return np.concatenate([st[1], st[3]], axis=1).astype(np.float32)


def oracle_inputs(st):
    """What pre_physics makes of actions(st) in that state, no env resetting: PD targets, force and torque on the root."""
    _, pd, _, force, torque = O.pre_physics(actions(st), np.zeros(len(st[0]), dtype=np.int64), st[1], st[0][:, 3:7], _model().kp.astype(np.float32))
    return pd, force, torque


def oracle_for(st, model=None, **params):
    """A fresh float64 oracle set to a batch's state (step() advances it: one per step).  params: fields of default_params."""
    oracle = BatchOracle(_model() if model is None else model, len(st[0]), default_params(**params))
    oracle.set_state(*st[:3])
    return oracle
