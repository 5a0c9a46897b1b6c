"""Readers of tests/golden/frame_times.npz (oracle/gen_golden_frame_times.py) shared by the CPU and the GPU tests of the frame-exact motion
times: the reference's tables, the queries of parts S (frame boundaries) and R (rotation branch points) with what the reference answers,
the Start-mode epochs of part E with their regenerated forced states, and the comparison both tests hold their subject to.

The fixture stores no output twice (the generator checked each identity on the reference's own outputs): velocities are the table rows of
frame_idx0, root_pos / root_rot / key_pos are rows of rb_pos / rb_rot, adjust_height moves the z of the positions only, and the task's
observation after a step is the forced state.  `expected()` puts the nine outputs together again; rb_pos / rb_rot / dof_pos / key_pos of
part S exist for the rows `s_rows` only."""
import os

import numpy as np

from oracle import golden_inputs as GI
from oracle import task_oracle as O
from tests.gpu_util import close

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "frame_times.npz")
KEY = list(O.KEY_BODY_IDS)
BITWISE_ALWAYS = ("root_vel", "root_ang_vel", "dof_vel")   # table rows: any difference is a wrong frame
POSITIONS = ("root_pos", "key_pos", "rb_pos")
TOL = 5e-6   # the bound of test_motion_state_matches_reference_golden
_cache = {}


def golden():
    if "d" not in _cache:
        with np.load(GOLDEN, allow_pickle=False) as z:
            _cache["d"] = {k: z[k] for k in z.files}
    return _cache["d"]


def tables(part="S"):
    """The reference's tables as oracle.task_oracle / MotionLib take them: the nine clips of parts S and E, or the two-frame clips of part R."""
    pre = "tab_" if part in ("S", "E") else "r_tab_"
    return {k[len(pre):]: v for k, v in golden().items() if k.startswith(pre)}


def queries(part):
    g, p = golden(), part.lower() + "_"
    return g[p + "ids"].astype(np.int64), g[p + "times"]


def frames(part):
    g, p = golden(), part.lower() + "_"
    return g[p + "f0"].astype(np.int64), g[p + "f1"].astype(np.int64), g[p + "blend"]


def expected(part, adjust):
    """{output name: (rows or None for all, values)}: the reference's get_motion_state(..., return_rigid_body=True, adjust_height=adjust)."""
    g, tabs = golden(), tables(part)
    ids, _ = queries(part)
    f0l = frames(part)[0] + tabs["length_starts"][ids]
    out = {"root_vel": (None, tabs["grvs"][f0l]), "root_ang_vel": (None, tabs["gravs"][f0l]), "dof_vel": (None, tabs["dvs"][f0l])}
    p = part.lower() + "_"
    rows = g["s_rows"].astype(np.int64) if part == "S" else None
    rb_pos = g[p + "rb_pos"].copy()
    if not adjust:
        rb_pos[..., 2] = g[p + "rb_z_noadj"]
    out.update(dof_pos=(rows, g[p + "dof_pos"]), rb_pos=(rows, rb_pos), rb_rot=(rows, g[p + "rb_rot"]), key_pos=(rows, rb_pos[:, KEY]))
    if part == "S":
        root_pos = g["s_root_pos"].copy()
        if not adjust:
            root_pos[:, 2] = g["s_root_z_noadj"]
        out.update(root_pos=(None, root_pos), root_rot=(None, g["s_root_rot"]))
    else:
        out.update(root_pos=(None, rb_pos[:, 0]), root_rot=(None, g[p + "rb_rot"][:, 0]))
    return out


def bits_equal(a, b):
    a, b = np.ascontiguousarray(a, dtype=np.float32), np.ascontiguousarray(b, dtype=np.float32)
    return a.shape == b.shape and np.array_equal(a.view(np.uint32), b.view(np.uint32))


def assert_bits(a, b, what):
    a, b = np.ascontiguousarray(a, dtype=np.float32), np.ascontiguousarray(b, dtype=np.float32)
    assert a.shape == b.shape, (what, a.shape, b.shape)
    bad = a.view(np.uint32) != b.view(np.uint32)
    assert not bad.any(), "%s: %d of %d elements differ in their bits, first at %s (%r != %r)" % (
        what, int(bad.sum()), bad.size, tuple(int(x) for x in np.argwhere(bad)[0]), a[bad][0], b[bad][0])


def compare_motion_state(got, part, adjust, what, positions_bitwise=False):
    """`got`: the nine outputs in the order of O.MOTION_STATE_NAMES.  Velocities bit for bit; positions bit for bit where the subject states
    the reference's float32 arithmetic without contraction (the numpy oracle, the sampler kernel) and within TOL otherwise; rotations and
    dof_pos within TOL; no NaN (`close`).  Prints the largest error and the number of elements whose bits differ for what stands at TOL."""
    want = expected(part, adjust)
    for name, r in zip(O.MOTION_STATE_NAMES, got):
        rows, w = want[name]
        r = np.asarray(r) if rows is None else np.asarray(r)[rows]
        label = "%s %s%s" % (what, name, "" if adjust else " (no height adjustment)")
        assert not np.isnan(w).any()   # (the reference answers no query of this fixture with NaN)
        if name in BITWISE_ALWAYS or (positions_bitwise and name in POSITIONS):
            assert_bits(r, w, label)
        else:
            print("[frame times] %-58s max |err| %.1e, %d of %d elements differ in their bits" % (
                label, float(np.abs(r.astype(np.float64) - w).max()), int((np.ascontiguousarray(r, dtype=np.float32).view(np.uint32) != np.ascontiguousarray(w).view(np.uint32)).sum()), w.size))
            close(r, w, TOL, label)


# ---- part E ---------------------------------------------------------------------------------------------------------------------------
EPOCHS = ("a_", "b_")
MOTION_IDS = GI.FT_EPOCH_MOTION_IDS
CONTEXT_ENVS = (0, 4)          # envs whose context rows are stored; envs 1 and 5 start on the same clips at the same time
PARTIAL_AT, PARTIAL_ENVS = GI.FT_PARTIAL_AT, GI.FT_PARTIAL_ENVS
SLICES = {"root_pos": (0, 3), "root_rot": (3, 7), "dof_pos": (7, 76), "root_vel": (76, 79), "root_ang_vel": (79, 82), "dof_vel": (82, 151), "key_pos": (151, 163),
          "rb_pos": (163, 235), "rb_rot": (235, 331)}   # columns of a stored target row, in the order of O.MOTION_STATE_NAMES


def epoch_steps(tag):
    return int(golden()[tag + "steps"])


def has_partial(tag):
    return tag == "b_"


def step_inputs(tag, i):
    """Forced state and actions of step i of an epoch (the generator's own call): the oracle's state one frame ahead of the env's clock,
    perturbed; env 5 drops its head from step 5 on, env 7 dips at steps 20 and 21."""
    start = np.zeros(len(MOTION_IDS), np.float32)
    if has_partial(tag) and i >= PARTIAL_AT:
        start[PARTIAL_ENVS] = -np.float32(PARTIAL_AT) * np.float32(GI.DT)
    return GI.env_trace_step_inputs(tables("E"), MOTION_IDS, start, i, seed=GI.FT_EPOCH_SEED)


def forced_obs(s):
    """The reference's obs_buf after the step (checked by the generator bit for bit): the forced state in the order of obs_names."""
    n = len(MOTION_IDS)
    rb = s["rb_state"]
    return np.concatenate([rb[..., 0:3].reshape(n, -1), rb[..., 3:7].reshape(n, -1), s["dof_pos"], s["dof_vel"], rb[..., 7:10].reshape(n, -1),
                           rb[..., 10:13].reshape(n, -1), tables("E")["motion_bodies"][MOTION_IDS]], axis=1).astype(np.float32)


def duration_flags(tag):
    """[steps, envs] the duration part of the reference's reset flag, sticky: cur_time >= clip length on the reference's own float32 clock
    (max_episode_length is out of reach); an env that a partial reset restarts drops its flag there."""
    g = golden()
    length = tables("E")["motion_lengths"][MOTION_IDS]
    up = g[tag + "cur_time"] >= length[None, :]
    out = np.zeros_like(up)
    held = np.zeros(len(MOTION_IDS), bool)
    for i in range(len(up)):
        if has_partial(tag) and i == PARTIAL_AT:
            held[PARTIAL_ENVS] = False
        held |= up[i]
        out[i] = held
    return out


def target_velocity_rows(tag, i):
    """(root_vel, root_ang_vel, dof_vel) of every env's target after step i: the rows of the frame the reference took them from."""
    tabs = tables("E")
    f0l = golden()[tag + "target_f0"][i].astype(np.int64) + tabs["length_starts"][MOTION_IDS]
    return tabs["grvs"][f0l], tabs["gravs"][f0l], tabs["dvs"][f0l]


def compare_target(tag, i, target, what):
    """`target` [envs, 331] after step i: the velocities of every env bit for bit, the whole row of the sampled (step, env) pairs within TOL."""
    g = golden()
    for name, w in zip(BITWISE_ALWAYS, target_velocity_rows(tag, i)):
        a, b = SLICES[name]
        assert_bits(target[:, a:b], w, "%s %s" % (what, name))
    for r in np.nonzero(g[tag + "target_step"] == i)[0]:
        e = int(g[tag + "target_env"][r])
        for name, (a, b) in SLICES.items():
            close(target[e, a:b], g[tag + "target_rows"][r, a:b], TOL, "%s env %d target %s" % (what, e, name))
