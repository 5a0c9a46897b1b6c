"""The HIP sampler and the task state machine on frame-exact motion times, against the reference's answers in tests/golden/frame_times.npz.

In evaluation (StateInit.Start, 30 fps clips, control step 1/30 s) every query of every step sits on a frame boundary: `frame_lookup`
(csrc/motion_sample.inc) decides the frame index by a float32 truncation, `post_env` (csrc/post_ops.inc) the clip's end by `clock >= length`,
`env_context_kernel` (csrc/task_ops.hip) the context mask by `t <= length + 2 dt`.  The velocities of a motion state are the table rows of
the frame: they are compared bit for bit, so is the clock; the sampler's positions too.  Everything else stands at the bounds of
test_gpu_task_ops.py."""
import ctypes as C

import numpy as np
import pytest
import torch

from oracle import golden_inputs as GI
from oracle import task_oracle as O
from tests import frame_times_fixture as FT
from tests.gpu_util import DEV, N, T, close, make_task
from tests.guarded import Guarded

pytestmark = pytest.mark.gpu
NENV = len(FT.MOTION_IDS)


@pytest.fixture(scope="module")
def libs():
    from vid2player3d_amd.motion_lib import MotionLib

    return {part: MotionLib(FT.tables(part), DEV) for part in ("S", "R")}


@pytest.mark.parametrize("adjust", [True, False])
@pytest.mark.parametrize("part", ["S", "R"])
def test_motion_state_on_frame_boundaries_and_branch_points(libs, part, adjust):
    ids, times = FT.queries(part)
    res = libs[part].get_motion_state(T(ids, torch.long), T(times), return_rigid_body=True, adjust_height=adjust, ground_tolerance=0.0)
    # (positions bit for bit as well, which is more than the 5e-6 asked of them: the blend of two table rows is the reference's three float32
    # operations on the reference's blend, and the sampler's translation unit is built without contraction - a blend that differs in its last
    # bit, invisible at 5e-6, shows here)
    FT.compare_motion_state([N(r) for r in res], part, adjust, "kernel, part " + part, positions_bitwise=True)


def test_motion_state_on_every_frame_of_clips_of_2_to_130_frames():
    """Every frame time of 129 clips in its nine float32 forms, one launch through the C entry with the outputs between guard rows, against
    the numpy oracle (itself held to the reference on such times by tests/test_frame_times.py, positions and velocities bit for bit):
    velocities and positions bit for bit, rotations and dof_pos within 5e-6."""
    from vid2player3d_amd import _lib, motion_tables, synth
    from vid2player3d_amd.model import load_baked_model
    from vid2player3d_amd.motion_lib import MotionLib

    m = load_baked_model()
    tabs = motion_tables.build_tables([synth.make_clip(np.random.default_rng(500 + nf), nf) for nf in range(2, 131)], m.parents, m.local_pos)
    ids, times, ks, _ = GI.frame_time_queries(tabs["motion_dt"], tabs["motion_lengths"], tabs["motion_num_frames"])
    q = len(ids)
    f0 = O.calc_frame_blend(times, tabs["motion_lengths"][ids], tabs["motion_num_frames"][ids], tabs["motion_dt"][ids])[0]
    on_grid = (ks >= 1) & (ks <= tabs["motion_num_frames"][ids] - 1)
    assert q > 25000 and (on_grid & (f0 == ks - 1)).sum() > 5000 and (on_grid & (f0 == ks)).sum() > 5000
    lib = MotionLib(tabs, DEV)
    G = Guarded(DEV)
    shapes = [(q, 3), (q, 4), (q, 69), (q, 3), (q, 3), (q, 69), (q, 4, 3), (q, 24, 3), (q, 24, 4)]
    outs = [G.empty(name, s) for name, s in zip(O.MOTION_STATE_NAMES, shapes)]
    d_ids, d_times = G.of("ids", ids, torch.int64), G.of("times", times, torch.float32)
    G.arm()
    arr = (C.c_void_p * 9)(*[o.data_ptr() for o in outs])
    _lib.check(_lib.load().v2p_motion_state(lib.handle(), _lib.ptr(d_ids), _lib.ptr(d_times), q, 1, 0.0, C.byref(arr), _lib.current_stream(torch.device(DEV))),
               "v2p_motion_state")
    G.check()
    ref = O.get_motion_state(tabs, ids, times, True, 0.0)
    for name, r, o in zip(O.MOTION_STATE_NAMES, outs, ref):
        if name in FT.BITWISE_ALWAYS or name in FT.POSITIONS:
            FT.assert_bits(N(r), o, "sweep " + name)
        else:
            close(N(r), o, FT.TOL, "sweep " + name)


def _snapshot(task):
    return {k: N(v).copy() for k, v in (("obs", task.obs_buf), ("cur_time", task._cur_ref_motion_times), ("t0", task._target_bufs[0]), ("t1", task._target_bufs[1]),
                                        ("context_feat", task.context_feat), ("context_mask", task.context_mask), ("progress", task.progress_buf),
                                        ("reset", task.reset_buf), ("terminate", task._terminate_buf), ("root", task._humanoid_root_states), ("dof_pos", task._dof_pos),
                                        ("dof_vel", task._dof_vel), ("rb", task._rigid_body_state))}


def _target(task):
    return N(task._target_bufs[task._cur])


@pytest.mark.parametrize("tag", FT.EPOCHS)
def test_start_mode_epoch_replay_matches_the_reference(libs, tag):
    """The reference's HumanoidSMPLIM in StateInit.Start, physics teacher-forced, from the task's own reset() until every reset flag is up
    (test_env_trace_replay_matches_reference on frame-exact times): flags, progress and context mask equal, the clock and the target's
    velocity rows bit for bit.  In the second epoch envs 1 and 3 are reset again after 10 steps: the other envs keep their bits."""
    g = FT.golden()
    task = make_task(NENV, libs["S"], motion_ids=FT.MOTION_IDS, stateInit="Start")
    task.reset()
    assert not N(task._reset_ref_motion_times).any()
    FT.assert_bits(N(task._cur_ref_motion_times), g[tag + "reset_cur_time"], tag + "reset clock")
    close(N(task._humanoid_root_states), g[tag + "reset_root_states"], FT.TOL, tag + "root_states")
    close(N(task._dof_pos), g[tag + "reset_dof_pos"], FT.TOL, tag + "dof_pos")
    FT.assert_bits(N(task._dof_vel), g[tag + "reset_dof_vel"], tag + "dof_vel")
    close(N(task._rigid_body_state).reshape(NENV, 24, 13), g[tag + "reset_rb_state"], FT.TOL, tag + "rb_state")
    close(N(task.obs_buf), g[tag + "reset_obs"], FT.TOL, tag + "reset obs")
    close(_target(task), g[tag + "reset_target"], FT.TOL, tag + "reset target")
    feat = N(task.context_feat)
    for row, e in enumerate(FT.CONTEXT_ENVS):   # (envs e and e + 1 start on the same clip at the same time)
        close(feat[e, :, :237], g[tag + "context_feat"][row], FT.TOL, tag + "context_feat env %d" % e)
        assert np.array_equal(feat[e + 1], feat[e])
    assert np.array_equal(feat[..., 237:309], feat[..., 0:72]) and np.array_equal(feat[..., 309:378], feat[..., 168:237])
    assert np.array_equal(N(task.context_mask).astype(np.uint8), g[tag + "context_mask"])
    assert not N(task.reset_buf).any() and not N(task._terminate_buf).any() and not N(task.progress_buf).any()
    for i in range(FT.epoch_steps(tag)):
        what = "%sstep %d" % (tag, i)
        if FT.has_partial(tag) and i == FT.PARTIAL_AT:
            before = _snapshot(task)
            task.reset(T(FT.PARTIAL_ENVS, torch.long))
            after = _snapshot(task)
            keep = np.setdiff1d(np.arange(NENV), FT.PARTIAL_ENVS)
            for k in before:
                a, b = after[k].reshape(NENV, -1)[keep], before[k].reshape(NENV, -1)[keep]
                assert np.array_equal(a.view(np.uint8), b.view(np.uint8)), "%s: the partial reset changed %s of an env it does not reset" % (what, k)
            FT.assert_bits(after["cur_time"], g[tag + "partial_cur_time"], what + " clock after the partial reset")
            close(after["obs"][FT.PARTIAL_ENVS], g[tag + "partial_obs"], FT.TOL, what + " partial reset obs")
            close(_target(task)[FT.PARTIAL_ENVS], g[tag + "partial_target"], FT.TOL, what + " partial reset target")
            close(after["root"][FT.PARTIAL_ENVS], g[tag + "partial_root_states"], FT.TOL, what + " partial reset root states")
            close(after["rb"].reshape(NENV, 24, 13)[FT.PARTIAL_ENVS], g[tag + "partial_rb_state"], FT.TOL, what + " partial reset rb_state")
            assert np.array_equal(np.stack([after["reset"], after["terminate"], after["progress"]]), g[tag + "partial_flags"])
            # (the reference's _init_context cannot take a subset of the envs; the engine rebuilds the windows of the reset envs: the rows of
            # a reset of the same clip at time 0)
            close(after["context_feat"][1, :, :237], g[tag + "context_feat"][0], FT.TOL, what + " context of env 1")
            assert np.array_equal(after["context_mask"][FT.PARTIAL_ENVS].astype(np.uint8), g[tag + "context_mask"][FT.PARTIAL_ENVS])
        s = FT.step_inputs(tag, i)
        a = T(s["actions"])
        task.pre_physics_step(a)
        assert np.array_equal((N(a) == 0).all(axis=1).astype(np.uint8), g[tag + "actions_masked_rows"][i]), what
        task._dof_pos[:] = T(s["dof_pos"])
        task._dof_vel[:] = T(s["dof_vel"])
        task._rigid_body_state.view(NENV, 24, 13)[:] = T(s["rb_state"])
        task._humanoid_root_states[:] = T(s["rb_state"][:, 0, :])
        task._reset_env_tensors(None, with_rb_state=True)
        task.post_physics_step()
        close(N(task.obs_buf), FT.forced_obs(s), FT.TOL, what + " obs")
        close(N(task.rew_buf), g[tag + "rew"][i], 1e-4, what + " rew")
        close(N(task.extras["sub_rewards"]), g[tag + "sub_rewards"][i], 5e-4, what + " sub_rewards")
        assert np.array_equal(N(task.reset_buf), g[tag + "reset"][i]), what
        assert np.array_equal(N(task.extras["terminate"]), g[tag + "terminate"][i]), what
        assert np.array_equal(N(task.progress_buf), g[tag + "progress"][i]), what
        FT.assert_bits(N(task._cur_ref_motion_times), g[tag + "cur_time"][i], what + " clock")
        FT.compare_target(tag, i, _target(task), what)
    task.close()


@pytest.mark.parametrize("build", [1, 2])
def test_fused_step_keeps_the_clock_and_targets_of_the_staged_step(libs, build):
    """The fused step (the target of a step is sampled inside the physics kernel, namespace strict of physics_ll.hip) cannot be teacher-forced:
    the same Start-mode epoch with real physics and early termination off, staged and fused.  Clock, progress, the duration flag and both
    target buffers: the fused run's bits are the staged run's at every step, and the reference's (clock, velocity rows, flag steps)."""
    g, tag = FT.golden(), "a_"
    want_flags = FT.duration_flags(tag)
    runs = {}
    for mode in ("staged", "fused"):
        task = make_task(NENV, libs["S"], motion_ids=FT.MOTION_IDS, stateInit="Start", enableEarlyTermination=False, kernel_build=build)
        task.reset()
        rec = []
        for i in range(FT.epoch_steps(tag)):
            a = T(FT.step_inputs(tag, i)["actions"])
            if mode == "fused":
                task.step_fused(a)
            else:
                task.pre_physics_step(a)
                task._physics_step()
                task.post_physics_step()
            rec.append(dict(cur_time=N(task._cur_ref_motion_times).copy(), progress=N(task.progress_buf).copy(), reset=N(task.reset_buf).copy(),
                            terminate=N(task._terminate_buf).copy(), cur=task._cur, t0=N(task._target_bufs[0]).copy(), t1=N(task._target_bufs[1]).copy()))
        task.check()
        task.close()
        runs[mode] = rec
    for i, (s, f) in enumerate(zip(runs["staged"], runs["fused"])):
        what = "build %d step %d" % (build, i)
        for r, mode in ((s, "staged"), (f, "fused")):
            FT.assert_bits(r["cur_time"], g[tag + "cur_time"][i], "%s %s clock" % (what, mode))
            assert np.array_equal(r["progress"], g[tag + "progress"][i]), (what, mode)
            assert np.array_equal(r["reset"].astype(bool), want_flags[i]) and not r["terminate"].any(), (what, mode, r["reset"], want_flags[i])
            FT.compare_target(tag, i, r["t%d" % r["cur"]], "%s %s" % (what, mode))
        assert s["cur"] == f["cur"]
        FT.assert_bits(f["t0"], s["t0"], what + " target buffer 0, fused against staged")
        FT.assert_bits(f["t1"], s["t1"], what + " target buffer 1, fused against staged")
