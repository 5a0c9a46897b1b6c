"""The numpy oracle on frame-exact motion times, against the reference's answers in tests/golden/frame_times.npz (CPU, no reference, no GPU).

Evaluation (StateInit.Start, 30 fps clips, control step 1/30 s) queries the sampler on a frame boundary at every step, where a float32
truncation decides the frame index and with it the velocity rows; the clip's end is decided by `clock >= length` on the accumulated
float32 clock.  Part S asks the sampler there, part R at the branch points of slerp / quat_to_exp_map, part E steps two Start-mode epochs.
The census asserts that the fixture holds the cases these tests exist for (printed under -s)."""
import numpy as np
import pytest

from oracle import golden_inputs as GI
from oracle import task_oracle as O
from tests import frame_times_fixture as FT
from tests.gpu_util import close


@pytest.mark.parametrize("part", ["S", "R"])
def test_calc_frame_blend_gives_the_references_frames_and_blend_bits(part):
    tabs = FT.tables(part)
    ids, times = FT.queries(part)
    f0, f1, blend = O.calc_frame_blend(times, tabs["motion_lengths"][ids], tabs["motion_num_frames"][ids], tabs["motion_dt"][ids])
    w0, w1, wb = FT.frames(part)
    assert np.array_equal(f0, w0) and np.array_equal(f1, w1)
    FT.assert_bits(blend, wb, "blend of part " + part)


@pytest.mark.parametrize("adjust", [True, False])
@pytest.mark.parametrize("part", ["S", "R"])
def test_oracle_motion_state_on_frame_boundaries_and_branch_points(part, adjust):
    """Positions and velocities bit for bit, rotations and dof_pos within 5e-6 (measured on the reference: 2.4e-7 and 6.1e-7)."""
    ids, times = FT.queries(part)
    got = O.get_motion_state(FT.tables(part), ids, times, adjust, 0.0)
    FT.compare_motion_state(got, part, adjust, "oracle, part " + part, positions_bitwise=True)


def _oracle_partial_reset(task, envs, kp):
    """_reset_envs(env_ids) of the reference in Start mode: the envs' state, clock, target, flags and observation as a fresh reset at time 0
    leaves them; nothing else moves (the reference's _init_context cannot take a subset of the envs, so the context stays)."""
    sub = O.TaskOracle(task.tabs, task.motion_ids[envs], kp)
    sub.reset_all(np.zeros(len(envs), np.float32))
    for name in ("root_states", "dof_pos", "dof_vel", "rb_state", "cur_time", "progress_buf", "reset_buf", "terminate_buf", "obs_buf"):
        getattr(task, name)[envs] = getattr(sub, name)
    for a, b in zip(task.target, sub.target):
        a[envs] = b


def _target_rows(task):
    return np.concatenate([t.reshape(task.n, -1) for t in task.target], axis=1)


@pytest.mark.parametrize("tag", FT.EPOCHS)
def test_task_oracle_start_mode_epoch(tag):
    """TaskOracle from a reset at time 0 until every env's flag is up: flags, progress and the bits of the clock at every step, the bits of the
    target's velocity rows for every env, whole target rows where the fixture has them, reward at the bounds of test_oracle_golden.py."""
    from vid2player3d_amd.model import load_baked_model

    g = FT.golden()
    kp = load_baked_model().kp.astype(np.float32)
    n = len(FT.MOTION_IDS)
    task = O.TaskOracle(FT.tables("E"), FT.MOTION_IDS, kp)
    task.reset_all(np.zeros(n, np.float32))
    FT.assert_bits(task.cur_time, g[tag + "reset_cur_time"], tag + "reset clock")
    close(task.root_states, g[tag + "reset_root_states"], FT.TOL, tag + "root_states")
    close(task.dof_pos, g[tag + "reset_dof_pos"], FT.TOL, tag + "dof_pos")
    FT.assert_bits(task.dof_vel, g[tag + "reset_dof_vel"], tag + "dof_vel")
    close(task.rb_state, g[tag + "reset_rb_state"], FT.TOL, tag + "rb_state")
    close(task.obs_buf, g[tag + "reset_obs"], FT.TOL, tag + "reset obs")
    close(_target_rows(task), g[tag + "reset_target"], FT.TOL, tag + "reset target")
    close(task.context_feat[list(FT.CONTEXT_ENVS), :, :237], g[tag + "context_feat"], FT.TOL, tag + "context_feat")
    assert np.array_equal(task.context_feat[..., 237:309], task.context_feat[..., 0:72]) and np.array_equal(task.context_feat[..., 309:378], task.context_feat[..., 168:237])
    assert np.array_equal(task.context_mask.astype(np.uint8), g[tag + "context_mask"])
    for i in range(FT.epoch_steps(tag)):
        what = "%sstep %d" % (tag, i)
        if FT.has_partial(tag) and i == FT.PARTIAL_AT:
            _oracle_partial_reset(task, FT.PARTIAL_ENVS, kp)
            FT.assert_bits(task.cur_time, g[tag + "partial_cur_time"], what + " clock after the partial reset")
            close(task.obs_buf[FT.PARTIAL_ENVS], g[tag + "partial_obs"], FT.TOL, what + " partial reset obs")
            close(_target_rows(task)[FT.PARTIAL_ENVS], g[tag + "partial_target"], FT.TOL, what + " partial reset target")
            assert np.array_equal(np.stack([task.reset_buf, task.terminate_buf, task.progress_buf]), g[tag + "partial_flags"])
        s = FT.step_inputs(tag, i)
        out = task.pre_physics_step(s["actions"])
        assert np.array_equal((out[0] == 0).all(axis=1).astype(np.uint8), g[tag + "actions_masked_rows"][i]), what
        task.set_sim_state(s["dof_pos"], s["dof_vel"], s["rb_state"])
        task.post_physics_step()
        FT.assert_bits(task.obs_buf, FT.forced_obs(s), what + " obs")
        close(task.rew_buf, g[tag + "rew"][i], 1e-4, what + " rew")
        close(task.sub_rewards, g[tag + "sub_rewards"][i], 5e-4, what + " sub_rewards")
        assert np.array_equal(task.reset_buf, g[tag + "reset"][i]), what
        assert np.array_equal(task.terminate_buf, g[tag + "terminate"][i]), what
        assert np.array_equal(task.progress_buf, g[tag + "progress"][i]), what
        FT.assert_bits(task.cur_time, g[tag + "cur_time"][i], what + " clock")
        FT.compare_target(tag, i, _target_rows(task), what)


def test_census_of_the_fixture():
    """The fixture holds the cases it was made for; the counts are printed under -s."""
    g = FT.golden()
    lines = []

    def say(fmt, *a):
        lines.append(fmt % a)

    # ---- part S
    tabs = FT.tables("S")
    ids, times = FT.queries("S")
    f0, f1, blend = FT.frames("S")
    k = g["s_k"].astype(np.int64)
    nf = tabs["motion_num_frames"][ids]
    on_grid = (k >= 1) & (k <= nf - 1)
    slipped, kept = on_grid & (f0 == k - 1), (k >= 0) & (k <= nf - 1) & (f0 == k)
    start = tabs["length_starts"][ids]
    jump = np.abs(tabs["dvs"][start + np.clip(k, 1, nf - 1) - 1] - tabs["dvs"][start + np.clip(k, 1, nf - 1)]).max(axis=1)
    exact = (g["s_forms"] & 0b001001001) != 0   # one of the three forms as it is, not moved by an ulp
    say("S: %d queries on %d clips (frames %s, fps %s); %d of them one of the three forms unmoved", len(ids), len(tabs["motion_num_frames"]),
        tabs["motion_num_frames"].tolist(), tabs["motion_fps"].astype(int).tolist(), int(exact.sum()))
    say("S: frame index k - 1 (slipped): %d, of them unmoved forms: %d of %d on the grid (%.0f %%); frame index k: %d", int(slipped.sum()), int((slipped & exact).sum()),
        int((on_grid & exact).sum()), 100.0 * (slipped & exact).sum() / max(1, (on_grid & exact).sum()), int(kept.sum()))
    say("S: slipped queries whose dof_vel rows of frames k - 1 and k differ by more than 1e-3: %d (median difference %.2f rad/s)", int((slipped & (jump > 1e-3)).sum()),
        float(np.median(jump[slipped])))
    say("S: last frame %d, blend > 1 %d, blend < 0 %d, two-frame clip %d, time -0.0 %d", int((f0 == nf - 1).sum()), int((blend > 1).sum()), int((blend < 0).sum()),
        int((nf == 2).sum()), int((np.signbit(times) & (times == 0)).sum()))
    assert slipped.sum() >= 500 and kept.sum() >= 500
    assert (slipped & (jump > 1e-3)).sum() >= 400
    assert (f0 == nf - 1).any() and (blend > 1).any() and (blend < 0).any() and (nf == 2).any()
    # ---- part R: the key frames in the tables, the reference's blended rotations
    rt = FT.tables("R")
    cos_l, sin_l = GI.slerp_terms(rt["lrs"][0::2], rt["lrs"][1::2])
    cos_g, sin_g = GI.slerp_terms(rt["grs"][0::2], rt["grs"][1::2])
    cos, sin = np.concatenate([cos_l.ravel(), cos_g.ravel()]), np.concatenate([sin_l.ravel(), sin_g.ravel()])
    inside = np.abs(cos) < 1
    below, above = np.unique(sin[inside & (sin < 1e-3)]), np.unique(sin[inside & (sin >= 1e-3)])
    w = g["r_rb_rot"][..., 3]
    with np.errstate(invalid="ignore"):
        angle = O.quat_to_angle_axis(rt["lrs"])[0]
    say("R: %d pairs; sin_half below 0.001: %s; at or above: %s", len(g["r_labels"]), " ".join("%.3e" % x for x in below), " ".join("%.3e" % x for x in above[:6]))
    near = (w > 1) & (w <= np.nextafter(np.nextafter(np.float32(1), np.float32(2)), np.float32(2)))
    say("R: |cos| >= 1 in %d slots, cos < 0 in %d; blended w == 1: %d, > 1: %d (%d of them one or two ulps, largest 1 + %.1e), < 1: %d; wrapped angle > 0: %d, < 0: %d", int((np.abs(cos) >= 1).sum()),
        int((cos < 0).sum()), int((w == 1).sum()), int((w > 1).sum()), int(near.sum()), float(w.max() - 1), int((w < 1).sum()), int((angle > 0).sum()), int((angle < 0).sum()))
    assert len(below) >= 2 and len(above) >= 2
    assert (np.abs(cos) >= 1).any() and (cos < 0).any()
    assert (w == 1).any() and near.any() and (w < 1).any()
    assert (angle > 0).any() and (angle < 0).any()
    # ---- part E
    et = FT.tables("E")
    enf, length = et["motion_num_frames"][FT.MOTION_IDS], et["motion_lengths"][FT.MOTION_IDS]
    a = "a_"
    rise = np.argmax(g[a + "reset"], axis=0) + 1   # control steps until the flag is up
    by_time = g[a + "terminate"][-1] == 0
    deciding = g[a + "cur_time"][enf - 2, np.arange(len(enf))]   # the clock after nf - 1 steps: frame counting puts it on the clip's length
    off = deciding.view(np.uint32) != length.view(np.uint32)
    dt = np.float32(GI.DT)
    ctx_t = (np.float32(0) + dt) + dt * np.arange(-8, 40).astype(np.float32)
    say("E: frames %s; steps until the reset flag is up %s; terminated early %s", enf.tolist(), rise.tolist(), (~by_time).astype(int).tolist())
    say("E: clock after nf - 1 steps minus the clip length, in ulps: %s", (deciding.view(np.int32) - length.view(np.int32)).tolist())
    say("E: context frames with a negative time %d, frames with mask 0 per env %s; second epoch: envs %s reset again after %d steps, %d steps", int((ctx_t < 0).sum()),
        (g[a + "context_mask"] == 0).sum(axis=1).tolist(), FT.PARTIAL_ENVS.tolist(), FT.PARTIAL_AT, FT.epoch_steps("b_"))
    assert (by_time & (rise == enf - 1)).any() and (by_time & (rise == enf)).any()
    assert (by_time & off).any()
    assert (ctx_t < 0).any() and (g[a + "context_mask"] == 0).any() and (g[a + "context_mask"] == 1).any()
    assert np.array_equal(FT.duration_flags(a)[:, by_time], g[a + "reset"][:, by_time].astype(bool))
    print("\n".join("[census] " + ln for ln in lines))
