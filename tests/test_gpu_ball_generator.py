"""The pool of incoming launches (vid2player3d_amd/ball_traj.py): TennisBallGenerator's filter recomputed in numpy, the pool file and its
offline reader, the reference's index rules, and a racket + ball task that draws its balls from the pool."""
import numpy as np
import pytest
import torch

from tests import ball_oracle as B
from vid2player3d_amd import ball_traj

gpu = pytest.mark.gpu
DEV = "cuda:0"


@pytest.fixture(scope="module")
def gen():
    return ball_traj.TennisBallGenerator({"num_samples": 1000}, device=DEV, seed=11)


def numpy_filter(g, calls, cfg, frames):
    """The five conditions of utils/tennis_ball.py:319-327 from per-call positions [n,S,3] of the drawn launches, in numpy."""
    lo, hi = g.bounce_min.cpu().numpy(), g.bounce_max.cpu().numpy()
    cfi = cfg["control_freq_inv"]
    rows = []
    for c in calls:
        s = np.zeros((len(c), 13))
        s[:, 0:3] = c
        bk = B.bookkeeping(cfg, s, frames)
        peak = c[::cfi][bk["bounce_idx"]:frames, 2].max()
        rows.append((bool(bk["pass_net"]), bk["bounce_pos"][0] > lo[0], bk["bounce_pos"][0] < hi[0], bk["bounce_pos"][1] > lo[1], bk["bounce_pos"][1] < hi[1], peak > 1.0,
                     bk["bounce_pos"].sum()))
    rows = np.array(rows)
    return rows[:, :6].astype(bool), rows[:, 6].sum() != 0


@gpu
def test_reset_keeps_exactly_the_launches_that_pass_the_filter(gen):
    d = gen.last_draw
    n, F = gen.num_env, gen.traj_length
    valid = d["valid"].cpu().numpy()
    # (under the oracle 4 of 16 launches of the default ranges pass: a pool of 1000 cannot come out empty unless the kernel is wrong)
    assert 0.05 * n < valid.sum() < 0.8 * n and len(gen.traj_pool) == valid.sum()
    # the same launches, one frame per simulate() call: bit-identical physics, positions at the start of every call
    cfi = gen.sim["control_freq_inv"]
    res = ball_traj.rollout(dict(gen.sim, control_freq_inv=1), d["launch_pos"], d["launch_vel"], d["launch_vspin"], num_frames=F * cfi, want=("traj",))
    calls = res["traj"].cpu().numpy()
    assert np.array_equal(calls[:, ::cfi], d["traj"].cpu().numpy()), "frame t is the position at the start of control step t"
    f32 = lambda v: float(np.float32(v))   # (the kernel compares float32 heights with float32 thresholds)
    conds, any_bounce = numpy_filter(gen, calls.astype(np.float64), dict(gen.sim, net_height=f32(gen.sim["net_height"]), bounce_height=f32(gen.sim["bounce_height"])), F)
    assert any_bounce
    ok = conds.all(axis=1)
    assert np.array_equal(ok, valid), "kept launches satisfy every condition, dropped ones fail at least one (%d differ)" % int((ok != valid).sum())
    for k, what in enumerate(("net", "x >", "x <", "y >", "y <", "peak")):
        assert (~conds[:, k]).any() or what in ("x >", "x <"), "no launch of the draw fails condition %r: it is not tested" % what
    # the pool is the kept rows, in draw order
    assert torch.equal(gen.traj_pool, d["traj"][d["valid"]]) and torch.equal(gen.launch_vspin, d["launch_vspin"][d["valid"]])
    tr, lp, lv, ls = gen.generate_all()
    assert tr is gen.traj_pool and tr.is_cuda and tr.shape[1:] == (100, 3)
    t2, p2, v2, s2 = gen.generate(7, need_init_state=True)
    assert t2.shape == (7, 100, 3) and torch.equal(t2[:, 0], p2)
    p3, v3, s3 = gen.generate_init_state(5)
    assert p3.shape == (5, 3) and s3.shape == (5,)


@gpu
def test_draws_follow_the_references_ranges(gen):
    pos, vel, vspin = gen.last_draw["launch_pos"].cpu().numpy(), gen.last_draw["launch_vel"].cpu().numpy(), gen.last_draw["launch_vspin"].cpu().numpy()
    assert (pos >= [-4, 12, 1]).all() and (pos <= [4, 13, 1.5]).all()
    speed = np.linalg.norm(vel, axis=1)
    theta = np.degrees(np.arcsin(vel[:, 2] / speed))
    assert speed.min() >= 28 - 1e-4 and speed.max() <= 30 + 1e-4 and theta.min() >= 5 - 1e-3 and theta.max() <= 15 + 1e-3
    assert vspin.min() >= 5 and vspin.max() <= 10 and (vel[:, 1] < 0).all()
    # same seed, same pool
    again = ball_traj.TennisBallGenerator({"num_samples": 1000}, device=DEV, seed=11)
    assert torch.equal(again.traj_pool, gen.traj_pool)


@gpu
def test_no_valid_launch_is_an_error():
    with pytest.raises(RuntimeError, match="none of the"):
        ball_traj.TennisBallGenerator({"num_samples": 64, "theta_range": [-30, -20]}, device=DEV, seed=1)   # fired into the ground


@gpu
def test_pool_file_round_trip(gen, tmp_path):
    path = str(tmp_path / "ball_traj_in.npy")
    gen.save(path)
    data = np.load(path)
    n = len(gen.traj_pool)
    assert data.shape == (n, 307) and data.dtype == np.float32 and (np.diff(data[:, 0]) >= 0).all()   # [pos3 vel3 vspin1 traj300], sorted by launch x
    order = np.argsort(gen.launch_pos[:, 0].cpu().numpy())
    off = ball_traj.TennisBallGeneratorOffline(path, sample_random=True, device=DEV, seed=2)
    assert np.array_equal(off.traj_pool.cpu().numpy(), gen.traj_pool.cpu().numpy()[order]) and off.traj_pool.shape == (n, 100, 3) and off.traj_pool.is_cuda
    assert np.array_equal(off.launch_vel.cpu().numpy(), gen.launch_vel.cpu().numpy()[order]) and np.array_equal(off.launch_vspin.cpu().numpy(), gen.launch_vspin.cpu().numpy()[order])
    assert np.array_equal(data[:, 7:10], data[:, 0:3]), "frame 0 of a trajectory is its launch position"
    tr, lp, lv, ls = off.generate(16, need_init_state=True, start_pos=torch.zeros((16, 3), device=DEV) - 5.0)
    assert tr.shape == (16, 100, 3) and torch.equal(tr[:, 0], lp) and ls.shape == (16,)


def synthetic_pool(n):
    data = np.zeros((n, 307), np.float32)
    data[:, 0] = np.linspace(-4, 4, n)
    data[:, 7:] = np.arange(n, dtype=np.float32)[:, None]
    return data


def test_offline_round_robin_follows_the_reference():
    """:445-447: every env walks the pool on its own, modulo its length (CPU tensors: the torch path is device-agnostic)."""
    off = ball_traj.TennisBallGeneratorOffline(synthetic_pool(5), sample_random=False, num_envs=4)
    seen = []
    for env_ids in ([0, 1, 2, 3], [1, 3], [1], [0, 1, 2, 3], [1], [1], [1]):
        tr = off.generate(len(env_ids), env_ids=torch.tensor(env_ids))
        seen.append(tr[:, 0, 0].long().tolist())
    assert seen == [[0, 0, 0, 0], [1, 1], [2], [1, 3, 1, 2], [4], [0], [1]]
    assert off.sample_idx.tolist() == [2, 2, 2, 3]


def test_offline_random_sampling_follows_the_reference():
    """:436-443: uniform rows; a ball that starts on the other side (y > 0) gets the row at its x in the x-sorted pool, +- 1000 rows, clamped."""
    n = 20000
    off = ball_traj.TennisBallGeneratorOffline(synthetic_pool(n), sample_random=True, seed=5)
    start = torch.zeros((4000, 3))
    start[:, 0] = torch.linspace(-4.5, 4.5, 4000)
    start[:, 1] = torch.where(torch.arange(4000) % 2 == 0, 1.0, -1.0)
    idx = off.indices(4000, start_pos=start)
    other = start[:, 1] > 0
    centre = ((start[:, 0] + 4) / 8 * n).long()
    assert idx.min() >= 0 and idx.max() <= n - 1
    lo, hi = torch.clamp(centre - 1000, 0, n - 1), torch.clamp(centre + 999, 0, n - 1)
    assert ((idx >= lo) & (idx <= hi))[other].all()
    assert (idx[other] == 0).any() and (idx[other] == n - 1).any(), "the clamp at both ends of the pool is reached"
    spread = (idx[~other] - centre[~other]).abs().float()
    assert (spread > 1000).float().mean() > 0.5, "this-side balls get rows from anywhere"
    assert len(off.generate(3)) == 3 and off.indices(50).max() < n


@gpu
def test_task_draws_its_balls_from_the_pool(gen, tmp_path):
    """cfg_v2p.ball_traj_file: reset_balls(env_ids) writes the drawn launch like `_reset_balls` (:503-524), clears the flags, returns the
    trajectories - and 30 steps later the task's ball is where the pooled trajectory says, both within the oracle bound of the oracle's
    own trajectory of that launch.  The task simulates the generator's ball (material, spin scale, substeps and solver set to it)."""
    from tests.gpu_util import N, T, synth_tables
    from vid2player3d_amd.motion_lib import MotionLib
    from vid2player3d_amd.tasks import HumanoidSMPLIMRacketBall, default_cfg

    path = str(tmp_path / "pool.npy")
    gen.save(path)
    n, steps = 4, 30
    cfg = default_cfg(n, motion_lib=MotionLib(synth_tables(seed=5, num_clips=8, min_frames=60, max_frames=120), DEV), sample_first_motions=True,
                      body_shape_mismatch="ignore", ball_body_contacts=False, contact_solver="tgs")
    cfg["sim"].update({"substeps": 6})
    cfg["sim"]["physx"]["num_position_iterations"] = 2
    cfg["v2p"] = {"ball_traj_file": path, "restitution": 1.4, "ball_friction": 0.2, "spin_scale": 5}
    task = HumanoidSMPLIMRacketBall(cfg, device_type="cuda", device_id=0)
    sim = ball_traj.ball_sim_cfg_of(task)
    assert sim == pytest.approx(gen.sim, rel=1e-12), "the task simulates the ball the pool was made with"
    task.reset_with_times(None, T(np.full(n, 0.2)))
    task._humanoid_root_states[:, 0:2] += 50.0
    task._reset_env_tensors(None)
    task._has_bounce[:] = True
    task._has_racket_ball_contact[:] = True
    task._bounce_pos[:] = 1.0
    before = N(task._ball_root_states).copy()
    ids = [1, 3]
    traj = task.reset_balls(ids)
    assert traj.shape == (2, 100, 3) and traj.is_cuda
    after = N(task._ball_root_states)
    assert np.array_equal(after[[0, 2]], before[[0, 2]]) and N(task._has_bounce).tolist() == [True, False, True, False]
    assert N(task._has_racket_ball_contact).tolist() == [True, False, True, False] and (N(task._bounce_pos)[ids] == 0).all() and (N(task._bounce_pos)[[0, 2]] == 1).all()
    pool = np.load(path)
    rows = [int(np.nonzero((pool[:, 7:] == r.reshape(-1)).all(axis=1))[0][0]) for r in N(traj)]
    assert np.array_equal(after[ids, 0:3], pool[rows, 0:3]) and np.array_equal(after[ids, 7:10], pool[rows, 3:6])
    want = N(ball_traj.launch_ang_vel(T(pool[rows, 3:6]), T(pool[rows, 6])))
    assert np.array_equal(after[ids, 10:13], want) and np.array_equal(after[ids, 3:7], [[0, 0, 0, 1]] * 2)
    # the other entry stays what it was: a launch state given by the caller, nothing returned
    assert task.reset_balls([0], T(before[:1, 0:3]), T(before[:1, 7:10]), T(before[:1, 10:13])) is None
    # ---- 30 steps
    frames = []
    act = torch.zeros((n, 75), device=DEV)
    for _ in range(steps):
        frames.append(N(task._ball_root_states)[ids, 0:3].copy())
        act[:, :69] = task._dof_pos
        task.pre_physics_step(act.clone())
        task._physics_step()
    frames.append(N(task._ball_root_states)[ids, 0:3].copy())
    got = np.stack(frames, axis=1)   # [2, 31, 3]: the ball at the start of control step t
    e = 0  # (one launch goes through the oracle: it takes seconds per trajectory)
    state = B.launch_state(pool[rows[e], 0:3].astype(np.float64), pool[rows[e], 3:6].astype(np.float64), float(pool[rows[e], 6]))
    calls, sens = B.rollouts(sim, state[None], steps)
    cfi = sim["control_freq_inv"]
    B.compare_with_oracle("generator", sim, got[e:e + 1], calls, sens, cfi, "task ball, 30 steps")
    B.compare_with_oracle("generator", sim, N(traj)[e:e + 1, :steps + 1], calls, sens, cfi, "pooled trajectory")
    print("[ball] task ball vs pooled trajectory over %d steps: largest difference %.2e m" % (steps, np.abs(got - N(traj)[:, :steps + 1]).max()))
    assert calls[0, :, 2].min() < 0.1, "the 30 steps include the bounce"
    task.close()
