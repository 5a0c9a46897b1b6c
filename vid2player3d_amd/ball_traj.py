"""Free tennis balls on the device: the pool of incoming launches and the estimator tables of vid2player's tennis task.

The reference makes three files offline by stepping 10000 ball actors alone in Isaac Gym, and ships none of them (`data` is ignored):

    cfg_v2p.ball_traj_file        valid incoming launches + their 100-frame trajectories (vid2player/utils/tennis_ball.py:221-394, read
                                  by TennisBallGeneratorOffline, :422-456; env/tasks/humanoid_smpl_im_mvae.py:121-130, 503-524)
    ball_traj_out_x / _y          outgoing flights resampled on a distance grid and a drop grid (utils/tennis_ball_out_estimator.py:21-121,
                                  208-258), read by TennisBallOutEstimator (:124-205; physics_mvae_controller.py:74-77, 300)
    ball_traj_in_dual             incoming 50-frame flights by launch height / speed / spin (utils/tennis_ball_in_estimator.py:82-140),
                                  read by TennisBallInEstimator (:16-79; humanoid_smpl_im_mvae_dual.py:24, 68)

Here the balls are simulated by `v2p_ball_rollout` (csrc/ball_rollout.hip): THIS engine's ball - the one a racket + ball batch steps -
one ball per lane, a whole trajectory per launch, so the files describe the ball the task really simulates.  There is no CPU path for
the simulation (a missing library or a CPU tensor is an error); the estimators' `estimate()` is plain torch and runs on whatever device
their tables are on.  `resample_reference` is a numpy statement of the resampling the kernel does online - the checker of the tests,
as in body_shapes.py.
"""
import ctypes as C
import math

import numpy as np
import torch

from . import _lib, racket

NET_HEIGHT = 1.07  # utils/tennis_ball.py:20
BALL_R = racket.BALL["radius"]


class traj_out_params:  # utils/tennis_ball_out_estimator.py:13-18
    VEL_X_RANGE = (10, 65, 0.1)
    VEL_Y_RANGE = (-5, 10, 0.1)
    VSPIN_RANGE = (-10, 10, 0.2)
    TRAJ_X_RANGE = (0, 30, 0.5)
    TRAJ_Y_RANGE = (0, 3, 0.1)


class traj_in_params:  # utils/tennis_ball_in_estimator.py:10-14
    VEL_X_RANGE = (25, 30, 0.1)
    VEL_Y_RANGE = (5, 8, 0.1)
    VSPIN_RANGE = (5, 10, 0.1)
    HEIGHT_RANGE = (0.5, 2, 0.1)


# ------------------------------------------------------------------------------------------------------------------ settings
def ball_sim_cfg(substeps=6, spin_scale=5, **overrides):
    """The settings of `TennisBallGeneratorIsaac` (utils/tennis_ball.py:44-81, 221-271) as the fields of v2p_ball_sim.

    Material: the ball shape's restitution 0.9 / friction 0.2 (:268-269) against the plane's 0.5 / 1.0 (create_sim's plane), combined by
    averaging (PhysX's default): 0.7 / 0.6.  The shape's `compliance = 0.5` (:270) is NOT modelled: the engine's contact rows are rigid.
    Solver: TGS, `num_position_iterations` 4 at 2 substeps, else 2 (:61-62); dt 1/60, control_freq_inv 2 (`simulate`, :114).
    `bounce_height`: 6 R above 2 substeps, else 4 R (:181-184)."""
    cfg = dict(radius=BALL_R, mass=racket.BALL["mass"], inertia=racket.BALL["inertia"], restitution_ground=0.5 * (0.9 + 0.5), friction_ground=0.5 * (0.2 + 1.0),
               bounce_threshold_velocity=0.2, angular_damping=racket.BALL_MATERIAL["ang_damp"], max_angular_velocity=racket.BALL_MATERIAL["max_ang_vel"],
               spin_scale=float(spin_scale), sim_dt=1.0 / 60.0, substeps=int(substeps), control_freq_inv=2, num_iterations=4 if substeps == 2 else 2, solver_type=1,
               gravity_z=-9.81, contact_offset=0.02, erp=0.2, max_depenetration_velocity=10.0, enable_ground=1, net_height=NET_HEIGHT,
               bounce_height=BALL_R * (6 if substeps > 2 else 4))
    unknown = set(overrides) - set(cfg)
    if unknown:
        raise ValueError("ball_sim_cfg: unknown settings %s" % sorted(unknown))
    cfg.update(overrides)
    return cfg


def ball_sim_cfg_of(task):
    """The settings of a racket + ball task's OWN ball (HumanoidSMPLIMRacketBall: its v2p_ball_cfg and sim block), so that a pool or a
    table can be made for the ball that task simulates (humanoid_smpl_im_mvae.py:414-416, 436-438 material; :731-737 bounce height)."""
    sp, mat = task.sim_params, task.ball_material
    env = task.cfg["env"]
    return ball_sim_cfg(substeps=sp.substeps, spin_scale=task.cfg_v2p.get("spin_scale", 1.0), restitution_ground=mat["rest_ground"], friction_ground=mat["fric_ground"],
                        bounce_threshold_velocity=sp.physx.bounce_threshold_velocity, angular_damping=mat["ang_damp"], max_angular_velocity=mat["max_ang_vel"],
                        sim_dt=sp.dt, control_freq_inv=task.control_freq_inv, num_iterations=int(sp.physx.num_position_iterations),
                        solver_type={"pgs": 0, "tgs": 1}[task.contact_solver], gravity_z=sp.gravity[2], contact_offset=float(sp.physx.contact_offset),
                        erp=env.get("contact_erp", 0.2), max_depenetration_velocity=float(sp.physx.max_depenetration_velocity),
                        enable_ground=int(env.get("enable_contact", True)), bounce_height=BALL_R * (6 if sp.substeps > 2 else 4))


def grid_cells(g):
    """Cells of a (lo, hi, step) grid as the reference counts them: int((hi - lo) / step) (tennis_ball_out_estimator.py:95-96)."""
    return int((g[1] - g[0]) / g[2])


def grid_values(g):
    """float32 value of every cell: lo + k step, evaluated in float64 (what the kernel computes)."""
    return (float(g[0]) + np.arange(grid_cells(g), dtype=np.float64) * float(g[2])).astype(np.float32)


def sim_struct(cfg, num_frames, resample=None):
    """v2p_ball_sim of a settings dict; resample = (grid_x, grid_y), each (lo, hi, step)."""
    c = _lib.BallSim(num_frames=int(num_frames), resample=0 if resample is None else 1, **cfg)
    if resample is not None:
        c.grid_x[:] = [float(x) for x in resample[0]]
        c.grid_y[:] = [float(x) for x in resample[1]]
    return c


def launch_ang_vel(launch_vel, launch_vspin):
    """vspin x 2 pi x normalize(launch_vel x (0, 0, -1)) (utils/tennis_ball.py:135-136, humanoid_smpl_im_mvae.py:508-509)."""
    g = torch.tensor([0.0, 0.0, -1.0], dtype=launch_vel.dtype, device=launch_vel.device).expand_as(launch_vel)
    return launch_vspin.view(-1, 1) * math.pi * 2 * torch.nn.functional.normalize(torch.cross(launch_vel, g, dim=1), dim=1)


def rollout(cfg, launch_pos, launch_vel, launch_vspin, num_frames=100, want=("traj", "bounce_pos", "bounce_idx", "pass_net", "peak_after_bounce"), resample=None):
    """`simulate` (utils/tennis_ball.py:113-218) - or, with resample = (grid_x, grid_y), `simulate_without_bounce`
    (tennis_ball_out_estimator.py:21-121) - of n balls in ONE kernel launch.  launch_* are float32 tensors on a GPU; returns the wanted
    outputs of v2p_ball_rollout_out (resample: traj_x, traj_y too) as device tensors."""
    lib = _lib.load()
    if not launch_pos.is_cuda:
        raise RuntimeError("ball_traj.rollout: the balls are simulated by the HIP kernel only - launch tensors must be on a GPU (no CPU fallback)")
    dev = launch_pos.device
    lp, lv, ls = (t.to(device=dev, dtype=torch.float32).contiguous() for t in (launch_pos, launch_vel, launch_vspin))
    n = lp.shape[0]
    assert lp.shape == (n, 3) and lv.shape == (n, 3) and ls.shape == (n,), (lp.shape, lv.shape, ls.shape)
    c = sim_struct(cfg, num_frames, resample)
    shapes = {"traj": ((n, num_frames, 3), torch.float32), "bounce_pos": ((n, 3), torch.float32), "bounce_idx": ((n,), torch.int64), "pass_net": ((n,), torch.uint8),
              "peak_after_bounce": ((n,), torch.float32), "final_state": ((n, 13), torch.float32)}
    want = [w for w in want if not (resample is not None and w in ("traj", "peak_after_bounce"))]
    if resample is not None:
        shapes["traj_x"], shapes["traj_y"] = ((n, grid_cells(resample[0])), torch.float32), ((n, grid_cells(resample[1]), 2), torch.float32)
        want = list(want) + ["traj_x", "traj_y"]
    out = {w: torch.empty(shapes[w][0], dtype=shapes[w][1], device=dev) for w in want}
    o = _lib.BallRolloutOut(**{w: t.data_ptr() for w, t in out.items()})
    with torch.cuda.device(dev):
        _lib.check(lib.v2p_ball_rollout(C.byref(c), n, _lib.ptr(lp), _lib.ptr(lv), _lib.ptr(ls), C.byref(o), _lib.current_stream(dev)), "v2p_ball_rollout")
    if "pass_net" in out:
        out["pass_net"] = out["pass_net"].bool()
    return out


# ------------------------------------------------------------------------------------------------------------------ the checker
def resample_reference(samples, grid_x, grid_y, sim_dt=1.0 / 60.0):
    """`simulate_without_bounce`'s resampling (tennis_ball_out_estimator.py:93-119) of stored positions, in numpy float32: samples
    [N,S,3] = the position at the start of every simulate() call; returns (traj_x [N,nx], traj_y [N,ny,2]).  Kept as the reference has
    it: the pointer t only moves forward and is shared by the cells of a grid, a cell is the linear interpolation between samples t-1
    and t, t stops at the last sample (the end clamp), and t = 0 pairs sample 0 with sample -1, the LAST one (the wrap).  Heights are
    relative to each ball's own launch height (the reference subtracts ball 0's: the same number there); time is t x sim_dt (the
    reference divides by control_freq_inv x 30, the same at its 60 Hz)."""
    s = np.asarray(samples, dtype=np.float32)
    n, S = s.shape[0], s.shape[1]
    Y, Z = s[:, :, 1], s[:, :, 2] - s[:, :1, 2]
    gx, gy = grid_values(grid_x), grid_values(grid_y)
    ids = np.arange(n)
    traj_x, traj_y = np.zeros((n, len(gx)), np.float32), np.zeros((n, len(gy), 2), np.float32)
    one, dt = np.float32(1.0), np.float32(sim_dt)
    with np.errstate(divide="ignore", invalid="ignore"):
        t = np.zeros(n, dtype=np.int64)
        for k, x in enumerate(gx):
            while True:
                adv = (t < S - 1) & (Y[ids, t] < x)
                if not adv.any():
                    break
                t[adv] += 1
            w = (x - Y[ids, t - 1]) / (Y[ids, t] - Y[ids, t - 1])
            traj_x[:, k] = Z[ids, t - 1] * (one - w) + Z[ids, t] * w
        t = np.zeros(n, dtype=np.int64)
        for k, y in enumerate(gy):
            while True:
                adv = (t < S - 1) & (-Z[ids, t] < y)
                if not adv.any():
                    break
                t[adv] += 1
            w = (-y - Z[ids, t - 1]) / (Z[ids, t] - Z[ids, t - 1])
            traj_y[:, k, 0] = Y[ids, t - 1] * (one - w) + Y[ids, t] * w
            traj_y[:, k, 1] = ((t - 1).astype(np.float32) * (one - w) + t.astype(np.float32) * w) * dt
    return traj_x, traj_y


# ------------------------------------------------------------------------------------------------------------------ incoming pool
class TennisBallGenerator:
    """`TennisBallGeneratorIsaac` (utils/tennis_ball.py:221-356) on this engine: draws launches, simulates them in one kernel launch,
    keeps the valid ones.  cfg: the reference's keys (ball_traj_length, origin_min / max, bounce_min / max, vel_range, vspin_range,
    theta_range, :277-284) + `num_samples` (the reference's num_env: 10000 in training, 1000 else, :245) and `sim` (a settings dict,
    default ball_sim_cfg()).  Pool and launches stay on the device."""

    def __init__(self, cfg=None, device="cuda:0", seed=None, is_train=True, need_reset=True):
        cfg = dict(cfg or {})
        self.device = torch.device(device)
        self.sim = dict(cfg.get("sim") or ball_sim_cfg())
        self.num_env = int(cfg.get("num_samples", 10000 if is_train else 1000))
        self.traj_length = int(cfg.get("ball_traj_length", 100))
        f = lambda k, d: torch.tensor(cfg.get(k, d), dtype=torch.float32, device=self.device)
        self.origin_min, self.origin_max = f("origin_min", [-4, 12, 1]), f("origin_max", [4, 13, 1.5])
        self.bounce_min, self.bounce_max = f("bounce_min", [-3, -10, 0]), f("bounce_max", [3, -7, 0])
        self.vel_range, self.vspin_range, self.theta_range = f("vel_range", [28, 30]), f("vspin_range", [5, 10]), f("theta_range", [5, 15])
        self._gen = torch.Generator(device=self.device)
        if seed is not None:
            self._gen.manual_seed(int(seed))
        self.traj_pool = None
        if need_reset:
            self.reset()

    def _sample_range(self, size, lo, hi):  # torch_sample_range (:40-41)
        return torch.rand(size, generator=self._gen, device=self.device) * (hi - lo) + lo

    def draw_launches(self, n):
        """:292-306, same ranges, same order of the draws."""
        origin = self._sample_range((n, 3), self.origin_min, self.origin_max)
        bounce = self._sample_range((n, 3), self.bounce_min, self.bounce_max)
        d = torch.nn.functional.normalize(bounce[:, :2] - origin[:, :2], dim=1)
        speed = self._sample_range((n,), self.vel_range[0], self.vel_range[1])
        theta = self._sample_range((n,), self.theta_range[0], self.theta_range[1])
        vspin = self._sample_range((n,), self.vspin_range[0], self.vspin_range[1])
        vel = torch.stack([speed * torch.cos(theta / 180 * np.pi) * d[:, 0], speed * torch.cos(theta / 180 * np.pi) * d[:, 1], speed * torch.sin(theta / 180 * np.pi)]).T.contiguous()
        return origin, vel, vspin

    def valid_mask(self, res):
        """The filter of :319-327 on the device: passes the net, bounced at all, first bounce inside the box on the other side, and
        rises above 1 m from the bounce frame on (`peak_after_bounce`: the reference's host loop over balls, :326-327)."""
        bp = res["bounce_pos"]
        return (res["pass_net"].bool() & (bp.sum() != 0) & (bp[:, 0] > self.bounce_min[0]) & (bp[:, 0] < self.bounce_max[0])
                & (bp[:, 1] > self.bounce_min[1]) & (bp[:, 1] < self.bounce_max[1]) & (res["peak_after_bounce"] > 1.0))

    def reset(self):
        """:289-335."""
        pos, vel, vspin = self.draw_launches(self.num_env)
        res = rollout(self.sim, pos, vel, vspin, num_frames=self.traj_length)
        valid = self.valid_mask(res)
        self.last_draw = dict(res, launch_pos=pos, launch_vel=vel, launch_vspin=vspin, valid=valid)  # (what reset() looked at: tests, tools)
        if int(valid.sum()) == 0:
            raise RuntimeError("TennisBallGenerator.reset: none of the %d launches is a valid trajectory" % self.num_env)
        self.traj_pool, self.launch_pos, self.launch_vel, self.launch_vspin = res["traj"][valid], pos[valid], vel[valid], vspin[valid]
        return int(valid.sum())

    def _indices(self, n):
        return torch.randint(0, len(self.traj_pool), (n,), generator=self._gen, device=self.device)

    def generate(self, n_traj, need_init_state=False, start_pos=None, env_ids=None):
        """:337-346 (start_pos / env_ids: accepted and unused, so that the object can stand in for the offline generator)."""
        idx = self._indices(n_traj)
        if need_init_state:
            return self.traj_pool[idx].clone(), self.launch_pos[idx], self.launch_vel[idx], self.launch_vspin[idx]
        return self.traj_pool[idx].clone()

    def generate_init_state(self, n_ball):
        """:348-353."""
        idx = self._indices(n_ball)
        return self.launch_pos[idx], self.launch_vel[idx], self.launch_vspin[idx]

    def generate_all(self):
        """:355-356."""
        return self.traj_pool, self.launch_pos, self.launch_vel, self.launch_vspin

    def rows(self):
        """The pool in the reference's row format [pos3 vel3 vspin1 traj(3 x frames)], sorted by launch x (:378, 389-394)."""
        data = torch.cat([self.launch_pos, self.launch_vel, self.launch_vspin.view(-1, 1), self.traj_pool.reshape(len(self.traj_pool), -1)], dim=1).cpu().numpy()
        return data[np.argsort(data[:, 0])]

    def save(self, path):
        np.save(path, self.rows())


class TennisBallGeneratorOffline:
    """`TennisBallGeneratorOffline` (utils/tennis_ball.py:422-456): a pool file of rows [pos3 vel3 vspin1 traj300]; pool and indices stay
    on the device."""

    def __init__(self, traj_file, sample_random=False, num_envs=None, device="cpu", seed=None):
        data = torch.from_numpy(np.load(traj_file) if isinstance(traj_file, str) else np.asarray(traj_file)).to(device=device, dtype=torch.float32)
        self.device = data.device
        self.data = data  # [rows, 7 + 3 frames]: what the controller's device reset reads rows of
        self.launch_pos, self.launch_vel, self.launch_vspin = data[:, 0:3], data[:, 3:6], data[:, 6]
        self.traj_pool = data[:, 7:].reshape(len(data), -1, 3)
        self.sample_random = sample_random
        self._gen = torch.Generator(device=self.device)
        if seed is not None:
            self._gen.manual_seed(int(seed))
        if not self.sample_random:
            self.sample_idx = torch.zeros((num_envs,), dtype=torch.int64, device=self.device)

    def indices(self, n_traj, start_pos=None, env_ids=None):
        """:436-447: random rows - for balls that start on the other side (y > 0) the row whose launch x matches the ball's x (the pool is
        sorted by launch x over [-4, 4]) +- 1000 rows -, or every env's own round robin."""
        n_pool = len(self.traj_pool)
        if self.sample_random:
            idx = torch.randint(0, n_pool, (n_traj,), generator=self._gen, device=self.device)
            if start_pos is not None:
                start_pos = start_pos.to(self.device)
                other = start_pos[:, 1] > 0
                near = ((start_pos[:, 0] + 4) / 8 * n_pool).long() + torch.randint(-1000, 1000, (n_traj,), generator=self._gen, device=self.device)
                idx = torch.where(other, torch.clamp(near, 0, n_pool - 1), idx)
            return idx
        env_ids = torch.as_tensor(env_ids, device=self.device, dtype=torch.long)
        idx = self.sample_idx[env_ids].clone()
        self.sample_idx[env_ids] += 1
        self.sample_idx[env_ids] %= n_pool
        return idx

    def generate(self, n_traj, need_init_state=False, start_pos=None, env_ids=None):
        idx = self.indices(n_traj, start_pos, env_ids)
        if need_init_state:
            return self.traj_pool[idx].clone(), self.launch_pos[idx], self.launch_vel[idx], self.launch_vspin[idx]
        return self.traj_pool[idx].clone()


# ------------------------------------------------------------------------------------------------------------------ outgoing tables
def _arange(r):
    return np.arange(*r)


def build_out_tables(params=traj_out_params, cfg=None, chunk=1 << 20, device="cuda:0", num_frames=60, launch_height=100.0, progress=None):
    """`generate_outgoing_trajectory` (tennis_ball_out_estimator.py:208-258): every (horizontal speed, vertical speed, spin) of the
    grids, launched along +y from a height of 100 m without ground, resampled by the kernel; returns (traj_x [B,nx], traj_y [B,ny,2])
    as numpy, B in the reference's order (speed slowest, spin fastest).  The launches are enumerated and simulated `chunk` at a time:
    no trajectory is ever stored.  (The reference spreads its launches along x, "extremely slow if all start from the same pos" in
    PhysX; here every ball starts at x = 0 - the flight does not depend on it.)"""
    cfg = dict(cfg or ball_sim_cfg(), enable_ground=0)
    vy, vz, vs = (torch.tensor(_arange(r), dtype=torch.float32, device=device) for r in (params.VEL_X_RANGE, params.VEL_Y_RANGE, params.VSPIN_RANGE))
    total = len(vy) * len(vz) * len(vs)
    grids = (params.TRAJ_X_RANGE, params.TRAJ_Y_RANGE)
    tx, ty = np.zeros((total, grid_cells(grids[0])), np.float32), np.zeros((total, grid_cells(grids[1]), 2), np.float32)
    for b0 in range(0, total, chunk):
        idx = torch.arange(b0, min(b0 + chunk, total), device=device)
        pos = torch.zeros((len(idx), 3), dtype=torch.float32, device=device)
        pos[:, 2] = launch_height
        vel = torch.zeros_like(pos)
        vel[:, 1], vel[:, 2] = vy[idx // (len(vz) * len(vs))], vz[(idx // len(vs)) % len(vz)]
        res = rollout(cfg, pos, vel, vs[idx % len(vs)], num_frames=num_frames, want=(), resample=grids)
        tx[b0:b0 + len(idx)], ty[b0:b0 + len(idx)] = res["traj_x"].cpu().numpy(), res["traj_y"].cpu().numpy()
        if progress:
            progress(b0 + len(idx), total)
    return tx, ty


def _index_f32(v, r):
    """round((clamp(v, lo, hi - step) - lo) / step) as the reference evaluates it on float32 tensors."""
    return torch.round((torch.clamp(v, r[0], r[1] - r[2]) - r[0]) / r[2])


class TennisBallOutEstimator:
    """`TennisBallOutEstimator` (tennis_ball_out_estimator.py:124-205): bounce position, bounce time and peak height of a ball that has
    just left the racket, looked up in the outgoing tables.  Tables: file names or arrays; they live on `device`, and so do the indices
    (the reference indexes host tables with `.cpu()` indices).  `vel_x_overflow` counts what the reference prints ('velocity X
    overflow', :180)."""

    def __init__(self, ball_traj_out_x, ball_traj_out_y, device="cpu", params=traj_out_params):
        load = lambda t: torch.from_numpy(np.load(t) if isinstance(t, str) else np.asarray(t)).to(device)
        self._ball_traj_out_x, self._ball_traj_out_y = load(ball_traj_out_x), load(ball_traj_out_y)
        self.params = params
        self.vel_x_overflow = torch.zeros((), dtype=torch.int64, device=device)

    def get_ball_traj_out_index(self, vel_x, vel_y, vspin):
        """:132-148."""
        VX, VY, VS = self.params.VEL_X_RANGE, self.params.VEL_Y_RANGE, self.params.VSPIN_RANGE
        dim = ((VX[1] - VX[0]) / VX[2], (VY[1] - VY[0]) / VY[2], (VS[1] - VS[0]) / VS[2])
        index = _index_f32(vel_x, VX) * dim[1] * dim[2] + _index_f32(vel_y, VY) * dim[2] + _index_f32(vspin, VS)
        return index.long()

    def get_ball_traj_out_x_index(self, x):
        """:150-155."""
        return _index_f32(x, self.params.TRAJ_X_RANGE).long()

    def get_ball_traj_out_y_index(self, y):
        """:157-162."""
        return _index_f32(y, self.params.TRAJ_Y_RANGE).long()

    def estimate(self, ball_states_all):
        """:164-205.  ball_states_all [N,13] on the tables' device -> (has_valid_contact [N], bounce_pos [M,2], bounce_time [M],
        max_height [M]) for the M valid rows, or (has_valid_contact, None, None, None)."""
        VX, VY, TY = self.params.VEL_X_RANGE, self.params.VEL_Y_RANGE, self.params.TRAJ_Y_RANGE
        s = ball_states_all
        has_valid_contact = (s[:, 8] > VX[0]) & (s[:, 9] > VY[0]) & (s[:, 9] < VY[1]) & (s[:, 2] < TY[1])
        # inside when passing the net
        x_net = s[:, 0] + s[:, 7] * abs(s[:, 1] / s[:, 8])
        has_valid_contact &= ((x_net > -4) & (x_net < 4))
        num = int(has_valid_contact.sum())
        if num == 0:
            return has_valid_contact, None, None, None
        b = s[has_valid_contact]
        vel_x = b[:, 7:9].norm(dim=-1)
        self.vel_x_overflow += (vel_x >= VX[1]).sum()
        vel_y = b[:, 9]
        vspin = b[:, 10:13].norm(dim=1) / (math.pi * 2)
        traj_index = self.get_ball_traj_out_index(vel_x, vel_y, vspin)
        ball_traj_x, ball_traj_y = self._ball_traj_out_x[traj_index], self._ball_traj_out_y[traj_index]
        rows = torch.arange(num, device=s.device)
        # bounce position according to the launch height
        height_index = self.get_ball_traj_out_y_index(b[:, 2])
        bounce_pos = b[:, :2] + ball_traj_y[rows, height_index, :1] * b[:, 7:9] / vel_x.unsqueeze(-1)
        bounce_time = ball_traj_y[rows, height_index, 1]
        # bounce position 0 if the ball goes into the net
        net_dist = -b[:, 1] / b[:, 8] * vel_x
        net_index = self.get_ball_traj_out_x_index(net_dist)
        not_pass_net = ball_traj_x[rows, net_index] + b[:, 2] < NET_HEIGHT
        bounce_pos[not_pass_net, :] = 0
        bounce_time = bounce_time.clone()
        bounce_time[not_pass_net] = 0
        max_height = b[:, 2] + ball_traj_x.max(dim=1).values
        return has_valid_contact, bounce_pos.float(), bounce_time.float(), max_height.float()


# ------------------------------------------------------------------------------------------------------------------ incoming table
def build_in_table(params=traj_in_params, cfg=None, chunk=1 << 18, device="cuda:0", num_frames=50):
    """`generate_incoming_trajectory` (tennis_ball_in_estimator.py:82-140): every (height, horizontal speed, vertical speed, spin) of the
    grids launched along +y with the ground on; the table is traj[:, :, 1:] (distance, height) of the 50-frame flights, [B,50,2] numpy,
    B in the reference's order (height slowest, spin fastest).  (Launch x: 0, as in build_out_tables.)"""
    cfg = dict(cfg or ball_sim_cfg())
    hh, vy, vz, vs = (torch.tensor(_arange(r), dtype=torch.float32, device=device)
                      for r in (params.HEIGHT_RANGE, params.VEL_X_RANGE, params.VEL_Y_RANGE, params.VSPIN_RANGE))
    total = len(hh) * len(vy) * len(vz) * len(vs)
    table = np.zeros((total, num_frames, 2), np.float32)
    for b0 in range(0, total, chunk):
        idx = torch.arange(b0, min(b0 + chunk, total), device=device)
        pos = torch.zeros((len(idx), 3), dtype=torch.float32, device=device)
        pos[:, 2] = hh[idx // (len(vy) * len(vz) * len(vs))]
        vel = torch.zeros_like(pos)
        vel[:, 1], vel[:, 2] = vy[(idx // (len(vz) * len(vs))) % len(vy)], vz[(idx // len(vs)) % len(vz)]
        res = rollout(cfg, pos, vel, vs[idx % len(vs)], num_frames=num_frames, want=("traj",))
        table[b0:b0 + len(idx)] = res["traj"][:, :, 1:].cpu().numpy()
    return table


class TennisBallInEstimator:
    """`TennisBallInEstimator` (tennis_ball_in_estimator.py:16-79): the incoming flight that matches an outgoing ball state, mirrored to
    the other side of the court.  The table lives on `device`."""

    def __init__(self, ball_traj, device="cpu", params=traj_in_params):
        self._ball_traj = torch.from_numpy(np.load(ball_traj) if isinstance(ball_traj, str) else np.asarray(ball_traj)).to(device)
        self.params = params

    def get_ball_traj_index(self, height, vel_x, vel_y, vspin):
        """:22-46."""
        VX, VY, VS, HR = self.params.VEL_X_RANGE, self.params.VEL_Y_RANGE, self.params.VSPIN_RANGE, self.params.HEIGHT_RANGE
        dim = ((HR[1] - HR[0]) / HR[2], (VX[1] - VX[0]) / VX[2], (VY[1] - VY[0]) / VY[2], (VS[1] - VS[0]) / VS[2])
        ih, ix, iy, iv = _index_f32(height, HR), _index_f32(vel_x, VX), _index_f32(vel_y, VY), _index_f32(vspin, VS)
        index = ih * dim[1] * dim[2] * dim[3] + ix * dim[2] * dim[3] + iy * dim[3] + iv
        return index.long(), (ih * HR[2] + HR[0], ix * VX[2] + VX[0], iy * VY[2] + VY[0], iv * VS[2] + VS[0])

    def estimate(self, ball_states, adjust=False):
        """:48-79 -> (traj_trans [N,F,3], ball_states_in [N,13], ball_states_out [N,13])."""
        height = ball_states[:, 2]
        vel_x = ball_states[:, 7:9].norm(dim=-1)
        d = ball_states[:, 7:9] / vel_x.view(-1, 1)
        vel_y = ball_states[:, 9]
        vspin = ball_states[:, 10:13].norm(dim=1) / (math.pi * 2)
        traj_index, (height, vel_x, vel_y, vspin) = self.get_ball_traj_index(height, vel_x, vel_y, vspin)
        traj = self._ball_traj[traj_index].clone()
        traj_trans = torch.cat([traj[:, :, :1] * d.view(-1, 1, 2) + ball_states[:, :2].view(-1, 1, 2), traj[:, :, 1:]], dim=-1)
        traj_trans[:, :, :2] *= -1
        ball_states_in = ball_states.clone()
        ball_states_in[:, :2] *= -1
        ball_states_in[:, 2] = height
        ball_states_in[:, 7:9] = -vel_x.view(-1, 1) * d
        ball_states_in[:, 9] = vel_y
        ball_states_in[:, 10:13] = launch_ang_vel(ball_states_in[:, 7:10], vspin)
        ball_states_out = ball_states_in.clone()
        ball_states_out[:, :2] *= -1
        ball_states_out[:, 7:9] *= -1
        ball_states_out[:, 10:13] = launch_ang_vel(ball_states_out[:, 7:10], vspin)
        return traj_trans, ball_states_in, ball_states_out
