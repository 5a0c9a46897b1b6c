"""What the single-player controller's per-step task reset and the action part of its pre_physics_step cost on the GPU
(vid2player3d_amd/tasks/tennis_controller.py).  rl_games calls env.reset(done_ids) after every step, so `ctl.reset([])` runs every
control step:

    reset torch     cfg v2p task_reset 'torch' (the default): the reference's `_reset_envs` on device tensors - three nonzero() host
                    reads, then indexed torch launches for the envs the flags name
    reset device    task_reset 'device': v2p_tennis_task_reset, one launch, no host read
    actions torch   the torch lines of pre_physics_step (:247-266) without the random walk: three clones and three products
    actions walk    the same with the reference's random_walk_in_recovery lines (:252-257): a host read sizes the slice
    actions kernel  v2p_controller_actions with the random walk, one launch

8192 envs, L = 10, a pool of 10,000 rows.  Before every reset both candidates get the same forced flags: of every `share` envs one
reacts and one recovers - one in 40 (a rally) and every env.  Each figure is the median of three alternating rounds of `--iters` steps,
as device-event time per step and as host wall time per step; the wall time ends with ONE synchronise per round, because what the torch
path costs is its host reads.  One JSON line per figure and a summary line at the end.
    python tools/tennis_reset_bench.py [--envs 8192] [--iters 200] [--warmup 30]
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from vid2player3d_amd import ball_traj  # noqa: E402
from vid2player3d_amd.motion_lib import MotionLib  # noqa: E402
from vid2player3d_amd.tasks import HumanoidSMPLIMRacketBall, default_cfg  # noqa: E402
from vid2player3d_amd.tasks import tennis_controller as tc  # noqa: E402

DEV = "cuda:0"
POOL_ROWS, POOL_FRAMES = 10000, 100


class MidGrid:  # a mid-sized out-estimator table: 12000 rows
    VEL_X_RANGE = (10, 40, 1.0)
    VEL_Y_RANGE = (-10, 10, 1.0)
    VSPIN_RANGE = (-10, 10, 1.0)
    TRAJ_X_RANGE = (0, 20, 0.5)
    TRAJ_Y_RANGE = (0, 3, 0.1)


def make_pool(rng):
    """rows [pos3 vel3 vspin1 traj300] sorted by launch x, launches in the generator's ranges"""
    pool = rng.normal(0, 3, (POOL_ROWS, 7 + 3 * POOL_FRAMES)).astype(np.float32)
    pool[:, 0] = np.sort(rng.uniform(-4, 4, POOL_ROWS))
    pool[:, 1], pool[:, 2] = rng.uniform(12, 13, POOL_ROWS), rng.uniform(1, 1.5, POOL_ROWS)
    pool[:, 3:6] = np.stack([rng.uniform(-3, 3, POOL_ROWS), rng.uniform(-29, -26, POOL_ROWS), rng.uniform(2, 7, POOL_ROWS)], -1)
    pool[:, 6] = rng.uniform(5, 10, POOL_ROWS)
    return pool


def timed(fn, iters, warmup):
    """(device-event ms per step, host wall ms per step with one synchronise at the end)"""
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0 = time.perf_counter()
    a.record()
    for _ in range(iters):
        fn()
    b.record()
    torch.cuda.synchronize()
    wall = (time.perf_counter() - t0) * 1e3 / iters
    return a.elapsed_time(b) / iters, wall


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--envs", type=int, default=8192)
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=30)
    ap.add_argument("--rounds", type=int, default=3)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise RuntimeError("tennis_reset_bench measures on a GPU; there is none here")
    from tests.gpu_util import synth_tables

    n = args.envs
    rng = np.random.default_rng(1)
    grids = tc.grids_of(MidGrid)
    rows = int(np.prod([ball_traj.grid_cells(g) for g in grids[:3]]))
    tx = rng.uniform(-1.5, 2.5, (rows, ball_traj.grid_cells(grids[3]))).astype(np.float32)
    ty = np.stack([rng.uniform(0, 25, (rows, ball_traj.grid_cells(grids[4]))), rng.uniform(0, 2, (rows, ball_traj.grid_cells(grids[4])))], -1).astype(np.float32)
    gen = ball_traj.TennisBallGeneratorOffline(make_pool(rng), sample_random=True, device=DEV, seed=3)
    cfg = default_cfg(n, motion_lib=MotionLib(synth_tables(seed=5, num_clips=16, min_frames=60, max_frames=200), DEV), sample_first_motions=True,
                      body_shape_mismatch="ignore", contact_solver="tgs")
    cfg["sim"].update({"substeps": 6})
    cfg["sim"]["physx"]["num_position_iterations"] = 2
    v2p = {"ball_generator": gen, "restitution": 1.4, "ball_friction": 0.2, "spin_scale": 5, "reward_type": "return_w_estimate", "reward_weights": {"pos": 0.5, "ball_pos": 0.5},
           "court_min": [-30.0, -30.0], "court_max": [30.0, 30.0], "obs_ball_traj_length": 10, "reset_reaction_nframes": 30, "ball_traj_out_x_file": tx,
           "ball_traj_out_y_file": ty, "use_random_ball_target": True}
    cfg["v2p"] = v2p
    task = HumanoidSMPLIMRacketBall(cfg, device_type="cuda", device_id=0)
    env = {"episodeLength": 300, "enableEarlyTermination": False}
    ctl = {mode: tc.TennisControllerTask(task, {"env": env, "v2p": dict(v2p, task_reset=mode)}, params=MidGrid, seed=11) for mode in ("torch", "device")}
    task.reset()
    for c in ctl.values():
        c.reset()
    act = torch.zeros((n, 75), device=DEV)
    for _ in range(5):  # a few steps of flight, so that the state is one of a rollout
        task.step(act.clone())
    torch.cuda.synchronize()

    figures = {}
    for share in (40, 1):
        rx = torch.as_tensor(np.arange(n) % share == 0, device=DEV)
        rc = torch.as_tensor(np.arange(n) % share == (share // 2 if share > 1 else 0), device=DEV)

        def reset_of(c, rx=rx, rc=rc):
            def fn():
                c._reset_reaction_buf.copy_(rx)
                c._reset_recovery_buf.copy_(rc)
                c.reset([])
            return fn

        for mode in ("torch", "device"):
            figures["reset_%s_1_in_%d" % (mode, share)] = reset_of(ctl[mode])

    # ---- the action part: 32 latent + 3 residual-DoF columns, a third of the envs in recovery
    st = tc.action_settings(num_res_dof=3, num_res_root=0, vae_action_scale=1.5, residual_dof_scale=0.4, random_walk=True, seed=11)
    actions = torch.as_tensor(rng.normal(0, 0.5, (n, 35)).astype(np.float32), device=DEV)
    tar_action = torch.as_tensor((np.arange(n) % 3 != 0).astype(np.int64), device=DEV)
    out = tc.action_outputs(st, n, dtype=torch.float32, device=DEV)
    random_buf = torch.zeros((n, 32), device=DEV)
    calls = [0]

    def actions_kernel():
        tc.launch_actions(st, n, actions, tar_action, out, call=calls[0])
        calls[0] += 1

    def actions_torch(walk):
        def fn():
            _actions = actions.clone()  # noqa: F841
            mvae_actions = actions[:, :32].clone() * 1.5
            if walk:  # physics_mvae_controller.py:252-257
                in_recovery = tar_action == 0
                num_in_recovery = in_recovery.sum()
                random_buf[:num_in_recovery].normal_(0, 1)
                random_buf[:num_in_recovery] = torch.clamp(random_buf[:num_in_recovery], -5, 5)
                mvae_actions[in_recovery] = random_buf[:num_in_recovery]
            res = actions[:, 32:35].clone() * 0.4  # noqa: F841
        return fn

    figures.update(actions_torch=actions_torch(False), actions_torch_walk=actions_torch(True), actions_kernel=actions_kernel)
    res = {k: [] for k in figures}
    for r in range(args.rounds):
        for k, fn in figures.items():
            dev_ms, wall_ms = timed(fn, args.iters, args.warmup)
            res[k].append((dev_ms, wall_ms))
            print(json.dumps({"figure": k, "round": r, "device_ms_per_step": round(dev_ms, 5), "wall_ms_per_step": round(wall_ms, 5), "envs": n, "iters": args.iters}), flush=True)
    med = {k: [float(np.median([x[i] for x in v])) for i in (0, 1)] for k, v in res.items()}
    print(json.dumps({"summary": "single-player task reset and action step, %d envs, L = 10, pool of %d rows; [device ms, wall ms] per step, medians of %d rounds"
                      % (n, POOL_ROWS, args.rounds), **{k: [round(x, 5) for x in v] for k, v in med.items()},
                      "spread_device_ms": {k: [round(min(x[0] for x in v), 5), round(max(x[0] for x in v), 5)] for k, v in res.items()},
                      "device": torch.cuda.get_device_name(0)}), flush=True)
    task.close()


if __name__ == "__main__":
    main()
