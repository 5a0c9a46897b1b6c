"""Writes the three files of vid2player's tennis task that the reference makes offline with Isaac Gym - the pool of incoming launches
(cfg_v2p.ball_traj_file), the outgoing tables of TennisBallOutEstimator, the incoming table of TennisBallInEstimator - with this
engine's own ball (vid2player3d_amd/ball_traj.py, v2p_ball_rollout), and prints launches per second.

    python tools/ball_tables.py OUT_DIR                  # the reference's sizes: 10000 draws, 8.25 M + 675 k launches
    python tools/ball_tables.py OUT_DIR --time-only      # a pool of 10000 draws and ONE 1 M-launch chunk of the outgoing grid, nothing written
"""
import argparse
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from vid2player3d_amd import ball_traj  # noqa: E402


def timed(fn, repeat=1):
    torch.cuda.synchronize()
    best = None
    for _ in range(repeat):
        t = time.perf_counter()
        out = fn()
        torch.cuda.synchronize()
        dt = time.perf_counter() - t
        best = dt if best is None else min(best, dt)
    return out, best


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("out_dir")
    ap.add_argument("--device", default="cuda:0")
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--pool-draws", type=int, default=10000)
    ap.add_argument("--chunk", type=int, default=1 << 20)
    ap.add_argument("--time-only", action="store_true")
    a = ap.parse_args()
    dev = a.device
    cfg = ball_traj.ball_sim_cfg()
    gen = ball_traj.TennisBallGenerator({"num_samples": a.pool_draws}, device=dev, seed=a.seed)  # (the first launch also loads the code object)
    d = gen.last_draw
    _, t = timed(lambda: ball_traj.rollout(cfg, d["launch_pos"], d["launch_vel"], d["launch_vspin"], num_frames=gen.traj_length), repeat=3)
    sub = gen.traj_length * cfg["control_freq_inv"] * cfg["substeps"]
    print("pool: %d of %d draws valid; kernel + output allocation %.3f ms = %.2f M launches/s (%.1f G ball-substeps/s), %d frames x %d calls x %d substeps"
          % (len(gen.traj_pool), a.pool_draws, t * 1e3, a.pool_draws / t / 1e6, a.pool_draws * sub / t / 1e9, gen.traj_length, cfg["control_freq_inv"], cfg["substeps"]), flush=True)
    P = ball_traj.traj_out_params
    n = a.chunk
    pos = torch.zeros((n, 3), device=dev)
    pos[:, 2] = 100.0
    vs = torch.tensor(np.arange(*P.VSPIN_RANGE), dtype=torch.float32, device=dev)
    vz = torch.tensor(np.arange(*P.VEL_Y_RANGE), dtype=torch.float32, device=dev)
    vy = torch.tensor(np.arange(*P.VEL_X_RANGE), dtype=torch.float32, device=dev)
    idx = torch.arange(n, device=dev)
    vel = torch.zeros_like(pos)
    vel[:, 1], vel[:, 2] = vy[idx // (len(vz) * len(vs))], vz[(idx // len(vs)) % len(vz)]
    grids = (P.TRAJ_X_RANGE, P.TRAJ_Y_RANGE)
    cfg0 = dict(cfg, enable_ground=0)
    _, t = timed(lambda: ball_traj.rollout(cfg0, pos, vel, vs[idx % len(vs)], num_frames=60, want=(), resample=grids), repeat=3)
    sub = 61 * cfg["control_freq_inv"] * cfg["substeps"]
    print("outgoing grid, one chunk of %d launches (61 frames, resampled online onto %d + %d cells): %.1f ms = %.2f M launches/s (%.1f G ball-substeps/s)"
          % (n, ball_traj.grid_cells(grids[0]), ball_traj.grid_cells(grids[1]), t * 1e3, n / t / 1e6, n * sub / t / 1e9), flush=True)
    if a.time_only:
        return
    os.makedirs(a.out_dir, exist_ok=True)
    gen.save(os.path.join(a.out_dir, "ball_traj_in.npy"))
    t0 = time.perf_counter()
    tx, ty = ball_traj.build_out_tables(P, cfg, chunk=a.chunk, device=dev, progress=lambda k, tot: print("  outgoing %d / %d" % (k, tot), flush=True))
    np.save(os.path.join(a.out_dir, "ball_traj_out_x.npy"), tx)
    np.save(os.path.join(a.out_dir, "ball_traj_out_y.npy"), ty)
    print("outgoing tables: %d launches in %.1f s (with the copies to the host)" % (len(tx), time.perf_counter() - t0), flush=True)
    t0 = time.perf_counter()
    tab = ball_traj.build_in_table(ball_traj.traj_in_params, cfg, device=dev)
    np.save(os.path.join(a.out_dir, "ball_traj_in_dual.npy"), tab)
    print("incoming table: %d launches in %.1f s" % (len(tab), time.perf_counter() - t0), flush=True)


if __name__ == "__main__":
    main()
