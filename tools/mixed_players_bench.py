"""Throughput of a two-player racket + ball batch (cfg_v2p dual_mode `different`, nadal_federer.yaml) against two single-player batches
of half the size stepped one after the other (the `--groups 2` style workaround).  Whole epochs are timed the way bench.py times them:
per-epoch reset (a ball served at every player from 8 m) + stand-in actions from the context window, step_fused, TGS, joint limits.
Usage: python tools/mixed_players_bench.py [--num-envs 8192] [--epochs 10] [--warmup 2]   (prints one line per configuration)"""
import argparse
import json
import os
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import bench  # noqa: E402
from vid2player3d_amd.tasks import HumanoidSMPLIMRacketBall, default_cfg  # noqa: E402


def make(n, players, substeps, iterations, seed=7):
    cfg = default_cfg(n, synthetic_motions={"seed": 7, "num_clips": 64, "min_frames": 90, "max_frames": 300, "speed": 2.0}, contact_solver="tgs", substep_jobs=True)
    cfg["env"]["terminationHeadHeight"] = -0.5
    cfg["sim"]["substeps"] = substeps
    cfg["sim"]["physx"] = dict(cfg["sim"]["physx"], num_position_iterations=iterations)
    if len(players) == 2:
        cfg["v2p"] = {"dual_mode": "different", "player": list(players)}
    else:
        cfg["env"]["player"] = players[0]
    torch.manual_seed(seed)
    task = HumanoidSMPLIMRacketBall(cfg, device_type="cuda", device_id=0)
    inner = task.reset

    def reset_with_serve(env_ids=None):  # bench.py --racket-ball's serve
        inner(env_ids)
        dev = task.device
        root = task._humanoid_root_states[:, 0:3]
        g = torch.Generator(device=dev)
        g.manual_seed(seed)
        jitter = torch.rand((n, 3), device=dev, generator=g)
        task.reset_balls(torch.arange(n, device=dev), root + torch.tensor([8.0, 0.0, 0.3], device=dev) + jitter,
                         torch.tensor([-22.0, 0.0, 4.0], device=dev) + (jitter - 0.5) * torch.tensor([6.0, 3.0, 3.0], device=dev),
                         torch.tensor([0.0, -150.0, 0.0], device=dev).expand(n, 3))

    task.reset = reset_with_serve
    gen = torch.Generator(device=task.device)
    gen.manual_seed(seed)
    noise = torch.stack([0.17 * torch.randn((n, 75), device=task.device, generator=gen) for _ in range(bench.HORIZON)])
    return task, noise, torch.empty_like(noise)


def epochs(batches, count):
    for _ in range(count):
        for task, noise, acts in batches:
            task.reset()
            bench.make_epoch_actions(task, noise, acts)
        for i in range(bench.HORIZON):
            for task, _, acts in batches:  # (several batches: one after the other, step by step, on one stream)
                task.step_fused(acts[i])


def measure(name, batches, args):
    epochs(batches, args.warmup)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    epochs(batches, args.epochs)
    torch.cuda.synchronize()
    el = time.perf_counter() - t0
    for task, _, _ in batches:
        task.check()
    envs = sum(t.num_envs for t, _, _ in batches)
    out = {"config": name, "envs": envs, "epochs": args.epochs, "env_steps_per_s": envs * bench.HORIZON * args.epochs / el,
           "ms_per_step": 1e3 * el / (bench.HORIZON * args.epochs)}
    print(json.dumps(out), flush=True)
    for task, _, _ in batches:
        task.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--num-envs", type=int, default=8192)
    ap.add_argument("--epochs", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    args = ap.parse_args()
    n = args.num_envs
    for substeps, iterations in ((2, 4), (6, 2)):
        tag = "%d substeps x %d iterations" % (substeps, iterations)
        measure("nadal_federer mixed, %d envs, %s" % (n, tag), [make(n, ["nadal", "federer"], substeps, iterations)], args)
        measure("nadal + federer, two %d-env batches one after the other, %s" % (n // 2, tag),
                [make(n // 2, ["nadal"], substeps, iterations), make(n // 2, ["federer"], substeps, iterations, seed=8)], args)
        measure("federer alone, %d envs, %s" % (n, tag), [make(n, ["federer"], substeps, iterations)], args)


if __name__ == "__main__":
    main()
