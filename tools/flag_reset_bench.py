"""What the reset of done envs costs in a rollout step of the controller's PPO agent, by id list (`reset_mode = 'ids'`: one host read,
`dones.nonzero()`, indexed torch writes and three id-list launches) against by flags (`reset_mode = 'flags'`: `reset_by_flags()`, one
fixed sequence of six launches and no host read), on one GPU on the racket + ball controller with generator, target and low-level policy
attached, at the sizes of tools/ctl_ppo_bench.py: 10240 envs, horizon 64, units 1024 / 1024 / 512.  Both modes run in the same process
on controllers built alike; the 'ids' path is the default and the baseline.  Neither mode is given a start table: 'ids' draws the
start of a reset player with torch, 'flags' in its kernel.

  (a) the reset alone, per rollout step: `reset_buf` is loaded with a fixed pattern (one device copy, in both modes) and the mode's
      reset runs - 'ids': `_reset_lists` + `ctl.reset(done_ids)` as `play_steps` calls them; 'flags': `ctl.reset_by_flags()` - at about
      1 % of envs done and at none done.  Device events around `--iters` repetitions and the wall clock around the same loop, closed by
      a synchronisation.
  (b) `T_play`: `play_steps` of a whole horizon in both modes, wall clock and device events; episodes of 100 steps with the envs'
      clocks staggered, so that about 1 % of the envs are done at every step.

`--rounds` rounds alternate the modes; one JSON line per figure and a summary line (medians, min - max) at the end.
    python tools/flag_reset_bench.py [--envs 10240] [--horizon 64] [--iters 50] [--warmup 5] [--rounds 3] [--share 0.01]
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, HERE)

from tests import ctl_ppo_fixture as FX  # noqa: E402
from tests import flag_reset_fixture as FF  # noqa: E402
from tests import policies_fixture as PF  # noqa: E402
from vid2player3d_amd import ctl_ppo as CP  # noqa: E402
from vid2player3d_amd import policies as P  # noqa: E402

DEV = FF.DEV
UNITS = (1024, 1024, 512)
MODES = ("ids", "flags")


def make(n, horizon, mode, episode_length):
    ctl, task, player, target, _ = FF.controller(n, episode_length=episode_length)
    ctl._reset_root_xy = None  # (each mode draws the start its own way)
    ctl.attach_low_level_policy(P.LowLevelPolicy(target, PF.random_actors(1, 734, 75, units=UNITS, seed=31)[0], PF.random_norms(1, 734, seed=41)[0], 5.0, 1.0))
    ctl.progress_buf.copy_(torch.arange(n, device=DEV) % episode_length)
    minibatch = n * horizon if (n * horizon) % 16384 else 16384
    return CP.ControllerPPOAgent.from_config(ctl, FX.YAML_PARAMS["federer_train_stage_1"], horizon_length=horizon, minibatch_size=minibatch, reset_mode=mode)


def reset_form(agent, pattern):
    """one rollout step's reset of the envs of `pattern` ([N] int64), as play_steps runs it in the agent's mode"""
    ctl = agent.ctl
    dones = pattern.float()

    def ids():
        ctl.reset_buf.copy_(pattern)
        done_ids, _ = agent._reset_lists(dones)
        agent._env_reset(done_ids)

    def flags():
        ctl.reset_buf.copy_(pattern)
        ctl.reset_by_flags()

    return ids if agent.reset_mode == "ids" else flags


def timed(fn, iters, warmup):
    """(device ms, wall ms) per call"""
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
    return a.elapsed_time(b) / iters, (time.perf_counter() - t0) * 1e3 / iters


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--envs", type=int, default=10240)
    ap.add_argument("--horizon", type=int, default=64)
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--share", type=float, default=0.01, help="share of envs done per step")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise RuntimeError("flag_reset_bench measures on a GPU; there is none here")
    n, episode = args.envs, max(2, int(round(1.0 / args.share)))
    agents = {m: make(n, args.horizon, m, episode) for m in MODES}
    out = {}

    def note(k, v, **kw):
        out.setdefault(k, []).append(v)
        print(json.dumps(dict({"figure": k, "value": round(v, 5)}, **kw)), flush=True)

    # (b) whole rollouts first (they warm up code objects and GEMM algorithms, and leave the controllers in a played state)
    for m in MODES:
        agents[m].play_steps()
    torch.cuda.synchronize()
    for r in range(args.rounds):
        for m in MODES:
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            a.record()
            agents[m].play_steps()
            b.record()
            torch.cuda.synchronize()
            note("T_play_s_" + m, time.perf_counter() - t0, round=r)
            note("T_play_device_s_" + m, a.elapsed_time(b) * 1e-3, round=r)
            note("episodes_per_step_" + m, float(agents[m].acc[0]) / args.horizon, round=r)
    # (a) the reset alone
    rng = np.random.default_rng(1)
    some = np.zeros(n, np.int64)
    some[rng.choice(n, max(1, int(round(args.share * n))), replace=False)] = 1
    patterns = {"some_done": torch.as_tensor(some, device=DEV), "none_done": torch.zeros(n, dtype=torch.int64, device=DEV)}
    for r in range(args.rounds):
        for tag, pattern in patterns.items():
            for m in MODES:
                dev_ms, wall_ms = timed(reset_form(agents[m], pattern), args.iters, args.warmup)
                note("reset_%s_device_ms_%s" % (tag, m), dev_ms, round=r, iters=args.iters)
                note("reset_%s_wall_ms_%s" % (tag, m), wall_ms, round=r, iters=args.iters)
    med = {k: float(np.median(v)) for k, v in out.items()}
    ratio = lambda k: round(med[k + "flags"] / med[k + "ids"], 4)
    summary = {"summary": "reset of done envs by ids against by flags, %d envs, horizon %d, %d done of %d in 'some_done', units %s" % (n, args.horizon, int(some.sum()), n, list(UNITS)),
               **{k: round(v, 5) for k, v in med.items()}, "spread": {k: [round(min(v), 5), round(max(v), 5)] for k, v in out.items()},
               "T_play_flags_over_ids": ratio("T_play_s_"), "reset_some_done_wall_flags_over_ids": ratio("reset_some_done_wall_ms_"),
               "reset_none_done_wall_flags_over_ids": ratio("reset_none_done_wall_ms_"), "device": torch.cuda.get_device_name(0)}
    print(json.dumps(summary), flush=True)


if __name__ == "__main__":
    main()
