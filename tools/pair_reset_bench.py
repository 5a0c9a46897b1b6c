"""What the reset of finished pairs costs in a step of the two-player match loop, by id list (`MatchPlayer(reset_mode='ids')`: one host
read, `reset_buf.nonzero()`, the list checked on the host, gathers, indexed torch writes and two id-list launches) against by flags
(`reset_mode='flags'`: `reset_pairs_by_flags()`, one fixed sequence of seven launches and no host read), on one GPU on the two-player
controller (`dual_mode: different`) with generator, target, low-level policy (units 1024 / 1024 / 512) and a `ControllerPolicy`
attached, at 10240 envs.  Both modes run in the same process on controllers built alike; the 'ids' path is the code as it was and the
baseline.  Neither mode is given a table: 'ids' draws the start and the serve with torch, 'flags' in its kernels.

  (a) the reset alone, per step: `reset_buf` is loaded with one of `--rotate` fixed patterns in turn (one device copy, in both modes) -
      about 1 % of the pairs each, and none - and the mode's reset runs.  Device events around `--iters` repetitions and the wall clock
      around the same loop, closed by a synchronisation.
  (b) `MatchPlayer.play(steps)` per step, wall clock and device events: after every step `reset_buf` is SET to the next of the patterns
      (a device copy, in both modes: with seeded random networks the step's own law would finish another 2 % of the pairs per step,
      differently in the two modes' draws) - a rotating 1 % of the pairs, and a run with no pair done.

`--rounds` rounds alternate the modes; one JSON line per figure and a summary line (medians, min - max) at the end.
    python tools/pair_reset_bench.py [--envs 10240] [--steps 64] [--iters 50] [--warmup 5] [--rounds 3] [--share 0.01] [--rotate 8]
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

from tests import pair_reset_fixture as PX  # noqa: E402
from tests import policies_fixture as PF  # noqa: E402
from vid2player3d_amd import match  # noqa: E402
from vid2player3d_amd import policies as P  # noqa: E402

DEV = PX.DEV
UNITS = (1024, 1024, 512)
MODES = match.RESET_MODES


class SetFlags:
    """wraps `ctl.post_physics_step`: after the step's law, `reset_buf` becomes `patterns[k % len]` (k: the count of steps)"""

    def __init__(self, ctl):
        self.ctl, self.inner, self.patterns, self.k = ctl, ctl.post_physics_step, None, 0
        ctl.post_physics_step = self

    def __call__(self, *args, **kw):
        out = self.inner(*args, **kw)
        if self.patterns is not None:
            self.ctl.reset_buf.copy_(self.patterns[self.k % len(self.patterns)])
        self.k += 1
        return out


def make(n, mode):
    ctl, task, player, target = PF.two_player_controller(n)
    ctl.attach_low_level_policy(P.LowLevelPolicy(target, PF.random_actors(2, 734, 75, units=UNITS, seed=31), PF.random_norms(2, 734, seed=41), 5.0, 1.0))
    player.seed = ctl.seed = PX.SEED
    dim, act = int(ctl.obs_buf.shape[1]), ctl.get_action_size()
    pol = P.ControllerPolicy(ctl, PF.random_actors(2, dim, act, units=UNITS, seed=51), PF.random_norms(2, dim, ("mean_var", "mean_var"), seed=61), 5.0, 1.0)
    return match.MatchPlayer(ctl, pol, mode), SetFlags(ctl)


def reset_form(m, patterns):
    """one step's reset of the pairs of the patterns in turn, as `MatchPlayer` runs it in its mode"""
    ctl, k = m.ctl, [0]

    def fn():
        ctl.reset_buf.copy_(patterns[k[0] % len(patterns)])
        k[0] += 1
        m._reset_done()

    return fn


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
    ap.add_argument("--steps", type=int, default=64)
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--share", type=float, default=0.01, help="share of pairs finished per step")
    ap.add_argument("--rotate", type=int, default=8, help="number of patterns taken in turn")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise RuntimeError("pair_reset_bench measures on a GPU; there is none here")
    n = args.envs
    players = {m: make(n, m) for m in MODES}
    rng = np.random.default_rng(1)
    count = max(1, int(round(args.share * (n // 2))))
    some = []
    for _ in range(args.rotate):
        f = np.zeros(n // 2, np.int64)
        f[rng.choice(n // 2, count, replace=False)] = 1
        some.append(torch.as_tensor(np.repeat(f, 2), device=DEV))
    none = [torch.zeros(n, dtype=torch.int64, device=DEV)]
    out = {}

    def note(k, v, **kw):
        out.setdefault(k, []).append(v)
        print(json.dumps(dict({"figure": k, "value": round(v, 5)}, **kw)), flush=True)

    # (b) whole runs first (they warm up code objects and GEMM algorithms, and leave the controllers in a played state)
    for m in MODES:
        players[m][0].play(4)
    torch.cuda.synchronize()
    for r in range(args.rounds):
        for tag, patterns in (("some_done", some), ("none_done", none)):
            for m in MODES:
                player, hook = players[m]
                hook.patterns, hook.k = patterns, 0
                a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                a.record()
                pairs, _ = player.play(args.steps)
                b.record()
                torch.cuda.synchronize()
                note("run_%s_wall_ms_per_step_%s" % (tag, m), (time.perf_counter() - t0) * 1e3 / args.steps, round=r)
                note("run_%s_device_ms_per_step_%s" % (tag, m), a.elapsed_time(b) / args.steps, round=r)
                note("run_%s_pairs_per_step_%s" % (tag, m), float(pairs) / args.steps, round=r)
    # (a) the reset alone
    for m in MODES:
        players[m][1].patterns = None
    for r in range(args.rounds):
        for tag, patterns in (("some_done", some), ("none_done", none)):
            for m in MODES:
                dev_ms, wall_ms = timed(reset_form(players[m][0], patterns), args.iters, args.warmup)
                note("reset_%s_device_ms_%s" % (tag, m), dev_ms, round=r, iters=args.iters)
                note("reset_%s_wall_ms_%s" % (tag, m), wall_ms, round=r, iters=args.iters)
    med = {k: float(np.median(v)) for k, v in out.items()}
    ratio = lambda k: round(med[k + "flags"] / med[k + "ids"], 4)
    summary = {"summary": "reset of finished pairs by ids against by flags, %d envs, %d steps, %d of %d pairs in 'some_done', units %s" % (n, args.steps, count, n // 2, list(UNITS)),
               **{k: round(v, 5) for k, v in med.items()}, "spread": {k: [round(min(v), 5), round(max(v), 5)] for k, v in out.items()},
               "run_some_done_device_flags_over_ids": ratio("run_some_done_device_ms_per_step_"), "run_none_done_device_flags_over_ids": ratio("run_none_done_device_ms_per_step_"),
               "reset_some_done_device_flags_over_ids": ratio("reset_some_done_device_ms_"), "reset_none_done_device_flags_over_ids": ratio("reset_none_done_device_ms_"),
               "device": torch.cuda.get_device_name(0)}
    print(json.dumps(summary), flush=True)


if __name__ == "__main__":
    main()
