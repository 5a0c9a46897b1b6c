"""What the low-level policy of a control step costs on the GPU (vid2player3d_amd/policies.py), at 8192 envs with one network and at
15360 envs with two (units 1024, 1024, 512 as the shipped configs have them):

    by_hand     today's composition from the public pieces: `ImitationTarget.compute_observations()` (nine slice copies and
                v2p_obs_imitation), torch's clamp and normalise, the actor, torch's clamp, `target.actions`; with two networks also the
                two gathers (rows 0::2, 1::2) and the interleaving cat of models/im_network_builder_dual.py:37-45
    policy      `LowLevelPolicy.step()`: v2p_ll_policy_input -> the dense layers per side on contiguous halves -> v2p_ll_policy_actions
    gemms       the dense layers alone, on the policy's own buffers
    launch      a one-env launch of v2p_ll_policy_actions, back to back: what a launch costs here

Both forms compute the same actions; that is checked once per size before anything is timed.  Every timing is taken with device events
around `--iters` repetitions after `--warmup` repetitions, three rounds each, alternating the candidates; one JSON line per figure and
a summary line at the end.
    python tools/ll_policy_bench.py [--iters 200] [--warmup 20]
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, HERE)

from mvae_bench import DEV, timed  # noqa: E402

from tests import policies_fixture as PF  # noqa: E402
from vid2player3d_amd import policies as P  # noqa: E402

UNITS = (1024, 1024, 512)
CLIP_OBS, CLIP_ACTIONS = 5.0, 1.0


def make(n, sides):
    ctl, task, player, target = (PF.two_player_controller if sides == 2 else PF.single_controller)(n)
    actors = PF.random_actors(sides, 734, 75, units=UNITS, seed=31)
    norms = PF.random_norms(sides, 734, ("running", "running"), seed=41)
    pol = P.LowLevelPolicy(target, actors if sides == 2 else actors[0], norms if sides == 2 else norms[0], CLIP_OBS, CLIP_ACTIONS)
    rng = np.random.default_rng(1)
    for _ in range(3):  # a few control steps: velocities in the state, a target in front of it
        ctl.pre_physics_step(torch.as_tensor(rng.normal(0, 0.5, (n, ctl.get_action_size())).astype(np.float32), device=DEV))
        ctl.physics_step(torch.zeros((n, 75), device=DEV))
        ctl.post_physics_step()
    ctl.pre_physics_step(torch.as_tensor(rng.normal(0, 0.5, (n, ctl.get_action_size())).astype(np.float32), device=DEV))
    stats = [(torch.from_numpy(nm.mean).to(DEV), torch.from_numpy(nm.spread).to(DEV)) for nm in norms]

    @torch.no_grad()
    def by_hand():
        obs = torch.clamp(target.compute_observations(), -CLIP_OBS, CLIP_OBS)
        mus = []
        for s, (actor, (mean, std)) in enumerate(zip(pol.actors, stats)):
            x = obs if sides == 1 else obs[s::2]
            mus.append(actor(torch.clamp((x - mean) / (std + 1e-8), -5.0, 5.0)))
        mu = mus[0] if sides == 1 else torch.cat([mus[0].unsqueeze(1), mus[1].unsqueeze(1)], dim=1).reshape(-1, 75)
        return target.actions(torch.clamp(mu, -CLIP_ACTIONS, CLIP_ACTIONS))

    @torch.no_grad()
    def gemms():
        for actor, (x, mu) in zip(pol.actors, pol._halves):
            actor(x, out=mu)

    return pol, by_hand, gemms


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--sizes", default="8192:1,15360:2", help="envs:networks, comma-separated")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise RuntimeError("ll_policy_bench measures on a GPU; there is none here")
    figures, tags = {}, []
    for size in args.sizes.split(","):
        n, sides = (int(v) for v in size.split(":"))
        pol, by_hand, gemms = make(n, sides)
        a, b = by_hand().clone(), pol.step().clone()
        torch.cuda.synchronize()
        # (the dense layers run on other row blocks in the two forms: the actions agree to the GEMMs' rounding, the raw observation to the bit)
        print(json.dumps({"check": "policy against the composition by hand", "envs": n, "networks": sides, "actions_max_abs_diff": float((a - b).abs().max()),
                          "actions_max_abs": float(b.abs().max())}), flush=True)
        tag = "%d_%d" % (n, sides)
        tags.append(tag)
        figures["by_hand_ms_" + tag], figures["policy_ms_" + tag], figures["gemms_ms_" + tag] = by_hand, pol.step, gemms
        if "launch_ms" not in figures:
            tg = pol.target
            row = tg.task._target_bufs[tg.task._cur]
            tensors, one_in, one_out = tg._tensors(row), torch.zeros((1, 75), device=DEV), torch.zeros((1, 75), device=DEV)
            figures["launch_ms"] = lambda tg=tg, tensors=tensors, one_in=one_in, one_out=one_out: P.launch_ll_policy_actions(tg.settings, tensors, 1, 1, 1.0, one_in, one_out,
                                                                                                                             len(tg._joint_pos_bind))
    out = {k: [] for k in figures}
    for r in range(args.rounds):
        for k, fn in figures.items():
            ms = timed(fn, args.iters, args.warmup)
            out[k].append(ms)
            print(json.dumps({"figure": k, "round": r, "ms_per_step": round(ms, 5), "iters": args.iters}), flush=True)
    med = {k: float(np.median(v)) for k, v in out.items()}
    summary = {"summary": "low-level policy of a control step, units %s, clip_obs %g, clip_actions %g" % (list(UNITS), CLIP_OBS, CLIP_ACTIONS),
               **{k: round(v, 5) for k, v in med.items()}, "spread": {k: [round(min(v), 5), round(max(v), 5)] for k, v in out.items()}}
    for tag in tags:
        summary["policy_over_by_hand_" + tag] = round(med["policy_ms_" + tag] / med["by_hand_ms_" + tag], 4)
        summary["policy_minus_gemms_ms_" + tag] = round(med["policy_ms_" + tag] - med["gemms_ms_" + tag], 5)
        summary["by_hand_minus_gemms_ms_" + tag] = round(med["by_hand_ms_" + tag] - med["gemms_ms_" + tag], 5)
        summary["policy_minus_gemms_in_launches_" + tag] = round((med["policy_ms_" + tag] - med["gemms_ms_" + tag]) / med["launch_ms"], 2)
    summary["device"] = torch.cuda.get_device_name(0)
    print(json.dumps(summary), flush=True)


if __name__ == "__main__":
    main()
