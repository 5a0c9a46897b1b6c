"""What one control step of the two-player MotionVAE motion generator costs on the GPU (vid2player3d_amd/mvae.py, `dual_mode: different`):

    dual_parity MotionVAEPlayer.step of a two-player batch: one launch of v2p_mvae_dual_step, workgroup b serving side b & 1
    dual_halves the same launch with the other mapping of workgroups to sides (the grid's first half side 0, its second half side 1)
    single      v2p_mvae_step at the same number of envs (one weight set), in this tree
    torch       the reference's form in torch on device tensors: two half-batch passes over strided halves (`latents[::2]`,
                `condition_flat[::2]`), each with per-env blended weights, two state updates written back through strided env ids, the
                root columns of every env's condition rewritten by each, and the `.item()` of mvae_player.py:279 (tools/mvae_bench.py's
                transcription of one side, used twice)

at 8192 and at 1024 envs; federer / djokovic, training mode, with residuals.  Device events around `--iters` repetitions after `--warmup`,
three rounds, alternating the candidates; one JSON line per figure and a summary line with dual / single and halves / parity at the end.
    python tools/mvae_dual_bench.py [--envs 8192] [--iters 100] [--warmup 10]
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from mvae_bench import DEV, TorchPlayer, timed  # noqa: E402
from vid2player3d_amd import mvae  # noqa: E402

STATE = ("conditions", "root_pos", "root_vel", "joint_rot6d", "joint_rotmat", "phase_pred", "swing_type", "swing_type_cycle")


class TorchDualPlayer:
    """`MVAEPlayer.step` under `_is_dual` (mvae_player.py:191-199) on device tensors: the yardstick.  State is its own."""

    def __init__(self, st, w, avg, std, player):
        self.sides = []
        for i in (0, 1):
            view = type("Half", (), {"device": player.device, "num_envs": player.num_envs // 2})()
            for k in STATE + ("joint_rot",):
                setattr(view, "_" + k, getattr(player, "_" + k)[i::2].contiguous())
            self.sides.append(TorchPlayer(st["sides"][i], w[i], avg[i], std[i], view))
        for k in STATE:
            setattr(self, k, getattr(player, "_" + k).clone())
        self.righthand = [s["righthand"] for s in st["sides"]]

    def step(self, latents, residual):
        # (the reference runs both decoder passes before either state update; here a side's pass and update are one call, so the
        # conditions both passes read are kept aside: one copy of [n,288] more than the reference makes)
        before = self.conditions.clone()
        for i, side in enumerate(self.sides):
            env_ids = torch.arange(i, len(latents), 2, device=latents.device)
            side.conditions = before[i::2]  # (strided halves, as `latents[::2]` / `condition_flat[::2]`)
            for k in ("root_pos", "swing_type", "swing_type_cycle"):
                setattr(side, k, getattr(self, k)[i::2])
            _ = self.righthand[env_ids[0].item() % 2]  # (:279, a host read per side)
            side.step(latents[i::2], residual[i::2])
            for k in STATE:
                getattr(self, k)[env_ids] = getattr(side, k)
            self.conditions[:, -1, 0:3] = (self.root_pos - side.avg[0:3]) / side.std[0:3]  # (:262 writes every env)


def make(n, w, avg, std, rng):
    cfg = {"dual_mode": "different", "player": ["federer", "djokovic"], "righthand": [True, True], "grip": ["eastern", "semi_western"], "add_residual_dof": "euler"}
    frames = [[(avg[i] + std[i] * rng.normal(0, 0.8, (1, mvae.FRAME))).astype(np.float32) for i in (0, 1)] for _ in (0, 1)]
    bind = rng.uniform(-0.3, 0.3, (24, 3)).astype(np.float32)
    dual = mvae.MotionVAEPlayer(cfg, n, w, avg, std, None, bind, True, DEV, init_data_ready=frames[0], init_data_serve=frames[1])
    dual.dual_mapping = mvae.DUAL_MAP_PARITY
    ids = torch.arange(n, device=DEV)
    dual.reset_dual(ids[(ids // 2) % 2 == 0], ids[(ids // 2) % 2 == 1])
    swing = torch.as_tensor(rng.integers(-1, 4, n))
    dual._swing_type.copy_(swing)
    dual._swing_type_cycle.copy_(swing)
    halves = mvae.MotionVAEPlayer(cfg, n, w, avg, std, None, bind, True, DEV, init_data_ready=frames[0], init_data_serve=frames[1])
    halves.dual_mapping = mvae.DUAL_MAP_HALVES
    single = mvae.MotionVAEPlayer({"player": "federer", "righthand": True, "add_residual_dof": "euler"}, n, w[0], avg[0], std[0], frames[0][0], bind, True, DEV)
    for k in mvae.STATE_NAMES:
        getattr(halves, "_" + k).copy_(getattr(dual, "_" + k))
        getattr(single, "_" + k).copy_(getattr(dual, "_" + k))
    ref = TorchDualPlayer(dual.settings, w, avg, std, dual)
    z = torch.as_tensor(np.clip(rng.normal(0, 1, (n, mvae.LATENT)), -3, 3).astype(np.float32), device=DEV)
    res = torch.as_tensor(rng.uniform(-2, 2, (n, 3)).astype(np.float32), device=DEV)
    return dual, halves, single, ref, z, res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--envs", type=int, default=8192)
    ap.add_argument("--small", type=int, default=1024)
    ap.add_argument("--iters", type=int, default=100)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=3)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise RuntimeError("mvae_dual_bench measures on a GPU; there is none here")
    from tests import mvae_dual_fixture as DX

    w, avg, std = DX.weights()
    rng = np.random.default_rng(1)
    figures = {}
    for n in (args.envs, args.small):
        dual, halves, single, ref, z, res = make(n, w, avg, std, rng)
        # the forms compute the same step: checked once, before anything is timed
        for p in (dual, halves, ref):
            p.step(z, res)
        torch.cuda.synchronize()
        print(json.dumps({"check": "one step: the two mappings bit for bit, the kernel against the torch transcription", "envs": n,
                          "mappings_equal": all(bool(torch.equal(getattr(dual, "_" + k), getattr(halves, "_" + k))) for k in ("conditions", "joint_rotmat", "swing_type")),
                          "conditions_max_abs_diff": float((dual._conditions - ref.conditions).abs().max()),
                          "swing_types_equal": bool((dual._swing_type == ref.swing_type).all())}), flush=True)
        figures["dual_parity_ms_%d" % n] = (lambda p=dual, z=z, r=res: p.step(z, r))
        figures["dual_halves_ms_%d" % n] = (lambda p=halves, z=z, r=res: p.step(z, r))
        figures["single_ms_%d" % n] = (lambda p=single, z=z, r=res: p.step(z, r))
        figures["torch_ms_%d" % n] = (lambda p=ref, z=z, r=res: p.step(z, r))
    out = {k: [] for k in figures}
    for r in range(args.rounds):
        for k, fn in figures.items():
            ms = timed(fn, args.iters, args.warmup)
            out[k].append(ms)
            print(json.dumps({"figure": k, "round": r, "ms_per_step": round(ms, 5), "iters": args.iters}), flush=True)
    med = {k: float(np.median(v)) for k, v in out.items()}
    summary = {"summary": "two-player MotionVAE generator step, federer / djokovic, training mode, with residuals", **{k: round(v, 5) for k, v in med.items()},
               "spread": {k: [round(min(v), 5), round(max(v), 5)] for k, v in out.items()}, "device": torch.cuda.get_device_name(0)}
    for n in (args.envs, args.small):
        best = min(med["dual_parity_ms_%d" % n], med["dual_halves_ms_%d" % n])
        summary["parity_over_single_%d" % n] = round(med["dual_parity_ms_%d" % n] / med["single_ms_%d" % n], 3)
        summary["halves_over_single_%d" % n] = round(med["dual_halves_ms_%d" % n] / med["single_ms_%d" % n], 3)
        summary["halves_over_parity_%d" % n] = round(med["dual_halves_ms_%d" % n] / med["dual_parity_ms_%d" % n], 3)
        summary["torch_over_dual_%d" % n] = round(med["torch_ms_%d" % n] / best, 2)
    print(json.dumps(summary), flush=True)


if __name__ == "__main__":
    main()
