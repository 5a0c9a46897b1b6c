"""What the two-player motion-generator tests share: the two seeded weight sets, the fixture tests/golden/mvae_dual.npz (recorded from the
reference's own `reset_dual` and `step` under `dual_mode: different` by tools/gen_golden_mvae_dual.py) and its variants.  The seeded
weights, the tolerance rule (ORDER_ALLOWANCE x the recorded float32 - float64 scatter, integers exact) and `assert_state` are
tests/mvae_fixture.py's.

12 envs (env 2k: side 0, env 2k+1: side 1) x 6 steps.  A variant's keys: `<v>/init_ready`, `<v>/init_serve` [2,288] (the first frame of
each side), `<v>/reaction_ids`, `<v>/recovery_ids` and `<v>/root_xy` [12,2] of the reset of all envs, `<v>/reset/<state>` after it,
`<v>/preset_swing`, `<v>/latents`, `<v>/residual`, `<v>/traj/<state>` [7,...] (what a step reads), `<v>/post/<state>` [6,...] (what it
writes besides); a second reset, of ids PART_IDS only, from the state after the last step: `<v>/part/root_xy` [4,2], `<v>/part/<state>`
[4,...] (the rows of those ids afterwards).  `joint_pos_bind_rel` [12,24,3] differs row by row: which row a reset reads is part of
what is recorded.
"""
import os

import numpy as np

from tests import mvae_fixture as FX

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "mvae_dual.npz")
WEIGHT_SEEDS = (FX.WEIGHT_SEED, 20393)  # (the second: picked among 20312 .. 20399 for root-position std far from the first set's, 0.5 .. 1.1 in 1/std - the reproduced quirk then stands far above every allowance)
N, T = 12, 6
# variant: players, righthand, grip (side 0, side 1), is_train, residuals, serve_from
VARIANTS = {
    "A": dict(player=("nadal", "federer"), righthand=(False, True), grip=("semi_western", "eastern"), is_train=True, residual=True, serve_from="far"),
    "B": dict(player=("federer", "djokovic"), righthand=(True, True), grip=("eastern", "semi_western"), is_train=False, residual=True, serve_from="near"),
    "C": dict(player=("nadal", "federer"), righthand=(False, True), grip=("semi_western", "eastern"), is_train=True, residual=False, serve_from="near"),
}
PART_REACTION, PART_RECOVERY = (3, 8), (2, 9)
PART_IDS = (2, 3, 8, 9)
STATE = FX.FLOAT_STATE + FX.INT_STATE
RESET_STATE = STATE + ("racket_pos", "racket_normal")

_cache = {}


def golden():
    if "g" not in _cache:
        with np.load(GOLDEN) as z:
            _cache["g"] = {k: z[k] for k in z.files}
    return _cache["g"]


def weights():
    """((weights of side 0, of side 1), (avg, avg), (std, std)), built once."""
    if "w" not in _cache:
        from vid2player3d_amd import mvae

        sets = [FX.seeded_state_dict(seed) for seed in WEIGHT_SEEDS]
        _cache["w"] = (tuple(mvae.weights_from_state_dict(sd) for sd, _, _ in sets), tuple(a for _, a, _ in sets), tuple(s for _, _, s in sets))
    return _cache["w"]


def cfg(v):
    """the cfg_v2p keys of variant v"""
    s = VARIANTS[v]
    return {"dual_mode": "different", "player": list(s["player"]), "righthand": list(s["righthand"]), "grip": list(s["grip"]), "serve_from": s["serve_from"],
            "add_residual_dof": "euler"}


def settings(v):
    from vid2player3d_amd import mvae

    return mvae.player_settings(cfg(v), VARIANTS[v]["is_train"], N)


def residual(g, v, t):
    return g[v + "/residual"][t] if VARIANTS[v]["residual"] else None


def state_before(g, v, t):
    return {k: g["%s/traj/%s" % (v, k)][t] for k in ("conditions", "root_pos", "swing_type", "swing_type_cycle")}


def state_after(g, v, t):
    o = {k: g["%s/traj/%s" % (v, k)][t + 1] for k in ("conditions", "root_pos", "swing_type", "swing_type_cycle")}
    o.update({k: g["%s/post/%s" % (v, k)][t] for k in ("root_vel", "joint_rot6d", "joint_rotmat", "phase_pred")})
    if ("%s/post/joint_rot" % v) in g:
        o["joint_rot"] = g["%s/post/joint_rot" % v][t]
    return o


def reset_state(g, v):
    return {k: g["%s/reset/%s" % (v, k)] for k in RESET_STATE}


def state_before_part(g, v):
    """the whole state before the second reset: the state after the last step; racket and (when training) joint_rot still the first reset's"""
    s = dict(reset_state(g, v))
    s.update(state_after(g, v, T - 1))
    return s


def init_rows(g, v):
    """(`_init_data_ready`, `_init_data_serve`) [12,288]: the two sides' first frames interleaved by parity"""
    return tuple(np.tile(g["%s/init_%s" % (v, k)], (N // 2, 1)) for k in ("ready", "serve"))


def reset_inputs(g, v, reaction, recovery):
    """(ids ascending, their init features) of a `reset_dual(reaction, recovery)`"""
    from vid2player3d_amd import mvae

    ids, from_ready = mvae.dual_reset_rows(reaction, recovery)
    ready, serve = init_rows(g, v)
    return ids, np.where(from_ready[:, None], ready[ids], serve[ids])
