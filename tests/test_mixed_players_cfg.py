"""Two-player racket batches (cfg_v2p dual_mode `different`, vid2player/cfg/controller/nadal_federer.yaml, federer_djokovic.yaml) on the
CPU: the cfg surface and its refusals, the ctypes mirror of v2p_racket_geom, the setter's argument checks and the two folded players."""
import ctypes
import os
import subprocess
import tempfile

import numpy as np
import pytest

from vid2player3d_amd import _lib, racket
from vid2player3d_amd.model import load_baked_model
from vid2player3d_amd.tasks import default_cfg
from vid2player3d_amd.tasks.humanoid_racket_ball import HumanoidSMPLIMRacketBall, pair_players, racket_geom_struct

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NADAL_FEDERER = {"dual_mode": "different", "player": ["nadal", "federer"], "righthand": [False, True]}
FEDERER_DJOKOVIC = {"dual_mode": "different", "player": ["federer", "djokovic"], "righthand": [True, True]}


def test_the_match_configs_select_their_pairs():
    assert pair_players(NADAL_FEDERER, {"numEnvs": 8}) == ["nadal", "federer"]
    assert pair_players(FEDERER_DJOKOVIC, {"numEnvs": 8}) == ["federer", "djokovic"]
    # a righthand list without names: djokovic / nadal per entry, like the single-player path
    assert pair_players({"dual_mode": "different", "righthand": [False, True]}, {"numEnvs": 2}) == ["nadal", "djokovic"]
    assert pair_players({"dual_mode": "different", "righthand": [True, True]}, {"numEnvs": 2}) == ["djokovic", "djokovic"]


@pytest.mark.parametrize("v2p,env,what", [
    (NADAL_FEDERER, {"numEnvs": 7}, "even"),
    ({"dual_mode": "different", "player": ["nadal", "sampras"]}, {"numEnvs": 8}, "unknown player"),
    ({"dual_mode": "different", "player": ["nadal", "federer", "djokovic"]}, {"numEnvs": 8}, "2 entries"),
    ({"dual_mode": "different", "player": ["nadal"]}, {"numEnvs": 8}, "2 entries"),
    ({"dual_mode": "different", "righthand": [True, False, True]}, {"numEnvs": 8}, "2 entries"),
    ({"dual_mode": "different", "player": "nadal"}, {"numEnvs": 8}, "2 entries"),
    ({"dual_mode": "different"}, {"numEnvs": 8}, "needs"),
    ({"dual_mode": "different", "player": ["nadal", "federer"], "righthand": [True, True]}, {"numEnvs": 8}, "disagrees"),
    (NADAL_FEDERER, {"numEnvs": 8, "player": "djokovic"}, "ONE player"),
])
def test_pair_refusals(v2p, env, what):
    with pytest.raises(ValueError, match=what):
        pair_players(v2p, env)


def _cfg(n, v2p, **env):
    cfg = default_cfg(n, **env)
    cfg["v2p"] = v2p
    return cfg


@pytest.mark.parametrize("n,v2p,env,exc,what", [
    (9, NADAL_FEDERER, {}, ValueError, "even"),
    (8, {"dual_mode": "different", "player": ["nadal", "borg"]}, {}, ValueError, "unknown player"),
    (8, {"dual_mode": "different", "player": ["nadal", "federer", "nadal"]}, {}, ValueError, "2 entries"),
    (8, dict(NADAL_FEDERER, player_body_models=[None] * 3), {}, ValueError, "2 body models"),
    (8, NADAL_FEDERER, {"body_model": "per-clip"}, NotImplementedError, "per-clip"),
])
def test_the_task_refuses_before_touching_a_gpu(n, v2p, env, exc, what):
    if env.get("body_model") == "per-clip":
        base = load_baked_model()
        env = {"body_model": [base, base.scaled(1.1)]}
    if v2p.get("player_body_models"):
        base = load_baked_model()
        v2p = dict(v2p, player_body_models=[base] * 3)
    with pytest.raises(exc, match=what):
        HumanoidSMPLIMRacketBall(_cfg(n, v2p, **env), device_type="cuda", device_id=0)


def test_racket_geom_mirror_matches_the_header():
    prog = r'''
#include <stdio.h>
#include <stddef.h>
#include "v2p_rollout.h"
int main(void){ printf("%zu %zu %zu %zu\n", sizeof(v2p_racket_geom), offsetof(v2p_racket_geom, num_cylinders), offsetof(v2p_racket_geom, cylinders),
                       offsetof(v2p_racket_geom, racket_offset)); return 0; }
'''
    with tempfile.TemporaryDirectory() as d:
        src = os.path.join(d, "s.c")
        open(src, "w").write(prog)
        exe = os.path.join(d, "s")
        subprocess.check_call(["gcc", "-I", os.path.join(REPO, "include"), src, "-o", exe])
        sizes = [int(x) for x in subprocess.check_output([exe]).split()]
    G = _lib.RacketGeom
    assert sizes == [ctypes.sizeof(G), G.num_cylinders.offset, G.cylinders.offset, G.racket_offset.offset]
    assert "v2p_env_set_racket_shapes" in _lib.EXPORTED_SYMBOLS


def test_the_setter_refuses_without_a_batch():
    """Argument checks happen before any HIP call: a null batch or null records come back as V2P_ERR_INVALID with a message."""
    L = _lib.load()
    g = (_lib.RacketGeom * 2)()
    assert L.v2p_env_set_racket_shapes(None, g, 2) == -1
    assert b"v2p_env_set_racket_shapes" in L.v2p_last_error()
    assert L.v2p_env_set_racket_shapes(None, None, 2) == -1


@pytest.mark.parametrize("pair", [("nadal", "federer"), ("federer", "djokovic")])
def test_with_racket_folds_each_player_of_a_pair(pair):
    base = load_baked_model()
    for p in pair:
        m, g = racket.with_racket(base, player=p)
        spec = racket.PLAYERS[p]
        b = base.body_index(spec["parent"])
        assert g["racket_link"] == b == (17 if p == "nadal" else 22) and g["player"] == p
        assert np.allclose(g["racket_offset"], spec["offset"])
        assert m.mass[b] > base.mass[b] and np.isclose(m.mass[b] - base.mass[b], g["racket_mass"])
        other = base.body_index("R_Wrist" if b == 17 else "L_Wrist")
        assert m.mass[other] == base.mass[other]  # the free hand stays as it was
        # the racket arm's ranges are the player's (Federer's R_Wrist_x is -90 .. 10 deg, Djokovic's -10 .. 10)
        j = 3 * (b - 1)
        assert np.allclose(np.rad2deg([m.limit_lower[j], m.limit_upper[j]]), spec["limits"][spec["parent"]][0])
        r = racket_geom_struct(g)
        assert r.racket_link == b and r.num_cylinders == 2
        assert np.allclose(list(r.racket_offset), spec["offset"])
        assert np.allclose(list(r.cylinders[1])[0:3], g["cylinders"][1]["center"], atol=1e-7)
