"""CPU checks of the single-player controller's flag-driven task reset: the numpy statement `task_reset_reference` against the parent's
own torch lines (`TennisControllerTask._reset_envs`, `HumanoidSMPLIMRacketBall.reset_balls`, `TennisBallGeneratorOffline.indices`) said
again on CPU tensors with `torch.randint` / `torch.rand` served from the words, the argument checks of `v2p_tennis_task_reset` and the
layout of its two structs."""
import numpy as np
import torch

from tests import tennis_edges as E
from tests import tennis_fixture as F
from tests.test_gpu_tennis_reset import FLAGS, POOLS, TARGETS, case, edge_words
from vid2player3d_amd import _lib
from vid2player3d_amd import device_rng as R
from vid2player3d_amd.ball_traj import launch_ang_vel
from vid2player3d_amd.tasks import tennis_controller as tc


def torch_lines(st, s, words):
    """The parent's torch path on CPU tensors, in its order; the draws are the laws of device_rng on the env's own words."""
    T = lambda k, dt=None: torch.as_tensor(np.array(s[k])).to(dt) if dt else torch.as_tensor(np.array(s[k]))
    n = len(s["ball_state"])
    w = np.asarray(words, np.uint32)
    rx, rc = T("reset_reaction", torch.bool), T("reset_recovery", torch.bool)
    reaction_ids, recovery_ids = rx.nonzero().flatten(), rc.nonzero().flatten()
    o = {k: T(k) for k in ("ball_state", "bounce_pos", "ball_traj", "traj_cursor", "prev_ball_vy", "tar_action", "tar_time", "tar_time_total", "num_reset_reaction",
                           "est_bounce_pos", "est_bounce_time", "est_max_height", "swing_type_cycle", "target_bounce_pos")}
    o.update({k: T(k, torch.bool) for k in ("has_bounce", "has_racket_contact", "bounce_in", "est_bounce_in")})
    o["ball_traj"] = o["ball_traj"].reshape(n, 100, 3)
    pool = torch.as_tensor(s["pool"])
    launch_pos, launch_vel, launch_vspin, traj_pool = pool[:, 0:3], pool[:, 3:6], pool[:, 6], pool[:, 7:].reshape(len(pool), -1, 3)
    n_pool = len(pool)
    if len(reaction_ids):
        ids = reaction_ids
        # ---- TennisBallGeneratorOffline.indices
        if st["pool_rule"] == "random":
            idx = torch.as_tensor(R.integer(w[ids.numpy(), 0], 0, n_pool))  # torch.randint(0, n_pool, (n_traj,))
            start_pos = o["ball_state"][ids, 0:3]
            other = start_pos[:, 1] > 0
            near = ((start_pos[:, 0] + 4) / 8 * n_pool).long() + torch.as_tensor(R.integer(w[ids.numpy(), 1], -1000, 1000))  # torch.randint(-1000, 1000, (n_traj,))
            idx = torch.where(other, torch.clamp(near, 0, n_pool - 1), idx)
        else:
            sample_idx = T("sample_idx")
            idx = sample_idx[ids].clone()
            sample_idx[ids] += 1
            sample_idx[ids] %= n_pool
            o["sample_idx"] = sample_idx
        new_traj, lp, lv, vspin = traj_pool[idx].clone(), launch_pos[idx], launch_vel[idx], launch_vspin[idx]
        # ---- reset_balls
        o["ball_state"][ids, 0:3] = lp
        o["ball_state"][ids, 3:7] = torch.tensor([0.0, 0.0, 0.0, 1.0])
        o["ball_state"][ids, 7:10] = lv
        o["ball_state"][ids, 10:13] = launch_ang_vel(lv, vspin)
        o["has_bounce"][ids] = False
        o["bounce_pos"][ids] = 0
        o["has_racket_contact"][ids] = False
        # ---- _reset_envs
        frames = min(new_traj.shape[1], 100)
        o["ball_traj"][ids] = 0
        o["ball_traj"][ids, :frames] = new_traj[:, :frames]
        o["traj_cursor"][ids] = 0
        o["prev_ball_vy"][ids] = o["ball_state"][ids, 8]
    if len(recovery_ids):
        o["tar_action"][recovery_ids] = 0
        o["has_bounce"][recovery_ids] = False
        o["bounce_pos"][recovery_ids] = 0
    if len(reaction_ids):
        ids = reaction_ids
        if st["use_history"]:
            o["ball_obs"] = T("ball_obs")
            o["ball_obs"][ids] = o["ball_state"][ids, 0:3].view(-1, 1, 3).repeat(1, st["L"], 1)
        o["tar_time"][ids] = 0
        o["tar_action"][ids] = 1
        o["num_reset_reaction"][ids] += 1
        o["bounce_in"][ids] = False
        o["est_bounce_pos"][ids, :] = 0
        o["est_bounce_time"][ids] = 0
        o["est_bounce_in"][ids] = False
        o["est_max_height"][ids] = 0
        o["swing_type_cycle"][ids] = -1
        o["tar_time_total"][ids] = int(st["reset_reaction_nframes"]) + torch.as_tensor(R.integer(w[ids.numpy(), 2], -5, 5))  # torch.randint(-5, 5, (len(env_ids),))
        lo, hi = torch.tensor(st["target_min"]), torch.tensor(st["target_max"])
        if st["target_mode"] == "continuous":
            o["target_bounce_pos"][ids] = torch.as_tensor(R.uniform(w[0, 4:7])) * (hi - lo) + lo  # torch.rand((3,)): the whole call's draw
        elif st["target_mode"]:
            seed = torch.as_tensor(R.uniform(w[ids.numpy(), 3]))  # torch.rand((len(env_ids),))
            x = torch.where(seed < 0.33, -3.0, torch.where(seed > 0.67, 3.0, 0.0))
            o["target_bounce_pos"][ids] = torch.stack([x, torch.full_like(x, 10.0), torch.zeros_like(x)], -1)
    return {k: v.numpy() for k, v in o.items()}


def test_statement_is_the_parents_torch_path():
    """every variant (history on / off, three target modes), both pool rules, three pools, every row of the flag truth table, the near
    rule's clamp at both ends and inside, both edges of every word law: the statement's arrays are the torch lines' bits; the observation
    rows are `observation_reference` of the new state"""
    census, flag_rows = set(), set()
    for name in sorted(TARGETS):
        for rows in sorted(POOLS):
            for rule in ("random", "round_robin"):
                n = 40
                st, s = case(name, n, rows, rule)
                words = edge_words(n, rows)
                want = torch_lines(st, s, words)
                got = tc.task_reset_reference(st, s, words)
                what = "variant %s, pool of %d rows, %s" % (name, rows, rule)
                for k, w in want.items():
                    if k == "ball_obs":  # (the torch lines hold the fill; the statement's has been rolled by the observation: below)
                        continue
                    assert np.array_equal(got[k].reshape(w.shape), w, equal_nan=True), "%s: %s differs from the torch lines" % (what, k)
                rx, rc = s["reset_reaction"], s["reset_recovery"]
                flag_rows |= set(zip(rx.tolist(), rc.tolist()))
                ids = np.nonzero(rx | rc)[0]
                s2 = dict(s, **{k: want[k] for k in ("ball_state", "ball_traj", "traj_cursor", "target_bounce_pos") + (("ball_obs",) if st["use_history"] else ())})
                obs, hist, rpos, rnorm = tc.observation_reference(st, s2, ids)
                assert np.array_equal(got["obs"][ids], obs, equal_nan=True) and np.array_equal(got["racket_pos"][ids], rpos) and np.array_equal(got["racket_normal"][ids], rnorm)
                others = np.setdiff1d(np.arange(n), ids)
                for k in tc.RESET_WRITES:
                    if s.get(k) is not None:
                        assert np.array_equal(np.asarray(got[k]).reshape(np.asarray(s[k]).shape)[others], np.asarray(s[k])[others], equal_nan=True), "%s: %s of an env without a flag" % (what, k)
                if st["use_history"]:
                    assert np.array_equal(got["ball_obs"][ids], hist)
                if rule == "random" and rows == 2500:
                    near = rx & (s["ball_state"][:, 1] > 0)
                    picked = got["pool_rows"][near]
                    census |= ({"low"} if (picked == 0).any() else set()) | ({"high"} if (picked == rows - 1).any() else set())
                    census |= {"inside"} if ((picked > 0) & (picked < rows - 1)).any() else set()
                    assert (words[rx][:, 0:4] == 0).all(1).any() and (words[rx][:, 0:4] == 0xFFFFFFFF).all(1).any(), "both word edges reach a reacting env"
    assert flag_rows == set(FLAGS) and census == {"low", "high", "inside"}
    # nothing in the inputs was modified
    st, s = case("B", 8, 3, "round_robin")
    keep = {k: np.array(v) for k, v in s.items() if v is not None}
    tc.task_reset_reference(st, s, edge_words(8, 1))
    assert all(np.array_equal(keep[k], s[k], equal_nan=True) for k in keep)


def test_entry_refuses_bad_arguments_without_a_gpu():
    import ctypes as C

    L = _lib.load()
    one = 16  # (a non-null placeholder: every call below is refused before anything is dereferenced)
    st = dict(F.settings("A")[0])
    c = tc.cfg_struct(st, (1, 1), (1, 1, 2))

    def rcfg(**kw):
        d = dict(reset_reaction_nframes=6, target_mode=0, pool_rule=0, pool_rows=10, pool_frames=100, pool_stride=307, seed=1, call=0)
        d.update(kw)
        return _lib.TennisResetCfg(**d)

    def bufs(**kw):
        return _lib.TennisBuffers(**dict({k: one for k in _lib.TENNIS_BUFFER_NAMES}, **kw))

    def rbufs(**kw):
        return _lib.TennisResetBuffers(**dict({k: one for k in _lib.TENNIS_RESET_BUFFER_NAMES if k != "words"}, **kw))

    fn = L.v2p_tennis_task_reset
    ref = lambda x: None if x is None else C.byref(x)
    bad_L = tc.cfg_struct(dict(st, L=100), (1, 1), (1, 1, 2))
    bad_L.obs_ball_traj_length = 101
    refused = [(None, rcfg(), 4, bufs(), rbufs()), (c, None, 4, bufs(), rbufs()), (c, rcfg(), 4, None, rbufs()), (c, rcfg(), 4, bufs(), None), (c, rcfg(), -1, bufs(), rbufs()),
               (bad_L, rcfg(), 4, bufs(), rbufs()), (c, rcfg(pool_rows=0), 4, bufs(), rbufs()), (c, rcfg(pool_frames=0), 4, bufs(), rbufs()),
               (c, rcfg(pool_frames=101), 4, bufs(), rbufs()), (c, rcfg(pool_stride=306), 4, bufs(), rbufs()), (c, rcfg(target_mode=3), 4, bufs(), rbufs()),
               (c, rcfg(target_mode=-1), 4, bufs(), rbufs()), (c, rcfg(pool_rule=2), 4, bufs(), rbufs()), (c, rcfg(), 4, bufs(obs=None), rbufs()),
               (c, rcfg(), 4, bufs(reset_reaction=None), rbufs()), (c, rcfg(), 4, bufs(), rbufs(pool=None)), (c, rcfg(), 4, bufs(), rbufs(ball_state=None)),
               (c, rcfg(pool_rule=1), 4, bufs(), rbufs(sample_idx=None)), (c, rcfg(target_mode=1), 4, bufs(), rbufs(target_bounce_pos=None)),
               (c, rcfg(), 4, bufs(), rbufs(ball_traj=32))]
    for args in refused:
        assert fn(ref(args[0]), ref(args[1]), args[2], ref(args[3]), ref(args[4]), None) == -1
        assert b"v2p_tennis_task_reset" in L.v2p_last_error()
    assert fn(C.byref(c), C.byref(rcfg()), 0, C.byref(_lib.TennisBuffers()), C.byref(_lib.TennisResetBuffers()), None) == 0  # n = 0 is a no-op
    assert L.v2p_abi_version() == 15


def test_struct_sizes_match_the_header(tmp_path):
    import ctypes as C
    import os
    import subprocess

    prog = r'''
#include <stdio.h>
#include <stddef.h>
#include "v2p_rollout.h"
int main(void){ printf("%zu %zu %zu %zu\n", sizeof(v2p_tennis_reset_cfg), sizeof(v2p_tennis_reset_buffers), offsetof(v2p_tennis_reset_cfg, pool_stride),
                       offsetof(v2p_tennis_reset_cfg, seed)); return 0; }
'''
    src, exe = tmp_path / "s.c", tmp_path / "s"
    src.write_text(prog)
    subprocess.check_call(["gcc", "-I", os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include"), str(src), "-o", str(exe)])
    sizes = [int(x) for x in subprocess.check_output([str(exe)]).split()]
    assert sizes == [C.sizeof(_lib.TennisResetCfg), C.sizeof(_lib.TennisResetBuffers), _lib.TennisResetCfg.pool_stride.offset, _lib.TennisResetCfg.seed.offset]


# ------------------------------------------------------------------------------------------------------------------ the reference's fixture
def fixture():
    import os

    with np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "tennis_reset.npz")) as z:
        return {k: z[k] for k in z.files}


def test_statements_reproduce_what_the_reference_computed():
    """tests/golden/tennis_reset.npz (tools/gen_golden_tennis_reset.py): the reference's own `_reset_envs` / `_reset_balls` /
    `TennisBallGeneratorOffline.generate` / task resets / `_compute_observations` and `pre_physics_step`, its draws served from the
    recorded words.  Flags, integers, pool rows and copies exact; the spin within 8 x the recorded float32 - float64 scatter; the
    observation rows at the tolerance the task step's own fixture test holds them to (tests/tennis_fixture.py: OBS_TOL)."""
    g = fixture()
    n = len(g["ball_state"])
    root_states = np.zeros((n, 13), np.float32)
    root_states[:, 0:3], root_states[:, 7:10] = g["rb_state"][:, 0, 0:3], g["root_vel"]
    names = sorted(k.split("/")[0] for k in g if k.endswith("/settings"))
    assert names == ["R0", "R1", "R2", "S0"]
    modes = set()
    for name in names:
        sample_random, target, history = [int(x) for x in g[name + "/settings"]]
        target = (False, True, "continuous")[target]
        modes.add((sample_random, target, history))
        st = dict(tc.task_settings(obs_ball_traj_length=10, use_history_ball_obs=bool(history), use_random_ball_target=bool(target), court_min=(-20.0, -40.0),
                                   court_max=(20.0, 0.0)), **tc.reset_settings(6, target, bool(sample_random)))
        s = {k: g[k] for k in ("ball_state", "pool", "reset_reaction", "reset_recovery", "tar_action", "tar_time", "tar_time_total", "num_reset_reaction", "sample_idx",
                               "has_bounce", "has_racket_contact", "bounce_in", "est_bounce_in", "bounce_pos", "est_bounce_pos", "est_bounce_time", "est_max_height",
                               "swing_type_cycle", "target_bounce_pos", "ball_traj", "ball_obs", "prev_ball_vy", "rb_state", "racket_state")}
        s.update(root_states=root_states, wrist_link=np.full(n, 22, np.int64), traj_cursor=np.zeros(n, np.int32), obs=np.zeros((n, tc.obs_width(st)), np.float32),
                 racket_pos=np.zeros((n, 3), np.float32), racket_normal=np.zeros((n, 3), np.float32))
        got = tc.task_reset_reference(st, s, g["words"])
        flagged = g["reset_reaction"] | g["reset_recovery"]
        rx = g["reset_reaction"]
        exact = ["has_bounce", "bounce_pos", "has_racket_contact", "prev_ball_vy", "tar_action", "tar_time", "tar_time_total", "num_reset_reaction", "bounce_in",
                 "est_bounce_pos", "est_bounce_time", "est_bounce_in", "est_max_height", "swing_type_cycle", "target_bounce_pos", "ball_obs", "pool_rows"]
        exact += [k for k in ("ball_traj", "sample_idx") if "%s/%s" % (name, k) in g]
        for k in exact:
            want = g["%s/%s" % (name, k)]
            assert np.array_equal(np.asarray(got[k]).reshape(want.shape).astype(want.dtype), want), "variant %s: %s differs from the reference" % (name, k)
        want = g[name + "/ball_state"]
        assert np.array_equal(got["ball_state"][:, 0:10], want[:, 0:10]), "variant %s: the launch state is a copy" % name
        scatter = float(g[name + "/scatter_ball_state"])
        err = float(np.abs(got["ball_state"][:, 10:13].astype(np.float64) - want[:, 10:13]).max())
        print("variant %s: spin max |difference| %.3g, scatter %.3g" % (name, err, scatter))
        assert err <= 8 * scatter
        F.close_nan(got["obs"][flagged], g[name + "/obs"][flagged], F.OBS_TOL, "variant %s: observation rows" % name)
        assert np.array_equal(got["racket_pos"][flagged], g[name + "/racket_pos"][flagged])
        F.close_nan(got["racket_normal"][flagged], g[name + "/racket_normal"][flagged], F.OBS_TOL, "variant %s: racket normal" % name)
        assert (got["traj_cursor"][rx] == 0).all()  # (the reference's `_ball_traj` is the rolled tensor: every window here starts at frame 0)
    assert {m[0] for m in modes} == {0, 1} and {m[1] for m in modes} == {False, True, "continuous"} and {m[2] for m in modes} == {0, 1}
    # ---- the action part
    st = tc.action_settings(num_res_dof=3, num_res_root=3, vae_action_scale=1.5, residual_dof_scale=0.4, residual_root_scale=0.02, random_walk=True)
    got = tc.controller_actions_reference(st, g["actions/actions"], g["actions/tar_action"], g["actions/words"])
    for k in ("actions_out", "res_dof_actions", "res_root_actions"):
        assert np.array_equal(got[k], g["actions/" + k]), k
    walk = g["actions/tar_action"] == 0
    assert np.array_equal(got["mvae_actions"][~walk], g["actions/mvae_actions"][~walk])
    scatter = float(g["actions/scatter_mvae_actions"])
    err = float(np.abs(got["mvae_actions"][walk].astype(np.float64) - g["actions/mvae_actions"][walk]).max())
    print("drawn latents: max |difference| %.3g, scatter %.3g" % (err, scatter))
    assert scatter > 0 and err <= 8 * scatter and (np.abs(g["actions/mvae_actions"][walk]) == 5.0).any()
