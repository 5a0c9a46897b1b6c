"""Golden data of the single-player controller's flag-driven reset and of the action part of its pre_physics_step, recorded from the
reference itself: tests/golden/tennis_reset.npz.

As tools/gen_golden_tennis_controller.py: `PhysicsMVAEController` and `HumanoidSMPLIMMVAE` are imported on the CPU through
oracle/ref_shim, objects made with `__new__` (a stand-in for the task) get their attributes by hand, and the reference's OWN code runs on
them: `pre_physics_step`, `_reset_envs` (with an empty id list: the flag-driven half), through it `_reset_balls`,
`TennisBallGeneratorOffline.generate`, `_reset_recovery_tasks`, `_reset_reaction_tasks` and `_compute_observations(ids)`.  Inside those
calls `torch.randint`, `torch.rand` and `Tensor.normal_` serve the values that the laws of csrc/philox.hpp derive from the recorded
words, each env's own (the reference deals its draws to the flagged envs in order of env id; served this way draw k IS the k-th flagged
env's): the statement fed the same words must then reproduce what the reference computed.

12 envs, a pool of 64 rows sorted by launch x, both pool rules, all three target modes, history on and off.  The words are crafted, not
generated: the generator asserts that every row of the flag truth table occurs, that the near rule's clamp is hit at both ends and in
the interior, and that each word-to-integer edge (w = 0, w = 0xffffffff) occurs.  Run where the reference exists:
    python tools/gen_golden_tennis_reset.py
"""
import math
import os
import sys
import tempfile
import types

sys.dont_write_bytecode = True  # never leave __pycache__ in the read-only reference mount

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(HERE)
sys.path.insert(0, os.path.join(REPO, "oracle"))
sys.path.insert(0, REPO)

from ref_shim.install import REFERENCE_ROOT, _Sink, install  # noqa: E402

install()
for absent in ("players", "players.mvae_player", "env.utils.player_builder", "smpl_visualizer", "smpl_visualizer.vis_sport", "tqdm"):
    try:
        __import__(absent)
    except Exception:
        sys.modules[absent] = _Sink(absent)
sys.path.insert(0, os.path.join(REFERENCE_ROOT, "vid2player"))

import torch  # noqa: E402

torch.set_num_threads(1)
torch.Tensor.get_device = lambda self: self.device

import env.tasks.humanoid_smpl_im_mvae as ref_task  # noqa: E402
import env.tasks.physics_mvae_controller as ref_ctl  # noqa: E402
import utils.tennis_ball as ref_ball  # noqa: E402

from vid2player3d_amd import device_rng as R  # noqa: E402

OUT = os.path.join(REPO, "tests", "golden", "tennis_reset.npz")
N, ROWS, L, NFRAMES = 12, 64, 10, 6
FLAGS = ((True, False), (False, True), (True, True), (False, False))  # env i has row i % 4 of the truth table
VARIANTS = {  # name: (sample_random, use_random_ball_target, use_history_ball_obs)
    "R0": (True, False, False),
    "R1": (True, True, True),
    "R2": (True, "continuous", False),
    "S0": (False, True, False),
}


class Served:
    """`torch.randint`, `torch.rand` and `Tensor.normal_` for the reference's calls: answers queued in the order the reference asks."""

    def __init__(self):
        self.queue = []

    def push(self, kind, values):
        self.queue.append((kind, np.asarray(values)))

    def _pop(self, kind, shape):
        assert self.queue, "the reference drew (%s %s) where nothing was expected" % (kind, shape)
        k, v = self.queue.pop(0)
        assert k == kind and tuple(v.shape) == tuple(shape), "the reference asked for %s %s, %s %s was queued" % (kind, tuple(shape), k, v.shape)
        return torch.from_numpy(v.copy())

    def randint(self, lo, hi, size, **kw):
        return self._pop("randint %d %d" % (lo, hi), tuple(int(x) for x in size))

    def rand(self, size, **kw):
        return self._pop("rand", (int(size),) if isinstance(size, int) else tuple(int(x) for x in size))

    def normal_(self, tensor, mean=0, std=1):
        assert (mean, std) == (0, 1)
        tensor.copy_(self._pop("normal", tuple(tensor.shape)))
        return tensor

    def __enter__(self):
        self.saved = (torch.randint, torch.rand, torch.Tensor.normal_)
        served = self
        torch.randint, torch.rand = self.randint, self.rand
        torch.Tensor.normal_ = lambda t, mean=0, std=1: served.normal_(t, mean, std)
        return self

    def __exit__(self, *exc):
        torch.randint, torch.rand, torch.Tensor.normal_ = self.saved
        if exc[0] is None:
            assert not self.queue, "the reference did not ask for %s" % [k for k, _ in self.queue]


def word_of(value, lo, hi):
    """a word whose integer law on [lo, hi) gives `value` (the middle of its cell)"""
    w = int((value - lo + 0.5) / (hi - lo) * 2 ** 32)
    assert int(R.integer(np.array([w], np.uint32), lo, hi)[0]) == value
    return w


def make_inputs(rng):
    s = {}
    pos = np.zeros((N, 25, 3), np.float32)
    pos[:, 0] = np.stack([rng.uniform(-3, 3, N), rng.uniform(-14, -10, N), rng.uniform(0.8, 1.0, N)], -1)
    pos[:, 1:] = pos[:, :1] + rng.uniform(-0.8, 0.8, (N, 24, 3))
    rot = rng.normal(0, 1, (N, 25, 4)).astype(np.float32)
    rot /= np.linalg.norm(rot, axis=-1, keepdims=True) * rng.uniform(0.98, 1.02, (N, 25, 1))
    s["pos25"], s["rot25"] = pos, rot.astype(np.float32)
    ball = np.zeros((N, 13), np.float32)
    ball[:, 0:3] = np.stack([rng.uniform(-3.5, 3.5, N), rng.uniform(1, 12, N), rng.uniform(0.3, 2.0, N)], -1)
    ball[[2, 10], 1] = -5.0  # two reacting balls on this side: the random row
    ball[:, 6] = 1
    ball[:, 7:13] = rng.normal(0, 5, (N, 6))
    s["ball_state"] = ball
    s["root_vel"] = rng.normal(0, 1.5, (N, 3)).astype(np.float32)
    pool = rng.normal(0, 1, (ROWS, 307)).astype(np.float32)
    pool[:, 0] = np.sort(rng.uniform(-4, 4, ROWS))
    pool[:, 1], pool[:, 2] = rng.uniform(12, 13, ROWS), rng.uniform(1, 1.5, ROWS)
    pool[:, 3:6] = rng.normal(0, 1, (ROWS, 3)) * (3, 3, 2) + (0, -25, 4)
    pool[:, 6] = rng.uniform(5, 10, ROWS)
    pool[:, 7:] = (np.cumsum(rng.normal(0, 0.3, (ROWS, 100, 3)), 1) + np.array([0, -11, 1])).reshape(ROWS, 300)
    s["pool"] = pool
    s["reset_reaction"], s["reset_recovery"] = [np.array([FLAGS[i % 4][k] for i in range(N)]) for k in (0, 1)]
    # ---- the words: [N,8]; reacting envs are 0, 2, 4, 6, 8, 10
    w = rng.integers(0, 2 ** 32, (N, 8), dtype=np.uint64).astype(np.uint32)
    w[2, 0], w[10, 0] = 0, 0xFFFFFFFF                       # the random row: first and last
    w[0, 1], w[4, 1] = 0, 0xFFFFFFFF                        # the near offset: -1000 and 999, the clamp's two ends
    w[6, 1], w[8, 1] = word_of(-3, -1000, 1000), word_of(5, -1000, 1000)  # ... and inside the pool
    w[0, 2], w[2, 2] = 0, 0xFFFFFFFF                        # the reaction time: nframes - 5 and nframes + 4
    w[0, 3], w[2, 3], w[4, 3] = 0, 0xFFFFFFFF, word_of(50, 0, 100)  # the target: left, right, middle
    w[:, 4:8] = w[0, 4:8]                                   # the whole call's draw
    s["words"] = w
    s["tar_action"] = rng.integers(0, 2, N).astype(np.int64)
    s["tar_time"], s["tar_time_total"] = rng.integers(0, 9, N).astype(np.int64), rng.integers(1, 9, N).astype(np.int64)
    s["num_reset_reaction"] = rng.integers(0, 5, N).astype(np.int64)
    s["sample_idx"] = np.array([ROWS - 1, 3, 0, 7, ROWS - 1, 9, 20, 11, 63, 1, 62, 5], np.int64)
    s["has_bounce"], s["has_racket_contact"], s["bounce_in"], s["est_bounce_in"] = [rng.uniform(size=N) < 0.5 for _ in range(4)]
    s["bounce_pos"], s["est_bounce_pos"] = rng.normal(0, 3, (N, 3)).astype(np.float32), rng.normal(0, 3, (N, 3)).astype(np.float32)
    s["est_bounce_time"], s["est_max_height"] = rng.uniform(0, 1, N).astype(np.float32), rng.uniform(0, 3, N).astype(np.float32)
    s["swing_type_cycle"] = rng.integers(0, 4, N).astype(np.int64)
    s["target_bounce_pos"] = np.tile(np.float32([0, 10, 0]), (N, 1))
    s["ball_traj"] = rng.normal(0, 3, (N, 100, 3)).astype(np.float32)
    s["ball_obs"] = rng.normal(0, 3, (N, L, 3)).astype(np.float32)
    s["prev_ball_vy"] = rng.normal(0, 3, N).astype(np.float32)
    return s


def make_objects(s, sample_random, target, history, pool_file):
    F = torch.from_numpy
    z = lambda *shape, dtype=torch.float32: torch.zeros(shape, dtype=dtype)
    task = types.SimpleNamespace(cfg={"sim": {"substeps": 2}}, cfg_v2p={"grip": "eastern"}, _is_train=True, num_envs=N, device="cpu", viewer=None,
                                 _has_racket_ball_contact=F(s["has_racket_contact"].copy()), _has_racket_ball_contact_now=z(N, dtype=torch.bool),
                                 _ball_root_states=F(s["ball_state"].copy()), _ball_pos=z(N, 3), _ball_vel=z(N, 3), _ball_vspin=z(N), _root_pos=z(N, 3), _root_vel=z(N, 3),
                                 _humanoid_root_states=z(N, 13), _rigid_body_pos=F(s["pos25"].copy()), _rigid_body_rot=F(s["rot25"].copy()), _rigid_body_vel=z(N, 25, 3),
                                 _racket_body_id=24, _racket_pos=z(N, 3), _racket_vel=z(N, 3), _racket_normal=z(N, 3), _lefthand=None, _racket_wrist_body_id=22,
                                 _has_bounce=F(s["has_bounce"].copy()), _has_bounce_now=z(N, dtype=torch.bool), _bounce_pos=F(s["bounce_pos"].copy()))
    task._humanoid_root_states[:, 0:3] = task._rigid_body_pos[:, 0]
    task._humanoid_root_states[:, 7:10] = F(s["root_vel"])
    ref_task.HumanoidSMPLIMMVAE._update_state_from_sim(task)
    task._ball_vel[:, 1] = F(s["prev_ball_vy"])
    task._ball_generator = ref_ball.TennisBallGeneratorOffline(pool_file, sample_random=sample_random, num_envs=N)
    if not sample_random:
        task._ball_generator.sample_idx[:] = F(s["sample_idx"])
    # (`task.reset(humanoid_ids, reaction_ids)` of the physics player's task: with no humanoid to reset it is `_reset_balls`)
    task.reset = lambda humanoid_ids, reaction_ids: ref_task.HumanoidSMPLIMMVAE._reset_balls(task, reaction_ids, humanoid_ids)
    task.post_mvae_step = lambda: None
    mvae = types.SimpleNamespace(_swing_type_cycle=F(s["swing_type_cycle"].copy()), reset=lambda ids: None, step=lambda a, r: None)
    c = ref_ctl.PhysicsMVAEController.__new__(ref_ctl.PhysicsMVAEController)
    c.cfg = {"env": {"episodeLength": 300}}
    c.cfg_v2p = {"obs_ball_traj_length": L, "use_history_ball_obs": history, "use_random_ball_target": target, "reset_reaction_nframes": NFRAMES,
                 "random_walk_in_recovery": True, "vae_action_scale": 1.5, "add_residual_dof": "euler", "residual_dof_scale": 0.4, "add_residual_root": True,
                 "residual_root_scale": 0.02}
    c._is_train, c.device, c.num_envs, c.headless, c._has_init = True, "cpu", N, True, True
    c._physics_player, c._mvae_player = types.SimpleNamespace(task=task), mvae
    c.obs_buf = z(N, 225 + 3 * L + (2 if target else 0))
    c.reset_buf, c.progress_buf, c._terminate_buf = z(N, dtype=torch.long), z(N, dtype=torch.long), z(N, dtype=torch.long)
    c._obs_ball_traj_length, c._num_humanoid_bodies, c._racket_body_id = L, 24, 24
    c._ball_traj, c._ball_obs = F(s["ball_traj"].copy()), F(s["ball_obs"].copy())
    c._bounce_in, c._est_bounce_pos, c._est_bounce_time = F(s["bounce_in"].copy()), F(s["est_bounce_pos"].copy()), F(s["est_bounce_time"].copy())
    c._est_bounce_in, c._est_max_height = F(s["est_bounce_in"].copy()), F(s["est_max_height"].copy())
    c._tar_time, c._tar_time_total, c._tar_action = F(s["tar_time"].copy()), F(s["tar_time_total"].copy()), F(s["tar_action"].copy())
    c._target_bounce_pos = F(s["target_bounce_pos"].copy())
    c._target_bounce_min, c._target_bounce_max = torch.FloatTensor([-3, 9, 0]), torch.FloatTensor([3, 11, 0])
    c._reset_reaction_buf, c._reset_recovery_buf = F(s["reset_reaction"].copy()), F(s["reset_recovery"].copy())
    c._num_reset_reaction, c._num_reset, c._distance = F(s["num_reset_reaction"].copy()), z(N, dtype=torch.long), z(N)
    c._num_mvae_action, c._num_res_dof_action, c._mvae_actions_random = 32, 3, z(N, 32)
    c._root_pos, c._ball_pos, c._racket_normal = task._root_pos, task._ball_pos, task._racket_normal
    return c, task, mvae


def run_reset(name, s, pool_file):
    sample_random, target, history = VARIANTS[name]
    c, task, mvae = make_objects(s, sample_random, target, history, pool_file)
    w = s["words"]
    rx = np.nonzero(s["reset_reaction"])[0]
    with Served() as served:
        if sample_random:
            served.push("randint 0 %d" % ROWS, R.integer(w[rx, 0], 0, ROWS))
            other = s["ball_state"][rx, 1] > 0
            served.push("randint -1000 1000", R.integer(w[rx[other], 1], -1000, 1000))
        served.push("randint -5 5", R.integer(w[rx, 2], -5, 5))
        if target == "continuous":
            served.push("rand", R.uniform(w[0, 4:7]))
        elif target:
            served.push("rand", R.uniform(w[rx, 3]))
        c._reset_envs(torch.zeros(0, dtype=torch.long))
    o = dict(ball_state=task._ball_root_states, has_bounce=task._has_bounce, bounce_pos=task._bounce_pos, has_racket_contact=task._has_racket_ball_contact,
             prev_ball_vy=task._ball_vel[:, 1], tar_action=c._tar_action, tar_time=c._tar_time, tar_time_total=c._tar_time_total, num_reset_reaction=c._num_reset_reaction,
             bounce_in=c._bounce_in, est_bounce_pos=c._est_bounce_pos, est_bounce_time=c._est_bounce_time, est_bounce_in=c._est_bounce_in, est_max_height=c._est_max_height,
             swing_type_cycle=mvae._swing_type_cycle, target_bounce_pos=c._target_bounce_pos, obs=c.obs_buf, ball_obs=c._ball_obs)
    if not history:
        o["ball_traj"] = c._ball_traj  # (the reference keeps the window only where the observation reads it)
    if not sample_random:
        o["sample_idx"] = task._ball_generator.sample_idx
    o = {k: v.detach().clone().numpy() for k, v in o.items()}
    # the spin in double: what the float32 chain of `_reset_balls` scatters by
    rows = np.array([int(np.nonzero((s["pool"][:, 0:3] == o["ball_state"][e, 0:3]).all(1))[0][0]) for e in rx])
    vel, vspin = s["pool"][rows, 3:6].astype(np.float64), s["pool"][rows, 6].astype(np.float64)
    cr = np.stack([-vel[:, 1], vel[:, 0], np.zeros(len(rx))], -1)
    spin64 = vspin[:, None] * math.pi * 2 * cr / np.linalg.norm(cr, axis=1, keepdims=True)
    o["scatter_ball_state"] = np.float64(np.abs(o["ball_state"][rx, 10:13] - spin64).max())
    o["pool_rows"] = np.full(N, -1, np.int64)
    o["pool_rows"][rx] = rows
    o["racket_pos"], o["racket_normal"] = task._racket_pos.numpy().copy(), task._racket_normal.numpy().copy()
    o["settings"] = np.array([int(sample_random), {False: 0, True: 1, "continuous": 2}[target], int(history)], np.int64)
    return o


def run_actions(s, rng, pool_file):
    c, task, mvae = make_objects(s, True, False, False, pool_file)
    actions = rng.normal(0, 1, (N, 41)).astype(np.float32)  # three unused columns behind the 38
    tar_action = (np.arange(N) % 3 != 0).astype(np.int64)
    words = rng.integers(0, 2 ** 32, (N, 32), dtype=np.uint64).astype(np.uint32)
    words[0, :8] = [0, 0, 0xFFFFFFFF, 0, 0, 0x40000000, 255, 0xFFFFFFFF]  # the largest normal (clamped), r = 0, a quarter turn
    c._tar_action = torch.from_numpy(tar_action)
    walk = tar_action == 0
    with Served() as served:
        served.push("normal", R.normals(words[walk]))
        c.pre_physics_step(torch.from_numpy(actions))
    z64 = R.clamped_normals(words[walk], 5.0, np.float64)
    got = c._mvae_actions.numpy()
    assert (np.abs(got[walk]) == 5.0).any(), "the clamp was not reached"
    return {"actions/actions": actions, "actions/tar_action": tar_action, "actions/words": words, "actions/actions_out": c._actions.numpy()[:, :38],
            "actions/mvae_actions": got, "actions/res_dof_actions": c._res_dof_actions.numpy(), "actions/res_root_actions": c._res_root_actions.numpy(),
            "actions/scatter_mvae_actions": np.float64(np.abs(got[walk] - z64).max())}


def main():
    rng = np.random.default_rng(2032)
    s = make_inputs(rng)
    out = {k: v for k, v in s.items()}
    with tempfile.TemporaryDirectory() as d:
        pool_file = os.path.join(d, "pool.npy")
        np.save(pool_file, s["pool"])
        near_rows = set()
        for name in VARIANTS:
            o = run_reset(name, s, pool_file)
            out.update({"%s/%s" % (name, k): v for k, v in o.items()})
            if VARIANTS[name][0]:
                near = s["reset_reaction"] & (s["ball_state"][:, 1] > 0)
                picked = o["pool_rows"][near]
                near_rows |= ({"low"} if (picked == 0).any() else set()) | ({"high"} if (picked == ROWS - 1).any() else set())
                near_rows |= {"inside"} if ((picked > 0) & (picked < ROWS - 1)).any() else set()
                assert o["pool_rows"][2] == 0 and o["pool_rows"][10] == ROWS - 1, "the random row's word edges"
            if VARIANTS[name][1] is True:
                assert o["target_bounce_pos"][[0, 2, 4], 0].tolist() == [-3.0, 3.0, 0.0], "the three targets"
            assert o["tar_time_total"][0] == NFRAMES - 5 and o["tar_time_total"][2] == NFRAMES + 4, "the reaction time's word edges"
        assert near_rows == {"low", "high", "inside"}, near_rows
        assert set(zip(s["reset_reaction"].tolist(), s["reset_recovery"].tolist())) == set(FLAGS), "every row of the flag truth table"
        out.update(run_actions(s, rng, pool_file))
    rb = np.zeros((N, 24, 13), np.float32)
    rb[:, :, 0:3], rb[:, :, 3:7] = s["pos25"][:, :24], s["rot25"][:, :24]
    rk = np.zeros((N, 13), np.float32)
    rk[:, 0:3], rk[:, 3:7] = s["pos25"][:, 24], s["rot25"][:, 24]
    out.update(rb_state=rb, racket_state=rk)
    del out["pos25"], out["rot25"]
    np.savez_compressed(OUT, **out)
    print("wrote", os.path.relpath(OUT, REPO), "%.3f MB" % (os.path.getsize(OUT) / 1e6))


if __name__ == "__main__":
    main()
