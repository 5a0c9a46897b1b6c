"""Two players in one racket + ball batch (cfg_v2p dual_mode `different`: vid2player/cfg/controller/nadal_federer.yaml, federer_djokovic.yaml):
env i is player i % 2, each player's racket on its own wrist (v2p_env_set_racket_shapes) and its own arm ranges.  Every env against the
float64 oracle of its own player; a mixed batch against batches of one player, bit for bit; substep jobs; the setter's refusals."""
import numpy as np
import pytest
import torch
from scipy.spatial.transform import Rotation

from oracle import task_oracle as O
from oracle.phys_oracle import PhysOracle, default_params
from tests.gpu_util import DEV, N, T, close, synth_tables

pytestmark = pytest.mark.gpu

TIE_TOL = 5e-5
PAIRS = {"nadal_federer": (["nadal", "federer"], [False, True]), "federer_djokovic": (["federer", "djokovic"], [True, True])}
WRIST_X = 3 * (22 - 1)  # R_Wrist_x: Federer -90 .. 10 deg, Djokovic -10 .. 10 deg


@pytest.fixture(scope="module")
def mlib():
    from vid2player3d_amd.motion_lib import MotionLib

    return MotionLib(synth_tables(seed=5, num_clips=8, min_frames=60, max_frames=120), DEV)


def make_pair_task(n, lib, players, hands=None, sim_overrides=None, iterations=None, **env):
    from vid2player3d_amd.tasks import HumanoidSMPLIMRacketBall, default_cfg

    env.setdefault("debug_contacts", 2)
    env.setdefault("body_shape_mismatch", "ignore")
    env.setdefault("contact_forces_sum", True)
    env.setdefault("joint_limits", True)
    cfg = default_cfg(n, motion_lib=lib, sample_first_motions=True, **env)
    cfg["sim"].update(sim_overrides or {})
    if iterations is not None:
        cfg["sim"]["physx"] = dict(cfg["sim"]["physx"], num_position_iterations=iterations)
    cfg["v2p"] = {"dual_mode": "different", "player": list(players)}
    if hands is not None:
        cfg["v2p"]["righthand"] = list(hands)
    return HumanoidSMPLIMRacketBall(cfg, device_type="cuda", device_id=0)


def _launch(task, rng, mode):
    """Ball states [n,13]: 'hit' = at the face of each env's OWN racket head, 'body' = at a link's hull (not the racket's), 'ground'."""
    n = task.num_envs
    ball = np.zeros((n, 13), np.float32)
    ball[:, 6] = 1
    rb = N(task._rigid_body_state).reshape(n, 24, 13)
    for e in range(n):
        geom = task.racket_geometries[e % 2]
        rl = geom["racket_link"]
        if mode == "ground":
            ball[e, 0:2] = rb[e, 0, 0:2] + rng.uniform(3, 5, 2)
            ball[e, 2] = rng.uniform(0.03, 0.25)
            ball[e, 7:10] = [rng.normal(0, 6), rng.normal(0, 6), rng.uniform(-12, 1)]
            ball[e, 10:13] = rng.normal(0, 60, 3)
        elif mode == "body":
            bm = task.body_shapes[e % 2]
            off = np.asarray(bm.hull_offsets)
            hv = np.asarray(bm.hull_verts, dtype=np.float64)
            b = int(rng.choice([k for k in (0, 1, 2, 5, 6, 9, 10, 11, 12, 13, 14, 15, 16, 17, 19, 20, 21, 22, 23) if k != rl]))
            Rw = Rotation.from_quat(rb[e, b, 3:7]).as_matrix()
            v = hv[off[b]:off[b + 1]]
            target = rb[e, b, 0:3] + Rw @ (0.5 * (v.min(0) + v.max(0)))
            d = rng.normal(size=3)
            d[2] = abs(d[2])
            d /= np.linalg.norm(d)
            ball[e, 0:3] = target + rng.uniform(0.2, 0.45) * d
            ball[e, 7:10] = -rng.uniform(4, 30) * d + rng.normal(0, 1, 3) + rb[e, b, 7:10]
            ball[e, 10:13] = rng.normal(0, 80, 3)
        else:
            Rw = Rotation.from_quat(rb[e, rl, 3:7]).as_matrix()
            centre = rb[e, rl, 0:3] + Rw @ geom["cylinders"][1]["center"]
            normal = Rw @ geom["cylinders"][1]["axis"] * (1 if (e // 2) % 2 else -1)
            side = np.cross(normal, [0.3, 0.5, 0.8])
            side /= np.linalg.norm(side)
            ball[e, 0:3] = centre + rng.uniform(0.06, 0.25) * normal + rng.uniform(0, 0.11) * side
            ball[e, 7:10] = -rng.uniform(4, 30) * normal + rng.normal(0, 2, 3)
            ball[e, 10:13] = rng.normal(0, 80, 3)
    return ball


def _prepare(task, rng, lift=0.0, wrist_push=False):
    n = task.num_envs
    task.reset_with_times(None, T(rng.uniform(0.1, 1.0, size=n)))
    root = N(task._humanoid_root_states).copy()
    root[:, 2] += lift
    root[:, 7:13] += rng.normal(0, 0.5, (n, 6)).astype(np.float32)
    dpos = N(task._dof_pos).copy() + rng.normal(0, 0.05, (n, 69)).astype(np.float32)
    dvel = N(task._dof_vel).copy() + rng.normal(0, 1.0, (n, 69)).astype(np.float32)
    if wrist_push:  # R_Wrist_x just inside Djokovic's range, turning towards -45 deg: only the Djokovic envs stop at -10 deg
        dpos[:, WRIST_X] = np.deg2rad(-9.0)
        dvel[:, WRIST_X] = -3.0
    task._humanoid_root_states[:] = T(root)
    task._dof_pos[:] = T(dpos)
    task._dof_vel[:] = T(dvel)
    task._reset_env_tensors(None)
    return root, dpos, dvel


def _actions(task, rng, wrist_push=False):
    n = task.num_envs
    act = np.concatenate([N(task._target_dof_pos) + rng.normal(0, 0.17, (n, 69)), rng.normal(0, 0.17, (n, 6))], axis=1).astype(np.float32)
    if wrist_push:
        act[:, WRIST_X] = np.deg2rad(-45.0)
    return act


def _mixed_vs_oracle(mlib, pair, mode, solver, substeps=2, iterations=None, n=32, steps=2, **env):
    players, hands = PAIRS[pair]
    push = pair == "federer_djokovic"
    rng = np.random.default_rng({"ground": 2, "hit": 3, "body": 4}[mode] + 100 * substeps)
    task = make_pair_task(n, mlib, players, hands, sim_overrides={"substeps": substeps}, iterations=iterations, contact_solver=solver, **env)
    links = [g["racket_link"] for g in task.racket_geometries]
    assert links == [17 if p == "nadal" else 22 for p in players] and task.contact_solver == solver
    assert np.array_equal(task._env_shape_ids, np.arange(n) % 2)
    root, dpos, dvel = _prepare(task, rng, wrist_push=push)
    n_iter = task.sim_params.physx.num_position_iterations
    oracles = []
    for e in range(n):
        bm = task.body_shapes[e % 2]
        o = PhysOracle(bm, default_params(h=1.0 / (60.0 * substeps), joint_limits=1, solver_type={"pgs": 0, "tgs": 1}[solver], n_iter=n_iter),
                       kp=bm.kp.astype(np.float32), kd=bm.kd.astype(np.float32))
        o.set_state(root[e], dpos[e], dvel[e])
        o.attach_ball(task.racket_geometries[e % 2])
        oracles.append(o)
    task._rigid_body_state[:] = T(np.stack([o.get_state()[3] for o in oracles]).reshape(n * 24, 13))
    task._ball_root_states[:] = T(_launch(task, rng, mode))
    hits = np.zeros(n, dtype=int)
    deflected = 0
    has_hit = np.zeros(n, dtype=bool)
    for step in range(steps):
        act = _actions(task, rng, wrist_push=push)
        rb0 = N(task._rigid_body_state).reshape(n, 24, 13).copy()
        dpos_before = N(task._dof_pos).copy()
        ball_before = N(task._ball_root_states).copy()
        task.pre_physics_step(T(act))
        task._physics_step()
        torch.cuda.synchronize()
        pd = np.empty((n, 69), np.float32)
        force, torque = np.empty((n, 3), np.float32), np.empty((n, 3), np.float32)
        for k in range(2):  # (the PD clamp and the residual wrench with each player's gains)
            sel = np.arange(n) % 2 == k
            _, pdk, _, fk, tk = O.pre_physics(act[sel], N(task.reset_buf)[sel], dpos_before[sel], rb0[sel, 0, 3:7], task.body_shapes[k].kp.astype(np.float32))
            pd[sel], force[sel], torque[sel] = pdk, fk, tk
        ids_sub = N(task.debug_contacts_substeps())
        per_sim, hit, bc, rbs, ids, cf, bbf, cfs, sens, own, margin = [], [], [], [], [], [], [], [], [], [], []
        kw = dict(nsub=2 * substeps, hold=substeps, sub_per_sim=substeps)
        for e in range(n):
            o = oracles[e]
            o.set_ball(ball_before[e])
            sens.append(o.ball_sensitivity(pd_target=pd[e], ext_force=force[e], ext_torque=torque[e], seed=step, forced_ids=ids_sub[e], **kw))
            c, _, i, ps, h, b = o.step_ball(pd_target=pd[e], ext_force=force[e], ext_torque=torque[e], forced_ids=ids_sub[e], **kw)
            per_sim.append(ps); hit.append(h); bc.append(b); rbs.append(o.get_state()[3]); ids.append(i); cf.append(c); bbf.append(o.ball_body_force)
            cfs.append(o.contact_force_sum); own.append(o.own_ids); margin.append(o.margins)
        per_sim, hit, bc, rbs, ids, cf, bbf, cfs, own, margin = map(np.stack, (per_sim, hit, bc, rbs, ids, cf, bbf, cfs, own, margin))
        sens = {k: np.stack([s[k] for s in sens]) for k in sens[0]}
        assert np.array_equal(ids, ids_sub[:, -1])
        differ = (own != ids_sub).any(axis=-1)
        touching = (own >= 0).any(axis=-1) | (ids_sub >= 0).any(axis=-1)
        if differ.any():
            assert differ.sum() <= max(1, 0.01 * touching.sum()) and margin[differ].max() < TIE_TOL, "a selection difference is not a tie of the rule"
        what = "%s %s %s step %d" % (pair, mode, solver, step)
        got_ps = N(task._ball_states_per_sim)
        close(got_ps[..., 0:3], per_sim[..., 0:3], 2e-5, "ball pos " + what)
        qs = np.sign(np.sum(got_ps[..., 3:7] * per_sim[..., 3:7], -1, keepdims=True))
        close(got_ps[..., 3:7] * qs, per_sim[..., 3:7], 1e-4, "ball quat " + what, sens=sens["ball"][..., 3:7])
        close(got_ps[..., 7:10], per_sim[..., 7:10], 5e-4, "ball vel " + what, sens=sens["ball"][..., 7:10])
        close(got_ps[..., 10:13], per_sim[..., 10:13], 5e-4, "ball spin " + what, sens=sens["ball"][..., 10:13])
        assert np.array_equal(N(task._racket_ball_contact_per_sim), hit), "racket hit flags " + what
        now = (hit.any(axis=1) & ~has_hit) if substeps <= 2 else np.zeros(n, dtype=bool)
        has_hit |= now
        assert np.array_equal(N(task._has_racket_ball_contact_now), now) and np.array_equal(N(task._has_racket_ball_contact), has_hit)
        close(N(task._ball_contact_forces), bc, 2e-2, "contact forces on the ball " + what, sens=sens["bc"][:, 0:2])
        close(N(task._ball_body_contact_force), bbf, 2e-2, "ball x hull force " + what, sens=sens["bc"][:, 2])
        rb = N(task._rigid_body_state).reshape(n, 24, 13)
        close(rb[..., 0:3], rbs[..., 0:3], 2e-5, "rb pos " + what)
        close(rb[..., 7:13], rbs[..., 7:13], 1e-3, "rb vel " + what, sens=sens["rb"][..., 7:13])
        close(N(task._contact_forces), cf, 2e-2, "net contact forces " + what, sens=sens["cf"])
        close(N(task._contact_forces_sum), cfs, 2e-2, "_contact_forces_sum " + what, sens=sens["cfs"])
        # the racket rigid body = each env's OWN racket link moved by its player's weld offset
        rl = np.array([links[e % 2] for e in range(n)])
        wr = rbs[np.arange(n), rl]
        off = np.einsum("nij,nj->ni", Rotation.from_quat(wr[:, 3:7]).as_matrix(), np.stack([task.racket_geometries[e % 2]["racket_offset"] for e in range(n)]))
        close(N(task._racket_rb_state)[:, 0:3], wr[:, 0:3] + off, 2e-5, "racket pos " + what)
        close(N(task._racket_rb_state)[:, 7:10], wr[:, 7:10] + np.cross(wr[:, 10:13], off), 1e-3, "racket vel " + what)
        hits += hit.sum(1)
        after = got_ps[:, -1]
        deflected += int(((np.linalg.norm(after[:, 7:10] - ball_before[:, 7:10], axis=1) > 3.0) & (after[:, 2] > 0.2) & (ball_before[:, 2] > 0.2)).sum())
        task.post_physics_step()
    if push:
        wx = N(task._dof_pos)[:, WRIST_X]
        assert (wx[1::2] > np.deg2rad(-10.0) - 0.03).all(), "the Djokovic envs stop at their R_Wrist_x limit: %s" % np.rad2deg(wx[1::2].min())
        assert (wx[0::2] < np.deg2rad(-12.0)).sum() >= n // 4, "the Federer envs turn past -10 deg: %s" % np.rad2deg(np.sort(wx[0::2])[:4])
    if mode == "hit":
        if substeps <= 2:
            for k in range(2):
                assert hits[k::2].sum() >= 2, "player %s must get racket hits (%s)" % (players[k], hits[k::2])
        else:  # (the per-call flag looks at the call's LAST substep: one in six here) - balls deflected clear of the ground instead
            assert deflected >= n // 8, "the fixture must produce racket hits (%d balls deflected)" % deflected
    task.close()


@pytest.mark.parametrize("solver", ["pgs", "tgs"])
@pytest.mark.parametrize("mode", ["hit", "body", "ground"])
@pytest.mark.parametrize("pair", ["nadal_federer", "federer_djokovic"])
def test_mixed_batch_matches_each_players_oracle(mlib, pair, mode, solver):
    _mixed_vs_oracle(mlib, pair, mode, solver)


@pytest.mark.parametrize("solver", ["pgs", "tgs"])
@pytest.mark.parametrize("mode", ["hit", "ground"])
@pytest.mark.parametrize("pair", ["nadal_federer", "federer_djokovic"])
def test_mixed_batch_with_the_controller_substeps(mlib, pair, mode, solver):
    """The controller configs' sim block: 6 substeps per simulate() call, num_position_iterations 2."""
    _mixed_vs_oracle(mlib, pair, mode, solver, substeps=6, iterations=2)


@pytest.mark.parametrize("solver", ["pgs", "tgs"])
@pytest.mark.parametrize("mode", ["hit", "body"])
@pytest.mark.parametrize("pair", ["nadal_federer", "federer_djokovic"])
def test_mixed_batch_with_the_lds_parked_build(mlib, pair, mode, solver):
    _mixed_vs_oracle(mlib, pair, mode, solver, kernel_build=1)


def test_left_hand_hits_in_a_mixed_batch(mlib):
    """nadal_federer: a ball served at each env's own racket.  The Nadal envs (even) hit with the racket on L_Wrist: their hit flags, the
    racket's force on the ball and the racket rigid body all come from link 17."""
    n = 32
    rng = np.random.default_rng(31)
    task = make_pair_task(n, mlib, ["nadal", "federer"], [False, True], contact_solver="tgs")
    assert task._lefthand == 0 and task.racket_players == ["nadal", "federer"]
    assert task.racket_geometry is task.racket_geometries[0] and task.racket_geometry["player"] == "nadal"
    assert task._racket_wrist_body_id.dtype == torch.long and task._racket_wrist_body_id.shape == (n,)
    assert (N(task._racket_wrist_body_id) == np.where(np.arange(n) % 2 == 0, 17, 22)).all()
    _prepare(task, rng)
    task._ball_root_states[:] = T(_launch(task, rng, "hit"))
    seen_force = np.zeros(n, dtype=bool)
    for _ in range(2):
        task.step(T(_actions(task, rng)))
        torch.cuda.synchronize()
        seen_force |= np.linalg.norm(N(task._ball_contact_forces)[:, 0], axis=1) > 0
        rb = N(task._rigid_body_state).reshape(n, 24, 13)
        for k, link in ((0, 17), (1, 22)):
            w = rb[k::2, link]
            off = np.einsum("nij,j->ni", Rotation.from_quat(w[:, 3:7]).as_matrix(), task.racket_geometries[k]["racket_offset"])
            close(N(task._racket_rb_state)[k::2, 0:3], w[:, 0:3] + off, 2e-5, "racket pos, player %d" % k)
            assert np.array_equal(N(task._racket_rb_state)[k::2, 3:7], w[:, 3:7])
    hit = N(task._has_racket_ball_contact)
    assert hit[0::2].sum() >= n // 8, "Nadal envs must register racket hits: %s" % hit[0::2]
    assert seen_force[0::2].sum() >= 1, "a non-zero racket force on the ball in a Nadal env"
    assert hit[1::2].sum() >= n // 8
    task.close()


SNAP = ["_rigid_body_state", "_dof_state", "_contact_forces", "dof_force_tensor", "_humanoid_root_states", "_ball_root_states", "_ball_states_per_sim",
        "_racket_rb_state", "_racket_ball_contact_per_sim", "_has_bounce", "_has_bounce_now", "_bounce_pos", "_has_racket_ball_contact",
        "_has_racket_ball_contact_now", "_ball_contact_forces", "_ball_body_contact_force", "_contact_forces_sum"]


def _snap(task):
    n = task.num_envs
    return [N(getattr(task, k)).reshape(n, -1).copy() for k in SNAP]


def test_mixed_equals_homogeneous_batches(mlib):
    """The same states, actions and balls through a nadal_federer batch and through [nadal, nadal] / [federer, federer] batches (two shapes
    as well: the same kernel instantiation): every env's tensors are the same bits as in the batch of its own player."""
    n, steps = 32, 4
    rng = np.random.default_rng(77)
    mixed = make_pair_task(n, mlib, ["nadal", "federer"], contact_solver="tgs", debug_contacts=0)
    times = rng.uniform(0.1, 1.0, size=n)
    mixed.reset_with_times(None, T(times))
    ball = _launch(mixed, rng, "hit")
    ball[2::4] = _launch(mixed, rng, "body")[2::4]
    acts = [_actions(mixed, rng) for _ in range(steps)]
    runs = {}
    for name, players in (("mixed", None), ("nadal", ["nadal", "nadal"]), ("federer", ["federer", "federer"])):
        task = mixed if players is None else make_pair_task(n, mlib, players, contact_solver="tgs", debug_contacts=0)
        assert len(task.body_shapes) == 2
        if players is not None:
            task.reset_with_times(None, T(times))
        task._ball_root_states[:] = T(ball)
        snaps = []
        for a in acts:
            task.pre_physics_step(T(a))
            task._physics_step()
            torch.cuda.synchronize()
            snaps.append(_snap(task))
            task.post_physics_step()
        runs[name] = snaps
        task.close()
    hits = 0
    for k in range(steps):
        for j, key in enumerate(SNAP):
            got = runs["mixed"][k][j]
            for p, name in ((0, "nadal"), (1, "federer")):
                want = runs[name][k][j]
                assert np.array_equal(got[p::2], want[p::2]), "step %d, %s of the %s envs: %d values differ" % (k, key, name, int((got[p::2] != want[p::2]).sum()))
        hits += int(runs["mixed"][k][SNAP.index("_racket_ball_contact_per_sim")].sum())
    assert hits >= 4, "the fixture must produce racket hits (%d)" % hits
    assert np.abs(runs["nadal"][-1][0][1::2] - runs["federer"][-1][0][1::2]).max() > 0, "the players differ"


@pytest.mark.parametrize("n", [258, 8192])
def test_substep_jobs_are_invisible_with_mixed_players(mlib, n):
    outs = []
    for jobs in (False, True):
        task = make_pair_task(n, mlib, ["nadal", "federer"], contact_solver="tgs", substep_jobs=2 * int(jobs), debug_contacts=0)
        g = torch.Generator(device=DEV)
        g.manual_seed(23)
        task.reset_with_times(None, torch.rand(n, device=DEV, generator=g) * 0.8)
        root = task._humanoid_root_states[:, 0:3]
        jit = torch.rand((n, 3), device=DEV, generator=g)
        task.reset_balls(torch.arange(n, device=DEV), root + torch.tensor([2.5, 0.0, 0.3], device=DEV) + jit * 0.6,
                         torch.tensor([-20.0, 0.0, 1.0], device=DEV) + (jit - 0.5) * torch.tensor([6.0, 4.0, 4.0], device=DEV),
                         torch.tensor([0.0, -120.0, 0.0], device=DEV).expand(n, 3))
        snaps = []
        for _ in range(6):
            a = torch.cat([task._target_dof_pos + 0.4 * torch.randn((n, 69), device=DEV, generator=g), 0.3 * torch.randn((n, 6), device=DEV, generator=g)], dim=1).contiguous()
            task.step(a)
            snaps.append(_snap(task) + [N(task.rew_buf).copy(), N(task.reset_buf).copy()])
        task.check()
        outs.append(snaps)
        task.close()
    assert any(s[SNAP.index("_racket_ball_contact_per_sim")].any() for s in outs[0]), "the fixture must produce racket hits"
    for k, (sa, sb) in enumerate(zip(*outs)):
        for j, (x, y) in enumerate(zip(sa, sb)):
            assert np.array_equal(x, y), "step %d, tensor %d: %d of %d values differ" % (k, j, int((x != y).sum()), x.size)


def test_setter_refusals_leave_the_batch_as_it_was(mlib):
    from vid2player3d_amd import _lib, racket
    from vid2player3d_amd.model import load_baked_model
    from vid2player3d_amd.tasks import HumanoidSMPLIM, default_cfg
    from vid2player3d_amd.tasks.humanoid_racket_ball import racket_geom_struct

    n = 32
    outs = []
    for refuse in (False, True):
        task = make_pair_task(n, mlib, ["nadal", "federer"], contact_solver="tgs", debug_contacts=0)
        L = task._lib
        if refuse:
            good = [racket_geom_struct(g) for g in task.racket_geometries]
            cases = []
            for count in (1, 3):
                arr = (_lib.RacketGeom * count)(*[good[k % 2] for k in range(count)])
                cases.append((arr, count, "racket"))
            for field, val in (("racket_link", 0), ("racket_link", 24), ("num_cylinders", 3)):
                arr = (_lib.RacketGeom * 2)(*good)
                setattr(arr[1], field, val)
                cases.append((arr, 2, field))
            for arr, count, what in cases:
                assert L.v2p_env_set_racket_shapes(task._h_env, arr, count) == -1, what
                assert what.encode() in L.v2p_last_error(), L.v2p_last_error()
        g = torch.Generator(device=DEV)
        g.manual_seed(3)
        task.reset_with_times(None, torch.rand(n, device=DEV, generator=g) * 0.8)
        task._ball_root_states[:] = T(_launch(task, np.random.default_rng(3), "hit"))
        for _ in range(2):
            task.step(torch.cat([task._target_dof_pos + 0.3 * torch.randn((n, 69), device=DEV, generator=g), torch.zeros((n, 6), device=DEV)], dim=1).contiguous())
        outs.append(_snap(task))
        task.close()
    for j, (x, y) in enumerate(zip(*outs)):
        assert np.array_equal(x, y), SNAP[j]
    # before v2p_env_attach_ball: a two-shape batch without a ball
    base = load_baked_model()
    shapes = [racket.with_racket(base, player=p)[0] for p in ("nadal", "federer")]
    cfg = default_cfg(n, motion_lib=mlib, sample_first_motions=True, body_shape_mismatch="ignore", body_model=shapes, motion_shape_ids=np.arange(8) % 2)
    task = HumanoidSMPLIM(cfg, device_type="cuda", device_id=0)
    task.reset_with_times(None, torch.full((n,), 0.3, device=DEV))
    geoms = (_lib.RacketGeom * 2)(*[racket_geom_struct(racket.with_racket(base, player=p)[1]) for p in ("nadal", "federer")])
    assert task._lib.v2p_env_set_racket_shapes(task._h_env, geoms, 2) == -1
    assert b"attach_ball" in task._lib.v2p_last_error()
    task.step(torch.cat([task._target_dof_pos, torch.zeros((n, 6), device=DEV)], dim=1).contiguous())
    torch.cuda.synchronize()
    assert torch.isfinite(task._rigid_body_state).all()
    task.close()
