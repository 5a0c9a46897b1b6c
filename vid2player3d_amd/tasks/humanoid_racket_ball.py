"""The imitation task with vid2player's racket and ball in the simulation (BASELINE config 4's "racket+ball contacts").

`vid2player/env/tasks/humanoid_smpl_im_mvae.py` puts two actors in every env: the SMPL humanoid with a racket welded to the right
wrist (`smpl_mesh_humanoid_djokovic.xml:188-190`) and a free tennis ball (`tennis_ball.urdf`), applies the aerodynamic force of
`apply_external_force_to_ball` (:711-739) before every `simulate()` call and polls the net contact forces after it (:752-783).  What
this class takes from it is that PHYSICS: the observation / reward / MVAE machinery of the vid2player task is out of scope,
the task logic stays the imitation task's (`HumanoidSMPLIM`).  Exposed like the reference's tensors:

    _ball_root_states [N,13]     the ball actor's root state; write it (+ nothing else) to launch a ball, as `_reset_balls` does (:503-522)
    _racket_rb_state  [N,13]     rigid body 24
    _ball_states_per_sim [N,2,13], _racket_ball_contact_per_sim [N,2]   what the reference sees after each of the 2 simulate() calls
    _has_bounce / _has_bounce_now / _bounce_pos, _has_racket_ball_contact(_now)   the flags of :731-737 and :773-779, same rules
    _contact_forces_sum [N,24,3]  net contact forces summed over the simulate() calls of a control step (:781)
"""
import ctypes as C

import numpy as np
import torch

from .. import _lib, racket
from ..model import load_baked_model
from .humanoid_smpl_im import HumanoidSMPLIM

BALL_R = racket.BALL["radius"]


def pair_players(v2p, env):
    """The two players of cfg_v2p `dual_mode: different` (names of racket.PLAYERS): `player: [p0, p1]`, or - names absent - `righthand:
    [r0, r1]`, each entry djokovic (True) or nadal (False) like the single-player path.  Given both, they must agree."""
    if int(env["numEnvs"]) % 2:
        raise ValueError("dual_mode 'different' alternates the two players over the envs (env i = player i %% 2): numEnvs must be even, got %d" % int(env["numEnvs"]))
    if "player" in env:
        raise ValueError("cfg env.player selects ONE player; with dual_mode 'different' the pair comes from v2p.player / v2p.righthand")
    names, hands = v2p.get("player"), v2p.get("righthand")
    for key, val in (("player", names), ("righthand", hands)):
        if val is not None and (isinstance(val, (str, bool)) or len(val) != 2):
            raise ValueError("dual_mode 'different': v2p.%s must be a list of 2 entries (one per player), got %r" % (key, val))
    if names is None:
        if hands is None:
            raise ValueError("dual_mode 'different' needs v2p.player = [p0, p1] or v2p.righthand = [r0, r1]")
        names = ["djokovic" if bool(r) else "nadal" for r in hands]
    names = [str(p) for p in names]
    for p in names:
        if p not in racket.PLAYERS:
            raise ValueError("unknown player %r (known: %s)" % (p, ", ".join(sorted(racket.PLAYERS))))
    if hands is not None:
        for p, r in zip(names, hands):
            if bool(r) != (racket.PLAYERS[p]["parent"] == "R_Wrist"):
                raise ValueError("v2p.righthand %r disagrees with player %s" % (list(hands), p))
    return names


def _fill_racket(dst, g):
    """cylinders / racket_offset / (racket_link, num_cylinders) of a racket geometry dict into a BallCfg or a RacketGeom."""
    dst.racket_link, dst.num_cylinders = int(g["racket_link"]), len(g["cylinders"])
    for k, cy in enumerate(g["cylinders"]):
        dst.cylinders[k][:] = [float(x) for x in list(cy["center"]) + list(cy["axis"]) + [cy["half_len"], cy["radius"]]]
    dst.racket_offset[:] = [float(x) for x in g["racket_offset"]]


def racket_geom_struct(g):
    r = _lib.RacketGeom()
    _fill_racket(r, g)
    return r


class HumanoidSMPLIMRacketBall(HumanoidSMPLIM):
    def __init__(self, cfg, sim_params=None, physics_engine=None, device_type="cuda", device_id=0, headless=True):
        # (work on a copy: the caller's cfg stays what it was, a second task built from it starts from the plain body model again)
        cfg = dict(cfg)
        env = cfg["env"] = dict(cfg["env"])
        base = env.get("body_model") or load_baked_model(default_humanoid_mass=env.get("default_humanoid_mass", 90.0), kp_scale=env.get("kp_scale", 1.0),
                                                         kd_scale=env.get("kd_scale", env.get("kp_scale", 1.0)))
        if env.get("has_racket_collision", False):
            # (humanoid_smpl_im_mvae.py:42, 397-401: racket shapes with collision filter 0 = the racket collides with the links of its own
            # humanoid; default False in every config)
            raise NotImplementedError("has_racket_collision=True (racket x link contacts) is not built; the reference default is False")
        # the player asset: djokovic / federer (right hand) or nadal (left hand); cfg_v2p righthand = False selects the left-handed one
        # like the reference (humanoid_smpl_im_mvae.py:73-78).  The exposed rigid-body order is the canonical one either way (racket =
        # rigid body 24: the reference permutes the left-handed asset's tensor into it, :67, 197-201).
        v2p = dict(cfg.get("v2p") or {})
        # two players (the match configs nadal_federer.yaml / federer_djokovic.yaml: dual_mode `different`): env i is player i % 2
        # (humanoid_smpl_im_mvae.py:255-270, [::2] / [1::2]), each with its own asset - racket hand and arm ranges folded into one body
        # shape per player; other dual_mode values share one asset in the reference and take the single-player path
        self.racket_players = pair_players(v2p, env) if v2p.get("dual_mode") == "different" else None
        if self.racket_players is not None:
            if isinstance(base, (list, tuple)):
                raise NotImplementedError("dual_mode 'different' with per-clip body shapes (a body_model list) is not built: give one BodyModel, "
                                          "or v2p.player_body_models = [BodyModel, BodyModel] for the two players")
            bases = v2p.get("player_body_models") or [base, base]
            if len(bases) != 2:
                raise ValueError("v2p.player_body_models must hold 2 body models (one per player), got %d" % len(bases))
            # (two shapes even for two equal players: the batch runs the per-env-shape kernel either way)
            folded = [racket.with_racket(b, player=p) for b, p in zip(bases, self.racket_players)]
            model, self.racket_geometries = [m for m, _ in folded], [g for _, g in folded]
        else:
            player = env.get("player", "djokovic" if v2p.get("righthand", True) else "nadal")
            if isinstance(base, (list, tuple)):
                # one body shape per clip: the racket is the same object in every hand - welded at the same offset of the wrist frame - so
                # every shape gets it folded in, and the ball's cylinders (given in the wrist frame) are shared
                folded = [racket.with_racket(b, player=player) for b in base]
                model, self.racket_geometries = [m for m, _ in folded], [folded[0][1]]
            else:
                model, geom = racket.with_racket(base, player=player)
                self.racket_geometries = [geom]
        self.racket_geometry = self.racket_geometries[0]  # (player 0's)
        env["body_model"] = model
        # the player MJCF's racket-arm ranges (R_Wrist +-10 / +-45 / +-90 deg, R_Elbow_x <= 90 deg) are enforced like Isaac Gym does
        env.setdefault("joint_limits", True)
        # (the solver is the one the files name: vid2player/cfg/im/tennis_im.yaml:39, embodied_pose/cfg/djokovic_im.yaml:41 state
        # `solver_type: 1`, TGS - the racket-arm limit rows and the ball's rows are solved inside its slices like the hull rows;
        # `env.contact_solver` overrides as in the base task)
        self.cfg_v2p = dict(cfg.get("v2p") or {})
        super().__init__(cfg, sim_params, physics_engine, device_type, device_id, headless)
        n, dev = self.num_envs, self.device
        nsim = self.control_freq_inv
        B = self._buffer  # (guard rows under cfg env debug_guard_rows, like the base task's buffers)
        self._ball_root_states = B("_ball_root_states", (n, 13))
        self._ball_root_states[:, 2] = 1.0   # start_pose of the ball actor (:430-431)
        self._ball_root_states[:, 6] = 1.0
        self._racket_rb_state = B("_racket_rb_state", (n, 13))
        self._ball_states_per_sim = B("_ball_states_per_sim", (n, nsim, 13))
        self._racket_ball_contact_per_sim = B("_racket_ball_contact_per_sim", (n, nsim), torch.int32)
        self._ball_contact_forces = B("_ball_contact_forces", (n, 2, 3))
        self._ball_body_contact_force = B("_ball_body_contact_force", (n, 3))  # on the ball from the humanoid's links (ball x hull contacts)
        # `_contact_forces_sum` (:186, 690, 781): net contact forces of the links after each simulate() call, summed over the control step
        # (opt-in, cfg env contact_forces_sum: nothing in the reference reads it, and keeping it costs the launch 2 %)
        self._contact_forces_sum = B("_contact_forces_sum", (n, 24, 3)) if env.get("contact_forces_sum", False) else None
        self._has_bounce = B("_has_bounce", (n,), torch.bool)
        self._has_bounce_now = B("_has_bounce_now", (n,), torch.bool)
        self._bounce_pos = B("_bounce_pos", (n, 3))
        self._has_racket_ball_contact = B("_has_racket_ball_contact", (n,), torch.bool)
        self._has_racket_ball_contact_now = B("_has_racket_ball_contact_now", (n,), torch.bool)
        mat = dict(racket.BALL_MATERIAL)
        if "restitution" in self.cfg_v2p:  # cfg_v2p.restitution sets ball AND racket head (:414, :436); the plane keeps 0
            mat["rest_ground"], mat["rest_racket"] = 0.5 * self.cfg_v2p["restitution"], self.cfg_v2p["restitution"]
            mat["rest_body"] = 0.5 * self.cfg_v2p["restitution"]  # ball x a link's hull: the humanoid's shapes keep restitution 0
        if "ball_friction" in self.cfg_v2p or "racket_friction" in self.cfg_v2p:
            bf, rf = self.cfg_v2p.get("ball_friction", 0.8), self.cfg_v2p.get("racket_friction", 0.8)
            mat["fric_ground"], mat["fric_racket"], mat["fric_body"] = 0.5 * (bf + 1.0), 0.5 * (bf + rf), 0.5 * (bf + 1.0)
        g = self.racket_geometry
        c = _lib.BallCfg(radius=racket.BALL["radius"], mass=racket.BALL["mass"], inertia=racket.BALL["inertia"],
                         restitution_ground=mat["rest_ground"], friction_ground=mat["fric_ground"], restitution_racket=mat["rest_racket"],
                         friction_racket=mat["fric_racket"], bounce_threshold_velocity=self.sim_params.physx.bounce_threshold_velocity,
                         angular_damping=mat["ang_damp"], max_angular_velocity=mat["max_ang_vel"], spin_scale=self.cfg_v2p.get("spin_scale", 1.0),
                         restitution_body=mat["rest_body"], friction_body=mat["fric_body"], body_contacts=int(env.get("ball_body_contacts", True)),
                         bounce_height=BALL_R * (6 if self.sim_params.substeps > 2 else 4), poll_racket_hits=int(self.sim_params.substeps <= 2))
        _fill_racket(c, g)
        self._ball_cfg = c
        self._attach_ball()
        # the reference's per-env racket attributes (humanoid_smpl_im_mvae.py:68-82): the link the racket is welded to, and which player of
        # a pair is left-handed (-1: the single player is; None: no left hand)
        links = [g["racket_link"] for g in self.racket_geometries]
        if self.racket_players is None:
            self._racket_wrist_body_id = links[0]
            self._lefthand = -1 if racket.PLAYERS[self.racket_geometry["player"]]["parent"] == "L_Wrist" else None
        else:
            self._racket_wrist_body_id = torch.tensor(links, dtype=torch.long, device=dev).repeat(n // 2)
            left = [racket.PLAYERS[p]["parent"] == "L_Wrist" for p in self.racket_players]
            self._lefthand = left.index(True) if any(left) else None
        self.ball_material = mat
        # the ball generator (humanoid_smpl_im_mvae.py:121-130), opt-in: a pool file under cfg_v2p.ball_traj_file (ball_traj_file_test when
        # neither training nor test_mode 'random'), or a generator object under cfg_v2p.ball_generator; without either key reset_balls
        # takes the launch state from the caller as before.  Two departures from :121-130: the reference reads the task's own _is_train, here
        # it is a key of its own, cfg_v2p.is_train (default true); and the reference builds no generator under dual_mode, here a
        # two-player task that names a pool file gets one too
        self._ball_generator = self.cfg_v2p.get("ball_generator")
        if self._ball_generator is None and "ball_traj_file" in self.cfg_v2p:
            from ..ball_traj import TennisBallGeneratorOffline

            random_rows = bool(self.cfg_v2p.get("is_train", True)) or self.cfg_v2p.get("test_mode", "random") == "random"
            self._ball_generator = TennisBallGeneratorOffline(self.cfg_v2p["ball_traj_file" if random_rows else "ball_traj_file_test"], sample_random=random_rows,
                                                              num_envs=n, device=dev)

    def _attach_ball(self):
        """v2p_env_attach_ball with the task's buffers as they stand (a second call keeps the batch's ball and replaces its parameters and
        buffers; the engine allocates its per-call partial sums of the links' contact forces the first time `_contact_forces_sum` is given)."""
        b = _lib.BallBuffers(ball_state=self._ball_root_states.data_ptr(), racket_state=self._racket_rb_state.data_ptr(),
                             ball_per_sim=self._ball_states_per_sim.data_ptr(), racket_hit_per_sim=self._racket_ball_contact_per_sim.data_ptr(),
                             ball_contact=self._ball_contact_forces.data_ptr(), ball_body_contact=self._ball_body_contact_force.data_ptr(),
                             has_bounce=self._has_bounce.data_ptr(), has_bounce_now=self._has_bounce_now.data_ptr(), bounce_pos=self._bounce_pos.data_ptr(),
                             has_racket_contact=self._has_racket_ball_contact.data_ptr(), has_racket_contact_now=self._has_racket_ball_contact_now.data_ptr(),
                             contact_force_sum=None if self._contact_forces_sum is None else self._contact_forces_sum.data_ptr())
        _lib.check(self._lib.v2p_env_attach_ball(self._h_env, C.byref(self._ball_cfg), C.byref(b)), "v2p_env_attach_ball")
        if self.racket_players is not None:
            geoms = (_lib.RacketGeom * 2)(*[racket_geom_struct(g) for g in self.racket_geometries])
            _lib.check(self._lib.v2p_env_set_racket_shapes(self._h_env, geoms, 2), "v2p_env_set_racket_shapes")

    # ------------------------------------------------------------------ two players: shapes by env, not by clip
    def _env_body_shapes(self, env):
        if self.racket_players is None:
            return super()._env_body_shapes(env)
        return (np.arange(self.num_envs) % 2).astype(np.int32)

    def _players_share_the_clips(self, fn, env):
        # the motion library is built for (and checked against) player 0's skeleton, never clip by clip for the two player shapes
        shapes, self.body_shapes = self.body_shapes, None
        try:
            return fn(env)
        finally:
            self.body_shapes = shapes

    def _load_motion(self, env):
        if self.racket_players is None:
            return super()._load_motion(env)
        return self._players_share_the_clips(super()._load_motion, env)

    def _check_body_shapes(self, env):
        if self.racket_players is None:
            return super()._check_body_shapes(env)
        return self._players_share_the_clips(super()._check_body_shapes, env)

    # ------------------------------------------------------------------ the reference's flag bookkeeping around the physics step
    def reset_balls(self, env_ids, launch_pos=None, launch_vel=None, launch_ang_vel=None):
        """`_reset_balls` (:503-524).  With a launch state given by the caller it is written as it is; without one it is drawn from the
        task's ball generator (cfg_v2p.ball_traj_file / ball_generator) as the reference does - `generate(len(env_ids),
        need_init_state=True, start_pos=ball positions, env_ids=env_ids)`, spin axis from the launch velocity (:508-509) - and the drawn
        trajectories [len(env_ids),frames,3] are returned."""
        ids = torch.as_tensor(env_ids, device=self.device, dtype=torch.long)
        traj = None
        if launch_pos is None:
            if self._ball_generator is None:
                raise RuntimeError("reset_balls without a launch state needs cfg_v2p.ball_traj_file or cfg_v2p.ball_generator")
            from ..ball_traj import launch_ang_vel as spin_axis

            traj, launch_pos, launch_vel, vspin = self._ball_generator.generate(len(ids), need_init_state=True, start_pos=self._ball_root_states[ids, 0:3], env_ids=ids)
            launch_pos, launch_vel = launch_pos.to(self.device), launch_vel.to(self.device)
            launch_ang_vel = spin_axis(launch_vel, vspin.to(self.device))
        self._ball_root_states[ids, 0:3] = launch_pos
        self._ball_root_states[ids, 3:7] = torch.tensor([0.0, 0.0, 0.0, 1.0], device=self.device)
        self._ball_root_states[ids, 7:10] = launch_vel
        self._ball_root_states[ids, 10:13] = launch_ang_vel
        self._has_bounce[ids] = False
        self._bounce_pos[ids] = 0
        self._has_racket_ball_contact[ids] = False
        return traj

    # The reference's flag bookkeeping around every simulate() call - the bounce test on the ball height at the START of the call
    # (apply_external_force_to_ball, :731-737: threshold 4 ball radii, 6 with more than 2 substeps) and the contact-force poll after it
    # (:773-779, only with sim.substeps <= 2) - runs inside the physics launch: the flag tensors above are the buffers it writes.
