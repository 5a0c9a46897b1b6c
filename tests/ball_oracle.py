"""The float64 oracle's side of the free-ball tests (helpers, no tests): trajectories of balls without racket and humanoid, the
reference's bookkeeping around them, their conditioning under launch perturbations of float32-rounding size, and the numpy statement of
the back-spin rule that the oracle's aerodynamic call does not have.

A ball of the oracle lives next to a humanoid (PhysOracle): it is parked 50 m away with `body_contacts=False`, so nothing of it reaches
the ball.  One instance per trajectory; the runs of a fixture go through a thread pool (ctypes releases the GIL)."""
import math
from concurrent.futures import ThreadPoolExecutor

import numpy as np

from oracle.phys_oracle import PhysOracle, ball_aero, default_params
from vid2player3d_amd.model import load_baked_model

K_SENS = 16.0
EPS_POS, EPS_VEL, TRIALS = 2e-7, 1e-6, 8   # PhysOracle.ball_sensitivity's perturbation sizes; trials per launch
THREADS = 16
_BM = None


def body_model():
    global _BM
    if _BM is None:
        _BM = load_baked_model()
    return _BM


def launch_state(pos, vel, vspin):
    """Ball root state [13] of a launch: spin axis normalize(vel x (0,0,-1)) (utils/tennis_ball.py:135-136), in float64."""
    s = np.zeros(13)
    s[0:3], s[6], s[7:10] = pos, 1.0, vel
    c = np.cross(np.asarray(vel, dtype=np.float64), [0.0, 0.0, -1.0])
    s[10:13] = float(vspin) * 2 * math.pi * c / max(np.linalg.norm(c), 1e-12)
    return s


def make_oracle(cfg):
    bm = body_model()
    p = default_params(h=cfg["sim_dt"] / cfg["substeps"], n_iter=cfg["num_iterations"], solver_type=cfg["solver_type"], gravity_z=cfg["gravity_z"],
                       contact_offset=cfg["contact_offset"], erp=cfg["erp"], max_depen_vel=cfg["max_depenetration_velocity"])
    o = PhysOracle(bm, p, kp=bm.kp.astype(np.float32), kd=bm.kd.astype(np.float32))
    root = np.zeros(13)
    root[0:3], root[6] = [50.0, 50.0, 0.95], 1.0
    o.set_state(root, np.zeros(69), np.zeros(69))
    o.attach_ball(None, ball={"radius": cfg["radius"], "mass": cfg["mass"], "inertia": cfg["inertia"]},
                  material={"rest_ground": cfg["restitution_ground"], "fric_ground": cfg["friction_ground"], "bounce_threshold": cfg["bounce_threshold_velocity"],
                            "ang_damp": cfg["angular_damping"], "max_ang_vel": cfg["max_angular_velocity"]},
                  spin_scale=cfg["spin_scale"], body_contacts=False)
    return o


def run(cfg, state13, frames):
    """Per-call ball states [frames * cfi + 1, 13] of one launch: the launch state, then the state after every simulate() call."""
    o = make_oracle(cfg)
    o.set_ball(state13)
    sub, cfi = cfg["substeps"], cfg["control_freq_inv"]
    out = [np.asarray(state13, dtype=np.float64)]
    for _ in range(frames):
        ps = o.step_ball(nsub=cfi * sub, hold=0, sub_per_sim=sub)[3]
        out.extend(ps)
    return np.stack(out)


def rollouts(cfg, states, frames, trials=TRIALS, seed=0):
    """(calls [n, frames * cfi + 1, 13], sens of the same shape): the oracle's trajectories of the launch states [n,13] and the largest
    change of each element over `trials` runs whose launch is perturbed at float32-rounding size."""
    states = np.asarray(states, dtype=np.float64)
    rng = np.random.default_rng(seed)
    jobs = []
    for s in states:
        jobs.append(s)
        for _ in range(trials):
            p = s.copy()
            p[0:3] += EPS_POS * rng.normal(size=3)
            p[7:13] += EPS_VEL * rng.normal(size=6) * np.array([1, 1, 1, 30, 30, 30])  # (spins are tens of rad/s: one float32 ulp is larger there)
            jobs.append(p)
    with ThreadPoolExecutor(THREADS) as ex:
        res = list(ex.map(lambda s: run(cfg, s, frames), jobs))
    res = np.stack(res).reshape(len(states), trials + 1, -1, 13)
    return res[:, 0], np.abs(res[:, 1:] - res[:, :1]).max(axis=1) if trials else np.zeros_like(res[:, 0])


def bookkeeping(cfg, calls, frames):
    """`simulate`'s bookkeeping (utils/tennis_ball.py:167-187) on per-call states [S,13] of ONE ball: dict with bounce_pos, bounce_idx,
    pass_net, and `margin` = the smallest distance of a deciding quantity from its threshold (z against bounce_height up to the
    detection, y against 0 up to the crossing, z against net_height at the crossing)."""
    cfi = cfg["control_freq_inv"]
    has_bounce = has_pass = pass_ok = False
    bpos, bidx, margin = np.zeros(3), frames - 1, np.inf
    for t in range(frames):
        for i in range(cfi):
            p = calls[t * cfi + i, 0:3]
            if not has_pass:
                margin = min(margin, abs(p[1]))
                if p[1] < 0:
                    has_pass, pass_ok = True, (not has_bounce) and p[2] > cfg["net_height"]
                    margin = min(margin, abs(p[2] - cfg["net_height"]))
            if not has_bounce:
                margin = min(margin, abs(p[2] - cfg["bounce_height"]))
                if p[2] <= cfg["bounce_height"]:
                    has_bounce, bpos, bidx = True, p.copy(), t
    return {"bounce_pos": bpos, "bounce_idx": bidx, "pass_net": pass_ok, "margin": margin}


def first_contact_call(cfg, calls):
    """Index of the first simulate() call during which the ball x ground rows can become active (conservative: the gap at its start is
    within what the ball can close in the call), len(calls) if none."""
    gap = calls[:, 2] - cfg["radius"]
    reach = cfg["contact_offset"] + cfg["sim_dt"] * (np.maximum(0.0, -calls[:, 9]) + abs(cfg["gravity_z"]) * cfg["sim_dt"])
    hit = np.nonzero(gap <= reach)[0]
    return int(hit[0]) if len(hit) else len(calls)


def backspin_flight(cfg, state13, calls):
    """Numpy statement of the spin-sign rule (utils/tennis_ball.py:163-176) for a launch with NEGATIVE spin in free flight: the spin fed
    to the lift coefficient is -|w| / 2 pi, so the lift of the oracle's aerodynamic call (which knows non-negative spins only) flips and
    its coefficient becomes 1 / (2 + |v / (-spin x scale + 1e-6)|).  Per-call states [calls + 1, 13]: v* = v + h (g + F / m), angular
    damping, x += h v, substep by substep, F held over a call.  No ground."""
    s = np.asarray(state13, dtype=np.float64).copy()
    h, sub = cfg["sim_dt"] / cfg["substeps"], cfg["substeps"]
    kf, cd = 1.21 * math.pi * 0.032 ** 2 / 2.0, 0.55
    out = [s.copy()]
    for _ in range(calls):
        v = s[7:10]
        vs = np.linalg.norm(v) or 1.0
        drag = -kf * cd * vs * v
        lift = ball_aero(s, cfg["spin_scale"]) - drag          # the oracle's lift for spin +|w|
        spin = np.linalg.norm(s[10:13]) / (2 * math.pi)
        cl_pos = 1.0 / (2.0 + abs(vs / (spin * cfg["spin_scale"] + 1e-6)))
        cl_neg = 1.0 / (2.0 + abs(vs / (-spin * cfg["spin_scale"] + 1e-6)))
        F = drag - lift * (cl_neg / cl_pos)
        for _ in range(sub):
            s[7:10] = s[7:10] + h * (np.array([0.0, 0.0, cfg["gravity_z"]]) + F / cfg["mass"])
            s[10:13] = s[10:13] / (1.0 + h * cfg["angular_damping"])
            s[0:3] = s[0:3] + h * s[7:10]
        out.append(s.copy())
    return np.stack(out)


# Flat terms (x max(1, max |reference|), as gpu_util.close scales them).  POS_FLAT: 4 x the largest position error before the first
# ground contact measured on an MI355X over the fixtures of this file (see MEASURED_PRE_CONTACT; docs/NOTES.md "free balls").
# Measured (x max |pos| of the comparison): generator settings per frame 5.77e-7 (1.15e-5 m at 20.0 m); task settings per frame 3.61e-7
# (7.73e-6 m at 21.4 m); task settings per call, stand-alone kernel and env kernel alike, PGS and TGS alike, 4.98e-7 (7.73e-6 m at 15.5 m).
MEASURED_PRE_CONTACT = 5.77e-7
POS_FLAT = 4 * MEASURED_PRE_CONTACT


def compare_with_oracle(name, cfg, got_pos, calls, sens, stride, what):
    """got_pos [n,T,3] against calls[:, ::stride][:, :T] of the oracle.  Returns the launches that need the conditioning term; asserts
    the bound, and the flat term alone before the first ground contact.  Prints the largest pre-contact error (what POS_FLAT is 4 x of)."""
    ref, sn = calls[:, ::stride, 0:3][:, :got_pos.shape[1]], sens[:, ::stride, 0:3][:, :got_pos.shape[1]]
    scale = max(1.0, np.abs(ref).max())
    err = np.abs(got_pos.astype(np.float64) - ref)
    need, worst_pre, fails = [], 0.0, []
    for i in range(len(ref)):
        first = first_contact_call(cfg, calls[i])
        pre = np.arange(ref.shape[1]) * stride <= first   # frames whose every earlier call ran without ground rows
        worst_pre = max(worst_pre, float(err[i][pre].max()) / scale)
        if not (err[i][pre] <= POS_FLAT * scale).all():
            fails.append("%s %s launch %d: pre-contact error %.3e m, %.2f x the flat term" % (name, what, i, err[i][pre].max(), err[i][pre].max() / (POS_FLAT * scale)))
        lim = POS_FLAT * scale + K_SENS * sn[i]
        if not (err[i] <= lim).all():
            fails.append("%s %s launch %d: error %.3e m, %.2f x its bound" % (name, what, i, err[i].max(), (err[i] / lim).max()))
        if (err[i] > POS_FLAT * scale).any():
            need.append(i)
    print("[ball] %-9s %-22s largest pre-contact error %.2e (x max|pos| %.1f m = %.2e m); largest error %.2e m; launches that need the conditioning term: %s"
          % (name, what, worst_pre, scale, worst_pre * scale, err.max(), need))
    assert not fails, "; ".join(fails)
    return need


# ------------------------------------------------------------------------------------------------------------------ the fixture
FRAMES = 60
GOLDEN = "ball_rollout_oracle.npz"   # under tests/golden: what tools/gen_golden_ball_rollout.py records with the functions above


ENV_LAUNCHES = 8   # launches of the comparison with the env kernel (the drawn ones): all that `task_tgs` is recorded for


def fixture_cfgs():
    """The settings of the oracle fixture: the generator's (6 substeps, 2 iterations, TGS, 0.7 / 0.6, spin_scale 5), a racket + ball
    task's own ball at its defaults (2 substeps, 4 iterations, PGS, 0.5 / 0.9, spin_scale 1), and that task's ball under TGS."""
    from vid2player3d_amd import ball_traj, racket

    m = racket.BALL_MATERIAL
    task = ball_traj.ball_sim_cfg(substeps=2, spin_scale=1.0, solver_type=0, restitution_ground=m["rest_ground"], friction_ground=m["fric_ground"])
    return {"generator": ball_traj.ball_sim_cfg(substeps=6, spin_scale=5), "task": task, "task_tgs": dict(task, solver_type=1)}


def fixture_launches(seed=20261017):
    """(pos [10,3], vel [10,3], vspin [10]) float32: 8 launches from the default ranges of TennisBallGeneratorIsaac (utils/tennis_ball.py:
    278-306), one with back spin, one dropped from rest."""
    rng = np.random.default_rng(seed)
    u = lambda lo, hi, size=None: rng.uniform(size=size) * (np.asarray(hi, float) - np.asarray(lo, float)) + np.asarray(lo, float)
    origin, bounce = u([-4, 12, 1], [4, 13, 1.5], (8, 3)), u([-3, -10, 0], [3, -7, 0], (8, 3))
    d = bounce[:, :2] - origin[:, :2]
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    speed, theta, vspin = u(28, 30, 8), u(5, 15, 8) / 180 * np.pi, u(5, 10, 8)
    vel = np.stack([speed * np.cos(theta) * d[:, 0], speed * np.cos(theta) * d[:, 1], speed * np.sin(theta)], 1)
    pos = np.concatenate([origin, [[0.5, 12.5, 1.2], [1.0, 2.0, 1.0]]])
    vel = np.concatenate([vel, [[-1.0, -25.0 * np.cos(0.2), 25.0 * np.sin(0.2)], [0.0, 0.0, 0.0]]])
    vspin = np.concatenate([vspin, [-6.0, 0.0]])
    return pos.astype(np.float32), vel.astype(np.float32), vspin.astype(np.float32)


BACKSPIN, DROP = 8, 9


def cfg_arrays(cfg):
    """A settings dict as (names, float64 values), the form it is stored in beside the trajectories recorded with it."""
    keys = sorted(cfg)
    return np.array(keys), np.array([float(cfg[k]) for k in keys])


def load_golden():
    """The recorded fixture, after checking that it was recorded with the settings and launches that fixture_cfgs() / fixture_launches()
    give NOW: a change of a default would otherwise compare the kernel against a stale oracle."""
    import os

    gold = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", GOLDEN))
    for name, cfg in fixture_cfgs().items():
        keys, vals = cfg_arrays(cfg)
        assert list(gold[name + "/cfg_keys"]) == list(keys) and np.array_equal(gold[name + "/cfg"], vals), \
            "tests/golden/%s was recorded with other `%s` settings: run tools/gen_golden_ball_rollout.py" % (GOLDEN, name)
    for k, a in zip(("launch_pos", "launch_vel", "launch_vspin"), fixture_launches()):
        assert np.array_equal(gold[k], a), "tests/golden/%s was recorded with other launches (%s)" % (GOLDEN, k)
    return gold
