"""Contact generation of the tennis ball in the link-per-lane physics kernel, case by case: ball x the racket's two solid cylinders (face,
side, rim, centre inside, handle, throat), ball x the hulls of the links (nearest feature a vertex, an edge, a face; centre inside a hull
and at its bounding-box centre; the box cull; 0, 1, 2, 3 and more than 3 candidates; the racket's own link left out) and the
speculative activation test - one designed launch per env (tests/ball_contact_cases.py), one control step of the public task, judged
against each env's float64 C oracle at the bounds of tests/test_gpu_racket_ball.py.

What "the designed case" means is the numpy statement of the generation rule in tests/ball_contact_cases.py;
test_oracle_alone_produces_every_case checks on the CPU that every launch is classified as designed with 1e-4 m to spare, that the
oracle generates the same rows, and that the bounds of the GPU comparison are small against what each contact does to the ball.

Left out: exact float32 ties between two candidates, ball x ground (tests/test_gpu_ball_rollout.py and the `ground` scenarios), six
substeps per call, per-clip body shapes."""
import functools

import numpy as np
import pytest

from oracle import phys_oracle as po
from tests import ball_contact_cases as B

NSUB, SUB_PER_SIM = 4, 2
K_SENS = 16.0                 # the project's conditioning factor (tests/gpu_util.close)
SENS_CAP, SENS_SHARE, SENS_MIN_ENVS = 200.0, 0.02, 4  # tests/gpu_util.py (restated: this module's CPU tests import no torch)
TOL = {"pos": 2e-5, "vel": 5e-4, "quat": 1e-4, "force": 2e-2, "rbvel": 1e-3}  # the flat terms of tests/test_gpu_racket_ball.py
FREE = -np.ones((NSUB, 24, 4), dtype=np.int32)  # hull x ground vertices: none, the humanoid floats at 3 m


@functools.lru_cache(maxsize=None)
def oracle_step(case, player, solver, without=()):
    """The oracle's control step of one env from its designed launch (PD targets = the pose, no residual wrench) with the conditioning
    of that step; shared by the tests, nothing modifies what it returns."""
    e = B.env_of(case, player)
    o = B.oracle_for(player, solver, e["state"], without=without)
    o.set_ball(e["ball"])
    kw = dict(pd_target=e["state"][1], ext_force=np.zeros(3), ext_torque=np.zeros(3), nsub=NSUB, hold=2, sub_per_sim=SUB_PER_SIM, forced_ids=FREE)
    sens = o.ball_sensitivity(seed=0, **kw)
    cf, _, ids, per_sim, hit, bc = o.step_ball(**kw)
    assert (ids < 0).all() and (o.own_ids < 0).all(), "no link touches the ground"
    return {"per_sim": per_sim, "hit": hit, "bc": bc, "bbf": o.ball_body_force, "rb": o.get_state()[3], "cf": cf, "cfs": o.contact_force_sum, "sens": sens}


def first_substep(case, player, solver, nsub):
    """(hull points of the oracle in the first `nsub` substeps, ball state after them) from the designed launch."""
    e = B.env_of(case, player)
    o = B.oracle_for(player, solver, e["state"])
    o.set_ball(e["ball"])
    o.step_ball(pd_target=e["state"][1], nsub=nsub, hold=0, sub_per_sim=nsub)
    return o.max_hull_points, o.get_ball()


def free_flight_dv(ball):
    """Velocity change of a ball without contact over one simulate() call: gravity and the aerodynamic force held over the call."""
    return SUB_PER_SIM * B.H * (np.array([0.0, 0.0, -9.81]) + po.ball_aero(ball) / 0.057)


def batch_bounds(names, player, solver):
    """Flat terms of the GPU comparison for a batch (gpu_util.close: tol x max(1, max |reference|)) on ball velocity and spin."""
    ps = np.stack([oracle_step(c, player, solver)["per_sim"] for c in names])
    return TOL["vel"] * max(1.0, np.abs(ps[..., 7:10]).max()), TOL["vel"] * max(1.0, np.abs(ps[..., 10:13]).max())


def check_expectation(case, e):
    """The numpy statement classifies the launch as designed."""
    cl, ex = e["cl"], e["expect"]
    for j, c in enumerate(cl["cyl"]):
        assert c["row"] == (j in ex["cyl"]), (case, j, c)
        if c["row"]:
            assert c["region"] == ex["cyl"][j], (case, j, c["region"])
    if ex.get("speculative"):
        rows = [c for c in cl["cyl"] if c["row"]] + [cl["hulls"][b] for b in cl["cand"]]
        assert all(_speculative_only(r) for r in rows), (case, "every row of this case exists through the speculative margin alone")
    if "hull" in ex:
        b, feature = ex["hull"]
        hr = cl["hulls"][b]
        assert b in cl["cand"][:3] and not hr["inside"] and hr["feature"] == feature, (case, cl["cand"], hr)
        assert hr["feature_slack"] >= B.MARGIN and hr["feature_weight"] >= 0.2 and hr["feature_fit"] < 1e-9 and hr["qp_err"] < 2e-6, (case, hr)
    if "count" in ex:
        assert (len(cl["cand"]) >= 4) if ex["count"] == ">=4" else (len(cl["cand"]) == ex["count"]), (case, cl["cand"])
    if "inside" in ex:
        hr = cl["hulls"][ex["inside"]]
        assert hr["inside"] and cl["cand"][0] == ex["inside"] and sum(h["inside"] for h in cl["hulls"].values()) == 1, (case, cl["cand"])
        assert (hr["centre_dist"] < 0.1 * B.CENTRE_EPS) if ex.get("at centre") else (hr["centre_dist"] > 1e-2), (case, hr["centre_dist"])
    if ex.get("in racket hull"):
        assert cl["racket_hull"]["inside"] and cl["racket_hull"]["row"], (case, "the hull of the racket's link would be the nearest candidate")
    if ex.get("hand only"):
        assert cl["cand"] == [B.models(e["player"])[1]["racket_link"] + 1], (case, cl["cand"])
    if "boxes" in ex:
        assert bool(cl["boxes"]) == ex["boxes"], (case, cl["boxes"])
    if ex.get("free"):
        assert not cl["cand"] and not any(c["row"] for c in cl["cyl"]), case


def _speculative_only(row):
    return row["gap"] > B.COFF + B.MARGIN and row["gap"] < row["thr"] - B.MARGIN


def wave_kinds(names, player):
    """Kinds of wave in a batch (envs 2w, 2w + 1), by bounding boxes in reach (the any64(near) branch) and by hull candidates (the
    per-half selection): "boxes both / lower / upper / none", "candidates both / lower / upper / none", and a cylinder case beside a
    hull case."""
    kinds = set()
    for w in range(0, len(names) - 1, 2):
        a, b = (B.env_of(c, player)["cl"] for c in names[w:w + 2])
        for what, key in (("boxes", "boxes"), ("candidates", "cand")):
            na, nb = len(a[key]) > 0, len(b[key]) > 0
            kinds.add(what + (" both" if na and nb else " lower" if na else " upper" if nb else " none"))
        if any(c["row"] for c in a["cyl"]) != any(c["row"] for c in b["cyl"]) and (len(a["cand"]) > 0) != (len(b["cand"]) > 0):
            kinds.add("cylinder beside hull")
    return kinds


@pytest.mark.parametrize("player,sizes", [("djokovic", (3, 34)), ("nadal", (12,))])
def test_oracle_alone_produces_every_case(player, sizes):
    """CPU.  One line per case with its margins (pytest -s).  Seen: the bound of the GPU comparison is 0.03 ... 0.7 % of what the
    contact does to the ball (largest: a centre inside the solid head, pushed out at 0.8 m/s), the smallest decisive margin 2.9e-4 m
    (chest face: the spine's hull 0.3 mm nearer than the chest's)."""
    names = sorted(set(c for n in sizes for c in B.BATCHES[n]), key=list(B.CASES).index)
    if player == "djokovic":
        assert set(names) == set(B.CASES), "every case is in a batch"
        assert B.BATCH_3[0] == B.BATCH_34[0] and B.env_of(B.BATCH_3[1], player)["expect"].get("boxes") is False and B.env_of(B.BATCH_34[1], player)["expect"]["count"] == 3
        assert {"boxes both", "boxes lower", "boxes upper", "boxes none", "candidates both", "candidates lower", "candidates upper", "candidates none",
                "cylinder beside hull"} <= wave_kinds(B.BATCH_34, player), wave_kinds(B.BATCH_34, player)
        assert {1, 2, 3} <= {B.env_of(c, player)["cl"]["hulls"][B.env_of(c, player)["expect"]["hull"][0]]["feature"] for c in names if "hull" in B.env_of(c, player)["expect"]}
    print()
    unstable = []
    for case in names:
        e = B.env_of(case, player)
        cl = e["cl"]
        check_expectation(case, e)
        margin = B.decisive_margin(cl, at_centre=e["expect"]["inside"] if e["expect"].get("at centre") else None)
        assert margin >= B.MARGIN, (case, margin)
        rows = len(cl["cand"][:3]) + sum(c["row"] for c in cl["cyl"])
        line = "[ball case] %-21s cylinders %-16s hull candidates %-16s margin %.1e m" % (case, "/".join(c["region"] if c["row"] else "-" for c in cl["cyl"]), cl["cand"], margin)
        for solver in ("pgs", "tgs"):
            nh, _ = first_substep(case, player, solver, 1)
            assert nh == min(len(cl["cand"]), 3), (case, solver, nh, cl["cand"])
            _, after = first_substep(case, player, solver, SUB_PER_SIM)
            change = np.linalg.norm(after[7:10] - e["ball"][7:10] - free_flight_dv(e["ball"]))  # what the contacts of the first call did to the ball
            ref = oracle_step(case, player, solver)
            assert np.array_equal(ref["per_sim"][0], after)
            flat_v, flat_w = batch_bounds(tuple(names), player, solver)
            sens = ref["sens"]
            if rows == 0:
                assert change < 1e-9, (case, solver, change)
            else:
                bound = flat_v + min(K_SENS * sens["ball"][0, 7:10].max(), SENS_CAP * flat_v)
                assert bound < 0.05 * change, "%s %s: the bound %.2e is not small against the contact's effect %.2e m/s" % (case, solver, bound, change)
                line += " | %s: contact changes v by %.2f m/s, bound %.1e (%.2f %%)" % (solver, change, bound, 100 * bound / change)
            # the oracle alone, perturbed at float32 rounding, stays inside the flat terms: no env needs the conditioning term by itself
            shares = {"velocity": sens["ball"][:, 7:10].max() / flat_v, "spin": sens["ball"][:, 10:13].max() / flat_w, "quaternion": sens["ball"][:, 3:7].max() / TOL["quat"],
                      "force": sens["bc"].max() / (TOL["force"] * max(1.0, np.abs(ref["bc"]).max(), np.abs(ref["bbf"]).max()))}
            if max(shares.values()) > 1.0:
                unstable.append((case, solver, {k: round(float(v), 2) for k, v in shares.items() if v > 1.0}))
        print(line)
    assert not unstable, "the oracle's own step moves by more than a flat term under float32-rounding perturbations: %s" % unstable
    if player == "djokovic":
        # the third record carries load: with exactly three candidates and with more than three (the farthest is dropped - taking its
        # hull away changes nothing), the oracle without the THIRD candidate's hull gives another ball
        for case in ("count 3", "count 4"):
            cl = B.env_of(case, player)["cl"]
            third, dropped = cl["cand"][2], cl["cand"][3:]
            for solver in ("pgs", "tgs"):
                ref = oracle_step(case, player, solver)
                flat_v, _ = batch_bounds(tuple(names), player, solver)
                bound = flat_v + min(K_SENS * ref["sens"]["ball"][:, 7:10].max(), SENS_CAP * flat_v)
                if dropped:
                    same = oracle_step(case, player, solver, without=tuple(dropped))
                    assert np.abs(same["per_sim"] - ref["per_sim"]).max() < 1e-12
                other = oracle_step(case, player, solver, without=(third,))
                diff = np.abs(other["per_sim"][:, 7:10] - ref["per_sim"][:, 7:10]).max()
                assert diff > 20 * bound, (case, solver, diff, bound)
                print("[ball case] %s (%s): candidates %s, dropped %s; without the third (%d) the ball's velocity differs by %.2f m/s = %.0f bounds"
                      % (case, solver, cl["cand"], dropped, third, diff, diff / bound))


# ---------------------------------------------------------------------------------------------------------------- solid cylinder
def _cylinder_points():
    """(cylinder, region, body-frame point) in the face, side, rim and inside regions of handle and head."""
    _, geom = B.models("djokovic")
    out = []
    for j, c in enumerate(geom["cylinders"]):
        a, hl, rc = np.asarray(c["axis"]), float(c["half_len"]), float(c["radius"])
        u = np.cross(a, [0.3, -0.5, 0.8])
        u /= np.linalg.norm(u)
        for region, t, rho in (("face+", hl + 0.07, 0.6 * rc), ("face-", -hl - 0.065, 0.3 * rc), ("side", 0.4 * hl, rc + 0.068), ("rim+", hl + 0.05, rc + 0.05),
                               ("rim-", -hl - 0.06, rc + 0.045), ("inside+", 0.5 * hl, 0.5 * rc), ("inside-", -0.3 * hl, 0.7 * rc)):
            out.append((j, region, np.asarray(c["center"]) + t * a + rho * u))
    return geom, out


def _resting_racket(j):
    """The oracle with the humanoid at rest, no gravity, and cylinder j alone on the racket's link (no friction, no hull contacts)."""
    model, geom = B.models("djokovic")
    geom = dict(geom, cylinders=[geom["cylinders"][j]])
    o = po.PhysOracle(model, po.default_params(gravity_z=0.0, ang_damp=0.0), kp=model.kp.astype(np.float32), kd=model.kd.astype(np.float32))
    root = np.zeros(13)
    root[2], root[3:7] = 3.0, B.BASE
    o.set_state(root, np.zeros(69), np.zeros(69))
    o.attach_ball(geom, material={"fric_racket": 0.0, "bounce_threshold": 1e9}, body_contacts=False)
    return o, geom


def test_solid_cylinder_closest_point():
    """The numpy statement of the cylinder rule against a bounded minimisation over the solid, and the oracle against the numpy
    statement through step_ball on a resting racket (no gravity, no friction, no bounce, no spin: the impulse on the ball is along
    the oracle's normal, and the relative normal velocity it leaves is the oracle's gap over h)."""
    from scipy.optimize import minimize

    from scipy.spatial.transform import Rotation

    _, points = _cylinder_points()
    for j, region, pbody in points:
        o, geom = _resting_racket(j)
        rb = o.get_state()[3]
        link = geom["racket_link"]
        x, Rw = rb[link, 0:3], Rotation.from_quat(rb[link, 3:7]).as_matrix()
        c = geom["cylinders"][0]
        s = x + Rw @ pbody
        ball = np.zeros(13)
        ball[0:3], ball[6] = s, 1.0
        got = B.cyl_rule(rb, geom, 0, ball)
        assert got["region"] == region, (j, region, got["region"])
        # ---- the statement against a minimisation over the solid: p = centre + t a + r (cos f u + sin f w), |t| <= hl, 0 <= r <= rc
        cw, aw, hl, rc = x + Rw @ np.asarray(c["center"]), Rw @ np.asarray(c["axis"]), float(c["half_len"]), float(c["radius"])
        u = np.cross(aw, [1.0, 0.0, 0.0])
        u /= np.linalg.norm(u)
        w = np.cross(aw, u)
        point = lambda p: cw + p[0] * aw + p[1] * (np.cos(p[2]) * u + np.sin(p[2]) * w)
        best = min((minimize(lambda p: np.sum((point(p) - s) ** 2), [0.0, 0.5 * rc, f0], method="L-BFGS-B", bounds=[(-hl, hl), (0.0, rc), (None, None)],
                             options={"ftol": 1e-18, "gtol": 1e-14}) for f0 in np.arange(6) * np.pi / 3), key=lambda r: r.fun)
        assert abs(np.sqrt(best.fun) - (got["gap"] + B.RB)) < 1e-7, (j, region, np.sqrt(best.fun), got["gap"] + B.RB)
        if not region.startswith("inside"):
            assert np.linalg.norm(point(best.x) - got["pt"]) < 1e-5 and abs(np.linalg.norm(got["n"]) - 1) < 1e-12 and np.allclose(got["pt"] + (got["gap"] + B.RB) * got["n"], s, atol=1e-12)
        else:
            assert np.allclose(got["n"], (1 if region[-1] == "+" else -1) * aw, atol=1e-12)
        # ---- the oracle against the statement: one substep with a ball that flies along -n fast enough to reach the surface
        speed = 0.0 if region.startswith("inside") else (got["gap"] / B.H + 3.0)
        b0 = ball.copy()
        b0[7:10] = -speed * got["n"]
        o.set_ball(b0)
        o.step_ball(pd_target=np.zeros(69), nsub=1, hold=0, sub_per_sim=1)
        b1, rb1 = o.get_ball(), o.get_state()[3]
        dv = b1[7:10] - b0[7:10]
        assert np.linalg.norm(dv) > 0.5 and np.linalg.norm(dv - (dv @ got["n"]) * got["n"]) < 1e-7 * np.linalg.norm(dv), (j, region, dv, got["n"])  # the impulse is along the normal
        # ... and leaves the two contact points approaching at gap / h (they meet at the end of the substep), resp. separating at
        # erp R / h when the centre is inside
        vrel = (b1[7:10] - rb1[link, 7:10] - np.cross(rb1[link, 10:13], got["pt"] - x)) @ got["n"]  # (the row is written at the start of the substep)
        want = 0.2 * B.RB / B.H if region.startswith("inside") else -got["gap"] / B.H
        # (1e-4 m/s = 1e-6 m of gap: the link's velocity is read back in the pose AFTER the substep, which moves the recoiling racket's
        # contact point by some 1e-5 m/s)
        assert abs(vrel - want) < 1e-4, (j, region, vrel, want)


# ---------------------------------------------------------------------------------------------------------------- GPU
@functools.lru_cache(maxsize=None)
def _mlib():
    from tests.gpu_util import DEV, synth_tables
    from vid2player3d_amd.motion_lib import MotionLib

    return MotionLib(synth_tables(seed=5, num_clips=8, min_frames=60, max_frames=120), DEV)


@functools.lru_cache(maxsize=None)
def run_kernel(n, build, solver, player):
    """One control step of the kernel from the designed launches of a batch.  Shared by the tests; nothing modifies what it returns."""
    import torch

    from oracle import task_oracle as O
    from tests.gpu_util import N, T, close
    from tests.test_gpu_racket_ball import make_rb_task

    names = B.BATCHES[n]
    envs = [B.env_of(c, player) for c in names]
    task = make_rb_task(n, _mlib(), player=player, joint_limits=False, contact_solver=solver, kernel_build=build, pair_envs_by_load=False)
    model, geom = B.models(player)
    assert task.kernel_build().startswith({1: "lds-parked", 2: "registers"}[build]) and task.racket_geometry["racket_link"] == geom["racket_link"]
    assert np.array_equal(np.asarray(task.body_model.hull_verts), np.asarray(model.hull_verts)), "the task's body is the one the launches were designed on"
    task.reset_with_times(None, T(np.full(n, 0.3)))
    root, dpos, dvel = (np.stack([e["state"][k] for e in envs]) for k in range(3))
    task._humanoid_root_states[:] = T(root)
    task._dof_pos[:] = T(dpos)
    task._dof_vel[:] = T(dvel)
    task._reset_env_tensors(None)
    task._rigid_body_state[:] = T(np.stack([e["rb"] for e in envs]).reshape(n * 24, 13))
    task._ball_root_states[:] = T(np.stack([e["ball"] for e in envs]))
    act = np.concatenate([dpos, np.zeros((n, 6), dtype=np.float32)], axis=1)  # PD targets = the pose, no residual wrench
    rb0 = N(task._rigid_body_state).reshape(n, 24, 13).copy()
    task.pre_physics_step(T(act))
    task._physics_step()
    torch.cuda.synchronize()
    _, pd, _, force, torque = O.pre_physics(act, N(task.reset_buf), dpos, rb0[:, 0, 3:7], task.body_model.kp.astype(np.float32))
    close(N(task._pd_target), pd, 1e-6, "pd target")
    assert np.array_equal(pd, dpos) and not force.any() and not torque.any()
    got = {"per_sim": N(task._ball_states_per_sim).copy(), "ball": N(task._ball_root_states).copy(), "rb": N(task._rigid_body_state).reshape(n, 24, 13).copy(),
           "bc": N(task._ball_contact_forces).copy(), "bbf": N(task._ball_body_contact_force).copy(), "cf": N(task._contact_forces).copy(),
           "cfs": N(task._contact_forces_sum).copy(), "hit": N(task._racket_ball_contact_per_sim).copy(), "ids_sub": N(task.debug_contacts_substeps()).copy()}
    task.close()
    return got


def _compare(n, build, solver, player):
    from tests.gpu_util import close

    names = B.BATCHES[n]
    got = run_kernel(n, build, solver, player)
    assert (got["ids_sub"] < 0).all(), "no link touches the ground: the oracle is teacher-forced with no hull x ground vertex"
    ref = [oracle_step(c, player, solver) for c in names]
    R = {k: np.stack([r[k] for r in ref]) for k in ("per_sim", "hit", "bc", "bbf", "rb", "cf", "cfs")}
    S = {k: np.stack([r["sens"][k] for r in ref]) for k in ref[0]["sens"]}
    need = np.zeros(n, dtype=bool)  # envs that need the conditioning term somewhere
    failed = []

    def check(a, b, tol, what, sens=None):
        a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
        flat = tol * max(1.0, np.abs(b).max())
        err = np.abs(a - b).reshape(n, -1)
        lim = np.full_like(err, flat) if sens is None else (flat + np.minimum(K_SENS * np.asarray(sens, dtype=np.float64), SENS_CAP * flat)).reshape(n, -1)
        need[:] |= (err > flat).any(axis=1)
        worst = (err / lim).max(axis=1)
        print("[ball contacts] %-46s largest share of its bound %.3f (%s)" % (what, worst.max(), names[int(worst.argmax())]))
        try:
            close(a, b, tol, what, sens=sens, k_sens=K_SENS)
        except AssertionError as ex:
            failed.append("%s | cases over their bound: %s" % (ex, ", ".join("%s (env %d, %.1f x)" % (names[i], i, worst[i]) for i in np.nonzero(worst > 1.0)[0])))

    ps = got["per_sim"]
    check(ps[..., 0:3], R["per_sim"][..., 0:3], TOL["pos"], "ball position after each simulate() call")
    qs = np.sign(np.sum(ps[..., 3:7] * R["per_sim"][..., 3:7], -1, keepdims=True))
    check(ps[..., 3:7] * qs, R["per_sim"][..., 3:7], TOL["quat"], "ball quaternion", sens=S["ball"][..., 3:7])
    check(ps[..., 7:10], R["per_sim"][..., 7:10], TOL["vel"], "ball velocity after each simulate() call", sens=S["ball"][..., 7:10])
    check(ps[..., 10:13], R["per_sim"][..., 10:13], TOL["vel"], "ball spin after each simulate() call", sens=S["ball"][..., 10:13])
    assert np.array_equal(got["ball"], ps[:, -1]), "_ball_root_states is the state after the last call"
    check(got["bc"], R["bc"], TOL["force"], "_ball_contact_forces (racket, ground)", sens=S["bc"][:, 0:2])
    check(got["bbf"], R["bbf"], TOL["force"], "_ball_body_contact_force", sens=S["bc"][:, 2])
    check(got["rb"][..., 0:3], R["rb"][..., 0:3], TOL["pos"], "rigid-body positions")
    check(got["rb"][..., 7:13], R["rb"][..., 7:13], TOL["rbvel"], "rigid-body velocities", sens=S["rb"][..., 7:13])
    check(got["cf"], R["cf"], TOL["force"], "_contact_forces", sens=S["cf"])
    check(got["cfs"], R["cfs"], TOL["force"], "_contact_forces_sum", sens=S["cfs"])
    wrong = np.nonzero((got["hit"] != R["hit"]).any(axis=1))[0]
    if len(wrong):
        failed.append("_racket_ball_contact_per_sim differs in: %s" % ", ".join("%s (env %d: %s, oracle %s)" % (names[i], i, got["hit"][i].tolist(), R["hit"][i].tolist()) for i in wrong))
    assert not failed, "\n".join(failed)
    # (the flag looks at the LAST substep of a call: of the designed cases only a centre inside the head still carries force there)
    assert n != 34 or R["hit"].any(), "the batch of 34 holds a case that raises the racket-hit flag"
    allowed = min(max(SENS_MIN_ENVS, int(SENS_SHARE * n)), n // 2)
    print("[ball contacts] n=%d build %d %s %s: envs that need the conditioning term: %s (%d allowed)" % (n, build, solver, player, [names[i] for i in np.nonzero(need)[0]], allowed))
    assert need.sum() <= allowed, "%d of %d envs need the conditioning term: %s" % (need.sum(), n, [names[i] for i in np.nonzero(need)[0]])


@pytest.mark.gpu
@pytest.mark.parametrize("solver", ["pgs", "tgs"])
@pytest.mark.parametrize("build", [1, 2])
@pytest.mark.parametrize("n", [3, 34])
def test_ball_after_each_call_matches_oracle(n, build, solver):
    _compare(n, build, solver, "djokovic")


@pytest.mark.gpu
def test_ball_after_each_call_matches_oracle_left_handed():
    """The cylinder group with the racket on L_Wrist (player nadal): the mirror image of the racket's geometry."""
    _compare(12, 1, "tgs", "nadal")


@pytest.mark.gpu
@pytest.mark.parametrize("solver", ["pgs", "tgs"])
@pytest.mark.parametrize("build", [1, 2])
def test_env_bits_do_not_depend_on_the_partner(build, solver):
    """Env 0 holds the same state and launch next to a partner without any ball contact (batch of 3) and next to one with three hull
    candidates (batch of 34): bit-identical ball and rigid-body outputs."""
    a, b = run_kernel(3, build, solver, "djokovic"), run_kernel(34, build, solver, "djokovic")
    launched = B.env_of(B.BATCH_3[0], "djokovic")["ball"]
    assert np.linalg.norm(a["per_sim"][0, 0, 7:10] - launched[7:10]) > 1.0, "env 0 has a hull contact in its first call"
    for key in ("per_sim", "ball", "rb", "bc", "bbf", "cf", "cfs", "hit"):
        assert np.array_equal(a[key][0], b[key][0]), key
