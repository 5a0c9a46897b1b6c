"""v2p_ball_rollout (csrc/ball_rollout.hip): free balls on their own against the float64 oracle, against the ball lane of the env kernel,
the online resampler against its numpy statement, batch sizes, and - without a GPU - every refusal of the entry point.

The oracle's side is tests/golden/ball_rollout_oracle.npz, recorded by tools/gen_golden_ball_rollout.py with tests/ball_oracle.py (the
oracle steps a humanoid next to every ball and takes seconds per trajectory; 252 of them are behind the fixture).

The bound of a comparison follows tests/gpu_util.py: a flat term, plus K_SENS = 16 x the change of the oracle's own trajectory under
launch perturbations of float32-rounding size.  Before the first ground contact the flat term alone must hold."""
import ctypes as C

import numpy as np
import pytest
import torch

from tests import ball_oracle as B
from vid2player3d_amd import _lib, ball_traj

VEL_FLAT = 5e-4                 # velocities and spins of the final state: the flat term of the env kernel's ball test (test_gpu_racket_ball.py)
U32 = 2.0 ** -24                 # unit roundoff of float32


def quat_flat(cfg, calls):
    """Flat term of the final orientation of ONE ball, from the number format alone (first order, worst case).  Every substep multiplies
    the spin by 1 / (1 + h x damping): the sum is rounded (<= 1 u, the same way every time: a bias, not noise), the reciprocal is good to
    1 ulp (<= 1 u below 1), the product is rounded (<= 1 u) - the spin's relative error after k substeps is <= 3 u k, the turned angle's
    after S substeps <= 3 u S / 2 of theta = sum |w| sim_dt, and a quaternion component moves by half an angle.  Composing and normalising
    S rotations adds <= 4 u each.  (The env kernel's test allows 1e-4 after the 2 calls of one control step; here 120 calls turn the ball
    by ~55 rad, and the bias of the CORRECTLY rounded factor alone is 3.8e-8 / 6.0e-8 per substep at 6 / 2 substeps: 2e-4 .. 4e-4.)"""
    S = (len(calls) - 1) * cfg["substeps"]
    theta = float(np.linalg.norm(calls[:-1, 10:13], axis=1).sum()) * cfg["sim_dt"]
    return 3 * U32 * S / 2 * theta / 2 + 4 * U32 * S


MAX_CONDITIONED = 2             # launches of 10 that may need the conditioning term
MAX_UNDECIDED = 1               # launches whose integer outputs hang on a quantity within the flat term of its threshold


def sim_struct(**kw):
    return ball_traj.sim_struct(dict(ball_traj.ball_sim_cfg(), **kw), 10)


# ---------------------------------------------------------------------------------------------------------------- CPU: refusals
def test_refusals_come_before_any_gpu_call():
    L = _lib.load()
    one = C.c_void_p(16)  # (a non-null placeholder: every call below is refused before anything is dereferenced)
    out = _lib.BallRolloutOut()
    ok = sim_struct()

    def refused(c, n=8, pos=one, vel=one, spin=one, o=out):
        rc = L.v2p_ball_rollout(None if c is None else C.byref(c), n, pos, vel, spin, None if o is None else C.byref(o), None)
        return rc == -1 and b"v2p_ball_rollout" in L.v2p_last_error()

    assert refused(None) and refused(ok, o=None)
    assert refused(ok, pos=None) and refused(ok, vel=None) and refused(ok, spin=None) and refused(ok, n=-1)
    for field in ("substeps", "control_freq_inv", "num_iterations"):
        assert refused(sim_struct(**{field: 0})), field
    c = sim_struct()
    c.num_frames = 0
    assert refused(c)
    assert refused(sim_struct(solver_type=2)) and refused(sim_struct(solver_type=-1))
    for field in ("mass", "inertia", "radius"):
        assert refused(sim_struct(**{field: 0.0})) and refused(sim_struct(**{field: -1.0})), field
    gx, gy = (0.0, 30.0, 0.5), (0.0, 3.0, 0.1)
    cfg0 = dict(ball_traj.ball_sim_cfg(), enable_ground=0)
    assert refused(ball_traj.sim_struct(ball_traj.ball_sim_cfg(), 10, (gx, gy)))            # resample with the ground on
    assert refused(ball_traj.sim_struct(cfg0, 10, (gx, (0.0, 0.0, 0.0))))                   # without both grids
    assert refused(ball_traj.sim_struct(cfg0, 10, ((0.0, 0.0, 0.5), gy)))
    assert refused(ball_traj.sim_struct(cfg0, 10, ((0.0, 30.0, -0.5), gy)))                 # non-positive step
    assert refused(ball_traj.sim_struct(cfg0, 10, (gx, (0.0, 3.0, 0.0))))
    # n = 0 is a no-op, null arrays and all
    assert L.v2p_ball_rollout(C.byref(ok), 0, None, None, None, C.byref(out), None) == 0
    assert L.v2p_ball_rollout(C.byref(ball_traj.sim_struct(cfg0, 10, (gx, gy))), 0, None, None, None, C.byref(out), None) == 0


def test_struct_layout_matches_the_header():
    import os
    import subprocess
    import tempfile

    repo = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    prog = r'''
#include <stdio.h>
#include <stddef.h>
#include "v2p_rollout.h"
int main(void){ printf("%zu %zu %zu %zu %zu %zu\n", sizeof(v2p_ball_sim), offsetof(v2p_ball_sim, sim_dt), offsetof(v2p_ball_sim, enable_ground),
                       offsetof(v2p_ball_sim, grid_x), sizeof(v2p_ball_rollout_out), offsetof(v2p_ball_rollout_out, traj_y)); return 0; }
'''
    with tempfile.TemporaryDirectory() as d:
        open(os.path.join(d, "s.c"), "w").write(prog)
        subprocess.check_call(["gcc", "-I", os.path.join(repo, "include"), os.path.join(d, "s.c"), "-o", os.path.join(d, "s")])
        got = [int(x) for x in subprocess.check_output([os.path.join(d, "s")]).split()]
    S, O = _lib.BallSim, _lib.BallRolloutOut
    assert got == [C.sizeof(S), S.sim_dt.offset, S.enable_ground.offset, S.grid_x.offset, C.sizeof(O), O.traj_y.offset]
    assert _lib.ABI_VERSION == 15


def test_resample_reference_on_a_parabola():
    """The checker itself, on a flight it can be checked against by hand: y = 10 t, z = -5 t^2 sampled at 60 Hz."""
    t = np.arange(62) / 60.0
    s = np.zeros((1, 62, 3), np.float32)
    s[0, :, 1], s[0, :, 2] = 10 * t, 100 - 5 * t ** 2
    tx, ty = ball_traj.resample_reference(s, (0, 8, 0.5), (0, 3, 0.1))
    x = np.arange(16) * 0.5
    assert np.abs(tx[0, 1:] + 5 * (x[1:] / 10) ** 2).max() < 2e-3          # (linear interpolation of a parabola between 60 Hz samples)
    y = np.arange(30) * 0.1
    assert np.abs(ty[0, 1:, 1] - np.sqrt(y[1:] / 5)).max() < 2e-3 and np.abs(ty[0, 1:, 0] - 10 * np.sqrt(y[1:] / 5)).max() < 2e-2
    # cell 0 of both grids stops at sample 0 and pairs it with sample -1, the LAST one (the reference's wrap)
    w = (0 - s[0, -1, 1]) / (s[0, 0, 1] - s[0, -1, 1])
    assert np.isclose(tx[0, 0], (s[0, -1, 2] - 100) * (1 - w), rtol=1e-5)


# ---------------------------------------------------------------------------------------------------------------- GPU
gpu = pytest.mark.gpu


def run_kernel(cfg, pos, vel, vspin, frames, **kw):
    dev = "cuda:0"
    t = lambda a: torch.as_tensor(np.ascontiguousarray(a), dtype=torch.float32, device=dev)
    res = ball_traj.rollout(cfg, t(pos), t(vel), t(vspin), num_frames=frames, **kw)
    torch.cuda.synchronize()
    return {k: v.cpu().numpy() for k, v in res.items()}


def flat_close(a, b, tol):
    return np.abs(np.asarray(a, np.float64) - b) <= tol * max(1.0, np.abs(b).max())


@gpu
@pytest.mark.parametrize("name", ["generator", "task"])
def test_rollout_matches_the_oracle(name):
    gold = B.load_golden()
    cfg = B.fixture_cfgs()[name]
    pos, vel, vspin = B.fixture_launches()
    calls, sens = gold[name + "/calls"], gold[name + "/sens"].astype(np.float64)
    cfi, F = cfg["control_freq_inv"], B.FRAMES
    got = run_kernel(cfg, pos, vel, vspin, F, want=("traj", "bounce_pos", "bounce_idx", "pass_net", "peak_after_bounce", "final_state"))
    top = [i for i in range(len(pos)) if i != B.BACKSPIN]   # (the oracle's aerodynamic call has no back spin: that launch is checked below)
    need = [top[k] for k in B.compare_with_oracle(name, cfg, got["traj"][top], calls[top], sens[top], cfi, "positions per frame")]
    # ---- final state: after the last call
    fin, fsn = calls[top, F * cfi], sens[top, F * cfi]
    scale = max(1.0, np.abs(calls[top][:, :, 0:3]).max())
    g = got["final_state"][top].astype(np.float64)
    g[:, 3:7] *= np.sign(np.sum(g[:, 3:7] * fin[:, 3:7], -1, keepdims=True))
    qtol = np.array([[quat_flat(cfg, calls[i][:F * cfi + 1])] for i in top])
    for sl, tol, what in ((slice(0, 3), B.POS_FLAT * scale, "pos"), (slice(3, 7), qtol, "quat"), (slice(7, 10), VEL_FLAT * max(1.0, np.abs(fin[:, 7:10]).max()), "vel"),
                          (slice(10, 13), VEL_FLAT * max(1.0, np.abs(fin[:, 10:13]).max()), "spin")):
        err = np.abs(g[:, sl] - fin[:, sl])
        print("[ball] %-9s final %-4s largest error %.2e, %.2f x its flat term (flat term %.2e); launches over it: %s"
              % (name, what, err.max(), (err / tol).max(), np.max(tol), [top[i] for i in np.nonzero((err > tol).any(axis=1))[0]]))
        assert (err <= tol + B.K_SENS * fsn[:, sl]).all(), "%s final %s: %.3e, %.2f x its bound" % (name, what, err.max(), (err / (tol + B.K_SENS * fsn[:, sl])).max())
        need += [top[i] for i in np.nonzero((err > tol).any(axis=1))[0]]
    assert len(set(need)) <= MAX_CONDITIONED, "%s: launches %s need the conditioning term" % (name, sorted(set(need)))
    # ---- bookkeeping: equal wherever the oracle's deciding quantity is more than the flat term away from its threshold
    undecided = []
    for i in top:
        bk = B.bookkeeping(cfg, calls[i], F)
        if bk["margin"] <= B.POS_FLAT * scale:
            undecided.append(i)
            continue
        assert int(got["bounce_idx"][i]) == bk["bounce_idx"] and bool(got["pass_net"][i]) == bool(bk["pass_net"]), (name, i, bk, got["bounce_idx"][i], got["pass_net"][i])
        j = np.nonzero(calls[i, :, 2] <= cfg["bounce_height"])[0]
        bsn = sens[i, j[0], 0:3] if len(j) else 0.0
        assert (np.abs(got["bounce_pos"][i] - bk["bounce_pos"]) <= B.POS_FLAT * scale + B.K_SENS * bsn).all(), (name, i, got["bounce_pos"][i], bk["bounce_pos"])
        # the peak is the largest RECORDED height from the bounce frame on: recomputed from the kernel's own trajectory
        assert got["peak_after_bounce"][i] == got["traj"][i, got["bounce_idx"][i]:, 2].max()
    print("[ball] %-9s launches whose integer outputs are undecided at the flat term: %s" % (name, undecided))
    assert len(undecided) <= MAX_UNDECIDED
    # the dropped ball never crosses y = 0; drawn launches cross the net and bounce within the 60 frames
    assert not got["pass_net"][B.DROP] and got["pass_net"][:8].any() and (got["bounce_idx"][:8] < F - 1).all() and got["bounce_idx"][B.DROP] < F - 1
    # ---- back spin: the numpy statement of the sign rule on the oracle's aerodynamic call, for the flight before the bounce
    i = B.BACKSPIN
    s0 = B.launch_state(pos[i].astype(np.float64), vel[i].astype(np.float64), float(vspin[i]))
    fl = B.backspin_flight(cfg, s0, F * cfi)
    # (the flight before the bounce: up to the first call that can touch the ground, and no further than the call after the one that
    # detects the bounce - from there on the sign is +)
    first = min(B.first_contact_call(cfg, fl), int(np.nonzero(fl[:, 2] <= cfg["bounce_height"])[0][0]) + 1)
    nfr = first // cfi + 1
    assert nfr > 10, "the back-spin launch must fly for a while"
    err = np.abs(got["traj"][i, :nfr].astype(np.float64) - fl[::cfi][:nfr, 0:3])
    print("[ball] %-9s back spin: %d frames before the bounce, largest error %.2e m (flat term %.2e m)" % (name, nfr, err.max(), B.POS_FLAT * scale))
    assert (err <= B.POS_FLAT * scale).all()
    # ... and the rule matters: with top spin of the same size the ball is elsewhere by then (the lift points the other way)
    top_spin = run_kernel(cfg, pos[i:i + 1], vel[i:i + 1], -vspin[i:i + 1], F, want=("traj",))["traj"][0]
    assert np.abs(top_spin[nfr - 1, 2] - got["traj"][i, nfr - 1, 2]) > 0.05
    # after the bounce the sign is +: the lift coefficient of every later call is the oracle's own formula (a bounce was seen)
    assert got["bounce_idx"][i] < F - 1


@gpu
@pytest.mark.parametrize("solver", ["pgs", "tgs"])
def test_rollout_matches_the_env_kernels_ball(solver):
    """The ball lane of the humanoid kernel and the stand-alone kernel simulate the same ball: 8 envs of a racket + ball task, the
    humanoid moved 50 m away and the ball x hull contacts off, against v2p_ball_rollout with the task's own settings - both within the
    oracle bound of the oracle's trajectories (the `task` / `task_tgs` settings of the fixture ARE the task's defaults under PGS / TGS).
    For these 8 launches the oracle's own trajectories are the same under both solvers to the last bit: one fast bounce, whose normal row is
    decided by the restitution target in the first sweep, and three mutually orthogonal rows - later sweeps and slices change nothing.  What
    the TGS case adds is the env kernel's TGS ball rows and the stand-alone kernel's, call by call; a slow ball that bounces again and
    again under TGS (gaps advanced slice by slice) is the dropped launch of the `generator` settings in the test above."""
    from tests.gpu_util import DEV, N, T, synth_tables
    from tests.test_gpu_racket_ball import make_rb_task
    from vid2player3d_amd.motion_lib import MotionLib

    n, steps = 8, 40
    gold = B.load_golden()
    fix = {"pgs": "task", "tgs": "task_tgs"}[solver]
    calls, sens = gold[fix + "/calls"][:n], gold[fix + "/sens"][:n].astype(np.float64)
    pos, vel, vspin = (a[:n] for a in B.fixture_launches())
    task = make_rb_task(n, MotionLib(synth_tables(seed=5, num_clips=8, min_frames=60, max_frames=120), DEV), contact_solver=solver, ball_body_contacts=False,
                        debug_contacts=0, contact_forces_sum=False)
    cfg = ball_traj.ball_sim_cfg_of(task)
    assert cfg == pytest.approx(B.fixture_cfgs()[fix], rel=1e-12), "the fixture's `%s` settings are the task's defaults under %s" % (fix, solver)
    task.reset_with_times(None, T(np.full(n, 0.2)))
    task._humanoid_root_states[:, 0:2] += 50.0
    task._reset_env_tensors(None)
    ang = ball_traj.launch_ang_vel(T(vel), T(vspin))
    task.reset_balls(np.arange(n), T(pos), T(vel), ang)
    per_sim = []
    act = torch.zeros((n, 75), device=DEV)
    for _ in range(steps):
        act[:, :69] = task._dof_pos
        task.pre_physics_step(act.clone())
        task._physics_step()
        per_sim.append(N(task._ball_states_per_sim).copy())
    torch.cuda.synchronize()
    env_calls = np.concatenate(per_sim, axis=1)   # [n, steps * cfi, 13]: the state after every simulate() call
    cfi = cfg["control_freq_inv"]
    # the stand-alone kernel, one frame per call: frame t is the position at the start of call t
    got = run_kernel(dict(cfg, control_freq_inv=1), pos, vel, vspin, steps * cfi + 1, want=("traj", "final_state"))
    cfg1 = dict(cfg, control_freq_inv=1)
    need = B.compare_with_oracle(fix, cfg1, got["traj"], calls, sens, 1, "rollout, per call")
    need += B.compare_with_oracle(fix, cfg1, np.concatenate([pos[:, None], env_calls[..., 0:3]], axis=1), calls, sens, 1, "env kernel, per call")
    assert len(set(need)) <= MAX_CONDITIONED
    same = np.array_equal(got["traj"][:, 1:], env_calls[..., 0:3])
    diff = np.abs(got["traj"][:, 1:].astype(np.float64) - env_calls[..., 0:3]).max()
    print("[ball] env kernel vs stand-alone kernel over %d calls: bit-identical positions: %s (largest difference %.2e m); final states equal: %s"
          % (steps * cfi, same, diff, np.array_equal(got["final_state"], env_calls[:, -1])))
    task.close()


@gpu
def test_online_resampler_equals_its_numpy_statement():
    """64 launches on a 4 x 4 x 4 grid of (horizontal speed, vertical speed, spin): traj_x / traj_y of a resample = 1 run against
    resample_reference applied to the positions the same kernel records without resampling (one frame per simulate() call).  Among
    them: slow balls that never drop to the last grid height (the end clamp), and the y = 0 / x = 0 cells (the wrap to the last sample)."""
    from tests.gpu_util import close

    cfg = dict(ball_traj.ball_sim_cfg(), enable_ground=0)
    F, cfi = 60, cfg["control_freq_inv"]
    vy, vz, vs = np.meshgrid([10.0, 20.0, 35.0, 64.9], [-5.0, 0.0, 5.0, 9.9], [-10.0, -0.2, 0.0, 9.8], indexing="ij")
    n = vy.size
    pos = np.zeros((n, 3), np.float32)
    pos[:, 2] = 100.0
    vel = np.stack([np.zeros(n), vy.ravel(), vz.ravel()], 1).astype(np.float32)
    vspin = vs.ravel().astype(np.float32)
    gx, gy = ball_traj.traj_out_params.TRAJ_X_RANGE, (0, 24, 0.8)   # (the drop grid reaches 23.2 m: the slow risers never get there in 61 frames)
    got = run_kernel(cfg, pos, vel, vspin, F, want=(), resample=(gx, gy))
    S = (F + 1) * cfi
    samples = run_kernel(dict(cfg, control_freq_inv=1), pos, vel, vspin, S, want=("traj",))["traj"]
    ref_x, ref_y = ball_traj.resample_reference(samples, gx, gy, cfg["sim_dt"])
    assert got["traj_x"].shape == (n, 60) and got["traj_y"].shape == (n, 30, 2)
    assert np.isfinite(ref_x).all() and np.isfinite(ref_y).all()
    drop = samples[:, 0, 2] - samples[:, -1, 2]
    assert (drop < 23.2).any() and (drop > 23.2).any(), "some launches must end above the last grid height (the end clamp), some below"
    assert (samples[:, -1, 1] < 29.5).any(), "some launches must end short of the last grid distance"
    close(got["traj_x"], ref_x, 1e-6, "traj_x")
    close(got["traj_y"][..., 0], ref_y[..., 0], 1e-6, "traj_y distance")
    close(got["traj_y"][..., 1], ref_y[..., 1], 1e-6, "traj_y time")
    # the default grids through the same path
    got2 = run_kernel(cfg, pos, vel, vspin, F, want=(), resample=(gx, ball_traj.traj_out_params.TRAJ_Y_RANGE))
    ref2 = ball_traj.resample_reference(samples, gx, ball_traj.traj_out_params.TRAJ_Y_RANGE, cfg["sim_dt"])
    close(got2["traj_y"], ref2[1], 1e-6, "traj_y, the reference's drop grid")
    assert np.array_equal(got2["traj_x"], got["traj_x"])


@gpu
@pytest.mark.parametrize("name", ["generator", "task"])
def test_a_balls_result_does_not_depend_on_the_batch(name):
    """N of 1, 63, 64, 65 and 1000: every ball as an N = 1 run of the same ball, bit for bit (trajectory staging, lanes past the end)."""
    cfg = B.fixture_cfgs()[name]
    p10, v10, s10 = B.fixture_launches()
    rng = np.random.default_rng(3)
    pick = rng.integers(0, 10, 1000)
    pos, vel, vspin = p10[pick] + rng.uniform(-0.2, 0.2, (1000, 3)).astype(np.float32) * [1, 1, 0], v10[pick], s10[pick]
    pos = pos.astype(np.float32)
    F = 37   # (not a multiple of the staging depth)
    want = ("traj", "bounce_pos", "bounce_idx", "pass_net", "peak_after_bounce", "final_state")
    runs = {n: run_kernel(cfg, pos[:n], vel[:n], vspin[:n], F, want=want) for n in (1, 63, 64, 65, 1000)}
    for i in (0, 1, 62, 63, 64, 511, 999):
        one = run_kernel(cfg, pos[i:i + 1], vel[i:i + 1], vspin[i:i + 1], F, want=want)
        for n, r in runs.items():
            if i < n:
                for k in want:
                    assert np.array_equal(r[k][i], one[k][0]), (name, n, i, k)
    for n in (63, 64, 65):
        for k in want:
            assert np.array_equal(runs[n][k], runs[1000][k][:n]), (name, n, k)
    assert np.isfinite(runs[1000]["traj"]).all()
