"""Helpers shared by the `-m gpu` parity tests."""

import numpy as np
import torch

from vid2player3d_amd import synth
from vid2player3d_amd.model import load_baked_model
from vid2player3d_amd.motion_lib import MotionLib
from vid2player3d_amd.tasks import HumanoidSMPLIM, default_cfg

DEV = "cuda:0"


def T(x, dtype=torch.float32):
    return torch.as_tensor(np.ascontiguousarray(x)).to(device=DEV, dtype=dtype).contiguous()


def N(x):
    return x.detach().cpu().numpy()


def golden_motion_lib(golden_tables):
    return MotionLib(golden_tables, DEV)


def synth_tables(seed=7, num_clips=16, min_frames=60, max_frames=200):
    from vid2player3d_amd import motion_tables

    m = load_baked_model()
    clips = synth.make_clips(seed, num_clips, min_frames, max_frames)
    return motion_tables.build_tables(clips, m.parents, m.local_pos)


def make_task(num_envs, motion_lib, motion_ids=None, sim_overrides=None, **env_overrides):
    env_overrides.setdefault("debug_contacts", 1)  # tests look at the selected contact vertices
    env_overrides.setdefault("body_shape_mismatch", "ignore")  # the golden libraries carry per-clip betas over one baked body on purpose
    cfg = default_cfg(num_envs, motion_lib=motion_lib, **env_overrides)
    cfg["sim"].update(sim_overrides or {})
    if motion_ids is None:
        cfg["env"]["sample_first_motions"] = True
    task = HumanoidSMPLIM(cfg, device_type="cuda", device_id=0)
    if motion_ids is not None:
        # bind envs to given clips (the ids tensor is borrowed by the engine, so edit it in place)
        task._reset_ref_motion_ids.copy_(T(motion_ids, torch.long))
        task._reset_ref_motion_bodies = motion_lib._motion_bodies[task._reset_ref_motion_ids]
    return task


def close(a, b, tol, what="", sens=None, k_sens=16.0):
    """|a - b| <= tol * max(1, max|b|) everywhere (+ k_sens * sens per element: the conditioning of the oracle's own step there, see
    rows_close)."""
    a = np.asarray(a, dtype=np.float64)
    b = np.asarray(b, dtype=np.float64)
    assert a.shape == b.shape, (what, a.shape, b.shape)
    if a.size == 0:
        return
    flat = tol * max(1.0, np.abs(b).max())
    err = np.abs(a - b)
    lim = flat if sens is None else flat + np.minimum(k_sens * np.asarray(sens, dtype=np.float64), SENS_CAP * flat)
    over = err > lim
    use = float((err / np.maximum(lim, 1e-300)).max())
    assert np.isfinite(a).all(), what + ": non-finite values"
    if sens is not None and (err > flat).any():
        print("[close] %s: %d of %d elements need the conditioning term (largest error there = %.1f x sensitivity)"
              % (what, int((err > flat).sum()), err.size, float((err[err > flat] / np.maximum(np.asarray(sens, dtype=np.float64)[err > flat], 1e-300)).max())))
    if _report_only(what):  # A/B of kernel variants: print how much of each tolerance is used instead of asserting
        print("[close] %-40s err %.3e  limit %.3e  used %.3f" % (what, err.max(), flat, use))
        return
    assert not over.any(), "%s: max abs err %.3e, %.2f x its bound (%.1e%s)" % (what, err.max(), use, flat, "" if sens is None else " + %g x sensitivity" % k_sens)


SENS_CAP = 200.0    # the conditioning term never exceeds this many flat bounds (0.04 m/s + 0.1 |ref| on a velocity, 10 N + 0.2 |ref| on a force).
                    # Round 6 (VERDICT r5 #4a): 1000 -> 200; the largest excess over a flat bound that was ever traced to conditioning is ~130 x
                    # (one element of the 4-env epoch test, profiles/r05f_rows.log), 31 x in the 2048 / 16384-env sweeps
SENS_SHARE = 0.02   # share of the envs of a comparison that may need the conditioning term (round 6: 0.04 -> 0.02; measured <= 1.1 % of
                    # 2048 / 16384-env fixtures) ...
SENS_MIN_ENVS = 4   # ... or this many envs, never more than half of them (small fixtures; measured over the whole suite, profiles/r05f_rows_all.log:
                    # at most 3 of 48 - ragdolls late in an epoch -, 2 of 64, 1 of 4; largest use of a bound 0.75)
# Report mode: a TOOL that wants the percentiles of a comparison without its pass / fail (A/B of kernel variants) sets this attribute in its
# own process - `gpu_util.REPORT_ONLY = True` - and every comparison then says so, loudly.  (Until round 5 two environment variables did
# this: a stray export in a CI shell weakened every parity test without a trace.  No environment variable is read any more.)
REPORT_ONLY = False


def _report_only(what):
    if REPORT_ONLY:
        print("[gpu_util] WARNING: REPORT_ONLY is set by the calling tool - '%s' is printed, NOT asserted" % what, flush=True)
    return REPORT_ONLY


def rows_close(a, b, atol, rtol, what, sens=None, k_sens=16.0):
    """Per-element mixed bound |a - b| <= atol + rtol |b| (+ k_sens * sens, axis 0 = env).  `sens` = conditioning of the oracle's own
    step at every element (oracle.phys_oracle.BatchOracle.sensitivity: the largest change of the float64 result under input
    perturbations of float32-rounding size): with it the bound reads "the kernel's result is what the oracle gives for inputs within
    k_sens x float32 rounding".  Prints the 50 / 99 / 100th percentiles of the error and of the share of the bound it uses, the number
    of envs that need the conditioning term and the largest error in units of the sensitivity among them (pytest -s), and returns the
    boolean mask of the ENVS that break the bound somewhere."""
    a = np.asarray(a, dtype=np.float64)
    b = np.asarray(b, dtype=np.float64)
    assert a.shape == b.shape, (what, a.shape, b.shape)
    assert np.isfinite(a).all(), what + ": non-finite values"
    if a.size == 0:
        return np.zeros(a.shape[0], dtype=bool)
    err = np.abs(a - b)
    flat = atol + rtol * np.abs(b)
    # the conditioning term is CAPPED (SENS_CAP x the flat bound; the largest excess over a flat bound that was traced to conditioning: 31 x in
    # the 2048-env sweeps, profiles/r04g_parity_sweep.log, ~130 x at one element of the 4-env epoch test, whose error was 0.2 x its own
    # sensitivity, profiles/r05f_rows.log) - an element with a huge gain does not get an unbounded tolerance -
    # and only a small share of the envs may need it at all (SENS_SHARE; measured 0.15 - 1.1 % of 2048-env fixtures)
    lim = flat if sens is None else flat + np.minimum(k_sens * np.asarray(sens, dtype=np.float64), SENS_CAP * flat)
    use = err / lim
    bad = (use > 1.0).reshape(a.shape[0], -1).any(axis=1)
    if sens is not None:
        n_need = int((err > flat).reshape(a.shape[0], -1).any(axis=1).sum())
        assert _report_only(what + " (share of envs that need the conditioning term)") or n_need <= min(max(SENS_MIN_ENVS, int(SENS_SHARE * a.shape[0])), max(1, a.shape[0] // 2)), "%s: %d of %d envs need the conditioning term (more than %.0f %%): not a conditioning effect" % (what, n_need, a.shape[0], 100 * SENS_SHARE)
    pe, pu = np.percentile(err, [50, 99, 100]), np.percentile(use, [50, 99, 100])
    extra = ""
    if sens is not None:
        over_flat = err > flat
        need = over_flat.reshape(a.shape[0], -1).any(axis=1)
        worst = float((err[over_flat] / np.maximum(np.asarray(sens, dtype=np.float64)[over_flat], 1e-300)).max()) if over_flat.any() else 0.0
        extra = " | envs that need the conditioning term: %d (largest error there = %.1f x sensitivity)" % (int(need.sum()), worst)
    print("[rows] %-34s |err| p50 %.1e p99 %.1e max %.1e | share of (%.0e + %.0e|ref|%s) p50 %.3f p99 %.3f max %.2f | envs over: %d of %d%s"
          % (what, pe[0], pe[1], pe[2], atol, rtol, "" if sens is None else " + %g sens" % k_sens, pu[0], pu[1], pu[2], int(bad.sum()), a.shape[0], extra))
    return bad


# Velocities and forces are judged PER ELEMENT on EVERY env:  |hip - oracle| <= atol + rtol |oracle| + K_SENS * sens,  float32 O(n)
# recursion against float64 dense solve after 4 substeps.  `sens` is the CONDITIONING of the oracle's own step at that element
# (BatchOracle.sensitivity: largest change of the float64 result when its inputs are perturbed by float32 rounding - 2e-7 on positions
# and quaternions, 1e-6 on velocities).  Why it is there (round 4, profiles/r04_parity_*.log, tools/gain_probe.py): the step map of
# this model is piecewise linear but NOT contractive - box friction bounded by the current normal impulse couples the rows
# non-symmetrically - and in ~1 % of the perturbed states of these fixtures one substep multiplies a velocity perturbation by 10^2 and
# more (the float64 oracle does this to itself).  Those envs are exactly the ones that used to miss the flat bound, by the amounts the
# oracle's sensitivity predicts (error / sens 0.1 .. 9 in every one of 78 dumped outliers), in the precise build
# (V2P_LL_STRICT_MATH) and in the env-per-lane kernel as often as in the default build.  No share of the envs is exempt any more.
# Measured (pytest -s prints the percentiles of every comparison): median error 5e-7 .. 2e-6, 99th percentile 1e-5 .. 5e-5.
VEL_ATOL, VEL_RTOL = 2e-4, 5e-4
FORCE_ATOL, FORCE_RTOL = 0.05, 1e-3
POS_ATOL = 2e-5
K_SENS = 16.0   # the kernel's result must be what the oracle gives for inputs within K_SENS x float32 rounding


def assert_none_over(bad, what):
    assert not bad.any(), "%s: %d of %d envs over the per-element bounds (envs %s)" % (what, int(bad.sum()), bad.shape[0], np.nonzero(bad)[0][:8].tolist())


def rows_all(got, ref, what, contact=True, k_sens=K_SENS):
    """Every per-element comparison of one control step; returns the mask of the envs over a bound."""
    S = ref["sens"]
    qs = np.sign(np.sum(got["rb"][..., 3:7] * ref["rb"][..., 3:7], axis=-1, keepdims=True))  # quaternion sign is arbitrary
    bad = rows_close(got["root"][:, :3], ref["root"][:, :3], POS_ATOL, 0.0, what + " root pos", S["root"][:, :3], k_sens)
    bad |= rows_close(got["dpos"], ref["dpos"], 5e-5, 0.0, what + " dof_pos", S["dpos"], k_sens)
    bad |= rows_close(got["rb"][..., :3], ref["rb"][..., :3], POS_ATOL, 0.0, what + " rb pos", S["rb"][..., :3], k_sens)
    bad |= rows_close(got["rb"][..., 3:7] * qs, ref["rb"][..., 3:7], POS_ATOL, 0.0, what + " rb rot", S["rb"][..., 3:7], k_sens)
    bad |= rows_close(got["root"][:, 7:], ref["root"][:, 7:], VEL_ATOL, VEL_RTOL, what + " root vel", S["root"][:, 7:], k_sens)
    bad |= rows_close(got["dvel"], ref["dvel"], VEL_ATOL, VEL_RTOL, what + " dof_vel", S["dvel"], k_sens)
    bad |= rows_close(got["rb"][..., 7:], ref["rb"][..., 7:], VEL_ATOL, VEL_RTOL, what + " rb vel", S["rb"][..., 7:], k_sens)
    bad |= rows_close(got["df"], ref["df"], FORCE_ATOL, FORCE_RTOL, what + " dof force", S["df"], k_sens)
    if contact:
        bad |= rows_close(got["cf"], ref["cf"], FORCE_ATOL, FORCE_RTOL, what + " contact force", S["cf"], k_sens)
    return bad


def _compare(got, ref, what, contact=True):
    assert_none_over(rows_all(got, ref, what, contact), what)
