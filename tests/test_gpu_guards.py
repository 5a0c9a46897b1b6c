"""Stores outside an array and loads of memory nobody wrote - what parity tests cannot see: a stray store lands in the slack hipMalloc
leaves behind an array or in a neighbour that is rewritten before anybody reads it, and a fresh process reads zeros where a long-lived
trainer reads whatever the allocator recycled.

Every case below runs one short script twice: plain, and with guard zones + poison around the engine's own arrays (v2p_debug_guards,
4096 bytes) and 64 guard rows around every tensor the engine borrows from the task (cfg env debug_guard_rows).  The kernels are
deterministic, so the guarded run has an exact expected result - the same bits, step after step - with every zone and guard row intact
(task.check()) and no NaN anywhere (a floating-point array the engine leaves unfilled holds NaN in the guarded run: whoever reads it
before writing it shows up).  The shapes are the smallest at which the indexing can go wrong: one env (half a wave), odd counts, more
than one workgroup of the 256-thread kernels, the hand-over slots of uneven job splits, the recovery path.

Not seen by this: an overrun inside a structure-of-arrays buffer that stays inside its allocation (the batch-independence and oracle
tests are for that), and a read-before-write of an INTEGER array (those are zeroed, not poisoned: a garbage index must not be formed on a
shared GPU).  The second half of the file compares ragged batches with a full one, env by env."""
import warnings

import numpy as np
import pytest
import torch

from tests.gpu_util import DEV, N, T, make_task, synth_tables

pytestmark = pytest.mark.gpu

ZONE, ROWS = 4096, 64
SNAP = ["_rigid_body_state", "_dof_state", "_contact_forces", "dof_force_tensor", "rew_buf", "reset_buf", "obs_buf", "context_feat"]
BALL_SNAP = ["_ball_root_states", "_ball_states_per_sim", "_ball_contact_forces", "_ball_body_contact_force", "_racket_ball_contact_per_sim", "_has_bounce",
             "_has_bounce_now", "_bounce_pos", "_has_racket_ball_contact", "_has_racket_ball_contact_now", "_contact_forces_sum"]


@pytest.fixture(scope="module")
def cache():
    """What several tests of the module share (computed once, left unchanged, released with the module)."""
    c = {}
    yield c
    c.clear()


@pytest.fixture(scope="module")
def mlib():
    from vid2player3d_amd.motion_lib import MotionLib

    return MotionLib(synth_tables(seed=5, num_clips=8, min_frames=60, max_frames=120), DEV)


def _lib():
    from vid2player3d_amd import _lib as L

    return L.load()


def script(task, seed, ball=False, gen_n=None, reset_ids=None, schedule=None, after_first_step=None):
    """Seeded reset of the whole batch, 3 steps, reset of envs {0, n - 1} (reset_ids) + an edited root state pushed for the last of them,
    3 more steps (one through the staged API), check(); the snapshot tensors after every step.  gen_n: draw times and actions for that
    many envs and use the first n rows (two batches of different sizes then see the same numbers env by env)."""
    n = task.num_envs
    gen_n = gen_n or n
    g = torch.Generator(device=DEV)
    g.manual_seed(seed)
    names = SNAP + (BALL_SNAP if ball else [])

    def draw(*shape):
        return torch.rand((gen_n,) + shape, device=DEV, generator=g)[:n].contiguous()

    def normal(*shape):
        return torch.randn((gen_n,) + shape, device=DEV, generator=g)[:n].contiguous()

    def step(staged):
        a = torch.cat([task._target_dof_pos + 0.4 * normal(69), 0.3 * normal(6)], dim=1).contiguous()
        if staged:
            task.pre_physics_step(a); task._physics_step(); task.post_physics_step()
        else:
            task.step(a)
        return {k: N(getattr(task, k)).copy() for k in names if getattr(task, k, None) is not None}  # (_contact_forces_sum is optional)

    task.reset_with_times(None, draw() * 0.8)
    if schedule is not None:
        task.set_schedule(schedule)
    if ball:
        jit = draw(3)
        # served at the players from 2.5 m (test_substep_jobs_are_invisible_with_ball): body hits, racket hits and bounces within the steps
        task.reset_balls(torch.arange(n, device=DEV), task._humanoid_root_states[:, 0:3] + torch.tensor([2.5, 0.0, 0.3], device=DEV) + jit * 0.6,
                         torch.tensor([-20.0, 0.0, 1.0], device=DEV) + (jit - 0.5) * torch.tensor([6.0, 4.0, 4.0], device=DEV),
                         torch.tensor([0.0, -120.0, 0.0], device=DEV).expand(n, 3))
    snaps = [step(False)]
    if after_first_step is not None:
        after_first_step(task)
    snaps += [step(False) for _ in range(2)]
    ids = sorted(set([0, n - 1] if reset_ids is None else reset_ids))
    ids_t = torch.tensor(ids, device=DEV, dtype=torch.long)
    task.reset_with_times(ids_t, (draw() * 0.8)[ids_t].contiguous())
    last = ids[-1]
    task._humanoid_root_states[last, 2] += 0.05
    task._humanoid_root_states[last, 7:10] += torch.tensor([0.3, -0.2, 0.1], device=DEV)
    task._reset_env_tensors(ids_t[-1:].contiguous())
    snaps += [step(k == 1) for k in range(3)]
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")  # (a recovery count that grows is warned about: the recovery case wants it to)
        task.check()
    return snaps


def plain_and_guarded(make, seed, poisons, expect_recoveries=False, **how):
    """make(**env) -> task.  Runs the script plain and guarded, asserts what the module's head says and returns the plain snapshots
    (one {tensor name: array} per step)."""
    L = _lib()
    runs = []
    for guarded in (False, True):
        assert L.v2p_debug_guards(ZONE if guarded else 0) == 0
        try:
            task = make(debug_guard_rows=ROWS) if guarded else make()
            try:
                snaps = script(task, seed, **how)
                # the guard must be armed: a guarded run that silently ran unguarded fails here
                arrays, poisoned = task.guard_counts()
                offset = task.obs_buf.data_ptr() - task.obs_buf.untyped_storage().data_ptr()
                if guarded:
                    assert arrays >= 8 and offset == ROWS * task.obs_buf.shape[1] * 4, (arrays, offset)
                    assert poisoned >= poisons, "%d float array(s) the engine leaves unfilled were expected to be poisoned, %d were" % (poisons, poisoned)
                else:
                    assert (arrays, poisoned, offset) == (0, 0, 0)
                if expect_recoveries:
                    assert task.job_recoveries() > 0, "the fixture must exercise the recovery path"
            finally:
                task.close()
        finally:
            L.v2p_debug_guards(0)  # no other test module runs guarded by accident
        runs.append(snaps)
    for k, (sa, sb) in enumerate(zip(*runs)):
        assert list(sa) == list(sb) and len(sa) >= len(SNAP)
        for name in sa:
            x, y = sa[name], sb[name]
            assert np.isfinite(y.astype(np.float64)).all(), "step %d, %s: non-finite values in the guarded run (a read of memory nobody wrote?)" % (k, name)
            assert np.isfinite(x.astype(np.float64)).all(), "step %d, %s: non-finite values" % (k, name)
            assert np.array_equal(x, y), "step %d, %s: %d of %d values of the guarded run differ from the plain run" % (k, name, int((x != y).sum()), x.size)
    return runs[0]


# ---------------------------------------------------------------------------------------------------------------- the engine's own tests
def test_selftest_and_refusals():
    L = _lib()
    assert L.v2p_debug_guards_selftest(0) == 0, L.v2p_last_error()
    assert L.v2p_debug_guards(0) == 0, "the self-test must leave the process-wide setting as it found it"
    for bad in (100, -256, 255, (1 << 20) + 256):
        assert L.v2p_debug_guards(bad) == -1 and b"v2p_debug_guards" in L.v2p_last_error()
    assert L.v2p_debug_guards(512) == 0 and L.v2p_debug_guards(0) == 512  # (the previous value comes back)


# ---------------------------------------------------------------------------------------------------------------- the humanoid alone
# (a launch of one env pair is never cut: jobs from 3 envs on)
@pytest.mark.parametrize("n,build,jobs", [(n, b, j) for n in (1, 2, 3, 65, 257) for b in (1, 2) for j in (0, 2) if not (j and n < 3)])
def test_guarded_run_is_the_plain_run(mlib, n, build, jobs):
    plain_and_guarded(lambda **e: make_task(n, mlib, kernel_build=build, substep_jobs=jobs, **e), seed=41 + n, poisons=1 if jobs else 0)


def _limits_model():
    from vid2player3d_amd.model import load_baked_model
    from vid2player3d_amd.racket import with_racket

    return with_racket(load_baked_model())[0]


VARIANTS = {
    "tgs": (dict(contact_solver="tgs"), {}),
    "no contacts": (dict(enable_contact=False), {}),
    "velocity friction frame": (dict(friction_frame="velocity"), {}),
    "heavy x light pairs": (dict(pair_mix_permille=500), {}),
    "every substep's contact ids": (dict(debug_contacts=2), {}),
    "env per lane (out, ws)": ({}, dict(schedule="env_per_lane")),
    "limits pgs": (dict(joint_limits=True, body_model=_limits_model), {}),
    "limits tgs": (dict(joint_limits=True, contact_solver="tgs", body_model=_limits_model), {}),
}


@pytest.mark.parametrize("what", list(VARIANTS))
def test_guarded_run_is_the_plain_run_in_every_instantiation(mlib, what):
    env, how = VARIANTS[what]
    env = {k: (v() if callable(v) else v) for k, v in env.items()}
    jobs = 0 if how else 2
    plain_and_guarded(lambda **e: make_task(65, mlib, substep_jobs=jobs, **env, **e), seed=7, poisons=1 if jobs else 0, **how)


def test_guarded_hand_over_slots_of_an_uneven_split(mlib):
    """12 substeps in jobs of 5 + 5 + 2: three jobs per cut pair.  (A job writes the slot of its JOB index, and a pair's last job writes none:
    slots 0 and 1 of the 11; the slots up to nsub - 2 are the next test's.)"""
    plain_and_guarded(lambda **e: make_task(65, mlib, sim_overrides={"substeps": 6}, substep_jobs=2, job_len=5, **e), seed=9, poisons=1)


@pytest.mark.parametrize("n,substeps", [(3, 2), (65, 2), (65, 6)])
def test_guarded_hand_over_slots_up_to_the_last(mlib, n, substeps):
    """job_hand is [nsub - 1][N][224 floats]; job j of a cut pair writes slot j unless it is the pair's last.  The engine's own plan for the
    humanoid makes the first job two substeps long (nsub = 4: three jobs, slots 0 and 1 - the last slot is never written), so the array's
    END is reached only with jobs of equal length 1: cfg env job_lead = -1 (and job_len = 1) gives nsub jobs per pair and stores into
    every slot up to nsub - 2, at 4 and at 12 substeps per control step.  At 3 envs no pair is kept whole (2 pairs x 60 / 1000 = 0), so
    env N - 1 writes the last 896 bytes of the array for certain."""
    plain_and_guarded(lambda **e: make_task(n, mlib, sim_overrides={"substeps": substeps}, substep_jobs=2, job_len=1, job_lead=-1, **e), seed=11 + n, poisons=1)


def test_guarded_recovery_path(mlib):
    """job_timeout_spins < 0: a job whose predecessor is not done at its first look recomputes while the predecessor still writes."""
    plain_and_guarded(lambda **e: make_task(67, mlib, substep_jobs=2, job_timeout_spins=-1, **e), seed=13, poisons=1, expect_recoveries=True)


def test_guarded_per_env_body_shapes(mlib):
    """5 envs over 3 shapes: the last env has a shape of its own."""
    from vid2player3d_amd import body_shapes
    from vid2player3d_amd.model import load_baked_model

    shapes = body_shapes.synthetic_shape_family(load_baked_model(), 3, seed=21, device=DEV)
    plain_and_guarded(lambda **e: make_task(5, mlib, body_model=shapes, motion_shape_ids=np.array([0, 0, 1, 1, 2, 0, 0, 0]), substep_jobs=2, **e), seed=15, poisons=1)


# ---------------------------------------------------------------------------------------------------------------- racket + ball
@pytest.mark.parametrize("jobs", [0, 2])
@pytest.mark.parametrize("solver", ["pgs", "tgs"])
@pytest.mark.parametrize("n", [3, 35])
def test_guarded_racket_ball(mlib, n, solver, jobs):
    from tests.test_gpu_racket_ball import make_rb_task

    # (contact_part, the per-call partial sums of the links' contact forces, is a float array the engine leaves unfilled: poisoned)
    plain_and_guarded(lambda **e: make_rb_task(n, mlib, contact_solver=solver, substep_jobs=jobs, debug_contacts=0, **e), seed=23, poisons=2 if jobs else 1, ball=True)


def test_guarded_racket_ball_without_body_contacts(mlib):
    from tests.test_gpu_racket_ball import make_rb_task

    plain_and_guarded(lambda **e: make_rb_task(35, mlib, ball_body_contacts=False, substep_jobs=2, debug_contacts=0, **e), seed=27, poisons=2, ball=True)


def test_guarded_ball_attached_again_after_the_first_step(mlib):
    """The task is created without `_contact_forces_sum` and starts keeping it after the first step: the ball is attached a second time and
    the engine allocates contact_part (a float array it leaves unfilled) in the middle of a run."""
    from tests.test_gpu_racket_ball import make_rb_task

    def attach(task):  # (what the constructor does when cfg env contact_forces_sum is set, between two steps)
        assert task._contact_forces_sum is None
        torch.cuda.synchronize()
        task._contact_forces_sum = task._buffer("_contact_forces_sum", (task.num_envs, 24, 3))
        task._attach_ball()

    snaps = plain_and_guarded(lambda **e: make_rb_task(35, mlib, contact_forces_sum=False, substep_jobs=2, debug_contacts=0, **e), seed=31, poisons=2, ball=True,
                              after_first_step=attach)
    assert "_contact_forces_sum" not in snaps[0] and all("_contact_forces_sum" in s for s in snaps[1:])
    assert any(np.abs(s["_contact_forces_sum"]).max() > 0 for s in snaps[1:]), "the fixture must produce contact forces"


def test_guarded_mixed_players(mlib):
    from tests.test_gpu_mixed_players import make_pair_task

    # (env i is player i % 2: the task refuses an odd count, so 6 - three waves, each with one env of either player - stands for "5")
    plain_and_guarded(lambda **e: make_pair_task(6, mlib, ["nadal", "federer"], contact_solver="tgs", substep_jobs=2, debug_contacts=0, **e), seed=29,
                      poisons=2, ball=True)


# ---------------------------------------------------------------------------------------------------------------- ragged batches against a full one
FULL = 66


def _ragged_run(mlib, n, pair):
    ids = np.arange(FULL) % 8
    task = make_task(n, mlib, motion_ids=ids[:n], pair_envs_by_load=pair, kernel_build=1)
    try:
        return script(task, seed=37, gen_n=FULL, reset_ids=[0])
    finally:
        task.close()


@pytest.mark.parametrize("pair", [False, True])
@pytest.mark.parametrize("n", [1, 3, 65])
def test_ragged_batch_equals_the_first_envs_of_a_full_one(mlib, cache, n, pair):
    """Env i of an n-env batch (half of the last wave has no env when n is odd) == env i of a 66-env batch bound to the same clips, with the
    same times and actions: every snapshot tensor, bit for bit, over 6 steps."""
    if ("full", pair) not in cache:
        cache["full", pair] = _ragged_run(mlib, FULL, pair)  # (computed once per pairing and left unchanged)
    full = cache["full", pair]
    got = _ragged_run(mlib, n, pair)
    for k, (sa, sb) in enumerate(zip(got, full)):
        assert list(sa) == SNAP == list(sb)
        for name in SNAP:
            x, y = sa[name], sb[name]
            y = y.reshape((FULL, -1))[:n].reshape(x.shape)  # (_dof_state / _rigid_body_state are [n x links, ...]: env-major)
            assert np.isfinite(x.astype(np.float64)).all(), (k, name)
            assert np.array_equal(x, y), "step %d, %s: %d of %d values of the %d-env batch differ from the same envs of the %d-env batch" % (
                k, name, int((x != y).sum()), x.size, n, FULL)


# ---------------------------------------------------------------------------------------------------------------- stand-alone entries at block and wave tails
# n = 1, 7, 9, 257: below / above the 8 envs and the 4 waves of a workgroup, above its 256 threads.  Inputs are seeded draws of the shapes
# oracle/gen_golden.py draws (gen_task_ops); outputs live between guard rows (tests/guarded.py) and start out as NaN / 0x5A, so an element
# the kernel leaves unwritten fails the comparison too.  References: the numpy statements of oracle/task_oracle.py, at the tolerances
# tests/test_gpu_task_ops.py uses for the same quantities.
TAILS = [1, 7, 9, 257]


def _task_inputs(cache, n):
    if ("inputs", n) in cache:
        return cache["inputs", n]
    from vid2player3d_amd import synth

    rng = np.random.default_rng(500 + n)
    f32 = np.float32

    def rand_quat(*shape):
        q = rng.normal(size=shape + (4,))
        return (q / np.linalg.norm(q, axis=-1, keepdims=True)).astype(f32)

    g = {}
    g["body_pos"] = rng.normal(0, 0.5, size=(n, 24, 3)).astype(f32)
    g["body_pos"][..., 2] += 1.0
    g["body_rot"] = rand_quat(n, 24)
    g["tgt_pos"] = (g["body_pos"] + rng.normal(0, 0.05, size=(n, 24, 3))).astype(f32)
    dq = synth._quat_from_rotvec(rng.normal(0, 0.08, size=(n, 24, 3)))
    g["tgt_rot"] = synth._quat_mul(dq, g["body_rot"].astype(np.float64)).astype(f32)
    g["tgt_rot"][n - 1, :12] = -g["body_rot"][n - 1, :12]  # the LAST env: antipodal representation / identical rotations (acos(1) branch)
    g["tgt_rot"][n - 1, 12:] = g["body_rot"][n - 1, 12:]
    g["dof_pos"] = rng.normal(0, 0.6, size=(n, 69)).astype(f32)
    g["dof_pos"][n - 1, :9] = 0.0  # zero exp-map
    g["dof_vel"] = rng.normal(0, 2.0, size=(n, 69)).astype(f32)
    g["tgt_dof_pos"] = (g["dof_pos"] + rng.normal(0, 0.1, size=(n, 69))).astype(f32)
    g["tgt_dof_vel"] = (g["dof_vel"] + rng.normal(0, 0.5, size=(n, 69))).astype(f32)
    g["body_vel"] = rng.normal(0, 1.0, size=(n, 24, 3)).astype(f32)
    g["body_ang_vel"] = rng.normal(0, 2.0, size=(n, 24, 3)).astype(f32)
    g["weights"] = np.ones(24, dtype=f32)
    g["weights"][[13, 18, 23]] = [2.0, 1.5, 1.5]
    g["motion_bodies"] = rng.normal(size=(n, 11)).astype(f32)
    g["rn_mean"] = rng.normal(0, 0.5, size=734).astype(f32)
    g["rn_std"] = rng.uniform(0.5, 2.0, size=734).astype(f32)
    g["progress"] = rng.integers(0, 6, size=n).astype(np.int64)
    g["progress"][n - 1] = 299
    g["heights"] = np.full(24, -0.5, dtype=f32)
    g["heights"][13] = 1.0
    g["rb"] = g["body_pos"].copy()
    g["rb"][:, 13, 2] = rng.uniform(0.8, 1.6, size=n)  # head height straddles the 1.0 m threshold
    g["rb"][n // 2, 7, 2] = -0.7                       # contact body below its threshold: ignored
    g["cur_t"] = rng.uniform(0.0, 3.0, size=n).astype(f32)
    g["clip_len"] = rng.uniform(1.0, 4.0, size=n).astype(f32)
    cache["inputs", n] = g
    return g


@pytest.mark.parametrize("n", TAILS)
def test_reward_at_the_tails(cache, n):
    import ctypes as C

    from oracle import task_oracle as O
    from tests.guarded import Guarded
    from tests.gpu_util import close
    from vid2player3d_amd import _lib

    g, G = _task_inputs(cache, n), Guarded(DEV)
    rew, sub = G.empty("rew", (n,)), G.empty("sub_rewards", (n, 4))
    keys = ("body_pos", "body_rot", "tgt_pos", "tgt_rot", "dof_pos", "dof_vel", "tgt_dof_pos", "tgt_dof_vel")
    args = [T(g[k]) for k in keys]
    w, s = (C.c_float * 24)(*g["weights"].tolist()), (C.c_float * 8)(60, 0.2, 100, 40, 0.6, 0.1, 0.2, 0.1)
    _lib.check(_lib.load().v2p_reward(n, *[_lib.ptr(a) for a in args], w, s, _lib.ptr(rew), _lib.ptr(sub), None), "v2p_reward")
    G.check()
    want_rew, want_sub = O.compute_humanoid_reward(*[g[k] for k in keys], g["weights"])
    close(N(sub)[:, :3], want_sub[:, :3], 5e-6, "sub[dof,vel,pos]")
    close(N(sub)[:, 3], want_sub[:, 3], 2e-4, "sub[rot]")
    close(N(rew), want_rew, 5e-5, "reward")


@pytest.mark.parametrize("n", TAILS)
def test_reset_flags_at_the_tails(cache, n):
    import ctypes as C

    from oracle import task_oracle as O
    from tests.guarded import Guarded
    from vid2player3d_amd import _lib

    g, G = _task_inputs(cache, n), Guarded(DEV)
    rst, term = G.empty("reset", (n,), torch.long), G.empty("terminate", (n,), torch.long)
    h = g["heights"].copy()
    h[[7, 3]] = -np.inf
    prog, rb, ct, cl = T(g["progress"], torch.long), T(g["rb"]), T(g["cur_t"]), T(g["clip_len"])
    _lib.check(_lib.load().v2p_reset_flags(n, _lib.ptr(prog), _lib.ptr(rb), (C.c_float * 24)(*h.tolist()), _lib.ptr(ct), _lib.ptr(cl), 300.0, 1,
                                           _lib.ptr(rst), _lib.ptr(term), None), "v2p_reset_flags")
    G.check()
    want_rst, want_term = O.compute_humanoid_reset(g["progress"], g["rb"], g["heights"], g["cur_t"], g["clip_len"])
    assert np.array_equal(N(rst), want_rst) and np.array_equal(N(term), want_term)


@pytest.mark.parametrize("norm", [False, True])
@pytest.mark.parametrize("n", TAILS)
def test_obs_imitation_at_the_tails(cache, n, norm):
    from oracle import task_oracle as O
    from tests.guarded import Guarded
    from tests.gpu_util import close
    from vid2player3d_amd import _lib

    g, G = _task_inputs(cache, n), Guarded(DEV)
    obs = G.empty("obs734", (n, 734))
    keys = ("body_pos", "body_rot", "tgt_pos", "tgt_rot", "dof_pos", "dof_vel", "tgt_dof_pos", "body_vel", "body_ang_vel", "motion_bodies")
    args = [T(g[k]) for k in keys]
    mean, std = (T(g["rn_mean"]), T(g["rn_std"])) if norm else (None, None)
    _lib.check(_lib.load().v2p_obs_imitation(n, *[_lib.ptr(a) for a in args], _lib.ptr(mean), _lib.ptr(std), 5.0 if norm else 0.0, _lib.ptr(obs), None), "v2p_obs_imitation")
    G.check()
    want = O.obs_imitation_734(*[g[k] for k in keys])
    if norm:
        close(N(obs), O.running_norm_eval(want, g["rn_mean"], g["rn_std"], 5.0), 2e-5, "obs734 normalised")
    else:
        close(N(obs), want, 5e-6, "obs734")


@pytest.mark.parametrize("n", TAILS)
def test_gae_at_the_tails(n):
    from oracle import task_oracle as O
    from tests.guarded import Guarded
    from tests.gpu_util import close
    from vid2player3d_amd import _lib

    rng = np.random.default_rng(900 + n)
    t = 5
    fd_h = (rng.uniform(size=(t, n)) < 0.2).astype(np.float32)
    va_h, rw_h, nv_h = (rng.normal(size=(t, n, 1)).astype(np.float32) for _ in range(3))
    G = Guarded(DEV)
    # (the output is [T, N, 1]: the whole block lies between 64 x N guard elements on either side)
    adv = G.empty("advs", (t, n, 1))
    fd, va, rw, nv = T(fd_h), T(va_h), T(rw_h), T(nv_h)
    _lib.check(_lib.load().v2p_gae(t, n, _lib.ptr(fd), _lib.ptr(va), _lib.ptr(rw), _lib.ptr(nv), 0.99, 0.95, _lib.ptr(adv), None), "v2p_gae")
    G.check()
    close(N(adv), O.discount_values(fd_h, va_h, rw_h, nv_h, 0.99, 0.95), 1e-5, "gae %dx%d" % (t, n))


@pytest.mark.parametrize("ctx_dim", [378, 402])
@pytest.mark.parametrize("n", TAILS)
def test_obs_imitation_packed_at_the_tails(cache, n, ctx_dim):
    """n envs x 3 steps: row e * 3 + k pairs with context frame pad + k of env e; the other frames (and floats 378 .. 401 of a 402-wide
    frame) hold garbage that must not be read."""
    from oracle import task_oracle as O
    from tests.guarded import Guarded
    from tests.gpu_util import close
    from vid2player3d_amd import _lib

    steps, pad, frames = 3, 8, 48
    rows = n * steps
    g, G = _task_inputs(cache, rows), Guarded(DEV)
    obs = np.concatenate([g["body_pos"].reshape(rows, 72), g["body_rot"].reshape(rows, 96), g["dof_pos"], g["dof_vel"], g["body_vel"].reshape(rows, 72),
                          g["body_ang_vel"].reshape(rows, 72), g["motion_bodies"]], axis=1).astype(np.float32)
    frame = np.concatenate([g["tgt_pos"].reshape(rows, 72), g["tgt_rot"].reshape(rows, 96), g["tgt_dof_pos"]], axis=1).astype(np.float32)
    ctx = np.random.default_rng(n).normal(size=(n, frames, ctx_dim)).astype(np.float32)
    ctx[:, pad:pad + steps, :237] = frame.reshape(n, steps, 237)
    out = G.empty("obs734", (rows, 734))
    o, c, mean, std = T(obs), T(ctx), T(g["rn_mean"]), T(g["rn_std"])
    L = _lib.load()
    keys = ("body_pos", "body_rot", "tgt_pos", "tgt_rot", "dof_pos", "dof_vel", "tgt_dof_pos", "body_vel", "body_ang_vel", "motion_bodies")
    want = O.obs_imitation_734(*[g[k] for k in keys])
    for norm in (False, True):
        m, s, clip = (_lib.ptr(mean), _lib.ptr(std), 5.0) if norm else (None, None, 0.0)
        out.fill_(float("nan"))
        if ctx_dim == 378:
            _lib.check(L.v2p_obs_imitation_packed(rows, steps, _lib.ptr(o), _lib.ptr(c), frames, pad, m, s, clip, _lib.ptr(out), None), "v2p_obs_imitation_packed")
        else:
            _lib.check(L.v2p_obs_imitation_packed_w(rows, steps, _lib.ptr(o), _lib.ptr(c), frames, ctx_dim, pad, m, s, clip, _lib.ptr(out), None), "v2p_obs_imitation_packed_w")
        G.check()
        if norm:
            close(N(out), O.running_norm_eval(want, g["rn_mean"], g["rn_std"], 5.0), 2e-5, "packed normalised")
        else:
            close(N(out), want, 5e-6, "packed")


@pytest.mark.parametrize("record", [False, True])
@pytest.mark.parametrize("n", TAILS)
def test_policy_head_at_the_tails(n, record):
    """One wave per env, four per workgroup.  The float64 statement (im_network_builder.py:219-228, im_models.py:45-48): m = mu + the context
    frame's dof_pos (first 69), sigma = exp(logstd), a = m + sigma x noise, neglogp = 0.5 sum(((a - m) / sigma)^2) + 0.5 x 75 log(2 pi) + sum(logstd).
    Bounds from float32 arithmetic, relative to the largest value: m is one rounded sum (2^-24 -> 2e-7 asked); a one expf (2 ulp), a product
    and a sum (1e-6); neglogp is evaluated, like the reference evaluates it, on the float32 action, mean and sigma that were returned - what is
    left is the rounding of 75 quotients, squares and their sum, below (75 + 4) x 2^-24 = 4.7e-6 of the result (1e-5 asked)."""
    from tests.guarded import Guarded
    from tests.gpu_util import close
    from vid2player3d_amd import _lib

    rng = np.random.default_rng(700 + n)
    frames, frame = 48, 8 + 5
    mu0 = rng.normal(0, 0.5, size=(n, 75)).astype(np.float32)
    ctx = rng.normal(size=(n, frames, 378)).astype(np.float32)
    logstd = rng.uniform(-2.0, -0.5, size=75).astype(np.float32)
    noise = rng.normal(size=(n, 75)).astype(np.float32)
    G = Guarded(DEV)
    mu, action, sigma, nlp = G.empty("mu", (n, 75)), G.empty("action", (n, 75)), G.empty("sigma", (n, 75)), G.empty("neglogp", (n,))
    mu.copy_(T(mu0))
    c, ls, nz = T(ctx), T(logstd), T(noise)
    L = _lib.load()
    if record:
        a_row, mu_row = G.empty("action_row", (n, 75)), G.empty("mu_row", (n, 75))
        _lib.check(L.v2p_policy_head_record(n, _lib.ptr(mu), _lib.ptr(c), frames, frame, _lib.ptr(ls), _lib.ptr(nz), _lib.ptr(action), _lib.ptr(sigma), _lib.ptr(nlp),
                                            _lib.ptr(a_row), _lib.ptr(mu_row), None), "v2p_policy_head_record")
    else:
        _lib.check(L.v2p_policy_head(n, _lib.ptr(mu), _lib.ptr(c), frames, frame, _lib.ptr(ls), _lib.ptr(nz), _lib.ptr(action), _lib.ptr(sigma), _lib.ptr(nlp), None),
                   "v2p_policy_head")
    G.check()
    m64 = mu0.astype(np.float64)
    m64[:, :69] += ctx[:, frame, 168:237]
    s64 = np.broadcast_to(np.exp(logstd.astype(np.float64)), (n, 75))
    close(N(mu), m64, 2e-7, "residual mean")
    close(N(sigma), s64, 1e-6, "sigma")
    close(N(action), m64 + s64 * noise, 1e-6, "action")
    z = (N(action).astype(np.float64) - N(mu)) / N(sigma)
    close(N(nlp), 0.5 * np.sum(z * z, axis=1) + 0.5 * 75 * np.log(2 * np.pi) + logstd.astype(np.float64).sum(), 1e-5, "neglogp")
    if record:
        assert torch.equal(a_row, action) and torch.equal(mu_row, mu)


@pytest.mark.parametrize("absent", ["values_row", "next_values_row"])
@pytest.mark.parametrize("n", TAILS)
def test_value_record_at_the_tails(n, absent):
    """im_agent.py:292-303, 355, 398 in float64: y = sqrt(var + eps) x clamp(x, -5, 5) + mean, next = y x (1 - terminated).  Float32: the
    rounded variance and mean, a square root, a product and a sum - a few 2^-24 of the largest value (2e-6 asked)."""
    from tests.guarded import Guarded
    from tests.gpu_util import close
    from vid2player3d_amd import _lib

    rng = np.random.default_rng(800 + n)
    x = rng.normal(0, 3.0, size=n).astype(np.float32)  # (some beyond the clamp at +-5)
    x[n - 1] = 7.5
    term = (rng.uniform(size=n) < 0.3).astype(np.float32)
    mean, var, eps = np.array([1.25]), np.array([3.7]), 1e-5
    G = Guarded(DEV)
    values = None if absent == "values_row" else G.empty("values_row", (n,))
    nxt = None if absent == "next_values_row" else G.empty("next_values_row", (n,))
    xd, td, md, vd = T(x), T(term), T(mean, torch.float64), T(var, torch.float64)
    _lib.check(_lib.load().v2p_value_record(n, _lib.ptr(xd), _lib.ptr(md), _lib.ptr(vd), eps, None if nxt is None else _lib.ptr(td), _lib.ptr(values), _lib.ptr(nxt), None),
               "v2p_value_record")
    G.check()
    y = np.sqrt(var[0] + eps) * np.clip(x.astype(np.float64), -5, 5) + mean[0]
    if values is not None:
        close(N(values), y, 2e-6, "values")
    if nxt is not None:
        close(N(nxt), y * (1 - term), 2e-6, "next values")


@pytest.mark.parametrize("q", TAILS)
def test_motion_state_at_the_tails(cache, q):
    """MotionLib.get_motion_state allocates its nine outputs itself, so they cannot lie between guard rows: the tail sizes against the numpy
    statement only, at test_gpu_task_ops.py's tolerance."""
    from oracle import task_oracle as O
    from tests.gpu_util import close
    from vid2player3d_amd.motion_lib import MotionLib

    if "tabs" not in cache:
        cache["tabs"] = synth_tables(seed=11, num_clips=24)
        cache["lib"] = MotionLib(cache["tabs"], DEV)
    tabs, lib = cache["tabs"], cache["lib"]
    rng = np.random.default_rng(q)
    ids = rng.integers(0, 24, size=q)
    times = (rng.uniform(-0.05, 1.1, size=q) * tabs["motion_lengths"][ids]).astype(np.float32)
    res = lib.get_motion_state(T(ids, torch.long), T(times), return_rigid_body=True, adjust_height=True, ground_tolerance=0.01)
    for name, r, o in zip(O.MOTION_STATE_NAMES, res, O.get_motion_state(tabs, ids, times, True, 0.01)):
        close(N(r), o, 5e-6, name)
