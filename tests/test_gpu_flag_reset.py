"""GPU checks of the controller's reset by flags: every flagged entry against its id-list sibling called with ids = nonzero(flags), bit
for bit on every buffer, between the guard rows of tests/guarded.py; the kernel's own draw against the numpy statement; the controller's
`reset_by_flags()` against `reset(done ids)` step by step; the agent's `reset_mode = 'flags'` against 'ids'; and that a 'flags' rollout
makes no host read."""
import traceback

import numpy as np
import pytest
import torch

from tests import flag_reset_fixture as FF
from tests import mvae_fixture as MF
from tests import mvae_target_fixture as TX
from tests.guarded import Guarded
from vid2player3d_amd import device_rng as R
from vid2player3d_amd import mvae
from vid2player3d_amd import mvae_target as mt

gpu = pytest.mark.gpu
DEV = FF.DEV
SIZES = [1, 7, 8, 9, 67]  # one env, the tails of the 4- and 8-env workgroups, more than one workgroup
i64 = torch.int64


def B(t):
    """the bytes of a tensor"""
    return t.detach().contiguous().cpu().view(torch.uint8).numpy().copy()


def random_bits(rng, shape, dtype):
    """random bits of a dtype (floats: any pattern, NaNs and infinities included)"""
    if dtype == np.float32:
        return rng.integers(0, 2 ** 32, shape, dtype=np.uint32).view(np.float32)
    return rng.integers(-5, 6, shape).astype(dtype)


def assert_same_bytes(got, want, what):
    for k in want:
        assert np.array_equal(got[k], want[k]), "%s: %s differs" % (what, k)


# ------------------------------------------------------------------------------------------------------------------ the generator
class PlayerCase:
    """One player of n envs in evaluation mode (every output is written) whose state, initial frames, flags and start table sit between
    guard rows; `run` loads the same random bits, resets by ids or by flags and returns the bytes of every state tensor."""

    def __init__(self, n, cfg=None):
        e = MF.edge_inputs()
        w, avg, std = MF.weights()
        self.n, self.e = n, e
        self.p = mvae.MotionVAEPlayer(dict({"player": "federer", "righthand": True, "add_residual_dof": "euler", "seed": FF.SEED}, **(cfg or {})), n, w, avg, std, e["init"][:n],
                                      e["bind"], False, DEV)
        rng = np.random.default_rng(100 + n)
        self.s0 = {k: random_bits(rng, tuple(getattr(self.p, "_" + k).shape), np.float32 if getattr(self.p, "_" + k).dtype == torch.float32 else np.int64)
                   for k in mvae.STATE_NAMES}
        self.xy = e["xy"][:n]

    def run(self, flags, how, xy="table", call=None):
        g, p = Guarded(DEV), self.p
        for k, x in self.s0.items():
            setattr(p, "_" + k, g.of(k, x))
        p._init_data = g.of("init_data", self.e["init"][:self.n])
        f = g.of("flags", flags, dtype=i64)
        table = g.of("root_xy", self.xy) if xy == "table" else None
        if call is not None:
            p._reset_calls = call
        if how == "flags":
            p.reset_flagged(f, table)
        else:
            ids = torch.as_tensor(np.flatnonzero(flags), device=DEV)
            p.reset(ids, table[ids])
        g.check()
        assert np.array_equal(B(f), B(torch.as_tensor(flags))), "the flags were written"
        return {k: B(getattr(p, "_" + k)) for k in mvae.STATE_NAMES}


@pytest.fixture(scope="module")
def player_cases():
    cache = {}
    return lambda n: cache.setdefault(n, PlayerCase(n))


@gpu
@pytest.mark.parametrize("n", SIZES)
def test_generator_reset_by_flags_equals_the_reset_by_ids(n, player_cases):
    c = player_cases(n)
    for name, flags in FF.flag_patterns(n).items():
        what = "%d envs, flags %s" % (n, name)
        got = c.run(flags, "flags")
        assert_same_bytes(got, c.run(flags, "ids"), what)
        assert_same_bytes(c.run(flags, "flags"), got, what + ", second run")
        keep = flags == 0
        for k, x in c.s0.items():
            row = lambda a: a.reshape(n, -1)
            assert np.array_equal(row(got[k])[keep], row(B(torch.as_tensor(x)))[keep]), "%s: %s of an env that is not flagged was written" % (what, k)
        if flags.any():
            assert not np.array_equal(got["root_pos"], B(torch.as_tensor(c.s0["root_pos"]))), what + ": nothing was reset"


@gpu
@pytest.mark.parametrize("n", SIZES)
def test_generator_draws_its_own_start_as_the_statement_has_it(n, player_cases):
    c = player_cases(n)
    _, avg, std = MF.weights()
    patterns = FF.flag_patterns(n)
    call = 2 ** 32 + 7
    want_xy = R.root_xy_reference(FF.SEED, call, n)
    runs = {}
    for name in ("all", "alternating", "values_2_and_minus_1", "last"):
        flags = patterns[name]
        got = c.run(flags, "flags", xy=None, call=call)
        assert c.p._reset_calls == call + 1, "the call counter advances by one per launch that draws"
        runs[name] = got
        up = flags != 0
        root = got["root_pos"].view(np.float32).reshape(n, 3)
        assert np.array_equal(root[up, :2], want_xy[up]), "%d envs, flags %s: the start is not the statement's draw" % (n, name)
        # the whole result: the same kernel fed the statement's draw as a table (itself equal to the id-list sibling, above)
        saved, c.xy = c.xy, want_xy
        assert_same_bytes(got, c.run(flags, "flags"), "%d envs, flags %s: own draw against the statement's table" % (n, name))
        c.xy = saved
    # an env's result does not change when other envs' flags change
    for name in ("alternating", "values_2_and_minus_1", "last"):
        up = patterns[name] != 0
        for k in mvae.STATE_NAMES:
            assert np.array_equal(runs[name][k].reshape(n, -1)[up], runs["all"][k].reshape(n, -1)[up]), "%d envs: %s of an env depends on the other envs' flags (%s)" % (n, k, name)
    assert c.run(patterns["all"], "flags", xy=None, call=call + 1)["root_pos"].tobytes() != runs["all"]["root_pos"].tobytes(), "another call draws the same start"
    # the numpy statement of the whole reset on the statement's draw, within the recorded scatter of the id-list reset (float libraries differ)
    zero = {k: np.zeros_like(x) for k, x in c.s0.items()}
    args = (c.p.settings, avg, std, zero, patterns["all"], c.e["init"][:n], want_xy, c.e["bind"])
    want, want64 = mvae.mvae_reset_flagged_reference(*args), mvae.mvae_reset_flagged_reference(*args, dt=np.float64)
    sure = MF.well_conditioned(want, want64, MF.scatter_of(MF.golden(), "reset"))
    got = {k: runs["all"][k].view(np.float32 if c.s0[k].dtype == np.float32 else np.int64).reshape(c.s0[k].shape) for k in mvae.STATE_NAMES}
    MF.assert_state(got, {k: x for k, x in want.items() if k != "phase_pred"}, MF.scatter_of(MF.golden(), "reset"), "%d envs, own draw" % n, rows=np.nonzero(sure)[0])


@gpu
def test_generator_takes_the_centre_when_evaluating_in_a_test_mode():
    c = PlayerCase(9, {"test_mode": "fixed"})
    assert c.p.root_rule() == "centre" and PlayerCase(1).p.root_rule() == "draw"
    flags = FF.flag_patterns(9)["alternating"]
    got = c.run(flags, "flags", xy=None)
    root = got["root_pos"].view(np.float32).reshape(9, 3)
    assert (root[flags != 0, :2] == np.array([0.0, -13.0], np.float32)).all()
    saved, c.xy = c.xy, np.tile(np.array([0.0, -13.0], np.float32), (9, 1))
    assert_same_bytes(got, c.run(flags, "ids"), "the centre against the id-list reset given the centre")
    c.xy = saved


# ------------------------------------------------------------------------------------------------------------------ the target
def target_case(v, n, flags, how):
    g, tx = Guarded(DEV), TX.golden()
    st, r = TX.settings(tx, v), TX.reset_inputs(tx, v)
    idx = np.arange(n) % len(r["root_pos"])
    rng = np.random.default_rng(7 * n + 1)
    d = dict(root_pos=g.of("root_pos", r["root_pos"][idx]), joint_rotmat=g.of("joint_rotmat", r["joint_rotmat"][idx]), joint_pos_bind=g.of("joint_pos_bind", r["joint_pos_bind"]),
             env_shape_id=g.of("env_shape_id", r["env_shape_id"][idx].astype(np.int32)))
    before = {}
    for k, shape in (("target", (n, mt.ROW)), ("root_states", (n, 13)), ("dof_state", (n, 69, 2)), ("rb_state", (n, 24, 13))):
        before[k] = random_bits(rng, shape, np.float32)
        d[k] = g.of(k, before[k])
    f = g.of("flags", flags, dtype=i64)
    inputs = {k: B(d[k]) for k in ("root_pos", "joint_rotmat", "joint_pos_bind", "env_shape_id")}
    if how == "flags":
        mt.launch_reset_flagged(st, d, n, f, len(r["joint_pos_bind"]))
    else:
        mt.launch_reset(st, d, n, torch.as_tensor(np.flatnonzero(flags), device=DEV), len(r["joint_pos_bind"]))
    g.check()
    assert np.array_equal(B(f), B(torch.as_tensor(flags))), "the flags were written"
    for k, x in inputs.items():
        assert np.array_equal(B(d[k]), x), "the input %s was written" % k
    return {k: B(d[k]) for k in before}, {k: B(torch.as_tensor(x)) for k, x in before.items()}


@gpu
@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("v", TX.VARIANTS)
def test_target_reset_by_flags_equals_the_reset_by_ids(v, n):
    for name, flags in FF.flag_patterns(n).items():
        what = "variant %s, %d envs, flags %s" % (v, n, name)
        got, before = target_case(v, n, flags, "flags")
        want, _ = target_case(v, n, flags, "ids") if flags.any() else (before, None)  # (an empty id list is a no-op of the caller)
        assert_same_bytes(got, want, what)
        assert_same_bytes(target_case(v, n, flags, "flags")[0], got, what + ", second run")
        keep = flags == 0
        for k in got:
            assert np.array_equal(got[k].reshape(n, -1)[keep], before[k].reshape(n, -1)[keep]), "%s: %s of an env that is not flagged was written" % (what, k)
            if flags.any():
                assert not np.array_equal(got[k].reshape(n, -1)[~keep], before[k].reshape(n, -1)[~keep]), "%s: %s was not reset" % (what, k)


# ------------------------------------------------------------------------------------------------------------------ the bookkeeping
@gpu
@pytest.mark.parametrize("n", [1, 255, 256, 257])
def test_bookkeeping_of_the_flagged_envs(n):
    import ctypes as C

    from vid2player3d_amd import _lib

    L = _lib.load()
    rng = np.random.default_rng(n)
    for name, flags in FF.flag_patterns(n).items():
        g = Guarded(DEV)
        s0 = dict(progress=rng.integers(1, 9, n), terminate=rng.integers(0, 2, n), num_reset_reaction=rng.integers(1, 5, n), num_reset=rng.integers(0, 7, n),
                  distance=rng.uniform(1, 2, n).astype(np.float32), reset_reaction=rng.integers(0, 2, n).astype(bool), reset_recovery=rng.integers(0, 2, n).astype(bool))
        t = {k: g.of(k, x) for k, x in s0.items()}
        f = g.of("flags", flags, dtype=i64)
        b = _lib.CtlResetBuffers(**{k: x.data_ptr() for k, x in t.items()})
        up = flags != 0
        _lib.check(L.v2p_ctl_reset_begin(n, _lib.ptr(f), C.byref(b), _lib.current_stream(torch.device(DEV))), "v2p_ctl_reset_begin")
        g.check()
        got = {k: x.cpu().numpy() for k, x in t.items()}
        for k in ("progress", "terminate", "num_reset_reaction", "distance"):
            assert np.array_equal(got[k], np.where(up, 0, s0[k]).astype(s0[k].dtype)), (name, k)
        assert np.array_equal(got["num_reset"], s0["num_reset"] + up) and np.array_equal(got["reset_reaction"], s0["reset_reaction"])
        assert np.array_equal(f.cpu().numpy(), flags), "begin wrote the flags"
        _lib.check(L.v2p_ctl_reset_end(n, _lib.ptr(f), C.byref(b), _lib.current_stream(torch.device(DEV))), "v2p_ctl_reset_end")
        g.check()
        for k in ("reset_reaction", "reset_recovery"):
            assert np.array_equal(t[k].cpu().numpy(), s0[k] & ~up), (name, k)
        assert not f.cpu().numpy().any() and np.array_equal(t["num_reset"].cpu().numpy(), s0["num_reset"] + up), name


# ------------------------------------------------------------------------------------------------------------------ the engine's push
def _pushed_task(n, flags, how):
    from tests.gpu_util import synth_tables
    from vid2player3d_amd.motion_lib import MotionLib
    from vid2player3d_amd.tasks import HumanoidSMPLIM, default_cfg

    cfg = default_cfg(n, motion_lib=MotionLib(synth_tables(seed=5, num_clips=8, min_frames=60, max_frames=120), DEV), sample_first_motions=True,
                      body_shape_mismatch="ignore")
    task = HumanoidSMPLIM(cfg, device_type="cuda", device_id=0)
    rng = np.random.default_rng(3)
    task.reset_with_times(None, torch.as_tensor(rng.uniform(0.1, 1.0, n).astype(np.float32), device=DEV))
    # every env's exposed state is edited; only the flagged envs' edits reach the engine
    task._humanoid_root_states[:, 2] += torch.as_tensor(rng.uniform(0.01, 0.05, n).astype(np.float32), device=DEV)
    task._humanoid_root_states[:, 7:10] += torch.as_tensor(rng.normal(0, 0.2, (n, 3)).astype(np.float32), device=DEV)
    task._dof_state.view(n, 69, 2).add_(torch.as_tensor(rng.normal(0, 0.05, (n, 69, 2)).astype(np.float32), device=DEV))
    if how == "flags":
        task._reset_env_tensors_flagged(torch.as_tensor(flags, device=DEV, dtype=i64).contiguous(), with_rb_state=True)
    elif flags.any():
        task._reset_env_tensors(torch.as_tensor(np.flatnonzero(flags), device=DEV).contiguous(), with_rb_state=True)
    act = torch.as_tensor(rng.normal(0, 0.2, (n, 75)).astype(np.float32), device=DEV)
    task.step(act)
    torch.cuda.synchronize()
    out = {k: B(getattr(task, k)) for k in ("_humanoid_root_states", "_dof_state", "_rigid_body_state", "obs_buf", "rew_buf", "reset_buf")}
    task.close()
    return out


@gpu
@pytest.mark.parametrize("name", ["alternating", "half_a_wave", "none", "values_2_and_minus_1"])
def test_engine_push_by_flags_equals_the_push_by_ids(name):
    """two tasks built alike, one pushed by ids and one by flags, both stepped once on the same actions: the exported state is bit-equal;
    19 envs: two full 8-env workgroups and a tail"""
    n = 19
    flags = FF.flag_patterns(n)[name]
    a, b = _pushed_task(n, flags, "ids"), _pushed_task(n, flags, "flags")
    assert_same_bytes(b, a, "push by flags %s" % name)
    if name == "alternating":
        assert not np.array_equal(_pushed_task(n, np.zeros(n, np.int64), "ids")["_rigid_body_state"], a["_rigid_body_state"]), "the push changes nothing: the comparison is vacuous"


# ------------------------------------------------------------------------------------------------------------------ the controller
def _controller(n):
    from tests import policies_fixture as PF
    from vid2player3d_amd import policies as P

    ctl, task, player, target, gen = FF.controller(n)
    ctl.attach_low_level_policy(P.LowLevelPolicy(target, PF.random_actors(1, 734, 75)[0], PF.random_norms(1, 734)[0], 5.0, 1.0))
    ctl.progress_buf.copy_(torch.arange(n, device=DEV) % FF.EPISODE_LENGTH)
    return ctl, task, player, target


def _controller_bytes(ctl, task, player):
    out = {"ctl/" + k: B(v) for k, v in ctl._tensors().items()}
    out.update({"player/" + k: B(getattr(player, "_" + k)) for k in mvae.STATE_NAMES})
    out.update({"task/target%d" % i: B(t) for i, t in enumerate(task._target_bufs)})
    out.update({"ctl/_num_reset": B(ctl._num_reset), "ctl/_num_reset_reaction": B(ctl._num_reset_reaction), "task/_dof_state": B(task._dof_state),
                "task/_humanoid_root_states": B(task._humanoid_root_states), "task/_rigid_body_state": B(task._rigid_body_state),
                "task/_ball_root_states": B(task._ball_root_states), "task/_racket_rb_state": B(task._racket_rb_state)})
    return out


@gpu
def test_controller_reset_by_flags_equals_reset_of_the_done_ids_step_by_step():
    n, steps = 64, 12
    a, b = _controller(n), _controller(n)
    assert_same_bytes(_controller_bytes(*b[:3]), _controller_bytes(*a[:3]), "two controllers built alike")
    gen = torch.Generator().manual_seed(3)
    done_steps = flag_steps = 0
    for k in range(steps):
        act = (0.5 * torch.randn((n, a[0].get_action_size()), generator=gen)).to(DEV)
        for ctl, task, _, _ in (a, b):
            ctl.pre_physics_step(act.clone())
            ctl.physics_step()
            if k in (3, 8):  # forced hits of envs 1 and 6 (the flag the engine would set), forced misses of envs 2 and 7 (the ball behind the player)
                task._has_racket_ball_contact[1] = task._has_racket_ball_contact[6] = True
                for e in (2, 7):
                    task._ball_root_states[e, 1] = task._rigid_body_state.view(n, 24, 13)[e, 0, 1] - 2.0
            ctl.post_physics_step()
        done = a[0].reset_buf.cpu().numpy() != 0
        flagged = (a[0]._reset_reaction_buf | a[0]._reset_recovery_buf).cpu().numpy()
        done_steps += bool(done.any())
        flag_steps += bool((flagged & ~done).any())
        assert_same_bytes(_controller_bytes(*b[:3]), _controller_bytes(*a[:3]), "step %d, before the reset" % k)
        calls = (a[0]._reset_calls, b[0]._reset_calls)
        a[0].reset(a[0].reset_buf.nonzero(as_tuple=False).flatten())
        b[0].reset_by_flags()
        assert (a[0]._reset_calls, b[0]._reset_calls) == (calls[0] + 1, calls[1] + 1) and calls[0] == calls[1]
        assert_same_bytes(_controller_bytes(*b[:3]), _controller_bytes(*a[:3]), "step %d, after the reset (%d done)" % (k, done.sum()))
        assert not b[0].reset_buf.any() and bool((b[0]._num_reset.cpu().numpy() >= 1).all())
        # (a done env's flags were cleared by the reset; another env's flags were served by the task reset and stay, as in the id path)
    assert done_steps >= 5, "too few steps with a done env: %d" % done_steps
    assert flag_steps >= 1, "no step had a reaction or recovery flag on an env that was not done"
    assert int(b[0]._num_reset.sum()) > n, "no env was reset after the first reset"
    for _, task, _, _ in (a, b):
        if hasattr(task, "check"):
            task.check()
        task.close()
    with pytest.raises(NotImplementedError, match="task_reset 'device'"):
        ctl = b[0]
        ctl._task_reset = "torch"
        ctl.reset_by_flags()


# ------------------------------------------------------------------------------------------------------------------ the agent
@pytest.fixture(scope="module")
def agents():
    from tests import ctl_ppo_fixture as FX
    from vid2player3d_amd import ctl_ppo as CP

    n, T, out = 64, 12, {}
    for mode in ("ids", "flags"):
        ctl, task, player, target = _controller(n)
        params = FX.small_params()
        params["config"].update(horizon_length=T, minibatch_size=T * n, mini_epochs=1)
        out[mode] = CP.ControllerPPOAgent.from_config(ctl, params, reset_mode=mode)
    return out


@gpu
def test_agent_rollout_with_reset_mode_flags_equals_ids(agents):
    runs = {}
    for mode, agent in agents.items():
        assert agent.reset_mode == mode and agent.reuse_next_values
        agent.play_steps()
        torch.cuda.synchronize()
        runs[mode] = dict({k: B(v) for k, v in agent.tensor_dict.items()}, acc=B(agent.acc), sub_acc=B(agent.sub_acc), current_rewards=B(agent.current_rewards),
                          current_lengths=B(agent.current_lengths), obs_buf=B(agent.ctl.obs_buf), num_reset=B(agent.ctl._num_reset))
    assert_same_bytes(runs["flags"], runs["ids"], "play_steps, reset_mode 'flags' against 'ids'")
    dones = agents["ids"].tensor_dict["dones"].cpu().numpy()
    assert (dones.sum(1) > 0).sum() >= 5 and float(agents["ids"].acc[0]) == dones.sum(), "too few steps with a done env"
    for k, v in agents["flags"].tensor_dict.items():
        assert bool(torch.isfinite(v).all()), k


@gpu
def test_flags_rollout_makes_no_host_read(agents):
    """under torch's sync debug mode 'error' the 'ids' rollout raises at `_reset_lists` - which shows that the mode is honoured on this
    backend and that nothing in front of the read synchronises - and the 'flags' rollout completes"""
    torch.cuda.synchronize()
    raised = None
    torch.cuda.set_sync_debug_mode("error")
    try:
        try:
            agents["ids"].play_steps()
        except RuntimeError as e:
            raised = "".join(traceback.format_exception(type(e), e, e.__traceback__))
        if raised is not None:
            agents["flags"].play_steps()  # must complete
    finally:
        torch.cuda.set_sync_debug_mode("default")
    torch.cuda.synchronize()
    if raised is None:
        pytest.skip("torch.cuda.set_sync_debug_mode('error') is not honoured on this backend: the 'ids' rollout's host read did not raise")
    assert "_reset_lists" in raised, "the 'ids' rollout synchronised somewhere else than at its one host read:\n" + raised
    for k, v in agents["flags"].tensor_dict.items():
        assert bool(torch.isfinite(v).all()), k
