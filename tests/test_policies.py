"""Policy inference on the CPU side: the numpy statements of vid2player3d_amd/policies.py against what the reference's own classes
computed (tests/golden/policies.npz, tools/gen_golden_policies.py), the loading rules against the state the reference's loaders left,
and the refusals of the three C entry points - which happen before any HIP call."""
import ctypes as C
import math

import numpy as np
import pytest
import torch

from tests import mvae_target_fixture as TX
from tests import policies_fixture as PF
from vid2player3d_amd import _lib
from vid2player3d_amd import mvae_target as mt
from vid2player3d_amd import policies as P


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def same_bits(a, b):
    return a.shape == b.shape and np.array_equal(bits(a), bits(b))


def pd_settings(v):
    spec = PF.VARIANTS[v]
    return dict(pd_target_base=spec["base"], no_scale_action=spec["no_scale"])


def pd_bases(g, v):
    """the arrays `_action_to_pd_targets` was recorded on, as `target_actions_reference` takes them"""
    row = np.zeros((PF.N, mt.ROW), np.float32)
    a, b = mt.SLICES["dof_pos"]
    row[:, a:b] = g[v + "/target_dof_pos"]
    # (base 'none': the reference's object sits at the offsets; dof_state is not read by that base)
    dof_state = np.stack([g[v + "/dof_pos"], np.zeros_like(g[v + "/dof_pos"])], -1)
    return dict(target=row, dof_state=dof_state, pd_action_scale=g[v + "/pd_action_scale"], pd_action_offset=g[v + "/pd_action_offset"])


# ------------------------------------------------------------------------------------------------------------------ the statements
@pytest.mark.parametrize("v", sorted(PF.VARIANTS))
def test_input_statement_is_the_reference_bit_for_bit(v):
    """clamp -> normaliser -> side-major order: the float32 rows the reference's `RunningNorm.forward` / RunningMeanStd made"""
    g, spec = PF.golden(), PF.VARIANTS[v]
    _, norms = PF.loaded(v)
    x = P.policy_input_reference(PF.observations(v), norms, PF.sides(v), spec["clip_obs"])
    assert same_bits(x, g[v + "/x"]), "%s: %d elements differ" % (v, int((bits(x) != bits(g[v + "/x"])).sum()))
    assert [n.kind for n in norms] == [PF.NORM_KIND[k] for k in spec["stats"]]


@pytest.mark.parametrize("v", sorted(PF.VARIANTS))
def test_actor_statement_and_module_follow_the_reference(v):
    """mu of the recorded x: the numpy statement and the ActorMLP on the CPU, within the fp32-fp64 scatter of the reference against
    itself (x 8: a sum taken in another order)"""
    g = PF.golden()
    actors, _ = PF.loaded(v)
    sides, h = PF.sides(v), PF.N // PF.sides(v)
    tol = 8 * float(g[v + "/mu_scatter"])
    mu = np.concatenate([P.actor_reference(a.layer_arrays(), g[v + "/x"][s * h:(s + 1) * h]) for s, a in enumerate(actors)])
    assert np.abs(P.env_order(mu, sides) - g[v + "/mu"]).max() <= tol
    with torch.no_grad():
        mod = np.concatenate([a(torch.from_numpy(g[v + "/x"][s * h:(s + 1) * h])).numpy() for s, a in enumerate(actors)])
    assert np.abs(P.env_order(mod, sides) - g[v + "/mu"]).max() <= tol
    assert same_bits(P._clamp_np(g[v + "/mu"], PF.VARIANTS[v]["clip_actions"], np.float32), g[v + "/action"])


@pytest.mark.parametrize("v", [v for v in sorted(PF.VARIANTS) if PF.VARIANTS[v]["kind"] == "ll"])
def test_pd_target_statement_is_the_reference_bit_for_bit(v):
    """`_action_to_pd_targets` of the clamped mu, from the reference's own mu laid out side-major"""
    g, sides = PF.golden(), PF.sides(v)
    mu_sm = np.empty_like(g[v + "/mu"])
    mu_sm[P.side_major_rows(PF.N, sides)] = g[v + "/mu"]
    assert same_bits(P.env_order(mu_sm, sides), g[v + "/mu"])
    pd = P.ll_policy_actions_reference(pd_settings(v), mu_sm, sides, PF.VARIANTS[v]["clip_actions"], **pd_bases(g, v))
    assert same_bits(pd[:, :69], g[v + "/pd"]), v
    assert same_bits(pd[:, 69:], g[v + "/action"][:, 69:])


def test_side_major_order():
    assert list(P.side_major_rows(5, 1)) == [0, 1, 2, 3, 4]
    assert list(P.side_major_rows(6, 2)) == [0, 3, 1, 4, 2, 5]
    x = P.policy_input_reference(np.arange(12, dtype=np.float32).reshape(6, 2), [P.Normaliser("none")] * 2, 2)
    assert np.array_equal(x[:3], np.arange(12).reshape(6, 2)[0::2]) and np.array_equal(x[3:], np.arange(12).reshape(6, 2)[1::2])
    with pytest.raises(ValueError, match="odd"):
        P.policy_input_reference(np.zeros((3, 2), np.float32), [P.Normaliser("none")] * 2, 2)


def test_clamp_of_the_statement_is_torch_clamp():
    """a NaN stays a NaN, infinities go to the clip, an infinite clip changes nothing, |x| on the clip stays; std = 0 divides by 1e-8"""
    edge = np.array([[np.nan, np.inf, -np.inf, 2.0, -2.0, 1.9999999, 0.0, -0.0]], np.float32)
    for c in (2.0, math.inf):
        want = torch.clamp(torch.from_numpy(edge), -c, c).numpy()
        assert np.array_equal(bits(P._clamp_np(edge, c, np.float32)), bits(want))
    nm = P.Normaliser("running", np.zeros(8, np.float32), np.array([0, 0, 0, 0, 1, 1, 1, 1], np.float32))
    t = torch.from_numpy(edge)
    want = torch.clamp((torch.clamp(t, -2.0, 2.0) - 0.0) / (torch.from_numpy(nm.spread) + 1e-8), -5.0, 5.0).numpy()
    assert np.array_equal(bits(P.policy_input_reference(edge, nm, 1, 2.0)), bits(want))
    # (mean_var with a root that is exact in float32 - 0.25 + eps with eps 0 - so that a sqrt which is only faithful gives the same bits)
    mv = P.Normaliser("mean_var", np.zeros(8, np.float32), np.full(8, 0.25, np.float32), eps=0.0)
    want = torch.clamp((t - 0.0) / torch.sqrt(torch.from_numpy(mv.spread) + 0.0), -5.0, 5.0).numpy()
    assert np.array_equal(bits(P.policy_input_reference(edge, mv, 1)), bits(want))


# ------------------------------------------------------------------------------------------------------------------ the loading rules
@pytest.mark.parametrize("v", sorted(PF.VARIANTS))
def test_loaders_reproduce_the_state_the_reference_left(v):
    g, spec = PF.golden(), PF.VARIANTS[v]
    dim, act = PF.dims(v)
    actors, norms = PF.loaded(v)
    for s, (a, nm) in enumerate(zip(actors, norms)):
        p = "%s/loaded/%d/" % (v, s)
        w0 = a.actor_mlp[0].weight.numpy()
        assert w0.shape == (PF.UNITS[0], dim) and a.num_actions == act
        assert np.array_equal(w0.astype(np.float64).sum(1), g[p + "actor_mlp.0.weight_row_sums"]) and same_bits(a.mu.bias.numpy(), g[p + "mu.bias"])
        if p + "actor_mlp.0.weight" in g:
            assert same_bits(w0, g[p + "actor_mlp.0.weight"])
        width = spec.get("ckpt_dim", [dim] * 2)[s]
        assert not w0[:, width:].any() and w0[:, :width].any(), "the first layer is zero-padded on the right"
        kind = spec["stats"][s]
        if kind == "norm_n0":
            assert nm.kind == "none" and int(g[p + "n"]) == 0
        elif PF.NORM_KIND[kind] == "running":
            assert nm.kind == "running" and int(g[p + "n"]) > 0
            assert same_bits(nm.mean, g[p + "mean"]) and same_bits(nm.spread, g[p + "std"])
            if kind in ("rms", "rms_model"):  # (std = sqrt(var) of the float32 cast, zero-padded)
                var = PF.checkpoint_arrays(v, s)["running_mean_std" if kind == "rms" else "model"]
                var = var["running_var"] if kind == "rms" else var[PF.PREFIX + "running_obs.running_var"]
                assert same_bits(nm.spread[:width], np.sqrt(var.astype(np.float32))) and not nm.spread[width:].any() and not nm.mean[width:].any()
        else:
            assert nm.kind == "mean_var" and nm.eps == 1e-5 and nm.clip == 5.0
            assert same_bits(nm.mean, g[p + "mean"]) and same_bits(nm.spread, g[p + "var"])
            assert not nm.mean[width:].any() and (nm.spread[width:] == 1).all(), "a fresh RunningMeanStd behind the checkpoint's columns"


def test_loaders_refuse_what_is_not_built():
    model = PF.checkpoint_tensors("ctl_one_rl_game", 0)["model"]
    with pytest.raises(ValueError, match="first layer reads 40 columns"):
        P.ActorMLP.from_state_dict(model, obs_dim=39)
    with pytest.raises(ValueError, match="starts with"):
        P.ActorMLP.from_state_dict(model, prefix="network.")
    with pytest.raises(NotImplementedError, match="learned sigma"):
        P.ActorMLP.from_state_dict(dict(model, **{PF.PREFIX + "sigma.weight": torch.zeros(35, 32)}))
    with pytest.raises(NotImplementedError, match="CNN / RNN"):
        P.ActorMLP.from_state_dict(dict(model, **{PF.PREFIX + "actor_cnn.0.weight": torch.zeros(4, 4)}))
    with pytest.raises(NotImplementedError, match="CNN / RNN"):
        P.ActorMLP.from_state_dict(dict(model, **{PF.PREFIX + "a_rnn.rnn.weight_ih_l0": torch.zeros(4, 4)}))
    ok = {"mlp": {"units": [1024, 1024, 512], "activation": "relu"}, "space": {"continuous": {"mu_activation": "None", "fixed_sigma": True}}}
    P.ActorMLP.from_state_dict(model, params=ok)
    for bad, word in (({"mlp": {"activation": "elu"}}, "activation"), ({"rnn": {"units": 256}}, "rnn"), ({"cnn": {"type": "conv2d"}}, "cnn"),
                      ({"space": {"continuous": {"mu_activation": "tanh"}}}, "mu_activation"), ({"space": {"continuous": {"fixed_sigma": False}}}, "learned sigma"),
                      ({"space": {"discrete": {}}}, "continuous")):
        with pytest.raises(NotImplementedError, match=word):
            P.ActorMLP.from_state_dict(model, params=bad)
    with pytest.raises(ValueError, match="none of"):
        P.Normaliser("batch")
    with pytest.raises(ValueError, match="statistics have 40 columns"):
        P.input_norm({"running_mean_std": {"running_mean": np.zeros(40), "running_var": np.ones(40)}}, 39)
    with pytest.raises(ValueError, match="no running_mean_std"):
        P.input_norm({"model": model})
    assert P.network_norm({"model": {k: x for k, x in model.items() if "running_obs" not in k}}).kind == "none"
    with pytest.raises(TypeError, match="ImitationTarget"):
        P.LowLevelPolicy(object(), [], [])


def test_the_step_path_reads_nothing_back():
    """no host synchronisation between the launches: the code of the per-step path has no `.item()`, `nonzero`, `.cpu()`, `tolist` or
    `synchronize`, and allocates no tensor"""
    import inspect

    from vid2player3d_amd.tasks import tennis_controller as tc

    path = [P.LowLevelPolicy.step, P.LowLevelPolicy._src, P.ControllerPolicy.act, P.ActorMLP.forward, P.launch_policy_input, P.launch_ll_policy_input,
            P.launch_ll_policy_actions, tc.TennisControllerTask.physics_step, tc.TennisControllerTask.step]
    for fn in path:
        src = inspect.getsource(fn)
        for word in (".item(", "nonzero", ".cpu(", "tolist", "synchronize", "torch.zeros", "torch.empty", ".clone(", "torch.cat", "numpy"):
            assert word not in src, "%s: %s on the per-step path" % (fn.__qualname__, word)


# ------------------------------------------------------------------------------------------------------------------ the C boundary
def test_symbols_and_abi():
    for name in ("v2p_policy_input", "v2p_ll_policy_input", "v2p_ll_policy_actions"):
        assert name in _lib.EXPORTED_SYMBOLS
    assert _lib.ABI_VERSION == 15 and _lib.load().v2p_abi_version() == 15
    assert _lib.NORM_KINDS == {"none": 0, "running": 1, "mean_var": 2}


def test_struct_sizes_match_the_header():
    import os
    import subprocess
    import tempfile

    repo = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    prog = '#include <stdio.h>\n#include "v2p_rollout.h"\nint main(void){ printf("%zu %zu %zu\\n", sizeof(v2p_policy_norm), sizeof(v2p_policy_input_cfg), sizeof(v2p_ll_policy_src)); return 0; }\n'
    with tempfile.TemporaryDirectory() as d:
        src, exe = os.path.join(d, "s.c"), os.path.join(d, "s")
        open(src, "w").write(prog)
        subprocess.check_call(["gcc", "-I", os.path.join(repo, "include"), src, "-o", exe])
        sizes = [int(x) for x in subprocess.check_output([exe]).split()]
    assert sizes == [C.sizeof(_lib.PolicyNorm), C.sizeof(_lib.PolicyInputCfg), C.sizeof(_lib.LLPolicySrc)]


def _cfg(sides=1, clip_obs=math.inf, kinds=("running", "mean_var"), **norm0):
    c = _lib.PolicyInputCfg(sides=sides, clip_obs=clip_obs)
    for s in range(2):
        c.norm[s].kind, c.norm[s].eps, c.norm[s].clip, c.norm[s].mean, c.norm[s].spread = _lib.NORM_KINDS[kinds[s]], 1e-5, 5.0, 0x1000, 0x2000
    for k, x in norm0.items():
        setattr(c.norm[0], k, x)
    return c


def test_bad_arguments_are_refused_without_a_gpu():
    """every call below is refused before any HIP call: the pointers are placeholders that are never dereferenced"""
    L, p, q = _lib.load(), C.c_void_p(0x1000), C.c_void_p(0x3000)
    src = _lib.LLPolicySrc(rb_state=0x1000, dof_state=0x2000, target=0x3000, target_stride=331, motion_bodies=0x4000)

    def refused(rc, fn, word):
        assert rc == -1
        msg = L.v2p_last_error().decode()
        assert msg.startswith(fn + ":") and word in msg, msg

    def plain(c, n=4, dim=7, obs=p, x=q):
        return L.v2p_policy_input(C.byref(c) if c else None, n, dim, obs, x, None)

    def low(c, n=4, dim=734, s=src, raw=p, x=q):
        return L.v2p_ll_policy_input(C.byref(c) if c else None, n, dim, C.byref(s) if s else None, raw, x, None)

    for fn, call in (("v2p_policy_input", plain), ("v2p_ll_policy_input", low)):
        refused(call(None), fn, "null cfg")
        refused(call(_cfg(), n=-1), fn, "n -1")
        refused(call(_cfg(sides=0)), fn, "sides 0")
        refused(call(_cfg(sides=3)), fn, "sides 3")
        refused(call(_cfg(sides=2), n=5), fn, "odd")
        refused(call(_cfg(kind=3)), fn, "kind 3")
        refused(call(_cfg(kind=-1)), fn, "kind -1")
        refused(call(_cfg(mean=None)), fn, "null mean")
        refused(call(_cfg(spread=None)), fn, "null mean")
        refused(call(_cfg(clip=0.0)), fn, "clip")
        refused(call(_cfg(clip_obs=0.0)), fn, "clip_obs")
        refused(call(_cfg(clip_obs=float("nan"))), fn, "clip_obs")
        refused(call(_cfg(), x=None), fn, "null")
        assert call(_cfg(), n=0) == 0 and call(_cfg(sides=2), n=0) == 0, "n = 0 is a no-op"
        assert call(_cfg(kinds=("none", "none"), mean=None, spread=None), n=0) == 0, "a NONE normaliser reads no statistics"
    refused(plain(_cfg(), dim=0), "v2p_policy_input", "dim 0")
    refused(plain(_cfg(), obs=None), "v2p_policy_input", "null")
    refused(plain(_cfg(sides=2), x=p), "v2p_policy_input", "must not be obs")
    refused(low(_cfg(), dim=733), "v2p_ll_policy_input", "dim 733")
    refused(low(_cfg(), s=None), "v2p_ll_policy_input", "null src")
    refused(low(_cfg(), x=p), "v2p_ll_policy_input", "same buffer")
    for k in ("rb_state", "dof_state", "target", "motion_bodies"):
        bad = _lib.LLPolicySrc(rb_state=0x1000, dof_state=0x2000, target=0x3000, target_stride=331, motion_bodies=0x4000)
        setattr(bad, k, None)
        refused(low(_cfg(), s=bad), "v2p_ll_policy_input", "null rb_state")
    refused(low(_cfg(), s=_lib.LLPolicySrc(rb_state=0x1000, dof_state=0x2000, target=0x3000, target_stride=330, motion_bodies=0x4000)), "v2p_ll_policy_input", "target_stride")
    assert low(_cfg(), raw=None, n=0) == 0, "the raw observation is optional"

    g = TX.golden()
    st = TX.settings(g, "H")
    bufs = lambda **ch: _lib.MvaeTargetBuffers(**dict({k: 0x1000 * (i + 1) for i, k in enumerate(_lib.MVAE_TARGET_BUFFER_NAMES)}, **ch))

    def act(c=mt.cfg_struct(st, 1), n=4, sides=1, clip=math.inf, mu=p, b=bufs(), out=q):
        return L.v2p_ll_policy_actions(C.byref(c) if c else None, n, sides, clip, mu, C.byref(b) if b else None, out, None)

    fn = "v2p_ll_policy_actions"
    refused(act(c=None), fn, "null")
    refused(act(b=None), fn, "null")
    refused(act(n=-2), fn, "n -2")
    refused(act(sides=0), fn, "sides 0")
    refused(act(sides=2, n=3), fn, "odd")
    refused(act(clip=0.0), fn, "clip_actions")
    refused(act(mu=None), fn, "null mu")
    refused(act(out=None), fn, "null mu")
    refused(act(sides=2, out=p), fn, "must not be mu")
    refused(act(b=bufs(target=None)), fn, "null base")
    refused(act(b=bufs(pd_action_scale=None)), fn, "pd_action_scale")
    c = mt.cfg_struct(st, 1)
    c.pd_target_base = 3
    refused(act(c=c), fn, "pd_target_base")
    assert act(n=0) == 0 and act(n=0, sides=2) == 0
