"""CPU checks of the context transform (cfg env.transform_specs, humanoid_smpl_im.py:565-592): the numpy restatement against the
reference's own outputs (tests/golden/context_transform.npz, tools/gen_golden_context_transform.py), the v2p_context_transform struct
against the header, the setter's refusals and the task's parsing of the specs."""
import ctypes
import json
import os
import subprocess
import tempfile

import numpy as np
import pytest

from tests.conftest import load_golden
from tests.context_transform_ref import apply_transform, decode_fixture

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BODY_NAMES = ['Pelvis', 'L_Hip', 'L_Knee', 'L_Ankle', 'L_Toe', 'R_Hip', 'R_Knee', 'R_Ankle', 'R_Toe', 'Torso', 'Spine', 'Chest', 'Neck', 'Head',
              'L_Thorax', 'L_Shoulder', 'L_Elbow', 'L_Wrist', 'L_Hand', 'R_Thorax', 'R_Shoulder', 'R_Elbow', 'R_Wrist', 'R_Hand']


@pytest.fixture(scope="module")
def golden():
    return decode_fixture(load_golden("context_transform.npz"))


def _specs(golden):
    return json.loads(str(golden["specs"]))


def test_fixture_covers_every_op_and_the_quirk_orders(golden):
    specs = _specs(golden)
    orders = {tuple(name for name, _ in s) for s in specs.values()}
    for want in [(), ("mask_joints",), ("noisy_joints",), ("mask_random_joints",), ("mask_joints", "noisy_joints"), ("noisy_joints", "mask_joints"),
                 ("noisy_joints", "mask_random_joints"), ("mask_joints", "noisy_joints", "mask_random_joints")]:
        assert want in orders, want
    assert list(golden["body_names"]) == BODY_NAMES


@pytest.mark.parametrize("key", ["empty", "mask", "noisy", "random", "mask_noisy", "noisy_mask", "noisy_random", "mask_noisy_random",
                                 "random_noisy_mask"])
def test_restatement_equals_the_reference(golden, key):
    specs = _specs(golden)[key]
    pos, conf = apply_transform(specs, golden["body_pos"], golden["u_noise"], golden["z"], golden["u_drop"], BODY_NAMES)
    ref_pos, ref_conf = golden[key + "/body_pos"], golden[key + "/joint_conf"]
    assert pos.dtype == np.float32 and conf.dtype == np.float32
    assert np.array_equal(pos.view(np.uint32), ref_pos.view(np.uint32)), "positions differ in %d entries" % int((pos != ref_pos).sum())
    assert np.abs(conf - ref_conf).max() <= 1e-6
    assert np.array_equal(conf == 0, ref_conf == 0)


def test_reference_quirks_are_in_the_fixture(golden):
    """what the orders pin: noisy_joints reports 1 for an un-noised masked joint; mask_joints after noisy_joints zeroes positions only"""
    mask = [BODY_NAMES.index(j) for j in _specs(golden)["mask"][0][1]["joints"]]
    un_noised = golden["u_noise"][:, mask] >= 0.5
    assert (golden["mask_noisy/joint_conf"][:, mask][un_noised] == 1.0).all()
    assert (golden["mask_noisy/body_pos"][:, mask][un_noised] == 0.0).all()
    assert (golden["noisy_mask/body_pos"][:, mask] == 0.0).all()
    assert (golden["noisy_mask/joint_conf"][:, mask] > 0.0).any()
    assert (golden["random/joint_conf"][:, 0] == 1.0).all()


def test_struct_size_matches_the_header():
    from vid2player3d_amd import _lib

    prog = r'''
#include <stdio.h>
#include <stddef.h>
#include "v2p_rollout.h"
int main(void){ printf("%zu %zu %zu %d %d %d %d\n", sizeof(v2p_context_transform), offsetof(v2p_context_transform, mask_joints),
                       offsetof(v2p_context_transform, drop_prob), V2P_CONTEXT_DIM_CONF, V2P_CTX_MASK_JOINTS, V2P_CTX_NOISY_JOINTS,
                       V2P_CTX_MASK_RANDOM_JOINTS); return 0; }
'''
    with tempfile.TemporaryDirectory() as d:
        src = os.path.join(d, "s.c")
        open(src, "w").write(prog)
        exe = os.path.join(d, "s")
        subprocess.check_call(["gcc", "-I", os.path.join(REPO, "include"), src, "-o", exe])
        got = [int(x) for x in subprocess.check_output([exe]).split()]
    T = _lib.ContextTransform
    assert got == [ctypes.sizeof(T), T.mask_joints.offset, T.drop_prob.offset, _lib.CONTEXT_DIM_CONF, _lib.CTX_MASK_JOINTS, _lib.CTX_NOISY_JOINTS,
                   _lib.CTX_MASK_RANDOM_JOINTS]


def _xf(ops, **kw):
    from vid2player3d_amd import _lib

    t = _lib.ContextTransform(num_ops=len(ops), noise_prob=0.5, noise_std=0.03, conf_std=0.03, min_conf=0.2, drop_prob=0.3)
    for k, op in enumerate(ops):
        t.ops[k] = op
    for k, v in kw.items():
        setattr(t, k, v)
    return t


def test_setter_refuses_bad_transforms_without_a_gpu():
    """the transform is checked before the batch: a NULL env sees each refusal with its own message, and a valid transform reaches the
    'null env' check (no HIP call is made)"""
    from vid2player3d_amd import _lib

    L = _lib.load()
    M, N, R = _lib.CTX_MASK_JOINTS, _lib.CTX_NOISY_JOINTS, _lib.CTX_MASK_RANDOM_JOINTS
    draws = ctypes.c_void_p(16)  # (never dereferenced: every call below is refused)

    def refused(t, d, what):
        assert L.v2p_env_set_context_transform(None, None if t is None else ctypes.byref(t), d) == -1
        msg = L.v2p_last_error().decode()
        assert what in msg, msg

    refused(None, draws, "null transform")
    refused(_xf([M, M]), draws, "repeated")
    refused(_xf([N, R, N]), draws, "repeated")
    refused(_xf([4]), draws, "unknown op")
    refused(_xf([0]), draws, "unknown op")
    refused(_xf([M, N, R], num_ops=4), draws, "num_ops")
    refused(_xf([M], mask_joints=1 << 24), None, "above 23")
    refused(_xf([N], noise_prob=1.5), draws, "prob")
    refused(_xf([N], noise_prob=-0.1), draws, "prob")
    refused(_xf([N], noise_prob=float("nan")), draws, "prob")
    refused(_xf([R], drop_prob=1.01), draws, "prob")
    refused(_xf([N], conf_std=0.0), draws, "conf_std")
    refused(_xf([N], conf_std=-1.0), draws, "conf_std")
    refused(_xf([N]), None, "draws")
    refused(_xf([R]), None, "draws")
    # valid transforms reach the batch
    refused(_xf([]), None, "null env")
    refused(_xf([M], mask_joints=(1 << 24) - 1), None, "null env")
    refused(_xf([M, N, R]), draws, "null env")
    refused(_xf([R], drop_prob=1.0, noise_prob=7.0, conf_std=0.0), draws, "null env")  # (parameters of absent ops are not looked at)


def test_parse_transform_specs_keeps_order_and_resolves_names():
    from vid2player3d_amd import _lib
    from vid2player3d_amd.tasks.humanoid_smpl_im import parse_transform_specs

    specs = {"noisy_joints": {"prob": 0.25, "noise_std": 0.05, "conf_std": 0.1, "min_conf": 0.3}, "mask_joints": {"joints": ["Head", "L_Hand"]},
             "mask_random_joints": {"prob": 0.125}}
    t = parse_transform_specs(specs, BODY_NAMES)
    assert t.num_ops == 3 and list(t.ops) == [_lib.CTX_NOISY_JOINTS, _lib.CTX_MASK_JOINTS, _lib.CTX_MASK_RANDOM_JOINTS]
    assert t.mask_joints == (1 << 13) | (1 << 18)
    assert (t.noise_prob, t.noise_std, t.min_conf, t.drop_prob) == (np.float32(0.25), np.float32(0.05), np.float32(0.3), 0.125)
    assert t.conf_std == np.float32(0.1)
    t = parse_transform_specs({"mask_random_joints": {"prob": 0.5}, "mask_joints": {"joints": ["Pelvis"]}}, BODY_NAMES)
    assert t.num_ops == 2 and list(t.ops)[:2] == [_lib.CTX_MASK_RANDOM_JOINTS, _lib.CTX_MASK_JOINTS] and t.mask_joints == 1
    assert parse_transform_specs({}, BODY_NAMES).num_ops == 0


def test_parse_transform_specs_refuses_unknown_transforms_and_joints():
    from vid2player3d_amd.tasks.humanoid_smpl_im import parse_transform_specs

    with pytest.raises(ValueError, match="unknown transform"):
        parse_transform_specs({"noisy_joint": {"prob": 0.5, "noise_std": 0.1, "conf_std": 0.1, "min_conf": 0.1}}, BODY_NAMES)
    with pytest.raises(ValueError):
        parse_transform_specs({"mask_joints": {"joints": ["L_Pinky"]}}, BODY_NAMES)
    with pytest.raises(ValueError):
        parse_transform_specs(None, BODY_NAMES)
