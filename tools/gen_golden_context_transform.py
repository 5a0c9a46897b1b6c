"""Golden data of the context transform (cfg env.transform_specs), recorded from the reference itself:
tests/golden/context_transform.npz holds the inputs, the draws and the reference's outputs (encoded as tests/context_transform_ref.py
describes) of
`HumanoidSMPLIM._transform_target` (embodied_pose/env/tasks/humanoid_smpl_im.py:565-592) for every single op and for the orders that
pin its quirks (mask -> noisy, noisy -> mask, noisy -> random, mask -> noisy -> random, random -> noisy -> mask).

The method runs unbound on a stand-in for `self` (cfg + body_names).  Its randomness is replaced by recorded draws, the convention the
engine reads: torch.bernoulli(p) -> (u < p) with u the op's uniform draw (u_noise for noisy_joints, u_drop for mask_random_joints), and
torch.randn_like -> z.  Run where the reference exists:
    python tools/gen_golden_context_transform.py
"""
import json
import os
import sys
import types

sys.dont_write_bytecode = True  # never leave __pycache__ in the read-only reference mount

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(HERE)
sys.path.insert(0, os.path.join(REPO, "oracle"))
sys.path.insert(0, REPO)

from ref_shim.install import install  # noqa: E402

install()

import torch  # noqa: E402

torch.set_num_threads(1)

import env.tasks.humanoid_smpl_im as him  # noqa: E402

from tests.context_transform_ref import POS_Q, U_Q, Z_Q, decode_fixture, decode_inputs, encode_outputs  # noqa: E402
from vid2player3d_amd.model import load_baked_model  # noqa: E402

OUT = os.path.join(REPO, "tests", "golden", "context_transform.npz")
N_ENVS, W, NB = 4, 48, 24

MASK = ("mask_joints", {"joints": ["Pelvis", "L_Ankle", "Head", "R_Hand"]})
NOISY = ("noisy_joints", {"prob": 0.5, "noise_std": 0.03, "conf_std": 0.03, "min_conf": 0.2})
RANDOM = ("mask_random_joints", {"prob": 0.3})
SPECS = {
    "empty": [],
    "mask": [MASK],
    "noisy": [NOISY],
    "random": [RANDOM],
    "mask_noisy": [MASK, NOISY],
    "noisy_mask": [NOISY, MASK],
    "noisy_random": [NOISY, RANDOM],
    "mask_noisy_random": [MASK, NOISY, RANDOM],
    "random_noisy_mask": [RANDOM, NOISY, MASK],
}


def run_reference(specs, body_pos, u_noise, z, u_drop, body_names):
    me = types.SimpleNamespace(cfg={"env": {"transform_specs": dict(specs)}}, body_names=list(body_names))
    uniforms = {"noisy_joints": u_noise, "mask_random_joints": u_drop}
    pending = [uniforms[name] for name, _ in specs if name in uniforms]  # one torch.bernoulli call per random op, in op order

    def bernoulli(p, *a, **k):
        u = pending.pop(0)
        assert tuple(p.shape) == tuple(u.shape)
        return (u < p).to(p.dtype)

    def randn_like(t, *a, **k):
        assert tuple(t.shape) == tuple(z.shape)
        return z.clone()

    ctx = {"body_pos": body_pos.clone(), "body_rot": None, "dof_pos": None, "body_pos_gt": body_pos.clone(), "dof_pos_gt": None}
    keep = torch.bernoulli, torch.randn_like
    torch.bernoulli, torch.randn_like = bernoulli, randn_like
    try:
        him.HumanoidSMPLIM._transform_target(me, ctx)
    finally:
        torch.bernoulli, torch.randn_like = keep
    assert not pending
    assert torch.equal(ctx["body_pos_gt"], body_pos)
    return ctx["body_pos"].numpy().astype(np.float32), ctx["joint_conf"].numpy().astype(np.float32)


def main():
    names = load_baked_model().body_names
    rng = np.random.default_rng(2026)
    rows = N_ENVS * W
    # positions of a standing body's scale around the origin, the draws as torch.rand / torch.randn make them; all on coarse grids, kept
    # as integers (tests/context_transform_ref.py) - the outputs are what the reference makes of them, at full precision
    q = {"body_pos_q": np.round((rng.normal(0.0, 0.4, size=(rows, NB, 3)) + np.array([0.0, 0.0, 0.9])) * POS_Q).astype(np.int16),
         "z_q": np.round(rng.standard_normal((rows, NB, 3)) * Z_Q).astype(np.int16),
         "u_noise_q": np.floor(rng.random((rows, NB)) * U_Q).astype(np.uint16),
         "u_drop_q": np.floor(rng.random((rows, NB)) * U_Q).astype(np.uint16)}
    inputs = decode_inputs(q)
    t = {k: torch.from_numpy(v) for k, v in inputs.items()}
    res = {}
    for key, specs in SPECS.items():
        pos, conf = run_reference(specs, t["body_pos"], t["u_noise"], t["z"], t["u_drop"], names)
        res[key + "/body_pos"], res[key + "/joint_conf"] = pos, conf
        print("%-18s zero conf %.3f  changed positions %.3f" % (key, float((conf == 0).mean()), float((pos != inputs["body_pos"]).any(-1).mean())))
    out = dict(q, body_names=np.array(list(names)), specs=np.array(json.dumps(SPECS)), **encode_outputs(SPECS, inputs, res))
    back = decode_fixture(out)
    assert all(np.array_equal(back[k].view(np.uint32), v.view(np.uint32)) for k, v in res.items())  # the encoding is lossless
    np.savez_compressed(OUT, **out)
    print("wrote", os.path.relpath(OUT, REPO), "%.1f MB" % (os.path.getsize(OUT) / 1e6))


if __name__ == "__main__":
    main()
