"""Golden data for the two tests that used to read the reference tree at test time, recorded from the reference itself:
  * tests/golden/ref_rotation3d.npz: inputs and outputs of the reference's own quaternion library (poselib/poselib/core/rotation3d.py:
    quat_mul, quat_conjugate, quat_from_angle_axis, quat_rotate) - what tests/test_ref_shim.py pins the isaacgym.torch_utils shim to;
  * tests/golden/amass_im_params.json: the `params` block of embodied_pose/cfg/amass_im.yaml as yaml.safe_load returns it - what
    tests/test_ppo_reference.py builds the agent from.
Run where the reference exists:
    python oracle/gen_golden_ref_pins.py
"""
import json
import os
import sys

sys.dont_write_bytecode = True  # never leave __pycache__ in the read-only reference mount

import numpy as np
import torch
import yaml

from ref_shim.install import REFERENCE_ROOT

HERE = os.path.dirname(os.path.abspath(__file__))
OUT = os.path.join(HERE, "..", "tests", "golden")

sys.path.insert(0, os.path.join(REFERENCE_ROOT, "poselib"))
from poselib.core import rotation3d as R3  # noqa: E402

rng = np.random.default_rng(12)


def rand_quats(n):
    q = rng.normal(size=(n, 4))
    return torch.tensor(q / np.linalg.norm(q, axis=1, keepdims=True), dtype=torch.float32)


a, b = rand_quats(100), rand_quats(100)
ang = torch.tensor(rng.uniform(-3, 3, size=100), dtype=torch.float32)
ax = torch.tensor(rng.normal(size=(100, 3)), dtype=torch.float32)
v = torch.tensor(rng.normal(size=(100, 3)), dtype=torch.float32)
out = {"a": a, "b": b, "ang": ang, "ax": ax, "v": v, "quat_mul_ab": R3.quat_mul(a, b), "quat_conjugate_a": R3.quat_conjugate(a),
       "quat_from_angle_axis": R3.quat_from_angle_axis(ang, ax), "quat_rotate_a_v": R3.quat_rotate(a, v)}
out = {k: t.numpy().astype(np.float32) for k, t in out.items()}
np.savez(os.path.join(OUT, "ref_rotation3d.npz"), **out)
print("wrote tests/golden/ref_rotation3d.npz", {k: x.shape for k, x in out.items()})

with open(os.path.join(REFERENCE_ROOT, "embodied_pose", "cfg", "amass_im.yaml")) as f:
    params = yaml.safe_load(f)["params"]
with open(os.path.join(OUT, "amass_im_params.json"), "w") as f:
    json.dump(params, f, indent=1, sort_keys=True)
    f.write("\n")
print("wrote tests/golden/amass_im_params.json")
