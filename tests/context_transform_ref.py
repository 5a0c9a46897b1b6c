"""numpy restatement of the context transform (cfg env.transform_specs; HumanoidSMPLIM._transform_target,
embodied_pose/env/tasks/humanoid_smpl_im.py:565-592), the yardstick of the engine's fused version in env_context_kernel.

Written tensor for tensor after the reference, float32 where it is float32: `orig` is the ones tensor the reference makes first (its
local `joint_conf`, which mask_joints zeroes and multiplies body_pos with), `conf` is context_dict['joint_conf'] - the same tensor until
noisy_joints replaces it.  Draws as the engine reads them: u_noise [..,24], z [..,24,3], u_drop [..,24]; a Bernoulli(p) is u < p."""
import numpy as np
import torch

F = np.float32


def _ndtr(x):
    """scipy.stats.norm.cdf in float64"""
    return torch.special.ndtr(torch.from_numpy(np.asarray(x, dtype=np.float64))).numpy()


def apply_transform(specs, body_pos, u_noise, z, u_drop, body_names):
    """specs: [(name, spec dict)] in the order they run.  Returns (body_pos, joint_conf) as the reference leaves them."""
    pos = np.array(body_pos, dtype=F)
    orig = np.ones(pos.shape[:-1], dtype=F)
    conf = orig  # the same array until noisy_joints makes a new one
    for name, spec in specs:
        if name == "mask_joints":
            idx = [list(body_names).index(j) for j in spec["joints"]]
            orig[..., idx] = F(0.0)
            pos = pos * orig[..., None]
        elif name == "noisy_joints":
            std = np.where(u_noise < F(spec["prob"]), F(spec["noise_std"]), F(0.0)).astype(F)
            noise = (np.asarray(z, dtype=F) * std[..., None]).astype(F)
            nn = (np.sqrt((noise * noise).sum(-1, dtype=F)).astype(F) / F(np.sqrt(3) * spec["conf_std"])).astype(F)
            c = ((F(1.0) - _ndtr(nn).astype(F)) * F(2.0)).astype(F)
            pos = (pos + noise).astype(F)
            occluded = c < F(spec["min_conf"])
            c[occluded] = F(0.0)
            pos[occluded] = F(0.0)
            conf = c
        elif name == "mask_random_joints":
            drop = u_drop < F(spec["prob"])
            drop[..., 0] = False
            conf[drop] = F(0.0)
            pos[drop] = F(0.0)
        else:
            raise ValueError("unknown transform %r" % (name,))
    return pos, conf.copy()


def near_threshold(specs, body_pos, u_noise, z, u_drop, body_names, tol=1e-5):
    """bodies whose noisy_joints confidence lies within `tol` of min_conf: there the occlusion decision may flip with a rounding of Phi"""
    for name, spec in specs:
        if name == "noisy_joints":
            std = np.where(u_noise < F(spec["prob"]), F(spec["noise_std"]), F(0.0)).astype(F)
            noise = (np.asarray(z, dtype=F) * std[..., None]).astype(F)
            nn = np.sqrt((noise.astype(np.float64) ** 2).sum(-1)) / (np.sqrt(3) * spec["conf_std"])
            c = 2.0 * (1.0 - _ndtr(nn))
            return np.abs(c - spec["min_conf"]) < tol
    return np.zeros(np.shape(u_noise), dtype=bool)


# ---- the fixture's storage (tests/golden/context_transform.npz, written by tools/gen_golden_context_transform.py).  Inputs lie on
# coarse grids and are kept as integers: body_pos in 1/1024 m, z in 2^-12, the uniforms in 2^-16.  Each output is kept as the bit
# difference (XOR of the float32 bits) from a base - the noisy_joints-only output for the specs that noise, the clean input (positions)
# and ones (confidence) for the others - so that what the specs share is stored once.
POS_Q, Z_Q, U_Q = 1024.0, 4096.0, 65536.0
BASE_KEY = "noisy"


def decode_inputs(q):
    return {"body_pos": q["body_pos_q"].astype(F) / F(POS_Q), "z": q["z_q"].astype(F) / F(Z_Q),
            "u_noise": q["u_noise_q"].astype(F) / F(U_Q), "u_drop": q["u_drop_q"].astype(F) / F(U_Q)}


def _bits(x):
    return np.ascontiguousarray(x, dtype=F).view(np.uint32)


def _base(key, specs, inputs, out):
    if key != BASE_KEY and any(name == "noisy_joints" for name, _ in specs[key]):
        return out[BASE_KEY + "/body_pos"], out[BASE_KEY + "/joint_conf"]
    return inputs["body_pos"], np.ones(inputs["u_noise"].shape, dtype=F)


def encode_outputs(specs, inputs, out):
    """{key/body_pos, key/joint_conf} -> {key/body_pos_xor, key/joint_conf_xor}"""
    enc = {}
    for key in specs:
        bp, bc = _base(key, specs, inputs, out)
        enc[key + "/body_pos_xor"] = _bits(out[key + "/body_pos"]) ^ _bits(bp)
        enc[key + "/joint_conf_xor"] = _bits(out[key + "/joint_conf"]) ^ _bits(bc)
    return enc


def decode_fixture(z):
    """the stored arrays -> inputs (body_pos, u_noise, z, u_drop), specs, body_names and every key/body_pos, key/joint_conf"""
    import json

    d = decode_inputs(z)
    specs = json.loads(str(z["specs"]))
    d["specs"], d["body_names"] = z["specs"], z["body_names"]
    for key in [BASE_KEY] + [k for k in specs if k != BASE_KEY]:
        bp, bc = _base(key, specs, d, d)
        d[key + "/body_pos"] = (z[key + "/body_pos_xor"] ^ _bits(bp)).view(F)
        d[key + "/joint_conf"] = (z[key + "/joint_conf_xor"] ^ _bits(bc)).view(F)
    return d
