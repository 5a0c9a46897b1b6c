"""Records tests/golden/ball_rollout_oracle.npz: the float64 oracle's trajectories of the free-ball fixture (tests/ball_oracle.py: 10
launches x 60 frames under two settings, the first 8 under a third) and their conditioning under launch perturbations of float32-rounding size.  The oracle takes
seconds per trajectory (it steps a humanoid next to every ball), 252 trajectories in all: recorded once here, read by the GPU tests.
    python tools/gen_golden_ball_rollout.py
"""
import os
import sys
import time

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

from tests import ball_oracle as B  # noqa: E402


def main():
    pos, vel, vspin = B.fixture_launches()
    states = np.stack([B.launch_state(p, v, s) for p, v, s in zip(pos.astype(np.float64), vel.astype(np.float64), vspin.astype(np.float64))])
    out = {"launch_pos": pos, "launch_vel": vel, "launch_vspin": vspin}
    for name, cfg in B.fixture_cfgs().items():
        t = time.time()
        st = states[:B.ENV_LAUNCHES] if name == "task_tgs" else states   # (read by the comparison with the env kernel alone)
        calls, sens = B.rollouts(cfg, st, B.FRAMES)
        out[name + "/calls"], out[name + "/sens"] = calls, sens.astype(np.float32)
        out[name + "/cfg_keys"], out[name + "/cfg"] = B.cfg_arrays(cfg)
        print("%-10s %d launches x %d frames in %.0f s; largest sensitivity of a position %.2e m" % (name, len(st), B.FRAMES, time.time() - t, sens[..., 0:3].max()))
    path = os.path.join(REPO, "tests", "golden", B.GOLDEN)
    np.savez_compressed(path, **out)
    print("wrote", os.path.relpath(path, REPO), "%.2f MB" % (os.path.getsize(path) / 1e6))


if __name__ == "__main__":
    main()
