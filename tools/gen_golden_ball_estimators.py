"""Golden data of the two ball estimators, recorded from the reference itself: tests/golden/ball_estimators.npz holds small random
tables, the grids they belong to, query ball states and what the reference's own
`TennisBallOutEstimator.estimate` (vid2player/utils/tennis_ball_out_estimator.py:164-205) and
`TennisBallInEstimator.estimate` (vid2player/utils/tennis_ball_in_estimator.py:48-79) return for them.

The classes are constructed on tables written to temporary .npy files; `est.params` is swapped for a small-grid class afterwards.
On the CPU `Tensor.get_device()` is -1, which `.to(device)` refuses: it is patched HERE to return the tensor's device.  Only arrays are
stored.  Run where the reference exists:
    python tools/gen_golden_ball_estimators.py
"""
import os
import sys
import tempfile

sys.dont_write_bytecode = True  # never leave __pycache__ in the read-only reference mount

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(HERE)
sys.path.insert(0, os.path.join(REPO, "oracle"))
sys.path.insert(0, REPO)

from ref_shim.install import REFERENCE_ROOT, _Sink, install  # noqa: E402

install()
# (utils/tennis_ball.py imports a viewer package that is not part of the reference checkout, and a progress bar: inert stand-ins, as
# ref_shim gives the other absent third-party modules)
for absent in ("smpl_visualizer", "smpl_visualizer.vis_sport", "tqdm"):
    try:
        __import__(absent)
    except ImportError:
        sys.modules[absent] = _Sink(absent)
sys.path.insert(0, os.path.join(REFERENCE_ROOT, "vid2player"))

import torch  # noqa: E402

torch.set_num_threads(1)
torch.Tensor.get_device = lambda self: self.device

import utils.tennis_ball_in_estimator as ref_in  # noqa: E402
import utils.tennis_ball_out_estimator as ref_out  # noqa: E402

OUT = os.path.join(REPO, "tests", "golden", "ball_estimators.npz")


class OutGrid:
    VEL_X_RANGE = (10, 14, 1.0)
    VEL_Y_RANGE = (-2, 2, 1.0)
    VSPIN_RANGE = (-2, 2, 1.0)
    TRAJ_X_RANGE = (0, 10, 0.5)
    TRAJ_Y_RANGE = (0, 3, 0.1)


class InGrid:
    VEL_X_RANGE = (25, 27, 0.5)
    VEL_Y_RANGE = (5, 7, 0.5)
    VSPIN_RANGE = (5, 7, 0.5)
    HEIGHT_RANGE = (0.5, 1.0, 0.1)


def cells(r):
    return int((r[1] - r[0]) / r[2])


def states(rng, n, pos_lo, pos_hi, vel_lo, vel_hi, spin):
    s = np.zeros((n, 13), np.float32)
    s[:, 0:3] = rng.uniform(pos_lo, pos_hi, (n, 3))
    s[:, 6] = 1
    s[:, 7:10] = rng.uniform(vel_lo, vel_hi, (n, 3))
    s[:, 10:13] = rng.normal(0, spin, (n, 3))
    return s


def main():
    rng = np.random.default_rng(2026)
    out = {}
    with tempfile.TemporaryDirectory() as d:
        # ---- outgoing
        nb = cells(OutGrid.VEL_X_RANGE) * cells(OutGrid.VEL_Y_RANGE) * cells(OutGrid.VSPIN_RANGE)
        tx = rng.uniform(-1.5, 2.5, (nb, cells(OutGrid.TRAJ_X_RANGE))).astype(np.float32)
        ty = np.stack([rng.uniform(0, 25, (nb, cells(OutGrid.TRAJ_Y_RANGE))), rng.uniform(0, 2, (nb, cells(OutGrid.TRAJ_Y_RANGE)))], -1).astype(np.float32)
        fx, fy = os.path.join(d, "x.npy"), os.path.join(d, "y.npy")
        np.save(fx, tx); np.save(fy, ty)
        est = ref_out.TennisBallOutEstimator(fx, fy)
        est.params = OutGrid
        # a ball on the player's side (y < 0) flying towards the net: wide ranges so that every clamp is hit - speed below / above the
        # grid, vertical speed in the last cell, spin beyond both ends, height below 0 and in the last cell, net distance beyond both ends
        q = states(rng, 96, [-5, -14, -0.3], [5, 3, 3.4], [-6, 7, -2.6], [6, 16, 2.6], 9.0)
        q[0, 7:10] = [0.5, 13.9, 1.95]      # speed and vertical speed in their last cells
        q[1, 7:10] = [9.0, 13.0, 0.0]       # speed beyond the grid: 'velocity X overflow'
        q[2, 0:3] = [0.0, 2.0, 1.0]; q[2, 7:10] = [0.0, 12.0, 0.0]    # beyond the net already: net distance below the grid
        q[3, 0:3] = [0.0, -13.0, 2.95]; q[3, 7:10] = [0.1, 10.5, 1.0]  # far behind the baseline: net distance beyond the grid; height in the last cell
        q[4, 7:10] = [0.0, 5.0, 0.0]        # invalid contact: too slow
        q[5, 10:13] = 0                     # no spin
        valid, bpos, btime, peak = est.estimate(torch.from_numpy(q))
        assert bpos is not None and 10 < int(valid.sum()) < 90 and int((btime == 0).sum()) > 3 and int((btime != 0).sum()) > 3
        out.update({"out/traj_x": tx, "out/traj_y": ty, "out/query": q, "out/valid": valid.numpy(), "out/bounce_pos": bpos.numpy(), "out/bounce_time": btime.numpy(),
                    "out/max_height": peak.numpy(), "out/grid": np.array([OutGrid.VEL_X_RANGE, OutGrid.VEL_Y_RANGE, OutGrid.VSPIN_RANGE, OutGrid.TRAJ_X_RANGE, OutGrid.TRAJ_Y_RANGE], dtype=np.float64)})
        qn = q[:8].copy()
        qn[:, 8] = 3.0  # none valid
        vn, a, b, c = est.estimate(torch.from_numpy(qn))
        assert a is None and b is None and c is None and not vn.any()
        out.update({"out/query_none": qn, "out/valid_none": vn.numpy()})
        print("outgoing: %d of %d valid, %d into the net" % (int(valid.sum()), len(q), int((btime == 0).sum())))
        # ---- incoming
        nb = cells(InGrid.HEIGHT_RANGE) * cells(InGrid.VEL_X_RANGE) * cells(InGrid.VEL_Y_RANGE) * cells(InGrid.VSPIN_RANGE)
        tab = np.stack([np.cumsum(rng.uniform(0.5, 1.0, (nb, 12)), 1), rng.uniform(0, 2, (nb, 12))], -1).astype(np.float32)
        ft = os.path.join(d, "in.npy")
        np.save(ft, tab)
        ein = ref_in.TennisBallInEstimator(ft)
        ein.params = InGrid
        qi = states(rng, 64, [-4, -12, 0.2], [4, -2, 1.4], [-8, 20, 4], [8, 30, 8], 45.0)
        traj, s_in, s_out = ein.estimate(torch.from_numpy(qi))
        out.update({"in/table": tab, "in/query": qi, "in/traj": traj.numpy(), "in/states_in": s_in.numpy(), "in/states_out": s_out.numpy(),
                    "in/grid": np.array([InGrid.VEL_X_RANGE, InGrid.VEL_Y_RANGE, InGrid.VSPIN_RANGE, InGrid.HEIGHT_RANGE], dtype=np.float64)})
        print("incoming: %d queries, trajectories %s" % (len(qi), tuple(traj.shape)))
    np.savez_compressed(OUT, **out)
    print("wrote", os.path.relpath(OUT, REPO), "%.2f MB" % (os.path.getsize(OUT) / 1e6))


if __name__ == "__main__":
    main()
