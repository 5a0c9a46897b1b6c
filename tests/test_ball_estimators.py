"""The two ball estimators against the reference's own (tests/golden/ball_estimators.npz, recorded by tools/gen_golden_ball_estimators.py
from vid2player/utils/tennis_ball_out_estimator.py and tennis_ball_in_estimator.py on small random tables): CPU tensors - the torch
paths are the same on any device.  The queries of the golden hit every clamp of the index arithmetic, invalid contacts, balls into the
net and the none-valid return."""
import os

import numpy as np
import pytest
import torch

from vid2player3d_amd import ball_traj

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "ball_estimators.npz")
TOL = 1e-6


@pytest.fixture(scope="module")
def gold():
    return np.load(GOLDEN)


def grid_class(rows, names):
    return type("Grid", (), {n: tuple(float(x) for x in r) for n, r in zip(names, rows)})


def near(a, b, what):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    assert a.shape == b.shape, (what, a.shape, b.shape)
    assert np.abs(a - b).max() <= TOL * max(1.0, np.abs(b).max()), "%s: max abs err %.3e" % (what, np.abs(a - b).max())


def out_estimator(gold):
    grid = grid_class(gold["out/grid"], ("VEL_X_RANGE", "VEL_Y_RANGE", "VSPIN_RANGE", "TRAJ_X_RANGE", "TRAJ_Y_RANGE"))
    return ball_traj.TennisBallOutEstimator(gold["out/traj_x"], gold["out/traj_y"], params=grid)


def test_out_estimator_reproduces_the_reference(gold):
    est = out_estimator(gold)
    q = torch.from_numpy(gold["out/query"])
    valid, bpos, btime, peak = est.estimate(q)
    assert np.array_equal(valid.numpy(), gold["out/valid"])
    near(bpos, gold["out/bounce_pos"], "bounce_pos")
    near(btime, gold["out/bounce_time"], "bounce_time")
    near(peak, gold["out/max_height"], "max_height")
    assert bpos.dtype == btime.dtype == peak.dtype == torch.float32
    # balls into the net come back as zeros, at the rows where the reference has them
    assert np.array_equal(btime.numpy() == 0, gold["out/bounce_time"] == 0) and (gold["out/bounce_time"] == 0).sum() > 3
    # 'velocity X overflow' is counted, not printed
    vx = np.linalg.norm(gold["out/query"][gold["out/valid"]][:, 7:9], axis=1)
    assert int(est.vel_x_overflow) == int((vx >= est.params.VEL_X_RANGE[1]).sum()) > 0
    assert torch.equal(q, torch.from_numpy(gold["out/query"])), "the query is not edited"


def test_out_estimator_clamps_are_exercised(gold):
    """The golden's queries reach both ends of every index: otherwise the comparison above would not see a wrong clamp."""
    est = out_estimator(gold)
    b = torch.from_numpy(gold["out/query"][gold["out/valid"]])
    P = est.params
    vspin = b[:, 10:13].norm(dim=1) / (np.pi * 2)
    assert (vspin > P.VSPIN_RANGE[1]).any() and (b[:, 7:9].norm(dim=1) > P.VEL_X_RANGE[1] - P.VEL_X_RANGE[2]).any()
    assert (b[:, 9] > P.VEL_Y_RANGE[1] - P.VEL_Y_RANGE[2]).any()
    assert (b[:, 2] < 0).any() and (b[:, 2] > P.TRAJ_Y_RANGE[1] - P.TRAJ_Y_RANGE[2]).any()
    net = -b[:, 1] / b[:, 8] * b[:, 7:9].norm(dim=1)
    assert (net < 0).any() and (net > P.TRAJ_X_RANGE[1]).any()
    idx = est.get_ball_traj_out_index(b[:, 7:9].norm(dim=1), b[:, 9], vspin)
    assert idx.min() >= 0 and idx.max() < len(gold["out/traj_x"]) and idx.dtype == torch.int64


def test_out_estimator_none_valid(gold):
    est = out_estimator(gold)
    valid, bpos, btime, peak = est.estimate(torch.from_numpy(gold["out/query_none"]))
    assert bpos is None and btime is None and peak is None
    assert np.array_equal(valid.numpy(), gold["out/valid_none"]) and not valid.any()


def test_in_estimator_reproduces_the_reference(gold):
    grid = grid_class(gold["in/grid"], ("VEL_X_RANGE", "VEL_Y_RANGE", "VSPIN_RANGE", "HEIGHT_RANGE"))
    est = ball_traj.TennisBallInEstimator(gold["in/table"], params=grid)
    q = torch.from_numpy(gold["in/query"])
    traj, s_in, s_out = est.estimate(q)
    near(traj, gold["in/traj"], "traj_trans")
    near(s_in, gold["in/states_in"], "ball_states_in")
    near(s_out, gold["in/states_out"], "ball_states_out")
    # every clamp of the four indices is reached by the queries
    h, vx, vy = q[:, 2], q[:, 7:9].norm(dim=1), q[:, 9]
    vs = q[:, 10:13].norm(dim=1) / (np.pi * 2)
    for v, r in ((h, grid.HEIGHT_RANGE), (vx, grid.VEL_X_RANGE), (vy, grid.VEL_Y_RANGE), (vs, grid.VSPIN_RANGE)):
        assert (v < r[0]).any() and (v > r[1] - r[2]).any(), r
    assert torch.equal(q, torch.from_numpy(gold["in/query"]))


def test_default_grids_are_the_references():
    assert ball_traj.traj_out_params.VEL_X_RANGE == (10, 65, 0.1) and ball_traj.traj_out_params.TRAJ_X_RANGE == (0, 30, 0.5)
    assert ball_traj.grid_cells(ball_traj.traj_out_params.TRAJ_X_RANGE) == 60 and ball_traj.grid_cells(ball_traj.traj_out_params.TRAJ_Y_RANGE) == 30
    assert ball_traj.traj_in_params.HEIGHT_RANGE == (0.5, 2, 0.1)
