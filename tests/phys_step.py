"""One control step of the link-per-lane physics kernel from a given state, and the float64 oracle's step from the same state with the
kernel's contact vertices forced: what the phase tests (tests/test_gpu_tree_passes.py, _contact_scan, _walk_up, _sweep_visits,
_walk_down, _rows_points) compare.  States come from tests/phys_poses.py, bounds from tests/gpu_util.py."""
import functools

import numpy as np

from oracle import task_oracle as O
from tests.phys_poses import NB, NSUB

BITS = ("root", "dpos", "dvel", "rb", "cf", "df", "ids_sub")  # what of an env must not depend on the env it shares its wave with


@functools.lru_cache(maxsize=None)
def _mlib():
    from tests.gpu_util import DEV, synth_tables
    from vid2player3d_amd.motion_lib import MotionLib

    return MotionLib(synth_tables(seed=5, num_clips=8, min_frames=60, max_frames=120), DEV)


def kernel_step(root, dpos, dvel, act, build, solver="pgs", contact=True, body_model=None, substep_jobs=None):
    """One control step of build 1 / 2 of the kernel from the state (root [n, 13], dpos, dvel [n, 69]) under the actions act [n, 75]:
    the state after it, forces, the contact vertices of the last substep (`ids`) and of every substep (`ids_sub`), and the PD targets
    and root wrench of the step (checked against the numpy oracle of pre_physics).  body_model, substep_jobs: left to the task's
    defaults unless given."""
    import torch

    from tests.gpu_util import N, T, close, make_task

    n = len(root)
    given = {k: v for k, v in (("body_model", body_model), ("substep_jobs", substep_jobs)) if v is not None}
    task = make_task(n, _mlib(), enable_contact=contact, residual_force_hold="first_sim", debug_contacts=2, pair_envs_by_load=False,
                     kernel_build=build, contact_solver=solver, joint_limits=False, **given)
    task.reset_with_times(None, T(np.full(n, 0.3)))
    task._humanoid_root_states[:] = T(root)
    task._dof_pos[:] = T(dpos)
    task._dof_vel[:] = T(dvel)
    task._reset_env_tensors(None)
    rb0 = N(task._rigid_body_state).reshape(n, NB, 13).copy()
    dpos_before = N(task._dof_pos).copy()
    task.pre_physics_step(T(act))
    task._physics_step()
    torch.cuda.synchronize()
    pd_tar = N(task._pd_target)
    _, pd_ref, _, force, torque = O.pre_physics(act, N(task.reset_buf), dpos_before, rb0[:, 0, 3:7], task.body_model.kp.astype(np.float32))
    close(pd_tar, pd_ref, 1e-6, "pd target")
    got = {"root": N(task._humanoid_root_states), "dpos": N(task._dof_pos), "dvel": N(task._dof_vel), "rb": N(task._rigid_body_state).reshape(n, NB, 13),
           "cf": N(task._contact_forces), "df": N(task.dof_force_tensor), "ids": N(task.debug_contacts()), "ids_sub": N(task.debug_contacts_substeps()),
           "pd": pd_tar, "force": force, "torque": torque}
    name = task.kernel_build()
    task.close()
    assert name.startswith({1: "lds-parked", 2: "registers"}[build])
    return got


def reference(oracle, got, contact=True):
    """The step of a fresh oracle (tests.phys_poses.oracle_for: set to the state `got` started from) under got's PD targets and wrench,
    with got's contact vertices of every substep forced; `sens`: the conditioning of that step (None without contact: not needed)."""
    forced = got["ids_sub"] if contact else None
    args = (got["pd"], got["force"], got["torque"])
    sens = oracle.sensitivity(*args, nsub=NSUB, hold=2, forced_ids=forced, seed=len(got["pd"])) if contact else None
    ref = oracle.step(*args, nsub=NSUB, hold=2, forced_ids=forced, want_selection=True)
    ref["sens"] = sens
    return ref


def assert_oracle_holds_its_own_bound(oracle, inputs, own, what):
    """CPU: the float64 oracle moved by float32 rounding of its inputs (the largest change over 32 perturbed runs, on every element)
    against itself needs the conditioning term in no more envs than rows_close allows - it asserts that cap itself.  oracle: a fresh
    one; inputs: (pd, force, torque); own: the selection of its own step from there."""
    from tests.gpu_util import rows_all  # (imports torch; no GPU is touched here)

    ref = reference(oracle, dict(zip(("pd", "force", "torque"), inputs), ids_sub=own))
    moved = {k: ref[k] + ref["sens"][k] for k in ("root", "dpos", "dvel", "rb", "cf", "df")}
    assert not rows_all(moved, ref, "oracle at float32 rounding, " + what).any()


def assert_env0_ignores_its_partner(a, b):
    """a, b: results of two batches whose env 0 holds the same state beside different partners."""
    assert not np.array_equal(a["dvel"][1], b["dvel"][1]), "the partners must differ"
    for key in BITS:
        assert np.array_equal(a[key][0], b[key][0]), key
