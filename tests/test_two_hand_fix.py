"""The two-hand backhand fix on the CPU: the numpy statement `two_hand_fix_reference` against what the reference's own
`optimize_two_hand_backhand(single=True)` returned (tests/golden/two_hand_fix.npz, recorded by tools/gen_golden_two_hand_fix.py), its
hand-written gradient against torch autograd over the reference's own forward functions, and the laws around it."""
import os

import numpy as np
import pytest

from vid2player3d_amd import _lib, two_hand_fix as thf
from vid2player3d_amd.model import load_baked_model
from vid2player3d_amd.ref_rotations import angle_axis_to_rotmat_reference

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "two_hand_fix.npz")
CASES = ("right_one_shape", "left_two_shapes", "right_two_frames", "left_one_frame")


@pytest.fixture(scope="module")
def fx():
    with np.load(GOLDEN) as z:
        return {k: z[k] for k in z.files}


@pytest.fixture(scope="module")
def st():
    m = load_baked_model()
    return thf.fix_settings(m.body_names, m.parents)


@pytest.fixture(scope="module")
def runs(fx, st):
    """the statement over every case and iteration count, float32 and float64, computed once: {(case, iters, dt): (out, info)}"""
    out = {}
    for name in CASES:
        for iters in fx[name + "/iters"]:
            for dt in (np.float32, np.float64):
                info = {}
                o = thf.two_hand_fix_reference(st, fx[name + "/joint_rot"], fx[name + "/phase"], fx[name + "/swing_type"], bool(fx[name + "/righthand"]), fx[name + "/bind"],
                                               int(iters), dt, info)
                out[(name, int(iters), dt)] = (o, info)
    return out


def test_fixture_holds_the_cases_the_law_needs(fx):
    hands = {bool(fx[c + "/righthand"]) for c in CASES}
    rows = {len(fx[c + "/bind"]) for c in CASES}
    counts = sorted(int(thf.need_fix_reference(fx[c + "/phase"], fx[c + "/swing_type"]).sum()) for c in CASES)
    assert hands == {True, False} and rows == {1, 2} and counts == [1, 2, 12, 12]
    for c in CASES:
        assert list(fx[c + "/iters"]) == [1, 5, 20, 500]
        frames = np.flatnonzero(thf.need_fix_reference(fx[c + "/phase"], fx[c + "/swing_type"]))
        if len(frames) == 12:  # two separate swings, a gap between them; unflagged frames of every kind
            assert (np.diff(frames) > 1).sum() == 1
        off = np.ones(len(fx[c + "/phase"]), bool)
        off[frames] = False
        sw, ph = fx[c + "/swing_type"][off], fx[c + "/phase"][off]
        assert (sw != 2).any() and ((sw == 2) & (ph <= 2)).any() and ((sw == 2) & (ph >= 5)).any()


@pytest.mark.parametrize("name", CASES)
def test_gradient_against_autograd_over_the_references_functions(fx, st, name):
    """the statement's hand-written gradient of the `target` loss in float64 against torch autograd over the reference's own
    `angle_axis_to_rotation_matrix` and `_smpl_to_sim` in float64 (recorded), at random free-arm angles on both branches of Rodrigues.
    Bound 1e-9 absolute: far above float64 rounding, five orders below the smallest term of the law, 0.2 / (12 F)."""
    dt = np.float64
    frames = np.flatnonzero(thf.need_fix_reference(fx[name + "/phase"], fx[name + "/swing_type"]))
    F, rh, bind = len(frames), bool(fx[name + "/righthand"]), fx[name + "/bind"].astype(dt)
    r, want = fx["grad/" + name + "/r"], fx["grad/" + name + "/grad"]
    theta2 = (r ** 2).sum(-1)
    assert (theta2 <= 1e-6).any() and (theta2 > 1e-6).any(), "both branches"
    rotmat = angle_axis_to_rotmat_reference(fx[name + "/joint_rot"][frames].astype(dt), dt)
    con = thf.fix_constants(st, rotmat, bind[np.arange(F) % len(bind)], rh, dt)
    got = thf.free_hand_reference(r, con, dt, dt(1) / dt(3 * F))[2]
    err = float(np.abs(got - want).max())
    print("%s: gradient error %.3g (largest component %.3g)" % (name, err, np.abs(want).max()))
    assert np.abs(want).max() > 1e-3 and err < 1e-9


@pytest.mark.parametrize("name", CASES)
@pytest.mark.parametrize("iters", [1, 5, 20, 500])
@pytest.mark.parametrize("dt", [np.float32, np.float64])
def test_statement_lies_within_the_references_own_scatter(fx, runs, name, iters, dt):
    """the free arm's angles of the flagged frames: within 3 x scatter_max and 2 x scatter_rms of the reference's output, the scatter
    being that of eight reference runs whose input is nudged by 1e-6 (eight samples underestimate a tail: hence the factors).  At one
    iteration the scatter is a few 1e-6 and this is a check of every gradient's sign (a wrong sign: 0.01)."""
    k = "%s/%d/" % (name, iters)
    frames = np.flatnonzero(thf.need_fix_reference(fx[name + "/phase"], fx[name + "/swing_type"]))
    ik = list(thf.IK_JOINTS[bool(fx[name + "/righthand"])])
    got, want = runs[(name, iters, dt)][0], fx[k + "out"]
    dev = got[frames][:, ik].astype(np.float64) - want[frames][:, ik]
    worst, rms = float(np.abs(dev).max()), float(np.sqrt((dev ** 2).mean()))
    print("%s %s: max %.3g (scatter %.3g) rms %.3g (scatter %.3g)" % (k, dt.__name__, worst, fx[k + "scatter_max"], rms, fx[k + "scatter_rms"]))
    assert worst <= 3 * fx[k + "scatter_max"] and rms <= 2 * fx[k + "scatter_rms"]
    # the other joints of the flagged frames: a round trip, a few ulps from the reference's; every other frame: the reference's bits
    others = [j for j in range(24) if j not in ik]
    assert np.abs(got[frames][:, others].astype(np.float64) - want[frames][:, others]).max() < 2e-6
    off = np.ones(len(want), bool)
    off[frames] = False
    assert np.array_equal(got[off].astype(np.float32), want[off])


@pytest.mark.parametrize("name", CASES)
@pytest.mark.parametrize("iters", [1, 5, 20, 500])
def test_final_target_loss_is_no_larger_than_the_references(fx, runs, name, iters):
    """The `target` loss a run ends with (the last line the reference prints), float32 and float64, at every recorded step count: no
    larger than the largest of the reference's nine runs plus their own range, `loss_max + (loss_max - loss_min)`.  The margin: the
    statement is one more sample of what the nine runs sample, and a tenth sample lies above the largest of nine one time in ten - of
    the 32 samples here about three; the nine runs' range is the fixture's own measure of how wide that distribution is, so one range
    above the largest is where a sample of the same law may lie and a law that descends more slowly may not for long (at 500 steps
    the range is 1e-4 to 2e-3 of a loss that fell by 0.5).  Where the nine runs all but coincide (one step; one frame) the range is a few
    1e-7 and what is left is the number format: the reference's figure is a float32 mean of 3F terms, whose summation rounds by at most half an ulp
    per term, 3F x 2^-24 of the loss, while the statement's figure is formed in double."""
    k = "%s/%d/" % (name, iters)
    terms = 3 * int(thf.need_fix_reference(fx[name + "/phase"], fx[name + "/swing_type"]).sum())
    bound = fx[k + "loss_max"] + (fx[k + "loss_max"] - fx[k + "loss_min"]) + terms * 2.0 ** -24 * fx[k + "loss_max"]
    for dt in (np.float32, np.float64):
        loss = runs[(name, iters, dt)][1]["target_loss"]
        print("%s %s: target loss %.9g, the reference's nine runs %.9g .. %.9g, bound %.9g" % (k, dt.__name__, loss, fx[k + "loss_min"], fx[k + "loss_max"], bound))
        assert loss <= bound


def test_unflagged_frames_are_copied_and_no_flag_returns_a_copy(fx, st):
    name = CASES[0]
    jr, phase, swing, bind = fx[name + "/joint_rot"], fx[name + "/phase"], fx[name + "/swing_type"], fx[name + "/bind"]
    frames = thf.need_fix_reference(phase, swing)
    out = thf.two_hand_fix_reference(st, jr, phase, swing, True, bind, 3)
    assert out.dtype == np.float32 and np.array_equal(out[~frames].view(np.uint32), jr[~frames].view(np.uint32)) and not np.array_equal(out[frames], jr[frames])
    none = thf.two_hand_fix_reference(st, jr, np.zeros_like(phase), swing, True, bind, 3)  # F = 0
    assert none is not jr and np.array_equal(none.view(np.uint32), jr.view(np.uint32))
    # the window is open at both ends, and only swing type 2 counts
    assert list(thf.need_fix_reference([2.0, 2.5, 5.0, 3.0, np.nan], [2, 2, 2, 1, 2])) == [False, True, False, False, False]


def test_a_federer_side_is_skipped():
    assert thf.skips_fix("federer") and thf.skips_fix("federer_v2") and not thf.skips_fix("nadal") and not thf.skips_fix("djokovic") and not thf.skips_fix(None)


def test_the_cap_is_refused_by_its_message(st, fx):
    assert thf.MAX_FRAMES >= 1800, "the reference's record length fits"
    assert thf.MAX_FRAMES == _lib.TWO_HAND_FIX_THREADS * _lib.TWO_HAND_FIX_FRAMES_PER_THREAD and 48 * thf.MAX_FRAMES <= 160 * 1024
    n = thf.MAX_FRAMES + 1
    jr = np.zeros((n, 24, 3), np.float32)
    with pytest.raises(ValueError, match="%d flagged frames in one track, above the cap of %d" % (n, thf.MAX_FRAMES)):
        thf.two_hand_fix_reference(st, jr, np.full(n, 3.0, np.float32), np.full(n, 2), True, fx[CASES[0] + "/bind"], 1)
    thf.check_frames(thf.MAX_FRAMES)


def test_adam_terms_are_torchs_for_every_step_up_to_500():
    """the running products in double give, rounded to float32, what torch forms from `beta ** step` in double"""
    step, bc2 = thf.adam_terms(500)
    for t in range(1, 501):
        assert np.float32(step[t - 1]) == np.float32(thf.LR / (1 - thf.BETA1 ** t)) and np.float32(bc2[t - 1]) == np.float32((1 - thf.BETA2 ** t) ** 0.5), t


def test_header_constants_and_entry_are_bound():
    import re

    src = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "v2p_rollout.h")).read()
    assert int(re.search(r"#define V2P_TWO_HAND_FIX_THREADS (\d+)", src).group(1)) == _lib.TWO_HAND_FIX_THREADS
    assert int(re.search(r"#define V2P_TWO_HAND_FIX_FRAMES_PER_THREAD (\d+)", src).group(1)) == _lib.TWO_HAND_FIX_FRAMES_PER_THREAD
    assert "v2p_two_hand_fix" in _lib.EXPORTED_SYMBOLS and _lib.ABI_VERSION == 15
    L = _lib.load()
    assert L.v2p_abi_version() == 15
    # refused before any HIP call
    import ctypes as C

    m = load_baked_model()
    c = thf.cfg_struct(thf.fix_settings(m.body_names, m.parents), 5, 1)
    b = _lib.TwoHandFixBuffers(**{k: 16 for k in _lib.TWO_HAND_FIX_BUFFER_NAMES})
    assert L.v2p_two_hand_fix(None, 1, 1, C.byref(b), None) == -1
    assert L.v2p_two_hand_fix(C.byref(c), 1, 0, C.byref(b), None) == -1 and b"track_length" in L.v2p_last_error()
    assert L.v2p_two_hand_fix(C.byref(c), 1, 4, C.byref(b), None) == -1 and b"out is joint_rot" in L.v2p_last_error()
    b.out = 16 + 4 * 72 * 4 - 4  # (the last float of joint_rot)
    assert L.v2p_two_hand_fix(C.byref(c), 1, 4, C.byref(b), None) == -1 and b"out overlaps joint_rot" in L.v2p_last_error()
    b.out = 16 + 4 * 72 * 4
    b.bind = None
    assert L.v2p_two_hand_fix(C.byref(c), 1, 4, C.byref(b), None) == -1 and b"null array" in L.v2p_last_error()
    b.bind = 16
    bad = thf.cfg_struct(thf.fix_settings(m.body_names, m.parents), 5, 1)
    bad.smpl_parents[20] = 3
    assert L.v2p_two_hand_fix(C.byref(bad), 1, 4, C.byref(b), None) == -1 and b"free arm" in L.v2p_last_error()
    c.num_iters = -1
    assert L.v2p_two_hand_fix(C.byref(c), 1, 4, C.byref(b), None) == -1 and b"num_iters" in L.v2p_last_error()
    c.num_iters = 5
    assert L.v2p_two_hand_fix(C.byref(c), 0, 4, C.byref(b), None) == 0, "no track: a no-op"
