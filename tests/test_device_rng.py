"""CPU checks of the controller kernels' random generator: csrc/philox.hpp and its numpy statement vid2player3d_amd/device_rng.py.

Known answers of Philox4x32-10 (the Random123 test vectors), the same words from a stand-alone host program that includes the header
(built with the address and undefined-behaviour sanitizers), the edges of the three laws, the moments of the clamped normals and of the
integer law, the numpy statement of the controller's action step, and the argument checks of `v2p_controller_actions`."""
import ctypes as C
import math
import os
import shutil
import subprocess

import numpy as np
import pytest

from vid2player3d_amd import device_rng as R

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(REPO, "vid2player3d_amd", "csrc")

KNOWN = (  # counter, key, output (Random123 kat_vectors, philox4x32 10 rounds)
    ((0, 0, 0, 0), (0, 0), "6627e8d5 e169c58d bc57ac4c 9b00dbd8"),
    ((0xFFFFFFFF,) * 4, (0xFFFFFFFF,) * 2, "408f276d 41c83b0e a20bc7c6 6d5451fd"),
    ((0x243F6A88, 0x85A308D3, 0x13198A2E, 0x03707344), (0xA4093822, 0x299F31D0), "d16cfe09 94fdcceb 5001e420 24126ea1"),
)
SEED, CALL = 0x5EEDC0FFEE123457, (1 << 32) + 5  # fixed once: the stream is deterministic, so are the tests below


def hexwords(w):
    return " ".join("%08x" % int(x) for x in w)


def test_philox_known_answers():
    for counter, key, want in KNOWN:
        assert hexwords(R.philox4x32(counter, key)) == want
    both = R.philox4x32([k[0] for k in KNOWN[:2]], [k[1] for k in KNOWN[:2]])  # (arrays of counters)
    assert [hexwords(w) for w in both] == [k[2] for k in KNOWN[:2]]


def test_words_are_the_counter_layout():
    """philox_words: counter (env, block | stream << 28, call_lo, call_hi), key (seed_lo, seed_hi); word 4b + j = word j of block b"""
    w = R.philox_words(SEED, CALL, R.STREAM_RESET, 5, 3)
    assert w.shape == (5, 12) and w.dtype == np.uint32
    key = (SEED & 0xFFFFFFFF, SEED >> 32)
    for env in (0, 4):
        for block in (0, 2):
            want = R.philox4x32((env, block | (1 << 28), CALL & 0xFFFFFFFF, CALL >> 32), key)
            assert np.array_equal(w[env, 4 * block:4 * block + 4], want)
    whole = R.philox_words(SEED, CALL, R.STREAM_RESET, 1, 1, envs=[R.WHOLE_CALL])
    assert np.array_equal(whole[0], R.philox4x32((0xFFFFFFFF, 1 << 28, CALL & 0xFFFFFFFF, CALL >> 32), key))
    # a draw depends on (seed, call, stream, env, block) alone
    assert np.array_equal(R.philox_words(SEED, CALL, R.STREAM_RESET, 3, 2), w[:3, :8])
    for other in (R.philox_words(SEED + 1, CALL, R.STREAM_RESET, 5, 3), R.philox_words(SEED, CALL + 1, R.STREAM_RESET, 5, 3), R.philox_words(SEED, CALL, R.STREAM_WALK, 5, 3)):
        assert not (other == w).any(1).any()


HOST_PROGRAM = r'''
#include <stdio.h>
#include "philox.hpp"
int main() {
    const uint32_t c[3][4] = {{0, 0, 0, 0}, {0xffffffffu, 0xffffffffu, 0xffffffffu, 0xffffffffu}, {0x243f6a88u, 0x85a308d3u, 0x13198a2eu, 0x03707344u}};
    const uint32_t k[3][2] = {{0, 0}, {0xffffffffu, 0xffffffffu}, {0xa4093822u, 0x299f31d0u}};
    uint32_t w[4];
    for (int i = 0; i < 3; ++i) {
        v2p::philox4x32_10(c[i], k[i], w);
        printf("%08x %08x %08x %08x\n", w[0], w[1], w[2], w[3]);
    }
    v2p::philox_block(0x5EEDC0FFEE123457ull, (1ull << 32) + 5, v2p::PHILOX_STREAM_RESET, 4, 2, w);
    printf("%08x %08x %08x %08x\n", w[0], w[1], w[2], w[3]);
    v2p::philox_block(0x5EEDC0FFEE123457ull, (1ull << 32) + 5, v2p::PHILOX_STREAM_WALK, v2p::PHILOX_WHOLE_CALL, 0, w);
    printf("%08x %08x %08x %08x\n", w[0], w[1], w[2], w[3]);
    // the laws at their edges and on the words above
    printf("%lld %lld %lld %lld\n", (long long)v2p::philox_integer(0u, -5, 5), (long long)v2p::philox_integer(0xffffffffu, -5, 5),
           (long long)v2p::philox_integer(0u, -1000, 1000), (long long)v2p::philox_integer(0xffffffffu, -1000, 1000));
    printf("%.9g %.9g\n", (double)v2p::philox_uniform(0u), (double)v2p::philox_uniform(0xffffffffu));
    float z0, z1;
    v2p::philox_normal_pair(0u, 0u, &z0, &z1);
    printf("%.9g %.9g\n", (double)z0, (double)z1);
    v2p::philox_normal_pair(w[0], w[1], &z0, &z1);
    printf("%.9g %.9g %.9g\n", (double)z0, (double)z1, (double)v2p::philox_clamp(z0 * 100.f, 5.f));
    return 0;
}
'''


def test_host_program_prints_the_same_words(tmp_path):
    """The header in a stand-alone host program, under the address and undefined-behaviour sanitizers, run directly."""
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        pytest.fail("hipcc not found: the header cannot be compiled")
    src, exe = tmp_path / "philox_host.cpp", tmp_path / "philox_host"
    src.write_text(HOST_PROGRAM)
    subprocess.check_call([hipcc, "-x", "hip", "--cuda-host-only", "-O1", "-ffp-contract=off", "-std=c++17", "-I", CSRC, "-Xarch_host", "-fsanitize=address,undefined",
                           "-Xarch_host", "-fno-sanitize-recover=all", str(src), "-o", str(exe)])
    out = subprocess.run([str(exe)], stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=60)
    assert out.returncode == 0, out.stderr.decode()
    lines = out.stdout.decode().strip().split("\n")
    assert lines[:3] == [k[2] for k in KNOWN]
    assert lines[3] == hexwords(R.philox_words(SEED, CALL, R.STREAM_RESET, 5, 3)[4, 8:12])
    whole = R.philox_words(SEED, CALL, R.STREAM_WALK, 1, 1, envs=[R.WHOLE_CALL])[0]
    assert lines[4] == hexwords(whole)
    assert [int(x) for x in lines[5].split()] == [-5, 4, -1000, 999]
    assert [np.float32(x) for x in lines[6].split()] == [0.0, np.float32(1.0 - 2.0 ** -24)]  # (9 digits name a float32)
    top = [float(x) for x in lines[7].split()]
    assert abs(top[0] - R.LARGEST_NORMAL) < 1e-6 and top[1] == 0.0
    z = R.normals(whole[:2])
    got = [float(x) for x in lines[8].split()]
    # (two libms: the host's logf / sincosf against numpy's, a few units in the last place of values below 6)
    assert abs(got[0] - z[0]) < 4e-6 and abs(got[1] - z[1]) < 4e-6 and got[2] == math.copysign(5.0, got[0])


def test_law_edges():
    edge = np.array([0, 0xFFFFFFFF], np.uint32)
    for lo, hi in ((-5, 5), (-1000, 1000), (0, 1), (0, 2500), (-2 ** 31, 2 ** 31)):
        assert R.integer(edge, lo, hi).tolist() == [lo, hi - 1]
    assert R.uniform(edge).tolist() == [0.0, float(np.float32(1.0 - 2.0 ** -24))] and R.uniform(edge).dtype == np.float32
    # u1 is never 0: the smallest is 2^-24 (w0 = 0), the largest 1 (r = 0)
    z = R.normals(np.array([[0, 0], [0xFFFFFFFF, 0], [0, 0x40000000], [255, 0xFFFFFFFF]], np.uint32))
    assert np.isfinite(z).all()
    assert abs(z[0, 0] - R.LARGEST_NORMAL) < 1e-6 and z[0, 1] == 0 and z[1].tolist() == [0.0, 0.0]
    assert abs(z[2, 1] - R.LARGEST_NORMAL) < 1e-6 and abs(z[2, 0]) < 1e-6, "a quarter turn: the sine carries r"
    assert R.LARGEST_NORMAL > 5.0, "the reference's clamp at 5 is reachable"
    c = R.clamped_normals(R.philox_words(SEED, CALL, R.STREAM_WALK, 4096, 8), 1.0)
    assert c.max() == 1.0 and c.min() == -1.0 and (c == 1.0).sum() > 100 and (c == -1.0).sum() > 100
    assert np.array_equal(c, np.clip(R.normals(R.philox_words(SEED, CALL, R.STREAM_WALK, 4096, 8)), -1, 1))


def clamped_normal_moments(c):
    """mean, variance and the variance of the squares of clamp(N(0,1), -c, c)"""
    phi = math.exp(-c * c / 2) / math.sqrt(2 * math.pi)
    tail = 0.5 * math.erfc(c / math.sqrt(2))
    inside = 1 - 2 * tail
    m2 = inside - 2 * c * phi + 2 * c * c * tail
    m4 = 3 * inside - 2 * (c ** 3 + 3 * c) * phi + 2 * c ** 4 * tail
    return 0.0, m2, m4 - m2 * m2


@pytest.mark.parametrize("clamp", [5.0, 1.0])
def test_moments_of_the_clamped_normals(clamp):
    z = R.clamped_normals(R.philox_words(SEED, CALL, R.STREAM_WALK, 4096, 8), clamp).astype(np.float64)
    assert z.shape == (4096, 32)
    n = z.size
    mean, var, var_of_squares = clamped_normal_moments(clamp)
    print("clamp %g: mean %+.5f (se %.5f), variance %.5f against %.5f (se %.5f)" % (clamp, z.mean(), math.sqrt(var / n), (z * z).mean(), var, math.sqrt(var_of_squares / n)))
    assert abs(z.mean() - mean) < 5 * math.sqrt(var / n)
    assert abs((z * z).mean() - var) < 5 * math.sqrt(var_of_squares / n)
    # columns are as good as rows: no column (a fixed word of a fixed block) is off
    assert (np.abs(z.mean(0)) < 5 * math.sqrt(var / 4096)).all()


@pytest.mark.parametrize("span", [(-5, 5), (-1000, 1000), (0, 64)])
def test_integer_law_is_uniform(span):
    lo, hi = span
    w = R.philox_words(SEED, CALL, R.STREAM_RESET, 8192, 2).reshape(-1)
    assert w.size == 65536
    k = R.integer(w, lo, hi)
    assert k.min() >= lo and k.max() < hi
    cells = hi - lo
    counts = np.bincount(k - lo, minlength=cells)
    p = 1.0 / cells
    se = math.sqrt(w.size * p * (1 - p))
    print("[%d, %d): counts %d .. %d, expected %.1f, se %.1f" % (lo, hi, counts.min(), counts.max(), w.size * p, se))
    assert (np.abs(counts - w.size * p) < 5 * se).all()
    u = R.uniform(w).astype(np.float64)
    assert abs(u.mean() - 0.5) < 5 * math.sqrt(1 / 12 / w.size) and u.min() >= 0 and u.max() < 1


# ------------------------------------------------------------------------------------------------------------------ the statement
def test_action_statement_is_the_reference_law():
    """`controller_actions_reference` against pre_physics_step (physics_mvae_controller.py:247-266) said again line by line in torch on
    the CPU, the normals served from the statement's own words, env i owning its draws."""
    import torch

    from vid2player3d_amd.tasks import tennis_controller as tc

    rng = np.random.default_rng(11)
    n = 12
    for nr, nroot, walk in ((3, 3, True), (3, 0, True), (0, 0, True), (3, 3, False)):
        st = tc.action_settings(num_res_dof=nr, num_res_root=nroot, vae_action_scale=1.5, residual_dof_scale=0.4, residual_root_scale=0.02, random_walk=walk, seed=SEED)
        actions = rng.normal(0, 1, (n, 32 + nr + nroot + 3)).astype(np.float32)
        tar_action = (np.arange(n) % 3 != 0).astype(np.int64)
        words = R.philox_words(SEED, 7, R.STREAM_WALK, n, 8)
        got = tc.controller_actions_reference(st, actions, tar_action, words)
        a = torch.from_numpy(actions)
        mvae_actions = a[:, :32].clone() * 1.5
        if walk:
            in_recovery = torch.from_numpy(tar_action) == 0
            draws = torch.clamp(torch.from_numpy(R.normals(words)), -5, 5)
            mvae_actions[in_recovery] = draws[in_recovery]
        assert np.array_equal(got["actions_out"], actions[:, :32 + nr + nroot])
        assert np.array_equal(got["mvae_actions"], mvae_actions.numpy())
        assert np.array_equal(got["res_dof_actions"], (a[:, 32:32 + nr].clone() * 0.4).numpy())
        assert np.array_equal(got["res_root_actions"], (a[:, 32 + nr:32 + nr + nroot].clone() * 0.02).numpy())
        assert all(v.dtype == np.float32 for v in got.values())
        if walk:
            rec = tar_action == 0
            assert rec.sum() == 4 and not np.array_equal(got["mvae_actions"][rec], actions[rec, :32] * np.float32(1.5))
            assert np.abs(got["mvae_actions"][rec]).max() <= 5.0


# ------------------------------------------------------------------------------------------------------------------ the entry
def test_entry_refuses_bad_arguments_without_a_gpu():
    from vid2player3d_amd import _lib

    L = _lib.load()
    one = 16  # (a non-null placeholder: every call below is refused before anything is dereferenced)
    fn = L.v2p_controller_actions

    def cfg(**kw):
        d = dict(num_res_dof=3, num_res_root=3, random_walk=1, vae_action_scale=1.5, residual_dof_scale=0.4, residual_root_scale=0.02, clamp=5.0, seed=1, call=0)
        d.update(kw)
        return _lib.ControllerActionsCfg(**d)

    def buf(**kw):
        d = dict(actions=one, actions_stride=38, tar_action=one, words=None, actions_out=one, mvae_actions=one, res_dof_actions=one, res_root_actions=one)
        d.update(kw)
        return _lib.ControllerActionsBuffers(**d)

    refused = [(None, 4, buf()), (cfg(), 4, None), (cfg(), -1, buf()), (cfg(), 2 ** 31, buf()), (cfg(num_res_dof=-1), 4, buf()), (cfg(num_res_root=-1), 4, buf()),
               (cfg(), 4, buf(actions_stride=37)), (cfg(clamp=-1.0), 4, buf()), (cfg(clamp=float("nan")), 4, buf()), (cfg(), 4, buf(actions=None)),
               (cfg(), 4, buf(tar_action=None)), (cfg(), 4, buf(actions_out=None)), (cfg(), 4, buf(mvae_actions=None)), (cfg(), 4, buf(res_dof_actions=None)),
               (cfg(), 4, buf(res_root_actions=None))]
    for c, n, b in refused:
        assert fn(None if c is None else C.byref(c), n, None if b is None else C.byref(b), None) == -1
        assert b"v2p_controller_actions" in L.v2p_last_error()
    # n = 0 is a no-op, null buffers and all
    c, b = cfg(), buf(actions=None, tar_action=None, actions_out=None, mvae_actions=None, res_dof_actions=None, res_root_actions=None)
    assert fn(C.byref(c), 0, C.byref(b), None) == 0
    assert L.v2p_abi_version() == 15


def test_struct_sizes_match_the_header(tmp_path):
    from vid2player3d_amd import _lib

    prog = r'''
#include <stdio.h>
#include <stddef.h>
#include "v2p_rollout.h"
int main(void){ printf("%zu %zu %zu %zu\n", sizeof(v2p_controller_actions_cfg), sizeof(v2p_controller_actions_buffers), offsetof(v2p_controller_actions_cfg, seed),
                       offsetof(v2p_controller_actions_buffers, mvae_actions)); return 0; }
'''
    src, exe = tmp_path / "s.c", tmp_path / "s"
    src.write_text(prog)
    subprocess.check_call(["gcc", "-I", os.path.join(REPO, "include"), str(src), "-o", str(exe)])
    sizes = [int(x) for x in subprocess.check_output([str(exe)]).split()]
    assert sizes == [C.sizeof(_lib.ControllerActionsCfg), C.sizeof(_lib.ControllerActionsBuffers), _lib.ControllerActionsCfg.seed.offset,
                     _lib.ControllerActionsBuffers.mvae_actions.offset]
