"""The arithmetic of two level loops of the link-per-lane physics kernel as it is formed since 2026-10-20 (csrc/physics_ll.hip, forms LAMX
and P2SHIFT of csrc/ll_forms.hpp), in numpy, without a GPU.

A level of the Lambda recursion:  Lambda_b = [Di 0; 0 0] + T^T G T,  T = [P, 0; -E^T, 1],  P = aug Di,  G = [Ga Gb; Gb^T Gc].  By blocks
    Lam.B = P Gb - E Gc      M1 = P Ga - E Gb^T  ( = H1^T, which the joint-limit rows read )      Lam.A = Di + M1 P - Lam.B E^T      Lam.C = Gc
each entry as aug (Di . G) - E . G in seven fused multiply-adds (the scale on the finished dot: P rounded entry by entry first is one
instruction less per entry and up to three times the error where the dot cancels, printed below), of the symmetric Lam.A the upper
triangle.  The earlier form went through H1 = Ga P - Gb E^T, H2 = Gb^T P - Gc E^T ( = Lam.B^T, the same nine entries ) and
t = P H1 - E H2 (all nine entries, the off-diagonal pairs averaged).
Pass 2's shift of a link's articulated inertia to the parent's origin:  cB = Ba + [r]x Ca,  cA = Aa + Ba [r]x^T + [r]x Ba^T + [r]x Ca [r]x^T;
since cB [r]x^T = Ba [r]x^T + [r]x Ca [r]x^T:  cA_ij = Aa_ij + (r x row_i(Ba))_j + (r x row_j(cB))_i.

float64: the identities.  float32: both forms against the float64 value on the same draws; the earlier form's largest error is printed,
and the block form may have at most twice that (the margin comes from the earlier form, not from the form under test).  Last: the two
new switches of ll_forms.hpp for both builds x 16 flag combinations, against a table written out by hand (a stand-alone C++ program, the
pattern of tests/test_ll_forms.py, whose own columns the new switches leave alone)."""
import os
import subprocess
import tempfile

import numpy as np
import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(REPO, "vid2player3d_amd", "csrc")
N = 4000
F32 = np.float32


def skew(r):
    z = np.zeros(len(r), dtype=r.dtype)
    return np.stack([np.stack([z, -r[:, 2], r[:, 1]], -1), np.stack([r[:, 2], z, -r[:, 0]], -1), np.stack([-r[:, 1], r[:, 0], z], -1)], -2)


def T_(m):
    return np.swapaxes(m, -1, -2)


def spd(rng, n, k, lo, hi):
    """n symmetric positive definite k x k matrices with eigenvalues in lo .. hi (log-uniform)."""
    q = np.linalg.qr(rng.normal(size=(n, k, k)))[0]
    w = np.exp(rng.uniform(np.log(lo), np.log(hi), size=(n, k)))
    m = q @ (w[:, :, None] * T_(q))
    return 0.5 * (m + T_(m))


@pytest.fixture(scope="module")
def draws():
    """Random SPD Lambda_p (6 x 6, the parent's operational-space inverse inertia), SPD Di, general E, r and aug, in float64 - sizes of
    the baked body: inverse inertias 1 .. 1e3, offsets of 0.05 .. 0.5 m, aug 1e-3 .. 1e-1."""
    rng = np.random.default_rng(20261019)
    Lp = spd(rng, N, 6, 1.0, 1e3)
    Di = spd(rng, N, 3, 1.0, 1e3)
    E = rng.normal(0, 0.3, size=(N, 3, 3))
    r = rng.uniform(0.05, 0.5, size=(N, 3)) * rng.choice([-1.0, 1.0], size=(N, 3))
    aug = np.exp(rng.uniform(np.log(1e-3), np.log(1e-1), size=N))
    # pass 2: Aa, Ca symmetric, Ba general
    Aa, Ca, Ba = spd(rng, N, 3, 1e-3, 1.0), spd(rng, N, 3, 0.1, 10.0), rng.normal(0, 0.3, size=(N, 3, 3))
    return dict(La=Lp[:, :3, :3], Lb=Lp[:, :3, 3:], Lc=Lp[:, 3:, 3:], Di=Di, E=E, r=r, aug=aug, Aa=Aa, Ca=Ca, Ba=Ba)


def shifted_G(d):
    """G = X Lp X^T: Ga = La ; Gb = La [r]x + Lb ; Gc = Lc - [r]x Lb + Gb^T [r]x   (float64)"""
    R = skew(d["r"])
    Gb = d["La"] @ R + d["Lb"]
    return d["La"], Gb, d["Lc"] - R @ d["Lb"] + T_(Gb) @ R


def dense(d):
    """[Di 0; 0 0] + T^T G T as 6 x 6 matrices (float64)"""
    Ga, Gb, Gc = shifted_G(d)
    n = len(Ga)
    G = np.concatenate([np.concatenate([Ga, Gb], -1), np.concatenate([T_(Gb), Gc], -1)], -2)
    T = np.zeros((n, 6, 6))
    T[:, :3, :3] = d["aug"][:, None, None] * d["Di"]
    T[:, 3:, :3] = -T_(d["E"])
    T[:, 3:, 3:] = np.eye(3)
    out = T_(T) @ G @ T
    out[:, :3, :3] += d["Di"]
    return out


# ---- float32: every product and sum rounded as the kernel's instructions round them (a fused multiply-add rounds once)
def fma(a, b, c):
    return (a.astype(np.float64) * b.astype(np.float64) + c.astype(np.float64)).astype(F32)


def dot3(a, b):  # a.x b.x + a.y b.y + a.z b.z: a multiply and two FMAs
    return fma(a[..., 2], b[..., 2], fma(a[..., 1], b[..., 1], a[..., 0] * b[..., 0]))


def chain(c, s, a, b, dd, e):  # c + s (a.b) - dd.e: two chains and the FMA that joins them (scaled_dot_minus_dot of csrc/phys_math.hpp)
    t = -(dd[..., 0] * e[..., 0]) if c is None else fma(-dd[..., 0], e[..., 0], c)
    t = fma(-dd[..., 2], e[..., 2], fma(-dd[..., 1], e[..., 1], t))
    return fma(s, dot3(a, b), t)


def row(m, i):
    return m[:, i, :]


def col(m, j):
    return m[:, :, j]


def earlier_form(Ga, Gb, Gc, Di, E, aug):
    H1, H2, t, B, A = (np.zeros_like(Ga) for _ in range(5))
    for i in range(3):
        for j in range(3):
            H1[:, i, j] = aug * dot3(row(Ga, i), col(Di, j)) - dot3(row(Gb, i), row(E, j))
            H2[:, i, j] = aug * dot3(col(Gb, i), col(Di, j)) - dot3(row(Gc, i), row(E, j))
    for i in range(3):
        for j in range(3):
            t[:, i, j] = aug * dot3(row(Di, i), col(H1, j)) - dot3(row(E, i), col(H2, j))
            B[:, i, j] = aug * dot3(row(Di, i), col(Gb, j)) - dot3(row(E, i), row(Gc, j))
    for i in range(3):
        for j in range(3):
            A[:, i, j] = Di[:, i, j] + (t[:, i, j] if i == j else F32(0.5) * (t[:, i, j] + t[:, j, i]))
    return A, B, H1


def block_form(Ga, Gb, Gc, Di, E, aug):
    M1, B, A = (np.zeros_like(Ga) for _ in range(3))
    for i in range(3):
        for j in range(3):
            M1[:, i, j] = chain(None, aug, row(Di, i), col(Ga, j), row(E, i), row(Gb, j))
            B[:, i, j] = chain(None, aug, row(Di, i), col(Gb, j), row(E, i), row(Gc, j))
    for i in range(3):
        for j in range(i, 3):
            A[:, i, j] = A[:, j, i] = chain(Di[:, i, j], aug, row(M1, i), row(Di, j), row(B, i), row(E, j))
    return A, B, T_(M1)


def block_form_scaled_first(Ga, Gb, Gc, Di, E, aug):
    """(not the kernel's: P = aug Di rounded entry by entry first, then chains of six - one instruction less per entry)"""
    P = aug[:, None, None] * Di
    one = np.ones_like(aug)
    return block_form(Ga, Gb, Gc, P, E, one)[1:] + (P,)


def cross_at(c, a, b, k):  # c + (a x b)_k, two FMAs (cross_at_plus of csrc/phys_math.hpp)
    i, j = (k + 1) % 3, (k + 2) % 3
    return fma(a[:, i], b[:, j], fma(-a[:, j], b[:, i], c))


def cross(a, b):
    return np.stack([a[:, (k + 1) % 3] * b[:, (k + 2) % 3] - a[:, (k + 2) % 3] * b[:, (k + 1) % 3] for k in range(3)], -1)


def shift_cB(Ba, Ca, r):
    cB = np.zeros_like(Ba)
    for k in range(3):
        cB[:, :, k] = Ba[:, :, k] + cross(r, col(Ca, k))
    return cB


def earlier_shift(Aa, Ba, Ca, r):
    cB = shift_cB(Ba, Ca, r)
    S = cB - Ba if Ba.dtype == np.float64 else np.stack([cross(r, col(Ca, k)) for k in range(3)], -1)
    t1 = np.stack([cross(r, row(Ba, i)) for i in range(3)], -2)
    t2 = np.stack([cross(r, row(S, i)) for i in range(3)], -2)
    cA = np.zeros_like(Aa)
    for i in range(3):
        for j in range(i, 3):
            cA[:, i, j] = cA[:, j, i] = Aa[:, i, j] + t1[:, i, j] + t1[:, j, i] + t2[:, i, j]
    return cA, cB


def block_shift(Aa, Ba, Ca, r):
    cB = shift_cB(Ba, Ca, r)
    cA = np.zeros_like(Aa)
    for i in range(3):
        for j in range(i, 3):
            if Aa.dtype == np.float64:
                cA[:, i, j] = cA[:, j, i] = Aa[:, i, j] + cross(r, row(Ba, i))[:, j] + cross(r, row(cB, j))[:, i]
            else:
                cA[:, i, j] = cA[:, j, i] = cross_at(cross_at(Aa[:, i, j], r, row(Ba, i), j), r, row(cB, j), i)
    return cA, cB


def relerr(got, want):
    """largest error of a draw's block over the largest entry of that block, the largest over the draws"""
    return float((np.abs(got.astype(np.float64) - want).max(axis=(1, 2)) / np.abs(want).max(axis=(1, 2))).max())


# ---------------------------------------------------------------------------------------------------------------- float64
def test_blocks_equal_the_dense_form_in_float64(draws):
    d = draws
    Ga, Gb, Gc = shifted_G(d)
    want = dense(d)
    P = d["aug"][:, None, None] * d["Di"]
    B = P @ Gb - d["E"] @ Gc
    M1 = P @ Ga - d["E"] @ T_(Gb)
    A = d["Di"] + M1 @ P - B @ T_(d["E"])
    H1 = Ga @ P - Gb @ T_(d["E"])
    scale = np.abs(want).max(axis=(1, 2), keepdims=True)
    assert (np.abs(A - want[:, :3, :3]) / scale).max() < 1e-12
    assert (np.abs(B - want[:, :3, 3:]) / scale).max() < 1e-12
    assert (np.abs(Gc - want[:, 3:, 3:]) / scale).max() < 1e-12
    assert np.abs(H1 - T_(M1)).max() / np.abs(H1).max() < 1e-13, "H1 = M1^T"
    assert (np.abs(want - T_(want)) / scale).max() < 1e-12 and (np.abs(A - T_(A)) / scale).max() < 1e-12, "Lambda_b is symmetric"
    # the earlier form's pieces: H2 = Lam.B^T, t = Lam.A - Di, symmetric
    H2 = T_(Gb) @ P - Gc @ T_(d["E"])
    t = P @ H1 - d["E"] @ H2
    assert np.abs(H2 - T_(B)).max() / np.abs(B).max() < 1e-13 and (np.abs(t - T_(t)) / scale).max() < 1e-12
    assert (np.abs(d["Di"] + t - A) / scale).max() < 1e-12


def test_shift_through_cB_equals_the_three_crosses_in_float64(draws):
    d = draws
    R = skew(d["r"])
    want = d["Aa"] + d["Ba"] @ T_(R) + R @ T_(d["Ba"]) + R @ d["Ca"] @ T_(R)
    a0, b0 = earlier_shift(d["Aa"], d["Ba"], d["Ca"], d["r"])
    a1, b1 = block_shift(d["Aa"], d["Ba"], d["Ca"], d["r"])
    assert np.abs(b0 - (d["Ba"] + R @ d["Ca"])).max() < 1e-13 and np.array_equal(b0, b1)
    assert np.abs(a0 - want).max() < 1e-13 and np.abs(a1 - want).max() < 1e-13 and np.abs(a1 - T_(a1)).max() == 0.0


# ---------------------------------------------------------------------------------------------------------------- float32
def test_blocks_in_float32_stay_within_twice_the_earlier_forms_error(draws):
    d = draws
    want = dense(d)
    Ga, Gb, Gc = (m.astype(F32) for m in shifted_G(d))  # (the parent's blocks, shifted: the same inputs to both forms - what is compared is how the products are formed)
    # the float64 value OF THE ROUNDED INPUTS
    d32 = dict(d, Di=d["Di"].astype(F32), E=d["E"].astype(F32), aug=d["aug"].astype(F32))
    Pd = d32["aug"].astype(np.float64)[:, None, None] * d32["Di"].astype(np.float64)
    Ed = d32["E"].astype(np.float64)
    Bw = Pd @ Gb.astype(np.float64) - Ed @ Gc.astype(np.float64)
    Aw = d32["Di"].astype(np.float64) + (Pd @ Ga.astype(np.float64) - Ed @ T_(Gb.astype(np.float64))) @ Pd - Bw @ T_(Ed)
    H1w = Ga.astype(np.float64) @ Pd - Gb.astype(np.float64) @ T_(Ed)
    assert relerr(Aw.astype(F32), want[:, :3, :3]) < 1e-4  # (the rounded inputs still describe the same draw)
    args = (Ga, Gb, Gc, d32["Di"], d32["E"], d32["aug"])
    for name, k, w in (("Lam.A", 0, Aw), ("Lam.B", 1, Bw), ("H1", 2, H1w)):
        old, new = relerr(earlier_form(*args)[k], w), relerr(block_form(*args)[k], w)
        print("[lambda blocks] %-5s float32 against float64, %d draws: earlier form %.3e, by blocks %.3e (allowed: %.3e)" % (name, N, old, new, 2 * old))
        assert new <= 2 * old, name
    A = block_form(*args)[0]
    assert np.array_equal(A, T_(A))
    Bp, H1p, _ = block_form_scaled_first(*args)
    print("[lambda blocks] with P = aug Di rounded first (not built): Lam.B %.3e, H1 %.3e" % (relerr(Bp, Bw), relerr(H1p, H1w)))


def test_shift_in_float32_stays_within_twice_the_earlier_forms_error(draws):
    d = draws
    a32 = [d[k].astype(F32) for k in ("Aa", "Ba", "Ca", "r")]
    want = block_shift(*[a.astype(np.float64) for a in a32])[0]
    old, new = relerr(earlier_shift(*a32)[0], want), relerr(block_shift(*a32)[0], want)
    print("[lambda blocks] cA    float32 against float64, %d draws: earlier form %.3e, through cB %.3e (allowed: %.3e)" % (N, old, new, 2 * old))
    assert new <= 2 * old


# ---------------------------------------------------------------------------------------------------------------- the switches
# columns: LAMX P2SHIFT; rows: (TGS, DIAG, BALL, LIMITS).  LAMX = true: no instantiation gains scratch or loses a wave per SIMD with it;
# P2SHIFT = !(TGS && BALL): see ll_forms.hpp
TABLE = {
    "lds": {
        (0, 0, 0, 0): "1 1", (0, 0, 0, 1): "1 1", (0, 0, 1, 0): "1 1", (0, 0, 1, 1): "1 1",
        (0, 1, 0, 0): "1 1", (0, 1, 0, 1): "1 1", (0, 1, 1, 0): "1 1", (0, 1, 1, 1): "1 1",
        (1, 0, 0, 0): "1 1", (1, 0, 0, 1): "1 1", (1, 0, 1, 0): "1 0", (1, 0, 1, 1): "1 0",
        (1, 1, 0, 0): "1 1", (1, 1, 0, 1): "1 1", (1, 1, 1, 0): "1 0", (1, 1, 1, 1): "1 0",
    },
    "regs": {
        (0, 0, 0, 0): "1 1", (0, 0, 0, 1): "1 1", (0, 0, 1, 0): "1 1", (0, 0, 1, 1): "1 1",
        (0, 1, 0, 0): "1 1", (0, 1, 0, 1): "1 1", (0, 1, 1, 0): "1 1", (0, 1, 1, 1): "1 1",
        (1, 0, 0, 0): "1 1", (1, 0, 0, 1): "1 1", (1, 0, 1, 0): "1 0", (1, 0, 1, 1): "1 0",
        (1, 1, 0, 0): "1 1", (1, 1, 0, 1): "1 1", (1, 1, 1, 0): "1 0", (1, 1, 1, 1): "1 0",
    },
}

PROG = r'''
#include "ll_forms.hpp"
#include <stdio.h>
using namespace v2p;
template <LlBuild B, bool TGS, bool DIAG, bool BALL, bool LIMITS>
void row(const char* build) {
    typedef LlForms<B, TGS, DIAG, BALL, LIMITS> F;
    printf("%s %d %d %d %d : %d %d\n", build, (int)TGS, (int)DIAG, (int)BALL, (int)LIMITS, (int)F::LAMX, (int)F::P2SHIFT);
}
template <LlBuild B, int I>
void rows(const char* build) {
    if constexpr (I < 16) {
        row<B, (I & 8) != 0, (I & 4) != 0, (I & 2) != 0, (I & 1) != 0>(build);
        rows<B, I + 1>(build);
    }
}
int main() {
    rows<LlBuild::Lds, 0>("lds");
    rows<LlBuild::Regs, 0>("regs");
    return 0;
}
'''


@pytest.mark.parametrize("build", ["lds", "regs"])
def test_new_switches_table(build):
    with tempfile.TemporaryDirectory() as d:
        src = os.path.join(d, "s.cpp")
        open(src, "w").write(PROG)
        path = os.path.join(d, "s")
        subprocess.check_call(["g++", "-std=c++17", "-Wall", "-I", CSRC, src, "-o", path])
        out = subprocess.check_output([path]).decode()
    got = {}
    for line in out.splitlines():
        key, row_ = (part.strip() for part in line.split(":"))
        b, *flags = key.split()
        got[(b, tuple(int(f) for f in flags))] = row_
    assert len(got) == 32
    for flags, want in TABLE[build].items():
        assert got[(build, flags)] == want, (build, flags)
