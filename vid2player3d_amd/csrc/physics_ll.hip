// Articulated rigid-body step, LANE = LINK mapping: 32 lanes per environment (24 links + 8 idle), two
// environments per wave64, every per-link quantity in registers.  Same model and same arithmetic per
// link as physics.hip (see that file and oracle/phys/v2p_phys_oracle.c for the model); what changes is
// the schedule:
//
//   * the three tree recursions run level-synchronously (max depth 8 instead of 23 sequential links);
//     parent -> child and child -> parent transfers are cross-lane pulls (ds_bpermute / DPP lane shifts) inside the wave
//   * contact generation: a box test culls, each link near the ground is scanned by a group of 8 lanes (DPP reductions), the
//     8 groups of a wave take the near links of both environments
//   * the block Gauss-Seidel sweep visits, per environment, only the bodies that environment touches
//     (k-th touched body of both environments at once) and keeps their velocities current by WALKING the tree from one
//     touched link to the next (up to the lowest common ancestor, which answers with its Lambda, and down again); one
//     root -> leaves pass at the end of the sweep moves every link (see the sweep)
//   * envs are handed to waves in descending order of their contact load (the heaviest quarter each next to one of the lightest),
//     a counting sort spread over this kernel's epilogue (bin histogram + arrival lists) and the next launch's prologue (every wave
//     looks its two envs up: slot -> rank -> bin -> arrival list); an env's arithmetic never depends on
//     the env it shares a wave with
//   * one launch = (substep, env pair) JOBS: the heaviest pairs run their four substeps in one workgroup, the others hand the
//     state over from job to job through memory (16-byte write-through stores / loads + a progress word per pair)
//   * pre-physics (PD-target clamp, residual wrench) runs in the prologue of an env's first job, post-physics (observation, reward,
//     reset flags, next target) in the epilogue of its last: v2p_env_step is this one kernel
//   * no global workspace: a job reads the state once, keeps it in registers and writes the state (and, the last job, the
//     caller's row-major tensors: lane = body gives contiguous rows) once; hull vertices and per-link constants come from the
//     (per-env) shape table through L1/L2; LDS holds the contact records of a link (28 floats per lane) and values a phase does not touch
//   * 168 VGPRs, 3 waves per SIMD (needs -fno-slp-vectorize: SLP packing costs ~160 registers here)
//
// The sequential semantics of the Gauss-Seidel sweep (bodies ascending; inside a body the limit rows of its joint, then its points in slot
// order, rows n, t1, t2) are those of the one-env-per-lane kernel and of the float64 oracle, so the results agree with both to rounding.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdlib.h>
#include <string.h>

#include <type_traits>

// This translation unit is compiled with -fassociative-math -freciprocal-math -fno-signed-zeros -fno-trapping-math -fno-honor-nans
// (build.py) and NOT with -ffast-math: reassociation and NaN-free selects for the code of this file, but the device libraries it
// links and the way the HIP headers map sinf / cosf / atan2f stay the precise ones (-ffast-math, or the full set of its component
// flags, turns them into the hardware approximations for the whole file, which no pragma undoes; the helpers that restate the
// reference in the pre-physics prologue must round like task_ops.hip).  The physics model is this engine's own specification and
// is checked against the float64 oracle at fixed tolerances; its transcendental / division shortcuts are written out below
// (hardware sin, cos, sqrt, rcp).  V2P_LL_STRICT_MATH builds everything precise.
// (V2P_LL_PRECISE_SINCOS / _SQRT / _RCP switch one shortcut back at a time: tools/parity_ab.sh bisects a parity difference with them)
#if !defined(V2P_LL_STRICT_MATH)
#if !defined(V2P_LL_PRECISE_SINCOS)
#define PHYS_SINCOS(x, s, c) do { (s) = __sinf(x); (c) = __cosf(x); } while (0)
#endif
#if !defined(V2P_LL_PRECISE_SQRT)
#define PHYS_SQRT(x) __builtin_amdgcn_sqrtf(x)
#endif
#if !defined(V2P_LL_PRECISE_RCP)
#define PHYS_RCP(x) __builtin_amdgcn_rcpf(x)
#endif
#endif
#include "phys_common.hpp"
#include "hull_gjk.hpp"
#include "ll_forms.hpp"

// This file is compiled TWICE into libv2p_rollout.so (build.py): the default object (V2P_LL_WPS* = 3, V2P_LL_PARK2 / 3 = 1: 168 VGPRs,
// three waves per SIMD, contact records and phase-dead values parked in LDS) and, with -DV2P_LL_REGS_BUILD and the knobs set to
// 2 / 2 / 2 / 0 / 0, the register build (256 VGPRs, two waves per SIMD, everything in registers).  Only the kernel and its
// launcher carry a per-build name; every shared type is namespace v2p's own, and what does not depend on the build
// (env_pre_kernel, the pairing table, their launchers) is compiled once in physics_ll_host.hip.
#if defined(V2P_LL_REGS_BUILD)
#define V2P_LL_NS ll_regs
#define V2P_LL_LAUNCHER launch_env_physics_ll_regs
#define V2P_LL_BUILD LlBuild::Regs
#else
#define V2P_LL_NS ll_lds
#define V2P_LL_LAUNCHER launch_env_physics_ll
#define V2P_LL_BUILD LlBuild::Lds
#endif

namespace v2p {

// namespace strict: the pre- / post-physics arithmetic that restates the reference, compiled precise and without contraction; shared
// with the stand-alone env_pre_kernel (physics_ll_host.hip), so the fused step equals the staged step bit for bit (tests)
#include "strict_ops.inc"

typedef volatile __attribute__((address_space(3))) float lds_vfloat;  // a volatile float in LDS (ds_read / ds_write, 32-bit address + immediate offset)
constexpr int LPE = 32;  // lanes per environment

// wave-wide "any lane": a compare of the ballot in scalar registers (HIP's __any materialises the predicate as a 0/1 VGPR first:
// 2 VALU instructions per use, and the sweep loops use it ~20 times per block update)
__device__ __forceinline__ bool any64(bool p) { return __builtin_amdgcn_ballot_w64(p) != 0ull; }
// hand-off of a job's results to another workgroup (possibly on another XCD: per-XCD L2s are not coherent, a CU's L1 is never refreshed):
// system-scope relaxed atomics = `sc0 sc1` loads / stores on both sides (MI355X_MICROARCH.md, inter-workgroup visibility, valid forms)
__device__ __forceinline__ uint8_t flag_ld(const uint8_t* p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM); }
__device__ __forceinline__ void flag_st(uint8_t* p, uint8_t v) { __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM); }
__device__ __forceinline__ float cload(const float* p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM); }
__device__ __forceinline__ void cstore(float* p, float v) { __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM); }
// the same in 16-byte pieces (MI355X_MICROARCH.md: a dword `sc1` store is its own fabric write, ~6x the time per byte of a dwordx4 one;
// __hip_atomic_* stops at 8 bytes).  The compiler does not count these accesses: the loads are drained inside the asm block, the stores
// by the s_waitcnt vmcnt(0) in front of the progress word (memory operations retire in order, so the compiler's own counts only over-wait).
typedef float f4 __attribute__((ext_vector_type(4)));
__device__ __forceinline__ void cstore4(float* p, float x, float y, float z, float w) {
    const f4 v{x, y, z, w};
    // (s_nop 1: gfx940+ needs two wait states between a VMEM store of more than 8 bytes and a VALU write of its data registers; the
    // compiler's hazard recogniser does not look into inline asm and reuses the registers at once - with one wait state short, the
    // hand-offs of a loaded GPU carried the NEXT values of those registers)
    asm volatile("global_store_dwordx4 %0, %1, off sc0 sc1\n\ts_nop 1" ::"v"(p), "v"(v) : "memory");
}
__device__ __forceinline__ void cload4x2(const float* p0, const float* p1, f4& a, f4& b) {
    asm volatile("global_load_dwordx4 %0, %2, off sc0 sc1\n\tglobal_load_dwordx4 %1, %3, off sc0 sc1\n\ts_waitcnt vmcnt(0)" : "=&v"(a), "=&v"(b) : "v"(p0), "v"(p1) : "memory");
}

__device__ __forceinline__ float pull(float v, int src_lane) {
    return __int_as_float(__builtin_amdgcn_ds_bpermute(src_lane << 2, __float_as_int(v)));
}
__device__ __forceinline__ V3 pull(V3 v, int s) { return V3{pull(v.x, s), pull(v.y, s), pull(v.z, s)}; }
__device__ __forceinline__ Q4 pull(Q4 q, int s) { return Q4{pull(q.x, s), pull(q.y, s), pull(q.z, s), pull(q.w, s)}; }
__device__ __forceinline__ Sym3 pull(const Sym3& a, int s) {
    return Sym3{pull(a.xx, s), pull(a.xy, s), pull(a.xz, s), pull(a.yy, s), pull(a.yz, s), pull(a.zz, s)};
}
__device__ __forceinline__ M3 pull(const M3& a, int s) {
    M3 r;
#pragma unroll
    for (int i = 0; i < 9; ++i) r.m[i] = pull(a.m[i], s);
    return r;
}
// lane i <- lane i+1 through the DPP network (wave_shl:1, VALU speed, no LDS round trip): links are in depth-first order, so the
// first child of any link is the next lane.  (The mirror image for parents, wave_shr:1 + a select against the non-chain links,
// measured slower than a plain ds_bpermute and is not used.)
// (bound_ctrl: the lane without a source - lane 63 - gets 0 from the hardware; with bound_ctrl off it KEEPS the `old` operand, which the
// compiler then has to materialise with a v_mov 0 in front of every one of these moves, and which keeps it from folding the move into the
// add that consumes it)
__device__ __forceinline__ float from_next(float v) { return __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(v), 0x130, 0xf, 0xf, true)); }
__device__ __forceinline__ V3 from_next(V3 v) { return V3{from_next(v.x), from_next(v.y), from_next(v.z)}; }
__device__ __forceinline__ Sym3 from_next(const Sym3& a) {
    return Sym3{from_next(a.xx), from_next(a.xy), from_next(a.xz), from_next(a.yy), from_next(a.yz), from_next(a.zz)};
}
__device__ __forceinline__ M3 from_next(const M3& a) {
    M3 r;
#pragma unroll
    for (int i = 0; i < 9; ++i) r.m[i] = from_next(a.m[i]);
    return r;
}
// value held by the parent lane (ds_bpermute).  (`nonchain` = some link of the level being processed does not directly follow its parent;
// a DPP shift on the other levels measured slower: docs/NOTES.md.)  Calls through this struct instead of pull(v, plane) directly: the two
// forms compile to different machine code under -fassociative-math (other rounding), and the parity tests pin this one.
struct ParentPull {
    int plane;
    bool chain;
    __device__ __forceinline__ float operator()(float v, bool nonchain) const {
        return pull(v, plane);
    }
    __device__ __forceinline__ V3 operator()(V3 v, bool nonchain) const {
        return V3{pull(v.x, plane), pull(v.y, plane), pull(v.z, plane)};
    }
    __device__ __forceinline__ Q4 operator()(Q4 q, bool nonchain) const {
        return Q4{pull(q.x, plane), pull(q.y, plane), pull(q.z, plane), pull(q.w, plane)};
    }
    __device__ __forceinline__ Sym3 operator()(const Sym3& a, bool nonchain) const {
        return Sym3{pull(a.xx, plane), pull(a.xy, plane), pull(a.xz, plane), pull(a.yy, plane), pull(a.yz, plane), pull(a.zz, plane)};
    }
    __device__ __forceinline__ M3 operator()(const M3& a, bool nonchain) const {
        M3 r;
#pragma unroll
        for (int i = 0; i < 9; ++i) r.m[i] = pull(a.m[i], plane);
        return r;
    }
};
__device__ __forceinline__ Sym3 operator+(const Sym3& a, const Sym3& b) {
    return Sym3{a.xx + b.xx, a.xy + b.xy, a.xz + b.xz, a.yy + b.yy, a.yz + b.yz, a.zz + b.zz};
}
__device__ __forceinline__ Sym3 mask(bool c, const Sym3& a) {
    return Sym3{c ? a.xx : 0.f, c ? a.xy : 0.f, c ? a.xz : 0.f, c ? a.yy : 0.f, c ? a.yz : 0.f, c ? a.zz : 0.f};
}
__device__ __forceinline__ V3 mask(bool c, V3 a) { return V3{c ? a.x : 0.f, c ? a.y : 0.f, c ? a.z : 0.f}; }

// 8-lane group exchanges on the DPP network: lane ^ 1, lane ^ 2 (quad permutes) and lane -> 7 - lane (row_half_mirror)
__device__ __forceinline__ unsigned grp_xor1(unsigned v) { return (unsigned)__builtin_amdgcn_update_dpp(0, (int)v, 0xB1, 0xf, 0xf, false); }
__device__ __forceinline__ unsigned grp_xor2(unsigned v) { return (unsigned)__builtin_amdgcn_update_dpp(0, (int)v, 0x4E, 0xf, 0xf, false); }
__device__ __forceinline__ unsigned grp_mirror(unsigned v) { return (unsigned)__builtin_amdgcn_update_dpp(0, (int)v, 0x141, 0xf, 0xf, false); }
// (value, index) reductions over a group; index -1 = empty; ties go to the lower index so the result is what a serial scan finds
template <bool MAX, typename F>
__device__ __forceinline__ void grp_arg_step(float& v, int& k, F xch) {
    const float ov = __uint_as_float(xch(__float_as_uint(v)));
    const int ok = (int)xch((unsigned)k);
    const bool beats = MAX ? ov > v : ov < v;
    const bool take = ok >= 0 && (k < 0 || beats || (ov == v && ok < k));
    v = take ? ov : v;
    k = take ? ok : k;
}
__device__ __forceinline__ void grp_argmin(float& v, int& k) {
    grp_arg_step<false>(v, k, grp_xor1); grp_arg_step<false>(v, k, grp_xor2); grp_arg_step<false>(v, k, grp_mirror);
}
__device__ __forceinline__ void grp_argmax(float& v, int& k) {
    grp_arg_step<true>(v, k, grp_xor1); grp_arg_step<true>(v, k, grp_xor2); grp_arg_step<true>(v, k, grp_mirror);
}
// ... in two reductions of ONE value each instead of a (value, index) pair under a three-way comparison: the extreme itself
// (v_min / v_max on the DPP network), then the lowest index among the lanes that hold it.  The same winner: a lane's own index is the
// first of its slots that attains the lane's extreme, and an empty lane (index -1) takes no part.  A third of the instructions of
// grp_argmin / grp_argmax; it needs two registers more while it runs, which the racket + ball and joint-limit instantiations do not
// have (their scratch grew by 8 - 20 B per lane with it; in the register build the TGS kernels' too), so those keep the pairwise
// form (FAST = false).
__device__ __forceinline__ float grp_fmin(float v) {
    v = fminf(v, __uint_as_float(grp_xor1(__float_as_uint(v)))); v = fminf(v, __uint_as_float(grp_xor2(__float_as_uint(v)))); v = fminf(v, __uint_as_float(grp_mirror(__float_as_uint(v))));
    return v;
}
__device__ __forceinline__ float grp_fmax(float v) {
    v = fmaxf(v, __uint_as_float(grp_xor1(__float_as_uint(v)))); v = fmaxf(v, __uint_as_float(grp_xor2(__float_as_uint(v)))); v = fmaxf(v, __uint_as_float(grp_mirror(__float_as_uint(v))));
    return v;
}
__device__ __forceinline__ unsigned grp_umin(unsigned v) {
    unsigned o = grp_xor1(v); v = o < v ? o : v; o = grp_xor2(v); v = o < v ? o : v; o = grp_mirror(v); v = o < v ? o : v;
    return v;
}
template <bool MAX, bool FAST>
__device__ __forceinline__ void grp_arg(float& v, int& k) {
    if (!FAST) {
        if (MAX) grp_argmax(v, k); else grp_argmin(v, k);
        return;
    }
    const float m = k < 0 ? (MAX ? -3.0e38f : 3.0e38f) : v;
    const float g = MAX ? grp_fmax(m) : grp_fmin(m);
    const unsigned c = grp_umin((k >= 0 && m == g) ? (unsigned)k : 0x7fffffffu);
    k = c == 0x7fffffffu ? -1 : (int)c;
    v = g;
}

// maximum of a non-negative per-lane value over each env's 32 lanes, on the DPP network: four shifts inside the rows of 16 (a lane
// without a source takes 0), then the last lane of rows 0 and 2 handed to the row behind.  Lane 31 of the result holds the first
// env's maximum, lane 63 the second's.  All lanes have to be on.
__device__ __forceinline__ int half_max_last(int v) {
    int o = __builtin_amdgcn_update_dpp(0, v, 0x111, 0xf, 0xf, true); v = o > v ? o : v;
    o = __builtin_amdgcn_update_dpp(0, v, 0x112, 0xf, 0xf, true); v = o > v ? o : v;
    o = __builtin_amdgcn_update_dpp(0, v, 0x114, 0xf, 0xf, true); v = o > v ? o : v;
    o = __builtin_amdgcn_update_dpp(0, v, 0x118, 0xf, 0xf, true); v = o > v ? o : v;
    o = __builtin_amdgcn_update_dpp(0, v, 0x142, 0xa, 0xf, false); v = o > v ? o : v;
    return v;
}

// The probes of the diagnostic instantiation (counters: enum Prof, phys_common.hpp).  They read the kernel's `a`, `lane` and `F` (the
// form policy, ll_forms.hpp) where they stand.
// which lane of the launch samples: lane 0 of every 64th workgroup, or (V2P_PHASE_HEAVY) of the first 8 - the heaviest env pairs
#define LLSAMPLED (((a.prof_heavy ? blockIdx.x < 8u : (blockIdx.x & 63) == 0)) && lane == 0)
// add v to counter k.  LLADD: the caller has tested DIAG && a.prof; LLCOUNT tests them itself.  (Plain `if` statements, to be used as
// statements of their own, not do { } while (0) blocks: the wrapper's empty blocks, in kernels where the probe compiles to nothing,
// moved the block numbers of the rows' dispatch in the register build's kernels and their code with them: docs/NOTES.md L)
#define LLADD(k, v) if (LLSAMPLED) atomicAdd((unsigned long long*)&a.prof[k], (unsigned long long)(v))
#define LLCOUNT(k, v) if (DIAG && a.prof && LLSAMPLED) atomicAdd((unsigned long long*)&a.prof[k], (unsigned long long)(v))
// the cycles since the stamp tv into counter k, and tv moves on
#define LLSUBV(k, tv) do { if (DIAG && a.prof) { long long t_ = clock64(); LLADD(k, t_ - tv); tv = t_; } } while (0)
#define LLSUB(k) LLSUBV(k, tsub)
// the split of the sweep's remainder (F::DIAGX): timed where the policy says so, else nothing
#define LLSUBX(k, tv) do { if constexpr (F::DIAGX) LLSUBV(k, tv); } while (0)
#define LLSUBX_OR(k, kparent) LLSUB(F::DIAGX ? (k) : (kparent))  // (where the parent timed the same stretch into another counter: as the parent)
#define LLPH(k) LLSUBV(k, tprev)

// Everything from here to the end of the kernel depends on the build (register budget, what is parked in LDS and with it the LDS
// layout): it lives in a namespace of its own per build, which also keeps the two objects' kernels (and their host stubs) apart for
// the linker and in a kernel trace.  Inline: the launcher below names them unqualified.
inline namespace V2P_LL_NS {
// (V2P_LL_WPB, waves per workgroup, is defined in v2p_internal.hpp: the host sizes the progress words with it)
#ifndef V2P_LL_WPS
#define V2P_LL_WPS 3   // waves per SIMD the register budget is set for (168 VGPRs; 2 = 256 VGPRs with everything in registers)
#endif
#ifndef V2P_LL_WPS_BALL
#define V2P_LL_WPS_BALL 3     // ... of the racket + ball instantiations
#endif
#ifndef V2P_LL_WPS_LIMITS
#define V2P_LL_WPS_LIMITS 3   // ... of the joint-limit instantiations without a ball
#endif
constexpr int LL_WPB = V2P_LL_WPB;
constexpr LlBuild LL_BUILD = V2P_LL_BUILD;  // which of the two objects this is: the one place the macro is read for the form policy (ll_forms.hpp)
// V2P_LL_PARK2: phase-scoped parking of values that a phase does not touch (link velocities during pass 2 / contact generation / the
// Lambda recursion, Lambda of the root during contact generation, the contact records during the Lambda recursion): lowers the
// register peak of those phases so that nothing long-lived is spilled ACROSS the sweep loops when the kernel is built for 3 waves/SIMD.
#ifndef V2P_LL_PARK2
#define V2P_LL_PARK2 1
#endif
constexpr bool PARK2 = V2P_LL_PARK2 != 0;
// V2P_LL_PARK3: the contact records of a link (4 x offset, bias / gap, 3 impulses = 28 floats) live in the lane's LDS column instead of
// registers: they are touched once per block update (by the one lane being solved), not inside the per-level loops, and leave their
// 28 registers to the values those loops use.
#ifndef V2P_LL_PARK3
#define V2P_LL_PARK3 1
#endif
constexpr bool PARK3 = V2P_LL_PARK3 != 0;
#ifndef V2P_LL_WAIT_SLEEP
#define V2P_LL_WAIT_SLEEP 16  // s_sleep argument (x 64 clocks) between two polls of a job that waits for its predecessor's hand-over
#endif
constexpr int PARK_TAR = 0, PARK_W0 = 3, PARK_XD0 = 6, PARK_Q = 9, PARK_X = 13, PARK_CR = 16, PARK_CB = 28, PARK_CL = 32,
              PARK_SCR = PARK3 ? 44 : 16,  // (one row of 64 dwords per wave: lane of the k-th near link)
              PARK_SLOTS = PARK_SCR + 1;  // LDS parking slots (dwords per lane)
constexpr int ROOTLAM_FLOATS = 2 * 24;  // (PARK2) Lambda of the two root links while the contacts are generated
// ball block (80 floats per env, after the parking area of the wave): state 13 | aero force 3 | ground contact: active gap bias lambda3 |
// point j at BL_RK + 16 j: active gap bias rl3 n3 lambda3 link (j = 0, 1: against the racket's cylinders; j = 2 .. 4: against the hulls
// of up to three links, RK_LINK = the link that owns the point) | velocity at the start of the substep 3
// (TGS: GGAP / RK_GAP advance slice by slice; BL_GREST / RK_REST = the restitution target of the row, rest x approach speed of v*, taken once
// at the start of the substep, a large value when the row does not bounce: it caps the bias of every slice)
constexpr int BL_POS = 0, BL_QUAT = 3, BL_VEL = 7, BL_ANG = 10, BL_F = 13, BL_GA = 16, BL_GGAP = 17, BL_GBIAS = 18, BL_GLAM = 19, BL_GREST = 22, BL_RK = 24,
              RK_A = 0, RK_GAP = 1, RK_BIAS = 2, RK_RL = 3, RK_N = 6, RK_LAM = 9, RK_LINK = 12, RK_REST = 13, NBREC = 5, BL_V0 = BL_RK + 16 * NBREC, BL_SLOTS = BL_V0 + 8;
// The LDS block of a wave (`wave_lds` in the kernel), in floats - the one statement of its layout:
//   LDS_PARK     [PARK_SLOTS][64]   the parking slots: slot k of lane l at k * 64 + l (PARK_* above).  The last slot, PARK_SCR, is the
//                                   wave's scratch row (lane of the k-th near link during contact generation, the visit words of the
//                                   sweep's set-up).  In the PARK_TAR slots the columns of an env's lanes WRENCH_FORCE_LANE and
//                                   WRENCH_TORQUE_LANE hold the residual wrench of the fused step (neither lane has a joint target).
//   LDS_BALL     [2][BL_SLOTS]      the ball block of each env (BL_* above)
//   LDS_ROOTLAM  [2][ROOTLAM_ROW]   (PARK2) Lambda of each env's root while the contacts are generated
// and, once the substeps are over and the parking slots are idle, two overlays on LDS_PARK:
//   LDS_STAGE    [2][STAGE_FLOATS]  the rigid-body rows [24][13] of each env on their way to the caller's tensor
//   slots 0 .. REWARD_SLOTS - 1     the reward terms of the fused post-physics, a slot per term (the rows have left by then)
constexpr int ROOTLAM_ROW = ROOTLAM_FLOATS / 2, STAGE_FLOATS = NB * 13, REWARD_SLOTS = 4;
constexpr int WRENCH_FORCE_LANE = 0, WRENCH_TORQUE_LANE = 25;  // (lanes of the env)
constexpr int LDS_PARK = 0, LDS_STAGE = LDS_PARK, LDS_BALL = LDS_PARK + PARK_SLOTS * 64, LDS_ROOTLAM = LDS_BALL + 2 * BL_SLOTS;
constexpr int LDS_FLOATS_PER_WAVE = LDS_ROOTLAM + ROOTLAM_FLOATS;
static_assert(LDS_STAGE + 2 * STAGE_FLOATS <= LDS_BALL && REWARD_SLOTS <= PARK_SLOTS, "an overlay does not fit the parking slots");
// (F::CGEN_EARLY: the contact records are written in front of passes 2 and 3 and read behind them; what those passes park - velocities,
// pose, the PD target - lies below the records and the scratch row)
static_assert(PARK_TAR + 3 <= PARK_W0 && PARK_W0 + 3 <= PARK_XD0 && PARK_XD0 + 3 <= PARK_Q && PARK_Q + 4 <= PARK_X && PARK_X + 3 <= PARK_CR && PARK_X + 3 <= PARK_SCR &&
                  (!PARK3 || (PARK_CR + 12 <= PARK_CB && PARK_CB + 4 <= PARK_CL && PARK_CL + 12 <= PARK_SCR)),
              "a pass's parking slots overlap the contact records or the scratch row");
static_assert(WRENCH_TORQUE_LANE > NB && WRENCH_TORQUE_LANE < LPE, "the torque's lane must be one without a link (and not the ball's)");
// the residual wrench's home: envcol = wave_lds + the env's first lane, l = WRENCH_FORCE_LANE / WRENCH_TORQUE_LANE
__device__ __forceinline__ void wrench_put(float* envcol, int l, float x, float y, float z) {
    envcol[l + PARK_TAR * 64] = x; envcol[l + (PARK_TAR + 1) * 64] = y; envcol[l + (PARK_TAR + 2) * 64] = z;
}
__device__ __forceinline__ float wrench_at(const float* envcol, int l, int k) { return envcol[l + (PARK_TAR + k) * 64]; }  // component k
__device__ __forceinline__ V3 wrench_get(const float* envcol, int l) { return V3{wrench_at(envcol, l, 0), wrench_at(envcol, l, 1), wrench_at(envcol, l, 2)}; }
// ball x hull narrow phase, out of line: it runs on the few substeps in which a ball is within reach of a link, and inlined its
// registers would be spilled around on every substep
// (the closest point comes back BY VALUE, xyz = point, w = distance: an out-parameter by reference is a stack slot of the caller that the
// callee writes through a pointer)
__device__ __noinline__ f4 ball_hull_distance(ConstShape* S, int v0, int nv, V3 c) {
    V3 p;
    const float d = hull_closest([&](int k) { return V3{S->hull_verts[v0 + k][0], S->hull_verts[v0 + k][1], S->hull_verts[v0 + k][2]}; }, nv, c, p);
    return f4{p.x, p.y, p.z, d};
}
// contact records of this lane's link: registers, or (PARK3) the lane's LDS column
template <bool LDS>
struct ContactStore;
template <>
struct ContactStore<false> {
    V3 r_[4];
    float b_[4];
    V3 l_[4];
    __device__ __forceinline__ explicit ContactStore(float*) {}
    __device__ __forceinline__ V3 cr(int c) const { return r_[c]; }
    __device__ __forceinline__ void set_cr(int c, V3 v) { r_[c] = v; }
    __device__ __forceinline__ float bias(int c) const { return b_[c]; }
    __device__ __forceinline__ void set_bias(int c, float v) { b_[c] = v; }
    __device__ __forceinline__ V3 lam(int c) const { return l_[c]; }
    __device__ __forceinline__ void set_lam(int c, V3 v) { l_[c] = v; }
};
template <>
struct ContactStore<true> {
    float* p;  // slot 0 of this lane's column
    __device__ __forceinline__ explicit ContactStore(float* park) : p(park) {}
    __device__ __forceinline__ V3 cr(int c) const { return V3{p[(PARK_CR + 3 * c) * 64], p[(PARK_CR + 3 * c + 1) * 64], p[(PARK_CR + 3 * c + 2) * 64]}; }
    __device__ __forceinline__ void set_cr(int c, V3 v) { p[(PARK_CR + 3 * c) * 64] = v.x; p[(PARK_CR + 3 * c + 1) * 64] = v.y; p[(PARK_CR + 3 * c + 2) * 64] = v.z; }
    __device__ __forceinline__ float bias(int c) const { return p[(PARK_CB + c) * 64]; }
    __device__ __forceinline__ void set_bias(int c, float v) { p[(PARK_CB + c) * 64] = v; }
    __device__ __forceinline__ V3 lam(int c) const { return V3{p[(PARK_CL + 3 * c) * 64], p[(PARK_CL + 3 * c + 1) * 64], p[(PARK_CL + 3 * c + 2) * 64]}; }
    __device__ __forceinline__ void set_lam(int c, V3 v) { p[(PARK_CL + 3 * c) * 64] = v.x; p[(PARK_CL + 3 * c + 1) * 64] = v.y; p[(PARK_CL + 3 * c + 2) * 64] = v.z; }
};

// friction frame of a hull x ground point from the link's v* (w0, xd0) and the point's offset rr: t1 along the tangential velocity of the
// point, t2 = z x t1; below 1e-6 m/s the world frame (oracle: v2p_oparams.friction_frame = 1)
__device__ __forceinline__ void vfric_frame(const V3& w0, const V3& xd0, const V3& rr, V3& t1, V3& t2) {
    const float vx = xd0.x + w0.y * rr.z - w0.z * rr.y, vy = xd0.y + w0.z * rr.x - w0.x * rr.z;
    const float s2 = vx * vx + vy * vy;
    const bool on = s2 > 1e-12f;
    const float inv = on ? rsqrtf(s2) : 0.f;
    t1 = on ? V3{vx * inv, vy * inv, 0.f} : V3{1.f, 0.f, 0.f};
    t2 = V3{-t1.y, t1.x, 0.f};
}
// TGS: temporal Gauss-Seidel with frozen Jacobians (v2p_sim_cfg.solver_type 1; the model is stated in oracle/phys/v2p_phys_oracle.c):
// cbias[] then holds the GAP of each point, advanced after every sweep, and the row bias is evaluated where it is used.
// DIAG: the per-phase cycle counters (V2P_PHASE_TIMING) and per-wave timeline stamps (V2P_WAVE_TIMES) are compiled into a separate
// instantiation: in the production kernel they cost registers (spills) and ~2 scalar instructions per probe inside the sweep loops.
// BALL: racket + ball: the first idle lane of an env (lb == 24) simulates the free ball, its state and the ball contact
// records live in a 64-float LDS block per env; the ball-racket rows are solved inside the block update of the racket's link.
// JOBS: one launch = substeps x waves JOBS.  Job (s, p) runs substep s of wave p's env pair and hands the state over to job (s+1, p)
// through global memory (system-scope stores / loads + a progress word per pair).  With whole control steps as jobs, 8192 envs are
// 4096 indivisible jobs of 0.14-0.65 ms on 2048-3072 wave slots and the launch is as long as its worst slot (82 % utilisation,
// profiles/r02*_wave_times.txt); quarter-size jobs pack 4x finer.  Jobs are numbered (and, as observed, dispatched) substep-major,
// heavy pairs first, so a job normally waits for one that started before it; a job whose predecessor does not show up within the
// time-out RECOMPUTES the pair's earlier substeps itself (see the wait), so neither progress nor results depend on the dispatch order.
// (Numbering the jobs by tickets drawn from an atomic counter as the workgroups start - progress by construction - measured -13 %:
// 13 k atomics on one address per launch.)
// LIMITS: joint-limit rows (v2p_sim_cfg.joint_limits; the model is stated in oracle/phys/v2p_phys_oracle.c).  A DOF whose range is
// narrower than a full turn carries one row against its nearer limit; the rows of joint b form their own block update right before
// the contact block of link b.  A limit impulse is a joint-space impulse: it enters the propagation as the link's `un`, and its
// reaction (-impulse, a pure torque) joins what the link hands up to its parent.  The inverse mass of the rows is the joint-space
// inverse inertia K = Di + ((T - 1)^T G (T - 1))_ww = Lambda_b,ww - H1 - H1^T + Lambda_parent,ww in the notation of the recursion below.
// VFRIC: v2p_sim_cfg.friction_frame = velocity (ABI 14; the model is stated in oracle/phys/v2p_phys_oracle.c).  The tangent rows of a hull x
// ground point lie along / across the tangential velocity the point has under v* (the link's velocity at the start of the sweep, which
// stays parked in the PARK_W0 / PARK_XD0 slots of the lane's LDS column for the whole sweep) instead of along world x / y: the frame is
// re-derived from those six floats at every visit of the link (one rsqrt per point) - eight more floats per lane of LDS to keep it would
// cost the third wave per SIMD.  An instantiation of its own: with general tangent directions the rows lose the zeros the world frame
// gives them (~+40 % instructions in the friction rows), which the default kernel must not pay.
template <bool CONTACT, bool MULTI, bool TGS, bool DIAG, bool BALL, bool JOBS, bool LIMITS, bool VFRIC = false>
__global__ __launch_bounds__(64 * LL_WPB, (LlForms<LL_BUILD, TGS, DIAG, BALL, LIMITS>::waves_per_simd(V2P_LL_WPS, V2P_LL_WPS_BALL, V2P_LL_WPS_LIMITS))) void physics_ll_kernel(PhysArgs a) {
    using F = LlForms<LL_BUILD, TGS, DIAG, BALL, LIMITS>;  // which form of each switched phase this instantiation runs (ll_forms.hpp)
    const int64_t N = a.n;
    const int lane = threadIdx.x & 63;
    const int half = lane >> 5;
    const int lb = lane & (LPE - 1);
    const bool valid = lb < NB;
    const int b = valid ? lb : 0;  // idle lanes shadow link 0 and never commit anything
    const int base = lane & LPE;
    // JOBS: the first job_mono workgroups run ALL substeps of the job_mono heaviest env pairs (their chain of substeps is the critical
    // path of the launch: it starts at once and never waits); the other pairs are cut into one job per substep, substep-major
    const int nblk = JOBS ? a.job_blocks : (int)gridDim.x;                 // env pairs (wave slots) of the launch
    const int jid = (int)blockIdx.x;  // jobs are numbered substep-major, heavy pairs first
    const bool mono = !JOBS || jid < a.job_mono;
    const int jcut = JOBS && nblk > a.job_mono ? nblk - a.job_mono : 1;     // pairs that are cut into substep jobs
    const int jrel = JOBS ? jid - a.job_mono : 0;
    const int sjob = mono ? 0 : jrel / jcut;                               // the substep this job runs
    // Order of the cut pairs within a substep.  Wave slots 0 .. pl_mix - 1 hold a heavy env next to a light one, the slots behind them
    // pairs of equals in descending rank - and the first of THOSE (two mid-heavy envs: the union of two contact structures) cost as much
    // as the heavy x light slots in front of them, yet were dispatched behind all of them: they ended every launch (job timeline:
    // the last 15 % of a launch ran at half occupancy).  The two lists are dispatched alternately, so both kinds of long job start early
    // and the tail of a substep is made of short ones.  (Only the order of dispatch changes: results are bit-identical.)
    int jpair = jrel % jcut;
    if (JOBS && !mono && a.job_interleave) {
        const int nmix = a.pl_mix > a.job_mono ? (a.pl_mix < nblk ? a.pl_mix : nblk) - a.job_mono : 0;  // cut slots that are heavy x light
        const int neq = jcut - nmix, both = 2 * (nmix < neq ? nmix : neq);
        if (jpair < both) jpair = (jpair & 1) ? nmix + (jpair >> 1) : (jpair >> 1);
        else jpair = nmix < neq ? jpair : jpair - neq;   // the rest of the longer list (neq >= nmix: positions keep their index)
    }
    const int bid = mono ? jid : a.job_mono + jpair;
    const int64_t slot = ((int64_t)bid * LL_WPB + (threadIdx.x >> 6)) * 2 + half;
    const bool live_env = slot < N;
    const int jlen = JOBS ? a.job_len : 1;  // substeps per job (v2p_env: job_len; 1 = one job per substep)
    // first substep of job j of a cut pair: the FIRST job may be longer than the others (job_lead substeps: one hand-over less per pair,
    // while the jobs that end a launch keep the fine granularity)
    const int jlead = JOBS ? a.job_lead : 1;
    auto jstart = [&](int j) -> int { return j <= 0 ? 0 : jlead + (j - 1) * jlen; };
    const bool first_job = mono || sjob == 0, last_job = mono || jstart(sjob + 1) >= a.p.nsub;
    // the inputs of this job were written by another workgroup of this launch - unless that one did not show up in time (below)
    bool handed = !mono && sjob > 0;
    int* const progress = JOBS ? a.job_progress + (bid * LL_WPB + (threadIdx.x >> 6)) : nullptr;
    // A job of a cut pair that starts after the pair's step is COMPLETE - its successors gave up waiting, replayed its substeps and the
    // last of them has written the results - must not run: the inputs of the step (state, actions, reset flags) are already those of the
    // next one.  The job of an env's last substep leaves the word at launch x (nsub + 1) + nsub when it ends; every other job looks before
    // it touches anything.  (Forward progress never needs this; it keeps a pathologically late job from writing the exposed PD targets,
    // per-call ball records or hand-overs from the wrong inputs.)
    if constexpr (JOBS) if (!mono) {
        int done = 0;
        if (lane == 0) done = __hip_atomic_load(progress, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM) >= a.job_epoch * (a.p.nsub + 1) + a.p.nsub;
        if (__builtin_amdgcn_readfirstlane(done)) {
            // (counted: what this job owns besides its substeps - the exposed PD targets, the in-place action masking, the ball's per-call
            // records - was published by nobody for that step; v2p_env_check reports it as an error, not as lost time)
            if (lane == 0 && half == 0) __hip_atomic_fetch_add(a.job_progress + a.job_blocks * LL_WPB + 1, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
            return;
        }
    }
    // (a lambda called once: written out in place, the same code compiles to other machine code - see ParentPull)
    auto wait_for_predecessor = [&]() {
    if constexpr (JOBS) if (handed) {
        // wait for the previous substep of this env pair
        // progress word of a pair = launch number x (nsub + 1) + substeps handed over: the last hand-over of launch E stores
        // E (nsub + 1) + nsub - 1, below every value a job of launch E + 1 waits for, whatever nsub is (vid2player's controller
        // configs run substeps 6 x controlFrequencyInv 2 = 12 per control step)
        const int want = a.job_epoch * (a.p.nsub + 1) + sjob;
        int ok = 1;
        if (lane == 0) {
            long spins = 0;
            while (__hip_atomic_load(progress, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM) < want) {
                if (spins >= a.job_timeout_spins) {
                    // The predecessor is late beyond reason (jobs are dispatched in index order as far as observed, but nothing promises
                    // it).  This job then runs the pair's EARLIER substeps itself, from the inputs of the step, before its own: every job
                    // of a pair computes the same bits whoever runs it, the hand-over slots are per substep, and the replayed substeps
                    // publish nothing - so the late predecessor, when it does run, rewrites identical values and nothing else changes.
                    // Progress and results are independent of the dispatch order; only time is lost (counted: v2p_env_job_recoveries).
                    ok = 0;
                    __hip_atomic_fetch_add(a.job_progress + a.job_blocks * LL_WPB, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
                    break;
                }
                __builtin_amdgcn_s_sleep(V2P_LL_WAIT_SLEEP);
                ++spins;
            }
        }
        handed = __builtin_amdgcn_readfirstlane(ok) != 0;
        __builtin_amdgcn_wave_barrier();
    }
    };
    wait_for_predecessor();
    int64_t e = live_env ? slot : N - 1;
    if (a.pl_start && handed) {
        // (looked up by the job of the pair's first substep, which has handed it over with everything else)
        e = __hip_atomic_load(&a.pl_slot_env[live_env ? slot : N - 1], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
    } else if (a.pl_start) {
        // ---- which env this wave slot simulates: slot -> rank by contact load (the heaviest `mix` envs sit in the even slots 0, 2, ...,
        // each next to one of the lightest in the odd slot; the rest follows by rank) -> load bin (the last of the 256 bins that starts at
        // or before the rank: one 16-byte load per lane + four ballots) -> the env that arrived in that bin as number (rank - start).
        // The tables are what the previous launch left (physics epilogue); looked up here, no kernel has to scatter them in between.
        const int nn = (int)N, mixn = a.pl_mix;
        const int64_t sl0 = ((int64_t)bid * LL_WPB + (threadIdx.x >> 6)) * 2;
        const int s0 = (int)(sl0 < N ? sl0 : N - 1), s1 = (int)(sl0 + 1 < N ? sl0 + 1 : N - 1);
        const int r0 = s0 < 2 * mixn ? ((s0 & 1) ? nn - 1 - (s0 >> 1) : (s0 >> 1)) : s0 - mixn;
        const int r1 = s1 < 2 * mixn ? ((s1 & 1) ? nn - 1 - (s1 >> 1) : (s1 >> 1)) : s1 - mixn;
        const int4 st = ((const int4*)a.pl_start)[lane];
        const int c0 = __popcll(__ballot(st.x <= r0)) + __popcll(__ballot(st.y <= r0)) + __popcll(__ballot(st.z <= r0)) + __popcll(__ballot(st.w <= r0));
        const int c1 = __popcll(__ballot(st.x <= r1)) + __popcll(__ballot(st.y <= r1)) + __popcll(__ballot(st.z <= r1)) + __popcll(__ballot(st.w <= r1));
        const int bin = half ? c1 - 1 : c0 - 1, rk = half ? r1 : r0;
        e = a.pl_list[(int64_t)bin * N + (rk - a.pl_start[bin])];
        if (JOBS && !mono && lb == 0 && live_env) __hip_atomic_store(&a.pl_slot_env[slot], (int32_t)e, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
    }
    // the env index behind an opaque move: addresses formed from it inside the substep loop are computed where they are used instead of
    // being hoisted in front of the loop and kept (spilled: 64-bit pointers, 8 bytes of scratch per lane each) across all of it
    auto env_here = [&]() -> int64_t { int64_t v = e; asm volatile("" : "+v"(v)); return v; };
    ConstModel& M = *(ConstModel*)a.model;
    // numeric data of this env's body shape: the model's own shape, or (MULTI) one of the batch's shapes, per env
    const int sid = MULTI ? a.env_shape[e] : 0;
    ConstShape* S = MULTI ? (ConstShape*)(a.shapes + sid) : &M.shape;
    float* __restrict__ st = a.state;
    const EnvParams& P = a.p;
    const float h_launch = P.h;
    const int maxd = M.max_depth;
    const int multi = M.multi_child_levels;
    const int nonchain = M.nonchain_levels;

    // hull vertex `idx` of this env's shape, from the shape table through L1/L2.  (An LDS copy per workgroup measured 3.5 % slower
    // at 8192 envs: 4096 workgroups x 19 KB of staging traffic and a barrier before the first substep.)
    auto hullv = [&](int idx) -> float4 { return make_float4(S->hull_verts[idx][0], S->hull_verts[idx][1], S->hull_verts[idx][2], 0.f); };

    // ---- LDS "parking": per-lane values that live for the whole launch but are touched once or twice per substep (the PD target,
    // the velocities at the start of the sweep).  Holding them in registers made the allocator spill them (or something else) to
    // scratch - private memory that ends up as HBM write traffic; 9 dwords x 64 lanes of LDS per wave cost nothing.
    extern __shared__ float park_all[];
    float* const wave_lds = park_all + (threadIdx.x >> 6) * LDS_FLOATS_PER_WAVE;  // this wave's block (the map: LDS_FLOATS_PER_WAVE)
    float* const park = wave_lds + LDS_PARK + lane;  // slot k of this lane: park[k * 64]
    // this env's ball block.  The pointer carries the LDS address space in its TYPE: the accesses are volatile (the ball lane writes what
    // link lanes read within the wave), and address-space inference leaves volatile accesses alone - as a plain `volatile float*` every
    // bl[k] was a FLAT load / store through its own 64-bit address, ~50 loop-invariant pointers that were kept (spilled: 400 B of
    // scratch per lane) across the substep loop
    lds_vfloat* const bl = (lds_vfloat*)(wave_lds + LDS_BALL + half * BL_SLOTS);
    auto park_put3 = [&](int slot, V3 v) { park[slot * 64] = v.x; park[(slot + 1) * 64] = v.y; park[(slot + 2) * 64] = v.z; };
    auto park_get3 = [&](int slot) -> V3 { return V3{park[slot * 64], park[(slot + 1) * 64], park[(slot + 2) * 64]}; };
    // (PARK2) the link velocities leave the registers for the phases that do not touch them; the W0 / XD0 slots are free outside the sweep
    auto park_vel = [&](const V3& w_, const V3& xd_) { if (PARK2) { park_put3(PARK_W0, w_); park_put3(PARK_XD0, xd_); } };
    auto unpark_vel = [&](V3& w_, V3& xd_) { if (PARK2) { w_ = park_get3(PARK_W0); xd_ = park_get3(PARK_XD0); } };

    // ---- per-lane model constants
    const int par = b ? M.parents[b] : 0;
    const int plane = base + par;
    const ParentPull pp{plane, par == b - 1};
    const bool firstchild = par == b - 1;  // depth-first order: the first child directly follows its parent
    const int dep = valid ? M.depth[b] : 99;
    const int c0 = M.children[b][0], c1 = M.children[b][1], c2 = M.children[b][2];
    const bool has0 = valid && c0 >= 0, has1 = valid && c1 >= 0, has2 = valid && c2 >= 0;
    const int cl1 = has1 ? base + c1 : lane, cl2 = has2 ? base + c2 : lane;
    const float aug = MULTI ? a.shape_aug[sid * NB + b] : P.aug[b];
    const int desc = M.desc_mask[b];  // links of the subtree rooted here (self included)
    const int aj = valid ? M.anc_jump[b] : -1;  // the ancestors 1, 2, 4, 8 levels up, 8 bits each (255 = none): the kinematics by pointer doubling
    const int jrounds = M.jump_rounds;
    // Kinematics of the whole tree in jrounds = ceil(log2(depth + 1)) rounds of pointer doubling (4 for the SMPL tree, depth 8) instead of
    // one step per level: every link holds its pose RELATIVE to the ancestor 2^k levels up (to the world once that ancestor lies above the
    // root) and composes it with that ancestor's entry - all lanes work in every round, where the level loop has the links of one depth
    // work and the others wait (~1100 -> ~420 instruction slots per substep).  Poses first, then the velocities the same way:
    //   w_b = w_A + W,   xd_b = xd_A + w_A x (x_b - x_A) + V       (W, V) of b relative to A;  composing with A's own (W_A, V_A) over A':
    //   W' = W_A + W,    V' = V_A + W_A x (x_b - x_A) + V
    // The root's lane holds the world values (the floating base's state) from the start.  qj / wj: the joint's quaternion and rate (body
    // axes), lp: the joint's offset in the parent's frame.  Out: world pose and velocity of every link, rr = the offset in world axes,
    // wrel = the joint's rate in world axes.
    auto kin_jump = [&](Q4& q_, V3& x_, V3& w_, V3& xd_, const Q4& qj, const V3& wj, const V3& lp, V3& rr, V3& wrel) {
        const bool link = valid && dep >= 1;
        Q4 Q = link ? qj : q_;
        V3 X = link ? lp : x_;
        for (int rd = 0; rd < jrounds; ++rd) {
            const int al = (aj >> (8 * rd)) & 255;
            const bool has = al != 255;
            const int src = has ? base + al : lane;
            const Q4 Qa = pull(Q, src);
            const V3 Xa = pull(X, src);
            if (has) {
                X = Xa + mul(q2mat(Qa), X);
                Q = qmul(Qa, Q);
            }
        }
        if (link) {
            q_ = qnormalize(Q);
            x_ = X;
        }
        const Q4 pq = pull(q_, plane);
        if (link) {
            rr = mul(q2mat(pq), lp);
            wrel = mul(q2mat(q_), wj);
        }
        V3 W = link ? wrel : w_, V = link ? V3{0.f, 0.f, 0.f} : xd_;
        for (int rd = 0; rd < jrounds; ++rd) {
            const int al = (aj >> (8 * rd)) & 255;
            const bool has = al != 255;
            const int src = has ? base + al : lane;
            const V3 Wa = pull(W, src), Va = pull(V, src), xa = pull(x_, src);
            if (has) {
                V = Va + cross(Wa, x_ - xa) + V;
                W = Wa + W;
            }
        }
        if (link) {
            w_ = W;
            xd_ = V;
        }
    };
    // opt-in (v2p_sim_cfg.freeze_terminated_envs): an env whose reset flag is set keeps its state; a wave whose two envs are frozen
    // skips the substeps altogether (frozen envs sort to the end of the launch order, so they share waves)
    const bool frozen = P.freeze_terminated && a.reset[e] == 1;
    const int nsub = (P.freeze_terminated && !any64(!frozen)) ? 0 : P.nsub;
    // substeps of this job (a job that gave up waiting replays the earlier ones)
    const int sub0 = handed ? jstart(sjob) : 0, sub1 = mono ? nsub : (nsub ? (jstart(sjob + 1) < nsub ? jstart(sjob + 1) : nsub) : 0);
    auto ldin = [&](const float* p) -> float { return handed ? cload(p) : *p; };

    // inputs of the fused pre-physics, REQUESTED here, in front of the hand-over loads (inline asm that waits for its own loads), and used
    // behind them: the two memory latencies of a job's prologue overlap
    const bool pre_on = a.actions && valid && live_env;
    long long pre_reset = 0;
    float pre_a0 = 0.f, pre_a1 = 0.f, pre_a2 = 0.f, pre_q0 = 0.f, pre_q1 = 0.f, pre_q2 = 0.f;
    if (pre_on) {
        pre_reset = a.reset[e];
        if (b != 0) {
            const float* ap = a.actions + e * NACT + 3 * (b - 1);
            const float* qd = a.x_dof + (e * NDOF + 3 * (b - 1)) * 2;
            pre_a0 = ap[0]; pre_a1 = ap[1]; pre_a2 = ap[2];
            pre_q0 = qd[0]; pre_q1 = qd[2]; pre_q2 = qd[4];
        }
    }
    // ---- state: the root lane carries the root pose/velocity, every other lane its joint
    Q4 q{0.f, 0.f, 0.f, 1.f}, jq{0.f, 0.f, 0.f, 1.f};
    V3 x{0.f, 0.f, 0.f}, w{0.f, 0.f, 0.f}, xd{0.f, 0.f, 0.f}, wt{0.f, 0.f, 0.f}, tar{0.f, 0.f, 0.f};
    // (JOBS: the job of an env's first substep reads the engine's state, the others what the job before them handed over: 16-byte chunks,
    // chunk 2b, 2b+1 = joint b (quaternion | rate), chunks 0, 1, 48, 49 = the root (quat | pos, vx | vy, vz, wx, wy | wz))
    // (one hand-over slot per substep: slot s holds the state after substep s)
    float* const hand = JOBS && handed ? a.job_hand + ((int64_t)(sjob - 1) * N + e) * HAND_FLOATS : nullptr;
    bool got = false;
    bool bgot = false;  // (BALL) the ball lane has its state from the hand-over
    if constexpr (JOBS) if (handed) {
        f4 c0, c1;
        cload4x2(hand + 4 * hand_link(b), hand + 4 * (hand_link(b) + 1), c0, c1);
        if (b == 0) {
            f4 c2, c3;
            cload4x2(hand + 4 * HAND_ROOT_VEL, hand + 4 * (HAND_ROOT_VEL + 1), c2, c3);
            q = Q4{c0.x, c0.y, c0.z, c0.w};
            x = V3{c1.x, c1.y, c1.z};
            xd = V3{c1.w, c2.x, c2.y};
            w = V3{c2.z, c2.w, c3.x};
            if (a.actions && valid && jstart(sjob) < a.p.hold_sub) {
                // the residual wrench of the fused step travels with the root's chunks while a later job still needs it (it is held for the
                // first hold_sub substeps only): force behind w.z, torque in its own chunk
                f4 c4, c5;
                cload4x2(hand + 4 * HAND_TORQUE, hand + 4 * HAND_TORQUE, c4, c5);
                wrench_put(wave_lds + base, WRENCH_FORCE_LANE, c3[HAND_FORCE_AT], c3[HAND_FORCE_AT + 1], c3[HAND_FORCE_AT + 2]);
                wrench_put(wave_lds + base, WRENCH_TORQUE_LANE, c4.x, c4.y, c4.z);
            }
        } else {
            jq = Q4{c0.x, c0.y, c0.z, c0.w};
            wt = V3{c1.x, c1.y, c1.z};
        }
        got = true;
    }
    if (b == 0) {
        if (!got) {
            q = Q4{st[SIDX(ST_ROOT_QUAT + 0)], st[SIDX(ST_ROOT_QUAT + 1)], st[SIDX(ST_ROOT_QUAT + 2)], st[SIDX(ST_ROOT_QUAT + 3)]};
            x = V3{st[SIDX(ST_ROOT_POS + 0)], st[SIDX(ST_ROOT_POS + 1)], st[SIDX(ST_ROOT_POS + 2)]};
            xd = V3{st[SIDX(ST_VEL + 0)], st[SIDX(ST_VEL + 1)], st[SIDX(ST_VEL + 2)]};
            w = V3{st[SIDX(ST_VEL + 3)], st[SIDX(ST_VEL + 4)], st[SIDX(ST_VEL + 5)]};
        }
    } else {
        const int jb = ST_JQUAT + 4 * (b - 1), vb = ST_VEL + 6 + 3 * (b - 1), cb = CT_PD + 3 * (b - 1);
        if (!got) {
            jq = Q4{st[SIDX(jb + 0)], st[SIDX(jb + 1)], st[SIDX(jb + 2)], st[SIDX(jb + 3)]};
            wt = V3{st[SIDX(vb + 0)], st[SIDX(vb + 1)], st[SIDX(vb + 2)]};
        }
        if (!a.actions) tar = V3{ldin(&a.ctrl[CIDX(cb + 0)]), ldin(&a.ctrl[CIDX(cb + 1)]), ldin(&a.ctrl[CIDX(cb + 2)])};
    }
    // the residual root wrench of the fused step: lanes WRENCH_FORCE_LANE and WRENCH_TORQUE_LANE of the env keep it in the PARK_TAR slots of
    // their LDS columns (neither has a joint target)
    float* const wrench_park = wave_lds + base;
    if (pre_on) {
        // ---- pre-physics fused in (same functions, same rounding as env_pre_kernel below): lane b owns the three action components of
        // its joint, the root lane the residual wrench; dead envs are masked in place on the caller's tensor.  EVERY job of the env derives
        // the PD targets and the wrench itself - from the caller's actions and the exposed state of the start of the step, which nothing
        // overwrites before the env's last job has read them - instead of having the first job hand them over through `ctrl`: 75 dword
        // write-through stores per env, each its own fabric write (PMC: WRITE_SIZE)
        const bool dead = pre_reset == 1;
        if (b != 0) {
            float* ap = a.actions + e * NACT + 3 * (b - 1);
            float ax = pre_a0, ay = pre_a1, az = pre_a2;
            if (dead) {
                ax = ay = az = 0.f;
                if (first_job) { ap[0] = 0.f; ap[1] = 0.f; ap[2] = 0.f; }
            }
            const float lim = P.pd_tar_lim;
            tar = V3{strict::pd_clamp(ax, pre_q0, lim), strict::pd_clamp(ay, pre_q1, lim), strict::pd_clamp(az, pre_q2, lim)};
            if (first_job) {
                float* pt = a.pd_target + e * NDOF + 3 * (b - 1);
                pt[0] = tar.x; pt[1] = tar.y; pt[2] = tar.z;
            }
        } else {
            float* ap = a.actions + e * NACT + NDOF;
            float af[6] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
            const bool need_wrench = sub0 < P.hold_sub && !handed;
            if (!dead && need_wrench) {
#pragma unroll
                for (int k = 0; k < 6; ++k) af[k] = ap[k];
            }
            if (dead && first_job) {
#pragma unroll
                for (int k = 0; k < 6; ++k) ap[k] = 0.f;
            }
            if (need_wrench) {  // (a job past the substeps that hold the wrench has no use for it; a later job is handed it)
                const float* rq4 = a.x_rb + e * NB * 13 + 3;
                strict::V3 Fr, Tq;  // (not `F`: that is the form policy in this function)
                strict::residual_wrench2(rq4, af, P.res_force_scale, P.res_torque_scale, Fr, Tq);
                wrench_put(wrench_park, WRENCH_FORCE_LANE, Fr.x, Fr.y, Fr.z);
                wrench_put(wrench_park, WRENCH_TORQUE_LANE, Tq.x, Tq.y, Tq.z);
            }
        }
    }

    if (valid && b != 0) park_put3(PARK_TAR, tar);  // constant for the whole launch (the columns of the two wrench lanes hold the wrench there)
    const BallDev& BP = a.ball;
    // this env's racket, through its shape (BALL only).  (MULTI: the address is formed where it is used, from sid - live anyway - instead
    // of being kept in a register pair across the substep loop: that pair cost the per-env-shape ball kernels 16 B of scratch per lane)
    auto racket = [&]() -> ConstRacket* {
        int s = sid;
        if constexpr (MULTI) asm volatile("" : "+v"(s));
        return (ConstRacket*)BP.rackets + s;
    };
    const bool racket_lane = BALL && lb == racket()->racket_link;  // this lane's link carries the env's racket
    const bool ball_lane = BALL && lb == NB;  // the first idle lane of the env carries the ball
    if (ball_lane) {
        // (JOBS: state and aerodynamic force - held over a simulate() call - come from the job of the substep before: the ball's chunks,
        // BL_POS .. BL_F + 2 of the block)
        static_assert(BL_POS == 0 && BL_QUAT == 3 && BL_VEL == 7 && BL_ANG == 10 && BL_F == 13 && BL_GA == 4 * HAND_BALL_CHUNKS, "what is handed over of the ball: state 13 | aerodynamic force 3");
        if constexpr (JOBS) if (handed) {
            f4 c0, c1, c2, c3;
            cload4x2(hand + 4 * HAND_BALL, hand + 4 * (HAND_BALL + 1), c0, c1);
            cload4x2(hand + 4 * (HAND_BALL + 2), hand + 4 * (HAND_BALL + 3), c2, c3);
            // (written out, not a loop over the chunks: see the note at the storing side)
            bl[BL_POS] = c0.x; bl[BL_POS + 1] = c0.y; bl[BL_POS + 2] = c0.z; bl[BL_QUAT] = c0.w; bl[BL_QUAT + 1] = c1.x; bl[BL_QUAT + 2] = c1.y; bl[BL_QUAT + 3] = c1.z; bl[BL_VEL] = c1.w;
            bl[BL_VEL + 1] = c2.x; bl[BL_VEL + 2] = c2.y; bl[BL_ANG] = c2.z; bl[BL_ANG + 1] = c2.w; bl[BL_ANG + 2] = c3.x; bl[BL_F] = c3.y; bl[BL_F + 1] = c3.z; bl[BL_F + 2] = c3.w;
            bgot = true;
        }
        if (!bgot) {
#pragma unroll
            for (int k = BL_POS; k < BL_F; ++k) bl[k] = BP.state[e * 13 + k];
#pragma unroll
            for (int k = BL_F; k < BL_GA; ++k) bl[k] = 0.f;
        }
#pragma unroll
        for (int k = BL_GA; k < BL_SLOTS; ++k) bl[k] = 0.f;
    }
    long long tprev = DIAG && a.prof ? clock64() : 0;
    const long long wt0 = DIAG && a.wave_times ? wall_clock64() : 0;
    const int key_pred = DIAG && a.wave_times ? a.pair_key[e] : 0;  // what the launch order was built from (diagnostics)
    int tsum = 0, tmaxs = 0;
    V3 r{0.f, 0.f, 0.f};
    int ksum = 0, kdep = 0;  // contact load of this env over the launch (pairing key)
#if defined(V2P_LL_TIMELINE)
    // build-time diagnostics (tools/mkvariant.sh): wall-clock start / end of every JOB of the production kernels, by workgroup index
    const long long tl0 = a.wave_times ? wall_clock64() : 0, tc0 = a.wave_times ? clock64() : 0;
    auto timeline = [&]() {
        if (!DIAG && a.wave_times && lane == 0) {
            long long* tl = a.wave_times + (int64_t)jid * 4;
            tl[0] = tl0; tl[1] = wall_clock64(); tl[2] = (long long)bid + ((long long)sjob << 24) + ((long long)(mono ? 1 : 0) << 28) + ((long long)ksum << 32);
            tl[3] = clock64() - tc0;  // shader cycles of the job: with the wall clock, the clock the job ran at
        }
    };
#else
    auto timeline = [&]() {};
#endif

    for (int sub = sub0; sub < sub1; ++sub) {
        // (the substep length behind an opaque scalar move: the dozen uniform expressions of it - 1 / h, h / n_iter, erp / hs, 1 / (1 + h damping),
        // margin / h ... - are then evaluated where they are used, a few scalar-operand instructions each, instead of being hoisted in front
        // of the substep loop and kept - spilled: in the racket + ball kernels - across all of it)
        float h = h_launch;
        if constexpr (F::OPAQUE_H) asm volatile("" : "+s"(h));
        const bool wrench_on = sub < P.hold_sub;
        const bool last = sub == nsub - 1;
        // a substep that is being recomputed by a job that gave up waiting for its predecessor: it publishes nothing (the predecessor does)
        const bool replay = JOBS && !mono && sub < jstart(sjob);
        LLPH(PROF_HEAD);
        // per-link model constants are (re)loaded where they are used (L1/K$ hits) instead of pinning ~20 registers for the whole
        // kernel; the opaque index keeps the compiler from hoisting the loads back out of the substep loop
        int bo = b;
        asm volatile("" : "+v"(bo));
        const V3 lpos{S->local_pos[bo][0], S->local_pos[bo][1], S->local_pos[bo][2]};
        // ================================================================ pass 1: kinematics, by pointer doubling (kin_jump)
        V3 zw{0.f, 0.f, 0.f}, zv{0.f, 0.f, 0.f};
        {
            V3 wrel{0.f, 0.f, 0.f};
            kin_jump(q, x, w, xd, jq, wt, lpos, r, wrel);
            if (valid && dep >= 1) {
                const V3 pw = w - wrel, wpr = cross(pw, r);
                zw = cross(pw, wrel);
                zv = cross(pw, wpr);
            }
        }
        // (racket + ball: the ball lane and the ball x hull narrow phase run HERE, right after the kinematics, where a lane holds little
        // more than its pose and velocity: further down, next to the link's inertia blocks, their temporaries did not fit)
        if (BALL) {
            // pose and (start-of-substep) velocity of the racket's link, handed to the ball lane of the same env
            const int src = base + racket()->racket_link;
            const Q4 wq = pull(q, src);
            const V3 wx = pull(x, src), ww = pull(w, src), wxd = pull(xd, src);
            if (ball_lane) {
                const V3 bp{bl[BL_POS], bl[BL_POS + 1], bl[BL_POS + 2]}, bv{bl[BL_VEL], bl[BL_VEL + 1], bl[BL_VEL + 2]}, bw{bl[BL_ANG], bl[BL_ANG + 1], bl[BL_ANG + 2]};
                bl[BL_V0] = bv.x; bl[BL_V0 + 1] = bv.y; bl[BL_V0 + 2] = bv.z;  // (the hull points' activation test reads the velocity of the start of the substep)
#pragma unroll
                for (int j = 2; j < NBREC; ++j) {
                    lds_vfloat* rk = bl + BL_RK + 16 * j;
                    rk[RK_A] = 0.f; rk[RK_LINK] = -1.f;
                    rk[RK_LAM] = 0.f; rk[RK_LAM + 1] = 0.f; rk[RK_LAM + 2] = 0.f;
                }
                if (sub % BP.sub_per_sim == 0) {
                    // the reference's bounce test on the ball height at the start of every simulate() call (apply_external_force_to_ball, :731-737)
                    // (system-scope accesses: with substep jobs the calls of one step run in different workgroups)
                    const int64_t e = env_here();
                    if (BP.has_bounce && live_env && !replay) {
                        if (sub == 0) flag_st(&BP.has_bounce_now[e], 0);
                        if (bp.z <= BP.bounce_height && !flag_ld(&BP.has_bounce[e])) {
                            flag_st(&BP.has_bounce[e], 1);
                            flag_st(&BP.has_bounce_now[e], 1);
                            BP.bounce_pos[e * 3] = bp.x; BP.bounce_pos[e * 3 + 1] = bp.y; BP.bounce_pos[e * 3 + 2] = bp.z;
                        }
                    }
                    // aerodynamic force, re-evaluated before every simulate() call (humanoid_smpl_im_mvae.py:711-739, utils/tennis_ball.py)
                    const float kf = 1.21f * 3.14159265358979f * 0.032f * 0.032f * 0.5f, cd = 0.55f;
                    const float sp = PHYS_SQRT(dot(bv, bv)), vs = sp == 0.f ? 1.f : sp;
                    const V3 vn = PHYS_RCP(vs) * bv;
                    const V3 vt = cross(vn, V3{0.f, 0.f, -1.f}), lt = cross(vt, vn);
                    const float vspin = PHYS_SQRT(dot(bw, bw)) * (1.f / 6.28318530717959f);
                    float cl = PHYS_RCP(2.f + fabsf(vs * PHYS_RCP(vspin * BP.spin_scale + 1e-6f)));
                    cl = vspin > 0.f ? -cl : cl;
                    const V3 Fa = (-kf * cd * vs) * bv - (kf * cl * vs * vs) * lt;
                    bl[BL_F] = Fa.x; bl[BL_F + 1] = Fa.y; bl[BL_F + 2] = Fa.z;
                }
                const V3 Fa{bl[BL_F], bl[BL_F + 1], bl[BL_F + 2]};
                const V3 bvs = bv + h * (V3{0.f, 0.f, P.gravity_z} + BP.inv_mass * Fa);  // free flight: v*
                bl[BL_VEL] = bvs.x; bl[BL_VEL + 1] = bvs.y; bl[BL_VEL + 2] = bvs.z;
                const float ih = PHYS_RCP(h), coff = P.contact_offset;
                // ---- ball x ground (speculative margin: the distance the ball can close within this substep)
                {
                    const float gap = bp.z - BP.radius;
                    const bool on = CONTACT && gap < coff + h * fmaxf(0.f, -bv.z);
                    float bias = gap >= 0.f ? gap * ih : fmaxf(P.erp * gap * ih, -P.max_depen);
                    const float rest = (bvs.z < -BP.bounce_thr && gap * ih + bvs.z < 0.f) ? BP.rest_ground * bvs.z : 3.0e38f;  // restitution
                    bias = fminf(bias, rest);
                    bl[BL_GA] = on ? 1.f : 0.f; bl[BL_GGAP] = gap; bl[BL_GBIAS] = bias;
                    if (TGS) bl[BL_GREST] = rest;
                    bl[BL_GLAM] = 0.f; bl[BL_GLAM + 1] = 0.f; bl[BL_GLAM + 2] = 0.f;
                }
                // ---- ball x the racket's solid cylinders: closest point, normal from the cylinder to the ball
                const M3 Rw = q2mat(wq);
                ConstRacket* const RS = racket();
#pragma unroll
                for (int j = 0; j < 2; ++j) {
                    lds_vfloat* rk = bl + BL_RK + 16 * j;
                    bool on = false;
                    if (CONTACT && j < RS->ncyl) {
                        const V3 cw = wx + mul(Rw, V3{RS->cyl[j][0], RS->cyl[j][1], RS->cyl[j][2]}), aw = mul(Rw, V3{RS->cyl[j][3], RS->cyl[j][4], RS->cyl[j][5]});
                        const float hl = RS->cyl[j][6], rc = RS->cyl[j][7];
                        const V3 d = bp - cw;
                        const float t = dot(d, aw);
                        const V3 qv = d - t * aw;
                        const float rho = PHYS_SQRT(dot(qv, qv));
                        const float tc = fminf(fmaxf(t, -hl), hl), kq = rho > rc ? rc * PHYS_RCP(rho) : 1.f;
                        const V3 pt = cw + tc * aw + kq * qv;
                        const V3 ev = bp - pt;
                        // (centre inside the solid: pt is bp up to rounding and the direction of ev is noise - out through the nearer cap)
                        const float dist = (fabsf(t) <= hl && rho <= rc) ? 0.f : PHYS_SQRT(dot(ev, ev));
                        const V3 n = dist > 1e-6f ? PHYS_RCP(dist) * ev : (t >= 0.f ? aw : -aw);
                        const V3 rl = pt - wx;
                        const float vrel = dot(bv - wxd - cross(ww, rl), n);
                        const float gap = dist - BP.radius;
                        on = gap < coff + h * fmaxf(0.f, -vrel);
                        rk[RK_GAP] = gap;
                        rk[RK_RL] = rl.x; rk[RK_RL + 1] = rl.y; rk[RK_RL + 2] = rl.z;
                        rk[RK_N] = n.x; rk[RK_N + 1] = n.y; rk[RK_N + 2] = n.z;
                    }
                    rk[RK_A] = on ? 1.f : 0.f;
                    rk[RK_LAM] = 0.f; rk[RK_LAM + 1] = 0.f; rk[RK_LAM + 2] = 0.f;
                }
            }
            if (CONTACT && BP.body_contacts) {
                // ---- ball x the hulls of the links (every shape of the humanoid collides with the ball actor): each link lane tests its
                // own hull - bounding box first -, the nearest hull that the ball can reach within this substep carries the point
                const V3 bp{bl[BL_POS], bl[BL_POS + 1], bl[BL_POS + 2]}, bv0{bl[BL_V0], bl[BL_V0 + 1], bl[BL_V0 + 2]};
                const float coff = P.contact_offset;
                bool near = false;
                V3 cb{0.f, 0.f, 0.f};
                const M3 R = q2mat(q);
                if (valid && !racket_lane) {
                    cb = mulT(R, bp - x);  // ball centre, body frame
                    const V3 ac{S->aabb_c[bo][0], S->aabb_c[bo][1], S->aabb_c[bo][2]}, ae{S->aabb_e[bo][0], S->aabb_e[bo][1], S->aabb_e[bo][2]};
                    const V3 ex{fmaxf(fabsf(cb.x - ac.x) - ae.x, 0.f), fmaxf(fabsf(cb.y - ac.y) - ae.y, 0.f), fmaxf(fabsf(cb.z - ac.z) - ae.z, 0.f)};
                    const V3 dv = bv0 - xd;
                    const float vmax = PHYS_SQRT(dot(dv, dv)) + PHYS_SQRT(dot(w, w)) * (PHYS_SQRT(dot(ac, ac)) + PHYS_SQRT(dot(ae, ae)));
                    const float reach = BP.radius + coff + h * vmax;
                    near = dot(ex, ex) < reach * reach && S->hull_count[bo] > 0;
                }
                if (any64(near)) {
                    float gap = 3.0e38f;
                    V3 rlw{0.f, 0.f, 0.f}, nw{0.f, 0.f, 1.f};
                    if (near) {
                        const int hv0 = S->hull_offsets[bo], hnv = S->hull_count[bo];
                        const f4 hc = ball_hull_distance(S, hv0, hnv, cb);
                        V3 pb{hc.x, hc.y, hc.z};
                        float dist = hc.w;
                        V3 nb;
                        if (dist > 1e-6f) nb = PHYS_RCP(dist) * (cb - pb);
                        else {  // centre inside the hull: out along the direction from the centre of the bounding box
                            const V3 ev = cb - V3{S->aabb_c[bo][0], S->aabb_c[bo][1], S->aabb_c[bo][2]};
                            const float l = PHYS_SQRT(dot(ev, ev));
                            nb = l > 1e-5f ? PHYS_RCP(l) * ev : V3{0.f, 0.f, 1.f};  // (closer than float32 resolves: +z, like the oracle)
                            dist = 0.f;
                            pb = cb;
                        }
                        nw = mul(R, nb);
                        rlw = mul(R, pb);
                        const float vrel = dot(bv0 - xd - cross(w, rlw), nw);
                        const float g = dist - BP.radius;
                        if (g < coff + h * fmaxf(0.f, -vrel)) gap = g;
                    }
                    // the (up to) three nearest of the env's candidates, nearest first (ties: the lower link): one point per overlapping link,
                    // as PhysX generates one per overlapping pair - the LDS block holds three next to the cylinders' two
#pragma unroll 1
                    for (int k = 0; k < NBREC - 2; ++k) {
                        float gmin = gap;
#pragma unroll
                        for (int sh = 1; sh < 32; sh <<= 1) gmin = fminf(gmin, __shfl_xor(gmin, sh));
                        const unsigned long long wb = __ballot(gap == gmin && gap < 3.0e38f);
                        if (!wb) break;
                        const unsigned wmine = half ? (unsigned)(wb >> 32) : (unsigned)wb;
                        if (wmine && lb == __ffs(wmine) - 1) {
                            lds_vfloat* rk = bl + BL_RK + 16 * (2 + k);
                            rk[RK_A] = 1.f;
                            rk[RK_GAP] = gap;
                            rk[RK_RL] = rlw.x; rk[RK_RL + 1] = rlw.y; rk[RK_RL + 2] = rlw.z;
                            rk[RK_N] = nw.x; rk[RK_N + 1] = nw.y; rk[RK_N + 2] = nw.z;
                            rk[RK_LINK] = (float)lb;
                            gap = 3.0e38f;  // taken
                        }
                    }
                }
            }
        }
        // ================================================================ contact generation
        // One block (ll_contact_setup.inc: a fragment of this function, included at both places - the same statements either way), run at
        // one of two places (F::CGEN_EARLY, ll_forms.hpp): HERE, right behind the kinematics, with the pose still in registers - it reads
        // nothing but the pose, the shape tables and constants -, or between pass 3 and the Lambda recursion, where the pose comes back from
        // its slots and the root's Lambda waits in LDS meanwhile.  What it leaves behind: the records in the lane's LDS column (PARK_CR ..
        // PARK_CL; no pass parks anything there, see the slots) and the number of points, from which the touched masks, the depth of each
        // env's deepest stop and sweep_on are formed in front of the Lambda recursion.
        // (what the early place hands to the later one; the other kernels declare `cnt`, `CS` where they always did - a declaration that
        // moves changes their register allocation)
        [[maybe_unused]] int cnt_early = 0;
        [[maybe_unused]] ContactStore<PARK3> CS_early(park);
        if constexpr (F::CGEN_EARLY) {
            LLPH(PROF_PASS1);  // (the kinematics; the per-link block below adds itself to the same counter)
            int cnt = 0;
            ContactStore<PARK3> CS(park);
#include "ll_contact_setup.inc"
            cnt_early = cnt;
            CS_early = CS;
            LLPH(PROF_CONTACTS);  // (a substep without a sweep too)
        }
        // ---- per link, all lanes at once: joint torque, body inertia at its origin (world axes), bias force
        // mass properties are needed once per substep: reload them (L1/K$ hits) instead of pinning 10 registers for the
        // whole kernel; the opaque index keeps the loads from being hoisted back out of the loop
        const float mass = S->mass[bo];
        const V3 com{S->com[bo][0], S->com[bo][1], S->com[bo][2]};
        const Sym3 Ib{S->inertia[bo][0], S->inertia[bo][1], S->inertia[bo][2], S->inertia[bo][3], S->inertia[bo][4], S->inertia[bo][5]};
        V3 tau{0.f, 0.f, 0.f};
        float lsgn[3] = {0.f, 0.f, 0.f}, lbias[3] = {0.f, 0.f, 0.f}, llam[3] = {0.f, 0.f, 0.f};  // LIMITS: this joint's rows (sign 0 = none)
        bool limact = false;
        Sym3 Kd{1.f, 0.f, 0.f, 1.f, 0.f, 1.f};  // LIMITS: joint-space inverse inertia of this joint, body axes
        Sym3 A;
        M3 B;
        Sym3 C{mass, 0.f, 0.f, mass, 0.f, mass};
        V3 pn, pf;
        {
            const M3 R = q2mat(q);
            const float kp = S->kp[bo], kd = S->kd[bo];
            const V3 qe = b != 0 ? quat_to_expmap_stable(jq) : V3{0.f, 0.f, 0.f};
            if (b != 0) tau = mul(R, kp * (park_get3(PARK_TAR) - qe) - (kd + h * kp) * wt);
            if (LIMITS) {
                limact = false;
                const float ih = PHYS_RCP(h);
#pragma unroll
                for (int i = 0; i < 3; ++i) {
                    const float lo = S->limit_lo[bo][i], hi = S->limit_hi[bo][i], qi = i == 0 ? qe.x : (i == 1 ? qe.y : qe.z);
                    const bool on = P.joint_limits && valid && b != 0 && hi - lo < 6.28f;
                    const float clo = qi - lo, chi = hi - qi;
                    const float gap = clo <= chi ? clo : chi;
                    lsgn[i] = on ? (clo <= chi ? 1.f : -1.f) : 0.f;
                    lbias[i] = TGS ? gap : (gap >= 0.f ? gap * ih : fmaxf(P.erp * gap * ih, -P.max_depen));  // (TGS: the gap, advanced slice by slice)
                    llam[i] = 0.f;
                    limact = limact || on;
                }
            }
            V3 dc = mul(R, com);
            V3 k0 = mul(Ib, V3{R.m[0], R.m[1], R.m[2]});
            V3 k1 = mul(Ib, V3{R.m[3], R.m[4], R.m[5]});
            V3 k2 = mul(Ib, V3{R.m[6], R.m[7], R.m[8]});
            V3 r0 = row(R, 0), r1 = row(R, 1), r2 = row(R, 2);
            Sym3 Ic{dot(r0, k0), dot(r0, k1), dot(r0, k2), dot(r1, k1), dot(r1, k2), dot(r2, k2)};
            float dd = dot(dc, dc);
            A = Sym3{Ic.xx + mass * (dd - dc.x * dc.x), Ic.xy - mass * dc.x * dc.y, Ic.xz - mass * dc.x * dc.z,
                     Ic.yy + mass * (dd - dc.y * dc.y), Ic.yz - mass * dc.y * dc.z, Ic.zz + mass * (dd - dc.z * dc.z)};
            B.m[0] = 0.f;            B.m[1] = -mass * dc.z;  B.m[2] = mass * dc.y;
            B.m[3] = mass * dc.z;    B.m[4] = 0.f;           B.m[5] = -mass * dc.x;
            B.m[6] = -mass * dc.y;   B.m[7] = mass * dc.x;   B.m[8] = 0.f;
            V3 wwd = cross(w, cross(w, dc));
            pf = mass * (wwd - V3{0.f, 0.f, P.gravity_z});
            pn = cross(w, mul(Ic, w)) + cross(dc, pf);
            if (b == 0 && wrench_on) {
                V3 extF, extT;
                if (a.actions) {
                    extF = wrench_get(wrench_park, WRENCH_FORCE_LANE);
                    extT = wrench_get(wrench_park, WRENCH_TORQUE_LANE);
                } else {
                    const float* cw = a.ctrl + env_here() * CTRL_SLOTS;
                    extF = V3{ldin(&cw[CT_FORCE + 0]), ldin(&cw[CT_FORCE + 1]), ldin(&cw[CT_FORCE + 2])};
                    extT = V3{ldin(&cw[CT_TORQUE + 0]), ldin(&cw[CT_TORQUE + 1]), ldin(&cw[CT_TORQUE + 2])};
                }
                pn = pn - extT - cross(dc, extF);  // force acts at the root COM
                pf = pf - extF;
            }
        }

        // pose of the link: next used by contact generation (unless it has run already, F::CGEN_EARLY), then by the integration
        park[PARK_Q * 64] = q.x; park[(PARK_Q + 1) * 64] = q.y; park[(PARK_Q + 2) * 64] = q.z; park[(PARK_Q + 3) * 64] = q.w;
        park_put3(PARK_X, x);
        LLPH(PROF_PASS1);
        park_vel(w, xd);
        // ================================================================ pass 2: articulated inertia, leaves -> root by level
        Sym3 Di{1.f, 0.f, 0.f, 1.f, 0.f, 1.f};
        M3 E;
#pragma unroll
        for (int i = 0; i < 9; ++i) E.m[i] = 0.f;
        V3 u{0.f, 0.f, 0.f};
        // A level's contributions are written by the lanes at that depth only and stay in their registers (no zero-fill per level: the
        // other lanes keep what they last wrote).  The receiving adds run under an EXEC mask instead: the parents of the level - and,
        // with them, every lane at depth >= d.  Those have to stay switched on, because a DPP shift or a ds_bpermute returns 0 for a
        // source lane that EXEC has switched off, and they are the sources; what they add onto their own A, B, C, pn, pf in passing is
        // never read: a link's own level is the last to read them (only the root's are read after the loop, and the root, depth 0, is
        // never among these lanes).  Links are in depth-first order: the lane after a parent with a first child is that child, at
        // depth d.  The sums of the values that are used are the same adds as with zero-filled contributions and selects.
        Sym3 cA{0.f, 0.f, 0.f, 0.f, 0.f, 0.f}, cC{0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
        M3 cB;
#pragma unroll
        for (int i = 0; i < 9; ++i) cB.m[i] = 0.f;
        V3 cn{0.f, 0.f, 0.f}, cf{0.f, 0.f, 0.f};
        for (int d = maxd; d >= 1; --d) {
            // (the comparisons below read an opaque scalar copy of the level: comparing `dep` with the loop counter itself lets value
            // numbering put the per-lane `dep` in the counter's place, and the loop then runs with its counter in a VGPR and per-lane exits)
            int dl = d;
            asm volatile("" : "+s"(dl));
            if (dep == dl) {
                Sym3 D{A.xx + aug, A.xy, A.xz, A.yy + aug, A.yz, A.zz + aug};
                Di = inv(D);
                E = mul(Di, B);
                u = tau - pn;
                Sym3 Aa{aug * (1.f - aug * Di.xx), -aug * aug * Di.xy, -aug * aug * Di.xz, aug * (1.f - aug * Di.yy), -aug * aug * Di.yz,
                        aug * (1.f - aug * Di.zz)};
                M3 Ba;
#pragma unroll
                for (int i = 0; i < 9; ++i) Ba.m[i] = aug * E.m[i];
                V3 b0 = col(B, 0), b1 = col(B, 1), b2 = col(B, 2), e0 = col(E, 0), e1 = col(E, 1), e2 = col(E, 2);
                Sym3 Ca{C.xx - dot(b0, e0), C.xy - dot(b0, e1), C.xz - dot(b0, e2), C.yy - dot(b1, e1), C.yz - dot(b1, e2), C.zz - dot(b2, e2)};
                V3 Diu = mul(Di, u);
                V3 pan = pn + mul(Aa, zw) + mul(Ba, zv) + (u - aug * Diu);
                V3 paf = pf + V3{dot(col(Ba, 0), zw), dot(col(Ba, 1), zw), dot(col(Ba, 2), zw)} + mul(Ca, zv) +
                         V3{dot(e0, u), dot(e1, u), dot(e2, u)};
                // shift to the parent origin: S = [r]x Ca (columns r x Ca_col)
                V3 s0 = cross(r, V3{Ca.xx, Ca.xy, Ca.xz}), s1 = cross(r, V3{Ca.xy, Ca.yy, Ca.yz}), s2 = cross(r, V3{Ca.xz, Ca.yz, Ca.zz});
                cB.m[0] = Ba.m[0] + s0.x; cB.m[1] = Ba.m[1] + s1.x; cB.m[2] = Ba.m[2] + s2.x;
                cB.m[3] = Ba.m[3] + s0.y; cB.m[4] = Ba.m[4] + s1.y; cB.m[5] = Ba.m[5] + s2.y;
                cB.m[6] = Ba.m[6] + s0.z; cB.m[7] = Ba.m[7] + s1.z; cB.m[8] = Ba.m[8] + s2.z;
                if constexpr (F::P2SHIFT) {
                    // cA = Aa + [r]x Ba^T + cB^T [r]x^T:  cA_ij = Aa_ij + (r x row_i(Ba))_j + (r x row_j(cB))_i, upper triangle; the second
                    // cross carries [r]x Ca [r]x^T through the cB formed above
                    auto shifted = [&](float aa, int i, int j) { return cross_at_plus(cross_at_plus(aa, r, row(Ba, i), j), r, row(cB, j), i); };
                    cA = Sym3{shifted(Aa.xx, 0, 0), shifted(Aa.xy, 0, 1), shifted(Aa.xz, 0, 2), shifted(Aa.yy, 1, 1), shifted(Aa.yz, 1, 2), shifted(Aa.zz, 2, 2)};
                } else {
                    V3 t10 = cross(r, row(Ba, 0)), t11 = cross(r, row(Ba, 1)), t12 = cross(r, row(Ba, 2));
                    V3 sr0{s0.x, s1.x, s2.x}, sr1{s0.y, s1.y, s2.y}, sr2{s0.z, s1.z, s2.z};
                    V3 t20 = cross(r, sr0), t21 = cross(r, sr1), t22 = cross(r, sr2);
                    cA = Sym3{Aa.xx + 2.f * t10.x + t20.x, Aa.xy + t10.y + t11.x + t20.y, Aa.xz + t10.z + t12.x + t20.z,
                              Aa.yy + 2.f * t11.y + t21.y, Aa.yz + t11.z + t12.y + t21.z, Aa.zz + 2.f * t12.z + t22.z};
                }
                cC = Ca;
                cn = pan + cross(r, paf);
                cf = paf;
            }
            if (dep >= dl || (dep == dl - 1 && has0)) {
                A = A + from_next(cA);
                C = C + from_next(cC);
                M3 t = from_next(cB);
#pragma unroll
                for (int i = 0; i < 9; ++i) B.m[i] += t.m[i];
                pn = pn + from_next(cn);
                pf = pf + from_next(cf);
            }
            if ((multi >> d) & 1) {
#pragma unroll 1
                for (int sl = 1; sl <= 2; ++sl) {  // one extra child at a time keeps the register peak down
                    const int cl = sl == 1 ? cl1 : cl2;
                    const bool hs = sl == 1 ? has1 : has2;
                    if (dep >= dl || (dep == dl - 1 && hs)) {
                        A = A + pull(cA, cl);
                        C = C + pull(cC, cl);
                        M3 t1 = pull(cB, cl);
#pragma unroll
                        for (int i = 0; i < 9; ++i) B.m[i] += t1.m[i];
                        pn = pn + pull(cn, cl);
                        pf = pf + pull(cf, cl);
                    }
                }
            }
        }

        LLPH(PROF_PASS2);
        unpark_vel(w, xd);
        // ================================================================ root: 6x6 solve (lane 0 of each env)
        // (F::CGEN_EARLY: the root's Lambda goes straight from here into the recursion; the other lanes keep these placeholders until the
        // recursion writes them)
        Blocks Lam;  // operational-space inverse inertia of this lane's link (root: inverse articulated inertia)
        Lam.A = Lam.C = Sym3{1.f, 0.f, 0.f, 1.f, 0.f, 1.f};
#pragma unroll
        for (int i = 0; i < 9; ++i) Lam.B.m[i] = 0.f;
        V3 al{0.f, 0.f, 0.f}, ac{0.f, 0.f, 0.f}, dw{0.f, 0.f, 0.f}, dv{0.f, 0.f, 0.f};
        if (lb == 0) {
            float a6[21], inv6[21];
            a6[tri(0, 0)] = A.xx; a6[tri(1, 0)] = A.xy; a6[tri(2, 0)] = A.xz; a6[tri(1, 1)] = A.yy; a6[tri(2, 1)] = A.yz; a6[tri(2, 2)] = A.zz;
#pragma unroll
            for (int i = 0; i < 3; ++i)
#pragma unroll
                for (int j = 0; j < 3; ++j) a6[tri(3 + i, j)] = B.m[3 * j + i];
            a6[tri(3, 3)] = C.xx; a6[tri(4, 3)] = C.xy; a6[tri(5, 3)] = C.xz; a6[tri(4, 4)] = C.yy; a6[tri(5, 4)] = C.yz; a6[tri(5, 5)] = C.zz;
            spd6_inverse(a6, inv6);
            Lam.A = Sym3{inv6[tri(0, 0)], inv6[tri(1, 0)], inv6[tri(2, 0)], inv6[tri(1, 1)], inv6[tri(2, 1)], inv6[tri(2, 2)]};
#pragma unroll
            for (int i = 0; i < 3; ++i)
#pragma unroll
                for (int j = 0; j < 3; ++j) Lam.B.m[3 * i + j] = inv6[tri(3 + j, i)];
            Lam.C = Sym3{inv6[tri(3, 3)], inv6[tri(4, 3)], inv6[tri(5, 3)], inv6[tri(4, 4)], inv6[tri(5, 4)], inv6[tri(5, 5)]};
            al = -(mul(Lam.A, pn) + mul(Lam.B, pf));
            ac = -(V3{dot(col(Lam.B, 0), pn), dot(col(Lam.B, 1), pn), dot(col(Lam.B, 2), pn)} + mul(Lam.C, pf));
            dw = h * al;
            dv = h * ac;
            w = w + dw;
            xd = xd + dv;
        }

        // ================================================================ pass 3: accelerations -> v*, root -> leaves by level
        for (int d = 1; d <= maxd; ++d) {
            const bool nc = (nonchain >> d) & 1;
            V3 alp = pp(al, nc), acp = pp(ac, nc), dwp = pp(dw, nc), dvp = pp(dv, nc);
            if (dep == d) {
                V3 aw = alp + zw;
                V3 av = acp + cross(alp, r) + zv;
                V3 qdd = mul(Di, u + aug * aw) - aw - mul(E, av);
                al = aw + qdd;
                ac = av;
                dw = dwp + h * qdd;  // v* - v_old at the OLD configuration
                dv = dvp + cross(dwp, r);
                w = w + dw;
                xd = xd + dv;
            }
        }

        LLPH(PROF_PASS3);
        if (CONTACT) park_vel(w, xd);
        float* const rootlam = wave_lds + LDS_ROOTLAM + half * ROOTLAM_ROW;
        if (PARK2 && CONTACT && !F::CGEN_EARLY && lb == 0) {  // only the root's Lambda exists yet: 21 floats per env, out of the way while contacts are generated
            const float lv[21] = {Lam.A.xx, Lam.A.xy, Lam.A.xz, Lam.A.yy, Lam.A.yz, Lam.A.zz, Lam.B.m[0], Lam.B.m[1], Lam.B.m[2], Lam.B.m[3], Lam.B.m[4], Lam.B.m[5],
                                  Lam.B.m[6], Lam.B.m[7], Lam.B.m[8], Lam.C.xx, Lam.C.xy, Lam.C.xz, Lam.C.yy, Lam.C.yz, Lam.C.zz};
#pragma unroll
            for (int k = 0; k < 21; ++k) rootlam[k] = lv[k];
        }
        if (PARK2 && CONTACT && !F::CGEN_EARLY) {  // (the other lanes' values are placeholders until the recursion writes them)
            Lam.A = Lam.C = Sym3{1.f, 0.f, 0.f, 1.f, 0.f, 1.f};
#pragma unroll
            for (int i = 0; i < 9; ++i) Lam.B.m[i] = 0.f;
        }
        if constexpr (!F::CGEN_EARLY) {
            q = Q4{park[PARK_Q * 64], park[(PARK_Q + 1) * 64], park[(PARK_Q + 2) * 64], park[(PARK_Q + 3) * 64]};
            x = park_get3(PARK_X);
        }
        int cnt = 0;
        ContactStore<PARK3> CS(park);
        if constexpr (F::CGEN_EARLY) {
            cnt = cnt_early;
            CS = CS_early;
        } else {
#include "ll_contact_setup.inc"
        }
        if (CONTACT) {
            if (PARK2 && !F::CGEN_EARLY && lb == 0) {  // Lambda of the root back from its block
                float lv[21];
#pragma unroll
                for (int k = 0; k < 21; ++k) lv[k] = rootlam[k];
                Lam.A = Sym3{lv[0], lv[1], lv[2], lv[3], lv[4], lv[5]};
#pragma unroll
                for (int k = 0; k < 9; ++k) Lam.B.m[k] = lv[6 + k];
                Lam.C = Sym3{lv[15], lv[16], lv[17], lv[18], lv[19], lv[20]};
            }
            // (with a ball: the racket's link joins the touched links while the ball is in contact with a cylinder)
            // (point j of the ball block belongs to this lane's link: j = 0, 1 the racket's cylinders, j = 2 .. 4 the hull points)
            auto ball_rec_mine = [&](int j) -> bool { return j < 2 ? racket_lane : lb == (int)bl[BL_RK + 16 * j + RK_LINK]; };
            bool myhull = false;  // this link's hull carries a ball point
            if (BALL) {
#pragma unroll
                for (int j = 2; j < NBREC; ++j) myhull = myhull || (bl[BL_RK + 16 * j + RK_A] != 0.f && lb == (int)bl[BL_RK + 16 * j + RK_LINK]);
            }
            const bool ballhit = BALL && valid && ((racket_lane && (bl[BL_RK + RK_A] != 0.f || bl[BL_RK + 16 + RK_A] != 0.f)) || myhull);
            const bool ballground = BALL && ball_lane && bl[BL_GA] != 0.f;
            const bool touched = valid && (cnt > 0 || ballhit);
            const unsigned long long tb = __ballot(touched);
            const unsigned m0 = (unsigned)tb, m1 = (unsigned)(tb >> 32);
            if (LIMITS && any64(limact)) {
                // speculative activation of the limit rows (the model is stated in oracle/phys/v2p_phys_oracle.c): a row exists in this substep
                // only while its DOF is within limit_margin of the limit or would reach it at the approach rate of v* (the joint rate after
                // the unconstrained update: link velocity minus the parent's, body axes).  Joints far from their limits are no stops of the
                // walk and Lambda is not carried down to them.
                const V3 wv = PARK2 ? park_get3(PARK_W0) : w;
                const V3 pwv = pp(wv, true);
                const V3 om = mulT(q2mat(q), wv - pwv);
                const float mrate = P.limit_margin * PHYS_RCP(h);
                const float lscale = TGS ? PHYS_RCP(h) : 1.f;  // (TGS keeps the gap itself: gap / h is what the test compares, negative when violated either way)
                bool anyrow = false;
#pragma unroll
                for (int i = 0; i < 3; ++i) {
                    const float omi = i == 0 ? om.x : (i == 1 ? om.y : om.z);
                    const bool on = lsgn[i] != 0.f && lbias[i] * lscale < mrate + fmaxf(0.f, -lsgn[i] * omi);  // (violated: lbias < 0)
                    if (!on) lsgn[i] = 0.f;
                    anyrow = anyrow || on;
                }
                limact = anyrow;
            }
            const unsigned long long lmb = LIMITS ? __ballot(valid && limact) : 0ull;
            const unsigned lm0 = (unsigned)lmb, lm1 = (unsigned)(lmb >> 32);
            if (DIAG && a.wave_times) { const int tt = __popc(half ? m1 : m0); tsum += tt; tmaxs = tt > tmaxs ? tt : tmaxs; }
            // (F::SETUPX, with the visit table: the depth of each env's deepest touched link by a reduction on the DPP network, ll_forms.hpp)
            [[maybe_unused]] int tdep0 = 0, tdep1 = 0;
            if constexpr (F::SETUPX) {
                // (half_max_last: all 64 lanes are on here - top level of the substep - and the value is never negative; `touched` keeps
                // the 99 of the idle lanes out)
                const int tdred = half_max_last(touched ? dep : 0);
                tdep0 = __builtin_amdgcn_readlane(tdred, 31);
                tdep1 = __builtin_amdgcn_readlane(tdred, 63);
            }
            if (last) {
                const unsigned mine = half ? m1 : m0;
                ksum = __popc(mine);
                if constexpr (F::SETUPX) {
                    kdep = half ? tdep1 : tdep0;
                } else {
                    kdep = 0;
                    for (unsigned t = mine; t; t &= t - 1) { const int dd = M.depth[__ffs(t) - 1]; kdep = dd > kdep ? dd : kdep; }
                }
            }
            if (DIAG && a.prof && LLSAMPLED) { atomicAdd((unsigned long long*)&a.prof[PROF_TOUCHED], (unsigned long long)(__popc(m0) + __popc(m1))); atomicAdd((unsigned long long*)&a.prof[PROF_SUBSTEPS], 1ull); }
            const bool sweep_on = ((m0 | m1 | lm0 | lm1) || (BALL && any64(ballground))) && P.n_iter > 0;
            if (PARK2 && !sweep_on) unpark_vel(w, xd);
            if (sweep_on) {
                // deepest touched link of either env: links below it are never read during the sweep, so Lambda and the
                // per-update propagation stop there; their velocities catch up once at the end (the propagation is linear)
                // (each env stops at ITS deepest touched link, so its arithmetic does not depend on which env shares the wave)
                int dn0 = 0, dn1 = 0;
                if constexpr (F::SETUPX) {
                    dn0 = tdep0;
                    dn1 = tdep1;
                } else {
                    for (unsigned t = m0 | lm0; t; t &= t - 1) { const int dd = M.depth[__ffs(t) - 1]; dn0 = dd > dn0 ? dd : dn0; }
                    for (unsigned t = m1 | lm1; t; t &= t - 1) { const int dd = M.depth[__ffs(t) - 1]; dn1 = dd > dn1 ? dd : dn1; }
                }
                const int dneed = dn0 > dn1 ? dn0 : dn1, dmin = dn0 < dn1 ? dn0 : dn1;
                const bool insweep = dep <= (half ? dn1 : dn0);  // this link moves with every update; the others catch up afterwards
                LLPH(PROF_CONTACTS);
                // ======================================================== Lambda_b, root -> leaves by level
                for (int d = 1; d <= dneed; ++d) {
                    Blocks Lp;
                    const bool nc = (nonchain >> d) & 1;
                    Lp.A = pp(Lam.A, nc);
                    Lp.B = pp(Lam.B, nc);
                    Lp.C = pp(Lam.C, nc);
                    if (dep == d) {
                        // G = X Lp X^T: Ga = La ; Gb = La [r]x + Lb ; Gc = Lc - [r]x Lb + Gb^T [r]x
                        V3 la0{Lp.A.xx, Lp.A.xy, Lp.A.xz}, la1{Lp.A.xy, Lp.A.yy, Lp.A.yz}, la2{Lp.A.xz, Lp.A.yz, Lp.A.zz};
                        M3 Gb;
                        Sym3 Gc;
                        if constexpr (F::LAMX) {
                            // (every entry two / four fused multiply-adds on the parent's entry: Gc_kj = Lc_kj + (col_k(Gb) x r)_j + (col_j(Lb) x r)_k)
#pragma unroll
                            for (int i = 0; i < 3; ++i)
#pragma unroll
                                for (int j = 0; j < 3; ++j) Gb.m[3 * i + j] = cross_at_plus(Lp.B.m[3 * i + j], i == 0 ? la0 : (i == 1 ? la1 : la2), r, j);
                            auto gc = [&](float c, int k, int j) { return cross_at_plus(cross_at_plus(c, col(Gb, k), r, j), col(Lp.B, j), r, k); };
                            Gc = Sym3{gc(Lp.C.xx, 0, 0), gc(Lp.C.xy, 0, 1), gc(Lp.C.xz, 0, 2), gc(Lp.C.yy, 1, 1), gc(Lp.C.yz, 1, 2), gc(Lp.C.zz, 2, 2)};
                        } else {
                            {
                                V3 g0 = cross(la0, r) + row(Lp.B, 0), g1 = cross(la1, r) + row(Lp.B, 1), g2 = cross(la2, r) + row(Lp.B, 2);
                                Gb.m[0] = g0.x; Gb.m[1] = g0.y; Gb.m[2] = g0.z; Gb.m[3] = g1.x; Gb.m[4] = g1.y; Gb.m[5] = g1.z; Gb.m[6] = g2.x; Gb.m[7] = g2.y; Gb.m[8] = g2.z;
                            }
                            {
                                V3 q0 = cross(col(Gb, 0), r), q1 = cross(col(Gb, 1), r), q2 = cross(col(Gb, 2), r);
                                V3 n0 = cross(r, col(Lp.B, 0)), n1 = cross(r, col(Lp.B, 1)), n2 = cross(r, col(Lp.B, 2));
                                Gc.xx = Lp.C.xx + q0.x - n0.x;
                                Gc.xy = Lp.C.xy + q0.y - n1.x;
                                Gc.xz = Lp.C.xz + q0.z - n2.x;
                                Gc.yy = Lp.C.yy + q1.y - n1.y;
                                Gc.yz = Lp.C.yz + q1.z - n2.y;
                                Gc.zz = Lp.C.zz + q2.z - n2.z;
                            }
                        }
                        // Lambda_b = [Di 0; 0 0] + T^T G T,  T = [aug Di, 0; -E^T, 1]
                        // By blocks, with P = aug Di (symmetric) and Ga = Lp.A:  H1 = Ga P - Gb E^T ( = M1^T, M1 = P Ga - E Gb^T ),
                        // Lam.B = P Gb - E Gc,  Lam.A = Di + M1 P - Lam.B E^T,  Lam.C = Gc.
                        M3 H1;  // (the joint-limit block below reads it)
                        if constexpr (F::LAMX) {
                            // every entry once: aug (Di . G) - E . G in fused multiply-adds, the scale on the finished dot (scaled_dot_minus_dot);
                            // of the symmetric Lam.A the upper triangle
#pragma unroll
                            for (int i = 0; i < 3; ++i)
#pragma unroll
                                for (int j = 0; j < 3; ++j) {
                                    H1.m[3 * j + i] = scaled_dot_minus_dot(aug, row(Di, i), j == 0 ? la0 : (j == 1 ? la1 : la2), row(E, i), row(Gb, j));
                                    Lam.B.m[3 * i + j] = scaled_dot_minus_dot(aug, row(Di, i), col(Gb, j), row(E, i), row(Gc, j));
                                }
                            auto lam_a = [&](float di, int i, int j) { return scaled_dot_minus_dot(di, aug, col(H1, i), row(Di, j), row(Lam.B, i), row(E, j)); };
                            Lam.A = Sym3{lam_a(Di.xx, 0, 0), lam_a(Di.xy, 0, 1), lam_a(Di.xz, 0, 2), lam_a(Di.yy, 1, 1), lam_a(Di.yz, 1, 2), lam_a(Di.zz, 2, 2)};
                        } else {
                            M3 DiM;
                            DiM.m[0] = Di.xx; DiM.m[1] = Di.xy; DiM.m[2] = Di.xz; DiM.m[3] = Di.xy; DiM.m[4] = Di.yy; DiM.m[5] = Di.yz; DiM.m[6] = Di.xz; DiM.m[7] = Di.yz; DiM.m[8] = Di.zz;
                            M3 H2;
#pragma unroll
                            for (int i = 0; i < 3; ++i) {
                                V3 gai = i == 0 ? la0 : (i == 1 ? la1 : la2);
                                V3 gbi = row(Gb, i);
                                V3 gbti = col(Gb, i);
                                V3 gci = i == 0 ? V3{Gc.xx, Gc.xy, Gc.xz} : (i == 1 ? V3{Gc.xy, Gc.yy, Gc.yz} : V3{Gc.xz, Gc.yz, Gc.zz});
#pragma unroll
                                for (int j = 0; j < 3; ++j) {
                                    V3 dj = col(DiM, j);
                                    V3 ej = row(E, j);
                                    H1.m[3 * i + j] = aug * dot(gai, dj) - dot(gbi, ej);
                                    H2.m[3 * i + j] = aug * dot(gbti, dj) - dot(gci, ej);
                                }
                            }
                            M3 t;
#pragma unroll
                            for (int i = 0; i < 3; ++i)
#pragma unroll
                                for (int j = 0; j < 3; ++j) t.m[3 * i + j] = aug * dot(row(DiM, i), col(H1, j)) - dot(row(E, i), col(H2, j));
                            Lam.A = Sym3{Di.xx + t.m[0], Di.xy + 0.5f * (t.m[1] + t.m[3]), Di.xz + 0.5f * (t.m[2] + t.m[6]), Di.yy + t.m[4],
                                         Di.yz + 0.5f * (t.m[5] + t.m[7]), Di.zz + t.m[8]};
#pragma unroll
                            for (int i = 0; i < 3; ++i)
#pragma unroll
                                for (int j = 0; j < 3; ++j) {
                                    V3 gcj = j == 0 ? V3{Gc.xx, Gc.xy, Gc.xz} : (j == 1 ? V3{Gc.xy, Gc.yy, Gc.yz} : V3{Gc.xz, Gc.yz, Gc.zz});
                                    Lam.B.m[3 * i + j] = aug * dot(row(DiM, i), col(Gb, j)) - dot(row(E, i), gcj);
                                }
                        }
                        Lam.C = Gc;
                        if (LIMITS && limact) {
                            const Sym3 K{Lam.A.xx - 2.f * H1.m[0] + Lp.A.xx, Lam.A.xy - H1.m[1] - H1.m[3] + Lp.A.xy, Lam.A.xz - H1.m[2] - H1.m[6] + Lp.A.xz,
                                         Lam.A.yy - 2.f * H1.m[4] + Lp.A.yy, Lam.A.yz - H1.m[5] - H1.m[7] + Lp.A.yz, Lam.A.zz - 2.f * H1.m[8] + Lp.A.zz};
                            const M3 R = q2mat(Q4{park[PARK_Q * 64], park[(PARK_Q + 1) * 64], park[(PARK_Q + 2) * 64], park[(PARK_Q + 3) * 64]});
                            const V3 c0 = col(R, 0), c1 = col(R, 1), c2 = col(R, 2);
                            const V3 k0 = mul(K, c0), k1 = mul(K, c1), k2 = mul(K, c2);
                            Kd = Sym3{dot(c0, k0), dot(c0, k1), dot(c0, k2), dot(c1, k1), dot(c1, k2), dot(c2, k2)};
                        }
                    }
                }

                // direction a = 0, 1, 2 of a ball x racket point: its normal and the tangent basis t1 = normalize(n x z) (n x x when n is
                // within 1e-3 of +-z), t2 = n x t1 - the oracle's rule
                auto ball_dirs = [&](V3 n, V3& t1, V3& t2) {
                    t1 = cross(n, V3{0.f, 0.f, 1.f});
                    if (dot(t1, t1) < 1e-6f) t1 = cross(n, V3{1.f, 0.f, 0.f});
                    t1 = rsqrtf(dot(t1, t1)) * t1;
                    t2 = cross(n, t1);
                };
                if (PARK2) unpark_vel(w, xd);
                if (BALL && ballhit) {
                    // row biases of the ball x racket points from the velocities before the sweep (restitution: Newton, against the approach speed)
                    const V3 bv{bl[BL_VEL], bl[BL_VEL + 1], bl[BL_VEL + 2]}, bw{bl[BL_ANG], bl[BL_ANG + 1], bl[BL_ANG + 2]};
                    const float ih = PHYS_RCP(h);
#pragma unroll
                    for (int j = 0; j < NBREC; ++j) {
                        lds_vfloat* rk = bl + BL_RK + 16 * j;
                        if (rk[RK_A] != 0.f && ball_rec_mine(j)) {
                            const V3 n{rk[RK_N], rk[RK_N + 1], rk[RK_N + 2]}, rl{rk[RK_RL], rk[RK_RL + 1], rk[RK_RL + 2]};
                            const float gap = rk[RK_GAP];
                            const float vn0 = dot(bv + cross(bw, -BP.radius * n) - xd - cross(w, rl), n);
                            float bias = gap >= 0.f ? gap * ih : fmaxf(P.erp * gap * ih, -P.max_depen);
                            const float rest = (vn0 < -BP.bounce_thr && gap * ih + vn0 < 0.f) ? (j < 2 ? BP.rest_racket : BP.rest_body) * vn0 : 3.0e38f;
                            bias = fminf(bias, rest);
                            rk[RK_BIAS] = bias;
                            if (TGS) rk[RK_REST] = rest;
                        }
                    }
                }
                LLPH(PROF_LAMBDA);
                if (!PARK2) {
                    park_put3(PARK_W0, w);  // the sweep's total delta-velocity of a link = its velocity at the end - these
                    park_put3(PARK_XD0, xd);
                }
                // touched links whose parent is the touched link right before them (ascending).  Nothing reads these masks any more (the
                // per-group sweep that did is gone), but without this loop the compiler lowered the control flow of the sweep differently
                // (-0.5 %, later -1.1 %: docs/NOTES.md B, 2026-10-19).  With the set-up of F::SETUPX in front of the sweep that no longer
                // holds (measured again, same section): those kernels go without it; the others keep the loop and stay as they were.
                if constexpr (!F::SETUPX) {
                    [[maybe_unused]] unsigned chain0 = 0u, chain1 = 0u;
                    int prev = -1;
                    for (unsigned t = m0; t; t &= t - 1) {
                        const int nn = __ffs(t) - 1;
                        if ((int)((a.par_pack[nn / 12] >> (5 * (nn % 12))) & 31ull) == prev) chain0 |= 1u << nn;
                        prev = nn;
                    }
                    prev = -1;
                    for (unsigned t = m1; t; t &= t - 1) {
                        const int nn = __ffs(t) - 1;
                        if ((int)((a.par_pack[nn / 12] >> (5 * (nn % 12))) & 31ull) == prev) chain1 |= 1u << nn;
                        prev = nn;
                    }
                    chain0 &= ~lm0;  // the limit rows of a joint come between its parent's block and its own: no chaining into it
                    chain1 &= ~lm1;
                }
                // ======================================================== block Gauss-Seidel: k-th touched body of each env at once
                const float hs = h / (float)P.n_iter;  // TGS: length of a time slice
                float tgs_irem = 1.f / h;                // TGS: 1 / (time left in the substep) for separated points
                const float tgs_pen = P.erp / hs;
                auto rowbias = [&](float v) -> float { return TGS ? (v >= 0.f ? v * tgs_irem : fmaxf(tgs_pen * v, -P.max_depen)) : v; };
                // ---- the sweep as ONE WALK over the tree.  Solving the touched links one by one in ascending order visits them in depth-first
                // order, cyclically, iteration after iteration; between two of them only
                // the links on the tree path cur -> LCA -> next need anything:
                //   up    cur .. LCA: every link hands what its subtree has collected since it last did so (un_new, uf_new) to its parent,
                //         and the LCA answers what arrives with its own Lambda (Lambda_cc is the response of the whole system at c);
                //   down  LCA .. next: velocity change of a link = its parent's, carried over the joint, + the joint's answer to everything
                //         its subtree has collected so far (un_tot) - the relation the root -> leaves pass uses, valid here because a
                //         depth-first walk enters a subtree only after everything applied inside it has been handed up through its root.
                // (Dw, Dv) of a link = its velocity change since the start of the sweep, valid whenever the walk stands on it; w, xd keep
                // the velocities of the start of the sweep.  After the last iteration the walk returns to the root and ONE root -> leaves
                // pass moves every link.  By linearity the row updates see exactly the velocities of the one-by-one sweep with a
                // leaf -> root -> leaves propagation after every link; that costs (touched groups x 2 x depth) level steps per iteration,
                // the walk 2 x (edges of the subtree the touched links span): the same for two feet on the ground, about half for a
                // fallen humanoid with 7 scattered touched links - the critical path of a launch.
                // TGS advances the gaps with the velocities after every iteration: there the walk is closed after every iteration.
                V3 un_tot{0.f, 0.f, 0.f}, un_new{0.f, 0.f, 0.f}, uf_new{0.f, 0.f, 0.f}, Dw{0.f, 0.f, 0.f}, Dv{0.f, 0.f, 0.f};
                int cur0 = 0, cur1 = 0;            // link the walk of each env stands on
                bool live0 = false, live1 = false;  // the env has applied an impulse (until then all its changes are zero and its walk rests)
                // the move INTO each touched link, from the touched link before it (cyclically): depth of their lowest common ancestor |
                // depth of the link before << 4 | own depth << 8 | side-entry levels << 12 (12 bits).  (A link has depth + 1 ancestors-or-self: depths from ballots.)
                // LIMITS: the walk also stops at the joints that carry limit rows (their block comes right before the contact block of the link)
                const unsigned v0 = LIMITS ? m0 | lm0 : m0, v1 = LIMITS ? m1 | lm1 : m1;
                V3 jt_new{0.f, 0.f, 0.f};  // LIMITS: limit impulse of this joint not yet handed up (its reaction, -jt, goes to the parent)
                // F::VTAB (the kernels without joint limits and TGS): the same moves filed by VISIT instead of by link.  The walk takes the k-th
                // stop of both envs in the same visit, in every iteration, so everything about visit k but `live` and `done` is fixed for the
                // substep:
                //   vis    lane k of an env's half: the move into its k-th stop (as minfo) | bit 24: the env moves in this visit once it is
                //          live - it has a k-th stop and more than one stop.  (An env with fewer stops than its partner rests in the surplus
                //          visits, its lanes there hold 0; an env with a single stop stands on it for the whole substep.)
                //   anc    per lane: bit k + 1 = this link is an ancestor (or self) of its env's k-th stop, bit 0 = ... of its LAST stop.
                //          The walk stands on the previous stop, cyclically, from the env's first visit on, whether it is live or not, and
                //          before that visit the env is not live and does not move: in visit k "on the path from where the walk stands"
                //          is bit k, "on the path to the next stop" bit k + 1 (the move into stop 0 of a later iteration comes from the
                //          env's own last stop, whose number differs between the envs: hence a bit of its own).  24 links: 25 bits.
                //   mystop the visit in which this lane's link is its env's stop, or -1
                // (24 links per env: every env's stops fit the 32 lanes of its half, the table has no capacity limit.)
                // (which kernels run which form - F::VTAB, and with it F::LIVEM, F::ROWX, F::ROWCNT - and why: ll_forms.hpp)
                int minfo = 0;
                [[maybe_unused]] int vis = 0, mystop = -1, nvis0 = 0, nvis1 = 0;
                [[maybe_unused]] int livem = 0;  // F::LIVEM: bit h = env h is live (wave-uniform, in a scalar register)
                [[maybe_unused]] unsigned anc = 0u;
                // The table (F::VTAB) is formed by the STOPS' OWN LANES, all at once, instead of stop by stop for the wave: a stop's lane knows
                // its number (the stops below it in its env's mask), the stop before it (cyclically), its own depth and number of points;
                // the depths of the stop before and of their lowest common ancestor are counts of the model's ancestor masks (what the
                // three ballots per stop of the earlier form counted), read with the side levels in loads under one wait.  The word goes
                // to lane k of the env through the wave's scratch row in LDS (free outside contact generation).  What is left of the loop
                // over the stops is the bit of `anc`: the ancestor mask of the env's k-th stop, read from the stop's lane, IS the lane
                // mask of bit k + 1 - both envs' masks side by side are one 64-bit lane mask, one select and one OR per stop.
                if constexpr (F::VTAB) {
                    const unsigned mine = half ? v1 : v0;
                    nvis0 = __popc(v0);
                    nvis1 = __popc(v1);
                    const int nmine = half ? nvis1 : nvis0;
                    const unsigned below = mine & ((1u << lb) - 1u);
                    const int kme = __popc(below);
                    const int plast0 = v0 ? 31 - __clz(v0) : 0, plast1 = v1 ? 31 - __clz(v1) : 0;
                    const unsigned ancme = valid ? (unsigned)M.anc_mask[bo] : 0u;  // (bit i: link i is an ancestor of this lane's link, or the link itself)
                    int* const vrow = (int*)(park + PARK_SCR * 64);  // this lane's word of the scratch row
                    if (valid && ((mine >> lb) & 1u)) {
                        const int pv = below ? 31 - __clz(below) : (half ? plast1 : plast0);
                        const unsigned ancp = (unsigned)M.anc_mask[pv];
                        const int sdp = M.side_depths[pv];
                        const int du = __popc(ancp) - 1, dl = __popc(ancp & ancme) - 1;
                        // (levels of the way up where the path link is not its parent's first child: it hands over through a pull, see walk_to)
                        const int sd = sdp & ~((2 << dl) - 1);
                        // (bits 25 - 27, F::ROWCNT: the stop's number of points)
                        vrow[kme - lb] = dl | (du << 4) | (dep << 8) | ((sd & 0xfff) << 12) | (nmine > 1 ? 1 << 24 : 0) | (F::ROWCNT ? cnt << 25 : 0);
                        mystop = kme;
                    }
                    vis = lb < nmine ? vrow[0] : 0;
                    auto lanes_of = [&](unsigned lo, unsigned hi) -> bool { return __builtin_amdgcn_inverse_ballot_w64(((unsigned long long)hi << 32) | lo); };
                    // (bit 0: the env's last stop; an env without stops: link 0, as before)
                    anc = lanes_of(__builtin_amdgcn_readlane(ancme, plast0), __builtin_amdgcn_readlane(ancme, 32 + plast1)) ? 1u : 0u;
                    // (an env that has run out of stops reads lane 31 of its half: no link, an empty mask)
                    int k = 1;
                    for (unsigned s0 = v0, s1 = v1; s0 | s1; s0 &= s0 - 1, s1 &= s1 - 1, ++k) {
                        const unsigned a0 = __builtin_amdgcn_readlane(ancme, __ffs(s0 | 0x80000000u) - 1);
                        const unsigned a1 = __builtin_amdgcn_readlane(ancme, 32 + __ffs(s1 | 0x80000000u) - 1);
                        anc |= lanes_of(a0, a1) ? 1u << k : 0u;
                    }
                } else {
                    int p0 = v0 ? 31 - __clz(v0) : 0, p1 = v1 ? 31 - __clz(v1) : 0;
                    for (unsigned s0 = v0, s1 = v1; s0 | s1; s0 &= s0 - 1, s1 &= s1 - 1) {
                        const int b0 = s0 ? __ffs(s0) - 1 : p0, b1 = s1 ? __ffs(s1) - 1 : p1;
                        const int selp = half ? p1 : p0, selb = half ? b1 : b0;
                        const bool ap = valid && ((desc >> selp) & 1), ab = valid && ((desc >> selb) & 1);
                        const unsigned long long bp = __ballot(ap), bb = __ballot(ab), bc = __ballot(ap && ab);
                        const int du = __popc(half ? (unsigned)(bp >> 32) : (unsigned)bp) - 1, dn = __popc(half ? (unsigned)(bb >> 32) : (unsigned)bb) - 1,
                                  dl = __popc(half ? (unsigned)(bc >> 32) : (unsigned)bc) - 1;
                        // (levels of the way up where the path link is not its parent's first child: it hands over through a pull, see walk_to)
                        const int sd = (half ? M.side_depths[p1] : M.side_depths[p0]) & ~((2 << dl) - 1);
                        // (bit 28: the link itself is not its parent's first child - the one-joint bounce of a limit block needs it)
                        if (valid && lb == selb && ((half ? s1 : s0) != 0u)) minfo = dl | (du << 4) | (dn << 8) | (sd << 12) | ((LIMITS && !firstchild) ? 1 << 28 : 0);
                        p0 = b0;
                        p1 = b1;
                    }
                }
                if constexpr (F::VTAB) {  // (nothing tracks where a walk stands; where it closes, after whole sweeps, it stands on the env's last stop)
                    cur0 = v0 ? 31 - __clz(v0) : 0;
                    cur1 = v1 ? 31 - __clz(v1) : 0;
                }
                // (F::UPMASK: whether walk_to runs the way up in its masked form, ll_forms.hpp)
                // one move of both walks: env h goes from cur_h to its next link when mv_h (info_h = the move, see minfo), else it rests
                [[maybe_unused]] int vk = 0;  // F::VTAB: the visit in which walk_to runs (it reads the roles from anc; nx0, nx1 are not used then)
                auto walk_to = [&](int nx0, int nx1, int info0, int info1, bool mv0, bool mv1) {
                    long long tsub = DIAG && a.prof ? clock64() : 0;
                    // a resting env: empty ranges that do not widen the loops (LCA depth 15, depths 0)
                    // (readfirstlane: the compiler must see wave-uniform loop bounds, or it runs the level loops with per-lane exits)
                    const int pk0 = __builtin_amdgcn_readfirstlane(mv0 ? info0 : 0x00f), pk1 = __builtin_amdgcn_readfirstlane(mv1 ? info1 : 0x00f);
                    const int dl0 = pk0 & 15, dn0 = (pk0 >> 8) & 15;
                    const int dl1 = pk1 & 15, dn1 = (pk1 >> 8) & 15;
                    const int selc = half ? cur1 : cur0, seln = half ? nx1 : nx0, mydl = half ? dl1 : dl0;
                    // ancestors (or self) of cur / of next
                    const bool onc = F::VTAB ? ((anc >> vk) & 1u) != 0u : valid && ((desc >> selc) & 1), onn = F::VTAB ? ((anc >> vk) & 2u) != 0u : valid && ((desc >> seln) & 1);
                    // LIMITS: a way up on which no link holds anything to hand over is not walked (the stops at joints whose limit rows
                    // do not act - most of them - leave nothing behind; the lowest common ancestor has been current since the walk came
                    // down through it): that env's way up counts as resting
                    int uk0 = pk0, uk1 = pk1;
                    if constexpr (LIMITS) {
                        const bool pend = onc && dep > mydl && (un_new.x != 0.f || un_new.y != 0.f || un_new.z != 0.f || uf_new.x != 0.f || uf_new.y != 0.f || uf_new.z != 0.f ||
                                                                jt_new.x != 0.f || jt_new.y != 0.f || jt_new.z != 0.f);
                        const unsigned long long pb = __ballot(pend);
                        uk0 = __builtin_amdgcn_readfirstlane((unsigned)pb ? pk0 : 0x00f);
                        uk1 = __builtin_amdgcn_readfirstlane((unsigned)(pb >> 32) ? pk1 : 0x00f);
                    }
                    const int du0 = (uk0 >> 4) & 15, du1 = (uk1 >> 4) & 15, ul0 = uk0 & 15, ul1 = uk1 & 15, myul = half ? ul1 : ul0;
                    // depth of this lane's link if it is on the way up (cur .. LCA + 1) / on the way down (LCA + 1 .. next), else -1
                    const int updep = (onc && dep > myul) ? dep : -1, dndep = (onn && dep > mydl) ? dep : -1;
                    const int turndep = (onc && dep == myul) ? dep : -2;  // the LCA itself: where this env's move turns
                    const int ulmin = ul0 < ul1 ? ul0 : ul1, dlmin = dl0 < dl1 ? dl0 : dl1;
                    // levels (bit d = the links at depth d hand over) on which a path link is not the first child of its parent (it does not
                    // sit in the lane next to it and hands over through a pull)
                    const unsigned sideb = ((unsigned)(uk0 >> 12) | (unsigned)(uk1 >> 12)) & 0xfffu;
                    // ---- up  (levels in a gap between the two envs' ranges run idle: a range test here makes the compiler run the whole
                    // loop with per-lane exits and d in a VGPR)
                    // A level's cn, cf are written by the one link per env that hands over (updep == d) and stay in its registers: no
                    // zero-fill, the other lanes hold whatever they last wrote.  What arrives is added under an EXEC mask instead: the
                    // handing links and their parents (the ancestor of cur at depth d - 1).  A DPP shift and a ds_bpermute return 0 for a
                    // source lane that EXEC has switched off, and the only lanes switched on at depth d are the handing ones; so a parent
                    // receives its handing child's values through the shift (first child), through a pull (second, third child; a link
                    // without such a child pulls from lane 31 of its env, which is never on), and zeros from every other source, and
                    // the handing links - the lane after them and their children are off - add zeros onto what they have just cleared.
                    // rn, rf = what arrived last; a lane receives on one level of a move only (its own depth + 1), so after the loop the
                    // link where this env's walk turns still holds what arrived there, and answers it with its Lambda - once, behind the
                    // loop, for both envs together (zeros if its level was not walked).  One form for every level: no select, no copy
                    // between two forms, Dw, Dv are not touched inside the loop.
                    if constexpr (F::UPMASK) {
                        const int dmax = du0 > du1 ? du0 : du1;
                        if (dmax > ulmin) {
                            const int rcdep = onc ? dep + 1 : -1;  // the level on which this lane's link receives
                            const int ucl1 = has1 ? cl1 : base + 31, ucl2 = has2 ? cl2 : base + 31;
                            V3 cn, cf, rn{0.f, 0.f, 0.f}, rf{0.f, 0.f, 0.f};
                            asm("" : "=v"(cn.x), "=v"(cn.y), "=v"(cn.z), "=v"(cf.x), "=v"(cf.y), "=v"(cf.z));  // (never read before they are written)
                            for (int dctr = dmax; dctr > ulmin; --dctr) {
                                // (an opaque SCALAR copy of the level for everything the body compares with per-lane depths: value numbering
                                // otherwise rewrites the loop counter itself with the per-lane value it was found equal to, and the whole loop
                                // runs with its counter in a VGPR and per-lane exits - +20 VALU instructions per level)
                                int d = dctr;
                                asm volatile("" : "+s"(d));
                                if (updep == d) {
                                    // cn = aug Di un_new + r x fa,  fa = uf_new - E^T un_new.  (Written as the fused chains the compiler used to
                                    // make of the plain expressions: under -fassociative-math the order of a sum follows the shape of the code
                                    // around it, and the dumps of bench.py pin this one)
                                    const float axx = aug * Di.xx, axy = aug * Di.xy, axz = aug * Di.xz, ayy = aug * Di.yy, ayz = aug * Di.yz, azz = aug * Di.zz;
                                    const V3 na{__builtin_fmaf(un_new.x, axx, __builtin_fmaf(un_new.y, axy, un_new.z * axz)),
                                                __builtin_fmaf(un_new.x, axy, __builtin_fmaf(un_new.y, ayy, un_new.z * ayz)),
                                                __builtin_fmaf(un_new.x, axz, __builtin_fmaf(un_new.y, ayz, un_new.z * azz))};
                                    const V3 fa{uf_new.x - __builtin_fmaf(un_new.x, E.m[0], __builtin_fmaf(E.m[3], un_new.y, E.m[6] * un_new.z)),
                                                uf_new.y - __builtin_fmaf(un_new.x, E.m[1], __builtin_fmaf(E.m[4], un_new.y, E.m[7] * un_new.z)),
                                                uf_new.z - __builtin_fmaf(un_new.x, E.m[2], __builtin_fmaf(E.m[5], un_new.y, E.m[8] * un_new.z))};
                                    cn = V3{__builtin_fmaf(fa.z, r.y, __builtin_fmaf(-r.z, fa.y, na.x)), __builtin_fmaf(-r.x, fa.z, __builtin_fmaf(fa.x, r.z, na.y)),
                                            __builtin_fmaf(fa.y, r.x, __builtin_fmaf(-r.y, fa.x, na.z))};
                                    cf = fa;
                                    un_new = V3{0.f, 0.f, 0.f};
                                    uf_new = V3{0.f, 0.f, 0.f};
                                }
                                if (updep == d || rcdep == d) {
                                    rn = from_next(cn);
                                    rf = from_next(cf);
                                    if ((sideb >> d) & 1u) {
                                        rn = rn + pull(cn, ucl1) + pull(cn, ucl2);
                                        rf = rf + pull(cf, ucl1) + pull(cf, ucl2);
                                    }
                                    un_new = un_new + rn;
                                    uf_new = uf_new + rf;
                                    un_tot = un_tot + rn;
                                }
                            }
                            if (turndep >= 0) {
                                Dw = Dw + mul(Lam.A, rn) + mul(Lam.B, rf);
                                Dv = Dv + V3{dot(col(Lam.B, 0), rn), dot(col(Lam.B, 1), rn), dot(col(Lam.B, 2), rn)} + mul(Lam.C, rf);
                            }
                        }
                    } else {
                        // (the earlier form: contributions zero-filled on every level, selects for the first-child and side-entry masks,
                        // the turn inside the loop on the levels of the long form)
                        const unsigned longb = sideb | (ul0 < 15 ? 2u << ul0 : 0u) | (ul1 < 15 ? 2u << ul1 : 0u);
                        for (int dctr = du0 > du1 ? du0 : du1; dctr > ulmin; --dctr) {
                            // (an opaque SCALAR copy of the level for everything the body compares with per-lane depths: where the body tests
                            // `turndep == d - 1`, value numbering rewrites the loop counter itself with the per-lane value it was found equal to, and
                            // the whole loop runs with its counter in a VGPR and per-lane exits - +20 VALU instructions per level)
                            int d = dctr;
                            asm volatile("" : "+s"(d));
                            V3 cn{0.f, 0.f, 0.f}, cf{0.f, 0.f, 0.f};
                            if (updep == d) {
                                const V3 na = aug * mul(Di, un_new);
                                const V3 fa = uf_new - V3{dot(col(E, 0), un_new), dot(col(E, 1), un_new), dot(col(E, 2), un_new)};
                                cn = na + cross(r, fa);
                                cf = fa;
                                un_new = V3{0.f, 0.f, 0.f};
                                uf_new = V3{0.f, 0.f, 0.f};
                                if (LIMITS) {  // the reaction of the joint's limit impulses: a pure torque on the parent
                                    cn = cn - jt_new;
                                    jt_new = V3{0.f, 0.f, 0.f};
                                }
                            }
                            if (!((longb >> d) & 1u)) {
                                // every link that hands over is the first child of its parent = the lane before it; the others hand over zeros:
                                // the shifted values are added as they are (DPP operand of the add)
                                un_new = un_new + from_next(cn);
                                uf_new = uf_new + from_next(cf);
                                un_tot = un_tot + from_next(cn);
                            } else {
                                // what arrives is kept apart: the link where a walk turns answers it with its Lambda
                                V3 rn = from_next(mask(firstchild, cn)), rf = from_next(mask(firstchild, cf));
                                if ((sideb >> d) & 1u) {
                                    rn = rn + mask(has1, pull(cn, cl1)) + mask(has2, pull(cn, cl2));
                                    rf = rf + mask(has1, pull(cf, cl1)) + mask(has2, pull(cf, cl2));
                                }
                                un_new = un_new + rn;
                                uf_new = uf_new + rf;
                                un_tot = un_tot + rn;
                                if (turndep == d - 1) {
                                    Dw = Dw + mul(Lam.A, rn) + mul(Lam.B, rf);
                                    Dv = Dv + V3{dot(col(Lam.B, 0), rn), dot(col(Lam.B, 1), rn), dot(col(Lam.B, 2), rn)} + mul(Lam.C, rf);
                                }
                            }
                        }
                    }
                    LLSUB(PROF_UP);
                    // ---- down
                    const int dtop = dn0 > dn1 ? dn0 : dn1;
                    for (int d = dlmin + 1; d <= dtop; ++d) {
                        const bool nc = (nonchain >> d) & 1;
                        const V3 pdw = pp(Dw, nc), pdv = pp(Dv, nc);
                        if (dndep == d) {
                            const V3 tv = pdv + cross(pdw, r);
                            Dw = mul(Di, aug * pdw + un_tot) - mul(E, tv);
                            Dv = tv;
                        }
                    }
                    LLSUB(PROF_DOWN);
                };
                // the walk returns to the root (its Lambda answers the total) and one root -> leaves pass moves the links down to depth dlast
                // (all of them, or those the sweep reads: the links down to the env's deepest stop)
                auto walk_close = [&](int dlast, bool all) {
                    [[maybe_unused]] long long tclose = F::DIAGX && a.prof ? clock64() : 0;
                    const int i0 = ((int)__builtin_amdgcn_readlane(dep, cur0) << 4) | (M.side_depths[cur0] << 12);
                    const int i1 = ((int)__builtin_amdgcn_readlane(dep, 32 + cur1) << 4) | (M.side_depths[cur1] << 12);
                    const int slive = F::LIVEM ? livem : __builtin_amdgcn_readfirstlane((live0 ? 1 : 0) | (live1 ? 2 : 0));
                    // (F::VTAB: a walk closes after whole sweeps only - it stands on the env's last stop, bit 0 of anc; nothing goes down)
                    vk = 0;
                    [[maybe_unused]] const long long tmove = F::DIAGX && a.prof ? clock64() : 0;
                    walk_to(0, 0, i0, i1, (slive & 1) != 0, (slive & 2) != 0);
                    // (PROF_CLOSE_MOVE: the closing move - its descriptor, the way up to the root, the turn there.  walk_to has timed itself into
                    // the counters of the moves: taken out of `up` again, so that a counter of walk_to's own - one more captured variable,
                    // which moves the register allocation of every kernel - is not needed; `down` keeps the closing move's test of its
                    // empty range, a few cycles per substep)
                    if (F::DIAGX && a.prof) {
                        const long long tdone = clock64();
                        LLADD(PROF_UP, tmove - tdone);
                    }
                    LLSUBX(PROF_CLOSE_MOVE, tclose);
                    long long tsub = DIAG && a.prof ? clock64() : 0;
                    V3 ddw{0.f, 0.f, 0.f}, ddv{0.f, 0.f, 0.f};
                    if (lb == 0) {
                        ddw = Dw;
                        ddv = Dv;
                        w = w + ddw;
                        xd = xd + ddv;
                    }
                    for (int d = 1; d <= dlast; ++d) {
                        const bool nc = (nonchain >> d) & 1;
                        const V3 pdw = pp(ddw, nc), pdv = pp(ddv, nc);
                        if (dep == d && (all || insweep)) {
                            const V3 av = pdv + cross(pdw, r);
                            ddw = mul(Di, aug * pdw + un_tot) - mul(E, av);
                            ddv = av;
                            w = w + ddw;
                            xd = xd + ddv;
                        }
                    }
                    LLSUBX_OR(PROF_CLOSE_PASS, PROF_DOWN);  // (the root -> leaves pass of a closing walk; it was counted with the ways down before)
                };
                // ---- ball x ground: a stop of its own after the last link - the last rows of a sweep (point at -R z of the centre; rows
                // n = z, t1 = x, t2 = y); returns whether any lane's rows changed something
                auto ball_ground_rows = [&](int done) -> int {
                    bool bmoved = false;
                    if (ballground && !((done >> half) & 1)) {
                        V3 bv{bl[BL_VEL], bl[BL_VEL + 1], bl[BL_VEL + 2]}, bw{bl[BL_ANG], bl[BL_ANG + 1], bl[BL_ANG + 2]};
                        const V3 rb{0.f, 0.f, -BP.radius};
                        float lamn = bl[BL_GLAM];
                        const float gbias = TGS ? fminf(rowbias(bl[BL_GGAP]), bl[BL_GREST]) : bl[BL_GBIAS];
#pragma unroll
                        for (int ax = 0; ax < 3; ++ax) {
                            const V3 dir = ax == 0 ? V3{0.f, 0.f, 1.f} : (ax == 1 ? V3{1.f, 0.f, 0.f} : V3{0.f, 1.f, 0.f});
                            const V3 jb = cross(rb, dir);
                            const float wii = BP.inv_mass + BP.inv_inertia * dot(jb, jb);
                            const float rel = dot(dir, bv) + dot(jb, bw) + (ax == 0 ? gbias : 0.f);
                            const float old = bl[BL_GLAM + ax];
                            float nl = old - rel * __builtin_amdgcn_rcpf(wii);
                            if (ax == 0) nl = fmaxf(nl, 0.f);
                            else { const float lim = BP.fric_ground * lamn; nl = fminf(fmaxf(nl, -lim), lim); }
                            const float dl = nl - old;
                            bl[BL_GLAM + ax] = nl;
                            if (ax == 0) lamn = nl;
                            bv = bv + (dl * BP.inv_mass) * dir;
                            bw = bw + (dl * BP.inv_inertia) * jb;
                            bmoved = bmoved || dl != 0.f;
                        }
                        bl[BL_VEL] = bv.x; bl[BL_VEL + 1] = bv.y; bl[BL_VEL + 2] = bv.z;
                        bl[BL_ANG] = bw.x; bl[BL_ANG + 1] = bw.y; bl[BL_ANG + 2] = bw.z;
                    }
                    const unsigned long long bm = __ballot(bmoved);
                    return ((unsigned)bm != 0u ? 1 : 0) | ((unsigned)(bm >> 32) != 0u ? 2 : 0);
                };
                // an env whose whole sweep changed nothing has reached the fixed point of its rows: it takes no part in the remaining sweeps,
                // whatever the env it shares the wave with still does.  (Its later sweeps change nothing: the same moves re-derive the same
                // velocities - the block updates they would take are saved.)
                int done = 0;
                if (F::DIAGX && a.prof) { long long tsub = tprev; LLSUBX(PROF_SWEEP_SETUP, tsub); }  // (the sweep's set-up since the end of the Lambda phase - moves, visit table)
                for (int it = 0; it < P.n_iter; ++it) {
                    unsigned t0 = (done & 1) ? 0u : v0, t1 = (done & 2) ? 0u : v1;
                    int moved = 0;  // bit h: env h changed something in this sweep (wave-uniform)
                    if (TGS && it > 0) {
                        // gaps advance with the normal velocity the points have after the previous sweep (touched links are current)
#pragma unroll
                        for (int c = 0; c < 4; ++c) { const V3 rc = CS.cr(c); CS.set_bias(c, CS.bias(c) + hs * (rc.y * w.x - rc.x * w.y + xd.z)); }
                        tgs_irem = 1.f / (h - (float)it * hs);
                        if (LIMITS && any64(limact)) {
                            // ... a limit row's with the joint rate of its DOF (the walk was closed down to the deepest stop: joint and parent are current)
                            const V3 pw = pp(w, true);
                            if (limact) {
                                const V3 om = mulT(q2mat(Q4{park[PARK_Q * 64], park[(PARK_Q + 1) * 64], park[(PARK_Q + 2) * 64], park[(PARK_Q + 3) * 64]}), w - pw);
                                lbias[0] += hs * lsgn[0] * om.x; lbias[1] += hs * lsgn[1] * om.y; lbias[2] += hs * lsgn[2] * om.z;
                            }
                        }
                        if (BALL) {
                            // ... the ball's rows with the relative normal velocity of the two contact points (the ball's own point is at -R n of its
                            // centre: its spin does not move it along n)
                            const V3 bv{bl[BL_VEL], bl[BL_VEL + 1], bl[BL_VEL + 2]};
                            if (ballground) bl[BL_GGAP] = bl[BL_GGAP] + hs * bv.z;
                            if (ballhit) {
#pragma unroll 1
                                for (int j = 0; j < NBREC; ++j) {
                                    lds_vfloat* rk = bl + BL_RK + 16 * j;
                                    if (rk[RK_A] == 0.f || !ball_rec_mine(j)) continue;
                                    const V3 n{rk[RK_N], rk[RK_N + 1], rk[RK_N + 2]}, rl{rk[RK_RL], rk[RK_RL + 1], rk[RK_RL + 2]};
                                    rk[RK_GAP] = rk[RK_GAP] + hs * dot(bv - xd - cross(w, rl), n);
                                }
                            }
                        }
                    }
                    // F::VTAB: a counted loop over the visits of the envs that still iterate
                    const int nvis = F::VTAB ? __builtin_amdgcn_readfirstlane(max((done & 1) ? 0 : nvis0, (done & 2) ? 0 : nvis1)) : 0;
                    if (F::VTAB && ((done >> half) & 1)) {  // (done only grows: the env's visits are struck out once)
                        vis = 0;
                        mystop = -1;
                    }
                    // one visit: the k-th stop of both envs (F::VTAB; the earlier form takes the stops off t0, t1 and does not count)
                    [[maybe_unused]] int k = 0;
                    while (F::VTAB ? k < nvis : (t0 | t1) != 0u) {
                        const int b0 = !F::VTAB && t0 ? __ffs(t0) - 1 : -1, b1 = !F::VTAB && t1 ? __ffs(t1) - 1 : -1;  // (F::VTAB: not needed)
                        if constexpr (!F::VTAB) {
                            t0 &= ~(b0 < 0 ? 0u : 1u << b0);
                            t1 &= ~(b1 < 0 ? 0u : 1u << b1);
                        }
                        LLCOUNT(PROF_UPDATES, 1ull);
                        [[maybe_unused]] long long thead = F::DIAGX && a.prof ? clock64() : 0;  // (PROF_VISIT_ENDS: head and tail of a visit - what neither the move nor the rows time)
                        int came_down = 0;  // LIMITS: bit h = env h has just come DOWN to its link (the lowest common ancestor of the move lies above it)
                        [[maybe_unused]] int npts = 0;  // F::ROWCNT: the larger of the two stops' numbers of points (0 for an env that rests or is done)
                        // (readfirstlane: wave-uniform by construction, and the compiler must know it - the level loops are scalar loops)
                        if constexpr (F::VTAB) {
                            // (bit 24 of a visit word: the env has a stop here and more than one stop - it moves if it is live)
                            const int vi0 = __builtin_amdgcn_readlane(vis, k), vi1 = __builtin_amdgcn_readlane(vis, 32 + k);
                            if constexpr (F::ROWCNT) npts = max((vi0 >> 25) & 7, (vi1 >> 25) & 7);
                            const int smv = F::LIVEM ? livem & (((vi0 >> 24) & 1) | ((vi1 >> 23) & 2))
                                                  : __builtin_amdgcn_readfirstlane((live0 ? (vi0 >> 24) & 1 : 0) | (live1 ? (vi1 >> 23) & 2 : 0));
                            if (smv) {
                                vk = k;
                                LLSUBX(PROF_VISIT_ENDS, thead);
                                walk_to(0, 0, vi0, vi1, (smv & 1) != 0, (smv & 2) != 0);
                                if (F::DIAGX && a.prof) thead = clock64();
                            }
                        } else {
                            const int smv = __builtin_amdgcn_readfirstlane(((live0 && b0 >= 0 && b0 != cur0) ? 1 : 0) | ((live1 && b1 >= 0 && b1 != cur1) ? 2 : 0));
                            if (smv) {
                                const int i0 = __builtin_amdgcn_readlane(minfo, b0 < 0 ? 0 : b0), i1 = __builtin_amdgcn_readlane(minfo, 32 + (b1 < 0 ? 0 : b1));
                                LLSUBX(PROF_VISIT_ENDS, thead);
                                walk_to(b0 < 0 ? 0 : b0, b1 < 0 ? 0 : b1, i0, i1, (smv & 1) != 0, (smv & 2) != 0);
                                if (F::DIAGX && a.prof) thead = clock64();
                                if (LIMITS) came_down = smv & (((i0 & 15) < ((i0 >> 8) & 15) ? 1 : 0) | ((i1 & 15) < ((i1 >> 8) & 15) ? 2 : 0));
                            }
                            if (b0 >= 0) cur0 = b0;
                            if (b1 >= 0) cur1 = b1;
                        }
                        const int bsel = half ? b1 : b0;
                        if constexpr (LIMITS) {
                            // ---- the limit rows of the joint the walk stands on (before the contact rows of its link).  A limit impulse is a
                            // joint-space impulse: it joins the link's collected impulse, and its reaction, a pure torque, what the link hands up.
                            const bool hl0 = b0 >= 0 && ((lm0 >> b0) & 1u), hl1 = b1 >= 0 && ((lm1 >> b1) & 1u);
                            if (hl0 || hl1) {
                                // one joint up (the parent turns), one joint down again: the move that makes the joint and its parent current
                                const int m0i = __builtin_amdgcn_readlane(minfo, b0 < 0 ? 0 : b0), m1i = __builtin_amdgcn_readlane(minfo, 32 + (b1 < 0 ? 0 : b1));
                                const int d0 = (m0i >> 8) & 15, d1 = (m1i >> 8) & 15;
                                const int j0i = (d0 - 1) | (d0 << 4) | (d0 << 8) | ((((m0i >> 28) & 1) << d0) << 12);
                                const int j1i = (d1 - 1) | (d1 << 4) | (d1 << 8) | ((((m1i >> 28) & 1) << d1) << 12);
                                // the rows read the PARENT's velocity as well.  It is current when the walk came down through it; when the walk
                                // turned at this very link (or never left it) the parent still lacks what this link's subtree has collected since
                                // - this move hands exactly that up.
                                const int spre = __builtin_amdgcn_readfirstlane((((live0 && hl0) ? 1 : 0) | ((live1 && hl1) ? 2 : 0)) & ~came_down);
                                if (spre) walk_to(b0 < 0 ? 0 : b0, b1 < 0 ? 0 : b1, j0i, j1i, (spre & 1) != 0, (spre & 2) != 0);
                                const V3 wc = w + Dw;
                                const V3 pw = pp(wc, true);
                                bool lchg = false;
                                if (valid && lb == bsel && (half ? hl1 : hl0)) {
                                    const M3 R = q2mat(Q4{park[PARK_Q * 64], park[(PARK_Q + 1) * 64], park[(PARK_Q + 2) * 64], park[(PARK_Q + 3) * 64]});
                                    const V3 om0 = mulT(R, wc - pw);  // joint rate, body axes
                                    float om[3] = {om0.x, om0.y, om0.z}, tq[3] = {0.f, 0.f, 0.f};
#pragma unroll
                                    for (int i = 0; i < 3; ++i) {
                                        const V3 kc = i == 0 ? V3{Kd.xx, Kd.xy, Kd.xz} : (i == 1 ? V3{Kd.xy, Kd.yy, Kd.yz} : V3{Kd.xz, Kd.yz, Kd.zz});
                                        const float kii = i == 0 ? kc.x : (i == 1 ? kc.y : kc.z);
                                        const float rel = lsgn[i] * om[i] + rowbias(lbias[i]);
                                        const float nl = fmaxf(llam[i] - rel * __builtin_amdgcn_rcpf(kii), 0.f);
                                        const float dl = lsgn[i] != 0.f ? nl - llam[i] : 0.f;
                                        llam[i] += dl;
                                        const float sdl = lsgn[i] * dl;
                                        tq[i] = sdl;
                                        om[0] += kc.x * sdl; om[1] += kc.y * sdl; om[2] += kc.z * sdl;
                                    }
                                    const V3 jt = mul(R, V3{tq[0], tq[1], tq[2]});
                                    un_new = un_new + jt;
                                    un_tot = un_tot + jt;
                                    jt_new = jt_new + jt;
                                    lchg = tq[0] != 0.f || tq[1] != 0.f || tq[2] != 0.f;
                                }
                                const unsigned long long lc = __ballot(lchg);
                                const int sl = __builtin_amdgcn_readfirstlane(((unsigned)lc != 0u ? 1 : 0) | ((unsigned)(lc >> 32) != 0u ? 2 : 0));
                                if (sl) {
                                    // the joint answers, and so does everything above it: one joint up (the parent turns), one joint down again
                                    live0 = live0 || (sl & 1);
                                    live1 = live1 || (sl & 2);
                                    moved |= sl;
                                    // (deferring this move to the env's next one - it goes up through the parent anyway, or can be widened by a level when it
                                    // goes down into the joint's subtree - was built and measured in round 6: +0.4 %, inside the noise, because most limit
                                    // stops of the racket arm carry contact rows too and need the link current at once; not kept)
                                    walk_to(b0 < 0 ? 0 : b0, b1 < 0 ? 0 : b1, j0i, j1i, (sl & 1) != 0, (sl & 2) != 0);
                                }
                            }
                        }
                        // ---- the rows of the link the walk stands on
                        LLSUBX(PROF_VISIT_ENDS, thead);
                        long long tsub = DIAG && a.prof ? clock64() : 0;
                        const bool me = F::VTAB ? mystop == k : valid && lb == bsel && (!LIMITS || (((half ? m1 : m0) >> (bsel < 0 ? 0 : bsel)) & 1u));
                        V3 gn{0.f, 0.f, 0.f}, gf{0.f, 0.f, 0.f};  // what these rows add to the link's impulse
                        if (me) {
                            V3 wl = w + Dw, xl = xd + Dv;
                            // all four records of the link at once (one LDS round trip instead of one per point; unused slots hold zeros)
                            V3 rr4[4], lam4[4];
                            float bias4[4];
#pragma unroll
                            for (int c = 0; c < 4; ++c) { rr4[c] = CS.cr(c); lam4[c] = CS.lam(c); bias4[c] = CS.bias(c); }
                            V3 ws0{0.f, 0.f, 0.f}, xs0{0.f, 0.f, 0.f};  // VFRIC: v* of the link
                            if constexpr (VFRIC) { ws0 = park_get3(PARK_W0); xs0 = park_get3(PARK_XD0); }
                            if constexpr (F::ROWX) {
                                // An unrolled loop without `break` / `continue`.  F::ROWCNT: npts is a scalar, "c < npts" for c = 0 .. 3 are four
                                // scalar compares, and since c >= npts implies c + 1 >= npts the compiler threads them into four nested blocks.
                                // Without the table: four votes (uniform over the at most two touched links solved here).
                                // (The same body as an inlined lambda per point, called from four nested ifs, is NOT the same arithmetic: a
                                // function is optimised on its own first, the rows' loop is unrolled there, and the relaxed-math flags then
                                // merge the normal row's relative velocity with the one of the `act` test and fold `ln + (nl - ln)`.)
#pragma unroll
                                for (int c = 0; c < 4; ++c) {
                                    if (F::ROWCNT ? c < npts : any64(c < cnt)) {
                                        const V3 rr = rr4[c];
                                        V3 t1{1.f, 0.f, 0.f}, t2{0.f, 1.f, 0.f};
                                        if constexpr (VFRIC) vfric_frame(ws0, xs0, rr, t1, t2);
                                        const V3 lam0 = lam4[c];
                                        float ln = lam0.x, l1 = lam0.y, l2 = lam0.z;
                                        // a point without normal impulse (hence without friction impulses: they are clamped to mu x normal)
                                        // that is separating stays as it is: its three rows would change nothing.  The rows run under EXEC for
                                        // the lanes whose point is active and write in place; a lane whose point is not active, or does not
                                        // exist, executes nothing, so an env's numbers do not depend on what its wave partner does by construction
                                        // (`&`, not `&&`: one region per point; with `&&` the compiler nests a region for c < cnt around it)
                                        const float bias_c = rowbias(bias4[c]);
                                        const bool act = bool((c < cnt) & !((ln == 0.f) & (rr.y * wl.x - rr.x * wl.y + xl.z + bias_c >= 0.f)));
                                        if (act) {
#pragma unroll
                                            for (int ax = 0; ax < 3; ++ax) {
                                                const V3 dir = ax == 0 ? V3{0.f, 0.f, 1.f} : (VFRIC ? (ax == 1 ? t1 : t2) : (ax == 1 ? V3{1.f, 0.f, 0.f} : V3{0.f, 1.f, 0.f}));
                                                const V3 jn = cross(rr, dir);
                                                const V3 yw = mul(Lam.A, jn) + mul(Lam.B, dir);
                                                const V3 yv = V3{dot(col(Lam.B, 0), jn), dot(col(Lam.B, 1), jn), dot(col(Lam.B, 2), jn)} + mul(Lam.C, dir);
                                                const float wii = dot(jn, yw) + dot(dir, yv);
                                                const float rel = dot(jn, wl) + dot(dir, xl) + (ax == 0 ? bias_c : 0.f);
                                                const float old = ax == 0 ? ln : (ax == 1 ? l1 : l2);
                                                float nl = old - rel * __builtin_amdgcn_rcpf(wii);
                                                if (ax == 0) nl = fmaxf(nl, 0.f);
                                                else { const float lim = P.mu * ln; nl = fminf(fmaxf(nl, -lim), lim); }
                                                float dl = nl - old;
                                                // (opaque: without the select of the earlier form the relaxed-math flags fold `old + (nl - old)`
                                                // below to `nl`, which rounds differently)
                                                asm("" : "+v"(dl));
                                                if (ax == 0) ln += dl; else if (ax == 1) l1 += dl; else l2 += dl;
                                                wl = wl + dl * yw;
                                                xl = xl + dl * yv;
                                                gn = gn + dl * jn;
                                                gf = gf + dl * dir;
                                            }
                                            CS.set_lam(c, V3{ln, l1, l2});
                                        }
                                    }
                                }
                            } else {
#pragma unroll
                            for (int c = 0; c < 4; ++c) {
                                const bool active = c < cnt;
                                if (!any64(active)) break;  // uniform over the (at most two) touched links solved here
                                const V3 rr = rr4[c];
                                V3 t1{1.f, 0.f, 0.f}, t2{0.f, 1.f, 0.f};
                                if constexpr (VFRIC) vfric_frame(ws0, xs0, rr, t1, t2);
                                const V3 lam0 = lam4[c];
                                float ln = lam0.x, l1 = lam0.y, l2 = lam0.z;
                                // a point without normal impulse (hence without friction impulses: they are clamped to mu x normal)
                                // that is separating stays as it is: its three rows would change nothing
                                // (masked per lane as well, so that an env's numbers do not depend on what its wave partner does)
                                const float bias_c = rowbias(bias4[c]);
                                const bool act = active && !(ln == 0.f && rr.y * wl.x - rr.x * wl.y + xl.z + bias_c >= 0.f);
                                if (!any64(act)) continue;
#pragma unroll
                                for (int ax = 0; ax < 3; ++ax) {
                                    const V3 dir = ax == 0 ? V3{0.f, 0.f, 1.f} : (VFRIC ? (ax == 1 ? t1 : t2) : (ax == 1 ? V3{1.f, 0.f, 0.f} : V3{0.f, 1.f, 0.f}));
                                    const V3 jn = cross(rr, dir);
                                    const V3 yw = mul(Lam.A, jn) + mul(Lam.B, dir);
                                    const V3 yv = V3{dot(col(Lam.B, 0), jn), dot(col(Lam.B, 1), jn), dot(col(Lam.B, 2), jn)} + mul(Lam.C, dir);
                                    const float wii = dot(jn, yw) + dot(dir, yv);
                                    const float rel = dot(jn, wl) + dot(dir, xl) + (ax == 0 ? bias_c : 0.f);
                                    const float old = ax == 0 ? ln : (ax == 1 ? l1 : l2);
                                    float nl = old - rel * __builtin_amdgcn_rcpf(wii);
                                    if (ax == 0) nl = fmaxf(nl, 0.f);
                                    else { const float lim = P.mu * ln; nl = fminf(fmaxf(nl, -lim), lim); }
                                    const float dl = act ? nl - old : 0.f;
                                    if (ax == 0) ln += dl; else if (ax == 1) l1 += dl; else l2 += dl;
                                    wl = wl + dl * yw;
                                    xl = xl + dl * yv;
                                    gn = gn + dl * jn;
                                    gf = gf + dl * dir;
                                }
                                CS.set_lam(c, V3{ln, l1, l2});
                            }
                            }
                            if (BALL && ballhit) {
                                // ---- ball x racket points: two-body rows (ball point velocity minus racket point velocity); the ball side is
                                // a free sphere (1/m, 1/I), the link side goes through Lambda_b like every row of this block
                                V3 bv{bl[BL_VEL], bl[BL_VEL + 1], bl[BL_VEL + 2]}, bw{bl[BL_ANG], bl[BL_ANG + 1], bl[BL_ANG + 2]};
#pragma unroll 1
                                for (int j = 0; j < NBREC; ++j) {
                                    lds_vfloat* rk = bl + BL_RK + 16 * j;
                                    if (rk[RK_A] == 0.f || !ball_rec_mine(j)) continue;
                                    const V3 n{rk[RK_N], rk[RK_N + 1], rk[RK_N + 2]}, rl{rk[RK_RL], rk[RK_RL + 1], rk[RK_RL + 2]};
                                    V3 t1v, t2v;
                                    ball_dirs(n, t1v, t2v);
                                    const V3 rb = -BP.radius * n;
                                    float lamn = rk[RK_LAM];
                                    const float rkbias = TGS ? fminf(rowbias(rk[RK_GAP]), rk[RK_REST]) : rk[RK_BIAS];
#pragma unroll 1
                                    for (int ax = 0; ax < 3; ++ax) {
                                        const V3 dir = ax == 0 ? n : (ax == 1 ? t1v : t2v);
                                        const V3 jn = cross(rl, dir), jb = cross(rb, dir);
                                        const V3 yw = mul(Lam.A, jn) + mul(Lam.B, dir);
                                        const V3 yv = V3{dot(col(Lam.B, 0), jn), dot(col(Lam.B, 1), jn), dot(col(Lam.B, 2), jn)} + mul(Lam.C, dir);
                                        const float wii = dot(jn, yw) + dot(dir, yv) + BP.inv_mass + BP.inv_inertia * dot(jb, jb);
                                        const float rel = dot(dir, bv) + dot(jb, bw) - dot(jn, wl) - dot(dir, xl) + (ax == 0 ? rkbias : 0.f);
                                        const float old = rk[RK_LAM + ax];
                                        float nl = old - rel * __builtin_amdgcn_rcpf(wii);
                                        if (ax == 0) nl = fmaxf(nl, 0.f);
                                        else { const float lim = (j < 2 ? BP.fric_racket : BP.fric_body) * lamn; nl = fminf(fmaxf(nl, -lim), lim); }
                                        const float dl = nl - old;
                                        rk[RK_LAM + ax] = nl;
                                        if (ax == 0) lamn = nl;
                                        bv = bv + (dl * BP.inv_mass) * dir;      // +impulse on the ball
                                        bw = bw + (dl * BP.inv_inertia) * jb;
                                        wl = wl - dl * yw;                        // -impulse on the racket's link
                                        xl = xl - dl * yv;
                                        gn = gn - dl * jn;
                                        gf = gf - dl * dir;
                                    }
                                }
                                bl[BL_VEL] = bv.x; bl[BL_VEL + 1] = bv.y; bl[BL_VEL + 2] = bv.z;
                                bl[BL_ANG] = bw.x; bl[BL_ANG + 1] = bw.y; bl[BL_ANG + 2] = bw.z;
                            }
                            Dw = wl - w;
                            Dv = xl - xd;
                            un_tot = un_tot + gn;
                            un_new = un_new + gn;
                            uf_new = uf_new + gf;
                        }
                        LLSUBX(PROF_ROWS, tsub);
                        const unsigned long long chg = __ballot(gn.x != 0.f || gn.y != 0.f || gn.z != 0.f || gf.x != 0.f || gf.y != 0.f || gf.z != 0.f);
                        if constexpr (F::LIVEM) {
                            // (the same ballot, its halves as two opaque scalars: `(unsigned)(chg >> 32) != 0` otherwise becomes a 64-bit
                            // "greater than", which the scalar unit does not have, and `live` a pair of lane masks that every visit turns
                            // into a scalar through a VGPR again)
                            int clo = (int)(unsigned)chg, chi = (int)(unsigned)(chg >> 32);
                            asm("" : "+s"(clo), "+s"(chi));
                            const int cb = (clo != 0 ? 1 : 0) | (chi != 0 ? 2 : 0);
                            livem |= cb;
                            moved |= cb;
                        } else {
                            live0 = live0 || (unsigned)chg != 0u;
                            live1 = live1 || (unsigned)(chg >> 32) != 0u;
                            moved |= ((unsigned)chg != 0u ? 1 : 0) | ((unsigned)(chg >> 32) != 0u ? 2 : 0);
                        }
                        if (DIAG && a.prof && !chg && LLSAMPLED) atomicAdd((unsigned long long*)&a.prof[PROF_NULL_UPDATES], 1ull);
                        LLSUBX_OR(PROF_VISIT_ENDS, PROF_ROWS);  // (the tail: the ballot of the change, live, moved)
                        if constexpr (F::VTAB) ++k;
                    }
                    if (BALL) moved |= ball_ground_rows(done);
                    if (TGS && (live0 || live1)) {
                        walk_close(dneed, false);  // (the links below catch up once, after the last iteration)
                        un_tot = un_new = uf_new = Dw = Dv = V3{0.f, 0.f, 0.f};
                        live0 = live1 = false;
                    }
                    if (!TGS) {  // (PGS: fixed biases - a sweep without any change would be repeated by the remaining ones)
                        done |= ~moved & 3;
                        if (done == 3) break;
                    }
                }
                if (!TGS && (F::LIVEM ? livem != 0 : (live0 || live1))) walk_close(maxd, true);
                // links below the deepest touched one: one catch-up pass with the accumulated motion of their parents
                // (PGS: the walk moves every link when it closes)
                V3 accw = w - park_get3(PARK_W0), accv = xd - park_get3(PARK_XD0);
                for (int d = dmin + 1; d <= (TGS ? maxd : 0); ++d) {
                    const bool nc = (nonchain >> d) & 1;
                    V3 pdw = pp(accw, nc), pdv = pp(accv, nc);
                    if (dep == d && !insweep) {
                        V3 av = pdv + cross(pdw, r);
                        accw = mul(Di, aug * pdw) - mul(E, av);
                        accv = av;
                        w = w + accw;
                        xd = xd + accv;
                    }
                }
            }
        }

        LLPH(PROF_SWEEP);
        V3 cimp_v{0.f, 0.f, 0.f};  // VFRIC: net contact impulse of this link's ground points, world axes (v* is about to leave its slots)
        if constexpr (VFRIC && CONTACT) {
            const V3 ws0 = park_get3(PARK_W0), xs0 = park_get3(PARK_XD0);
#pragma unroll
            for (int c = 0; c < 4; ++c)
                if (c < cnt) {
                    V3 t1, t2;
                    vfric_frame(ws0, xs0, CS.cr(c), t1, t2);
                    const V3 lc = CS.lam(c);
                    cimp_v = cimp_v + V3{lc.y * t1.x + lc.z * t2.x, lc.y * t1.y + lc.z * t2.y, lc.x};
                }
        }
        q = Q4{park[PARK_Q * 64], park[(PARK_Q + 1) * 64], park[(PARK_Q + 2) * 64], park[(PARK_Q + 3) * 64]};
        x = park_get3(PARK_X);
        // ================================================================ velocities -> generalized, damping, clamp, integrate
        const float sc = 1.f / (1.f + h * P.ang_damp);
        const float wmax = P.max_ang_vel;
        {
            Q4 pq = pp(q, true);
            V3 pw = pp(w, true);
            if (b != 0) {
                V3 wn = mulT(q2mat(q), w - pw);               // joint rate, body axes (undamped)
                Q4 jold = qnormalize(qmul(qconj(pq), q));  // joint quaternion of the old configuration
                if (last && valid && live_env && !frozen) {  // joint drive torque actually applied over the substep (implicit form)
                    const float kp = S->kp[b], kd = S->kd[b];
                    V3 tf = kp * (park_get3(PARK_TAR) - quat_to_expmap_stable(jold) - h * wn) - kd * wn;
                    int bh = b;
                    asm volatile("" : "+v"(bh));
                    float* of = a.x_dof_force + env_here() * NDOF + 3 * (bh - 1);
                    of[0] = tf.x; of[1] = tf.y; of[2] = tf.z;
                }
                wn = sc * wn;
                float n2 = dot(wn, wn);
                if (n2 > wmax * wmax) wn = (wmax * rsqrtf(n2)) * wn;
                wt = wn;
                jq = qnormalize(qmul(jold, rotvec_to_quat(h * wn)));  // body-frame rate: right multiply
            } else {
                V3 w0 = sc * w;
                float n2 = dot(w0, w0);
                if (n2 > wmax * wmax) w0 = (wmax * rsqrtf(n2)) * w0;
                w = w0;
                x = x + h * xd;
                q = qnormalize(qmul(rotvec_to_quat(h * w0), q));  // world-frame rate: left multiply
            }
        }
        if (BALL) {
            auto ball_rec_mine_out = [&](int j) -> bool { return j < 2 ? racket_lane : lb == (int)bl[BL_RK + 16 * j + RK_LINK]; };
            // force on the ball in this substep from the racket (sum over the two cylinders) and from the hull points, world axes
            V3 frk{0.f, 0.f, 0.f}, fbd{0.f, 0.f, 0.f}, fmine{0.f, 0.f, 0.f};  // from the racket, from all hulls, from this lane's hull
            {
                const float ih = PHYS_RCP(h);
#pragma unroll
                for (int j = 0; j < NBREC; ++j) {
                    lds_vfloat* rk = bl + BL_RK + 16 * j;
                    if (rk[RK_A] != 0.f && (ball_lane || (valid && ball_rec_mine_out(j)))) {
                        const V3 n{rk[RK_N], rk[RK_N + 1], rk[RK_N + 2]};
                        V3 t1, t2;
                        t1 = cross(n, V3{0.f, 0.f, 1.f});
                        if (dot(t1, t1) < 1e-6f) t1 = cross(n, V3{1.f, 0.f, 0.f});
                        t1 = rsqrtf(dot(t1, t1)) * t1;
                        t2 = cross(n, t1);
                        const V3 f = ih * (rk[RK_LAM] * n + rk[RK_LAM + 1] * t1 + rk[RK_LAM + 2] * t2);
                        if (j < 2) frk = frk + f;
                        else { fbd = fbd + f; if (!ball_lane) fmine = fmine + f; }
                    }
                }
            }
            if (ball_lane) {
                // ---- the ball: angular damping, clamp, integrate; outputs after the last substep of every simulate() call
                V3 bp{bl[BL_POS], bl[BL_POS + 1], bl[BL_POS + 2]}, bv{bl[BL_VEL], bl[BL_VEL + 1], bl[BL_VEL + 2]}, bw{bl[BL_ANG], bl[BL_ANG + 1], bl[BL_ANG + 2]};
                Q4 bq{bl[BL_QUAT], bl[BL_QUAT + 1], bl[BL_QUAT + 2], bl[BL_QUAT + 3]};
                bw = PHYS_RCP(1.f + h * BP.ang_damp) * bw;
                const float n2 = dot(bw, bw);
                if (n2 > BP.max_ang_vel * BP.max_ang_vel) bw = (BP.max_ang_vel * rsqrtf(n2)) * bw;
                bp = bp + h * bv;
                bq = qnormalize(qmul(rotvec_to_quat(h * bw), bq));
                bl[BL_POS] = bp.x; bl[BL_POS + 1] = bp.y; bl[BL_POS + 2] = bp.z;
                bl[BL_QUAT] = bq.x; bl[BL_QUAT + 1] = bq.y; bl[BL_QUAT + 2] = bq.z; bl[BL_QUAT + 3] = bq.w;
                bl[BL_ANG] = bw.x; bl[BL_ANG + 1] = bw.y; bl[BL_ANG + 2] = bw.z;
                // (output addresses from the opaque env index: formed from `e` they are loop invariants, hoisted in front of the substep
                // loop and kept - spilled - across all of it: 70 dwords of scratch per lane in the racket + ball kernels)
                const int64_t e = env_here();
                if (live_env && !replay && sub % BP.sub_per_sim == BP.sub_per_sim - 1) {
                    const int ks = sub / BP.sub_per_sim, nsim = nsub / BP.sub_per_sim;
                    float* o = BP.per_sim + (e * nsim + ks) * 13;
                    o[0] = bp.x; o[1] = bp.y; o[2] = bp.z; o[3] = bq.x; o[4] = bq.y; o[5] = bq.z; o[6] = bq.w;
                    o[7] = bv.x; o[8] = bv.y; o[9] = bv.z; o[10] = bw.x; o[11] = bw.y; o[12] = bw.z;
                    const bool hit = frk.x != 0.f || frk.y != 0.f || frk.z != 0.f;
                    BP.hit_per_sim[e * nsim + ks] = hit ? 1 : 0;
                    if (BP.has_hit) {  // the reference's poll of the net contact forces after every simulate() call (:773-779)
                        if (ks == 0) flag_st(&BP.has_hit_now[e], 0);
                        if (BP.poll_hits && hit && !flag_ld(&BP.has_hit[e])) { flag_st(&BP.has_hit[e], 1); flag_st(&BP.has_hit_now[e], 1); }
                    }
                }
                if (last && live_env) {
                    const float ih = PHYS_RCP(h);
                    float* oc = BP.contact + e * 6;
                    oc[0] = frk.x; oc[1] = frk.y; oc[2] = frk.z;
                    oc[3] = bl[BL_GA] != 0.f ? bl[BL_GLAM + 1] * ih : 0.f; oc[4] = bl[BL_GA] != 0.f ? bl[BL_GLAM + 2] * ih : 0.f;
                    oc[5] = bl[BL_GA] != 0.f ? bl[BL_GLAM] * ih : 0.f;
                    if (BP.body_contact) { float* ob = BP.body_contact + e * 3; ob[0] = fbd.x; ob[1] = fbd.y; ob[2] = fbd.z; }
                }
            }
            if ((last || (BP.contact_sum && sub % BP.sub_per_sim == BP.sub_per_sim - 1)) && valid && live_env && !frozen) {
                // the reaction on the touched link enters its net contact force below
                const V3 fr = mask(racket_lane, frk) + fmine;
                park[PARK_W0 * 64] = fr.x; park[(PARK_W0 + 1) * 64] = fr.y; park[(PARK_W0 + 2) * 64] = fr.z;
            }
        }
        // (racket + ball, opt-in: `_contact_forces_sum`, the net contact forces summed over the simulate() calls of a control step,
        // humanoid_smpl_im_mvae.py:781 - what refresh_net_contact_force_tensor shows after EVERY call is needed then, not only after the last)
        // One slot per simulate() call (`contact_part`, engine-owned), written by whoever runs the call's last substep - a replaying job
        // included: the same bits whoever writes them, so the order in which a pair's jobs run cannot matter - and added up by the job of the
        // env's LAST substep, which either waited for the jobs before it (their stores were drained in front of the progress word) or has
        // just replayed them itself.  (Round 3 accumulated in place, load + add + store per call: a job that ran ahead of a late predecessor
        // added onto a stale value, and the predecessor's own store then dropped what had been added.)
        const bool sum_now = BALL && BP.contact_sum && sub % BP.sub_per_sim == BP.sub_per_sim - 1;
        if ((last || sum_now) && valid && live_env && !frozen) {
            // net contact force per body = sum of impulses / h  (refresh_net_contact_force_tensor)
            V3 cforce{0.f, 0.f, 0.f};
            if (CONTACT) {
                const float ih = 1.f / h;
                if constexpr (VFRIC) cforce = ih * cimp_v;
                else {
#pragma unroll
                    for (int c = 0; c < 4; ++c)
                        if (c < cnt) { const V3 lc = CS.lam(c); cforce.z += lc.x * ih; cforce.x += lc.y * ih; cforce.y += lc.z * ih; }
                }
                if (BALL) cforce = cforce - park_get3(PARK_W0);
            }
            if (last) {
                float* oc = a.x_contact + (env_here() * NB + b) * 3;
                oc[0] = cforce.x; oc[1] = cforce.y; oc[2] = cforce.z;
            }
            if (sum_now) {  // (system-scope accesses: the calls of one step may run in different workgroups)
                const int ks = sub / BP.sub_per_sim, nsim = nsub / BP.sub_per_sim;
                float* const part = BP.contact_part + ((env_here() * nsim) * NB + b) * 3;
                if (!last) {
                    float* op = part + (int64_t)ks * NB * 3;
                    cstore(op, cforce.x); cstore(op + 1, cforce.y); cstore(op + 2, cforce.z);
                } else {
                    V3 tot{0.f, 0.f, 0.f};
                    for (int k = 0; k < ks; ++k) {
                        const float* ip = part + (int64_t)k * NB * 3;
                        tot = tot + V3{cload(ip), cload(ip + 1), cload(ip + 2)};
                    }
                    tot = tot + cforce;
                    float* os = BP.contact_sum + (env_here() * NB + b) * 3;
                    os[0] = tot.x; os[1] = tot.y; os[2] = tot.z;
                }
            }
        }
    }

    LLPH(PROF_INTEGRATE);
    // (opaque copy of the link index for everything after the substeps: indices and addresses formed from it are computed here instead of
    // being kept - spilled to scratch, which is HBM write traffic for every wave - since the prologue)
    int bo2 = b;
    asm volatile("" : "+v"(bo2));
    if (frozen && nsub > 0) {  // frozen env sharing a wave with a live one: it was carried along, its result is dropped
        if (b == 0) {
            q = Q4{st[SIDX(ST_ROOT_QUAT + 0)], st[SIDX(ST_ROOT_QUAT + 1)], st[SIDX(ST_ROOT_QUAT + 2)], st[SIDX(ST_ROOT_QUAT + 3)]};
            x = V3{st[SIDX(ST_ROOT_POS + 0)], st[SIDX(ST_ROOT_POS + 1)], st[SIDX(ST_ROOT_POS + 2)]};
            xd = V3{st[SIDX(ST_VEL + 0)], st[SIDX(ST_VEL + 1)], st[SIDX(ST_VEL + 2)]};
            w = V3{st[SIDX(ST_VEL + 3)], st[SIDX(ST_VEL + 4)], st[SIDX(ST_VEL + 5)]};
        } else {
            const int jb = ST_JQUAT + 4 * (bo2 - 1), vb = ST_VEL + 6 + 3 * (bo2 - 1);
            jq = Q4{st[SIDX(jb + 0)], st[SIDX(jb + 1)], st[SIDX(jb + 2)], st[SIDX(jb + 3)]};
            wt = V3{st[SIDX(vb + 0)], st[SIDX(vb + 1)], st[SIDX(vb + 2)]};
        }
    }
    // ==================================================================== final kinematics -> state, rigid-body state, dof_pos
    // (JOBS: only the job of the last substep produces the exposed tensors and the pairing keys; the others hand the state over)
    const V3 lpos{S->local_pos[bo2][0], S->local_pos[bo2][1], S->local_pos[bo2][2]};
    if (last_job) {
        V3 rr{0.f, 0.f, 0.f}, wrel{0.f, 0.f, 0.f};
        kin_jump(q, x, w, xd, jq, wt, lpos, rr, wrel);
    }
    if (DIAG && a.wave_times && lane == 0) {
        long long* wt = a.wave_times + ((int64_t)blockIdx.x * LL_WPB + (threadIdx.x >> 6)) * 4;
        wt[0] = wt0; wt[1] = wall_clock64(); wt[2] = ksum * 8 + kdep + 1024 * (long long)tsum + 1048576ll * tmaxs + 1073741824ll * key_pred;
        unsigned hw; asm volatile("s_getreg_b32 %0, hwreg(HW_REG_HW_ID)" : "=s"(hw)); wt[3] = hw;
    }
    if (a.pair_hist && last_job) {
        // ---- pairing key of this env (touched links, then the deepest of them: what the sweep's cost follows) into its load bin;
        // the workgroup that finishes last turns the histogram into the first rank of every bin, what the next launch's lookup starts from
        // links about to touch (bounding box within the contact offset of the ground after one more control step at the current
        // vertical speed) count like touched ones: a humanoid that falls goes from 2-4 to 12+ touched links within one control
        // step, and a heavy pair that is dispatched late because it was predicted light is the tail of the whole launch (+17 %)
        int ksoon = 0;
        {
            const float rz0 = 2.f * (q.x * q.z - q.w * q.y), rz1 = 2.f * (q.y * q.z + q.w * q.x), rz2 = 1.f - 2.f * (q.x * q.x + q.y * q.y);
            const float zl = x.z + rz0 * S->aabb_c[bo2][0] + rz1 * S->aabb_c[bo2][1] + rz2 * S->aabb_c[bo2][2] -
                             (fabsf(rz0) * S->aabb_e[bo2][0] + fabsf(rz1) * S->aabb_e[bo2][1] + fabsf(rz2) * S->aabb_e[bo2][2]);
            const unsigned long long nb2 = __ballot(valid && zl + fminf(xd.z, 0.f) * P.dt < P.contact_offset);
            ksoon = __popc(half ? (unsigned)(nb2 >> 32) : (unsigned)nb2);
        }
        if (lb == 0 && live_env) {
            int key = frozen ? 0 : (ksum > ksoon ? ksum : ksoon) * 8 + (kdep > 7 ? 7 : kdep);
            key = key > PAIR_BINS - 1 ? PAIR_BINS - 1 : key;
            const int pos = atomicAdd(&a.pair_hist[PAIR_BINS - 1 - key], 1);
            a.pair_key[e] = key;
            a.pair_pos[e] = pos;
            a.pl_list_next[(int64_t)(PAIR_BINS - 1 - key) * N + pos] = (int32_t)e;  // what the next launch looks its envs up in
        }
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");  // this wave's bin counts are in before its ticket is drawn
        int ticket = -1;
        if (lane == 0) ticket = atomicAdd(a.pair_done, 1);
        ticket = __builtin_amdgcn_readfirstlane(ticket);
        if (ticket == nblk * LL_WPB - 1) {
            int c[4], mine = 0;
#pragma unroll
            for (int k = 0; k < 4; ++k) { c[k] = __hip_atomic_load(&a.pair_hist[4 * lane + k], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); mine += c[k]; }
            int inc = mine;
            for (int o = 1; o < 64; o <<= 1) { const int u = __shfl_up(inc, o); if (lane >= o) inc += u; }
            int ex = inc - mine;
#pragma unroll
            for (int k = 0; k < 4; ++k) { a.pair_start[4 * lane + k] = ex; ex += c[k]; a.pair_hist[4 * lane + k] = 0; }
            if (lane == 0) *a.pair_done = 0;
        }
    }
    // the output addresses are formed here, from an index the compiler cannot trace back to the prologue: computed up front they were
    // kept across the whole kernel as spilled 64-bit pointers (36 B of scratch per lane = 9 MB of HBM traffic per launch)
    int64_t e_out = e;
    asm volatile("" : "+v"(e_out));
    {
    const int64_t e = e_out;
    if constexpr (JOBS) if (!last_job) {
        // ---- hand the state over to the job of the next substep: system-scope stores, drained, then the progress word of the pair
        {
            // Link b owns the adjacent chunks 2b, 2b + 1 (one 32-byte read per lane on the other side).  Written by their owner, every
            // store instruction would touch half of each 64-byte line (PMC WRITE_SIZE: +14 MB per launch of partial-line write-throughs);
            // instead lane l of an env writes chunk hand_link(12 k) + l in instruction k = 0, 1 - 24 adjacent chunks = six full lines -,
            // fetching the values from the lane that owns them (link 12 k + l / 2, its first or second chunk).
            const bool root = b == 0;
            const float A0 = root ? q.x : jq.x, A1 = root ? q.y : jq.y, A2 = root ? q.z : jq.z, A3 = root ? q.w : jq.w;
            const float B0 = root ? x.x : wt.x, B1 = root ? x.y : wt.y, B2 = root ? x.z : wt.z, B3 = root ? xd.x : 0.f;
            float* const ho = a.job_hand + ((int64_t)sjob * N + e) * HAND_FLOATS;
            const bool second = lb & 1;
#pragma unroll
            for (int k = 0; k < 2; ++k) {
                const int src = base + 12 * k + ((lb >> 1) < 12 ? (lb >> 1) : 0);
                const float a0 = pull(A0, src), a1 = pull(A1, src), a2 = pull(A2, src), a3 = pull(A3, src);
                const float b0 = pull(B0, src), b1 = pull(B1, src), b2 = pull(B2, src), b3 = pull(B3, src);
                if (valid && live_env) cstore4(ho + 4 * (hand_link(NB / 2 * k) + lb), second ? b0 : a0, second ? b1 : a1, second ? b2 : a2, second ? b3 : a3);
            }
            if (root && valid && live_env) {
                static_assert(HAND_FORCE_AT == 1, "the residual force rides behind w.z");
                cstore4(ho + 4 * HAND_ROOT_VEL, xd.y, xd.z, w.x, w.y);
                if (a.actions && jstart(sjob + 1) < a.p.hold_sub) {  // the next job still applies the residual wrench: it travels along
                    // (component by component in the argument lists, not through wrench_get: with a V3 in between, the register build's
                    // racket + ball kernels compile to other code)
                    const float* wp = wave_lds + base;
                    cstore4(ho + 4 * (HAND_ROOT_VEL + 1), w.z, wrench_at(wp, WRENCH_FORCE_LANE, 0), wrench_at(wp, WRENCH_FORCE_LANE, 1), wrench_at(wp, WRENCH_FORCE_LANE, 2));
                    cstore4(ho + 4 * HAND_TORQUE, wrench_at(wp, WRENCH_TORQUE_LANE, 0), wrench_at(wp, WRENCH_TORQUE_LANE, 1), wrench_at(wp, WRENCH_TORQUE_LANE, 2), 0.f);
                } else {
                    cstore4(ho + 4 * (HAND_ROOT_VEL + 1), w.z, 0.f, 0.f, 0.f);
                }
            }
        }
        if (BALL && ball_lane && live_env) {
            float* const ho = a.job_hand + ((int64_t)sjob * N + e) * HAND_FLOATS;
            // (written out: as an unrolled loop over the chunks the same stores move the block numbers of the rows' dispatch in the
            // register build's ball kernels, and their code with them)
            cstore4(ho + 4 * HAND_BALL, bl[BL_POS], bl[BL_POS + 1], bl[BL_POS + 2], bl[BL_QUAT]);
            cstore4(ho + 4 * (HAND_BALL + 1), bl[BL_QUAT + 1], bl[BL_QUAT + 2], bl[BL_QUAT + 3], bl[BL_VEL]);
            cstore4(ho + 4 * (HAND_BALL + 2), bl[BL_VEL + 1], bl[BL_VEL + 2], bl[BL_ANG], bl[BL_ANG + 1]);
            cstore4(ho + 4 * (HAND_BALL + 3), bl[BL_ANG + 2], bl[BL_F], bl[BL_F + 1], bl[BL_F + 2]);
        }
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");  // (inline asm: the compiler must not drop or move this drain)
        if (lane == 0) {
            int bid_here = bid;  // (the address of the progress word is formed here: kept from the prologue it is a spilled 64-bit pointer)
            asm volatile("" : "+s"(bid_here));
            // (max, not store: a job that is overtaken - its successor gave up waiting and has already handed over further - must not turn
            // the word back)
            __hip_atomic_fetch_max(a.job_progress + (bid_here * LL_WPB + (threadIdx.x >> 6)), a.job_epoch * (a.p.nsub + 1) + sjob + 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
        }
        timeline();
        return;
    }
    V3 qe{0.f, 0.f, 0.f};  // exposed dof position of this lane's joint
    if (valid && live_env) {
        if (b == 0) {
            st[SIDX(ST_ROOT_QUAT + 0)] = q.x; st[SIDX(ST_ROOT_QUAT + 1)] = q.y; st[SIDX(ST_ROOT_QUAT + 2)] = q.z; st[SIDX(ST_ROOT_QUAT + 3)] = q.w;
            st[SIDX(ST_ROOT_POS + 0)] = x.x; st[SIDX(ST_ROOT_POS + 1)] = x.y; st[SIDX(ST_ROOT_POS + 2)] = x.z;
            st[SIDX(ST_VEL + 0)] = xd.x; st[SIDX(ST_VEL + 1)] = xd.y; st[SIDX(ST_VEL + 2)] = xd.z;
            st[SIDX(ST_VEL + 3)] = w.x; st[SIDX(ST_VEL + 4)] = w.y; st[SIDX(ST_VEL + 5)] = w.z;
        } else {
            const int jb = ST_JQUAT + 4 * (bo2 - 1), vb = ST_VEL + 6 + 3 * (bo2 - 1);
            st[SIDX(jb + 0)] = jq.x; st[SIDX(jb + 1)] = jq.y; st[SIDX(jb + 2)] = jq.z; st[SIDX(jb + 3)] = jq.w;
            st[SIDX(vb + 0)] = wt.x; st[SIDX(vb + 1)] = wt.y; st[SIDX(vb + 2)] = wt.z;
            // exposed dof state: (exp-map position, joint rate) interleaved like gym's dof state tensor
            qe = quat_to_expmap_stable(jq);
            float* od = a.x_dof + (e * NDOF + 3 * (bo2 - 1)) * 2;
            od[0] = qe.x; od[1] = wt.x; od[2] = qe.y; od[3] = wt.y; od[4] = qe.z; od[5] = wt.z;
        }
        if (b == 0) {
            float* orr = a.x_root + e * 13;
            orr[0] = x.x; orr[1] = x.y; orr[2] = x.z;
            orr[3] = q.x; orr[4] = q.y; orr[5] = q.z; orr[6] = q.w;
            orr[7] = xd.x; orr[8] = xd.y; orr[9] = xd.z;
            orr[10] = w.x; orr[11] = w.y; orr[12] = w.z;
        }
    }
    if (BALL && live_env) {
        if (ball_lane) {
#pragma unroll
            for (int k = 0; k < 13; ++k) BP.state[e * 13 + k] = bl[k];
        }
        if (valid && racket_lane) {  // rigid body 24 of the reference's tensor: the racket frame, welded to this link
            ConstRacket* const RS = racket();
            const V3 off = mul(q2mat(q), V3{RS->racket_off[0], RS->racket_off[1], RS->racket_off[2]});
            const V3 rx = x + off, rv = xd + cross(w, off);
            float* o = BP.racket_state + e * 13;
            o[0] = rx.x; o[1] = rx.y; o[2] = rx.z; o[3] = q.x; o[4] = q.y; o[5] = q.z; o[6] = q.w;
            o[7] = rv.x; o[8] = rv.y; o[9] = rv.z; o[10] = w.x; o[11] = w.y; o[12] = w.z;
        }
    }
    // rigid-body state [24][13] of the env: a lane's row is 13 dwords at a 52-byte stride, which as 13 scalar stores per lane left the
    // L2 with partial lines from two XCDs' worth of neighbours (PMC WRITE_SIZE 1.7x the bytes).  The rows are staged through the
    // (now idle) LDS parking area and leave as 78 contiguous 16-byte stores per env: full lines.
    {
        float* const stage = wave_lds + LDS_STAGE + half * STAGE_FLOATS;
        if (valid) {
            float* o = stage + b * 13;
            o[0] = x.x; o[1] = x.y; o[2] = x.z;
            o[3] = q.x; o[4] = q.y; o[5] = q.z; o[6] = q.w;
            o[7] = xd.x; o[8] = xd.y; o[9] = xd.z;
            o[10] = w.x; o[11] = w.y; o[12] = w.z;
        }
        if (live_env) {
            const float4* src = (const float4*)stage;
            float4* dst = (float4*)(a.x_rb + e * NB * 13);
#pragma unroll
            for (int r = 0; r < 3; ++r) {
                const int j = lb + 32 * r;
                if (j < NB * 13 / 4) dst[j] = src[j];
            }
        }
    }
    if constexpr (JOBS && !DIAG) {
        // ---- post-physics fused in (v2p_env_step): the same functions, compiled with the same semantics, as env_post_kernel; lane = body
        // holds exactly the values the exposed tensors were just given.  The post-physics kernel cost a launch of its own right behind
        // the tail of this one (the heaviest env pairs finish last, on an almost empty GPU); here every pair does it as it finishes.
        if (a.post.on) {
            const PostArgs& Z = a.post;
            bool fl = false;
            int64_t mid = 0;
            float t_new = 0.f;
            strict::RewardPartial rp{0.f, 0.f, 0.f, 0.f};
            if (valid && live_env) {
                mid = Z.motion_id[e];
                t_new = Z.b.cur_time[e] + P.dt;  // _cur_ref_motion_times += dt
                rp = strict::post_body(Z.b, Z.t, P, mid, t_new, Z.cur, e, b, strict::V3{x.x, x.y, x.z}, strict::Q4{q.x, q.y, q.z, q.w}, strict::V3{xd.x, xd.y, xd.z},
                                       strict::V3{w.x, w.y, w.z}, strict::V3{qe.x, qe.y, qe.z}, strict::V3{wt.x, wt.y, wt.z}, fl, true);
            }
            // reward sums over the bodies, bodies ascending like env_post_kernel: the terms go through this lane's LDS column (the parking
            // area is idle by now; a wave's LDS accesses execute in order), lanes 0..3 of each env add one term each
            static_assert(REWARD_SLOTS == 4, "dof, vel, pos, rot");
            park[0] = rp.dof; park[64] = rp.vel; park[128] = rp.pos; park[192] = rp.rot;
            const unsigned long long fb = __ballot(fl);
            const bool fell = (half ? (unsigned)(fb >> 32) : (unsigned)fb) != 0u;
            float sk = 0.f;
            if (lb < REWARD_SLOTS) sk = strict::sum_bodies(wave_lds + LDS_PARK + lb * 64 + base);
            const float s4[4] = {pull(sk, base), pull(sk, base + 1), pull(sk, base + 2), pull(sk, base + 3)};
            if (lb == 0 && live_env) strict::post_env(Z.b, Z.t, P, mid, t_new, e, s4, fell);
        }
    }
    }
    if constexpr (JOBS) if (!mono) {
        // the step of this pair is complete: jobs of it that have not started yet must not (see the look at the word in the prologue)
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        if (lane == 0) {
            int bid_here = bid;
            asm volatile("" : "+s"(bid_here));
            __hip_atomic_fetch_max(a.job_progress + (bid_here * LL_WPB + (threadIdx.x >> 6)), a.job_epoch * (a.p.nsub + 1) + a.p.nsub, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
        }
    }
    timeline();
}
}  // namespace V2P_LL_NS

// run-time bools -> template arguments: f(std::bool_constant<b0>{}, std::bool_constant<b1>{}, ...)
template <typename Fn, typename... Cs>
static void with_bools(Fn&& f, Cs... cs) { f(cs...); }
template <typename Fn, typename... Rest>
static void with_bools(Fn&& f, bool b, Rest... rest) {
    if (b) with_bools(f, rest..., std::true_type{});
    else with_bools(f, rest..., std::false_type{});
}

int V2P_LL_LAUNCHER(v2p_env* env, hipStream_t s, float* actions, int* fused_post) {
    const unsigned blocks = (unsigned)((env->n + 2 * LL_WPB - 1) / (2 * LL_WPB));
    const dim3 block(64 * LL_WPB);
    const size_t lds = sizeof(float) * LDS_FLOATS_PER_WAVE * LL_WPB;
#if defined(V2P_LL_TIMELINE)
    const bool diag = env->prof != nullptr;
#else
    const bool diag = env->prof || env->wave_times;
#endif
    // everything of the launch that is the same in both builds: the refusals, the kernel's arguments, the job plan (physics_ll_host.hip)
    LlLaunch launch;
    const int rc = ll_launch_prepare(env, s, actions, fused_post, blocks, diag, launch);
    if (rc != V2P_OK) return rc;
    const PhysArgs& a = launch.a;
    const dim3 grid(launch.grid);
    // ONE instantiation whether the launch is cut into substep jobs or not (job_mono = every pair: whole control steps per workgroup,
    // nothing handed over): "substep jobs are invisible" holds by construction - two instantiations of the template are two
    // compilations, and under -fassociative-math nothing makes them round alike
    if (launch.diag) {
        // the diagnostic kernel is the one fixed instantiation: the headline configuration, whole control steps per workgroup
        hipLaunchKernelGGL((physics_ll_kernel<true, false, false, true, false, false, false>), grid, block, lds, s, a);
    } else {
        // The production instantiations, from the batch's configuration.  The rules, once:
        //   JOBS is always on, DIAG always off
        //   BALL or LIMITS imply CONTACT (their rows are solved in the contact sweep)
        //   TGS and VFRIC (friction_frame = velocity) exist only with CONTACT: a batch without contacts has no rows
        // which makes 2 (MULTI) x (1 without contacts + 16 with: TGS x BALL x LIMITS x VFRIC) = 34 kernels per build.
        const bool ball = env->ball != nullptr, lim = env->p.joint_limits != 0;
        const bool con = env->p.enable_contact != 0 || ball || lim;
        const bool multi = env->num_shapes > 1;  // per-env shapes: hull vertices come from the shape tables instead of the LDS copy
        const bool tgs = env->p.solver_type == 1 && con;
        const bool vfric = env->p.friction_frame == 1 && env->p.enable_contact != 0;
        with_bools([&](auto C, auto M, auto T, auto B, auto L, auto V) {
            if constexpr (C() || !(T() || B() || L() || V()))
                hipLaunchKernelGGL((physics_ll_kernel<C(), M(), T(), false, B(), true, L(), V()>), grid, block, lds, s, a);
        }, con, multi, tgs, ball, lim, vfric);
    }
    ll_launch_done(env);
    return check_hip(hipGetLastError(), "physics_ll_kernel");
}

}  // namespace v2p
