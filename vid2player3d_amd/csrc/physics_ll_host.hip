// The part of the link-per-lane schedule that does not depend on how physics_ll_kernel is built (physics_ll.hip is compiled twice,
// see its head): the stand-alone pre-physics kernel of the staged API, the explicit slot -> env table of the pairing, and the host
// helpers both launchers of the physics kernel use.  Compiled once, with the flags of the default physics_ll.hip object (build.py):
// env_pre_kernel shares namespace strict with the fused prologue of physics_ll_kernel and must round like it.
#include <hip/hip_runtime.h>

#include "phys_common.hpp"

namespace v2p {

#include "strict_ops.inc"

// ---- pairing: a wave costs the union of its two envs' contact structure, so envs are handed to waves in descending order of
// their contact load (heavy waves first also keeps the tail of the launch short; the heaviest quarter each next to one of the lightest).
// A counting sort without a sorting kernel: every env draws an arrival index in its load bin at the end of the physics kernel (atomics)
// and appends itself to the bin's arrival list, the workgroup that finishes last scans the 256 bin counts, and the next launch looks
// its envs up (prologue of physics_ll_kernel).  The order inside a bin depends on arrival, which is harmless: an env's arithmetic does
// not depend on the env it shares a wave with (tests: bit-identical results).  The explicit slot -> env table below is built on
// demand only (v2p_env_debug_pairing).
__global__ void pair_scatter_kernel(PairView pv, int64_t n) {
    const int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (e < n) pair_scatter(pv, e);
}

// ---- stand-alone pre-physics (the staged API, v2p_env_pre_physics): one thread per action component
__global__ void env_pre_kernel(PhysArgs a, PairView pv) {
    const int64_t tid = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const int64_t e = tid / NACT;
    const int c = (int)(tid - e * NACT);
    if (e >= a.n) return;
    if (c == 0 && pv.perm) pair_scatter(pv, e);
    const bool dead = a.reset[e] == 1;
    float act = a.actions[tid];
    if (dead) { act = 0.f; a.actions[tid] = 0.f; }  // in place on the caller's tensor, like the reference
    if (c < NDOF) {
        const float tar = strict::pd_clamp(act, a.x_dof[(e * NDOF + c) * 2], a.p.pd_tar_lim);
        a.pd_target[e * NDOF + c] = tar;
        a.ctrl[CIDX(CT_PD + c)] = tar;
    } else if (c == NDOF || c == NDOF + 3) {
        const float a1 = dead ? 0.f : a.actions[tid + 1], a2 = dead ? 0.f : a.actions[tid + 2];
        const strict::V3 w = strict::residual_wrench(a.x_rb + e * NB * 13 + 3, act, a1, a2, c == NDOF ? a.p.res_force_scale : a.p.res_torque_scale);
        const int base = c == NDOF ? CT_FORCE : CT_TORQUE;
        a.ctrl[CIDX(base + 0)] = w.x; a.ctrl[CIDX(base + 1)] = w.y; a.ctrl[CIDX(base + 2)] = w.z;
    }
}

int launch_env_pre(v2p_env* env, float* actions, hipStream_t s) {
    PhysArgs a = {};
    a.ctrl = env->ctrl;
    a.actions = actions;
    a.reset = env->buf.reset;
    a.pd_target = env->buf.pd_target;
    a.x_dof = env->buf.dof_state;
    a.x_rb = env->buf.rb_state;
    a.n = env->n;
    a.p = env->p;
    PairView pv{nullptr, nullptr, nullptr, nullptr, 0, 0};  // (the physics kernel looks its envs up itself: nothing to scatter here)
    const int64_t threads = env->n * NACT;
    hipLaunchKernelGGL(env_pre_kernel, dim3((unsigned)((threads + 255) / 256)), dim3(256), 0, s, a, pv);
    return check_hip(hipGetLastError(), "env_pre_kernel");
}

bool env_pairing_on(const v2p_env* env) { return env->pair_period > 0 && env->schedule == 0 && env->p.enable_contact && env->n > 2; }

PairView env_pair_view(const v2p_env* env) {
    int mix = (int)(env->n * (int64_t)env->pair_mix_permille / 1000);
    if (2 * mix > env->n) mix = (int)(env->n / 2);
    return PairView{env->pair_key, env->pair_pos, env->pair_start, env->perm, (int32_t)env->n, mix};
}

int launch_env_pairing(v2p_env* env, hipStream_t s) {
    // (v2p_env_debug_pairing only: the wave order the next launch will look up, as an explicit slot -> env table)
    hipLaunchKernelGGL(pair_scatter_kernel, dim3((unsigned)((env->n + 255) / 256)), dim3(256), 0, s, env_pair_view(env), env->n);
    return check_hip(hipGetLastError(), "pair_scatter_kernel");
}

}  // namespace v2p
