// Free tennis balls on their own: one ball per lane, the state in registers, a whole trajectory in one launch (v2p_ball_rollout).
//
// What vid2player/utils/tennis_ball.py:113-218 (`simulate`) and tennis_ball_out_estimator.py:21-121 (`simulate_without_bounce`) do with
// Isaac Gym - 10000 ball actors stepped alone, to fill the pool of incoming launches and the estimator tables - with THIS engine's ball:
// the model is the ball lane of physics_ll.hip (aerodynamics, free flight, the ball x ground row block, integration, angular damping
// and cap) restated for a ball without a humanoid next to it, with the same formulas in the same order and compiled with the same
// floating-point flags (build.py), and the float64 oracle's (oracle/phys/v2p_phys_oracle.c, attach_ball(None, ...)).  Nothing is shared
// with physics_ll.hip as source: that file's kernels must not change when this one does.
//
// From `simulate`, and not in the env kernel: the spin SIGN of a launch (:163-176, 190-195), the pass-net / bounce bookkeeping at the
// start of every simulate() call (:167-187), the peak height after the bounce (:326-327), and - resample - the outgoing tables'
// resampling onto a distance grid and a drop grid (`simulate_without_bounce`:93-119), done online so that a table build of millions of
// launches never holds a trajectory.
#include <math.h>

#if !defined(V2P_LL_STRICT_MATH)
#define PHYS_SINCOS(x, s, c) do { (s) = __sinf(x); (c) = __cosf(x); } while (0)
#define PHYS_SQRT(x) __builtin_amdgcn_sqrtf(x)
#define PHYS_RCP(x) __builtin_amdgcn_rcpf(x)
#endif
#include "v2p_dev.hpp"

namespace v2p {

// what restates torch arithmetic (the launch spin axis, the resampler's interpolation): precise division, no contraction, inside a
// translation unit that is otherwise built relaxed like physics_ll.hip
namespace exact {
#pragma clang fp reassociate(off) reciprocal(off) contract(off)
// launch_vspin * pi * 2 * F.normalize(cross(launch_vel, (0, 0, -1))) (tennis_ball.py:135-136)
__device__ __forceinline__ V3 launch_ang_vel(V3 v, float vspin) {
    const V3 c{-v.y, v.x, 0.f};
    const float d = fmaxf(sqrtf(c.x * c.x + c.y * c.y), 1e-12f);
    const float k = vspin * 3.14159265358979f * 2.f;
    return V3{k * (c.x / d), k * (c.y / d), 0.f};
}
// the weight of sample t between samples t-1 and t (interpolate_x_batch / interpolate_y_batch, :26-37), and the blend
__device__ __forceinline__ float weight(float x, float x1, float x2) { return (x - x1) / (x2 - x1); }
__device__ __forceinline__ float blend(float a, float b, float w) { return a * (1.f - w) + b * w; }
}  // namespace exact
#if !defined(V2P_LL_STRICT_MATH)
#pragma clang fp reassociate(on) reciprocal(on) contract(fast)
#endif

constexpr int BR_LANES = 64;       // one wave per workgroup
constexpr int BR_STAGE = 16;       // frames a wave collects in LDS before it writes them out
constexpr int BR_ROW = BR_STAGE * 3 + 1;  // floats per lane of the staging area (odd: lanes fall on different banks)

struct BallRolloutArgs {
    v2p_ball_sim c;
    v2p_ball_rollout_out o;
    const float *launch_pos, *launch_vel, *launch_vspin;
    int64_t n;
    float h, inv_mass, inv_inertia;
    int32_t nx, ny;
};

// One ball per lane.  Loop nest: frames x simulate() calls x substeps.  Every loop bound is uniform, lanes past the end of the batch
// compute the last ball again and store nothing, so the workgroup barriers around the staging area are reached by all lanes.
template <bool TGS, bool RESAMPLE>
__global__ __launch_bounds__(BR_LANES) void ball_rollout_kernel(const BallRolloutArgs a) {
    extern __shared__ float stage[];
    const v2p_ball_sim& P = a.c;
    const int lane = threadIdx.x;
    const int64_t n0 = (int64_t)blockIdx.x * BR_LANES;
    const bool live = n0 + lane < a.n;
    const int64_t i = live ? n0 + lane : a.n - 1;
    V3 bp{a.launch_pos[i * 3], a.launch_pos[i * 3 + 1], a.launch_pos[i * 3 + 2]};
    V3 bv{a.launch_vel[i * 3], a.launch_vel[i * 3 + 1], a.launch_vel[i * 3 + 2]};
    const float vspin0 = a.launch_vspin[i];
    V3 bw = exact::launch_ang_vel(bv, vspin0);
    Q4 bq{0.f, 0.f, 0.f, 1.f};
    // the sign of the launch spin (:164): kept until the simulate() call that detects the bounce (:191-195)
    bool spin_pos = vspin0 > 0.f;
    const float h = a.h;
    const int F = P.num_frames, cfi = P.control_freq_inv;
    const bool want_q = a.o.final_state != nullptr, want_traj = !RESAMPLE && a.o.traj != nullptr;

    bool has_pass = false, pass_ok = false, has_bounce = false;
    V3 bounce_pos{0.f, 0.f, 0.f};
    int bounce_idx = F - 1;
    float zrec = bp.z, peak = 0.f;  // the height recorded for the current frame; the largest recorded height from the bounce frame on

    // ---- resampler state (RESAMPLE): the monotone pointers of the two grids, the previous sample, the first sample, and how many cells
    // of each grid stopped at sample 0 (their "previous" sample is the LAST one, the reference's t - 1 = -1 wrap: they are written at the end)
    const float z0 = bp.z, y0 = bp.y;
    const int S = (F + 1) * cfi;
    int kx = 0, ky = 0, k0x = 0, k0y = 0;
    float pY = 0.f, pZ = 0.f;
    auto cell_x = [&](int k) -> float { return (float)(P.grid_x[0] + (double)k * P.grid_x[2]); };
    auto cell_y = [&](int k) -> float { return (float)(P.grid_y[0] + (double)k * P.grid_y[2]); };
    auto put_x = [&](int k, float x, float Y1, float Z1, float Y2, float Z2) {
        const float w = exact::weight(x, Y1, Y2);
        if (live) a.o.traj_x[i * a.nx + k] = exact::blend(Z1, Z2, w);
    };
    auto put_y = [&](int k, float y, float Y1, float Z1, float Y2, float Z2, int t) {
        const float w = exact::weight(-y, Z1, Z2);
        if (live) {
            a.o.traj_y[(i * a.ny + k) * 2] = exact::blend(Y1, Y2, w);
            a.o.traj_y[(i * a.ny + k) * 2 + 1] = exact::blend((float)(t - 1), (float)t, w) * P.sim_dt;
        }
    };
    auto sample = [&](int t, float Y, float Z) {
        const bool last = t == S - 1;
        while (kx < a.nx) {  // (the pointer stays at t for every cell that t satisfies: :102-108)
            const float x = cell_x(kx);
            if (Y < x && !last) break;
            if (t == 0) ++k0x;
            else put_x(kx, x, pY, pZ, Y, Z);
            ++kx;
        }
        while (ky < a.ny) {
            const float y = cell_y(ky);
            if (-Z < y && !last) break;
            if (t == 0) ++k0y;
            else put_y(ky, y, pY, pZ, Y, Z, t);
            ++ky;
        }
        pY = Y; pZ = Z;
    };

    V3 Fa{0.f, 0.f, 0.f};
    const int nfr = RESAMPLE ? F + 1 : F;
    for (int t = 0; t < nfr; ++t) {
        if (!RESAMPLE) {
            // frame t = the position at the start of control step t (:151-155)
            zrec = bp.z;
            if (has_bounce) peak = fmaxf(peak, zrec);
            if (want_traj) {
                float* o = stage + lane * BR_ROW + (t % BR_STAGE) * 3;
                o[0] = bp.x; o[1] = bp.y; o[2] = bp.z;
                if (t % BR_STAGE == BR_STAGE - 1 || t == F - 1) {
                    // the wave's frames t0 .. t leave as runs of consecutive dwords: 3 (t - t0 + 1) floats per ball, consecutive lanes on
                    // consecutive addresses (a lane's own stores would be 12 bytes at a stride of 12 F)
                    const int t0 = t - t % BR_STAGE, run = (t - t0 + 1) * 3;
                    __syncthreads();
                    for (int j = lane; j < BR_LANES * run; j += BR_LANES) {
                        const int ball = j / run, r = j - ball * run;
                        if (n0 + ball < a.n) a.o.traj[((n0 + ball) * F + t0) * 3 + r] = stage[ball * BR_ROW + r];
                    }
                    __syncthreads();
                }
            }
        }
        for (int ic = 0; ic < cfi; ++ic) {
            if (RESAMPLE) sample(t * cfi + ic, bp.y, bp.z - z0);
            // ---- bookkeeping at the start of every simulate() call (:167-169)
            if (!has_pass && bp.y < 0.f) { has_pass = true; pass_ok = !has_bounce && bp.z > P.net_height; }
            // ---- aerodynamic force, held over the call's substeps (physics_ll.hip, the ball lane; :160-179)
            {
                const float kf = 1.21f * 3.14159265358979f * 0.032f * 0.032f * 0.5f, cd = 0.55f;
                const float sp = PHYS_SQRT(dot(bv, bv)), vs = sp == 0.f ? 1.f : sp;
                const V3 vn = PHYS_RCP(vs) * bv;
                const V3 vt = cross(vn, V3{0.f, 0.f, -1.f}), lt = cross(vt, vn);
                float vspin = PHYS_SQRT(dot(bw, bw)) * (1.f / 6.28318530717959f);
                if (!spin_pos) vspin = -vspin;
                float cl = PHYS_RCP(2.f + fabsf(vs * PHYS_RCP(vspin * P.spin_scale + 1e-6f)));
                cl = vspin > 0.f ? -cl : cl;
                Fa = (-kf * cd * vs) * bv - (kf * cl * vs * vs) * lt;
            }
            // ---- the bounce test on the height at the start of the call (:181-195); the force above still carries the old sign
            if (!has_bounce && bp.z <= P.bounce_height) {
                has_bounce = true;
                bounce_pos = bp;
                bounce_idx = t;
                peak = zrec;
                if (!RESAMPLE) spin_pos = true;  // (simulate_without_bounce keeps the launch's sign, :72)
            }
            for (int sub = 0; sub < P.substeps; ++sub) {
                const V3 bvs = bv + h * (V3{0.f, 0.f, P.gravity_z} + a.inv_mass * Fa);  // free flight: v*
                const V3 bv0 = bv;
                bv = bvs;
                // ---- ball x ground (speculative margin: the distance the ball can close within this substep)
                const float ih = PHYS_RCP(h), coff = P.contact_offset;
                float gap = bp.z - P.radius;
                const bool on = P.enable_ground && gap < coff + h * fmaxf(0.f, -bv0.z);
                if (on && P.num_iterations > 0) {
                    float bias = gap >= 0.f ? gap * ih : fmaxf(P.erp * gap * ih, -P.max_depenetration_velocity);
                    const float rest = (bvs.z < -P.bounce_threshold_velocity && gap * ih + bvs.z < 0.f) ? P.restitution_ground * bvs.z : 3.0e38f;  // restitution
                    bias = fminf(bias, rest);
                    float lam[3] = {0.f, 0.f, 0.f};
                    const float hs = h / (float)P.num_iterations;  // TGS: length of a time slice
                    float tgs_irem = 1.f / h;                        // TGS: 1 / (time left in the substep) for a separated point
                    const float tgs_pen = P.erp / hs;
                    const V3 rb{0.f, 0.f, -P.radius};
                    for (int it = 0; it < P.num_iterations; ++it) {
                        if (TGS && it > 0) {
                            gap = gap + hs * bv.z;  // the gap advances with the normal velocity after the previous sweep
                            tgs_irem = 1.f / (h - (float)it * hs);
                        }
                        const float gbias = TGS ? fminf(gap >= 0.f ? gap * tgs_irem : fmaxf(tgs_pen * gap, -P.max_depenetration_velocity), rest) : bias;
                        float lamn = lam[0];
                        // rows n = z, t1 = x, t2 = y at the point -R z of the centre
#pragma unroll
                        for (int ax = 0; ax < 3; ++ax) {
                            const V3 dir = ax == 0 ? V3{0.f, 0.f, 1.f} : (ax == 1 ? V3{1.f, 0.f, 0.f} : V3{0.f, 1.f, 0.f});
                            const V3 jb = cross(rb, dir);
                            const float wii = a.inv_mass + a.inv_inertia * dot(jb, jb);
                            const float rel = dot(dir, bv) + dot(jb, bw) + (ax == 0 ? gbias : 0.f);
                            const float old = lam[ax];
                            float nl = old - rel * __builtin_amdgcn_rcpf(wii);
                            if (ax == 0) nl = fmaxf(nl, 0.f);
                            else { const float lim = P.friction_ground * lamn; nl = fminf(fmaxf(nl, -lim), lim); }
                            const float dl = nl - old;
                            lam[ax] = nl;
                            if (ax == 0) lamn = nl;
                            bv = bv + (dl * a.inv_mass) * dir;
                            bw = bw + (dl * a.inv_inertia) * jb;
                        }
                    }
                }
                // ---- angular damping, cap, integrate
                bw = PHYS_RCP(1.f + h * P.angular_damping) * bw;
                const float n2 = dot(bw, bw);
                if (n2 > P.max_angular_velocity * P.max_angular_velocity) bw = (P.max_angular_velocity * rsqrtf(n2)) * bw;
                bp = bp + h * bv;
                if (want_q) bq = qnormalize(qmul(rotvec_to_quat(h * bw), bq));
            }
        }
    }
    if (RESAMPLE) {
        // the cells whose pointer never left sample 0: between the LAST sample (pY, pZ after the loop) and sample 0
        for (int k = 0; k < k0x; ++k) put_x(k, cell_x(k), pY, pZ, y0, 0.f);
        for (int k = 0; k < k0y; ++k) put_y(k, cell_y(k), pY, pZ, y0, 0.f, 0);
    }
    if (!live) return;
    if (!has_bounce) peak = zrec;  // bounce_idx = num_frames - 1: the last frame alone
    if (a.o.bounce_pos) { float* o = a.o.bounce_pos + i * 3; o[0] = bounce_pos.x; o[1] = bounce_pos.y; o[2] = bounce_pos.z; }
    if (a.o.bounce_idx) a.o.bounce_idx[i] = bounce_idx;
    if (a.o.pass_net) a.o.pass_net[i] = pass_ok ? 1 : 0;
    if (a.o.peak_after_bounce) a.o.peak_after_bounce[i] = peak;
    if (a.o.final_state) {
        float* o = a.o.final_state + i * 13;
        o[0] = bp.x; o[1] = bp.y; o[2] = bp.z; o[3] = bq.x; o[4] = bq.y; o[5] = bq.z; o[6] = bq.w;
        o[7] = bv.x; o[8] = bv.y; o[9] = bv.z; o[10] = bw.x; o[11] = bw.y; o[12] = bw.z;
    }
}

// cells of a (lo, hi, step) grid as the reference counts them: int((hi - lo) / step) in float64 (tennis_ball_out_estimator.py:95-96)
int ball_grid_cells(const double g[3]) {
    if (!(g[2] > 0.0) || !(g[1] > g[0])) return 0;
    const double n = (g[1] - g[0]) / g[2];
    return n > 1e6 ? 0 : (int)n;
}

int launch_ball_rollout(const v2p_ball_sim& c, int64_t n, const float* launch_pos, const float* launch_vel, const float* launch_vspin,
                        const v2p_ball_rollout_out& out, hipStream_t s) {
    BallRolloutArgs a;
    a.c = c;
    a.o = out;
    a.launch_pos = launch_pos; a.launch_vel = launch_vel; a.launch_vspin = launch_vspin;
    a.n = n;
    a.h = c.sim_dt / (float)c.substeps;
    a.inv_mass = 1.f / c.mass;
    a.inv_inertia = 1.f / c.inertia;
    a.nx = c.resample ? ball_grid_cells(c.grid_x) : 0;
    a.ny = c.resample ? ball_grid_cells(c.grid_y) : 0;
    const dim3 grid((unsigned)((n + BR_LANES - 1) / BR_LANES)), block(BR_LANES);
    const size_t lds = (!c.resample && out.traj) ? sizeof(float) * BR_LANES * BR_ROW : 0;
    const bool tgs = c.solver_type == 1;
    if (c.resample) {
        if (tgs) hipLaunchKernelGGL((ball_rollout_kernel<true, true>), grid, block, lds, s, a);
        else hipLaunchKernelGGL((ball_rollout_kernel<false, true>), grid, block, lds, s, a);
    } else {
        if (tgs) hipLaunchKernelGGL((ball_rollout_kernel<true, false>), grid, block, lds, s, a);
        else hipLaunchKernelGGL((ball_rollout_kernel<false, false>), grid, block, lds, s, a);
    }
    return check_hip(hipGetLastError(), "ball_rollout_kernel");
}

}  // namespace v2p
