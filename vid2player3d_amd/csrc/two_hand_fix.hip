// The two-hand backhand fix of a record (vid2player/env/tasks/humanoid_smpl_im_mvae.py:948-1031, optimize_two_hand_backhand with
// single=True as render_one_result calls it): the frames of a two-hand backhand get num_iters Adam steps of inverse kinematics on the
// free arm's four joints, so that the free hand lands on the racket handle.  The reference builds 500 autograd graphs over one tensor;
// here the work is what it is - a chain of four joints per frame and twelve unknowns:
//
//   v2p_two_hand_fix   two_hand_fix_kernel: ONE workgroup of THF_THREADS per track, all tracks of a call in one launch.
//     1. flags: every thread counts the flagged frames of its contiguous chunk, thread 0 sums the THF_THREADS counts, every thread
//        writes the frame numbers of its chunk to its place of the list - the compaction in frame order.  Above the cap the track is
//        copied whole and overflow[t] = F.  The frames that are not flagged are copied, a wave per frame.
//     2. set-up, once per flagged frame i (thread i % THF_THREADS, its slot i / THF_THREADS): the walk from the root to the racket
//        hand gives the target, the walk to the free collar's parent the constant prefix (its global rotation G and the collar's
//        position); the round trip of the four joints gives their angle-axis vectors.  These 27 floats are kept in the frame's own
//        row of `out` until the row is written - the row is the frame's workspace, read only by the thread that wrote it.
//     3. num_iters steps: delta and Adam's two moments stay in registers, THF_K frames per thread.  Forward: four Rodrigues matrices
//        behind the prefix.  Backward by hand: each of the twelve partials is (prefix^T g) . dR/dtheta (suffix) with the
//        `theta + 1e-6` denominator and the constant first-order branch, g a sign over 3F.  A mean's gradient is a sign over a count:
//        no reduction.  The one cross-thread value is the previous iteration's delta of the frame before (the smoothness term, whose
//        gradient goes to the later frame only); it goes through LDS, component-major, between two barriers.
//     4. the 24 joints' round trip and the four optimised joints are written to the row.
//
// Bit equality with the numpy statement (two_hand_fix.two_hand_fix_reference): the law takes the sign of rounding noise, so every
// operation is the statement's in its order (this unit is built without FMA contraction), sine and cosine are evaluated in double and
// rounded once, the closing arctangent is tennis_pose_dev.hpp's wide one, Adam's bias terms are running products in double.
// No atomics; every address has one writer per phase.
#include <limits.h>

#include "tennis_pose_dev.hpp"
#include "two_hand_fix.hpp"

namespace v2p {

namespace {

constexpr int THF_THREADS = V2P_TWO_HAND_FIX_THREADS;
constexpr int THF_K = V2P_TWO_HAND_FIX_FRAMES_PER_THREAD;
constexpr int THF_MAXF = V2P_TWO_HAND_FIX_MAX_FRAMES;
constexpr int THF_WAVE = 64;
constexpr int THF_MAXP = 12;  // joints of a chain from the root
constexpr int THF_ROW = TE_JOINTS * 3;
constexpr int ST_G = 0, ST_P13 = 9, ST_TARGET = 12, ST_ORIGIN = 15, ST_SIZE = 27;  // the frame's constants in its row of `out`
static_assert(ST_SIZE <= THF_ROW, "the constants of a frame live in its own row");
constexpr size_t THF_LDS_BYTES = (size_t)(12 * THF_MAXF + THF_MAXF + THF_THREADS + 1) * 4;
static_assert(THF_LDS_BYTES <= 160 * 1024, "the exchange of delta, the frame list and the counts fit the LDS of a CU");

struct ThfPaths {
    int32_t pre_len, arm_len;
    int32_t pre[THF_MAXP];  // root .. the free collar's parent
    int32_t arm[THF_MAXP];  // root .. racket wrist, racket hand
    int32_t ik[4];          // wrist, elbow, shoulder, collar of the free arm
    int32_t free_hand;
};

struct TwoHandFixArgs {
    v2p_two_hand_fix_buffers b;
    int64_t length;
    int32_t num_iters, num_bind;
    ThfPaths path[2];  // by righthand != 0
};

struct ThfTrig {
    float theta2, theta, d, c, s, t;
};

__device__ __forceinline__ float thf_sign(float x) { return (float)((x > 0.f) - (x < 0.f)); }

// what angle_axis_to_rotation_matrix and its derivative share; sine and cosine in double, rounded once
__device__ __forceinline__ ThfTrig thf_trig(const float* r) {
    ThfTrig g;
    g.theta2 = r[0] * r[0] + r[1] * r[1] + r[2] * r[2];
    g.theta = sqrtf(ref_clamp_min(g.theta2, 1e-6f));
    g.d = g.theta + 1e-6f;
    g.c = (float)cos((double)g.theta);
    g.s = (float)sin((double)g.theta);
    g.t = 1.f - g.c;
    return g;
}

// ref_angle_axis_to_rotmat's lines over thf_trig
__device__ __forceinline__ void thf_rotmat(const float* r, const ThfTrig& g, float* m) {
    if (g.theta2 > 1e-6f) {
        const float wx = r[0] / g.d, wy = r[1] / g.d, wz = r[2] / g.d;
        const float c = g.c, s = g.s, t = g.t;
        m[0] = c + wx * wx * t;        m[1] = wx * wy * t - wz * s;   m[2] = wy * s + wx * wz * t;
        m[3] = wz * s + wx * wy * t;   m[4] = c + wy * wy * t;        m[5] = -wx * s + wy * wz * t;
        m[6] = -wy * s + wx * wz * t;  m[7] = wx * s + wy * wz * t;   m[8] = c + wz * wz * t;
    } else {
        m[0] = 1.f;   m[1] = -r[2]; m[2] = r[1];
        m[3] = r[2];  m[4] = 1.f;   m[5] = -r[0];
        m[6] = -r[1]; m[7] = r[0];  m[8] = 1.f;
    }
}

__device__ __forceinline__ void thf_aa_to_rotmat(const float* r, float* m) {
    const ThfTrig g = thf_trig(r);
    thf_rotmat(r, g, m);
}

// rotation_matrix_to_angle_axis with the wide arctangent
__device__ __forceinline__ void thf_rotmat_to_aa(const float* m, float* aa) {
    float q[4];
    ref_rotmat_to_quat(m, q);
    te_quat_to_angle_axis(q, aa);
}

// P @ m, P t, P^T g as batch_rigid_transform's statement sums them
__device__ __forceinline__ void thf_matmul(const float* P, const float* m, float* o) {
#pragma unroll
    for (int a = 0; a < 3; ++a)
#pragma unroll
        for (int c = 0; c < 3; ++c) o[a * 3 + c] = P[a * 3] * m[c] + P[a * 3 + 1] * m[3 + c] + P[a * 3 + 2] * m[6 + c];
}
__device__ __forceinline__ void thf_matvec(const float* P, const float* t, float* o) {
#pragma unroll
    for (int a = 0; a < 3; ++a) o[a] = P[a * 3] * t[0] + P[a * 3 + 1] * t[1] + P[a * 3 + 2] * t[2];
}
__device__ __forceinline__ void thf_mattvec(const float* P, const float* g, float* o) {
#pragma unroll
    for (int c = 0; c < 3; ++c) o[c] = P[c] * g[0] + P[3 + c] * g[1] + P[6 + c] * g[2];
}
__device__ __forceinline__ float thf_dot(const float* a, const float* b) { return a[0] * b[0] + a[1] * b[1] + a[2] * b[2]; }

// d/dr of q^T R(r) u (two_hand_fix.rodrigues_partials)
__device__ __forceinline__ void thf_partials(const float* r, const ThfTrig& g, const float* q, const float* u, float* o) {
    const float b[3] = {u[1] * q[2] - u[2] * q[1], u[2] * q[0] - u[0] * q[2], u[0] * q[1] - u[1] * q[0]};
    if (!(g.theta2 > 1e-6f)) {
        o[0] = b[0]; o[1] = b[1]; o[2] = b[2];
        return;
    }
    const float w[3] = {r[0] / g.d, r[1] / g.d, r[2] / g.d};
    const float e[3] = {r[0] / g.theta, r[1] / g.theta, r[2] / g.theta};
    const float wq = thf_dot(w, q), wu = thf_dot(w, u), qu = thf_dot(q, u), wb = thf_dot(w, b);
    const float dd = g.d * g.d;
    const float rq = thf_dot(r, q) / dd, ru = thf_dot(r, u) / dd, rb = thf_dot(r, b) / dd;
    const float S = g.s * (wq * wu - qu) + g.c * wb;
#pragma unroll
    for (int k = 0; k < 3; ++k)
        o[k] = e[k] * S + g.t * ((q[k] / g.d - e[k] * rq) * wu + wq * (u[k] / g.d - e[k] * ru)) + g.s * (b[k] / g.d - e[k] * rb);
}

__device__ __forceinline__ bool thf_flagged(const float* phase, const int64_t* swing, int64_t f) {
    const float p = phase[f];
    return swing[f] == 2 && p > 2.0f && p < 5.0f;
}

// the walk from the root along `path` (batch_rigid_transform's lines for these joints): R, p of the last joint, p of the one before
__device__ __forceinline__ void thf_walk(const float* in, const float* bind, const int32_t* path, int len, float* R, float* p, float* p_before) {
    thf_aa_to_rotmat(in + path[0] * 3, R);
    for (int c = 0; c < 3; ++c) p[c] = p_before[c] = bind[path[0] * 3 + c];
    for (int k = 1; k < len; ++k) {
        const int j = path[k], pj = path[k - 1];
        const float t[3] = {bind[j * 3] - bind[pj * 3], bind[j * 3 + 1] - bind[pj * 3 + 1], bind[j * 3 + 2] - bind[pj * 3 + 2]};
        float pn[3], m[9], Rn[9];
        thf_matvec(R, t, pn);
        thf_aa_to_rotmat(in + j * 3, m);
        thf_matmul(R, m, Rn);
        for (int c = 0; c < 3; ++c) {
            p_before[c] = p[c];
            p[c] = pn[c] + p[c];
        }
        for (int c = 0; c < 9; ++c) R[c] = Rn[c];
    }
}

// the constants of flagged frame i, into its row of `out`
__device__ __forceinline__ void thf_setup(const float* in, const float* bind, const ThfPaths& P, float* row) {
    float R[9], p[3], pb[3];
    thf_walk(in, bind, P.arm, P.arm_len, R, p, pb);  // p: the racket hand, pb: the racket wrist
    const float b0[3] = {bind[0], bind[1], bind[2]};
    float target[3];
    for (int c = 0; c < 3; ++c) {
        const float hand = p[c] - b0[c], wrist = pb[c] - b0[c], root = b0[c] - b0[c];
        target[c] = 2.f * hand - wrist - root;
    }
    thf_walk(in, bind, P.pre, P.pre_len, R, p, pb);  // R, p: the free collar's parent
    const int collar = P.ik[3], last = P.pre[P.pre_len - 1];
    const float t[3] = {bind[collar * 3] - bind[last * 3], bind[collar * 3 + 1] - bind[last * 3 + 1], bind[collar * 3 + 2] - bind[last * 3 + 2]};
    float p13[3];
    thf_matvec(R, t, p13);
    float origin[12];
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        float m[9];
        thf_aa_to_rotmat(in + P.ik[k] * 3, m);
        thf_rotmat_to_aa(m, origin + k * 3);
    }
    for (int c = 0; c < 9; ++c) row[ST_G + c] = R[c];
    for (int c = 0; c < 3; ++c) {
        row[ST_P13 + c] = p13[c] + p[c];
        row[ST_TARGET + c] = target[c];
    }
    for (int c = 0; c < 12; ++c) row[ST_ORIGIN + c] = origin[c];
}

struct ThfStep {
    float g_target, g_reg, g_smooth;  // the three signs' weights over their counts
    float step_size, bc2_sqrt;        // Adam's bias terms of this step
    bool smooth;                      // F > 1
};

// one Adam step of one frame: d, m, v [12] are (wrist, elbow, shoulder, collar) x 3
__device__ __forceinline__ void thf_step(const float* row, const float* bind, const ThfPaths& P, const ThfStep& a, bool has_prev, const float* prev, float* d, float* m, float* v) {
    float G[9], p13[3], target[3], r[4][3];
#pragma unroll
    for (int c = 0; c < 9; ++c) G[c] = row[ST_G + c];
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        p13[c] = row[ST_P13 + c];
        target[c] = row[ST_TARGET + c];
    }
#pragma unroll
    for (int k = 0; k < 4; ++k)
#pragma unroll
        for (int c = 0; c < 3; ++c) r[k][c] = row[ST_ORIGIN + k * 3 + c] + d[k * 3 + c];
    // the chain's offsets: shoulder - collar, elbow - shoulder, wrist - elbow, hand - wrist
    const int chain[5] = {P.ik[3], P.ik[2], P.ik[1], P.ik[0], P.free_hand};
    float off[4][3], b0[3];
#pragma unroll
    for (int k = 0; k < 4; ++k)
#pragma unroll
        for (int c = 0; c < 3; ++c) off[k][c] = bind[chain[k + 1] * 3 + c] - bind[chain[k] * 3 + c];
#pragma unroll
    for (int c = 0; c < 3; ++c) b0[c] = bind[c];
    ThfTrig tg[4];
    float D[9], Cm[9], B[9], A[9];
#pragma unroll
    for (int k = 0; k < 4; ++k) tg[k] = thf_trig(r[k]);
    thf_rotmat(r[0], tg[0], D);
    thf_rotmat(r[1], tg[1], Cm);
    thf_rotmat(r[2], tg[2], B);
    thf_rotmat(r[3], tg[3], A);
    float G13[9], G16[9], G18[9], G20[9], p16[3], p18[3], p20[3], p22[3];
    thf_matmul(G, A, G13);
    thf_matvec(G13, off[0], p16);
    thf_matmul(G13, B, G16);
    thf_matvec(G16, off[1], p18);
    thf_matmul(G16, Cm, G18);
    thf_matvec(G18, off[2], p20);
    thf_matmul(G18, D, G20);
    thf_matvec(G20, off[3], p22);
    float g[3];
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        p16[c] = p16[c] + p13[c];
        p18[c] = p18[c] + p16[c];
        p20[c] = p20[c] + p18[c];
        p22[c] = p22[c] + p20[c];
        const float p_free = p22[c] - b0[c];
        g[c] = thf_sign(p_free - target[c]) * a.g_target;
    }
    float uC[3], uB[3], uA[3], q[3], grad[12];
    thf_matvec(D, off[3], uC);
#pragma unroll
    for (int c = 0; c < 3; ++c) uC[c] = off[2][c] + uC[c];
    thf_matvec(Cm, uC, uB);
#pragma unroll
    for (int c = 0; c < 3; ++c) uB[c] = off[1][c] + uB[c];
    thf_matvec(B, uB, uA);
#pragma unroll
    for (int c = 0; c < 3; ++c) uA[c] = off[0][c] + uA[c];
    thf_mattvec(G18, g, q);
    thf_partials(r[0], tg[0], q, off[3], grad);
    thf_mattvec(G16, g, q);
    thf_partials(r[1], tg[1], q, uC, grad + 3);
    thf_mattvec(G13, g, q);
    thf_partials(r[2], tg[2], q, uB, grad + 6);
    thf_mattvec(G, g, q);
    thf_partials(r[3], tg[3], q, uA, grad + 9);
    const float om1 = (float)(1.0 - 0.9), b2 = 0.999f, om2 = (float)(1.0 - 0.999);
#pragma unroll
    for (int c = 0; c < 12; ++c) {
        float gg = grad[c] + thf_sign(d[c]) * a.g_reg;
        if (a.smooth) gg = gg + (has_prev ? thf_sign(d[c] - prev[c]) * a.g_smooth : 0.f);
        m[c] = m[c] + (gg - m[c]) * om1;
        v[c] = v[c] * b2 + om2 * gg * gg;
        const float denom = sqrtf(v[c]) / a.bc2_sqrt + 1e-8f;
        d[c] = d[c] - a.step_size * m[c] / denom;
    }
}

// the frame's row as the fix returns it: the round trip of the 24 joints, the free arm's four with delta added in between
__device__ __forceinline__ void thf_finish(const float* in, const ThfPaths& P, const float* d, float* row) {
    float origin[12];
#pragma unroll
    for (int c = 0; c < 12; ++c) origin[c] = row[ST_ORIGIN + c];  // (before the row is written)
    for (int j = 0; j < TE_JOINTS; ++j) {
        if (j == P.ik[0] || j == P.ik[1] || j == P.ik[2] || j == P.ik[3]) continue;
        float m[9], aa[3];
        thf_aa_to_rotmat(in + j * 3, m);
        thf_rotmat_to_aa(m, aa);
        for (int c = 0; c < 3; ++c) row[j * 3 + c] = aa[c];
    }
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const float r[3] = {origin[k * 3] + d[k * 3], origin[k * 3 + 1] + d[k * 3 + 1], origin[k * 3 + 2] + d[k * 3 + 2]};
        float m[9], aa[3];
        thf_aa_to_rotmat(r, m);
        thf_rotmat_to_aa(m, aa);
        for (int c = 0; c < 3; ++c) row[P.ik[k] * 3 + c] = aa[c];
    }
}

// The THF_K frames of a thread, slot by slot.  Recursion over the slot instead of a loop: the registers' arrays are indexed by constants
// whatever the unroller decides about a body of this size.
template <int K>
__device__ __forceinline__ void thf_steps(int tid, int F, int R, const int32_t* frame_of, const float* ex, float* out, const float* bind, const ThfPaths& P, const ThfStep& a,
                                          float (&d)[THF_K][12], float (&m)[THF_K][12], float (&v)[THF_K][12]) {
    const int i = tid + K * THF_THREADS;
    if (i < F) {
        float prev[12];
#pragma unroll
        for (int c = 0; c < 12; ++c) prev[c] = i > 0 ? ex[c * THF_MAXF + i - 1] : 0.f;
        const int64_t f = frame_of[i];
        thf_step(out + f * THF_ROW, bind + (int64_t)(i % R) * THF_ROW, P, a, i > 0, prev, d[K], m[K], v[K]);
    }
    if constexpr (K + 1 < THF_K) thf_steps<K + 1>(tid, F, R, frame_of, ex, out, bind, P, a, d, m, v);
}

template <int K>
__device__ __forceinline__ void thf_publish(int tid, int F, float* ex, const float (&d)[THF_K][12]) {
    const int i = tid + K * THF_THREADS;
    if (i < F) {
#pragma unroll
        for (int c = 0; c < 12; ++c) ex[c * THF_MAXF + i] = d[K][c];
    }
    if constexpr (K + 1 < THF_K) thf_publish<K + 1>(tid, F, ex, d);
}

template <int K>
__device__ __forceinline__ void thf_finish_all(int tid, int F, const int32_t* frame_of, const float* in, float* out, const ThfPaths& P, const float (&d)[THF_K][12]) {
    const int i = tid + K * THF_THREADS;
    if (i < F) {
        const int64_t f = frame_of[i];
        thf_finish(in + f * THF_ROW, P, d[K], out + f * THF_ROW);
    }
    if constexpr (K + 1 < THF_K) thf_finish_all<K + 1>(tid, F, frame_of, in, out, P, d);
}

__global__ __launch_bounds__(THF_THREADS) void two_hand_fix_kernel(const TwoHandFixArgs h) {
    extern __shared__ float thf_lds[];
    float* ex = thf_lds;                                     // [12][THF_MAXF]: delta, component-major
    int32_t* frame_of = (int32_t*)(thf_lds + 12 * THF_MAXF);  // [THF_MAXF]: the flagged frames in frame order
    int32_t* scan = frame_of + THF_MAXF;                     // [THF_THREADS + 1]
    const int tid = threadIdx.x, lane = tid & (THF_WAVE - 1);
    const int64_t t = blockIdx.x, L = h.length;
    const v2p_two_hand_fix_buffers& b = h.b;
    int64_t nf = b.nframes[t];
    nf = nf < 0 ? 0 : (nf > L ? L : nf);
    const ThfPaths& P = b.righthand[t] != 0 ? h.path[1] : h.path[0];
    const float* in = b.joint_rot + t * L * THF_ROW;
    const float* phase = b.phase + t * L;
    const int64_t* swing = b.swing_type + t * L;
    float* out = b.out + t * L * THF_ROW;

    // 1. the flags: counts per chunk, their prefix, the list
    const int64_t per = (nf + THF_THREADS - 1) / THF_THREADS;
    const int64_t f0 = tid * per < nf ? tid * per : nf, f1 = f0 + per < nf ? f0 + per : nf;
    int count = 0;
    for (int64_t f = f0; f < f1; ++f) count += thf_flagged(phase, swing, f) ? 1 : 0;
    scan[tid] = count;
    __syncthreads();
    if (tid == 0) {
        int sum = 0;
        for (int i = 0; i < THF_THREADS; ++i) {
            const int c = scan[i];
            scan[i] = sum;
            sum += c;
        }
        scan[THF_THREADS] = sum;
    }
    __syncthreads();
    const int64_t F = scan[THF_THREADS];
    const bool over = F > THF_MAXF;
    if (tid == 0) b.overflow[t] = over ? (int32_t)(F > INT_MAX ? INT_MAX : F) : 0;
    if (!over) {
        int at = scan[tid];
        for (int64_t f = f0; f < f1; ++f)
            if (thf_flagged(phase, swing, f)) frame_of[at++] = (int32_t)f;
    }
    for (int64_t f = tid / THF_WAVE; f < nf; f += THF_THREADS / THF_WAVE)
        if (over || !thf_flagged(phase, swing, f))
            for (int c = lane; c < THF_ROW; c += THF_WAVE) out[f * THF_ROW + c] = in[f * THF_ROW + c];
    if (over || F == 0) return;  // (the whole workgroup)
    __syncthreads();

    // 2. the constants, delta = 0
    const int R = h.num_bind;
    for (int i = tid; i < (int)F; i += THF_THREADS) {
        const int64_t f = frame_of[i];
        thf_setup(in + f * THF_ROW, b.bind + (int64_t)(i % R) * THF_ROW, P, out + f * THF_ROW);
#pragma unroll
        for (int c = 0; c < 12; ++c) ex[c * THF_MAXF + i] = 0.f;
    }
    __syncthreads();

    // 3. the steps
    float d[THF_K][12], m[THF_K][12], v[THF_K][12];
#pragma unroll
    for (int k = 0; k < THF_K; ++k)
#pragma unroll
        for (int c = 0; c < 12; ++c) d[k][c] = m[k][c] = v[k][c] = 0.f;
    ThfStep a;
    a.g_target = 1.f / (float)(3 * F);
    a.g_reg = 0.2f / (float)(12 * F);
    a.smooth = F > 1;
    a.g_smooth = a.smooth ? 0.5f / (float)(12 * (F - 1)) : 0.f;
    double b1 = 1.0, b2 = 1.0;
    for (int it = 0; it < h.num_iters; ++it) {
        b1 *= 0.9;
        b2 *= 0.999;
        a.step_size = (float)(0.005 / (1.0 - b1));
        a.bc2_sqrt = (float)sqrt(1.0 - b2);
        thf_steps<0>(tid, (int)F, h.num_bind, frame_of, ex, out, b.bind, P, a, d, m, v);
        __syncthreads();  // every delta of the step before has been read
        thf_publish<0>(tid, (int)F, ex, d);
        __syncthreads();
    }

    // 4. the rows
    thf_finish_all<0>(tid, (int)F, frame_of, in, out, P, d);
}

// the chain root .. joint j into path (root first); its length, 0 when it is longer than THF_MAXP
int chain_to(const int32_t* parents, int j, int32_t* path) {
    int32_t rev[TE_JOINTS];
    int len = 0;
    for (; j >= 0; j = parents[j]) rev[len++] = j;  // (parents[j] < j: it ends)
    if (len > THF_MAXP) return 0;
    for (int k = 0; k < len; ++k) path[k] = rev[len - 1 - k];
    return len;
}

const char* fill_paths(const v2p_two_hand_fix_cfg& c, ThfPaths* path) {
    if (c.smpl_parents[0] != -1) return "smpl_parents[0] is not -1";
    for (int j = 1; j < TE_JOINTS; ++j)
        if (c.smpl_parents[j] < 0 || c.smpl_parents[j] >= j) return "smpl_parents is no tree with every parent before its children";
    if (te_body_of_smpl_fault(c.smpl_of_body) >= 0) return "smpl_of_body is not a permutation of 0..23 with the root first";
    for (int rh = 0; rh < 2; ++rh) {
        ThfPaths& p = path[rh];
        const int hand = c.smpl_of_body[rh ? 23 : 18], wrist = c.smpl_of_body[rh ? 22 : 17], free_hand = c.smpl_of_body[rh ? 18 : 23];
        const int ik[4] = {rh ? 20 : 21, rh ? 18 : 19, rh ? 16 : 17, rh ? 13 : 14};
        if (c.smpl_parents[free_hand] != ik[0] || c.smpl_parents[ik[0]] != ik[1] || c.smpl_parents[ik[1]] != ik[2] || c.smpl_parents[ik[2]] != ik[3] || c.smpl_parents[ik[3]] < 0)
            return "the free arm is not the chain collar - shoulder - elbow - wrist - hand of the law's joints";
        if (c.smpl_parents[hand] != wrist) return "the racket wrist's body is not the parent of the racket hand's";
        for (int k = 0; k < THF_MAXP; ++k) p.pre[k] = p.arm[k] = 0;
        p.pre_len = chain_to(c.smpl_parents, c.smpl_parents[ik[3]], p.pre);
        p.arm_len = chain_to(c.smpl_parents, hand, p.arm);
        if (p.pre_len < 1 || p.arm_len < 2) return "a chain from the root is longer than 12 joints";
        for (int k = 0; k < 4; ++k) p.ik[k] = ik[k];
        p.free_hand = free_hand;
    }
    return nullptr;
}

}  // namespace

const char* two_hand_fix_cfg_fault(const v2p_two_hand_fix_cfg& c) {
    ThfPaths path[2];
    return fill_paths(c, path);
}

int launch_two_hand_fix(const v2p_two_hand_fix_cfg& c, int64_t num_tracks, int64_t track_length, const v2p_two_hand_fix_buffers& b, hipStream_t s) {
    TwoHandFixArgs h;
    h.b = b;
    h.length = track_length;
    h.num_iters = c.num_iters;
    h.num_bind = c.num_bind;
    if (const char* why = fill_paths(c, h.path)) {
        set_error("v2p_two_hand_fix: %s", why);
        return V2P_ERR_INVALID;
    }
    // (more than the 64 KB a kernel gets unasked; the attribute is the function's on the current device: set at every launch)
    const int rc = check_hip(hipFuncSetAttribute((const void*)two_hand_fix_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)THF_LDS_BYTES), "hipFuncSetAttribute(two_hand_fix_kernel)");
    if (rc != V2P_OK) return rc;
    hipLaunchKernelGGL(two_hand_fix_kernel, dim3((unsigned)num_tracks), dim3(THF_THREADS), THF_LDS_BYTES, s, h);
    return check_hip(hipGetLastError(), "two_hand_fix_kernel");
}

}  // namespace v2p
