// The MotionVAE motion generator of a control step (vid2player/players/mvae_player.py `MVAEPlayer.step` / `reset`, around
// motion_vae/model.py:186-252 `MixedDecoder.forward`): v2p_mvae_step is the gate, the three expert-blended layers and
// `_update_mvae_state(init=False)` in one launch; v2p_mvae_reset is `_update_mvae_state(init=True)` for a list of env ids.
//
// The decoder.  The reference blends the six experts' weights per env and multiplies with one matrix per env (239,168 blended weights
// per env, written and read back).  Here every expert is computed and the RESULTS are blended, out = sum_e c_e (x W_e + b_e): the same
// function, a GEMM with shared weights and the blend in its epilogue.  A workgroup of four waves owns MV_TILE = 32 envs.  Its
// activations stay in LDS: two [32][324] buffers hold cat(z, previous) of the layer being read and of the layer being written, and the
// gate has two small ones.  The product runs on v_mfma_f32_32x32x2_f32 (fp32 in, fp32 accumulate: a k-ordered fmaf chain per output): a
// wave takes a tile of 32 output columns, keeps SIX accumulators - one per expert, 96 registers - and walks K once; lane l feeds
// A[env l&31][k = 2s + (l>>5)] from LDS and B[k][column l&31] from the packed weights.  Both operands are laid out so that four
// consecutive k-steps of a lane are 16 contiguous bytes: the weights are repacked on the host (v2p_rollout.h, v2p_mvae_weights), and the
// LDS buffers store column k of a row at mv_perm(k).  The weights (5.7 MB) are read by every workgroup and stay in L2 / Infinity Cache.
//
// The state update restates torch elementwise float32 code (built without FMA contraction like tennis_task.hip): the same operations in
// the same order.  Eight threads share an env: columns are stored coalesced over the tile, joints are dealt three to a thread.
#include "mvae_player.hpp"

namespace v2p {

namespace {

constexpr int MV_FRAME = V2P_MVAE_FRAME, MV_LATENT = V2P_MVAE_LATENT, MV_HIDDEN = V2P_MVAE_HIDDEN, MV_EXPERTS = V2P_MVAE_EXPERTS, MV_GATE = V2P_MVAE_GATE;
constexpr int MV_IN0 = MV_LATENT + MV_FRAME;   // 320: cat(z, condition)
constexpr int MV_IN1 = MV_LATENT + MV_HIDDEN;  // 288: cat(z, hidden)
constexpr int MV_OUT = MV_FRAME + 2;           // 290: the feature and the two phase numbers
constexpr int MV_TILE = 32;                    // envs of a workgroup
constexpr int MV_THREADS = 256;
constexpr int MV_XS = 324;                     // floats of a row of the two activation buffers (320, + 4: rows 16 bytes aligned, banks skewed)
constexpr int MV_GS = 68;                      // ... of the gate's buffers
constexpr int MV_JOINTS = 24;
constexpr int MV_COL_JOINT_POS = 6, MV_COL_ROT6D = 144, MV_COL_ROOT_VEL = 3;
constexpr int MV_RWRIST = 21;
constexpr float MV_PI = 3.14159265358979323846f;

typedef float f32x16 __attribute__((ext_vector_type(16)));

// where column k of a row lives in an LDS activation buffer: within its group of 8, k = 8g + 2q + h sits at 8g + 4h + q, so that the four
// k-steps q = 0..3 of lane half h are one 16-byte read
__device__ __host__ inline int mv_perm(int k) { return (k & ~7) | ((k & 1) << 2) | ((k >> 1) & 3); }

// the residual-DoF rule of a player (mvae_player.py:306-408) as a table.  A row: envs of swing type `swing` whose phase lies in
// (lo, hi) - [lo, hi) with ge - get the base angles whose bit is set in `set`, rows applied in order (elbow twist, wrist twist, wrist
// shake, wrist swing; in units of pi).  fh / bh: the two windows outside of which a residual is zeroed when not training.
struct MvWindow {
    int swing;
    float lo, hi;
    int ge, set;
    float base[4];
};
struct MvPlayer {
    int rows;
    MvWindow w[7];
    float fh_lo, fh_hi, bh_lo, bh_hi;
};
__constant__ MvPlayer MV_PLAYERS[3] = {
    {5,  // djokovic
     {{1, 2.0f, 3.2f, 0, 1, {-0.75f, 0, 0, 0}}, {1, 2.0f, 3.1f, 0, 8, {0, 0, 0, -0.25f}}, {1, 3.1f, 3.2f, 1, 8, {0, 0, 0, 0.25f}}, {2, 2.0f, 3.2f, 0, 1, {-0.25f, 0, 0, 0}},
      {2, 2.0f, 3.0f, 0, 8, {0, 0, 0, 0.1f}}},
     2.0f, 3.2f, 2.0f, 3.2f},
    {7,  // federer
     {{1, 2.0f, 3.2f, 0, 1, {-0.5f, 0, 0, 0}}, {1, 2.0f, 3.1f, 0, 8, {0, 0, 0, -0.25f}}, {1, 3.1f, 3.2f, 1, 8, {0, 0, 0, 0.25f}}, {2, 2.0f, 3.5f, 0, 6, {0, -0.25f, 0.15f, 0}},
      {3, 2.0f, 3.5f, 0, 2, {0, -0.1f, 0, 0}}, {0, 2.0f, 3.3f, 0, 7, {-0.25f, -0.5f, 0.1f, 0}}, {0, 2.0f, 3.0f, 0, 8, {0, 0, 0, -0.5f}}},
     2.0f, 3.2f, 2.0f, 3.5f},
    {3,  // nadal
     {{1, 2.5f, 3.2f, 0, 9, {-0.75f, 0, 0, 0.25f}}, {2, 2.0f, 3.5f, 0, 2, {0, -0.4f, 0, 0}}, {2, 2.0f, 3.0f, 0, 8, {0, 0, 0, -0.25f}}},
     2.5f, 3.2f, 2.0f, 3.5f},
};

struct MvArgs {
    v2p_mvae_cfg c;
    v2p_mvae_weights w;
    v2p_mvae_buffers b;
    const float *latents, *residual;
    const int64_t* env_ids;                        // reset only
    const float *init_feature, *root_xy, *bind;    // reset only
    int64_t n, num_envs;
};

// ---------------------------------------------------------------------------------------------------------------- rotations
// x.clamp_min(lo) as torch evaluates it: a NaN stays a NaN
__device__ inline float mv_clamp_min(float x, float lo) { return x < lo ? lo : x; }
__device__ inline float mv_norm3(float x, float y, float z) { return sqrtf(x * x + y * y + z * z); }

// rot6d_to_rotmat (utils/torch_transform.py:221-235) with its two eps = 1e-8 fallbacks; m row-major, columns b1 b2 b3
__device__ inline void mv_rot6d_to_rotmat(const float* r, float* m) {
    float ax = r[0], ay = r[1], az = r[2];
    const float cx = r[3], cy = r[4], cz = r[5];
    if (mv_norm3(ax, ay, az) < 1e-8f) { ax = 1.f; ay = 0.f; az = 0.f; }
    const float n1 = mv_clamp_min(mv_norm3(ax, ay, az), 1e-9f);
    const float b1x = ax / n1, b1y = ay / n1, b1z = az / n1;
    const float d = b1x * cx + b1y * cy + b1z * cz;
    const float ux = cx - d * b1x, uy = cy - d * b1y, uz = cz - d * b1z;
    const float n2 = mv_clamp_min(mv_norm3(ux, uy, uz), 1e-9f);
    float b2x = ux / n2, b2y = uy / n2, b2z = uz / n2;
    if (mv_norm3(b2x, b2y, b2z) < 1e-8f) { b2x = 0.f; b2y = 1.f; b2z = 0.f; }
    m[0] = b1x; m[3] = b1y; m[6] = b1z;
    m[1] = b2x; m[4] = b2y; m[7] = b2z;
    m[2] = b1y * b2z - b1z * b2y;
    m[5] = b1z * b2x - b1x * b2z;
    m[8] = b1x * b2y - b1y * b2x;
}

// safe_zero_division (utils/konia_transform.py:336-344)
__device__ inline float mv_szd(float num, float den) {
    if (fabsf(den) < 1e-6f) den += 1e-6f;
    return num / den;
}
// torch_safe_atan2 (:41-49)
__device__ inline float mv_safe_atan2(float y, float x) {
    if (fabsf(y) < 1e-6f && fabsf(x) < 1e-6f) y += 1e-6f;
    return atan2f(y, x);
}

// rotation_matrix_to_angle_axis (:631-655) = rotation_matrix_to_quaternion (:347-438, wxyz) then quaternion_to_angle_axis (:557-628)
__device__ inline void mv_rotmat_to_angle_axis(const float* m, float* aa) {
    const float m00 = m[0], m01 = m[1], m02 = m[2], m10 = m[3], m11 = m[4], m12 = m[5], m20 = m[6], m21 = m[7], m22 = m[8];
    const float trace = m00 + m11 + m22;
    float qw, qx, qy, qz;
    if (trace > 0.f) {
        const float sq = sqrtf(mv_clamp_min(trace + 1.f, 1e-6f)) * 2.f;
        qw = 0.25f * sq; qx = mv_szd(m21 - m12, sq); qy = mv_szd(m02 - m20, sq); qz = mv_szd(m10 - m01, sq);
    } else if (m00 > m11 && m00 > m22) {
        const float sq = sqrtf(mv_clamp_min(1.f + m00 - m11 - m22, 1e-6f)) * 2.f;
        qw = mv_szd(m21 - m12, sq); qx = 0.25f * sq; qy = mv_szd(m01 + m10, sq); qz = mv_szd(m02 + m20, sq);
    } else if (m11 > m22) {
        const float sq = sqrtf(mv_clamp_min(1.f + m11 - m00 - m22, 1e-6f)) * 2.f;
        qw = mv_szd(m02 - m20, sq); qx = mv_szd(m01 + m10, sq); qy = 0.25f * sq; qz = mv_szd(m12 + m21, sq);
    } else {
        const float sq = sqrtf(mv_clamp_min(1.f + m22 - m00 - m11, 1e-6f)) * 2.f;
        qw = mv_szd(m10 - m01, sq); qx = mv_szd(m02 + m20, sq); qy = mv_szd(m12 + m21, sq); qz = 0.25f * sq;
    }
    const float s2 = qx * qx + qy * qy + qz * qz;
    const float s = sqrtf(mv_clamp_min(s2, 1e-6f));
    const float two_theta = 2.f * (qw < 0.f ? mv_safe_atan2(-s, -qw) : mv_safe_atan2(s, qw));
    const float k = s2 > 0.f ? mv_szd(two_theta, s) : 2.f;
    aa[0] = qx * k; aa[1] = qy * k; aa[2] = qz * k;
}

// angle_axis_to_rotation_matrix (:282-333): the Rodrigues form above theta^2 = 1e-6, the first-order form below
__device__ inline void mv_angle_axis_to_rotmat(const float* aa, float* m) {
    const float rx = aa[0], ry = aa[1], rz = aa[2];
    const float theta2 = rx * rx + ry * ry + rz * rz;
    if (theta2 > 1e-6f) {
        const float theta = sqrtf(mv_clamp_min(theta2, 1e-6f));
        const float wx = rx / (theta + 1e-6f), wy = ry / (theta + 1e-6f), wz = rz / (theta + 1e-6f);
        const float c = cosf(theta), s = sinf(theta), t = 1.f - c;
        m[0] = c + wx * wx * t;        m[1] = wx * wy * t - wz * s;   m[2] = wy * s + wx * wz * t;
        m[3] = wz * s + wx * wy * t;   m[4] = c + wy * wy * t;        m[5] = -wx * s + wy * wz * t;
        m[6] = -wy * s + wx * wz * t;  m[7] = wx * s + wy * wz * t;   m[8] = c + wz * wz * t;
    } else {
        m[0] = 1.f; m[1] = -rz; m[2] = ry;
        m[3] = rz;  m[4] = 1.f; m[5] = -rx;
        m[6] = -ry; m[7] = rx;  m[8] = 1.f;
    }
}

__device__ inline float mv_elu(float x) { return x > 0.f ? x : expm1f(x); }

// ---------------------------------------------------------------------------------------------------------------- the product
// acc[e] += X[32 envs][K] * W_e[K][columns of `tile`] for E experts: X an LDS buffer in mv_perm layout with row stride xs, Wp the packed
// stack of `tiles` column tiles and `groups` = K / 8 k-groups (v2p_mvae_weights).  (Requesting the operands of group g + 1 by hand before
// the MFMAs of group g, over two register sets with scheduling barriers, was measured and is slower: 0.320 against 0.296 ms at 8192 envs.)
template <int E>
__device__ __forceinline__ void mv_product(const float* X, int xs, const float* Wp, int groups, int tiles, int tile, int lane, f32x16 (&acc)[E]) {
    const float4* xa = reinterpret_cast<const float4*>(X + (lane & 31) * xs + 4 * (lane >> 5));
    const float4* wb = reinterpret_cast<const float4*>(Wp) + (size_t)tile * groups * 64 + lane;
    const size_t estride = (size_t)tiles * groups * 64;
#pragma unroll 2
    for (int g = 0; g < groups; ++g) {
        const float4 a = xa[2 * g];
        float4 b[E];
#pragma unroll
        for (int e = 0; e < E; ++e) b[e] = wb[e * estride + (size_t)g * 64];
#pragma unroll
        for (int e = 0; e < E; ++e) acc[e] = __builtin_amdgcn_mfma_f32_32x32x2f32(a.x, b[e].x, acc[e], 0, 0, 0);
#pragma unroll
        for (int e = 0; e < E; ++e) acc[e] = __builtin_amdgcn_mfma_f32_32x32x2f32(a.y, b[e].y, acc[e], 0, 0, 0);
#pragma unroll
        for (int e = 0; e < E; ++e) acc[e] = __builtin_amdgcn_mfma_f32_32x32x2f32(a.z, b[e].z, acc[e], 0, 0, 0);
#pragma unroll
        for (int e = 0; e < E; ++e) acc[e] = __builtin_amdgcn_mfma_f32_32x32x2f32(a.w, b[e].w, acc[e], 0, 0, 0);
    }
}

// the env (row of the tile) of accumulator register r of a lane
__device__ inline int mv_acc_row(int r, int lane) { return (r & 3) + 8 * (r >> 2) + 4 * (lane >> 5); }

// one Linear layer of the gate: dst[row][mv_perm(col)] = act(X W + bias), tiles of 32 columns dealt to the waves
template <bool ELU>
__device__ __forceinline__ void mv_gate_layer(const float* X, int xs, const float* Wp, const float* bias, int K, int tiles, float* dst, int ds, bool perm, int wave, int lane) {
    for (int tile = wave; tile < tiles; tile += MV_THREADS / 64) {
        f32x16 acc[1] = {f32x16(0.f)};
        mv_product<1>(X, xs, Wp, K / 8, tiles, tile, lane, acc);
        const int col = tile * 32 + (lane & 31);
        const float bv = bias[col];
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const float v = acc[0][r] + bv;
            dst[mv_acc_row(r, lane) * ds + (perm ? mv_perm(col) : col)] = ELU ? mv_elu(v) : v;
        }
    }
}

// one expert-blended layer: dst[row][...] = act(sum_e coef[row][e] (X W_e + b_e)); N columns, Np = its tiles * 32 the padded width of bias
template <bool ELU>
__device__ __forceinline__ void mv_blend_layer(const float* X, const float* Wp, const float* bias, int K, int N, const float* coef, float* dst, int col0, bool perm, int wave,
                                      int lane) {
    const int tiles = (N + 31) / 32, Np = tiles * 32;
    for (int tile = wave; tile < tiles; tile += MV_THREADS / 64) {
        f32x16 acc[MV_EXPERTS];
#pragma unroll
        for (int e = 0; e < MV_EXPERTS; ++e) acc[e] = f32x16(0.f);
        mv_product<MV_EXPERTS>(X, MV_XS, Wp, K / 8, tiles, tile, lane, acc);
        const int col = tile * 32 + (lane & 31);
        float bv[MV_EXPERTS];
#pragma unroll
        for (int e = 0; e < MV_EXPERTS; ++e) bv[e] = bias[e * Np + col];
        if (col < N) {
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int row = mv_acc_row(r, lane);
                float v = coef[row * 8] * (acc[0][r] + bv[0]);
#pragma unroll
                for (int e = 1; e < MV_EXPERTS; ++e) v += coef[row * 8 + e] * (acc[e][r] + bv[e]);
                dst[row * MV_XS + (perm ? mv_perm(col0 + col) : col0 + col)] = ELU ? mv_elu(v) : v;
            }
        }
    }
}

// ---------------------------------------------------------------------------------------------------------------- the step
__global__ __launch_bounds__(MV_THREADS) void mvae_step_kernel(const MvArgs a) {
    __shared__ __attribute__((aligned(16))) float bufA[MV_TILE * MV_XS];
    __shared__ __attribute__((aligned(16))) float bufB[MV_TILE * MV_XS];
    __shared__ __attribute__((aligned(16))) float g1[MV_TILE * MV_GS];
    __shared__ __attribute__((aligned(16))) float g2[MV_TILE * MV_GS];
    __shared__ float coef[MV_TILE * 8];
    __shared__ float s_phase[MV_TILE];
    __shared__ int s_swing[MV_TILE];
    const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
    const int64_t env0 = (int64_t)blockIdx.x * MV_TILE;
    const int rows = (int)((a.n - env0) < MV_TILE ? (a.n - env0) : MV_TILE);

    // cat(z, condition) of the tile's envs (zeros for the rows past n); z goes into both buffers
    for (int i = t; i < MV_TILE * MV_IN0; i += MV_THREADS) {
        const int row = i / MV_IN0, k = i - row * MV_IN0;
        float v = 0.f;
        if (row < rows) v = k < MV_LATENT ? a.latents[(env0 + row) * MV_LATENT + k] : a.b.conditions[(env0 + row) * MV_FRAME + (k - MV_LATENT)];
        bufA[row * MV_XS + mv_perm(k)] = v;
        if (k < MV_LATENT) bufB[row * MV_XS + mv_perm(k)] = v;
    }
    __syncthreads();
    // the gate: 320 -> 64 -> 64 -> 6, ELU, softmax
    mv_gate_layer<true>(bufA, MV_XS, a.w.gate_w0, a.w.gate_b0, MV_IN0, MV_GATE / 32, g1, MV_GS, true, wave, lane);
    __syncthreads();
    mv_gate_layer<true>(g1, MV_GS, a.w.gate_w1, a.w.gate_b1, MV_GATE, MV_GATE / 32, g2, MV_GS, true, wave, lane);
    __syncthreads();
    mv_gate_layer<false>(g2, MV_GS, a.w.gate_w2, a.w.gate_b2, MV_GATE, 1, g1, MV_GS, false, wave, lane);  // (logits: columns 0..5 of g1)
    __syncthreads();
    if (t < MV_TILE) {
        float x[MV_EXPERTS], mx = g1[t * MV_GS];
        for (int e = 0; e < MV_EXPERTS; ++e) { x[e] = g1[t * MV_GS + e]; mx = x[e] > mx ? x[e] : mx; }
        float sum = 0.f;
        for (int e = 0; e < MV_EXPERTS; ++e) { x[e] = expf(x[e] - mx); sum += x[e]; }
        for (int e = 0; e < MV_EXPERTS; ++e) coef[t * 8 + e] = x[e] / sum;
    }
    __syncthreads();
    // the three blended layers
    mv_blend_layer<true>(bufA, a.w.w0, a.w.b0, MV_IN0, MV_HIDDEN, coef, bufB, MV_LATENT, true, wave, lane);
    __syncthreads();
    mv_blend_layer<true>(bufB, a.w.w1, a.w.b1, MV_IN1, MV_HIDDEN, coef, bufA, MV_LATENT, true, wave, lane);
    __syncthreads();
    mv_blend_layer<false>(bufA, a.w.w2, a.w.b2, MV_IN1, MV_OUT, coef, bufB, 0, false, wave, lane);
    __syncthreads();

    // ---- `_update_mvae_state(init=False)`: bufB[row][0..289] is the normalized feature and the two phase numbers
    const float* avg = a.w.avg;
    const float* sd = a.w.std;
    const bool residual = a.residual != nullptr;
    const int elbow = a.c.righthand ? 19 : 18, wrist = a.c.righthand ? 21 : 20;
    if (t < rows) {  // the env's scalars: root, phase, swing type
        const int64_t e = env0 + t;
        const float* o = bufB + t * MV_XS;
        for (int k = 0; k < 3; ++k) {
            const float vel = o[MV_COL_ROOT_VEL + k] * sd[MV_COL_ROOT_VEL + k] + avg[MV_COL_ROOT_VEL + k];
            const float pos = a.b.root_pos[e * 3 + k] + vel;
            a.b.root_pos[e * 3 + k] = pos;
            a.b.root_vel[e * 3 + k] = vel;
            a.b.conditions[e * MV_FRAME + k] = (pos - avg[k]) / sd[k];
        }
        float ph = atan2f(o[MV_FRAME], o[MV_FRAME + 1]);
        if (ph < 0.f) ph = ph + 2.f * MV_PI;
        int64_t st = a.b.swing_type[e];
        const int col = MV_COL_JOINT_POS + (MV_RWRIST - 1) * 3;  // the RIGHT wrist's x, whatever the hand
        const float wx = o[col] * sd[col] + avg[col];
        if (st == -1 && ph > 2.0f && ph < 3.5f) st = (wx > 0.f) == (a.c.righthand != 0) ? 1 : 2;
        if (st != -1 && ph > 3.5f) st = -1;
        a.b.phase_pred[e] = ph;
        a.b.swing_type[e] = st;
        if (st != -1) a.b.swing_type_cycle[e] = st;
        s_phase[t] = ph;
        s_swing[t] = (int)st;
    }
    // columns, coalesced over the tile: the condition (its root columns are written above) and the rot6d of the joints no residual rewrites
    for (int i = t; i < rows * MV_FRAME; i += MV_THREADS) {
        const int row = i / MV_FRAME, k = i - row * MV_FRAME;
        const float v = bufB[row * MV_XS + k];
        if (k >= 3) a.b.conditions[(env0 + row) * MV_FRAME + k] = v;
        if (k >= MV_COL_ROT6D) {
            const int j = (k - MV_COL_ROT6D) / 6;
            if (!(residual && (j == elbow || j == wrist))) a.b.joint_rot6d[(env0 + row) * (MV_JOINTS * 6) + (k - MV_COL_ROT6D)] = v * sd[k] + avg[k];
        }
    }
    __syncthreads();
    // joints: thread (row, sub) takes joints sub, sub + 8, sub + 16
    const int row = t >> 3, sub = t & 7;
    if (row < rows) {
        const int64_t e = env0 + row;
        const float* o = bufB + row * MV_XS;
        for (int j = sub; j < MV_JOINTS; j += 8) {
            float r6[6], m[9];
            for (int k = 0; k < 6; ++k) { const int col = MV_COL_ROT6D + j * 6 + k; r6[k] = o[col] * sd[col] + avg[col]; }
            mv_rot6d_to_rotmat(r6, m);
            const bool is_elbow = j == elbow, is_wrist = j == wrist;
            if (residual && (is_elbow || is_wrist)) {
                const MvPlayer& P = MV_PLAYERS[a.c.player];
                const float ph = s_phase[row];
                const int st = s_swing[row];
                float res[3], base[4] = {0.f, 0.f, 0.f, 0.f};
                for (int k = 0; k < 3; ++k) {
                    const float v = a.residual[e * 3 + k] * 0.25f;
                    res[k] = v < -0.25f ? -0.25f : (v > 0.25f ? 0.25f : v);
                }
                for (int w = 0; w < P.rows; ++w) {
                    const MvWindow& W = P.w[w];
                    if (st == W.swing && (W.ge ? ph >= W.lo : ph > W.lo) && ph < W.hi)
                        for (int k = 0; k < 4; ++k)
                            if (W.set >> k & 1) base[k] = W.base[k];
                }
                if (!a.c.is_train) {
                    const bool swing = (st == 1 && ph > P.fh_lo && ph < P.fh_hi) || (st == 2 && ph > P.bh_lo && ph < P.bh_hi);
                    if (!swing) res[0] = res[1] = res[2] = 0.f;
                }
                float aa[3];
                mv_rotmat_to_angle_axis(m, aa);
                if (is_elbow) {
                    aa[0] = (base[0] + res[0]) * MV_PI;
                } else {
                    aa[0] = base[1] * MV_PI;
                    aa[1] = (base[2] + res[1]) * MV_PI;
                    aa[2] = (base[3] + res[2]) * MV_PI;
                }
                mv_angle_axis_to_rotmat(aa, m);
                r6[0] = m[0]; r6[1] = m[3]; r6[2] = m[6]; r6[3] = m[1]; r6[4] = m[4]; r6[5] = m[7];
                for (int k = 0; k < 6; ++k) a.b.joint_rot6d[e * (MV_JOINTS * 6) + j * 6 + k] = r6[k];
            }
            for (int k = 0; k < 9; ++k) a.b.joint_rotmat[e * (MV_JOINTS * 9) + j * 9 + k] = m[k];
            if (!a.c.is_train) {  // rot6d_to_angle_axis of the rot6d as stored: of a rewritten joint, its new two columns
                float m2[9], aa[3];
                if (residual && (is_elbow || is_wrist)) mv_rot6d_to_rotmat(r6, m2);
                else for (int k = 0; k < 9; ++k) m2[k] = m[k];
                mv_rotmat_to_angle_axis(m2, aa);
                for (int k = 0; k < 3; ++k) a.b.joint_rot[e * (MV_JOINTS * 3) + j * 3 + k] = aa[k];
            }
        }
    }
}

// ---------------------------------------------------------------------------------------------------------------- the reset
// one wave per id: lanes stride the columns, lanes 0..23 take a joint each, lane 0 walks the racket's chain
__global__ __launch_bounds__(256) void mvae_reset_kernel(const MvArgs a) {
    const int lane = threadIdx.x & 63;
    const int64_t i = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (i >= a.n) return;  // (the whole wave)
    const int64_t e = a.env_ids[i];
    if (e < 0 || e >= a.num_envs) return;
    const float* f = a.init_feature + i * MV_FRAME;
    const float* avg = a.w.avg;
    const float* sd = a.w.std;
    float root[3] = {a.root_xy[i * 2], a.root_xy[i * 2 + 1], f[2]};
    for (int k = lane; k < MV_FRAME; k += 64) {
        const float v = k < 2 ? a.root_xy[i * 2 + k] : f[k];  // (the root's z is the feature's)
        a.b.conditions[e * MV_FRAME + k] = (v - avg[k]) / sd[k];
        if (k < 3) a.b.root_pos[e * 3 + k] = v;
        else if (k < 6) a.b.root_vel[e * 3 + (k - 3)] = v;
        if (k >= MV_COL_ROT6D) a.b.joint_rot6d[e * (MV_JOINTS * 6) + (k - MV_COL_ROT6D)] = v;
    }
    if (lane == 0) { a.b.swing_type[e] = -1; a.b.swing_type_cycle[e] = -1; }
    if (lane < MV_JOINTS) {
        float m[9], aa[3];
        mv_rot6d_to_rotmat(f + MV_COL_ROT6D + lane * 6, m);
        for (int k = 0; k < 9; ++k) a.b.joint_rotmat[e * (MV_JOINTS * 9) + lane * 9 + k] = m[k];
        if (!a.c.is_train) {
            mv_rotmat_to_angle_axis(m, aa);
            for (int k = 0; k < 3; ++k) a.b.joint_rot[e * (MV_JOINTS * 3) + lane * 3 + k] = aa[k];
        }
    }
    if (lane == 0) {
        // infer_racket_with_fk (utils/racket.py:235-269): the chain of 4x4 transforms Pelvis .. Hand, products in matmul's order
        const int rh = a.c.righthand != 0;
        const int chain[9] = {0, 3, 6, 9, rh ? 14 : 13, rh ? 17 : 16, rh ? 19 : 18, rh ? 21 : 20, rh ? 23 : 22};
        float R[9], p[3];
        mv_rot6d_to_rotmat(f + MV_COL_ROT6D, R);
        for (int k = 0; k < 3; ++k) p[k] = a.bind[k];
        for (int c = 1; c < 8; ++c) {  // (up to the wrist: the hand's transform is not read by `infer_with_fk`)
            float m[9], Rn[9], pn[3];
            const int j = chain[c];
            mv_rot6d_to_rotmat(f + MV_COL_ROT6D + j * 6, m);
            for (int r = 0; r < 3; ++r) {
                for (int q = 0; q < 3; ++q) Rn[r * 3 + q] = R[r * 3] * m[q] + R[r * 3 + 1] * m[3 + q] + R[r * 3 + 2] * m[6 + q];
                pn[r] = R[r * 3] * a.bind[j * 3] + R[r * 3 + 1] * a.bind[j * 3 + 1] + R[r * 3 + 2] * a.bind[j * 3 + 2] + p[r];
            }
            for (int k = 0; k < 9; ++k) R[k] = Rn[k];
            for (int k = 0; k < 3; ++k) p[k] = pn[k];
        }
        // the eastern racket: direction (-1, 0, 0), normal (0, 1, 0) in the wrist's frame; handle 0.2, shaft 0.15, head radius 0.15
        for (int r = 0; r < 3; ++r) {
            const float dir = R[r * 3] * -1.f + R[r * 3 + 1] * 0.f + R[r * 3 + 2] * 0.f;
            const float nrm = R[r * 3] * 0.f + R[r * 3 + 1] * 1.f + R[r * 3 + 2] * 0.f;
            const float wr = p[r] + root[r];
            a.b.racket_pos[e * 3 + r] = ((wr + dir * 0.2f) + dir * 0.15f) + dir * 0.15f;
            a.b.racket_normal[e * 3 + r] = nrm;
        }
    }
}

}  // namespace

int launch_mvae_step(const v2p_mvae_cfg& c, int64_t n, const v2p_mvae_weights& w, const v2p_mvae_buffers& b, const float* latents, const float* residual,
                     hipStream_t s) {
    MvArgs a = {};
    a.c = c; a.w = w; a.b = b;
    a.latents = latents; a.residual = residual;
    a.n = a.num_envs = n;
    const dim3 grid((unsigned)((n + MV_TILE - 1) / MV_TILE)), block(MV_THREADS);
    hipLaunchKernelGGL(mvae_step_kernel, grid, block, 0, s, a);
    return check_hip(hipGetLastError(), "mvae_step_kernel");
}

int launch_mvae_reset(const v2p_mvae_cfg& c, int64_t num_envs, const v2p_mvae_weights& w, const v2p_mvae_buffers& b, const int64_t* env_ids, int64_t n_ids,
                      const float* init_feature, const float* root_xy, const float* joint_pos_bind_rel, hipStream_t s) {
    MvArgs a = {};
    a.c = c; a.w = w; a.b = b;
    a.env_ids = env_ids; a.init_feature = init_feature; a.root_xy = root_xy; a.bind = joint_pos_bind_rel;
    a.n = n_ids; a.num_envs = num_envs;
    const dim3 grid((unsigned)((n_ids + 3) / 4)), block(256);
    hipLaunchKernelGGL(mvae_reset_kernel, grid, block, 0, s, a);
    return check_hip(hipGetLastError(), "mvae_reset_kernel");
}

}  // namespace v2p
