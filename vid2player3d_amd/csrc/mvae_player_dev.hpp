// What the kernels of the MotionVAE motion generator share: sizes, the residual-DoF tables, the rotation conversions and the MFMA layers.
// Included by mvae_player.hip (one player) and mvae_player_dual.hip (two players, a weight set per side).  The two are separate
// translation units on purpose: with the two-player kernels in the same unit the compiler lays mvae_step_kernel out differently
// (7346 against 7309 instructions, the same text), and that kernel must stay the machine code it was (tools/kernel_identity.py).
#pragma once
#include "mvae_player.hpp"
#include "ref_rotations.hpp"

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
// the eastern tennis racket's canonical direction and normal (utils/racket.py:10-19), as the tokens the single player's reset multiplies by
#define MV_EASTERN_DIR_0 -1.f
#define MV_EASTERN_DIR_1 0.f
#define MV_EASTERN_DIR_2 0.f
#define MV_EASTERN_NORMAL_0 0.f
#define MV_EASTERN_NORMAL_1 1.f
#define MV_EASTERN_NORMAL_2 0.f

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
// (clamp_min, safe_zero_division, quaternion -> angle-axis, angle-axis -> matrix: ref_rotations.hpp)
__device__ inline float mv_norm3(float x, float y, float z) { return sqrtf(x * x + y * y + z * z); }

// rot6d_to_rotmat (utils/torch_transform.py:221-235) with its two eps = 1e-8 fallbacks; m row-major, columns b1 b2 b3
__device__ inline void mv_rot6d_to_rotmat(const float* r, float* m) {
    float ax = r[0], ay = r[1], az = r[2];
    const float cx = r[3], cy = r[4], cz = r[5];
    if (mv_norm3(ax, ay, az) < 1e-8f) { ax = 1.f; ay = 0.f; az = 0.f; }
    const float n1 = ref_clamp_min(mv_norm3(ax, ay, az), 1e-9f);
    const float b1x = ax / n1, b1y = ay / n1, b1z = az / n1;
    const float d = b1x * cx + b1y * cy + b1z * cz;
    const float ux = cx - d * b1x, uy = cy - d * b1y, uz = cz - d * b1z;
    const float n2 = ref_clamp_min(mv_norm3(ux, uy, uz), 1e-9f);
    float b2x = ux / n2, b2y = uy / n2, b2z = uz / n2;
    if (mv_norm3(b2x, b2y, b2z) < 1e-8f) { b2x = 0.f; b2y = 1.f; b2z = 0.f; }
    m[0] = b1x; m[3] = b1y; m[6] = b1z;
    m[1] = b2x; m[4] = b2y; m[7] = b2z;
    m[2] = b1y * b2z - b1z * b2y;
    m[5] = b1z * b2x - b1x * b2z;
    m[8] = b1x * b2y - b1y * b2x;
}

// rotation_matrix_to_angle_axis (utils/konia_transform.py:631-655) with the table of rotation_matrix_to_quaternion (:347-438, wxyz) in
// locals: the second statement of that table, kept because ref_rotations.hpp's form moves these kernels (see there)
__device__ inline void mv_rotmat_to_angle_axis(const float* m, float* aa) {
    const float m00 = m[0], m01 = m[1], m02 = m[2], m10 = m[3], m11 = m[4], m12 = m[5], m20 = m[6], m21 = m[7], m22 = m[8];
    const float trace = m00 + m11 + m22;
    float qw, qx, qy, qz;
    if (trace > 0.f) {
        const float sq = sqrtf(ref_clamp_min(trace + 1.f, 1e-6f)) * 2.f;
        qw = 0.25f * sq; qx = ref_szd(m21 - m12, sq); qy = ref_szd(m02 - m20, sq); qz = ref_szd(m10 - m01, sq);
    } else if (m00 > m11 && m00 > m22) {
        const float sq = sqrtf(ref_clamp_min(1.f + m00 - m11 - m22, 1e-6f)) * 2.f;
        qw = ref_szd(m21 - m12, sq); qx = 0.25f * sq; qy = ref_szd(m01 + m10, sq); qz = ref_szd(m02 + m20, sq);
    } else if (m11 > m22) {
        const float sq = sqrtf(ref_clamp_min(1.f + m11 - m00 - m22, 1e-6f)) * 2.f;
        qw = ref_szd(m02 - m20, sq); qx = ref_szd(m01 + m10, sq); qy = 0.25f * sq; qz = ref_szd(m12 + m21, sq);
    } else {
        const float sq = sqrtf(ref_clamp_min(1.f + m22 - m00 - m11, 1e-6f)) * 2.f;
        qw = ref_szd(m10 - m01, sq); qx = ref_szd(m02 + m20, sq); qy = ref_szd(m12 + m21, sq); qz = 0.25f * sq;
    }
    const float q[4] = {qw, qx, qy, qz};
    ref_quat_to_angle_axis(q, aa);
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

}  // namespace

}  // namespace v2p
