// The host-side compiler of a body model: v2p_model_desc -> DevModel, the tree tables and the padded hull lists as the kernels read them.
// Pure host code: it validates and computes, and makes no GPU call (v2p_model_create uploads the result).
#include <math.h>
#include <string.h>

#include "v2p_internal.hpp"

namespace v2p {

int compile_model(const v2p_model_desc& d, DevModel* out) {
    if (d.num_bodies != NB) { set_error("v2p_model_create: num_bodies must be %d, got %d", NB, d.num_bodies); return V2P_ERR_UNSUPPORTED; }
    if (d.hull_offsets[NB] > MAX_HULL_VERTS) { set_error("v2p_model_create: %d hull vertices exceed the limit %d", d.hull_offsets[NB], MAX_HULL_VERTS); return V2P_ERR_UNSUPPORTED; }
    memset(out, 0, sizeof(*out));
    DevModel& h = *out;
    for (int b = 0; b < NB; ++b) {
        int p = d.parents[b];
        if ((b == 0 && p != -1) || (b > 0 && (p < 0 || p >= b))) {
            set_error("v2p_model_create: parents must be topologically ordered with a single root (body %d has parent %d)", b, p);
            return V2P_ERR_INVALID;
        }
        h.parents[b] = p;
        h.depth[b] = b == 0 ? 0 : h.depth[p] + 1;
        if (h.depth[b] >= MAX_DEPTH) { set_error("v2p_model_create: tree depth exceeds %d", MAX_DEPTH); return V2P_ERR_UNSUPPORTED; }
        for (int k = 0; k < 3; ++k) { h.shape.local_pos[b][k] = d.local_pos[3 * b + k]; h.shape.com[b][k] = d.com[3 * b + k]; }
        h.shape.mass[b] = d.mass[b];
        const float* I = d.inertia + 9 * b;
        h.shape.inertia[b][0] = I[0]; h.shape.inertia[b][1] = 0.5f * (I[1] + I[3]); h.shape.inertia[b][2] = 0.5f * (I[2] + I[6]);
        h.shape.inertia[b][3] = I[4]; h.shape.inertia[b][4] = 0.5f * (I[5] + I[7]); h.shape.inertia[b][5] = I[8];
        if (b > 0) {
            const float *kp = d.kp + 3 * (b - 1), *kd = d.kd + 3 * (b - 1), *ar = d.armature + 3 * (b - 1);
            if (kp[0] != kp[1] || kp[0] != kp[2] || kd[0] != kd[1] || kd[0] != kd[2] || ar[0] != ar[1] || ar[0] != ar[2]) {
                set_error("v2p_model_create: joint of body %d has per-axis gains; only isotropic spherical-joint gains are built", b);
                return V2P_ERR_UNSUPPORTED;
            }
            h.shape.kp[b] = kp[0]; h.shape.kd[b] = kd[0]; h.shape.arm[b] = ar[0];
        }
        for (int k = 0; k < 3; ++k) {
            h.shape.limit_lo[b][k] = b > 0 && d.limit_lower ? d.limit_lower[3 * (b - 1) + k] : -3.14159265f;
            h.shape.limit_hi[b][k] = b > 0 && d.limit_upper ? d.limit_upper[3 * (b - 1) + k] : 3.14159265f;
            if (!(h.shape.limit_lo[b][k] <= h.shape.limit_hi[b][k])) { set_error("v2p_model_create: body %d: joint range is empty", b); return V2P_ERR_INVALID; }
        }
    }
    {
        int off = 0;
        for (int b = 0; b < NB; ++b) {
            int n = d.hull_offsets[b + 1] - d.hull_offsets[b];
            int np = (n + HULL_PAD - 1) / HULL_PAD * HULL_PAD;
            if (n < 1 || n > 64) { set_error("v2p_model_create: body %d has %d hull vertices (1..64 supported)", b, n); return V2P_ERR_UNSUPPORTED; }
            if (off + np > MAX_HULL_VERTS) { set_error("v2p_model_create: padded hull vertices exceed the limit %d", MAX_HULL_VERTS); return V2P_ERR_UNSUPPORTED; }
            h.shape.hull_offsets[b] = off;
            h.shape.hull_count[b] = n;
            float r2 = 0.f, lo[3] = {1e30f, 1e30f, 1e30f}, hi[3] = {-1e30f, -1e30f, -1e30f};
            for (int v = 0; v < np; ++v) {
                const float* src = d.hull_verts + 3 * (d.hull_offsets[b] + (v < n ? v : n - 1));
                for (int k = 0; k < 3; ++k) {
                    h.shape.hull_verts[off + v][k] = src[k];
                    lo[k] = src[k] < lo[k] ? src[k] : lo[k];
                    hi[k] = src[k] > hi[k] ? src[k] : hi[k];
                }
                float n2 = src[0] * src[0] + src[1] * src[1] + src[2] * src[2];
                if (n2 > r2) r2 = n2;
            }
            h.shape.bound_radius[b] = sqrtf(r2);
            for (int k = 0; k < 3; ++k) { h.shape.aabb_c[b][k] = 0.5f * (lo[k] + hi[k]); h.shape.aabb_e[b][k] = 0.5f * (hi[k] - lo[k]) * 1.0001f + 1e-6f; }
            off += np;
        }
        h.shape.hull_offsets[NB] = off;
        h.shape.hull_cofs[0] = 0;
        for (int b = 0; b < NB; ++b) h.shape.hull_cofs[b + 1] = h.shape.hull_cofs[b] + h.shape.hull_count[b];
    }
    {
        int k = 0;
        for (int dpt = 0; dpt < MAX_DEPTH; ++dpt)
            for (int b = 0; b < NB; ++b)
                if (h.depth[b] == dpt) h.order[k++] = b;
    }
    {
        int nch[NB] = {0};
        h.max_depth = 0;
        h.multi_child_levels = 0;
        h.nonchain_levels = 0;
        h.max_hull_count = 0;
        for (int b = 0; b < NB; ++b) {
            for (int k = 0; k < 3; ++k) h.children[b][k] = -1;
            h.anc_mask[b] = 1 << b;
            if (h.depth[b] > h.max_depth) h.max_depth = h.depth[b];
            if (h.shape.hull_count[b] > h.max_hull_count) h.max_hull_count = h.shape.hull_count[b];
        }
        for (int b = 1; b < NB; ++b) {
            int p = h.parents[b];
            if (nch[p] >= 3) { set_error("v2p_model_create: link %d has more than 3 children", p); return V2P_ERR_UNSUPPORTED; }
            h.children[p][nch[p]++] = b;
            if (nch[p] > 1) h.multi_child_levels |= 1 << h.depth[b];
            h.anc_mask[b] |= h.anc_mask[p];
            if (p != b - 1) h.nonchain_levels |= 1 << h.depth[b];
            if (h.children[p][0] != p + 1) { set_error("v2p_model_create: links must be in depth-first order (first child of %d is %d)", p, h.children[p][0]); return V2P_ERR_UNSUPPORTED; }
        }
    }
    if (h.max_depth > 15) { set_error("v2p_model_create: tree deeper than 15 levels"); return V2P_ERR_UNSUPPORTED; }
    h.jump_rounds = 0;
    while ((1 << h.jump_rounds) <= h.max_depth) ++h.jump_rounds;
    for (int b = 0; b < NB; ++b) {
        h.anc_jump[b] = 0;
        for (int k = 0; k < 4; ++k) {
            int a = b, steps = 1 << k;
            while (steps > 0 && a > 0) { a = h.parents[a]; --steps; }
            h.anc_jump[b] = (int32_t)((uint32_t)h.anc_jump[b] | ((uint32_t)((steps == 0 && b != 0) ? a : 255) << (8 * k)));
        }
    }
    h.side_depths[0] = 0;
    for (int b = 1; b < NB; ++b) h.side_depths[b] = h.side_depths[h.parents[b]] | ((h.parents[b] != b - 1) ? 1 << h.depth[b] : 0);
    for (int b = 0; b < NB; ++b) {
        h.desc_mask[b] = 0;
        for (int j = 0; j < NB; ++j)
            if ((h.anc_mask[j] >> b) & 1) h.desc_mask[b] |= 1 << j;
    }
    {
        int nslot = 1;
        for (int b = 0; b < NB; ++b) h.lam_slot[b] = -1;
        h.lam_slot[0] = 0;
        for (int b = 1; b < NB; ++b) {
            // a child that does not directly follow its parent needs the parent's Lambda from a saved slot
            int p = h.parents[b];
            if (p != b - 1 && h.lam_slot[p] < 0) {
                if (nslot >= MAX_BRANCH) { set_error("v2p_model_create: more than %d branching links", MAX_BRANCH); return V2P_ERR_UNSUPPORTED; }
                h.lam_slot[p] = nslot++;
            }
        }
    }
    return V2P_OK;
}

}  // namespace v2p
