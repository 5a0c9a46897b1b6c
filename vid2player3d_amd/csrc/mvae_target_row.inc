// The body of the imitation target's row kernel as TEXT, included by mvae_target_kernel<RESET> (mvae_target.hip) and by the reset by
// flags (flag_reset.hip).  Text and not a function template because mvae_target_kernel must stay the machine code it was
// (tools/kernel_identity.py): included with that kernel's definitions the text is, token for token, what it held.  Reads a (MtArgs),
// RESET (a compile-time bool: no head rule, no previous pose, the engine's state rows written) and
//   MT_ROW_ENV(i)                 the env of row i of the launch, i < a.n; an env outside 0 .. num_envs-1 has no live lanes
// Every lane of the workgroup reaches the barrier: lanes of a slot without a live env run along on env 0 and store nothing.
    __shared__ float s_row[MT_ENVS][MT_ROW];
    const int j = threadIdx.x & (MT_LANES - 1), slot = threadIdx.x / MT_LANES;
    const int64_t i = (int64_t)blockIdx.x * MT_ENVS + slot;
    int64_t e = -1;
    if (i < a.n) e = MT_ROW_ENV(i);
    // lanes of a slot without an env run along on env 0, for the shuffles and the barrier.  What they read there may be in the middle of
    // being written (env 0's own slot, perhaps in another workgroup, writes Head and Neck back into joint_rotmat): a race by design,
    // harmless because nothing computed from it is stored - every global store below is under `live`
    const bool live = e >= 0 && e < a.num_envs;
    const int64_t er = live ? e : 0;
    const bool joint = j < MT_JOINTS;
    const int jj = joint ? j : 0;
    const v2p_mvae_target_buffers& b = a.b;

    // the lane's place in the tree (a select chain over the launch's uniform tables)
    int parent = -1, depth = 0, body = 0;
#pragma unroll
    for (int k = 0; k < MT_JOINTS; ++k)
        if (k == jj) { parent = a.c.smpl_parents[k]; depth = a.depth[k]; body = a.body_of_smpl[k]; }
    const int src = parent < 0 ? jj : parent;

    int shape = b.env_shape_id ? b.env_shape_id[er] : 0;
    shape = shape < 0 ? 0 : (shape >= a.c.num_shapes ? a.c.num_shapes - 1 : shape);
    const float* bind = b.joint_pos_bind + (size_t)shape * (MT_JOINTS * 3);
    float m[9], rel[3], root[3], bind0[3];
#pragma unroll
    for (int k = 0; k < 9; ++k) m[k] = b.joint_rotmat[er * (MT_JOINTS * 9) + jj * 9 + k];
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        bind0[k] = bind[k];
        rel[k] = bind[jj * 3 + k];
        if (parent >= 0) rel[k] = rel[k] - bind[parent * 3 + k];
        root[k] = b.root_pos[er * 3 + k];
        if (!RESET && b.residual_root) root[k] = root[k] + b.residual_root[er * 3 + k];
    }

    float R[9], p[3];
#pragma unroll
    for (int k = 0; k < 9; ++k) R[k] = m[k];
#pragma unroll
    for (int k = 0; k < 3; ++k) p[k] = rel[k];
    mt_chain(1, a.max_depth, depth, src, m, rel, R, p);

    if (!RESET && a.c.fix_head_orientation) {
        // the head rule (:605-634), by every lane on its own transform; the head's lane has the answer
        float q[4];
        ref_rotmat_to_quat(R, q);
        // quaternion_to_rotation_matrix (utils/konia_transform.py:474-549) x (0, 0, 1): the third column's x and y
        const float qn = ref_clamp_min(sqrtf(q[0] * q[0] + q[1] * q[1] + q[2] * q[2] + q[3] * q[3]), 1e-12f);
        const float w = q[0] / qn, x = q[1] / qn, y = q[2] / qn, z = q[3] / qn;
        const float tx = 2.f * x, ty = 2.f * y, tz = 2.f * z;
        float l0 = tz * x + ty * w, l1 = tz * y - tx * w;
        const float ln = ref_clamp_min(sqrtf(l0 * l0 + l1 * l1), 1e-12f);
        l0 = l0 / ln; l1 = l1 / ln;
        const float ball_x = b.ball_state[er * 13], ball_y = b.ball_state[er * 13 + 1];
        float h0 = ball_x - (p[0] - (bind0[0] - root[0])), h1 = ball_y - (p[1] - (bind0[1] - root[1]));
        const float hn = ref_clamp_min(sqrtf(h0 * h0 + h1 * h1), 1e-12f);
        h0 = h0 / hn; h1 = h1 / hn;
        float diff = atan2f(h1, h0) - atan2f(l1, l0);
        if (diff > MT_PI) diff = diff - 2.f * MT_PI;
        if (diff < -MT_PI) diff = diff + 2.f * MT_PI;
        const float sim_root_y = b.rb_state[er * (NB * 13) + 1];
        if ((ball_y < sim_root_y - 0.5f) || (fabsf(ball_x) > 4.f)) diff = 0.f;  // no need to correct the head if it is a miss
        diff = __shfl(diff, a.c.smpl_head, MT_LANES);
        if (joint && (j == a.c.smpl_head || j == a.c.smpl_neck)) {
            float aa[3];
            ref_rotmat_to_angle_axis(m, aa);
            aa[1] = aa[1] + diff / 2.f;
            ref_angle_axis_to_rotmat(aa, m);
            if (live) {
#pragma unroll
                for (int k = 0; k < 9; ++k) b.joint_rotmat[e * (MT_JOINTS * 9) + j * 9 + k] = m[k];
            }
        }
        mt_chain(a.fix_lo, a.fix_hi, depth, src, m, rel, R, p);
    }

    // ---- `_smpl_to_sim` of the lane's joint into the staged row, in the engine's body order
    float* row = s_row[slot];
    if (joint) {
        float q[4], aa[3];
        ref_rotmat_to_quat(R, q);
        ref_rotmat_to_angle_axis(m, aa);
        const float cur[4] = {q[1], q[2], q[3], q[0]};
#pragma unroll
        for (int k = 0; k < 4; ++k) row[MS_RB_ROT + 4 * body + k] = cur[k];
#pragma unroll
        for (int k = 0; k < 3; ++k) row[MS_RB_POS + 3 * body + k] = p[k] - (bind0[k] - root[k]);
        float v[3] = {0.f, 0.f, 0.f};
        if (!RESET) {
            float prev[4];
#pragma unroll
            for (int k = 0; k < 4; ++k) prev[k] = b.prev_target[er * MSD + MS_RB_ROT + 4 * body + k];
            mt_quat_diff_velocity(prev, cur, a.c.dt, v);
        }
        if (body > 0) {
#pragma unroll
            for (int k = 0; k < 3; ++k) {
                row[MS_DOF_POS + 3 * (body - 1) + k] = aa[k];
                row[MS_DOF_VEL + 3 * (body - 1) + k] = v[k];
            }
        } else {
#pragma unroll
            for (int k = 0; k < 4; ++k) row[MS_ROOT_ROT + k] = cur[k];
#pragma unroll
            for (int k = 0; k < 3; ++k) {
                row[MS_ROOT_POS + k] = root[k];
                row[MS_ROOT_VEL + k] = RESET ? 0.f : (root[k] - b.prev_target[er * MSD + MS_ROOT_POS + k]) / a.c.dt;
                row[MS_ROOT_ANG_VEL + k] = v[k] / a.c.dt;  // (divided by dt once more, as the reference has it, :919)
            }
        }
    }
    __syncthreads();
    if (!live) return;

    // ---- the env's 32 lanes stride the row; key_pos is rb_pos of the key bodies
    float* out = b.target + e * MSD;
    for (int col = j; col < MSD; col += MT_LANES) {
        int from = col;
        if (col >= MS_KEY_POS && col < MS_RB_POS) {
            const int k = (col - MS_KEY_POS) / 3;
            const int kb = k == 0 ? a.c.key_bodies[0] : (k == 1 ? a.c.key_bodies[1] : (k == 2 ? a.c.key_bodies[2] : a.c.key_bodies[3]));
            from = MS_RB_POS + 3 * kb + (col - MS_KEY_POS - 3 * k);
        }
        out[col] = row[from];
    }
    if (RESET) {  // `_set_env_state` (:477-490): pose, zero velocities
        if (b.root_states && j < 13) b.root_states[e * 13 + j] = j < 7 ? row[j] : 0.f;  // (root_pos and root_rot open the row)
        if (b.dof_state)
            for (int k = j; k < NDOF * 2; k += MT_LANES) b.dof_state[e * (NDOF * 2) + k] = (k & 1) ? 0.f : row[MS_DOF_POS + (k >> 1)];
        if (b.rb_state)
            for (int k = j; k < NB * 13; k += MT_LANES) {
                const int bd = k / 13, c = k - bd * 13;
                b.rb_state[e * (NB * 13) + k] = c < 3 ? row[MS_RB_POS + 3 * bd + c] : (c < 7 ? row[MS_RB_ROT + 4 * bd + (c - 3)] : 0.f);
            }
    } else if (j == 0) {
        if (b.hold_reset) b.hold_reset[e] = 0;
        if (b.hold_progress) b.hold_progress[e] = 0;
        if (b.hold_cur_time) b.hold_cur_time[e] = 0.f;
    }
