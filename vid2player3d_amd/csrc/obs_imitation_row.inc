// The 734-d in-network imitation observation, body j's share of one row - shared by obs_imitation_kernel (task_ops.hip) and
// ll_policy_input_kernel (policy_io.hip), so that both round alike (no include guard, no namespace: see v2p_math.inc).  Needs
// v2p_math.inc, motion_sample.inc and post_ops.inc in the same namespace.
// (humanoid_smpl_im.py:773-850, next row f-1)
// layout: root_h 1 | local_body_pos 69 | local_body_rot 144 | local_vel 72 | local_ang_vel 72 | dof_vel 69 |
//         rel_root_h 1 | rel_root_rot 6 | rel_2d_pos 2 | rel_heading 2 | rel_dof 69 | rel_body_pos 72 | rel_body_rot 144 | motion_bodies 11
//
// Row r of the inputs: element pointers + row strides (floats), so that the same code reads either nine separate contiguous
// tensors or the packed 461-d observation row + the 378-d context frame the network is handed (im_network_builder.py:150-189),
// or the engine's own state tensors in place.
struct ObsImSrc {
    const float *body_pos, *body_rot, *dof_pos, *dof_vel, *body_vel, *body_ang_vel, *motion_bodies;  // per row
    int64_t s_body_pos, s_body_rot, s_dof_pos, s_dof_vel, s_body_vel, s_body_ang_vel, s_motion_bodies;
    const float *tgt_pos, *tgt_rot, *tgt_dof_pos;  // per row, or (steps > 1 / context) per (env, frame)
    int64_t s_tgt_pos, s_tgt_rot, s_tgt_dof_pos;   // stride between FRAMES of the target
    int64_t steps, ctx_frames, first_frame;         // row r = env * steps + k reads target frame env * ctx_frames + first_frame + k
};

// floats between the bodies of a row's state (position, rotation, velocity, angular velocity) and between its DoF values
struct ObsImDense {   // [.,24,3] / [.,24,4] / [.,69] tensors
    static constexpr int POS = 3, ROT = 4, VEL = 3, ANG = 3, DOF = 1;
};
struct ObsImEngine {  // the engine's `_rigid_body_state` [.,24,13] (pos 3 | rot 4 | vel 3 | ang vel 3) and `_dof_state` [.,69,2] (pos | vel)
    static constexpr int POS = 13, ROT = 13, VEL = 13, ANG = 13, DOF = 2;
};

template <typename L>
__device__ __forceinline__ V3 obs_im_ld_dof(const float* p) {
    if constexpr (L::DOF == 1) return ld3(p);
    else return V3{p[0], p[L::DOF], p[2 * L::DOF]};
}

// the row's target pieces are dense in every layout (separate tensors, a context frame, the packed target row)
template <typename L>
__device__ __forceinline__ void obs_imitation_row(const ObsImSrc& in, int64_t e, int j, float* o) {
    const int64_t tf = (e / in.steps) * in.ctx_frames + in.first_frame + e % in.steps;  // target frame of this row
    const float* body_pos = in.body_pos + e * in.s_body_pos;
    const float* body_rot = in.body_rot + e * in.s_body_rot;
    const float* tgt_pos = in.tgt_pos + tf * in.s_tgt_pos;
    const float* tgt_rot = in.tgt_rot + tf * in.s_tgt_rot;
    V3 root_pos = ld3(body_pos);
    Q4 root_rot = ref_remove_base_rot(ld4(body_rot));
    float heading = ref_calc_heading(root_rot);
    Q4 hinv = ref_heading_quat(-heading);
    V3 p = ld3(body_pos + j * L::POS);
    Q4 q = ld4(body_rot + j * L::ROT);
    V3 lp = ref_quat_rotate(hinv, p - root_pos);
    if (j > 0) st3(o + 1 + 3 * (j - 1), lp);
    V3 tn, nm;
    if (j == 0) ref_quat_to_tan_norm(root_rot, tn, nm);  // reference overwrites the root entry with the un-headed root (:807-808)
    else ref_quat_to_tan_norm(qmul(hinv, q), tn, nm);
    st3(o + 70 + 6 * j, tn);
    st3(o + 70 + 6 * j + 3, nm);
    st3(o + 214 + 3 * j, ref_quat_rotate(hinv, ld3(in.body_vel + e * in.s_body_vel + j * L::VEL)));
    st3(o + 286 + 3 * j, ref_quat_rotate(hinv, ld3(in.body_ang_vel + e * in.s_body_ang_vel + j * L::ANG)));
    V3 tp = ld3(tgt_pos + j * 3);
    Q4 tq = ld4(tgt_rot + j * 4);
    st3(o + 507 + 3 * j, ref_quat_rotate(hinv, tp - p));
    ref_quat_to_tan_norm(qmul(qconj(q), tq), tn, nm);
    st3(o + 579 + 6 * j, tn);
    st3(o + 579 + 6 * j + 3, nm);
    if (j > 0) {
        const int dj = 3 * (j - 1);
        st3(o + 358 + dj, obs_im_ld_dof<L>(in.dof_vel + e * in.s_dof_vel + dj * L::DOF));
        st3(o + 438 + dj, ld3(in.tgt_dof_pos + tf * in.s_tgt_dof_pos + dj) - obs_im_ld_dof<L>(in.dof_pos + e * in.s_dof_pos + dj * L::DOF));
    } else {
        o[0] = root_pos.z;
        V3 t_root_pos = tp;
        Q4 t_root_rot = ref_remove_base_rot(tq);
        o[427] = root_pos.z - t_root_pos.z;
        ref_quat_to_tan_norm(qmul(t_root_rot, qconj(root_rot)), tn, nm);
        st3(o + 428, tn);
        st3(o + 431, nm);
        V3 rel = ref_quat_rotate(hinv, t_root_pos - root_pos);
        o[434] = rel.x; o[435] = rel.y;
        float dh = ref_calc_heading(t_root_rot) - heading;
        o[436] = cosf(dh); o[437] = sinf(dh);
    }
    if (j < 11) o[723 + j] = in.motion_bodies[e * in.s_motion_bodies + j];
}
