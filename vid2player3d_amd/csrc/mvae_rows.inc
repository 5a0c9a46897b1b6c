// The bodies of the motion generator's two kernels as TEXT, included by the single-player kernels and by the two-player ones of
// mvae_player.hip.  They are text and not function templates because mvae_step_kernel and mvae_reset_kernel must stay the machine code
// they were (tools/kernel_identity.py): included with the single player's definitions the text is, token for token, what those kernels
// held.  A change that is allowed to move the old kernels' code should turn both pieces into __device__ function templates.
//
// MV_TEXT_STEP: a tile's control step from the loads of cat(z, condition) to the last store of `_update_mvae_state(init=False)`.  Reads
// a (latents, residual, b), t, lane, wave, rows, the seven LDS arrays, and
//   MV_ENV(row)                   the env of row `row` of the tile
//   MV_SIDE_W, MV_SIDE_C          the v2p_mvae_weights and v2p_mvae_cfg of the tile's envs
//   MV_ROOT_AVG, MV_ROOT_STD      the statistics that normalise the root-position columns of the condition (the single player's own; the
//                                 two-player step: side 1's for every env, see mvae_dual_step_kernel)
//
// MV_TEXT_RESET: a wave's reset of list entry i.  Reads a (env_ids, init_feature, root_xy, num_envs, b), i, lane, and
//   MV_SIDE_W, MV_SIDE_C          as above, of env e
//   MV_RACKET_RIGHTHAND           the hand of the racket's FK chain
//   MV_RACKET_DIR(k), MV_RACKET_NORMAL(k)   component k of the racket's canonical direction and normal
//   MV_BIND                       joint_pos_bind_rel [24,3] of list entry i
#if defined(MV_TEXT_STEP)
    // cat(z, condition) of the tile's envs (zeros for the rows past n); z goes into both buffers
    for (int i = t; i < MV_TILE * MV_IN0; i += MV_THREADS) {
        const int row = i / MV_IN0, k = i - row * MV_IN0;
        float v = 0.f;
        if (row < rows) v = k < MV_LATENT ? a.latents[MV_ENV(row) * MV_LATENT + k] : a.b.conditions[MV_ENV(row) * MV_FRAME + (k - MV_LATENT)];
        bufA[row * MV_XS + mv_perm(k)] = v;
        if (k < MV_LATENT) bufB[row * MV_XS + mv_perm(k)] = v;
    }
    __syncthreads();
    // the gate: 320 -> 64 -> 64 -> 6, ELU, softmax
    mv_gate_layer<true>(bufA, MV_XS, MV_SIDE_W.gate_w0, MV_SIDE_W.gate_b0, MV_IN0, MV_GATE / 32, g1, MV_GS, true, wave, lane);
    __syncthreads();
    mv_gate_layer<true>(g1, MV_GS, MV_SIDE_W.gate_w1, MV_SIDE_W.gate_b1, MV_GATE, MV_GATE / 32, g2, MV_GS, true, wave, lane);
    __syncthreads();
    mv_gate_layer<false>(g2, MV_GS, MV_SIDE_W.gate_w2, MV_SIDE_W.gate_b2, MV_GATE, 1, g1, MV_GS, false, wave, lane);  // (logits: columns 0..5 of g1)
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
    mv_blend_layer<true>(bufA, MV_SIDE_W.w0, MV_SIDE_W.b0, MV_IN0, MV_HIDDEN, coef, bufB, MV_LATENT, true, wave, lane);
    __syncthreads();
    mv_blend_layer<true>(bufB, MV_SIDE_W.w1, MV_SIDE_W.b1, MV_IN1, MV_HIDDEN, coef, bufA, MV_LATENT, true, wave, lane);
    __syncthreads();
    mv_blend_layer<false>(bufA, MV_SIDE_W.w2, MV_SIDE_W.b2, MV_IN1, MV_OUT, coef, bufB, 0, false, wave, lane);
    __syncthreads();

    // ---- `_update_mvae_state(init=False)`: bufB[row][0..289] is the normalized feature and the two phase numbers
    const float* avg = MV_SIDE_W.avg;
    const float* sd = MV_SIDE_W.std;
    const bool residual = a.residual != nullptr;
    const int elbow = MV_SIDE_C.righthand ? 19 : 18, wrist = MV_SIDE_C.righthand ? 21 : 20;
    if (t < rows) {  // the env's scalars: root, phase, swing type
        const int64_t e = MV_ENV(t);
        const float* o = bufB + t * MV_XS;
        for (int k = 0; k < 3; ++k) {
            const float vel = o[MV_COL_ROOT_VEL + k] * sd[MV_COL_ROOT_VEL + k] + avg[MV_COL_ROOT_VEL + k];
            const float pos = a.b.root_pos[e * 3 + k] + vel;
            a.b.root_pos[e * 3 + k] = pos;
            a.b.root_vel[e * 3 + k] = vel;
            a.b.conditions[e * MV_FRAME + k] = (pos - MV_ROOT_AVG[k]) / MV_ROOT_STD[k];
        }
        float ph = atan2f(o[MV_FRAME], o[MV_FRAME + 1]);
        if (ph < 0.f) ph = ph + 2.f * MV_PI;
        int64_t st = a.b.swing_type[e];
        const int col = MV_COL_JOINT_POS + (MV_RWRIST - 1) * 3;  // the RIGHT wrist's x, whatever the hand
        const float wx = o[col] * sd[col] + avg[col];
        if (st == -1 && ph > 2.0f && ph < 3.5f) st = (wx > 0.f) == (MV_SIDE_C.righthand != 0) ? 1 : 2;
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
        if (k >= 3) a.b.conditions[MV_ENV(row) * MV_FRAME + k] = v;
        if (k >= MV_COL_ROT6D) {
            const int j = (k - MV_COL_ROT6D) / 6;
            if (!(residual && (j == elbow || j == wrist))) a.b.joint_rot6d[MV_ENV(row) * (MV_JOINTS * 6) + (k - MV_COL_ROT6D)] = v * sd[k] + avg[k];
        }
    }
    __syncthreads();
    // joints: thread (row, sub) takes joints sub, sub + 8, sub + 16
    const int row = t >> 3, sub = t & 7;
    if (row < rows) {
        const int64_t e = MV_ENV(row);
        const float* o = bufB + row * MV_XS;
        for (int j = sub; j < MV_JOINTS; j += 8) {
            float r6[6], m[9];
            for (int k = 0; k < 6; ++k) { const int col = MV_COL_ROT6D + j * 6 + k; r6[k] = o[col] * sd[col] + avg[col]; }
            mv_rot6d_to_rotmat(r6, m);
            const bool is_elbow = j == elbow, is_wrist = j == wrist;
            if (residual && (is_elbow || is_wrist)) {
                const MvPlayer& P = MV_PLAYERS[MV_SIDE_C.player];
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
                if (!MV_SIDE_C.is_train) {
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
                ref_angle_axis_to_rotmat(aa, m);
                r6[0] = m[0]; r6[1] = m[3]; r6[2] = m[6]; r6[3] = m[1]; r6[4] = m[4]; r6[5] = m[7];
                for (int k = 0; k < 6; ++k) a.b.joint_rot6d[e * (MV_JOINTS * 6) + j * 6 + k] = r6[k];
            }
            for (int k = 0; k < 9; ++k) a.b.joint_rotmat[e * (MV_JOINTS * 9) + j * 9 + k] = m[k];
            if (!MV_SIDE_C.is_train) {  // rot6d_to_angle_axis of the rot6d as stored: of a rewritten joint, its new two columns
                float m2[9], aa[3];
                if (residual && (is_elbow || is_wrist)) mv_rot6d_to_rotmat(r6, m2);
                else for (int k = 0; k < 9; ++k) m2[k] = m[k];
                mv_rotmat_to_angle_axis(m2, aa);
                for (int k = 0; k < 3; ++k) a.b.joint_rot[e * (MV_JOINTS * 3) + j * 3 + k] = aa[k];
            }
        }
    }
#elif defined(MV_TEXT_RESET)
    const int64_t e = a.env_ids[i];
    if (e < 0 || e >= a.num_envs) return;
    const float* f = a.init_feature + i * MV_FRAME;
    const float* avg = MV_SIDE_W.avg;
    const float* sd = MV_SIDE_W.std;
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
        if (!MV_SIDE_C.is_train) {
            mv_rotmat_to_angle_axis(m, aa);
            for (int k = 0; k < 3; ++k) a.b.joint_rot[e * (MV_JOINTS * 3) + lane * 3 + k] = aa[k];
        }
    }
    if (lane == 0) {
        // infer_racket_with_fk (utils/racket.py:235-269): the chain of 4x4 transforms Pelvis .. Hand, products in matmul's order
        const int rh = MV_RACKET_RIGHTHAND != 0;
        const int chain[9] = {0, 3, 6, 9, rh ? 14 : 13, rh ? 17 : 16, rh ? 19 : 18, rh ? 21 : 20, rh ? 23 : 22};
        float R[9], p[3];
        mv_rot6d_to_rotmat(f + MV_COL_ROT6D, R);
        for (int k = 0; k < 3; ++k) p[k] = MV_BIND[k];
        for (int c = 1; c < 8; ++c) {  // (up to the wrist: the hand's transform is not read by `infer_with_fk`)
            float m[9], Rn[9], pn[3];
            const int j = chain[c];
            mv_rot6d_to_rotmat(f + MV_COL_ROT6D + j * 6, m);
            for (int r = 0; r < 3; ++r) {
                for (int q = 0; q < 3; ++q) Rn[r * 3 + q] = R[r * 3] * m[q] + R[r * 3 + 1] * m[3 + q] + R[r * 3 + 2] * m[6 + q];
                pn[r] = R[r * 3] * MV_BIND[j * 3] + R[r * 3 + 1] * MV_BIND[j * 3 + 1] + R[r * 3 + 2] * MV_BIND[j * 3 + 2] + p[r];
            }
            for (int k = 0; k < 9; ++k) R[k] = Rn[k];
            for (int k = 0; k < 3; ++k) p[k] = pn[k];
        }
        // the racket: its canonical direction and normal in the wrist's frame; handle 0.2, shaft 0.15, head radius 0.15
        for (int r = 0; r < 3; ++r) {
            const float dir = R[r * 3] * MV_RACKET_DIR(0) + R[r * 3 + 1] * MV_RACKET_DIR(1) + R[r * 3 + 2] * MV_RACKET_DIR(2);
            const float nrm = R[r * 3] * MV_RACKET_NORMAL(0) + R[r * 3 + 1] * MV_RACKET_NORMAL(1) + R[r * 3 + 2] * MV_RACKET_NORMAL(2);
            const float wr = p[r] + root[r];
            a.b.racket_pos[e * 3 + r] = ((wr + dir * 0.2f) + dir * 0.15f) + dir * 0.15f;
            a.b.racket_normal[e * 3 + r] = nrm;
        }
    }
#endif
