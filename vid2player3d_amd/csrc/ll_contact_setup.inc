// A fragment of physics_ll_kernel's substep (physics_ll.hip includes it at the two places where an instantiation may run it, F::CGEN_EARLY):
// contact generation - the cull, the scan rounds, the four records into the lane's LDS column, the diagnostic ids.  It reads the pose q, x
// of the link from registers and leaves `cnt`, the number of points, and the records in `CS`.
#pragma unroll
for (int c = 0; c < 4; ++c) { CS.set_cr(c, V3{0.f, 0.f, 0.f}); CS.set_bias(c, 0.f); CS.set_lam(c, V3{0.f, 0.f, 0.f}); }
if (CONTACT) {
    // ============================================================ contact generation: every lane scans its own hull
    // pass A marks the candidate vertices (z < contact_offset) in a per-lane 64-bit mask; the manifold reduction then
    // walks only the candidates.  Hull vertices come from the LDS copy of the model (staged once per launch).
    const float coff = P.contact_offset;
    const int v0 = S->hull_offsets[bo], nv = S->hull_count[bo];
    // conservative culling: lowest point of the hull's body-frame bounding box (third row of the link's rotation)
    const float rz0 = 2.f * (q.x * q.z - q.w * q.y), rz1 = 2.f * (q.y * q.z + q.w * q.x), rz2 = 1.f - 2.f * (q.x * q.x + q.y * q.y);
    const float zlow = x.z + rz0 * S->aabb_c[bo][0] + rz1 * S->aabb_c[bo][1] + rz2 * S->aabb_c[bo][2] -
                       (fabsf(rz0) * S->aabb_e[bo][0] + fabsf(rz1) * S->aabb_e[bo][1] + fabsf(rz2) * S->aabb_e[bo][2]);
    const bool near = valid && (zlow < coff + 1e-4f);
    int pack = 0x0fffffff;  // four 7-bit vertex slots (127 = none), manifold size in bits 28..30
    long long tsub = DIAG && a.prof ? clock64() : 0;
    const unsigned long long nball = __ballot(near);
    LLSUB(PROF_CULL);
    if (nball) {
        // The hulls of the few links near the ground are scanned by GROUPS of 8 lanes, 8 groups per wave: in every round group g
        // takes the next near link of the WAVE (the near links of both envs in lane order), whichever env it belongs to - a
        // ragdoll with 17 near links that shares its wave with a standing humanoid needs 3 rounds instead of 5.  Lane gl of a
        // group takes vertices gl, gl+8, ... and the group combines with three DPP steps.  Every selection keeps the serial rule
        // "first index attaining the extreme": per lane indices ascend, across lanes ties go to the lower index; which group
        // scans a link changes nothing in its numbers.
        const unsigned nm = half ? (unsigned)(nball >> 32) : (unsigned)nball;
        const int nr0 = __popc((unsigned)nball), nr1 = __popc((unsigned)(nball >> 32));
        const int ntot = nr0 + nr1;
        const int rounds = (ntot + 7) >> 3;
        const int myk = (half ? nr0 : 0) + __popc(nm & ((1u << lb) - 1u));  // rank of this link among the near links of the wave
        const int grp = lane >> 3, gl = lane & 7;
        int* const scr = (int*)(wave_lds + LDS_PARK + PARK_SCR * 64);  // k-th near link -> its lane
        if (near) scr[myk] = lane;
        LLCOUNT(PROF_ROUNDS, rounds);
        for (int rd = 0; rd < rounds; ++rd) {
            const int kk = 8 * rd + grp;
            const bool gon = kk < ntot;
            const int src = gon ? scr[kk] : lane;
            // the group works in the frame of ITS link: pose pulled from the owner lane (7 values instead of 12)
            const M3 RL = q2mat(pull(q, src));
            const V3 xL = pull(x, src);
            const float r6 = RL.m[6], r7 = RL.m[7], r8 = RL.m[8], xz = xL.z;
            const int v0L = __builtin_amdgcn_ds_bpermute(src << 2, v0), nvL = __builtin_amdgcn_ds_bpermute(src << 2, nv);
            // (per-env shapes: the link may belong to the other env of the wave)
            ConstShape* const SL = MULTI ? (ConstShape*)(a.shapes + __builtin_amdgcn_ds_bpermute(src << 2, sid)) : S;
            auto hullv = [&](int idx) -> float4 { return make_float4(SL->hull_verts[idx][0], SL->hull_verts[idx][1], SL->hull_verts[idx][2], 0.f); };
            // ---- one pass over the hull: 8 vertices per lane (all loads in flight at once), ground-plane coordinates kept
            // for the manifold reduction; candidates (z < contact_offset) as a bit mask, deepest one tracked
            const float r0 = RL.m[0], r1 = RL.m[1], r2 = RL.m[2], xx = xL.x;
            const float r3 = RL.m[3], r4 = RL.m[4], r5 = RL.m[5], xy = xL.y;
            const unsigned gbit = 1u << gl;
            float4 vv[8];
#pragma unroll
            for (int k = 0; k < 8; ++k) {
                const int i = 8 * k + gl;
                vv[k] = hullv(v0L + ((gon && i < nvL) ? i : 0));
            }
            float px[8], py[8];
            unsigned clo = 0u, chi = 0u;
            int k0 = -1;
            float zmin = 0.f;
#pragma unroll
            for (int k = 0; k < 8; ++k) {
                const int i = 8 * k + gl;
                const bool in = gon && i < nvL;
                const float z = xz + r6 * vv[k].x + r7 * vv[k].y + r8 * vv[k].z;
                px[k] = xx + r0 * vv[k].x + r1 * vv[k].y + r2 * vv[k].z;
                py[k] = xy + r3 * vv[k].x + r4 * vv[k].y + r5 * vv[k].z;
                const bool c = in && (z < coff);
                const unsigned bit = c ? gbit << (8 * (k & 3)) : 0u;
                if (k < 4) clo |= bit; else chi |= bit;
                const bool better = c && (k0 < 0 || z < zmin);
                k0 = better ? i : k0;
                zmin = better ? z : zmin;
            }
            clo |= grp_xor1(clo); chi |= grp_xor1(chi);
            clo |= grp_xor2(clo); chi |= grp_xor2(chi);
            clo |= grp_mirror(clo); chi |= grp_mirror(chi);
            grp_arg<false, F::FASTARG>(zmin, k0);
            const unsigned long long cm = ((unsigned long long)chi << 32) | clo;
            const int cntg = __popc(clo) + __popc(chi);
            unsigned long long t = cm;
            int s0 = t ? __ffsll((long long)t) - 1 : -1; t &= t - 1;
            int s1 = t ? __ffsll((long long)t) - 1 : -1; t &= t - 1;
            int s2 = t ? __ffsll((long long)t) - 1 : -1; t &= t - 1;
            int s3 = t ? __ffsll((long long)t) - 1 : -1;
            int ns = cntg < 4 ? cntg : 4;
            const bool big = gon && cntg > 4;
            if (any64(big)) {
                LLCOUNT(PROF_MANIFOLDS, 1ull);
                // manifold reduction: deepest, farthest from it, extreme on either side of that line
                const int k0s = k0 < 0 ? 0 : k0;
                const float4 u0 = hullv(v0L + k0s);
                const float p0x = xx + r0 * u0.x + r1 * u0.y + r2 * u0.z;
                const float p0y = xy + r3 * u0.x + r4 * u0.y + r5 * u0.z;
                const unsigned long long remB = big ? (cm & ~(1ull << k0s)) : 0ull;
                const unsigned blo = (unsigned)remB, bhi = (unsigned)(remB >> 32);
                int k1 = -1;
                float best = -1.f;
#pragma unroll
                for (int k = 0; k < 8; ++k) {
                    const bool on = ((k < 4 ? blo : bhi) & (gbit << (8 * (k & 3)))) != 0u;
                    const float dx = px[k] - p0x, dy = py[k] - p0y;
                    const float d2 = dx * dx + dy * dy;
                    const bool take = on && (d2 > best);
                    best = take ? d2 : best;
                    k1 = take ? 8 * k + gl : k1;
                }
                grp_arg<true, F::FASTARG>(best, k1);
                const int k1s = k1 < 0 ? 0 : k1;
                const float4 u1 = hullv(v0L + k1s);
                const float ex = xx + r0 * u1.x + r1 * u1.y + r2 * u1.z - p0x;
                const float ey = xy + r3 * u1.x + r4 * u1.y + r5 * u1.z - p0y;
                const unsigned long long remC = remB & ~(1ull << k1s);
                const unsigned elo = (unsigned)remC, ehi = (unsigned)(remC >> 32);
                int k2 = -1, k3 = -1;
                float amax = 0.f, amin = 0.f;
#pragma unroll
                for (int k = 0; k < 8; ++k) {
                    const bool on = ((k < 4 ? elo : ehi) & (gbit << (8 * (k & 3)))) != 0u;
                    const float dx = px[k] - p0x, dy = py[k] - p0y;
                    const float area = ex * dy - ey * dx;
                    const bool up = on && area > amax;
                    const bool dn = on && area < amin;
                    amax = up ? area : amax; k2 = up ? 8 * k + gl : k2;
                    amin = dn ? area : amin; k3 = dn ? 8 * k + gl : k3;
                }
                grp_arg<true, F::FASTARG>(amax, k2);
                grp_arg<false, F::FASTARG>(amin, k3);
                if (big) {
                    s0 = k0; s1 = k1;
                    s2 = k2 >= 0 ? k2 : k3;
                    s3 = k2 >= 0 ? k3 : -1;
                    ns = 2 + (k2 >= 0 ? 1 : 0) + (k3 >= 0 ? 1 : 0);
                }
            }
            const int gpack = (s0 & 0x7f) | ((s1 & 0x7f) << 7) | ((s2 & 0x7f) << 14) | ((s3 & 0x7f) << 21) | (ns << 28);
            const int got = __builtin_amdgcn_ds_bpermute(((myk & 7) << 3) << 2, gpack);
            pack = (near && (myk >> 3) == rd) ? got : pack;
        }
    }
    LLSUB(PROF_SCAN);
    int sel4[4];
#pragma unroll
    for (int c = 0; c < 4; ++c) {
        const int sv = (pack >> (7 * c)) & 0x7f;
        sel4[c] = sv == 0x7f ? -1 : sv;
    }
    cnt = (pack >> 28) & 7;
    if (any64(cnt > 0)) {
        const M3 R = q2mat(q);
        const float ih = 1.f / h;
#pragma unroll
        for (int c = 0; c < 4; ++c) {
            const float4 uu = hullv(v0 + (sel4[c] < 0 ? 0 : sel4[c]));
            const V3 crc = mul(R, V3{uu.x, uu.y, uu.z});
            CS.set_cr(c, crc);
            float dz = x.z + crc.z - P.rest_offset;
            CS.set_bias(c, TGS ? dz : (dz >= 0.f ? dz * ih : fmaxf(P.erp * dz * ih, -P.max_depen)));
        }
    }
    if (a.contact_ids && last && valid && live_env && !frozen) {  // diagnostics (v2p_sim_cfg.debug_contacts)
#pragma unroll
        for (int c = 0; c < 4; ++c) a.contact_ids[(env_here() * NB + b) * 4 + c] = c < cnt ? b * 64 + sel4[c] : -1;
    }
    if (a.contact_ids_sub && valid && live_env && !frozen) {  // diagnostics: the ids of every substep (parity tests)
#pragma unroll
        for (int c = 0; c < 4; ++c) a.contact_ids_sub[((env_here() * nsub + sub) * NB + b) * 4 + c] = c < cnt ? b * 64 + sel4[c] : -1;
    }

    LLSUB(PROF_POINTS);
}
