// qg_kernel_pair.hip -- the two-legs-per-lane step kernels in a code object of their own: qg_step_kernel_pair, its sequence form
// qg_step_kernel_pair_multi, their launchers and the leaves of the QG_MAP_PAIR mapping (entry points: qg_step_launch.h).
#include "qg_step_dev.h"
#include "qg_step_launch.h"

// ------------------------------------------------------------------------------------------
// env-step kernel, TWO LEGS PER LANE (packed FP32): the two lanes 2e, 2e+1 share env e; lane h owns legs 2h and
// 2h+1 as the two components of f2 quantities, so every fma / mul / add of the leg physics is ONE v_pk_* instruction for
// both legs.  32 envs per wave.  Base prelude, FRAME terms, 6x6 solve and base integration are scalar and redundant in the
// two lanes; leg terms are summed over the two components (a scalar add of the two halves of the register pair) and over the
// lane pair (one DPP add).  Per env this issues 0.59x the instructions of one leg per lane.  v_pk_*_f32 is half rate on gfx950
// (tools/ubench/valu_rate.hip), so this pays only where a wave has its SIMD to itself anyway -- a lone wave issues at most
// every ~4.5 cycles, packed or not: grids of 16-32 Ki envs and, by a smaller margin, >= 56 Ki.  Compiled-in robot only.
// ------------------------------------------------------------------------------------------
DEV float pair_sum(float x) {                                     // quad_perm [1,0,3,2]: the other lane of the pair
#pragma clang fp contract(off)
    return x + dpp_quad<0xB1>(x);
}
DEV float hsum(f2 v) {
#pragma clang fp contract(off)
    return v.x + v.y;
}
DEV V3 hsum(V3T<f2> v) { return v3<float>(hsum(v.x), hsum(v.y), hsum(v.z)); }
DEV V3 pair_sum(V3 a) { return v3<float>(pair_sum(a.x), pair_sum(a.y), pair_sum(a.z)); }
DEV Sym3 hpsum(const Sym3T<f2> &a) {
    Sym3 r = {pair_sum(hsum(a.xx)), pair_sum(hsum(a.yy)), pair_sum(hsum(a.zz)), pair_sum(hsum(a.xy)), pair_sum(hsum(a.xz)), pair_sum(hsum(a.yz))};
    return r;
}
DEV Sym6 hpsum(const Sym6T<f2> &a) {
    Sym6 r;
    r.AA = hpsum(a.AA);
    r.LL = hpsum(a.LL);
    r.AL.r0 = pair_sum(hsum(a.AL.r0)); r.AL.r1 = pair_sum(hsum(a.AL.r1)); r.AL.r2 = pair_sum(hsum(a.AL.r2));
    return r;
}
DEV SV hpsum(const SVT<f2> &v) { SV r = {pair_sum(hsum(v.a)), pair_sum(hsum(v.l))}; return r; }

struct LegPair { f2 q[3], qd[3], act[3], u[3], sc[6]; };   // sc: sin, cos of (q[i] - ref_i) of both legs, advanced with the hinges

DEV void substep_pair(const KModel &C, f2 cm, f2 sm, BaseState &B, LegPair &L, bool want_sensors, float *__restrict__ row, int half, float &zaxis_z) {
    const float h = C.h;
    const BaseCtx bc0 = base_prelude<true>(C, B);
    V3 gb_keep;
    Sym6 Ic;
    SV fc, Fu;
    f2 Y0[6], Y1[6], Y2[6], u[3];
    {
        const BaseCtx &bc = bc0;
        gb_keep = bc.gb;
        if (want_sensors) {          // the step's sensordata describes the state at the start of its last substep
            zaxis_z = bc.cz.z;
            float *jr = row + 6 * half;                  // legs 2*half and 2*half + 1
            jr[0] = L.q[0].x; jr[1] = L.q[1].x; jr[2] = L.q[2].x;
            jr[3] = L.q[0].y; jr[4] = L.q[1].y; jr[5] = L.q[2].y;
            if (half == 0) {
                row[15] = B.wb.x; row[16] = B.wb.y; row[17] = B.wb.z;
                row[18] = B.pw.x; row[19] = B.pw.y; row[20] = B.pw.z;
                row[21] = B.vw.x; row[22] = B.vw.y; row[23] = B.vw.z;
                row[24] = bc.cx.x; row[25] = bc.cx.y; row[26] = bc.cx.z;
                row[27] = bc.cz.x; row[28] = bc.cz.y; row[29] = bc.cz.z;
                row[30] = bc.vb.x; row[31] = bc.vb.y; row[32] = bc.vb.z;
            }
        }
        // both legs of this lane, each in the frame turned by its quarter turn: there each of them is leg 0
        const f2 z2 = f2(0.f), o2 = f2(1.f);
        FrT<f2> Ek = {v3<f2>(cm, sm, z2), v3<f2>(-sm, cm, z2), v3<f2>(z2, z2, o2)};
        Sym6T<f2> Ic2, YFt2;
        SVT<f2> fc2, F2[3], Fu2;
        f2 Hd[3], H01, H02, H12, bj[3];
        leg_pass<f2, true, true, false, true>(C, 0, Ek, L.q, L.qd, L.act, bc, B.pw.z, h, Ic2, fc2, F2, Hd, H01, H02, H12, bj, L.sc);
        leg_eliminate<f2>(F2, Hd, H01, H02, H12, bj, Y0, Y1, Y2, u, YFt2, Fu2);
        sub(Ic2, YFt2);                     // the two legs' Schur complements
        // Sum over the two legs of the lane and over the two lanes of the env, HERE, far from the uses: the DPP moves then stay unfused
        // (33 v_mov_b32_dpp per substep: the compiler fuses a move into its add only when the two are close, see substep_quad), but
        // with the sums right in front of the 6x6 solve the lone wave of this kernel ran 2.6 % slower at 32 768 and at 262 144 envs
        // (same-box A/B, round 3: 25.0 -> 25.65 us; the dependent chain sum -> assemble -> solve has nothing to overlap with there)
        Ic = hpsum(Ic2);
        fc = hpsum(fc2);
        Fu = hpsum(Fu2);
    }
    float x6[6];
    {
        const BaseCtx &bc = bc0;
        SV p0;
        Sym6 Ic0;
        frame_body(C, bc, h, p0, Ic0);
        SV b;
        {   // FRAME contact: this lane evaluates two quarter turns of the three base sample points
            f2 wsum2 = f2(0.f);
            V3T<f2> s2 = v3<f2>(f2(0.f), f2(0.f), f2(0.f));
            const f2 zb = f2(C.contact_margin - B.pw.z);
            const V3T<f2> n2 = splat3<f2>(bc.n);
#pragma unroll
            for (int o = 0; o < 3; ++o) {
                V3 r0 = ld3(C.cp0[4 * o]);
                contact_point(v3<f2>(cm * r0.x - sm * r0.y, sm * r0.x + cm * r0.y, f2(r0.z)), n2, zb, wsum2, s2);
            }
            float wsum = pair_sum(hsum(wsum2));
            add(Ic0, Ic);
            b.a = v3<float>(0.f, 0.f, 0.f) - Fu.a - p0.a - fc.a;
            b.l = v3<float>(0.f, 0.f, 0.f) - Fu.l - p0.l - fc.l;
            if (__any(wsum > 0.f)) {        // wave-uniform skip, as in the quad kernel (the block is updated in place)
                V3 s = pair_sum(hsum(s2));
                Fr E0 = {v3<float>(1.f, 0.f, 0.f), v3<float>(0.f, 1.f, 0.f), v3<float>(0.f, 0.f, 1.f)};
                SV fe;
                contact_finish<float>(wsum, s, E0, v3<float>(0.f, 0.f, 0.f), bc.n, bc.V0, C.contact_k, C.contact_c, C.contact_inv_ramp, C.contact_mu, h, fe, Ic0);
                b.a = b.a + fe.a;
                b.l = b.l + fe.l;
            }
        }
        base_solve(Ic0, b, x6);     // (pk3::base_solve: 36 instructions fewer and 2.7 % SLOWER here, 24.96 -> 25.64 us at 32 768 envs: the solve sits on
                                     // this kernel's dependent tail, and a dependent packed instruction costs a lone wave ~1.5 plain ones; the same right-looking
                                     // order in plain FP32, 15 instructions fewer: no difference, 24.9-25.1 us either way)
    }
    V3 wdot = v3<float>(x6[0], x6[1], x6[2]);
    V3 acl = v3<float>(x6[3], x6[4], x6[5]);
    if (want_sensors && half == 0) {
        row[12] = acl.x - gb_keep.x; row[13] = acl.y - gb_keep.y; row[14] = acl.z - gb_keep.z;   // accelerometer
    }
    // back-substitution and integration of this lane's six hinges
    const f2 *Y[3] = {Y0, Y1, Y2};
#pragma unroll
    for (int i = 0; i < 3; ++i) {
        f2 acc = u[i];
#pragma unroll
        for (int r = 0; r < 6; ++r) acc = fma_(-Y[i][r], f2(x6[r]), acc);
        L.qd[i] = fma_(f2(h), acc, L.qd[i]);
        L.q[i] = fma_(f2(h), L.qd[i], L.q[i]);
        hinge_advance(f2(h) * L.qd[i], L.sc[2 * i], L.sc[2 * i + 1]);
        L.act[i] = fma_(L.u[i] - L.act[i], f2(C.link[i].act_decay), L.act[i]);
    }
    {
        const BaseCtx &bc = bc0;
        base_integrate<true>(bc, h, wdot, acl, B);
    }
}


// One wave per SIMD by construction (381 registers): capping it to 256 for two resident waves spills 592 B per lane and
// measured slower than this variant at every size (profiles/r01/pair_sweep.txt), so there is only this one.
// WAVES: waves per workgroup (1 or 4, one per SIMD of a CU; they do not interact).  A grid of 1024 one-wave workgroups costs ~1.6 us
// more fixed time per launch than 256 four-wave ones (the dispatch of the workgroups themselves: tools/fs_sweep.sh on the
// one-link-per-lane kernel), so grids of more than 256 waves are launched as four-wave workgroups.
// WALK: the walking task layer fused in as in qg_step_kernel_quad<.., WALK>; the lane owns the six control channels of its two legs
// (6 * half .. 6 * half + 5, contiguous in the env-major task state).
// PO (with WALK; round 3): the partially observable observation pack fused in as well -- POWalkingQuadrupedEnv.step is this one launch
// also at the batch sizes this kernel serves.  The copy of the W - 1 frames the new stack keeps rides on the substep loop
// (po_row_copy_*, qg_po_dev.h: loads at the head of a substep, stores at its tail), the env's lead lane runs the orientation filter
// on the step's sensors in the epilogue, the wave writes the new frames.  The 33 sensors themselves are not written to memory.
template <int WAVES, bool WALK = false, bool PO = false>
__global__ __launch_bounds__(QGK_WAVE * WAVES, 1) void qg_step_kernel_pair(const KTask *__restrict__ T, KStepArgs P,
                                                                           const typename WalkArgT<WALK>::type WK,
                                                                           const typename PoArgT<PO>::type PK) {
    static_assert(WALK || !PO, "the observation pack rides on the walking task layer");
    __shared__ float tile_all[WAVES][QGK_PAIR_ENVS * 35];
    QG_MARK(0);
    const KModel &C = QG_BAKED_MODEL;
    const int lane = threadIdx.x & (QGK_WAVE - 1);
    const int wave = threadIdx.x >> 6;
    float *tile = tile_all[wave];
    const int half = lane & 1;                      // legs 2*half, 2*half + 1
    const int el = lane >> 1;                       // env within the wave
    const int env0 = (blockIdx.x * WAVES + wave) * QGK_PAIR_ENVS;
    const int n = P.n;
    const bool live = env0 + el < n;
    int env = live ? env0 + el : n - 1;             // tail pairs shadow the last env; their stores are masked
    // quarter turns of this lane's two legs: (cos, sin)(90 deg * k), k = 2*half and 2*half + 1
    f2 cm, sm;
    cm.x = half ? -1.f : 1.f; cm.y = 0.f;
    sm.x = 0.f; sm.y = half ? -1.f : 1.f;

    BaseState B;
    QG_BASE_LOAD(B, P.st, QG_AT, n, env);
    quat_unit(B);   // unit quaternion once per launch (qg_set_state may hand in any length); the substeps keep it normalised (base_prelude<UNIT>)
    int nstep = P.st.nstep[env];
    LegPair L;
    float aclip[6];
    float ssq = 0.f;
    // WALK: every load of the task layer goes out among the state loads, every store of its prologue part after the last of them
    // (see qg_step_kernel_quad)
    bool settle = false;
    int calls = 0;
    WalkEnvIn win = {};
    int tt[6] = {0, 0, 0, 0, 0, 0};
    float xx[6] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f}, wprev[6] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f}, wf[6] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f},
          wa[6] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f}, a_eff[6] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
    WalkEstIn<6> west;
    WalkChanTargets wtg[6] = {};
    if constexpr (WALK) {
        settle = nstep < WK.P.settle_substeps;                      // data.time < settling_time (walking_quad.py:142-143)
        calls = WK.S.calls[env];
#pragma unroll
        for (int c6 = 0; c6 < 6; ++c6) {
            tt[c6] = env * 12 + 6 * half + c6;
            xx[c6] = P.st.ctrl[(6 * half + c6) * n + env];           // data.ctrl of the PREVIOUS step (walking_quad.py:136)
        }
        {
            float pc[6];
            walk_ldv<6>(WK.S.prev_ctrl + env * 12 + 6 * half, pc);    // previous_ctrl of the control cost (:260-262)
#pragma unroll
            for (int c6 = 0; c6 < 6; ++c6) wprev[c6] = pc[c6];
        }
        walk_estimator_load_n<6>(WK.P, WK.S, n, tt, calls, west);
#pragma unroll
        for (int c6 = 0; c6 < 6; ++c6) wtg[c6] = walk_channel_targets(WK.P, 6 * half + c6);
        if (half == 0) {
            win = walk_env_load(WK.S, n, env);
            win.episode_key = P.st.episode[env];              // not advanced yet: the key of the episode that begins if this one ends
        }
    }
#pragma unroll
    for (int c = 0; c < 2; ++c) {
#pragma unroll
        for (int i = 0; i < 3; ++i) {
            const int j = 3 * (2 * half + c) + i;
            float a_in = P.actions[(size_t)env * 12 + j];
            if constexpr (WALK) {
                if (settle) a_in = WK.P.joint_centers[j];            // the joint centres while the robot settles
                a_eff[3 * c + i] = a_in;
            }
            float a = fminf(fmaxf(a_in, -1.f), 1.f);    // quadruped.py:160
            aclip[3 * c + i] = a;
            ssq = fmaf(a, a, ssq);
            float uu = fminf(fmaxf(a, C.link[i].ctrl_lo), C.link[i].ctrl_hi);
            float qq, qv, aa;
            QG_HINGE_LOAD(qq, qv, aa, P.st, QG_AT, n, env, j);
            if (c == 0) { L.u[i].x = uu; L.q[i].x = qq; L.qd[i].x = qv; L.act[i].x = aa; }
            else { L.u[i].y = uu; L.q[i].y = qq; L.qd[i].y = qv; L.act[i].y = aa; }
        }
    }
    ssq = pair_sum(ssq);
#pragma unroll
    for (int i = 0; i < 3; ++i) sincos_f(L.q[i] - f2(C.link[i].ref), L.sc[2 * i], L.sc[2 * i + 1]);
    // PO: the env's filter state (lead lane) and ring position, this lane's share of its env's row copy ring -> out -- its loads go
    // out here, among the state loads and before the task layer's stores
    PoEnvIn pin = {};
    PoCopyState pcs = {};
    const int live_envs = max(0, min(QGK_PAIR_ENVS, n - env0));
    const int el_c = min(el, max(live_envs - 1, 0));     // row of this lane's env in the wave's block (tail lanes: the last live one)
    unsigned long long po_ring = 0, po_out = 0;          // the wave's block of the frame ring / of the output rows (scalar registers)
    if constexpr (PO) {
        // (a wave that lies wholly past the last env copies nothing, but its loads are unpredicated: they read block 0)
        const size_t po_block = (size_t)(live_envs > 0 ? env0 : 0) * (size_t)(PK.P.window * QG_PO_FRAME);
        po_ring = po_uniform_addr(PK.S.stack + 2 * po_block);
        po_out = po_uniform_addr(PK.out + po_block);
        if (half == 0) pin = po_env_load(PK.S, n, env);
        po_row_copy_init<2>(PK.P, el_c, PK.S.head[env], half, pcs);
    }
    if constexpr (WALK) {
        asm volatile("" :: "v"(B.pw.x), "v"(B.pw.y), "v"(B.pw.z), "v"(B.qw), "v"(B.qx), "v"(B.qy), "v"(B.qz), "v"(B.vw.x), "v"(B.vw.y), "v"(B.vw.z),
                     "v"(B.wb.x), "v"(B.wb.y), "v"(B.wb.z), "v"(L.q[0].x), "v"(L.q[1].x), "v"(L.q[2].x), "v"(L.q[0].y), "v"(L.q[1].y), "v"(L.q[2].y),
                     "v"(L.qd[0].x), "v"(L.qd[1].x), "v"(L.qd[2].x), "v"(L.qd[0].y), "v"(L.qd[1].y), "v"(L.qd[2].y),
                     "v"(L.act[0].x), "v"(L.act[1].x), "v"(L.act[2].x), "v"(L.act[0].y), "v"(L.act[1].y), "v"(L.act[2].y) : "memory");
        if (live) {
            walk_estimator_finish_n<6>(WK.P, WK.S, n, tt, xx, calls, west, wf, wa);    // math_utils.py:53-131
            walk_stv<6>(WK.S.eff_actions + (size_t)env * 12 + 6 * half, a_eff);
        }
    }

    // data.ctrl of this step (quadruped.py:164: the env-clipped action) is known here: it goes out now, behind the loads (the task
    // layer has read the PREVIOUS one above), instead of among the epilogue's stores -- at 32 768 envs all 1024 waves reach their 12.7 MB
    // of epilogue stores at the same moment; an env the step resets gets the default there.  (Same-box A/B, round 3: -0.9 % here, but
    // +0.4 us in the one-link-per-lane kernel at 4096 envs and +0.5 % in the one-leg-per-lane kernel at 16 384: only this kernel has it.)
    if (live && P.track_ctrl) {
#pragma unroll
        for (int c6 = 0; c6 < 6; ++c6) P.st.ctrl[(6 * half + c6) * n + env] = aclip[c6];
    }
    float *srow = tile + el * 35;
    float zaxis_z = 1.f;
    const int fs = T->frame_skip;
    const bool lag = T->sensor_lag != 0;
    // PO: the env's filter state (lead lane) and ring position, this lane's share of its env's row copy ring -> out
    QG_MARK(1);                                      // state in registers, prologue stores issued
#pragma unroll 1
    for (int s = 0; s < fs; ++s) {
        PoCopyRegs<PO ? QG_PO_COPY_K : 1> pcr;
        if constexpr (PO) po_row_copy_load<QG_PO_COPY_K, 2>(PK.P, po_ring, half, s == 0, pcs, pcr);
        substep_pair(C, cm, sm, B, L, lag && (s == fs - 1), srow, half, zaxis_z);
        if constexpr (PO) po_row_copy_store<QG_PO_COPY_K, 2>(PK.P, po_out, live, half, s == 0, pcs, pcr);
    }
    if constexpr (PO) po_row_copy_rest<QG_PO_COPY_K, 2>(PK.P, po_ring, po_out, live, half, pcs);
    nstep += fs;
    // the epilogue's store addresses are derived from `env` AFTER the loop: left visible, the compiler computes two dozen 64-bit
    // addresses before the loop and carries them through it -- ~60 registers of a kernel that already parks values in AGPRs
    // (tools/asm_liveness.py found the same in the one-leg-per-lane kernel in round 2)
    asm volatile("" : "+v"(env));
    QG_MARK(2);                                      // physics done
    if (!lag) {
        BaseState B2 = B;
        LegPair L2 = L;
        substep_pair(C, cm, sm, B2, L2, true, srow, half, zaxis_z);
    }

    QG_REWARD_TERMS(T->, B, ssq, nstep);
    QG_DONE_IF_BAD_STATE(B, pair_sum(hsum(L.q[0]) + hsum(L.q[1]) + hsum(L.q[2]) + hsum(L.qd[0]) + hsum(L.qd[1]) + hsum(L.qd[2])));
    const int od = T->obs_mode == 1 ? 21 : 33;
    const int row = P.packed ? od + 2 : od;
    QG_DONE_IF_FLIPPED(T->, zaxis_z);
    if (half == 0) {
        if (od == 21) { srow[18] = srow[30]; srow[19] = srow[31]; srow[20] = srow[32]; }
        if (P.packed) { srow[od] = reward; srow[od + 1] = done ? 1.f : 0.f; }
    }
    wave_sync();                                                   // the tile is this wave's own
    if constexpr (!PO) {
        const int total = live_envs * row;                               // (a whole wave may lie past the last env: live_envs = 0)
        float *dst = (P.packed ? P.packed : P.obs) + (size_t)env0 * row;
        QG_TILE_COPY_OUT(dst, tile, lane, total, row);
    }
    QG_MARK(3);                                      // obs tile written out
    const bool lead = live && half == 0;
    if (lead && !P.packed) {
        if constexpr (!WALK) P.reward[env] = reward;
        P.done[env] = done ? 1 : 0;
    }
    if constexpr (WALK) {
        WalkSums sum = {0.f, 0.f, 0.f, 0.f};
        if (live) {
#pragma unroll
            for (int c6 = 0; c6 < 6; ++c6) walk_channel_terms(WK.S, env, 6 * half + c6, wtg[c6], aclip[c6], wprev[c6], wf[c6], wa[c6], sum);
            walk_stv<6>(WK.S.prev_ctrl + (size_t)env * 12 + 6 * half, aclip);                          // previous_ctrl moves on (:260-262)
        }
        sum.cost = pair_sum(sum.cost); sum.posture = pair_sum(sum.posture); sum.amp = pair_sum(sum.amp); sum.frq = pair_sum(sum.frq);
        QG_MARK(4);                                  // channel terms + sums
        if (lead) walk_reward_env(WK.P, WK.S, n, env, tile + el * 35, sum, win, done, P.reward, WK.comps, WK.sample, P.seed, P.env_index_base);
        QG_MARK(5);                                  // reward
    }
    QG_COMPS_STORE(lead, P, env);

    const bool rst = done && T->auto_reset;
    if (rst) QG_BASE_RESET(B, nstep, C.qpos0, T->, P, env, P.st.episode[env]);
    if (lead) {
        QG_BASE_STORE(B, nstep, P.st, QG_PUT, n, env);
        if (rst) P.st.episode[env] += 1;
    }
    if (live) {
#pragma unroll
        for (int c = 0; c < 2; ++c) {
#pragma unroll
            for (int i = 0; i < 3; ++i) {
                const int j = 3 * (2 * half + c) + i;
                QG_HINGE_STORE(rst ? C.qpos0[7 + i] : (c == 0 ? L.q[i].x : L.q[i].y), rst ? 0.f : (c == 0 ? L.qd[i].x : L.qd[i].y), rst ? 0.f : (c == 0 ? L.act[i].x : L.act[i].y), P.st, QG_PUT, n, env, j);
                if (P.track_ctrl && rst) P.st.ctrl[j * n + env] = T->default_ctrl[j];          // (the step's data.ctrl went out in the prologue)
            }
        }
    }
    QG_MARK(6);                                      // reset block, state stores issued
    if constexpr (PO)
        po_wave_epilogue<QGK_PAIR_ENVS, 2, WAVES, false>(PK, WK, P, n, env, env0, live_envs, wave, lane, el, half, live, lead, pin, srow, B, win, done, aclip);
    QG_MARK(9);
}

// ---- the sequence form (16 385 .. 32 768 envs and >= 57 344: BASELINE configs 3 and 4's sizes) --------------------------------------------
// qg_step_kernel_pair with an outer loop over env-steps, exactly as qg_step_kernel_link_multi<.., DOOR = false> (qg_kernel_resident.hip) is
// to qg_step_kernel_link:
// state loaded once and stored once, per env-step what a fresh launch does with the state it loads, bit-identical results.  Compiled-in
// robot, lagged sensors, packed rows (the launcher falls back to per-step launches otherwise).
template <int WAVES>
__global__ __launch_bounds__(QGK_WAVE * WAVES, 1) void qg_step_kernel_pair_multi(const KTask *__restrict__ T, KStepArgs P, KResident R) {
    __shared__ float tile_all[WAVES][QGK_PAIR_ENVS * 35];
    const KModel &C = QG_BAKED_MODEL;
    const int lane = threadIdx.x & (QGK_WAVE - 1);
    const int wave = threadIdx.x >> 6;
    float *tile = tile_all[wave];
    const int half = lane & 1;
    const int el = lane >> 1;
    const int env0 = (blockIdx.x * WAVES + wave) * QGK_PAIR_ENVS;
    const int n = P.n;
    const bool live = env0 + el < n;
    int env = live ? env0 + el : n - 1;
    f2 cm, sm;
    cm.x = half ? -1.f : 1.f; cm.y = 0.f;
    sm.x = 0.f; sm.y = half ? -1.f : 1.f;
    QG_TASK_REGS(Tk, T);

    BaseState B;
    QG_BASE_LOAD(B, P.st, QG_AT, n, env);
    int nstep = P.st.nstep[env];
    int episode = P.st.episode[env];
    LegPair L;
#pragma unroll
    for (int c = 0; c < 2; ++c) {
#pragma unroll
        for (int i = 0; i < 3; ++i) {
            const int j = 3 * (2 * half + c) + i;
            float qq, qv, aa;
            QG_HINGE_LOAD(qq, qv, aa, P.st, QG_AT, n, env, j);
            if (c == 0) { L.q[i].x = qq; L.qd[i].x = qv; L.act[i].x = aa; L.u[i].x = 0.f; }
            else { L.q[i].y = qq; L.qd[i].y = qv; L.act[i].y = aa; L.u[i].y = 0.f; }
        }
    }
    const int od = Tk.obs_mode == 1 ? 21 : 33;
    const int row = od + 2;
    const int fs = Tk.frame_skip;
    const int live_envs = max(0, min(QGK_PAIR_ENVS, n - env0));
    const int total = live_envs * row;
    const bool lead = live && half == 0;
    float *srow = tile + el * 35;
    const size_t slot_act = (size_t)n * 12, slot_out = (size_t)n * row;
    float ctrl_reg[6] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
    float a_next[6] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
    bool have_next = false;

    for (int kstep = 0; kstep < R.count; ++kstep) {
        float a_in[6];
        const float *ap = R.actions + (size_t)kstep * slot_act + (size_t)env * 12 + 6 * half;
#pragma unroll
        for (int c6 = 0; c6 < 6; ++c6) a_in[c6] = have_next ? a_next[c6] : ap[c6];
        have_next = kstep + 1 < R.count;
        if (have_next) {
#pragma unroll
            for (int c6 = 0; c6 < 6; ++c6) a_next[c6] = ap[slot_act + c6];
        }
        float aclip[6];
        float ssq = 0.f;
#pragma unroll
        for (int c = 0; c < 2; ++c) {
#pragma unroll
            for (int i = 0; i < 3; ++i) {
                const float a = fminf(fmaxf(a_in[3 * c + i], -1.f), 1.f);    // quadruped.py:160
                aclip[3 * c + i] = a;
                ssq = fmaf(a, a, ssq);
                const float uu = fminf(fmaxf(a, C.link[i].ctrl_lo), C.link[i].ctrl_hi);
                if (c == 0) L.u[i].x = uu; else L.u[i].y = uu;
            }
        }
        ssq = pair_sum(ssq);
        quat_unit(B);
#pragma unroll
        for (int i = 0; i < 3; ++i) sincos_f(L.q[i] - f2(C.link[i].ref), L.sc[2 * i], L.sc[2 * i + 1]);
        float zaxis_z = 1.f;
#pragma unroll 1
        for (int s = 0; s < fs; ++s) substep_pair(C, cm, sm, B, L, s == fs - 1, srow, half, zaxis_z);
        nstep += fs;
        asm volatile("" : "+v"(env));

        QG_REWARD_TERMS(Tk., B, ssq, nstep);
        QG_DONE_IF_BAD_STATE(B, pair_sum(hsum(L.q[0]) + hsum(L.q[1]) + hsum(L.q[2]) + hsum(L.qd[0]) + hsum(L.qd[1]) + hsum(L.qd[2])));
        QG_DONE_IF_FLIPPED(Tk., zaxis_z);
        if (half == 0) {
            if (od == 21) { srow[18] = srow[30]; srow[19] = srow[31]; srow[20] = srow[32]; }
            srow[od] = reward; srow[od + 1] = done ? 1.f : 0.f;
        }
        wave_sync();
        {
            float *dst = R.packed + (size_t)kstep * slot_out + (size_t)env0 * row;
            QG_TILE_COPY_OUT(dst, tile, lane, total, row);
        }
        wave_sync();
        const bool rst = done && Tk.auto_reset;
#pragma unroll
        for (int c6 = 0; c6 < 6; ++c6) ctrl_reg[c6] = aclip[c6];
        if (rst) {
            QG_BASE_RESET(B, nstep, C.qpos0, Tk., P, env, episode);
            episode += 1;
#pragma unroll
            for (int i = 0; i < 3; ++i) {
                L.q[i] = f2(C.qpos0[7 + i]); L.qd[i] = f2(0.f); L.act[i] = f2(0.f);
            }
#pragma unroll
            for (int c6 = 0; c6 < 6; ++c6) ctrl_reg[c6] = Tk.default_ctrl[6 * half + c6];
        }
    }

    if (lead) {
        QG_BASE_STORE(B, nstep, P.st, QG_PUT, n, env);
        P.st.episode[env] = episode;
    }
    if (live && R.count > 0) {
#pragma unroll
        for (int c = 0; c < 2; ++c) {
#pragma unroll
            for (int i = 0; i < 3; ++i) {
                const int j = 3 * (2 * half + c) + i;
                QG_HINGE_STORE(c == 0 ? L.q[i].x : L.q[i].y, c == 0 ? L.qd[i].x : L.qd[i].y, c == 0 ? L.act[i].x : L.act[i].y, P.st, QG_PUT, n, env, j);
                if (P.track_ctrl) P.st.ctrl[j * n + env] = ctrl_reg[3 * c + i];
            }
        }
    }
}

// ---- host side: the launchers, and every leaf of the mapping ----------------------------------------------------------------------
template <int WAVES, bool WALK, bool PO = false> static void launch_pair(const StepLaunch &L) {
    static_assert(WAVES == 1 || WAVES == 4, "one-wave or four-wave workgroups");
    L.s->last_step_kernel = step_kernel_code<WAVES, WALK, PO>(KF_PAIR);
    hipLaunchKernelGGL((qg_step_kernel_pair<WAVES, WALK, PO>), wave_grid(pair_blocks(L.s), WAVES), dim3(QGK_WAVE * WAVES), 0, L.stream, L.s->d_task,
                       L.P, walk_arg<WALK>(L.walk), po_arg<PO>(L.po));
}
template <int WAVES> static void launch_pair_multi(const qg_sim *s, hipStream_t st, const KStepArgs &P, const KResident &R) {
    static_assert(WAVES == 1 || WAVES == 4, "one-wave or four-wave workgroups");
    s->last_step_kernel = step_kernel_code<WAVES>(KF_PAIR_MULTI);
    hipLaunchKernelGGL((qg_step_kernel_pair_multi<WAVES>), wave_grid(pair_blocks(s), WAVES), dim3(QGK_WAVE * WAVES), 0, st, s->d_task, P, R);
}

// Every leaf names the instantiation it launches.
void qg_select_step_pair(const StepLaunch &L) {      // (the compiled-in robot only)
    QG_PHASE_UNIT();
    const qg_sim *s = L.s;
    const bool walk = L.walk, po = L.po;
    if (po) launch_pair<4, true, true>(L);                             // qg_po_fusable(): four-wave workgroups
    else if (walk && pair_wg4(s)) launch_pair<4, true>(L);
    else if (walk) launch_pair<1, true>(L);
    else if (pair_wg4(s)) launch_pair<4, false>(L);
    else launch_pair<1, false>(L);
}

void qg_select_seq_pair(const qg_sim *s, hipStream_t st, const KStepArgs &P, const KResident &R) {
    QG_PHASE_UNIT();
    if (pair_wg4(s)) launch_pair_multi<4>(s, st, P, R);
    else launch_pair_multi<1>(s, st, P, R);
}
