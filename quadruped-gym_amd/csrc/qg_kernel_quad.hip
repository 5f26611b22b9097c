// qg_kernel_quad.hip -- the one-leg-per-lane step kernels in a code object of their own: qg_step_kernel_quad, its sequence form
// qg_step_kernel_quad_multi, their launchers and the leaves of the QG_MAP_QUAD mapping (entry points: qg_step_launch.h).
// The one-env-per-lane kernel qg_step_kernel (QG_MAP_LANE, on request only) is here as well: its table-driven form and the table-driven
// forms of the kernels above inline the same leg_pass instantiation, and device functions are internal to a code object, so what
// the compiler derives for that function from all of its callers -- and with it every listing that inlines it -- changes when the
// callers are split over two units (profiles/r17/asm_diff.txt).
#include "qg_step_dev.h"
#include "qg_step_launch.h"

// ------------------------------------------------------------------------------------------
// env-step kernel, ONE ENV PER LANE: one launch = frame_skip substeps + sensor pack + rewards +
// terminations (+ auto-reset) for every env.  grid = ceil(n / 64) workgroups of one wave.
// ------------------------------------------------------------------------------------------
template <bool BAKED>
__global__ __launch_bounds__(QGK_WAVE) void qg_step_kernel(const KModel *__restrict__ Mp, const KTask *__restrict__ T, KStepArgs P) {
    const KModel *M = &table<BAKED>(Mp);
    __shared__ float lds[QG_LDS_SLOTS * 64];
    __shared__ float tile[QG_OBS_TILE_FLOATS];
    const int lane = threadIdx.x;
    const int env0 = blockIdx.x * QGK_WAVE;
    const int n = P.n;
    const bool live = env0 + lane < n;
    const int env = live ? env0 + lane : n - 1;   // tail lanes shadow the last env; their stores are masked

    // ---- load state (coalesced: lane i reads base + i*4 of every field) -------------------
    BaseState B;
    QG_BASE_LOAD(B, P.st, QG_AT, n, env);
    int nstep = P.st.nstep[env];
    // action: clip to the action space [-1, 1] (quadruped.py:160), then to the servo's ctrlrange
    float ssq = 0.f;
    float aclip[12];
    {
        const float4 *ap = reinterpret_cast<const float4 *>(P.actions + (size_t)env * 12);
        float4 a0 = ap[0], a1 = ap[1], a2 = ap[2];
        float av[12] = {a0.x, a0.y, a0.z, a0.w, a1.x, a1.y, a1.z, a1.w, a2.x, a2.y, a2.z, a2.w};
#pragma unroll
        for (int j = 0; j < 12; ++j) {
            float a = fminf(fmaxf(av[j], -1.f), 1.f);
            aclip[j] = a;
            ssq = fmaf(a, a, ssq);
            lds[LU(j) * 64 + lane] = fminf(fmaxf(a, M->link[BAKED ? j % 3 : j].ctrl_lo), M->link[BAKED ? j % 3 : j].ctrl_hi);
            QG_HINGE_LOAD(lds[LQ(j) * 64 + lane], lds[LQD(j) * 64 + lane], lds[LACT(j) * 64 + lane], P.st, QG_AT, n, env, j);
        }
    }

    // ---- frame_skip physics substeps (quadruped.py:163-165) ----------------------------------
    SensorOut so;
    float jpos[12];
    const int fs = T->frame_skip;
    const bool lag = T->sensor_lag != 0;
#pragma unroll 1
    for (int s = 0; s < fs; ++s) substep<BAKED>(Mp, lds, lane, B, lag && (s == fs - 1), so, jpos);
    nstep += fs;
    if (!lag) {   // un-lagged sensors: one extra forward pass on a scratch copy of the state
        BaseState B2 = B;
        float keep[36];
#pragma unroll
        for (int j = 0; j < 36; ++j) keep[j] = lds[j * 64 + lane];
        substep<BAKED>(Mp, lds, lane, B2, true, so, jpos);
#pragma unroll
        for (int j = 0; j < 36; ++j) lds[j * 64 + lane] = keep[j];
    }

    // ---- rewards and terminations on the post-step state (README.md:64-90) ----------------
    QG_REWARD_TERMS(T->, B, ssq, nstep);
    QG_DONE_IF_FLIPPED(T->, so.zaxis.z);
    {   // (base first, hinges second: not the rounding of QG_DONE_IF_BAD_STATE)
        float probe = B.pw.x + B.pw.y + B.pw.z + B.qw + B.vw.x + B.vw.y + B.vw.z + B.wb.x + B.wb.y + B.wb.z;
#pragma unroll
        for (int j = 0; j < 12; ++j) probe += lds[LQ(j) * 64 + lane] + lds[LQD(j) * 64 + lane];
        done = done || state_is_bad(probe);
    }

    // ---- outputs: stage rows in LDS, then store the wave's contiguous chunk coalesced ------
    const int od = T->obs_mode == 1 ? 21 : 33;
    const int row = P.packed ? od + 2 : od;
    {
        float *r = tile + lane * row;
        write_obs_row(r, od, jpos, so);
        if (P.packed) { r[od] = reward; r[od + 1] = done ? 1.f : 0.f; }
    }
    __syncthreads();
    {
        const int live_envs = min(QGK_WAVE, n - env0);
        const int total = live_envs * row;
        float *dst = (P.packed ? P.packed : P.obs) + (size_t)env0 * row;
        for (int e = lane; e < total; e += QGK_WAVE) dst[e] = tile[e];
    }
    if (live && !P.packed) {
        P.reward[env] = reward;
        P.done[env] = done ? 1 : 0;
    }
    QG_COMPS_STORE(live, P, env);

    // ---- auto-reset (VecEnv semantics) and state write-back ---------------------------------
    const bool rst = done && T->auto_reset;
    if (rst) QG_BASE_RESET(B, nstep, M->qpos0, T->, P, env, P.st.episode[env]);
    if (live) {
        QG_BASE_STORE(B, nstep, P.st, QG_PUT, n, env);
        if (rst) P.st.episode[env] += 1;
#pragma unroll
        for (int j = 0; j < 12; ++j) {
            QG_HINGE_STORE(rst ? M->qpos0[7 + j] : lds[LQ(j) * 64 + lane], rst ? 0.f : lds[LQD(j) * 64 + lane], rst ? 0.f : lds[LACT(j) * 64 + lane], P.st, QG_PUT, n, env, j);
        }
        if (P.track_ctrl) {
#pragma unroll
            for (int j = 0; j < 12; ++j) P.st.ctrl[j * n + env] = rst ? T->default_ctrl[j] : aclip[j];
        }
    }
}

// ------------------------------------------------------------------------------------------
// env-step kernel, ONE LEG PER LANE: the four lanes 4e..4e+3 of a quad share env e, lane k owns
// leg k (and a quarter of the FRAME's contact points); the base prelude, the 6x6 base solve and
// the base integration run redundantly in all four lanes; the leg contributions to the base
// block (Schur complements, 33 numbers) are summed over the quad with DPP quad_perm moves --
// no LDS, no run-time indexed arrays.  A wave carries 16 envs, so 4096 envs fill 256 waves
// instead of 64: at batch sizes that cannot fill the chip with one env per lane this cuts the
// instructions per wave (= the time, a lone wave issues one VALU instruction per ~4.5-5 cycles) ~3.5x.
// BAKED variant: the compiled-in robot, whose legs are quarter-turn copies of one another (constants become literals).
// Generic variant: any model numbers; the tables are staged in LDS and each lane reads its own leg's rows.
// ------------------------------------------------------------------------------------------
struct LegState {
    float q[3], qd[3], act[3], u[3];
    float sc[6];      // sin, cos of (q[i] - ref_i), advanced with the hinge
};

// Ordered for low register pressure: the leg pass (the widest live set) runs first with only the base context alive;
// the FRAME terms are built afterwards; sensors go straight to the LDS tile; the rotation is rebuilt at integration.
// The one-leg-per-lane kernel of the compiled-in robot at ONE wave per SIMD takes the packed prelude / integration of the
// one-link-per-lane kernel (a lone wave pays per instruction: 2 109 -> 2 072 per substep, 17.74 -> 17.48 us at 8 192 envs, 18.3 -> 18.1
// at 16 384, sequence form 15.4 -> 15.2); at two waves per SIMD they measured 1.2 % slower and with the generic robot's tables 7 %
// slower (profiles/r04/quad_packed_prelude_ab.txt), so those keep the plain forms.
template <bool PKQ> DEV BaseCtx quad_prelude(const KModel &C, const BaseState &B) {
    if constexpr (PKQ) return pk3::base_prelude_unit(C, B);
    else return base_prelude<true>(C, B);
}
template <bool PKQ> DEV void quad_integrate(const BaseCtx &c, float h, V3 wdot, V3 acl, BaseState &B) {
    if constexpr (PKQ) pk3::base_integrate_unit(c, h, wdot, acl, B);
    else base_integrate<true>(c, h, wdot, acl, B);
}
// LOWREG: rebuild the base context (cheap) instead of keeping it alive across the leg pass -- pays off once two waves
// share a SIMD (register cap 256), costs ~2 % when a wave has the register file to itself.
// BAKED: the compiled-in robot, constants are literals and the lane works in its leg's quarter-turn frame.  Otherwise `C`
// is the model table staged in LDS and every lane reads the constants of its own leg (k) from it -- any model numbers.
// DYN: per-env dynamics (D) and, with `xon` (wave-uniform), the external wrenches X of this lane's leg and of the FRAME
template <bool BAKED, bool LOWREG, bool DYN = false>
DEV void substep_quad(const KModel &C, float cm, float sm, BaseState &B, LegState &L, bool want_sensors, float *__restrict__ row, int k, float &zaxis_z,
                      const KDyn &D = KDyn{}, bool xon = false, const KXfrcQuad *X = nullptr) {
    const float h = C.h;
    const BaseCtx bc0 = quad_prelude<BAKED && !LOWREG>(C, B);
    V3 gb_keep;
    Sym6 Ic;
    SV fc, Fu;
    float Y0[6], Y1[6], Y2[6], u[3];
    {
        const BaseCtx &bc = bc0;
        gb_keep = bc.gb;
        if (want_sensors) {          // the step's sensordata describes the state at the start of its last substep
            zaxis_z = bc.cz.z;
            row[3 * k + 0] = L.q[0]; row[3 * k + 1] = L.q[1]; row[3 * k + 2] = L.q[2];
            if (k == 0) {
                row[15] = B.wb.x; row[16] = B.wb.y; row[17] = B.wb.z;
                row[18] = B.pw.x; row[19] = B.pw.y; row[20] = B.pw.z;
                row[21] = B.vw.x; row[22] = B.vw.y; row[23] = B.vw.z;
                row[24] = bc.cx.x; row[25] = bc.cx.y; row[26] = bc.cx.z;
                row[27] = bc.cz.x; row[28] = bc.cz.y; row[29] = bc.cz.z;
                row[30] = bc.vb.x; row[31] = bc.vb.y; row[32] = bc.vb.z;
            }
        }
        Sym6 YFt;
        SV F[3];
        float Hd[3], H01, H02, H12, bj[3];
        if constexpr (BAKED) {
            // this lane's leg, in the frame turned by its quarter turn: there it is leg 0
            Fr Ek = {v3(cm, sm, 0.f), v3(-sm, cm, 0.f), v3(0.f, 0.f, 1.f)};
            leg_pass<float, true, true, LOWREG, false>(C, 0, Ek, L.q, L.qd, L.act, bc, B.pw.z, h, Ic, fc, F, Hd, H01, H02, H12, bj, L.sc);
        } else {
            Fr E0 = {v3(1.f, 0.f, 0.f), v3(0.f, 1.f, 0.f), v3(0.f, 0.f, 1.f)};
            if constexpr (DYN)
                leg_pass<float, false, false, LOWREG, false, DYN>(C, k, E0, L.q, L.qd, L.act, bc, B.pw.z, h, Ic, fc, F, Hd, H01, H02, H12, bj, L.sc, D,
                                                                  xon, X->link);
            else
                leg_pass<float, false, false, LOWREG, false, DYN>(C, k, E0, L.q, L.qd, L.act, bc, B.pw.z, h, Ic, fc, F, Hd, H01, H02, H12, bj, L.sc, D);
        }
        leg_eliminate(F, Hd, H01, H02, H12, bj, Y0, Y1, Y2, u, YFt, Fu);
        sub(Ic, YFt);                       // this leg's Schur complement
    }
    float x6[6];
    {
        const BaseCtx bc = LOWREG ? quad_prelude<BAKED && !LOWREG>(C, B) : bc0;      // rebuilt (cheap) rather than kept alive across the leg pass
        SV p0;
        Sym6 Ic0;
        frame_body<DYN>(C, bc, h, p0, Ic0, D);
        SV b;
        {   // FRAME contact: this lane evaluates its quarter turn of the three base sample points
            float wsum = 0.f;
            V3 s = v3(0.f, 0.f, 0.f);
            float zb = C.contact_margin - B.pw.z;
#pragma unroll
            for (int o = 0; o < 3; ++o) {
                if constexpr (BAKED) {
                    V3 r0 = ld3(C.cp0[4 * o]);
                    contact_point(v3(cm * r0.x - sm * r0.y, sm * r0.x + cm * r0.y, r0.z), bc.n, zb, wsum, s);
                } else {
                    contact_point(ld3(C.cp0[3 * k + o]), bc.n, zb, wsum, s);   // any partition of the 12 points over the 4 lanes
                }
            }
            wsum = quad_sum(wsum);
            // the sums over the quad sit right in front of their uses: the compiler fuses a DPP move into the add that consumes it only
            // when the two end up within a few instructions of each other in one basic block (33 unfused moves per substep otherwise)
            quad_sum(Ic);
            fc.a = quad_sum(fc.a); fc.l = quad_sum(fc.l);
            Fu.a = quad_sum(Fu.a); Fu.l = quad_sum(Fu.l);
            add(Ic0, Ic);
            b.a = v3(0.f, 0.f, 0.f) - Fu.a - p0.a - fc.a;
            b.l = v3(0.f, 0.f, 0.f) - Fu.l - p0.l - fc.l;
            // Wave-uniform skip: under actuation the robot stands on its feet and the FRAME practically never touches the
            // floor; when no env of the wave has a FRAME sample point below the margin every term below is exactly zero.
            // (A/B on one box: +3.4 % at 4096 envs, +6.5 % at 262 144.  The same skip per leg link does NOT pay: a taken
            // branch over a large block stalls the instruction fetch of a wave that is alone on its SIMD.)
            // The branch updates the assembled block IN PLACE (round 3): with the block assembled after it, the usual path -- no
            // contact -- had to materialise the FRAME's constant entries as the other arm of a phi, 17 moves per substep.
            if (__any(wsum > 0.f)) {
                s = quad_sum(s);
                Fr E0 = {v3(1.f, 0.f, 0.f), v3(0.f, 1.f, 0.f), v3(0.f, 0.f, 1.f)};
                SV fe;
                if constexpr (DYN) contact_finish(wsum, s, E0, v3(0.f, 0.f, 0.f), bc.n, bc.V0, D.kc, D.cc, C.contact_inv_ramp, D.mu, h, fe, Ic0);
                else contact_finish(wsum, s, E0, v3(0.f, 0.f, 0.f), bc.n, bc.V0, C.contact_k, C.contact_c, C.contact_inv_ramp, C.contact_mu, h, fe, Ic0);
                b.a = b.a + fe.a;
                b.l = b.l + fe.l;
            }
            if constexpr (DYN) {
                if (xon) {      // the FRAME's external wrench (and push): every lane of the env, as the rest of the base block
                    const SV xw = xfrc_spatial(bc, X->frame, X->com0);
                    b.a = b.a + xw.a;
                    b.l = b.l + xw.l;
                }
            }
        }
        if constexpr (BAKED) pk3::base_solve(Ic0, b, x6);      // packed row pairs: fewer instructions for a wave alone on its SIMD, as many
        else base_solve(Ic0, b, x6);                            // issue cycles at two waves per SIMD; the generic robot's register budget has no room for the pairs
    }
    V3 wdot = v3(x6[0], x6[1], x6[2]);
    V3 acl = v3(x6[3], x6[4], x6[5]);
    if (want_sensors && k == 0) {
        row[12] = acl.x - gb_keep.x; row[13] = acl.y - gb_keep.y; row[14] = acl.z - gb_keep.z;   // accelerometer
    }
    // back-substitution and integration of this lane's three hinges
    const float *Y[3] = {Y0, Y1, Y2};
#pragma unroll
    for (int i = 0; i < 3; ++i) {
        float acc = u[i];
#pragma unroll
        for (int r = 0; r < 6; ++r) acc = fmaf(-Y[i][r], x6[r], acc);
        L.qd[i] = fmaf(h, acc, L.qd[i]);
        L.q[i] = fmaf(h, L.qd[i], L.q[i]);
        hinge_advance(h * L.qd[i], L.sc[2 * i], L.sc[2 * i + 1]);
        L.act[i] = fmaf(L.u[i] - L.act[i], link_of<BAKED>(C, k, i).act_decay, L.act[i]);
    }
    {
        const BaseCtx bc = LOWREG ? quad_prelude<BAKED && !LOWREG>(C, B) : bc0;
        quad_integrate<BAKED && !LOWREG>(bc, h, wdot, acl, B);
    }
}

// WPE = waves per SIMD the register allocation is capped for: 1 (all 512 registers) is fastest while the grid has at
// most one wave per SIMD (n <= 16384); 2 lets a second wave share the SIMD once the grid is larger.
// WALK: the walking task layer fused in (qg_walk_dev.h) -- the whole WalkingQuadrupedEnv.step (walking_quad.py:128-148) is this
// one launch: settling-time action mask and the estimator update of the lane's three control channels in the prologue (they
// need data.ctrl of the PREVIOUS step, which is still in place there), ideal-position integration, the eleven reward terms and
// the episode bookkeeping in the epilogue on the sensor row the wave has just staged in LDS.
// WAVES: waves per workgroup (1, or 4 = one per SIMD of a CU for grids of more than 256 waves: fewer workgroups to dispatch,
// see qg_step_kernel_pair); the waves of a workgroup do not interact.
// PO (with WALK; round 3): the partially observable observation pack fused in as in qg_step_kernel_pair<.., PO> (history copy on the
// substep loop, frame by the env's lead lane, new frames written by the wave); the register-capped development variants (WPE > 2) have none.
// HELP (with WALK, two-waves-per-SIMD register budget): as in qg_step_kernel_link<.., HELP> -- WAVES more waves per workgroup run the
// estimator update of their partner wave's channels while that wave goes straight into the substep loop; for grids of at most one
// physics wave per SIMD (<= 16 384 envs), where the partner's issue slots are otherwise idle.  With the observation pack the helper also
// copies the history rows ring -> out (po_copy_history_now), so that nothing of the copy rides on the physics wave's substep loop: the
// first version, which kept the in-loop copy with the physics wave, lost to the one-role kernel (48.6 against 46.9 us per step at
// 16 384 envs, frame_skip 10: at this register budget the copy cannot park in AGPRs across a substep); this one measures 45.4.
// DYN (generic tables only): per-env dynamics -- `Mp` is a KModelDyn and each lane takes its env's row into registers (dyn_load);
// in wrench mode also its leg's and the FRAME's external wrench rows
template <int WPE, bool BAKED, bool WALK = false, int WAVES = 1, bool PO = false, bool HELP = false, bool DYN = false>
__global__ __launch_bounds__(QGK_WAVE * WAVES * (HELP ? 2 : 1), WPE) void qg_step_kernel_quad(const KModel *__restrict__ Mp, const KTask *__restrict__ T, KStepArgs P,
                                                                             const typename WalkArgT<WALK>::type WK,
                                                                             const typename PoArgT<PO>::type PK) {
    static_assert(WALK || !PO, "the observation pack rides on the walking task layer");
    static_assert(WPE == 1 || WPE == 2, "register budget: one wave per SIMD (all 512 registers) or two");
    static_assert(!HELP || (WALK && WPE == 2), "helper waves: the walking forms at the two-waves-per-SIMD register budget");
    static_assert(!DYN || (!BAKED && !HELP), "per-env dynamics: the table-driven variants");
    constexpr bool PO_COPY = PO && !HELP;          // HELP: the helper wave copies the history rows, nothing of it rides on the substep loop
    __shared__ float tile_all[WAVES][QGK_QUAD_ENVS * 35];
    __shared__ KModel smodel;                       // generic variant: the link / joint tables staged in LDS (3.2 KB)
    constexpr bool RWDH = HELP && !PO;              // walking without the observation pack: the helper wave also evaluates the reward
    constexpr bool POH = HELP && PO;                // with it: the helper wave builds the new frame and writes the rows, the reward stays here
    __shared__ float s_est[HELP ? WAVES : 1][QGK_WAVE][6];      // HELP: (f_est, a_est) of the lane's three channels, helper -> physics wave
    __shared__ float s_done[HELP ? WAVES : 1][QGK_QUAD_ENVS];   // HELP: the step's termination flags, physics -> helper
    __shared__ float s_q[POH ? WAVES : 1][QGK_QUAD_ENVS][4];    // POH: data.qpos[3:7] as the step leaves it (after the auto-reset), physics -> helper
    const int lane = threadIdx.x & (QGK_WAVE - 1);
    const int wave = HELP ? ((threadIdx.x >> 6) % WAVES) : (threadIdx.x >> 6);      // HELP: waves WAVES .. 2 WAVES - 1 shadow waves 0 .. WAVES - 1
    const bool helper = HELP && (int)(threadIdx.x >> 6) >= WAVES;
    float *tile = tile_all[wave];
    QG_MARK(0);
    QG_STAGE_MODEL(C, BAKED, smodel, Mp, QGK_WAVE * WAVES * (HELP ? 2 : 1));
    const int k = lane & 3;                         // leg of this lane
    const int el = lane >> 2;                       // env within the wave
    const int env0 = (blockIdx.x * WAVES + wave) * QGK_QUAD_ENVS;
    const int n = P.n;
    const bool live = env0 + el < n;
    const int env = live ? env0 + el : n - 1;       // tail quads shadow the last env; their stores are masked
    // quarter turn of this lane's leg: (cos, sin)(90 deg * k)
    const float cm = (k == 0) ? 1.f : (k == 2) ? -1.f : 0.f;
    const float sm = (k == 1) ? 1.f : (k == 3) ? -1.f : 0.f;
    KDyn D = {};
    if constexpr (DYN) D = dyn_load(Mp, C, n, env);     // this env's dynamics row, once per launch
    // external wrenches (wrench mode: KModelDyn::xfrc != NULL, wave-uniform): the rows of this lane's three links and the FRAME's with
    // this launch's push, once per launch; nothing is loaded with the mode off
    bool xon = false;
    typename XfrcQuadT<DYN>::type XQ = {};
    if constexpr (DYN) {
        const KModelDyn *Md = reinterpret_cast<const KModelDyn *>(Mp);
        xon = Md->xfrc != nullptr;
        if (xon) {
#pragma unroll
            for (int i = 0; i < 3; ++i) XQ.link[i] = xfrc_row(Md->xfrc, env, 1 + 3 * k + i);
            XQ.frame = xfrc_frame(Md, P, env, T->frame_skip);
            XQ.com0 = v3(Md->com0[0], Md->com0[1], Md->com0[2]);
        }
    }

    if constexpr (HELP) {
        if (helper) {
            const int ht[3] = {env * 12 + 3 * k + 0, env * 12 + 3 * k + 1, env * 12 + 3 * k + 2};
            const int hcalls = WK.S.calls[env];
            float hx[3], hf[3] = {0.f, 0.f, 0.f}, ha[3] = {0.f, 0.f, 0.f};
            // RWDH: what the reward needs and does not come out of the physics, loaded ahead of the estimator's stores
            float h_aclip[3] = {0.f, 0.f, 0.f}, h_wprev[3] = {0.f, 0.f, 0.f};
            WalkChanTargets h_wtg[3] = {};
            WalkEnvIn hwin = {};
            if constexpr (HELP) {
                const bool hsettle = P.st.nstep[env] < WK.P.settle_substeps;        // data.time < settling_time (walking_quad.py:142-143)
                if constexpr (RWDH) walk_ldv<3>(WK.S.prev_ctrl + ht[0], h_wprev);
#pragma unroll
                for (int i = 0; i < 3; ++i) {
                    if constexpr (RWDH) h_wtg[i] = walk_channel_targets(WK.P, 3 * k + i);
                    float a_in = P.actions[(size_t)env * 12 + 3 * k + i];
                    if (hsettle) a_in = WK.P.joint_centers[3 * k + i];
                    h_aclip[i] = fminf(fmaxf(a_in, -1.f), 1.f);                      // quadruped.py:160
                }
                if (k == 0) {
                    hwin = walk_env_load(WK.S, n, env);
                    hwin.episode_key = P.st.episode[env];      // not advanced yet: the physics wave does that behind the barrier
                }
            }
#pragma unroll
            for (int i = 0; i < 3; ++i) hx[i] = P.st.ctrl[(3 * k + i) * n + env];   // data.ctrl of the PREVIOUS step (walking_quad.py:136)
            WalkEstIn<3> hw;
            walk_estimator_load_n<3, true>(WK.P, WK.S, n, ht, hcalls, hw, live);     // block entry in rolled groups: no scratch at 256 registers
            if (live) walk_estimator_finish_n<3>(WK.P, WK.S, n, ht, hx, hcalls, hw, hf, ha);    // math_utils.py:53-131
#pragma unroll
            for (int i = 0; i < 3; ++i) { s_est[wave][lane][i] = hf[i]; s_est[wave][lane][3 + i] = ha[i]; }
            if constexpr (PO) {
                int slot = PK.S.head[env] + 1;                     // the ring slot the NEW frame will take
                if (slot >= PK.P.window) slot = 0;
                if (PK.P.window > 1) po_copy_history_now<4>(PK.P, PK.S, (size_t)env * (PK.P.window * QG_PO_FRAME), slot, k, PK.out, live);
            }
            // (partner: the physics waves' __syncthreads() behind their auto-reset block, "partner of the helper waves' one barrier"
            // below.  Exactly one barrier per wave on every path: a second one in either role, or a return in front of it, deadlocks
            // the workgroup -- and on this pool a hung workgroup is a hung GPU.)
            __syncthreads();      // the one barrier of the workgroup: behind it the physics waves read s_est and write what this wave read
            if constexpr (RWDH) {
                // the reward of the step, on the sensor tile the physics wave has finished (LDS), while that wave goes on with the resets and
                // the state stores
                const bool hdone = s_done[wave][el] != 0.f;
                WalkSums sum = {0.f, 0.f, 0.f, 0.f};
                if (live) {
#pragma unroll
                    for (int i = 0; i < 3; ++i) walk_channel_terms(WK.S, env, 3 * k + i, h_wtg[i], h_aclip[i], h_wprev[i], hf[i], ha[i], sum);
                    walk_stv<3>(WK.S.prev_ctrl + (size_t)env * 12 + 3 * k, h_aclip);                         // previous_ctrl moves on (:260-262)
                }
                sum.cost = quad_sum(sum.cost); sum.posture = quad_sum(sum.posture); sum.amp = quad_sum(sum.amp); sum.frq = quad_sum(sum.frq);
                if (live && k == 0)
                    walk_reward_env(WK.P, WK.S, n, env, tile + el * 35, sum, hwin, hdone, P.reward, WK.comps, WK.sample, P.seed, P.env_index_base);
            }
            if constexpr (POH) {
                // the observation pack's new frame and rows, on the finished sensor tile and the orientation the physics wave handed over,
                // while that wave evaluates the reward and stores the state
                BaseState hb = {};
                hb.qw = s_q[wave][el][0]; hb.qx = s_q[wave][el][1]; hb.qy = s_q[wave][el][2]; hb.qz = s_q[wave][el][3];
                const int h_live_envs = max(0, min(QGK_QUAD_ENVS, n - env0));
                po_wave_epilogue<QGK_QUAD_ENVS, 4, WAVES, true>(PK, WK, P, n, env, env0, h_live_envs, wave, lane, el, k, live, live && k == 0, PoEnvIn{},
                                                                tile + el * 35, hb, hwin, s_done[wave][el] != 0.f, h_aclip);
            }
            return;
        }
    }
    BaseState B;
    QG_BASE_LOAD(B, P.st, QG_AT, n, env);
    quat_unit(B);   // unit quaternion once per launch (qg_set_state may hand in any length); the substeps keep it normalised (base_prelude<UNIT>)
    LegState L;
    const int nstep0 = P.st.nstep[env];
    float aclip0[3];
    bool settle = false;
    int calls = 0;
    WalkEnvIn win = {};
    if constexpr (WALK) {
        settle = nstep0 < WK.P.settle_substeps;                     // data.time < settling_time (walking_quad.py:142-143)
        if constexpr (!HELP) calls = WK.S.calls[env];
    }
    // WALK: every load of the task layer goes out here, among the state loads, and every store of its prologue part comes after the
    // last load of the kernel's prologue (a load behind a store would wait for that store: vmcnt counts in order)
    const int tt[3] = {env * 12 + 3 * k + 0, env * 12 + 3 * k + 1, env * 12 + 3 * k + 2};     // task state: [n][12]
    float xx[3] = {0.f, 0.f, 0.f}, wprev[3] = {0.f, 0.f, 0.f}, wf[3] = {0.f, 0.f, 0.f}, wa[3] = {0.f, 0.f, 0.f}, a_eff[3] = {0.f, 0.f, 0.f};
    WalkEstIn<3> west;
    WalkChanTargets wtg[3] = {};
    if constexpr (WALK) {
#pragma unroll
        for (int i = 0; i < 3; ++i) if constexpr (!HELP) xx[i] = P.st.ctrl[(3 * k + i) * n + env];   // data.ctrl of the PREVIOUS step: what the estimator takes (walking_quad.py:136)
        walk_ldv<3>(WK.S.prev_ctrl + tt[0], wprev);   // previous_ctrl of the control cost (:260-262)
        if constexpr (!HELP) walk_estimator_load_n<3>(WK.P, WK.S, n, tt, calls, west);
        if constexpr (WPE == 1) {
#pragma unroll
            for (int i = 0; i < 3; ++i) wtg[i] = walk_channel_targets(WK.P, 3 * k + i);
            if (k == 0) {                                   // what the reward epilogue reads: fetched now, behind the physics
                win = walk_env_load(WK.S, n, env);
                win.episode_key = P.st.episode[env];        // not advanced yet: the key of the episode that begins if this one ends
            }
        }
    }
#pragma unroll
    for (int i = 0; i < 3; ++i) {
        const int j = 3 * k + i;
        float a_in = P.actions[(size_t)env * 12 + j];
        if constexpr (WALK) {
            if (settle) a_in = WK.P.joint_centers[j];                // the joint centres while the robot settles
            a_eff[i] = a_in;
        }
        float a = fminf(fmaxf(a_in, -1.f), 1.f);    // quadruped.py:160
        aclip0[i] = a;
        L.u[i] = fminf(fmaxf(a, link_of<BAKED>(C, k, i).ctrl_lo), link_of<BAKED>(C, k, i).ctrl_hi);
        QG_HINGE_LOAD(L.q[i], L.qd[i], L.act[i], P.st, QG_AT, n, env, j);
        sincos_f(L.q[i] - link_of<BAKED>(C, k, i).ref, L.sc[2 * i], L.sc[2 * i + 1]);
    }
    // PO: the env's filter state (lead lane) and ring position, this lane's share of its env's row copy ring -> out -- its loads go
    // out here, among the state loads and before the task layer's stores (see qg_step_kernel_pair)
    PoEnvIn pin = {};
    PoCopyState pcs = {};
    const int live_envs = max(0, min(QGK_QUAD_ENVS, n - env0));
    const int el_c = min(el, max(live_envs - 1, 0));     // row of this lane's env in the wave's block (tail lanes: the last live one)
    unsigned long long po_ring = 0, po_out = 0;          // the wave's block of the frame ring / of the output rows (scalar registers)
    if constexpr (PO) {
        const size_t po_block = (size_t)(live_envs > 0 ? env0 : 0) * (size_t)(PK.P.window * QG_PO_FRAME);
        po_ring = po_uniform_addr(PK.S.stack + 2 * po_block);
        po_out = po_uniform_addr(PK.out + po_block);
        if (k == 0) pin = po_env_load(PK.S, n, env);
        if constexpr (PO_COPY) po_row_copy_init<4>(PK.P, el_c, PK.S.head[env], k, pcs);
    }
    if constexpr (WALK) {
        // every state value is in its register before the first store of the task layer is issued: the waits for those loads
        // would otherwise sit behind the stores (vmcnt is in order) right in front of the substep loop
        asm volatile("" :: "v"(B.pw.x), "v"(B.pw.y), "v"(B.pw.z), "v"(B.qw), "v"(B.qx), "v"(B.qy), "v"(B.qz), "v"(B.vw.x), "v"(B.vw.y), "v"(B.vw.z),
                     "v"(B.wb.x), "v"(B.wb.y), "v"(B.wb.z), "v"(L.q[0]), "v"(L.q[1]), "v"(L.q[2]), "v"(L.qd[0]), "v"(L.qd[1]), "v"(L.qd[2]),
                     "v"(L.act[0]), "v"(L.act[1]), "v"(L.act[2]), "v"(L.u[0]), "v"(L.u[1]), "v"(L.u[2]) : "memory");
        if (live) {
            if constexpr (!HELP) walk_estimator_finish_n<3>(WK.P, WK.S, n, tt, xx, calls, west, wf, wa);    // math_utils.py:53-131
            walk_stv<3>(WK.S.eff_actions + (size_t)env * 12 + 3 * k, a_eff);                        // the action actually applied (the PO pack reads it)
        }
    }

    // the sensor values of the step go straight into this env's row of the output tile (full 33-value layout; the
    // 21-value pack is compacted below)
    float *srow = tile + el * 35;
    float zaxis_z = 1.f;
    const int fs = T->frame_skip;
    const bool lag = T->sensor_lag != 0;
    // Un-lagged sensors (task.sensor_lag = 0) take one extra forward pass whose state changes are discarded: the same loop body
    // runs once more with the state parked in LDS meanwhile -- one copy of the substep code and no extra live registers.
    // (Register caps for three / four waves per SIMD were built and measured in round 2 -- 197 / 255 us against 200 us at 262 144 envs,
    // slower below: profiles/r02/wpe_ab.txt, docs/EXPERIMENTS.md -- and removed in round 4: WPE is 1 or 2.)
    int env_e = env, k_e = k;
    int nstep;
    float aclip[3];
    {
        // Code placement: a wave that is alone on its SIMD is sensitive to where the 14 KB loop body falls relative to the
        // instruction-fetch lines -- the same loop, shifted by one dword through an unrelated edit of the prologue, measured
        // 18.57 instead of 18.36 us per launch at 4096 envs (same-box A/B of eight paddings).  Pinning the loop to a 64-byte
        // boundary makes its layout independent of what precedes it.
        QG_MARK(1);                                  // state in registers, prologue stores issued
        asm volatile(".p2align 6");
        // the history copy's loads at the head of a substep and its stores at the tail -- or both at the head where the registers in
        // between are taken: with two waves per SIMD the partner covers the latency, and the table-driven variant has none to spare
        constexpr bool PO_DEFER = PO && WPE == 1 && BAKED;
#pragma unroll 1
        for (int s = 0; s < fs; ++s) {
            PoCopyRegs<PO ? QG_PO_COPY_K : 1> pcr;
            if constexpr (PO_COPY) po_row_copy_load<QG_PO_COPY_K, 4>(PK.P, po_ring, k, s == 0, pcs, pcr);
            if constexpr (PO_COPY && !PO_DEFER) po_row_copy_store<QG_PO_COPY_K, 4>(PK.P, po_out, live, k, s == 0, pcs, pcr);
            substep_quad<BAKED, (WPE > 1), DYN>(C, cm, sm, B, L, lag && (s == fs - 1), srow, k, zaxis_z, D, xon, xfrc_quad_ptr(XQ));
            if constexpr (PO_DEFER) po_row_copy_store<QG_PO_COPY_K, 4>(PK.P, po_out, live, k, s == 0, pcs, pcr);
        }
        if constexpr (PO_COPY) po_row_copy_rest<QG_PO_COPY_K, 4>(PK.P, po_ring, po_out, live, k, pcs);
        // the epilogue's addresses are derived from (env, leg) AFTER the loop: visible, they are computed before it and carried through
        // it (see the register-capped variants below; with two waves per SIMD that was 60 bytes of scratch in the walking variant)
        if constexpr (WPE > 1 || !BAKED) asm volatile("" : "+v"(env_e), "+v"(k_e));
        QG_MARK(2);                                  // physics done
        if (!lag) {   // un-lagged sensors (task.sensor_lag = 0): one extra forward pass on a scratch copy of the state
            BaseState B2 = B;
            LegState L2 = L;
            substep_quad<BAKED, (WPE > 1), DYN>(C, cm, sm, B2, L2, true, srow, k, zaxis_z, D, xon, xfrc_quad_ptr(XQ));
        }
        nstep = nstep0 + fs;
#pragma unroll
        for (int i = 0; i < 3; ++i) aclip[i] = aclip0[i];
    }
    float ssq = 0.f;
#pragma unroll
    for (int i = 0; i < 3; ++i) ssq = fmaf(aclip[i], aclip[i], ssq);
    ssq = quad_sum(ssq);

    QG_REWARD_TERMS(T->, B, ssq, nstep);
    QG_DONE_IF_BAD_STATE(B, quad_sum(L.q[0] + L.q[1] + L.q[2] + L.qd[0] + L.qd[1] + L.qd[2]));

    const int od = T->obs_mode == 1 ? 21 : 33;
    const int row = P.packed ? od + 2 : od;
    QG_DONE_IF_FLIPPED(T->, zaxis_z);
    if (k == 0) {                                                  // lane 0 of the quad wrote these entries itself
        if (od == 21) { srow[18] = srow[30]; srow[19] = srow[31]; srow[20] = srow[32]; }   // IMU pack: velocimeter follows the gyro
        if (P.packed) { srow[od] = reward; srow[od + 1] = done ? 1.f : 0.f; }
    }
    wave_sync();                                                   // the tile is this wave's own
    if constexpr (!PO) {
        const int total = live_envs * row;                               // (a whole wave may lie past the last env: live_envs = 0)
        float *dst = (P.packed ? P.packed : P.obs) + (size_t)env0 * row;
        QG_TILE_COPY_OUT(dst, tile, lane, total, row);
    }
    QG_MARK(3);                                      // obs tile written out
    const bool lead = live && k_e == 0;
    if (lead && !P.packed) {
        if constexpr (!WALK) P.reward[env_e] = reward;
        P.done[env_e] = done ? 1 : 0;
    }
    bool rst_done = false;
    if constexpr (POH) {
        // the auto-reset of the base FIRST (the reward below does not look at B): the helper wave's frame shows data.qpos[3:7] as the step
        // leaves it
        if (done && T->auto_reset) QG_BASE_RESET(B, nstep, C.qpos0, T->, P, env_e, P.st.episode[env_e]);
        rst_done = true;
        if (k_e == 0) {
            s_done[wave][lane >> 2] = done ? 1.f : 0.f;
            s_q[wave][lane >> 2][0] = B.qw; s_q[wave][lane >> 2][1] = B.qx; s_q[wave][lane >> 2][2] = B.qy; s_q[wave][lane >> 2][3] = B.qz;
        }
    }
    if constexpr (WALK) {
        WalkSums sum = {0.f, 0.f, 0.f, 0.f};
        if constexpr (WPE > 1) {       // two waves share the SIMD: read the task state again here (the other wave covers the latency)
#pragma unroll                        // instead of carrying 21 values through the substep loop
            for (int i = 0; i < 3; ++i) {
                const int t = env_e * 12 + 3 * k_e + i;
                if constexpr (!RWDH) wprev[i] = WK.S.prev_ctrl[t];
                if constexpr (!HELP) { wf[i] = WK.S.f_est[t]; wa[i] = WK.S.a_est[t]; }
                if constexpr (!RWDH) wtg[i] = walk_channel_targets(WK.P, 3 * k_e + i);
            }
            if ((!RWDH || PO) && lead) {
                win = walk_env_load(WK.S, n, env_e);
                win.episode_key = P.st.episode[env_e];
            }
        }
        if constexpr (HELP) {
            // the helper wave of this SIMD finished its first job long ago (its estimator stores have landed: the barrier's wait covers
            // them); from here on this wave may overwrite what the helper read at entry (data.ctrl, the episode counter), and (RWDH)
            // the helper evaluates the reward on the finished sensor tile
            if constexpr (RWDH) { if (k_e == 0) s_done[wave][lane >> 2] = done ? 1.f : 0.f; }
            __syncthreads();      // partner of the helper waves' one barrier
            if constexpr (!RWDH) {
#pragma unroll
                for (int i = 0; i < 3; ++i) { wf[i] = s_est[wave][lane][i]; wa[i] = s_est[wave][lane][3 + i]; }
            }
        }
        if (!RWDH && live) {
#pragma unroll
            for (int i = 0; i < 3; ++i) walk_channel_terms(WK.S, env_e, 3 * k_e + i, wtg[i], aclip[i], wprev[i], wf[i], wa[i], sum);
            walk_stv<3>(WK.S.prev_ctrl + (size_t)env_e * 12 + 3 * k_e, aclip);                       // previous_ctrl moves on (:260-262)
        }
        if constexpr (!RWDH) { sum.cost = quad_sum(sum.cost); sum.posture = quad_sum(sum.posture); sum.amp = quad_sum(sum.amp); sum.frq = quad_sum(sum.frq); }
        QG_MARK(4);                                  // channel terms + sums
        if (!RWDH && lead) walk_reward_env(WK.P, WK.S, n, env_e, tile + (lane >> 2) * 35, sum, win, done, P.reward, WK.comps, WK.sample, P.seed, P.env_index_base);
    }
    QG_COMPS_STORE(lead, P, env_e);

    const bool rst = done && T->auto_reset;
    if (rst && !rst_done) QG_BASE_RESET(B, nstep, C.qpos0, T->, P, env_e, P.st.episode[env_e]);
    if (lead) {
        QG_BASE_STORE(B, nstep, P.st, QG_PUT, n, env_e);
        if (rst) P.st.episode[env_e] += 1;
    }
    if (live) {
#pragma unroll
        for (int i = 0; i < 3; ++i) {
            const int j = 3 * k_e + i;
            QG_HINGE_STORE(rst ? C.qpos0[7 + (BAKED ? i : j)] : L.q[i], rst ? 0.f : L.qd[i], rst ? 0.f : L.act[i], P.st, QG_PUT, n, env_e, j);
            if (P.track_ctrl) P.st.ctrl[j * n + env_e] = rst ? T->default_ctrl[j] : aclip[i];
        }
    }
    if constexpr (PO && !POH)
        po_wave_epilogue<QGK_QUAD_ENVS, 4, WAVES, (WPE > 1)>(PK, WK, P, n, env, env0, live_envs, wave, lane, el, k, live, lead, pin, srow, B, win, done, aclip);
}

// ---- the sequence form (4 097 .. 16 384 envs at one wave per SIMD, 32 769 .. 57 343 at two; any model numbers) ---------------------------
// As qg_step_kernel_link_multi<.., DOOR = false> (qg_kernel_resident.hip) is to qg_step_kernel_link: qg_step_kernel_quad's plain path with an outer loop over env-steps; WPE / BAKED choose the same substep instantiation the per-launch
// launcher picks for the grid, so the bits are the per-launch kernel's.  Four-wave workgroups (every grid AUTO gives this mapping).
template <int WPE, bool BAKED>
__global__ __launch_bounds__(QGK_WAVE * 4, WPE) void qg_step_kernel_quad_multi(const KModel *__restrict__ Mp, const KTask *__restrict__ T, KStepArgs P, KResident R) {
    constexpr int WAVES = 4;
    __shared__ float tile_all[WAVES][QGK_QUAD_ENVS * 35];
    __shared__ KModel smodel;
    const int lane = threadIdx.x & (QGK_WAVE - 1);
    const int wave = threadIdx.x >> 6;
    float *tile = tile_all[wave];
    QG_STAGE_MODEL(C, BAKED, smodel, Mp, QGK_WAVE * WAVES);
    const int k = lane & 3;
    const int el = lane >> 2;
    const int env0 = (blockIdx.x * WAVES + wave) * QGK_QUAD_ENVS;
    const int n = P.n;
    const bool live = env0 + el < n;
    const int env = live ? env0 + el : n - 1;
    const float cm = (k == 0) ? 1.f : (k == 2) ? -1.f : 0.f;
    const float sm = (k == 1) ? 1.f : (k == 3) ? -1.f : 0.f;
    QG_TASK_REGS(Tk, T);

    BaseState B;
    QG_BASE_LOAD(B, P.st, QG_AT, n, env);
    int nstep = P.st.nstep[env];
    int episode = P.st.episode[env];
    LegState L;
#pragma unroll
    for (int i = 0; i < 3; ++i) {
        const int j = 3 * k + i;
        QG_HINGE_LOAD(L.q[i], L.qd[i], L.act[i], P.st, QG_AT, n, env, j);
        L.u[i] = 0.f; L.sc[2 * i] = 0.f; L.sc[2 * i + 1] = 1.f;
    }
    const int od = Tk.obs_mode == 1 ? 21 : 33;
    const int row = od + 2;
    const int fs = Tk.frame_skip;
    const int live_envs = max(0, min(QGK_QUAD_ENVS, n - env0));
    const int total = live_envs * row;
    float *srow = tile + el * 35;
    const size_t slot_act = (size_t)n * 12, slot_out = (size_t)n * row;
    float ctrl_reg[3] = {0.f, 0.f, 0.f}, a_next[3] = {0.f, 0.f, 0.f};
    bool have_next = false;

    for (int kstep = 0; kstep < R.count; ++kstep) {
        const float *ap = R.actions + (size_t)kstep * slot_act + (size_t)env * 12 + 3 * k;
        float aclip[3];
#pragma unroll
        for (int i = 0; i < 3; ++i) {
            const float a_in = have_next ? a_next[i] : ap[i];
            const float a = fminf(fmaxf(a_in, -1.f), 1.f);    // quadruped.py:160
            aclip[i] = a;
            L.u[i] = fminf(fmaxf(a, link_of<BAKED>(C, k, i).ctrl_lo), link_of<BAKED>(C, k, i).ctrl_hi);
        }
        have_next = WPE == 1 && kstep + 1 < R.count;     // (two waves per SIMD: no registers to park the next action in; the partner covers the load)
        if (have_next) {
#pragma unroll
            for (int i = 0; i < 3; ++i) a_next[i] = ap[slot_act + i];
        }
        quat_unit(B);
#pragma unroll
        for (int i = 0; i < 3; ++i) sincos_f(L.q[i] - link_of<BAKED>(C, k, i).ref, L.sc[2 * i], L.sc[2 * i + 1]);
        float zaxis_z = 1.f;
        asm volatile(".p2align 6");
#pragma unroll 1
        for (int s = 0; s < fs; ++s) substep_quad<BAKED, (WPE > 1)>(C, cm, sm, B, L, s == fs - 1, srow, k, zaxis_z);
        nstep += fs;

        float ssq = 0.f;
#pragma unroll
        for (int i = 0; i < 3; ++i) ssq = fmaf(aclip[i], aclip[i], ssq);
        ssq = quad_sum(ssq);
        QG_REWARD_TERMS(Tk., B, ssq, nstep);
        QG_DONE_IF_BAD_STATE(B, quad_sum(L.q[0] + L.q[1] + L.q[2] + L.qd[0] + L.qd[1] + L.qd[2]));
        QG_DONE_IF_FLIPPED(Tk., zaxis_z);
        if (k == 0) {
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
        if constexpr (WPE == 1) {
#pragma unroll
            for (int i = 0; i < 3; ++i) ctrl_reg[i] = aclip[i];
        } else if (live && P.track_ctrl) {      // two waves per SIMD: data.ctrl goes out every env-step (as the per-launch kernel writes it) rather
#pragma unroll                                  // than riding through the substep loop in three more registers
            for (int i = 0; i < 3; ++i) P.st.ctrl[(3 * k + i) * n + env] = rst ? Tk.default_ctrl[3 * k + i] : aclip[i];
        }
        if (rst) {
            QG_BASE_RESET(B, nstep, C.qpos0, Tk., P, env, episode);
            episode += 1;
#pragma unroll
            for (int i = 0; i < 3; ++i) {
                L.q[i] = C.qpos0[7 + (BAKED ? i : 3 * k + i)]; L.qd[i] = 0.f; L.act[i] = 0.f;
                if constexpr (WPE == 1) ctrl_reg[i] = Tk.default_ctrl[3 * k + i];
            }
        }
    }

    // the addresses of the final stores are derived from (env, leg) AFTER the loops: visible to the optimiser they are computed ahead of
    // them and carried through the substep loop (qg_step_kernel_quad does the same for its epilogue)
    int env_e = env, k_e = k;
    asm volatile("" : "+v"(env_e), "+v"(k_e));
    if (live && k_e == 0) {
        QG_BASE_STORE(B, nstep, P.st, QG_PUT, n, env_e);
        P.st.episode[env_e] = episode;
    }
    if (live && R.count > 0) {
#pragma unroll
        for (int i = 0; i < 3; ++i) {
            const int j = 3 * k_e + i;
            QG_HINGE_STORE(L.q[i], L.qd[i], L.act[i], P.st, QG_PUT, n, env_e, j);
            if (WPE == 1 && P.track_ctrl) P.st.ctrl[j * n + env_e] = ctrl_reg[i];
        }
    }
}

// ---- host side: the launchers, and every leaf of the mapping --------------------------------------------------------------------
template <bool BAKED> static void launch_lane(const StepLaunch &L) {
    L.s->last_step_kernel = step_kernel_code<BAKED>(KF_LANE);
    hipLaunchKernelGGL(qg_step_kernel<BAKED>, dim3((L.s->n + QGK_WAVE - 1) / QGK_WAVE), dim3(QGK_WAVE), 0, L.stream, L.model, L.s->d_task, L.P);
}
template <int WPE, bool BAKED, bool WALK, int WAVES, bool PO = false, bool HELP = false, bool DYN = false> static void launch_quad(const StepLaunch &L) {
    static_assert(WAVES == 1 || WAVES == 4, "one-wave or four-wave workgroups");
    L.s->last_step_kernel = step_kernel_code<WPE, BAKED, WALK, WAVES, PO, HELP, DYN>(KF_QUAD);
    hipLaunchKernelGGL((qg_step_kernel_quad<WPE, BAKED, WALK, WAVES, PO, HELP, DYN>), wave_grid(quad_blocks(L.s), WAVES),
                       dim3(QGK_WAVE * WAVES * (HELP ? 2 : 1)), 0, L.stream, L.model, L.s->d_task, L.P, walk_arg<WALK>(L.walk), po_arg<PO>(L.po));
}
template <int WPE, bool BAKED> static void launch_quad_multi(const qg_sim *s, hipStream_t st, const KStepArgs &P, const KResident &R) {
    s->last_step_kernel = step_kernel_code<WPE, BAKED>(KF_QUAD_MULTI);
    hipLaunchKernelGGL((qg_step_kernel_quad_multi<WPE, BAKED>), wave_grid(quad_blocks(s), 4), dim3(QGK_WAVE * 4), 0, st, s->d_model, s->d_task, P, R);
}

// Every leaf names the instantiation it launches.  DYN: per-env dynamics, which run the table-driven (!baked) leaves only.
template <bool DYN> static void select_step_quad(const StepLaunch &L) {
    const qg_sim *s = L.s;
    const bool walk = L.walk, po = L.po;
    if (!qg_sim_baked(s)) {
        // tables in LDS: the 256-register cap spills 888 B per lane and measured 2x slower at every grid size (363 vs 741 us
        // at 262 144 envs), so any other robot runs the one-wave-per-SIMD form throughout
        if (po) launch_quad<1, false, true, 4, true, false, DYN>(L);     // qg_po_fusable(): four-wave workgroups
        else if (walk && quad_wg4(s)) launch_quad<1, false, true, 4, false, false, DYN>(L);
        else if (walk) launch_quad<1, false, true, 1, false, false, DYN>(L);
        else if (quad_wg4(s)) launch_quad<1, false, false, 4, false, false, DYN>(L);
        else launch_quad<1, false, false, 1, false, false, DYN>(L);
    } else if (po) {            // qg_po_fusable(): four-wave workgroups, register cap for one or two waves per SIMD
        if (quad_one_wave(s) && s->link_helpers) launch_quad<2, true, true, 4, true, true>(L);
        else if (quad_one_wave(s)) launch_quad<1, true, true, 4, true>(L);
        else launch_quad<2, true, true, 4, true>(L);
    } else if (walk) {
        // at most one physics wave per SIMD: helper waves beside them (QG_LINK_HELPERS, as for the one-link-per-lane kernel)
        if (quad_one_wave(s) && s->link_helpers) launch_quad<2, true, true, 4, false, true>(L);
        else if (quad_one_wave(s) && quad_wg4(s)) launch_quad<1, true, true, 4>(L);
        else if (quad_one_wave(s)) launch_quad<1, true, true, 1>(L);
        else launch_quad<2, true, true, 4>(L);
    } else if (quad_one_wave(s)) {
        if (quad_wg4(s)) launch_quad<1, true, false, 4>(L);
        else launch_quad<1, true, false, 1>(L);
    } else launch_quad<2, true, false, 4>(L);       // (more than one wave per SIMD is more than one per compute unit: quad_wg4)
}
void qg_select_step_quad(const StepLaunch &L, bool dyn) {
    QG_PHASE_UNIT();
    if (dyn) select_step_quad<true>(L);
    else select_step_quad<false>(L);
}
void qg_select_step_lane(const StepLaunch &L) {
    QG_PHASE_UNIT();
    if (qg_sim_baked(L.s)) launch_lane<true>(L);
    else launch_lane<false>(L);
}

// as select_step_quad: the whole register file while the grid is one wave per SIMD
void qg_select_seq_quad(const qg_sim *s, hipStream_t st, const KStepArgs &P, const KResident &R) {
    QG_PHASE_UNIT();
    if (!qg_sim_baked(s)) launch_quad_multi<1, false>(s, st, P, R);       // (tables in LDS: always the one-wave form)
    else if (quad_one_wave(s)) launch_quad_multi<1, true>(s, st, P, R);
    else launch_quad_multi<2, true>(s, st, P, R);
}
