// qg_step_shell.h -- the shell of an env-step around the physics substeps, ONCE for every step kernel: base-state load and store,
// plain reward and terminations, auto-reset of the base with the random heading, copy-out of the output tile, staging of the model
// tables, the register snapshot of the task.  The per-launch kernels and the many-steps-per-launch
// forms (qg_kernel_link.hip with qg_kernel_resident.hip, qg_kernel_quad.hip, qg_kernel_pair.hip) expand the same text, so a change to the shell is made here and reaches all of them.
//
// Statement MACROS, not device functions, on purpose: the macros expand to the very tokens the kernels held before and leave all 65
// kernels of the code object instruction for instruction what they were (tools/asm_diff.py, profiles/r09/asm_diff.txt), while the same
// fragments as __forceinline__ functions renumbered registers and commuted operands in 37 of them, 24 substep loops included -- and
// this project has measured 0.2 us from a one-dword shift of such a loop ("Shared kernel text").  Same idiom as
// qg_contact_eval.inc and qg_link_regs.inc.  After an edit here: `make asm` before and after, then tools/asm_diff.py.
//
// Arguments are names or expressions of the call site and are pasted, not evaluated: B the BaseState, ST the KState (P.st), TK the
// task as a prefix (`T->`, or `Tk.` for the register snapshot of QG_TASK_REGS), QPOS0 the table's qpos0 (C.qpos0, M->qpos0).  A
// parameter that is spelled like a member the text names would be replaced there too (ST.act, ST.nstep): those are in capitals.
#pragma once

// element `row` of env e in a [rows][n] state array, as an access pair (AT = read, PUT = write) handed to QG_BASE_LOAD / QG_BASE_STORE:
// plain indexing with (n, env), or the one-link-per-lane kernels' 32-bit byte offsets with (n4, e4) = (4 n, 4 env) (lk_ld / lk_st)
#define QG_AT(a, row, n, e) (a)[(row) * (n) + (e)]
#define QG_PUT(a, row, n, e, v) (a)[(row) * (n) + (e)] = (v)
#define QG_AT_LK(a, row, n4, e4) lk_ld(a, (row) * (n4) + (e4))
#define QG_PUT_LK(a, row, n4, e4, v) lk_st(a, (row) * (n4) + (e4), v)

// free joint of the base: position, quaternion, linear velocity (world), angular velocity (body)
#define QG_BASE_LOAD(B, ST, AT, n, e)                                                                                       \
    {                                                                                                                       \
        B.pw = v3(AT(ST.qpos, 0, n, e), AT(ST.qpos, 1, n, e), AT(ST.qpos, 2, n, e));                                        \
        B.qw = AT(ST.qpos, 3, n, e); B.qx = AT(ST.qpos, 4, n, e); B.qy = AT(ST.qpos, 5, n, e); B.qz = AT(ST.qpos, 6, n, e); \
        B.vw = v3(AT(ST.qvel, 0, n, e), AT(ST.qvel, 1, n, e), AT(ST.qvel, 2, n, e));                                        \
        B.wb = v3(AT(ST.qvel, 3, n, e), AT(ST.qvel, 4, n, e), AT(ST.qvel, 5, n, e));                                        \
    }
// ... and back, with the substep counter (the episode counter stays with the kernels: the per-launch forms advance it in memory, the
// many-steps forms carry it in a register)
#define QG_BASE_STORE(B, NSTEP, ST, PUT, n, e)                                                                    \
    {                                                                                                             \
        PUT(ST.qpos, 0, n, e, B.pw.x); PUT(ST.qpos, 1, n, e, B.pw.y); PUT(ST.qpos, 2, n, e, B.pw.z);              \
        PUT(ST.qpos, 3, n, e, B.qw); PUT(ST.qpos, 4, n, e, B.qx); PUT(ST.qpos, 5, n, e, B.qy); PUT(ST.qpos, 6, n, e, B.qz); \
        PUT(ST.qvel, 0, n, e, B.vw.x); PUT(ST.qvel, 1, n, e, B.vw.y); PUT(ST.qvel, 2, n, e, B.vw.z);              \
        PUT(ST.qvel, 3, n, e, B.wb.x); PUT(ST.qvel, 4, n, e, B.wb.y); PUT(ST.qvel, 5, n, e, B.wb.z);              \
        PUT(ST.nstep, 0, n, e, NSTEP);                                                                            \
    }

// hinge j (0 .. 11) of the env: position, velocity and servo activation into / from three lvalues / values of the call site
#define QG_HINGE_LOAD(Q, QD, ACT, ST, AT, n, e, j) \
    { Q = AT(ST.qpos, 7 + j, n, e); QD = AT(ST.qvel, 6 + j, n, e); ACT = AT(ST.act, j, n, e); }
#define QG_HINGE_STORE(Q, QD, ACT, ST, PUT, n, e, j) \
    { PUT(ST.qpos, 7 + j, n, e, Q); PUT(ST.qvel, 6 + j, n, e, QD); PUT(ST.act, j, n, e, ACT); }

// random heading (walking_quad.py:68-75): a yaw drawn for (seed, env, episode) into the quaternion (qw .. qz: lvalues)
#define QG_RESET_HEADING(seed, env_index, episode, qw, qx, qy, qz)                                  \
    {                                                                                               \
        float a = 6.283185307179586f * uniform24(seed, env_index, (uint64_t)episode);               \
        float sn, cs;                                                                               \
        sincos_f(0.5f * a, sn, cs);                                                                 \
        qw = cs; qx = 0.f; qy = 0.f; qz = sn;                                                       \
    }
// auto-reset of the base (VecEnv semantics): qpos0, the heading if the task asks for it, zero velocities, time 0.  EPISODE is pasted
// inside the `reset_flags & 1u` branch: where it is a load (P.st.episode[env]) it is issued only there.
#define QG_BASE_RESET(B, nstep, QPOS0, TK, P, env, EPISODE)                                                                  \
    {                                                                                                                        \
        B.pw = v3(QPOS0[0], QPOS0[1], QPOS0[2]);                                                                             \
        B.qw = QPOS0[3]; B.qx = QPOS0[4]; B.qy = QPOS0[5]; B.qz = QPOS0[6];                                                  \
        if (TK reset_flags & 1u) QG_RESET_HEADING(P.seed, P.env_index_base + (uint64_t)env, EPISODE, B.qw, B.qx, B.qy, B.qz); \
        B.vw = v3(0.f, 0.f, 0.f);                                                                                            \
        B.wb = v3(0.f, 0.f, 0.f);                                                                                            \
        nstep = 0;                                                                                                           \
    }

// rewards and terminations on the post-step state (README.md:64-90), in three pieces because the kernels place other work between them.
// QG_REWARD_TERMS DECLARES c_fwd, c_ctl, c_alive, reward and done (time limit, fall) in the scope of the call site.
#define QG_REWARD_TERMS(TK, B, ssq, nstep)                      \
    float c_fwd = TK w_forward * B.vw.x;                        \
    float c_ctl = TK w_ctrl * ssq;                              \
    float c_alive = TK alive_bonus;                             \
    float reward = reward_total(c_fwd, c_ctl, c_alive);         \
    bool done = nstep >= TK limit_substeps;                     \
    if (TK use_fall) done = done || (B.pw.z < TK fall_height)
// a state that left the numbers: `hinges` is the sum of the env's hinge positions and velocities, reduced as the work mapping has it
// (quad_sum / pair_sum / env_sum).  The probe is formed in front of the `||`, not inside it: the reductions exchange values between
// lanes and have to run in all of them, also those whose env is done already.  The one-env-per-lane kernel adds base first, hinges
// second -- another rounding -- and keeps its own probe.
#define QG_DONE_IF_BAD_STATE(B, hinges)                                                                                                 \
    {                                                                                                                                   \
        const float probe = hinges + B.pw.x + B.pw.y + B.pw.z + B.qw + B.vw.x + B.vw.y + B.vw.z + B.wb.x + B.wb.y + B.wb.z;             \
        done = done || state_is_bad(probe);                                                                                             \
    }
// walking_quad.py:156-160, on the step's sensordata
#define QG_DONE_IF_FLIPPED(TK, zaxis_z) \
    if (TK use_flip) done = done || (zaxis_z < 0.f)
// the three reward components of QG_REWARD_TERMS, for the callers that ask for them
#define QG_COMPS_STORE(cond, P, env)                \
    if (cond && P.comps) {                          \
        P.comps[(size_t)env * 3 + 0] = c_fwd;       \
        P.comps[(size_t)env * 3 + 1] = c_ctl;       \
        P.comps[(size_t)env * 3 + 2] = c_alive;     \
    }

// the wave's block of the output tile (rows staged with a stride of 35 floats) to `total` = live envs x row contiguous floats at dst.
// One table of multipliers for the per-launch kernels (row 21, 23, 33) and the many-steps forms (packed rows only: 23), where the
// compiler drops the entries `row` cannot take.  The one-link-per-lane kernels copy a tile row per pass instead and keep their own.
#define QG_TILE_COPY_OUT(dst, tile, lane, total, row)                                                                                \
    {                                                                                                                                \
        if (row == 35) {                       /* the packed full layout is a straight copy */                                       \
            for (int e = lane; e < total; e += QGK_WAVE) dst[e] = tile[e];                                                           \
        } else {                                                                                                                     \
            /* e / row without a division per element: row is 21, 23 or 33 here and e < 2^11, where (e * ceil(2^16 / row)) >> 16 is exact */ \
            const unsigned magic = row == 33 ? 1986u : row == 21 ? 3121u : row == 23 ? 2850u : (65536u + row - 1) / row;             \
            for (int e = lane; e < total; e += QGK_WAVE) {                                                                           \
                const int er = (int)(((unsigned)e * magic) >> 16), ec = e - er * row;                                                \
                dst[e] = tile[er * 35 + ec];                                                                                         \
            }                                                                                                                        \
        }                                                                                                                            \
    }

// generic variants (!BAKED): the link / joint tables staged in LDS (3.2 KB) by the workgroup's `nthreads` threads, behind one barrier
// that every wave reaches exactly once; DECLARES the table `C` the kernel reads from then on
#define QG_STAGE_MODEL(C, BAKED, smodel, Mp, nthreads)                                                               \
    if constexpr (!BAKED) {                                                                                          \
        const float *src = reinterpret_cast<const float *>(Mp);                                                      \
        float *dst = reinterpret_cast<float *>(&smodel);                                                             \
        for (int i = threadIdx.x; i < (int)(sizeof(KModel) / sizeof(float)); i += nthreads) dst[i] = src[i];         \
        __syncthreads();                                                                                             \
    }                                                                                                                \
    const KModel &C = BAKED ? QG_BAKED_MODEL : smodel

// the task constants into scalar registers up front: read where they are used, every read in the epilogue was its own scalar-load
// round trip in front of a wave that has nothing else to do.  DECLARES Tk.
#define QG_TASK_REGS(Tk, T)                                                                                                                          \
    struct { int32_t frame_skip, limit_substeps, use_fall, use_flip, obs_mode, auto_reset; uint32_t reset_flags; float fall_height, w_forward, w_ctrl, alive_bonus; \
             const float *default_ctrl; } Tk = {T->frame_skip, T->limit_substeps, T->use_fall, T->use_flip, T->obs_mode, T->auto_reset, T->reset_flags,             \
                                                T->fall_height, T->w_forward, T->w_ctrl, T->alive_bonus, T->default_ctrl}
