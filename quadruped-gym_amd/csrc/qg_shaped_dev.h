// qg_shaped_dev.h -- what the shaped-reward layers share (qg_gait.hip: the gait terms; qg_sched.hip: the gait schedule's): the strides of
// a launch's reward, component and command rows, the tail of a kernel that weighs the env's terms, adds them onto the reward and writes
// the component columns, and the host side's checks of those arguments.  Internal.
#pragma once
#include <stdint.h>

#include "qg_host.h"

// the call's rows: reward [n] and reward_out [n] at an element stride; components [n][base_terms + NT], base [n][base_terms] and
// command [n][2] at a row stride.  copy_base: the base columns are not already the front of the components' rows
struct KShapedIO {
    int32_t reward_stride, out_stride, comp_stride, base_stride, base_terms, copy_base, command_stride;
};

// ---- the tail of a kernel ----------------------------------------------------------------------------------------------------------------
// Statement macros, not device functions: DESIGN.md, "Shared kernel text" -- the function forms tried on these kernels moved the kernel
// arguments' base register and changed all four listings (docs/EXPERIMENTS.md).  After an edit here: `make asm` before and after, then
// tools/asm_diff.py.  The text is pasted, not evaluated; besides its arguments it reads the names both kernels have: lane, e, finished,
// and the parameters reward, reward_out, base, comps.  MUL / ADD spell the one f32 multiply and add of the layer: intrinsics in
// qg_gait.hip, operators under `fp contract(off)` in qg_sched.hip.

// max(|vx|, |vy|) of a command row: what a layer compares with its min_command_speed
#define QG_SHAPED_SPEED(c) fmaxf(fabsf((c)[0]), fabsf((c)[1]))

// Declares comp[NT], the weighted terms -- zeros for a finished env --, and shaped, their sum in ascending order.
#define QG_SHAPED_WEIGH(NT, W, TERM, MUL, ADD)                                                                                             \
    float comp[NT], shaped = 0.f;                                                                                                          \
    _Pragma("unroll") for (int k = 0; k < NT; ++k) {                                                                                       \
        comp[k] = finished ? 0.f : MUL(W[k], TERM[k]); /* rounded to f32 before the sum: the sum is over the stored columns */             \
        shaped = k ? ADD(shaped, comp[k]) : comp[0];                                                                                       \
    }

// The outputs: the 16 lanes copy the base columns, lanes 0 .. NT - 1 store one component each, lane NT the reward.
#define QG_SHAPED_STORE(NT, IO, ADD)                                                                                                       \
    if (comps) {                                                                                                                           \
        float *row = comps + e * (size_t)(IO).comp_stride;                                                                                 \
        if ((IO).copy_base) {                                                                                                              \
            const float *from = base + e * (size_t)(IO).base_stride;                                                                       \
            for (int c = lane; c < (IO).base_terms; c += 16) row[c] = from[c];                                                             \
        }                                                                                                                                  \
        if (lane < NT) {                                                                                                                   \
            float mine = comp[0];                                                                                                          \
            _Pragma("unroll") for (int k = 1; k < NT; ++k) mine = lane == k ? comp[k] : mine;                                              \
            row[(IO).base_terms + lane] = mine;                                                                                            \
        }                                                                                                                                  \
    }                                                                                                                                      \
    if (reward_out && lane == NT) {                                                                                                        \
        float r = shaped;                                                                                                                  \
        if (reward) {                                                                                                                      \
            const float r0 = reward[e * (size_t)(IO).reward_stride];                                                                       \
            r = finished ? r0 : ADD(r0, shaped); /* a finished env's reward passes through bit for bit */                                  \
        }                                                                                                                                  \
        reward_out[e * (size_t)(IO).out_stride] = r;                                                                                       \
    }

// ---- host side -------------------------------------------------------------------------------------------------------------------------
static inline int qg_check_weights(const float *w, int count, const char *who) {
    for (int k = 0; k < count; ++k)
        if (!qg_finite32(w[k])) return fail(QG_ERR_ARG, "%s: weights[%d] is not finite", who, k);
    return QG_OK;
}

// The reward, component, base and command arguments of the entry point `who` of a layer of `nt` terms over `n` envs: refused, or `io`
// filled.  The widest base is what still fits a monitor beside the layer's own columns.
static inline int qg_shaped_io(const char *who, int nt, const float *reward, int32_t reward_stride, const float *reward_out, int32_t reward_out_stride,
                               const float *components, int32_t components_stride, const float *base_components, int32_t base_stride,
                               int32_t base_terms, const float *command, int32_t command_stride, int64_t n, KShapedIO *io) {
    const int max_base = QG_MONITOR_MAX_TERMS - nt;
    if (reward && !reward_out) return fail(QG_ERR_ARG, "%s: reward without reward_out", who);
    if (reward && reward_stride < 1) return fail(QG_ERR_ARG, "%s: reward_stride %d must be >= 1", who, reward_stride);
    if (reward_out && reward_out_stride < 1) return fail(QG_ERR_ARG, "%s: reward_out_stride %d must be >= 1", who, reward_out_stride);
    if (base_terms < 0 || base_terms > max_base) return fail(QG_ERR_ARG, "%s: base_terms %d must be 0 .. %d", who, base_terms, max_base);
    if (!base_components && base_terms != 0) return fail(QG_ERR_ARG, "%s: base_terms %d without base_components", who, base_terms);
    if (base_components && !components) return fail(QG_ERR_ARG, "%s: base_components without components", who);
    if (components && components_stride < base_terms + nt)
        return fail(QG_ERR_ARG, "%s: components_stride %d must be >= base_terms + %d = %d", who, components_stride, nt, base_terms + nt);
    if (base_components && base_stride < base_terms) return fail(QG_ERR_ARG, "%s: base_stride %d must be >= base_terms %d", who, base_stride, base_terms);
    if (command && command_stride < 2) return fail(QG_ERR_ARG, "%s: command_stride %d must be >= 2", who, command_stride);
    // the base columns already at the front of the wide buffer: nothing to copy.  Any other overlap of the two would let a lane read what
    // another one writes
    const bool in_place = base_components && base_components == components && base_stride == components_stride;
    const bool copy_base = base_components && base_terms > 0 && !in_place;
    if (copy_base && qg_rows_overlap(base_components, base_stride, base_terms, components, components_stride, base_terms + nt, n))
        return fail(QG_ERR_ARG, "%s: base_components and components overlap (allowed only as the first base_terms columns of the same rows)", who);
    *io = {reward_stride, reward_out_stride, components_stride, base_stride, base_terms, copy_base ? 1 : 0, command_stride};
    return QG_OK;
}
