// qg_cmdcur.hip -- the command curriculum (include/quadgym.h: qg_cmdcur_*): a grid of (speed, velocity angle) bins with
// integer weights that grow outward from an easy region as the segments drawn from a bin succeed.  Bound to a qg_walk, whose command
// slots (KWalkState::vel / head / gvel) it writes behind the env-step; no step kernel knows of it.
//
// qg_cmdcur_advance_device is TWO launches on the caller's stream, 256 envs per block, one env per lane, bin t of the grid on thread t:
//   qg_cmdcur_judge_kernel  steps += 1, the criteria's sums take the step's component columns, a segment that ends (done, or the R-th
//                           step) is judged.  A wave whose ballot of "ended" is empty does nothing more; the others count ended and
//                           succeeded segments per bin with integer adds in LDS.  A block that saw an end stores its two rows of counts
//                           and raises its word of block_any[]; a block that saw none stores a zero there and no counts.  Lane 0 of
//                           block 0 bumps gen: the weights this advance reads are in half (gen + 1) & 1 from here on, the ones it
//                           forms go to half gen & 1.
//   qg_cmdcur_draw_kernel   a block without an ended env (and not block 0) skips to command_out.  The others sum the counts of the
//                           flagged blocks in ascending block order -- every such block forms the same integers --, form the new weights
//                           from the old half and their inclusive prefix sums in LDS, and their ended envs search it for the new bin
//                           and draw the command.  Block 0 alone stores the new half and adds the counts onto episodes / successes.
// No block reads what another block of the same launch writes, so none waits for another; the sums that cross blocks are integers (no
// floating-point atomics: there is no floating-point sum across envs at all); nothing is allocated; both launches are plain kernels of
// the stream, so a capture holds them and a replay advances the curriculum.
// qg_cmdcur_begin_device is one launch (the prefix sums of the weights as they stand, the draw); qg_cmdcur_create runs it once, without
// the segment increment, for segment 0.

#include <hip/hip_runtime.h>
#include <stdint.h>

#include <cmath>
#include <cstring>

#include "qg_sim.h"          // qg_walk: the layer whose command slots are written; through it qg_walk_dev.h: walk_write_command
#include "qg_key_dev.h"

#define QGU_SALT 0x5147434D44435531ull        // "QGCMDCU1"
#define QGU_BLOCK 256                         // envs per block = the most bins of a grid: thread t owns bin t
#define QGU_BLOB 0x52554351u                  /* "QCUR" */

struct QgcShared {                            // the handle's own words, one allocation
    int64_t episodes[QG_CMDCUR_MAX_BINS], successes[QG_CMDCUR_MAX_BINS];
    int32_t weight[2][QG_CMDCUR_MAX_BINS];    // ping-pong: the current half is gen & 1
    uint32_t gen, pad;
};

struct KCmdCur {
    int32_t n, n_speed, n_alpha, B, fixed_heading, W, delta, R, min_steps, n_criteria;
    int32_t column[QG_CMDCUR_MAX_CRITERIA], sense[QG_CMDCUR_MAX_CRITERIA];
    float threshold[QG_CMDCUR_MAX_CRITERIA];
    float speed_lo, ws, wa, heading_angle;
    uint64_t seed_c, base;
    int32_t nblocks, done_kind, done_stride, comp_stride, out_stride;
};

struct KCmdCurState {
    int32_t *bin, *steps;        // [n]
    float *sum;                  // [QG_CMDCUR_MAX_CRITERIA][n]
    int64_t *segment;            // [n]
    uint8_t *ended;              // [n]        judge -> draw
    QgcShared *sh;
    int32_t *block_any;          // [nblocks]  judge -> draw
    int32_t *partial;            // [nblocks][2][QG_CMDCUR_MAX_BINS]: ended, succeeded segments per bin; rows of flagged blocks only
};

// x >= y (ge) or x <= y on the bits: the device pass is compiled with -ffinite-math-only, under which a float comparison may be turned
// into its complement, and a NaN sum has to FAIL its criterion.  Any NaN fails; -0 equals +0.
__device__ __forceinline__ uint32_t qgu_order(uint32_t b) {
    if ((b << 1) == 0u) b = 0u;
    return (b & 0x80000000u) ? ~b : (b | 0x80000000u);        // monotonic in the float's value
}
__device__ __forceinline__ bool qgu_holds(float sum, float bound, int32_t sense) {
    const uint32_t a = __float_as_uint(sum), b = __float_as_uint(bound);
    if ((a & 0x7fffffffu) > 0x7f800000u || (b & 0x7fffffffu) > 0x7f800000u) return false;
    return sense > 0 ? qgu_order(a) >= qgu_order(b) : qgu_order(a) <= qgu_order(b);
}

// the new segment `seg` of env e: its bin from the prefix sums in LDS, its command into the walking layer's slots
__device__ __forceinline__ void qgu_draw(const KCmdCur &A, const KWalkState &S, const KCmdCurState &C, const int32_t *cdf, size_t e, uint64_t seg) {
#pragma clang fp contract(off)
    const uint64_t key = qgp_key(A.seed_c, A.base + e, seg);
    const uint64_t T = (uint64_t)cdf[A.B - 1];
    const int32_t r = (int32_t)(((uint64_t)qgp_k(key, 0) * T) >> 24);     // < T <= 2^24
    int lo = 0, hi = A.B - 1;                                             // the smallest b with cdf[b] > r: cdf[B - 1] = T > r
    while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (cdf[mid] > r) hi = mid;
        else lo = mid + 1;
    }
    const int32_t si = lo / A.n_alpha, ai = lo - si * A.n_alpha;
    const float pi = 3.14159265358979323846f;
    const float u_s = (float)qgp_k(key, 1) * 0x1p-24f, u_a = (float)qgp_k(key, 2) * 0x1p-24f, u_t = (float)qgp_k(key, 3) * 0x1p-24f;   // exact
    const float edge_s = A.speed_lo + (float)si * A.ws, edge_a = -pi + (float)ai * A.wa;
    const float speed = edge_s + A.ws * u_s, alpha = edge_a + A.wa * u_a;
    const float theta = A.fixed_heading ? A.heading_angle : pi * (2.f * u_t - 1.f);
    C.bin[e] = lo, C.steps[e] = 0, C.segment[e] = (int64_t)seg;
    for (int k = 0; k < QG_CMDCUR_MAX_CRITERIA; ++k) C.sum[(size_t)k * A.n + e] = 0.f;
    walk_write_command(S, A.n, (int)e, theta, alpha, speed);
}

// inclusive prefix sums of cdf[0 .. 255] in place; every thread of the block is here
__device__ __forceinline__ void qgu_scan(int32_t *cdf, int t) {
    for (int off = 1; off < QGU_BLOCK; off <<= 1) {
        __syncthreads();
        const int32_t v = t >= off ? cdf[t - off] : 0;
        __syncthreads();
        cdf[t] += v;
    }
    __syncthreads();
}

// launch 1 of an advance
__global__ __launch_bounds__(QGU_BLOCK) void qg_cmdcur_judge_kernel(KCmdCur A, KCmdCurState C, const void *done, const float *__restrict__ comps) {
#pragma clang fp contract(off)
    __shared__ int32_t cnt[2][QG_CMDCUR_MAX_BINS];
    __shared__ int32_t any;
    const int t = threadIdx.x;
    const int64_t e64 = (int64_t)blockIdx.x * QGU_BLOCK + t;
    const bool live = e64 < A.n;
    const size_t e = (size_t)e64, n = (size_t)A.n;
    if (blockIdx.x == 0 && t == 0) C.sh->gen += 1u;
    cnt[0][t] = 0, cnt[1][t] = 0;
    if (t == 0) any = 0;
    __syncthreads();
    bool end = false, success = false;
    int32_t b = 0;
    if (live) {
        const int32_t st = C.steps[e] + 1;
        float s[QG_CMDCUR_MAX_CRITERIA];
#pragma unroll
        for (int k = 0; k < QG_CMDCUR_MAX_CRITERIA; ++k)
            s[k] = k < A.n_criteria ? C.sum[(size_t)k * n + e] + comps[e * (size_t)A.comp_stride + A.column[k]] : 0.f;
        end = (done && qg_done_at(done, A.done_kind, A.done_stride, e)) || st == A.R;      // (R = 0: never, st >= 1)
        if (end) {
            success = st >= A.min_steps;
#pragma unroll
            for (int k = 0; k < QG_CMDCUR_MAX_CRITERIA; ++k)
                if (k < A.n_criteria) success = success && qgu_holds(s[k], A.threshold[k] * (float)st, A.sense[k]);
            b = C.bin[e];
        } else {                                          // (an ended env's words are the draw's to write)
            C.steps[e] = st;
#pragma unroll
            for (int k = 0; k < QG_CMDCUR_MAX_CRITERIA; ++k)
                if (k < A.n_criteria) C.sum[(size_t)k * n + e] = s[k];
        }
        C.ended[e] = end ? 1 : 0;
    }
    if (__ballot(end) != 0ull) {                          // wave-uniform; most steps no env of the wave ends
        if (end) {
            atomicAdd(&cnt[0][b], 1);
            if (success) atomicAdd(&cnt[1][b], 1);
        }
        if ((t & 63) == 0) any = 1;
    }
    __syncthreads();
    const int32_t flagged = any;
    if (flagged && t < A.B) {
        int32_t *row = C.partial + (size_t)blockIdx.x * 2 * QG_CMDCUR_MAX_BINS;
        row[t] = cnt[0][t], row[QG_CMDCUR_MAX_BINS + t] = cnt[1][t];
    }
    if (t == 0) C.block_any[blockIdx.x] = flagged;
}

// launch 2 of an advance
__global__ __launch_bounds__(QGU_BLOCK) void qg_cmdcur_draw_kernel(KCmdCur A, KWalkState S, KCmdCurState C, float *command_out) {
    __shared__ int32_t succ[QG_CMDCUR_MAX_BINS], cdf[QG_CMDCUR_MAX_BINS];
    const int t = threadIdx.x;
    const int64_t e64 = (int64_t)blockIdx.x * QGU_BLOCK + t;
    const bool live = e64 < A.n;
    const size_t e = (size_t)e64;
    const bool end = live && C.ended[e] != 0;
    const bool first = blockIdx.x == 0;
    if (first || C.block_any[blockIdx.x] != 0) {          // block-uniform
        const uint32_t gen = C.sh->gen;
        const int32_t *old = C.sh->weight[(gen + 1u) & 1u];
        int32_t ep = 0, su = 0;
        if (t < A.B)
            for (int blk = 0; blk < A.nblocks; ++blk)     // ascending block order
                if (C.block_any[blk] != 0) {
                    const int32_t *row = C.partial + (size_t)blk * 2 * QG_CMDCUR_MAX_BINS;
                    ep += row[t], su += row[QG_CMDCUR_MAX_BINS + t];
                }
        succ[t] = su;
        __syncthreads();
        int32_t w = 0;
        if (t < A.B) {                                    // N(t): the bin, its speed neighbours (no wrap), its angle neighbours (wrap), as a set
            const int32_t si = t / A.n_alpha, ai = t - si * A.n_alpha;
            int64_t s = succ[t];
            if (si > 0) s += succ[t - A.n_alpha];
            if (si < A.n_speed - 1) s += succ[t + A.n_alpha];
            if (A.n_alpha >= 2) s += succ[si * A.n_alpha + (ai + 1 == A.n_alpha ? 0 : ai + 1)];
            if (A.n_alpha >= 3) s += succ[si * A.n_alpha + (ai == 0 ? A.n_alpha - 1 : ai - 1)];
            const int64_t v = (int64_t)old[t] + (int64_t)A.delta * s;
            w = (int32_t)(v < (int64_t)A.W ? v : (int64_t)A.W);
            if (first) {
                C.sh->weight[gen & 1u][t] = w;
                C.sh->episodes[t] += ep, C.sh->successes[t] += su;
            }
        }
        cdf[t] = w;
        qgu_scan(cdf, t);
        if (end) qgu_draw(A, S, C, cdf, e, (uint64_t)C.segment[e] + 1u);
    }
    if (command_out && live) {                            // the commands in force after the launch, ended or not
        float *row = command_out + e * (size_t)A.out_stride;
        row[0] = S.vel[e], row[1] = S.vel[(size_t)A.n + e], row[2] = S.head[e], row[3] = S.head[(size_t)A.n + e];
    }
}

// begin (advance = 1), and the first draw of a new handle (advance = 0): the masked envs drop their segment unjudged and draw
__global__ __launch_bounds__(QGU_BLOCK) void qg_cmdcur_begin_kernel(KCmdCur A, KWalkState S, KCmdCurState C, const uint8_t *mask, int32_t advance) {
    __shared__ int32_t cdf[QG_CMDCUR_MAX_BINS];
    const int t = threadIdx.x;
    const int64_t e64 = (int64_t)blockIdx.x * QGU_BLOCK + t;
    const size_t e = (size_t)e64;
    cdf[t] = t < A.B ? C.sh->weight[C.sh->gen & 1u][t] : 0;
    qgu_scan(cdf, t);
    if (e64 >= A.n || (mask && mask[e] == 0)) return;
    qgu_draw(A, S, C, cdf, e, (uint64_t)C.segment[e] + (uint64_t)advance);
}

// ------------------------------------------------------------------------------------------------------
// host side
// ------------------------------------------------------------------------------------------------------
struct qg_cmdcur {
    qg_walk *walk;
    qg_cmdcur_desc desc;
    KCmdCur k;                // the handle's constants of a launch; the call's are filled in per launch
    KCmdCurState st;
    QgDevMem mem;
};

static int cmdcur_check_weights(const int32_t *w, int32_t B, int32_t W, const char *who, const char *name) {
    bool some = false;
    for (int b = 0; b < B; ++b) {
        if (w[b] < 0 || w[b] > W) return fail(QG_ERR_ARG, "%s: %s[%d] = %d outside 0 .. weight_max = %d", who, name, b, w[b], W);
        some = some || w[b] > 0;
    }
    if (!some) return fail(QG_ERR_ARG, "%s: %s holds no bin with a weight > 0: there would be nothing to draw from", who, name);
    return QG_OK;
}

static int cmdcur_validate(const qg_cmdcur_desc *d) {
    if (!d) return fail(QG_ERR_ARG, "qg_cmdcur_create: null description");
    QG_CHECK_STRUCT(d, qg_cmdcur_desc);
    if (d->reserved != 0 || d->reserved2 != 0) return fail(QG_ERR_ARG, "qg_cmdcur: reserved must be 0");
    if (d->n_speed < 1 || d->n_speed > QG_CMDCUR_MAX_SIDE) return fail(QG_ERR_ARG, "qg_cmdcur: n_speed %d outside 1 .. %d", d->n_speed, QG_CMDCUR_MAX_SIDE);
    if (d->n_alpha < 1 || d->n_alpha > QG_CMDCUR_MAX_SIDE) return fail(QG_ERR_ARG, "qg_cmdcur: n_alpha %d outside 1 .. %d", d->n_alpha, QG_CMDCUR_MAX_SIDE);
    if (!qg_finite32(d->speed_lo) || !qg_finite32(d->speed_hi) || !(d->speed_lo <= d->speed_hi))
        return fail(QG_ERR_ARG, "qg_cmdcur: speeds (%g, %g) must be finite and satisfy speed_lo <= speed_hi", d->speed_lo, d->speed_hi);
    if (d->fixed_heading != 0 && d->fixed_heading != 1) return fail(QG_ERR_ARG, "qg_cmdcur: fixed_heading %d must be 0 or 1", d->fixed_heading);
    if (!qg_finite32(d->heading_angle)) return fail(QG_ERR_ARG, "qg_cmdcur: heading_angle is not finite");
    if (d->weight_max < 1 || d->weight_max > QG_CMDCUR_MAX_WEIGHT)
        return fail(QG_ERR_ARG, "qg_cmdcur: weight_max %d outside 1 .. %d", d->weight_max, QG_CMDCUR_MAX_WEIGHT);
    if (d->delta < 1 || d->delta > d->weight_max) return fail(QG_ERR_ARG, "qg_cmdcur: delta %d outside 1 .. weight_max = %d", d->delta, d->weight_max);
    if (d->resample_steps < 0) return fail(QG_ERR_ARG, "qg_cmdcur: resample_steps %d must be >= 0", d->resample_steps);
    if (d->min_steps < 1) return fail(QG_ERR_ARG, "qg_cmdcur: min_steps %d must be >= 1", d->min_steps);
    if (d->n_criteria < 0 || d->n_criteria > QG_CMDCUR_MAX_CRITERIA)
        return fail(QG_ERR_ARG, "qg_cmdcur: n_criteria %d outside 0 .. %d", d->n_criteria, QG_CMDCUR_MAX_CRITERIA);
    for (int k = 0; k < d->n_criteria; ++k) {
        if (d->criteria[k].column < 0) return fail(QG_ERR_ARG, "qg_cmdcur: criteria[%d].column %d must be >= 0", k, d->criteria[k].column);
        if (d->criteria[k].sense != 1 && d->criteria[k].sense != -1)
            return fail(QG_ERR_ARG, "qg_cmdcur: criteria[%d].sense %d must be +1 or -1", k, d->criteria[k].sense);
        if (!qg_finite32(d->criteria[k].threshold)) return fail(QG_ERR_ARG, "qg_cmdcur: criteria[%d].threshold is not finite", k);
    }
    return cmdcur_check_weights(d->initial_weights, d->n_speed * d->n_alpha, d->weight_max, "qg_cmdcur", "initial_weights");
}

extern "C" int qg_cmdcur_destroy(qg_cmdcur *p) {
    if (!p) return QG_OK;
    p->walk->cmdcur = nullptr;
    qg_free_handle(p, p->walk->sim->device);              // launches may still be in flight on a caller's stream
    return QG_OK;
}

static int cmdcur_begin_launch(qg_cmdcur *p, const uint8_t *mask, int32_t advance, hipStream_t stream) {
    hipLaunchKernelGGL(qg_cmdcur_begin_kernel, dim3((unsigned)p->k.nblocks), dim3(QGU_BLOCK), 0, stream, p->k, p->walk->st, p->st, mask, advance);
    HIP_TRY(hipGetLastError(), QG_ERR_LAUNCH);
    return QG_OK;
}

extern "C" int qg_cmdcur_create(qg_walk *walk, const qg_cmdcur_desc *desc, qg_cmdcur **out) {
    if (!out) return fail(QG_ERR_ARG, "qg_cmdcur_create: null output");
    *out = nullptr;
    QG_TRY(cmdcur_validate(desc));
    if (!walk) return fail(QG_ERR_ARG, "qg_cmdcur_create: null walking layer");
    if (walk->kp.cmd_sample)
        return fail(QG_ERR_ARG, "qg_cmdcur_create: the walking layer has a command sampler installed, which would redraw the commands inside the "
                                "step (qg_walk_set_command_sampler(walk, NULL) first)");
    if (walk->cmdcur) return fail(QG_ERR_ARG, "qg_cmdcur_create: a command curriculum is already bound to this walking layer (destroy it first)");
    qg_sim *s = walk->sim;
    HIP_TRY(hipSetDevice(s->device), QG_ERR_DEVICE);
    qg_cmdcur *p = qg_new_handle<qg_cmdcur>();
    if (!p) return QG_ERR_ALLOC;
    p->walk = walk;
    p->desc = *desc;
    KCmdCur &k = p->k;
    k.n = s->n, k.n_speed = desc->n_speed, k.n_alpha = desc->n_alpha, k.B = desc->n_speed * desc->n_alpha;
    k.fixed_heading = desc->fixed_heading, k.heading_angle = desc->heading_angle;
    k.W = desc->weight_max, k.delta = desc->delta, k.R = desc->resample_steps, k.min_steps = desc->min_steps, k.n_criteria = desc->n_criteria;
    for (int c = 0; c < desc->n_criteria; ++c)
        k.column[c] = desc->criteria[c].column, k.sense[c] = desc->criteria[c].sense, k.threshold[c] = desc->criteria[c].threshold;
    k.speed_lo = desc->speed_lo;
    k.ws = (float)(((double)desc->speed_hi - (double)desc->speed_lo) / (double)desc->n_speed);
    k.wa = (float)(2.0 * 3.14159265358979323846 / (double)desc->n_alpha);
    k.seed_c = desc->seed + QGU_SALT, k.base = desc->env_index_base;
    k.nblocks = (int32_t)((s->n + QGU_BLOCK - 1) / QGU_BLOCK);
    const size_t n = (size_t)s->n, nb = (size_t)k.nblocks;
    KCmdCurState &C = p->st;
    if (p->mem.alloc(C.bin, n * sizeof(int32_t), true) || p->mem.alloc(C.steps, n * sizeof(int32_t), true) ||
        p->mem.alloc(C.sum, QG_CMDCUR_MAX_CRITERIA * n * sizeof(float), true) || p->mem.alloc(C.segment, n * sizeof(int64_t), true) ||
        p->mem.alloc(C.ended, n, true) || p->mem.alloc(C.sh, sizeof(QgcShared), true) || p->mem.alloc(C.block_any, nb * sizeof(int32_t), true) ||
        p->mem.alloc(C.partial, nb * 2 * QG_CMDCUR_MAX_BINS * sizeof(int32_t), true)) {
        qg_free_handle(p, s->device);
        return QG_ERR_ALLOC;
    }
    hipError_t e = hipMemcpy(C.sh->weight[0], desc->initial_weights, (size_t)k.B * sizeof(int32_t), hipMemcpyHostToDevice);    // gen = 0
    int rc = e == hipSuccess ? cmdcur_begin_launch(p, nullptr, 0, s->stream) : QG_OK;     // segment 0 of every env, and its command
    if (e == hipSuccess && rc == QG_OK) e = hipDeviceSynchronize();
    if (rc != QG_OK || e != hipSuccess) {
        qg_free_handle(p, s->device);
        return rc != QG_OK ? rc : fail(QG_ERR_DEVICE, "qg_cmdcur_create: %s", hipGetErrorString(e));
    }
    walk->cmdcur = p;
    *out = p;
    return QG_OK;
}

extern "C" int qg_cmdcur_advance_device(qg_cmdcur *p, const void *done, int32_t done_kind, int32_t done_stride, const float *components,
                                        int32_t components_stride, int32_t n_columns, float *command_out, int32_t command_out_stride, void *stream) {
    const char *who = "qg_cmdcur_advance_device";
    if (!p) return fail(QG_ERR_ARG, "%s: null handle", who);
    QG_TRY(qg_check_done(who, done, done_kind, done_stride));
    if (n_columns < 0) return fail(QG_ERR_ARG, "%s: n_columns %d must be >= 0", who, n_columns);
    if (!components && p->k.n_criteria > 0) return fail(QG_ERR_ARG, "%s: %d criteria without components", who, p->k.n_criteria);
    if (components && components_stride < n_columns)
        return fail(QG_ERR_ARG, "%s: components_stride %d must be >= n_columns %d", who, components_stride, n_columns);
    for (int c = 0; c < p->k.n_criteria; ++c)
        if (p->k.column[c] >= n_columns) return fail(QG_ERR_ARG, "%s: criteria[%d].column %d is not one of the %d columns", who, c, p->k.column[c], n_columns);
    if (command_out && command_out_stride < 4) return fail(QG_ERR_ARG, "%s: command_out_stride %d must be >= 4", who, command_out_stride);
    qg_sim *s = p->walk->sim;
    if (s->res.active) return fail(QG_ERR_ARG, "%s: the resident step mode is on (qg_resident_stop first)", who);

    HIP_TRY(hipSetDevice(s->device), QG_ERR_DEVICE);
    qg_note_caller_stream(s, (hipStream_t)stream);               // a later host-pointer call of the simulator waits for these launches
    KCmdCur A = p->k;
    A.done_kind = done_kind, A.done_stride = done ? done_stride : 1;
    A.comp_stride = components_stride, A.out_stride = command_out_stride;
    const dim3 grid((unsigned)A.nblocks), block(QGU_BLOCK);
    hipLaunchKernelGGL(qg_cmdcur_judge_kernel, grid, block, 0, (hipStream_t)stream, A, p->st, done, components);
    HIP_TRY(hipGetLastError(), QG_ERR_LAUNCH);
    hipLaunchKernelGGL(qg_cmdcur_draw_kernel, grid, block, 0, (hipStream_t)stream, A, p->walk->st, p->st, command_out);
    HIP_TRY(hipGetLastError(), QG_ERR_LAUNCH);
    return QG_OK;
}

extern "C" int qg_cmdcur_begin_device(qg_cmdcur *p, const uint8_t *mask, void *stream) {
    const char *who = "qg_cmdcur_begin_device";
    if (!p) return fail(QG_ERR_ARG, "%s: null handle", who);
    qg_sim *s = p->walk->sim;
    if (s->res.active) return fail(QG_ERR_ARG, "%s: the resident step mode is on (qg_resident_stop first)", who);
    HIP_TRY(hipSetDevice(s->device), QG_ERR_DEVICE);
    qg_note_caller_stream(s, (hipStream_t)stream);
    return cmdcur_begin_launch(p, mask, 1, (hipStream_t)stream);
}

// after everything in flight: the generation word
static int cmdcur_sync_gen(qg_cmdcur *p, uint32_t *gen) {
    HIP_TRY(hipSetDevice(p->walk->sim->device), QG_ERR_DEVICE);
    HIP_TRY(hipDeviceSynchronize(), QG_ERR_LAUNCH);               // a launch may be in flight on a caller's stream
    HIP_TRY(hipMemcpy(gen, &p->st.sh->gen, sizeof *gen, hipMemcpyDeviceToHost), QG_ERR_DEVICE);
    return QG_OK;
}

extern "C" int qg_cmdcur_get_weights(qg_cmdcur *p, int32_t *weights) {
    if (!p || !weights) return fail(QG_ERR_ARG, "qg_cmdcur_get_weights: null argument");
    uint32_t gen;
    QG_TRY(cmdcur_sync_gen(p, &gen));
    HIP_TRY(hipMemcpy(weights, p->st.sh->weight[gen & 1u], (size_t)p->k.B * sizeof(int32_t), hipMemcpyDeviceToHost), QG_ERR_DEVICE);
    return QG_OK;
}

extern "C" int qg_cmdcur_set_weights(qg_cmdcur *p, const int32_t *weights) {
    if (!p || !weights) return fail(QG_ERR_ARG, "qg_cmdcur_set_weights: null argument");
    QG_TRY(cmdcur_check_weights(weights, p->k.B, p->k.W, "qg_cmdcur_set_weights", "weights"));
    uint32_t gen;
    QG_TRY(cmdcur_sync_gen(p, &gen));
    HIP_TRY(hipMemcpy(p->st.sh->weight[gen & 1u], weights, (size_t)p->k.B * sizeof(int32_t), hipMemcpyHostToDevice), QG_ERR_DEVICE);
    return QG_OK;
}

extern "C" int qg_cmdcur_get_stats(qg_cmdcur *p, int64_t *episodes, int64_t *successes) {
    if (!p) return fail(QG_ERR_ARG, "qg_cmdcur_get_stats: null handle");
    uint32_t gen;
    QG_TRY(cmdcur_sync_gen(p, &gen));
    const size_t bytes = (size_t)p->k.B * sizeof(int64_t);
    if (episodes) HIP_TRY(hipMemcpy(episodes, p->st.sh->episodes, bytes, hipMemcpyDeviceToHost), QG_ERR_DEVICE);
    if (successes) HIP_TRY(hipMemcpy(successes, p->st.sh->successes, bytes, hipMemcpyDeviceToHost), QG_ERR_DEVICE);
    return QG_OK;
}

extern "C" int qg_cmdcur_get_bins(qg_cmdcur *p, int32_t *bin, int32_t *steps, int64_t *segment) {
    if (!p) return fail(QG_ERR_ARG, "qg_cmdcur_get_bins: null handle");
    uint32_t gen;
    QG_TRY(cmdcur_sync_gen(p, &gen));
    const size_t n = (size_t)p->k.n;
    if (bin) HIP_TRY(hipMemcpy(bin, p->st.bin, n * sizeof(int32_t), hipMemcpyDeviceToHost), QG_ERR_DEVICE);
    if (steps) HIP_TRY(hipMemcpy(steps, p->st.steps, n * sizeof(int32_t), hipMemcpyDeviceToHost), QG_ERR_DEVICE);
    if (segment) HIP_TRY(hipMemcpy(segment, p->st.segment, n * sizeof(int64_t), hipMemcpyDeviceToHost), QG_ERR_DEVICE);
    return QG_OK;
}

static int cmdcur_fields(const qg_cmdcur *p, QgField *f) {
    const size_t n = (size_t)p->k.n;
    const KCmdCurState &C = p->st;
    const QgField all[] = {{C.bin, n * sizeof(int32_t)}, {C.steps, n * sizeof(int32_t)}, {C.sum, QG_CMDCUR_MAX_CRITERIA * n * sizeof(float)},
                           {C.segment, n * sizeof(int64_t)}, {C.sh, sizeof(QgcShared)}};
    const int k = (int)(sizeof all / sizeof all[0]);
    if (f) memcpy(f, all, sizeof all);
    return k;
}
extern "C" int qg_cmdcur_state_bytes(const qg_cmdcur *p, int64_t *bytes) {
    if (!p || !bytes) return fail(QG_ERR_ARG, "qg_cmdcur_state_bytes: null argument");
    QgField f[QG_MAX_FIELDS];
    *bytes = qg_blob_bytes(f, cmdcur_fields(p, f));
    return QG_OK;
}
extern "C" int qg_cmdcur_get_state(qg_cmdcur *p, void *blob) {
    if (!p || !blob) return fail(QG_ERR_ARG, "qg_cmdcur_get_state: null argument");
    QgField f[QG_MAX_FIELDS];
    return qg_blob_out(p->walk->sim, QGU_BLOB, p->k.B, f, cmdcur_fields(p, f), blob);
}
extern "C" int qg_cmdcur_set_state(qg_cmdcur *p, const void *blob) {
    if (!p || !blob) return fail(QG_ERR_ARG, "qg_cmdcur_set_state: null argument");
    QgField f[QG_MAX_FIELDS];
    return qg_blob_in(p->walk->sim, QGU_BLOB, p->k.B, f, cmdcur_fields(p, f), blob, "qg_cmdcur_set_state");
}
