// qg_monitor.hip -- reward-term monitoring on the device (include/quadgym.h: qg_monitor_*): the row a training script logs at every
// env-step (the mean of every reward term over the envs, the reward's mean and population standard deviation, the number of envs
// that finished) into a ring at a cursor that lives in device memory, and per-term episode sums folded into totals over the finished
// episodes.  One record is TWO launches:
//
//   qg_monitor_tile_kernel      per tile of QGM_TILE x k envs (k = 1 up to QGM_TILE x QGM_MAX_TILES envs): every env's accumulators
//                               advance by one IEEE add per term, finished envs hand theirs over and start again; the tile's f64 column
//                               sums, the reward's (mean, M2), the finished envs' sums, lengths and count -> one slab row per tile.
//   qg_monitor_combine_kernel   ONE workgroup: the tiles' rows summed in runs whose bounds depend on the tile count alone, then a fixed
//                               tree over the runs; writes log[records % capacity], the totals and the cursor.
//
// No floating-point atomics, no integer atomics either, and no workgroup waits for, or reads what was written by, another workgroup
// of its own launch: the slab passes from the tile pass to the combine pass through a kernel boundary.  The tile pass reads the
// caller's rows and reads and writes its own envs' accumulators; the combine pass is the only reader and writer of the cursor.
//
// Layout.  A [n][C] row of C = 11 floats is not a whole number of 16-byte words, so lanes do not own envs at the load: the 256
// threads of a workgroup run along the flattened (env, column) index of a 256-env chunk -- consecutive lanes read consecutive floats,
// whatever C is, wherever the row stride equals C -- into LDS at an odd row pitch (C | 1 floats).  Then thread t owns env t of the
// chunk: its reads of the LDS rows are a stride of an odd number of banks (conflict-free), its accumulators are [C + 1][n] in global
// memory (term-major: a wave's access to one term is 512 contiguous bytes).
//
// Numerics.  Column sums are plain f64 sums in a fixed order (f32 inputs: the unit of the error is eps64 x sum |x|).  The standard
// deviation comes from the reward's f64 moments, K the thread's first reward (qg_moments_dev.h).

#include <hip/hip_runtime.h>

#include <cstring>

#include "qg_host.h"
#include "qg_moments_dev.h"

#define QGM_TILE 256              // envs per chunk = threads per workgroup of the tile pass (one env per thread)
#define QGM_WAVES (QGM_TILE / 64)
#define QGM_MAX_TILES 256         // slab rows; a tile takes k chunks in turn so that this holds
#define QGM_SUM_RUNS 4            // the combine pass adds the tiles' sums in 4 runs per column (one per wave), then ((0 + 1) + 2) + 3
#define QGM_CHAN_RUNS 64          // ... and merges the tiles' reward moments in 64 runs (one per lane), then a butterfly over the lanes
#define QGM_MAX_PITCH (QG_MONITOR_MAX_TERMS | 1)

// the sum over the 64 lanes in the order of the butterfly (32, 16, .. 1): the same bits in every lane, on every run
template <class T> __device__ __forceinline__ T qgm_wave_sum(T v) {
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) v += __shfl_xor(v, off, 64);
    return v;
}

// A slab row: W = 2 * (C + 1) + 2 doubles -- the column sums [C + 1], the finished envs' sums [C + 1], the reward's mean and M2 (its
// count is the tile's number of envs) -- and two integers beside it: the finished envs' lengths and their number.
struct KMonitor {
    int32_t n, C, Cp;              // Cp = C + 1: the reward is column C of every table
    int32_t R, chunks;             // envs per tile = QGM_TILE * chunks
    int32_t G;                     // tiles
    int32_t comp_stride, reward_stride;
    int32_t done_kind, done_stride;
    int32_t capacity;
};

__global__ __launch_bounds__(QGM_TILE) void qg_monitor_tile_kernel(KMonitor A, const float *__restrict__ comp, const float *__restrict__ reward,
                                                                   const void *done, double *__restrict__ acc, int32_t *__restrict__ len,
                                                                   double *__restrict__ part, long long *__restrict__ parti) {
    __shared__ float shx[QGM_TILE * QGM_MAX_PITCH];
    __shared__ double shr[QGM_WAVES][2 * (QG_MONITOR_MAX_TERMS + 1)];
    __shared__ double shc[QGM_WAVES][3];
    __shared__ long long shi[QGM_WAVES][2];
    const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
    const int C = A.C, Cp = A.Cp, P = C | 1, n = A.n;
    const long long row0 = (long long)blockIdx.x * A.R;
    const int W = 2 * Cp + 2;

    double sum[QG_MONITOR_MAX_TERMS + 1], fold[QG_MONITOR_MAX_TERMS + 1];
#pragma unroll
    for (int c = 0; c <= QG_MONITOR_MAX_TERMS; c++) sum[c] = 0.0, fold[c] = 0.0;
    double cnt = 0.0, K = 0.0, s1 = 0.0, s2 = 0.0;
    long long flen = 0, fcount = 0;

    for (int j = 0; j < A.chunks; j++) {
        const long long base = row0 + (long long)j * QGM_TILE;      // the chunk's first env
        const int rows = (int)min((long long)QGM_TILE, n - base);   // <= 0: the chunk is past the end (only in the last tile)
        if (j > 0) __syncthreads();                        // the previous chunk's rows have been read
        // the chunk's rows into LDS: the flattened (env, column) index runs along the threads
        const int items = max(rows, 0) * C;
        for (int idx = t; idx < items; idx += QGM_TILE) {
            const int r = idx / C, c = idx - r * C;
            shx[r * P + c] = comp[(size_t)(base + r) * A.comp_stride + c];
        }
        __syncthreads();
        if (t < rows) {
            const size_t i = (size_t)(base + t);
            const float rew = reward[i * A.reward_stride];
            const bool fin = done ? qg_done_at(done, A.done_kind, A.done_stride, i) : false;
#pragma unroll
            for (int c = 0; c <= QG_MONITOR_MAX_TERMS; c++) {
                if (c < Cp) {
                    const double x = (double)(c < C ? shx[t * P + c] : rew);
                    const double a = acc[(size_t)c * n + i] + x;          // ONE IEEE add per step and term
                    sum[c] += x;
                    fold[c] += fin ? a : 0.0;
                    acc[(size_t)c * n + i] = fin ? 0.0 : a;
                }
            }
            const int l = len[i] + 1;
            flen += fin ? l : 0;
            fcount += fin ? 1 : 0;
            len[i] = fin ? 0 : l;
            if (cnt == 0.0) K = (double)rew;
            const double d = (double)rew - K;
            s1 += d;
            s2 += d * d;
            cnt += 1.0;
        }
    }

    // the wave's sums by butterfly; the finished envs' sums only where the wave has one (a wave without adds up exact zeros)
    const bool any_fin = __any(fcount != 0);
#pragma unroll
    for (int c = 0; c <= QG_MONITOR_MAX_TERMS; c++) {
        if (c < Cp) {
            const double s = qgm_wave_sum(sum[c]);
            const double f = any_fin ? qgm_wave_sum(fold[c]) : 0.0;
            if (lane == 0) shr[wave][c] = s, shr[wave][Cp + c] = f;
        }
    }
    double mean, M2;
    qg_moments_finish(cnt, K, s1, s2, mean, M2);
    qg_moments_wave_merge(lane, cnt, mean, M2);
    flen = qgm_wave_sum(flen), fcount = qgm_wave_sum(fcount);
    if (lane == 0) {
        shc[wave][0] = cnt, shc[wave][1] = mean, shc[wave][2] = M2;
        shi[wave][0] = flen, shi[wave][1] = fcount;
    }
    __syncthreads();
    double *row = part + (size_t)blockIdx.x * W;
    if (t < 2 * Cp) {
        double s = shr[0][t];
        for (int w = 1; w < QGM_WAVES; w++) s += shr[w][t];
        row[t] = s;
    }
    if (t == 64) {                                          // (another wave than the sums' first)
        double na = shc[0][0], ma = shc[0][1], Ma = shc[0][2];
        for (int w = 1; w < QGM_WAVES; w++) qg_moments_merge(na, ma, Ma, shc[w][0], shc[w][1], shc[w][2]);
        row[2 * Cp] = ma, row[2 * Cp + 1] = Ma;
        long long fl = 0, fc = 0;
        for (int w = 0; w < QGM_WAVES; w++) fl += shi[w][0], fc += shi[w][1];
        parti[2 * blockIdx.x] = fl, parti[2 * blockIdx.x + 1] = fc;
    }
}

// counts: episodes | length_sum | records
__global__ __launch_bounds__(64 * QGM_SUM_RUNS) void qg_monitor_combine_kernel(KMonitor A, const double *__restrict__ part,
                                                                               const long long *__restrict__ parti, double *__restrict__ totals,
                                                                               long long *__restrict__ counts, double *__restrict__ log) {
    __shared__ double sh[QGM_SUM_RUNS][64];
    const int t = threadIdx.x, lane = t & 63, s = t >> 6;
    const int Cp = A.Cp, G = A.G, W = 2 * Cp + 2, n = A.n;
    const long long records = counts[2];
    double *out = log + (size_t)(records % A.capacity) * (Cp + 2);

    // the sums: run s of column v0 + lane, then the runs in order
    const int GS = (G + QGM_SUM_RUNS - 1) / QGM_SUM_RUNS;
    const int g1 = min(G, (s + 1) * GS);
    for (int v0 = 0; v0 < 2 * Cp; v0 += 64) {
        const int v = v0 + lane;
        const int vr = min(v, 2 * Cp - 1);
        double a = 0.0;
        for (int g = s * GS; g < g1; g++) a += part[(size_t)g * W + vr];
        if (v0 > 0) __syncthreads();
        sh[s][lane] = a;
        __syncthreads();
        if (s == 0 && v < 2 * Cp) {
            for (int r = 1; r < QGM_SUM_RUNS; r++) a += sh[r][lane];
            if (v < Cp) out[v] = a / (double)n;                      // the means: terms, then the reward
            else totals[v - Cp] = totals[v - Cp] + a;                // the fold: exact zero where nobody finished
        }
    }

    // the reward's moments and the integers, by the last wave: lane l merges run l of the tiles, then the butterfly
    if (s == QGM_SUM_RUNS - 1) {
        const int GC = (G + QGM_CHAN_RUNS - 1) / QGM_CHAN_RUNS;
        const int h1 = min(G, (lane + 1) * GC);
        double na = 0.0, ma = 0.0, Ma = 0.0;
        long long fl = 0, fc = 0;
        for (int g = lane * GC; g < h1; g++) {
            qg_moments_merge(na, ma, Ma, (double)min((long long)A.R, n - (long long)g * A.R), part[(size_t)g * W + 2 * Cp], part[(size_t)g * W + 2 * Cp + 1]);
            fl += parti[2 * g], fc += parti[2 * g + 1];
        }
        qg_moments_wave_merge(lane, na, ma, Ma);
        fl = qgm_wave_sum(fl), fc = qgm_wave_sum(fc);
        if (lane == 0) {
            out[Cp] = sqrt(Ma / (double)n);                          // population standard deviation (ddof = 0)
            out[Cp + 1] = (double)fc;
            counts[0] += fc;
            counts[1] += fl;
            counts[2] = records + 1;                                 // every thread read the cursor before the barriers above
        }
    }
}

// ------------------------------------------------------------------------------------------------------
// host side
// ------------------------------------------------------------------------------------------------------
struct qg_monitor {
    int32_t device;
    int32_t n, C, Cp, capacity;
    int32_t R, chunks, G;     // the tile pass's partition: a function of n alone
    QgDevMem mem;
    double *d_acc;            // [Cp][n]: the running episodes' sums, term-major
    int32_t *d_len;           // [n]
    double *d_totals;         // [Cp]
    long long *d_counts;      // episodes | length_sum | records
    double *d_part;           // [G][2 * Cp + 2]
    long long *d_parti;       // [G][2]
};

extern "C" int qg_monitor_destroy(qg_monitor *p) {
    if (p) qg_free_handle(p, p->device);           // records may still be in flight on a caller's stream
    return QG_OK;
}

extern "C" int qg_monitor_create(int32_t device_id, int32_t n_envs, int32_t n_terms, int32_t capacity, qg_monitor **out) {
    if (!out) return fail(QG_ERR_ARG, "qg_monitor_create: null output");
    *out = nullptr;
    if (n_envs < 1) return fail(QG_ERR_ARG, "qg_monitor: n_envs %d must be >= 1", n_envs);
    if (n_terms < 1 || n_terms > QG_MONITOR_MAX_TERMS)
        return fail(QG_ERR_ARG, "qg_monitor: n_terms %d outside 1 .. %d", n_terms, QG_MONITOR_MAX_TERMS);
    if (capacity < 1) return fail(QG_ERR_ARG, "qg_monitor: capacity %d must be >= 1", capacity);
    QG_TRY(qg_open_device(device_id, nullptr));
    qg_monitor *p = qg_new_handle<qg_monitor>();
    if (!p) return QG_ERR_ALLOC;
    p->device = device_id;
    p->n = n_envs, p->C = n_terms, p->Cp = n_terms + 1, p->capacity = capacity;
    p->chunks = (int32_t)(((int64_t)n_envs + (int64_t)QGM_TILE * QGM_MAX_TILES - 1) / ((int64_t)QGM_TILE * QGM_MAX_TILES));
    p->R = QGM_TILE * p->chunks;
    p->G = (int32_t)(((int64_t)n_envs + p->R - 1) / p->R);
    const size_t W = 2 * (size_t)p->Cp + 2;
    if (p->mem.alloc(p->d_acc, (size_t)p->Cp * n_envs * sizeof(double), true) || p->mem.alloc(p->d_len, (size_t)n_envs * sizeof(int32_t), true) ||
        p->mem.alloc(p->d_totals, (size_t)p->Cp * sizeof(double), true) || p->mem.alloc(p->d_counts, 3 * sizeof(long long), true) ||
        p->mem.alloc(p->d_part, (size_t)p->G * W * sizeof(double), true) || p->mem.alloc(p->d_parti, (size_t)p->G * 2 * sizeof(long long), true)) {
        qg_monitor_destroy(p);
        return QG_ERR_ALLOC;
    }
    hipError_t e = hipDeviceSynchronize();
    if (e != hipSuccess) {
        qg_monitor_destroy(p);
        return fail(QG_ERR_DEVICE, "qg_monitor_create: %s", hipGetErrorString(e));
    }
    *out = p;
    return QG_OK;
}

extern "C" int qg_monitor_record_device(qg_monitor *p, const float *components, int32_t comp_stride, const float *reward, int32_t reward_stride,
                                        const void *done, int32_t done_kind, int32_t done_stride, double *log, void *stream) {
    if (!p || !components || !reward || !log) return fail(QG_ERR_ARG, "qg_monitor_record_device: null argument");
    if (comp_stride < p->C) return fail(QG_ERR_ARG, "qg_monitor_record_device: comp_stride %d < n_terms %d", comp_stride, p->C);
    if (reward_stride < 1) return fail(QG_ERR_ARG, "qg_monitor_record_device: reward_stride %d must be >= 1", reward_stride);
    QG_TRY(qg_check_done("qg_monitor_record_device", done, done_kind, done_stride));
    HIP_TRY(hipSetDevice(p->device), QG_ERR_DEVICE);
    const hipStream_t st = (hipStream_t)stream;
    KMonitor A;
    memset(&A, 0, sizeof A);
    A.n = p->n, A.C = p->C, A.Cp = p->Cp, A.R = p->R, A.chunks = p->chunks, A.G = p->G;
    A.comp_stride = comp_stride, A.reward_stride = reward_stride;
    A.done_kind = done_kind, A.done_stride = done_stride;
    A.capacity = p->capacity;
    qg_monitor_tile_kernel<<<(unsigned)p->G, QGM_TILE, 0, st>>>(A, components, reward, done, p->d_acc, p->d_len, p->d_part, p->d_parti);
    HIP_TRY(hipGetLastError(), QG_ERR_LAUNCH);
    qg_monitor_combine_kernel<<<1, 64 * QGM_SUM_RUNS, 0, st>>>(A, p->d_part, p->d_parti, p->d_totals, p->d_counts, log);
    HIP_TRY(hipGetLastError(), QG_ERR_LAUNCH);
    return QG_OK;
}

// the accumulators between the device's [Cp][n] and the interface's [n][Cp]
static void monitor_transpose(const double *src, double *dst, int rows, int cols) {
    for (int r = 0; r < rows; r++)
        for (int c = 0; c < cols; c++) dst[(size_t)c * rows + r] = src[(size_t)r * cols + c];
}

extern "C" int qg_monitor_reset(qg_monitor *p, const uint8_t *host_mask, int32_t clear_totals, int32_t clear_log) {
    if (!p) return fail(QG_ERR_ARG, "qg_monitor_reset: null argument");
    HIP_TRY(hipSetDevice(p->device), QG_ERR_DEVICE);
    HIP_TRY(hipDeviceSynchronize(), QG_ERR_LAUNCH);         // a record may be in flight on a caller's stream
    const int n = p->n, Cp = p->Cp;
    if (!host_mask) {
        HIP_TRY(hipMemset(p->d_acc, 0, (size_t)Cp * n * sizeof(double)), QG_ERR_DEVICE);
        HIP_TRY(hipMemset(p->d_len, 0, (size_t)n * sizeof(int32_t)), QG_ERR_DEVICE);
    } else {
        QgHostBuf<double> acc((size_t)Cp * n);
        QgHostBuf<int32_t> len(n);
        QG_TRY(acc.oom());
        QG_TRY(len.oom());
        HIP_TRY(hipMemcpy(acc, p->d_acc, (size_t)Cp * n * sizeof(double), hipMemcpyDeviceToHost), QG_ERR_DEVICE);
        HIP_TRY(hipMemcpy(len, p->d_len, (size_t)n * sizeof(int32_t), hipMemcpyDeviceToHost), QG_ERR_DEVICE);
        for (int i = 0; i < n; i++)
            if (host_mask[i]) {
                for (int c = 0; c < Cp; c++) acc[(size_t)c * n + i] = 0.0;
                len[i] = 0;
            }
        HIP_TRY(hipMemcpy(p->d_acc, acc, (size_t)Cp * n * sizeof(double), hipMemcpyHostToDevice), QG_ERR_DEVICE);
        HIP_TRY(hipMemcpy(p->d_len, len, (size_t)n * sizeof(int32_t), hipMemcpyHostToDevice), QG_ERR_DEVICE);
    }
    if (clear_totals) {
        HIP_TRY(hipMemset(p->d_totals, 0, (size_t)Cp * sizeof(double)), QG_ERR_DEVICE);
        HIP_TRY(hipMemset(p->d_counts, 0, 2 * sizeof(long long)), QG_ERR_DEVICE);
    }
    if (clear_log) HIP_TRY(hipMemset(p->d_counts + 2, 0, sizeof(long long)), QG_ERR_DEVICE);
    HIP_TRY(hipDeviceSynchronize(), QG_ERR_LAUNCH);
    return QG_OK;
}

extern "C" int qg_monitor_get_info(qg_monitor *p, int64_t *records, int64_t *episodes, int64_t *length_sum, double *totals, int32_t clear) {
    if (!p || !records || !episodes || !length_sum || !totals) return fail(QG_ERR_ARG, "qg_monitor_get_info: null argument");
    HIP_TRY(hipSetDevice(p->device), QG_ERR_DEVICE);
    HIP_TRY(hipDeviceSynchronize(), QG_ERR_LAUNCH);
    long long counts[3];
    HIP_TRY(hipMemcpy(counts, p->d_counts, sizeof counts, hipMemcpyDeviceToHost), QG_ERR_DEVICE);
    HIP_TRY(hipMemcpy(totals, p->d_totals, (size_t)p->Cp * sizeof(double), hipMemcpyDeviceToHost), QG_ERR_DEVICE);
    *episodes = counts[0], *length_sum = counts[1], *records = counts[2];
    if (clear) {
        HIP_TRY(hipMemset(p->d_totals, 0, (size_t)p->Cp * sizeof(double)), QG_ERR_DEVICE);
        HIP_TRY(hipMemset(p->d_counts, 0, 2 * sizeof(long long)), QG_ERR_DEVICE);
        HIP_TRY(hipDeviceSynchronize(), QG_ERR_LAUNCH);
    }
    return QG_OK;
}

extern "C" int qg_monitor_get_state(qg_monitor *p, double *acc, int32_t *len, double *totals, int64_t *episodes, int64_t *length_sum,
                                    int64_t *records) {
    if (!p || !acc || !len) return fail(QG_ERR_ARG, "qg_monitor_get_state: null argument");
    QG_TRY(qg_monitor_get_info(p, records, episodes, length_sum, totals, 0));
    const int n = p->n, Cp = p->Cp;
    QgHostBuf<double> h((size_t)Cp * n);
    QG_TRY(h.oom());
    HIP_TRY(hipMemcpy(h, p->d_acc, (size_t)Cp * n * sizeof(double), hipMemcpyDeviceToHost), QG_ERR_DEVICE);
    HIP_TRY(hipMemcpy(len, p->d_len, (size_t)n * sizeof(int32_t), hipMemcpyDeviceToHost), QG_ERR_DEVICE);
    monitor_transpose(h, acc, Cp, n);
    return QG_OK;
}

extern "C" int qg_monitor_set_state(qg_monitor *p, const double *acc, const int32_t *len, const double *totals, int64_t episodes,
                                    int64_t length_sum, int64_t records) {
    if (!p || !acc || !len || !totals) return fail(QG_ERR_ARG, "qg_monitor_set_state: null argument");
    if (episodes < 0 || length_sum < 0 || records < 0)
        return fail(QG_ERR_ARG, "qg_monitor_set_state: episodes, length_sum and records must be >= 0");
    const int n = p->n, Cp = p->Cp;
    for (int i = 0; i < n; i++)
        if (len[i] < 0) return fail(QG_ERR_ARG, "qg_monitor_set_state: len[%d] is %d (>= 0)", i, len[i]);
    HIP_TRY(hipSetDevice(p->device), QG_ERR_DEVICE);
    HIP_TRY(hipDeviceSynchronize(), QG_ERR_LAUNCH);
    QgHostBuf<double> h((size_t)Cp * n);
    QG_TRY(h.oom());
    monitor_transpose(acc, h, n, Cp);
    const long long counts[3] = {episodes, length_sum, records};
    HIP_TRY(hipMemcpy(p->d_acc, h, (size_t)Cp * n * sizeof(double), hipMemcpyHostToDevice), QG_ERR_DEVICE);
    HIP_TRY(hipMemcpy(p->d_len, len, (size_t)n * sizeof(int32_t), hipMemcpyHostToDevice), QG_ERR_DEVICE);
    HIP_TRY(hipMemcpy(p->d_totals, totals, (size_t)Cp * sizeof(double), hipMemcpyHostToDevice), QG_ERR_DEVICE);
    HIP_TRY(hipMemcpy(p->d_counts, counts, sizeof counts, hipMemcpyHostToDevice), QG_ERR_DEVICE);
    HIP_TRY(hipDeviceSynchronize(), QG_ERR_LAUNCH);
    return QG_OK;
}
