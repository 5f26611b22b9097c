// qg_comm.hip -- native per-step exchange over RCCL.
//
// The reference has no distributed layer (SB3's process-per-env SubprocVecEnv only, src/train_quadruped.py:49-50);
// the MI355X counterpart shards the env batch over the GPUs of a node and gathers the packed (obs, reward, done) rows
// to the learner rank once per env-step.  torch.distributed can do that gather, but at 4096 envs per GPU an env-step is
// an 18 us kernel and torch's per-collective host cost (~30 us) is what bounds the rate.  This file is the same exchange
// issued from C: one loop, per step { wait for the reader of the buffer, launch the step, ncclGroupStart, ncclRecv x N on
// the root / ncclSend, ncclGroupEnd } on two HIP streams chained by events.  RCCL is loaded with dlopen(): the library
// has no link-time dependency on it, and a process that already holds torch's copy (same SONAME) reuses that one.
#include <dlfcn.h>

#include <cstring>
#include <new>

#include "qg_sim.h"

typedef struct { char internal[128]; } qg_nccl_unique_id;     // ncclUniqueId (rccl.h: NCCL_UNIQUE_ID_BYTES = 128)
typedef void *qg_nccl_comm;                                    // ncclComm_t
enum { QG_NCCL_FLOAT32 = 7 };                                  // ncclFloat32

struct qg_rccl_api {
    void *handle;
    int (*GetUniqueId)(qg_nccl_unique_id *);
    int (*CommInitRank)(qg_nccl_comm *, int, qg_nccl_unique_id, int);
    int (*CommDestroy)(qg_nccl_comm);
    int (*GroupStart)(void);
    int (*GroupEnd)(void);
    int (*Send)(const void *, size_t, int, int, qg_nccl_comm, hipStream_t);
    int (*Recv)(void *, size_t, int, int, qg_nccl_comm, hipStream_t);
    const char *(*GetErrorString)(int);
};

static qg_rccl_api g_rccl = {};

static int qg_rccl_load(void) {
    if (g_rccl.handle) return QG_OK;
    const char *names[] = {"librccl.so.1", "librccl.so", "/opt/rocm/lib/librccl.so.1"};
    void *h = nullptr;
    for (const char *nm : names) {
        h = dlopen(nm, RTLD_NOW | RTLD_GLOBAL);
        if (h) break;
    }
    if (!h) return fail(QG_ERR_DEVICE, "RCCL not found (librccl.so.1): %s", dlerror());
#define QG_SYM(field, sym)                                                                 \
    *(void **)(&g_rccl.field) = dlsym(h, sym);                                             \
    if (!g_rccl.field) return fail(QG_ERR_DEVICE, "RCCL symbol %s missing", sym)
    QG_SYM(GetUniqueId, "ncclGetUniqueId");
    QG_SYM(CommInitRank, "ncclCommInitRank");
    QG_SYM(CommDestroy, "ncclCommDestroy");
    QG_SYM(GroupStart, "ncclGroupStart");
    QG_SYM(GroupEnd, "ncclGroupEnd");
    QG_SYM(Send, "ncclSend");
    QG_SYM(Recv, "ncclRecv");
    QG_SYM(GetErrorString, "ncclGetErrorString");
#undef QG_SYM
    g_rccl.handle = h;
    return QG_OK;
}

#define RCCL_TRY(expr)                                                                     \
    do {                                                                                   \
        int r_ = (expr);                                                                   \
        if (r_ != 0) return fail(QG_ERR_DEVICE, "%s: %s", #expr, g_rccl.GetErrorString(r_)); \
    } while (0)

struct qg_comm {
    qg_sim *sim;
    qg_nccl_comm comm;
    int rank, world;
    hipStream_t comm_stream;
    hipEvent_t produced[2], consumed[2];
    int consumed_valid[2];
};

extern "C" int qg_comm_unique_id(uint8_t id[QG_COMM_ID_BYTES]) {
    if (!id) return fail(QG_ERR_ARG, "qg_comm_unique_id: null output");
    QG_TRY(qg_rccl_load());
    qg_nccl_unique_id u;
    RCCL_TRY(g_rccl.GetUniqueId(&u));
    memcpy(id, u.internal, QG_COMM_ID_BYTES);
    return QG_OK;
}

extern "C" int qg_comm_destroy(qg_comm *c) {
    if (!c) return QG_OK;
    (void)hipSetDevice(c->sim->device);
    if (c->comm_stream) (void)hipStreamSynchronize(c->comm_stream);
    if (c->comm && g_rccl.CommDestroy) (void)g_rccl.CommDestroy(c->comm);
    for (int i = 0; i < 2; i++) {
        if (c->produced[i]) (void)hipEventDestroy(c->produced[i]);
        if (c->consumed[i]) (void)hipEventDestroy(c->consumed[i]);
    }
    if (c->comm_stream) (void)hipStreamDestroy(c->comm_stream);
    delete c;
    return QG_OK;
}

extern "C" int qg_comm_create(qg_sim *s, int32_t rank, int32_t world, const uint8_t id[QG_COMM_ID_BYTES], qg_comm **out) {
    if (!s || !id || !out || world < 1 || rank < 0 || rank >= world) return fail(QG_ERR_ARG, "qg_comm_create: bad argument");
    *out = nullptr;
    QG_TRY(qg_rccl_load());
    HIP_TRY(hipSetDevice(s->device), QG_ERR_DEVICE);
    qg_comm *c = qg_new_handle<qg_comm>();
    if (!c) return QG_ERR_ALLOC;
    c->sim = s;
    c->rank = rank;
    c->world = world;
    hipError_t e = hipStreamCreateWithFlags(&c->comm_stream, hipStreamNonBlocking);
    for (int i = 0; i < 2 && e == hipSuccess; i++) {
        e = hipEventCreateWithFlags(&c->produced[i], hipEventDisableTiming);
        if (e == hipSuccess) e = hipEventCreateWithFlags(&c->consumed[i], hipEventDisableTiming);
    }
    if (e != hipSuccess) {
        qg_comm_destroy(c);
        return fail(QG_ERR_DEVICE, "qg_comm_create: %s", hipGetErrorString(e));
    }
    qg_nccl_unique_id u;
    memcpy(u.internal, id, QG_COMM_ID_BYTES);
    int r = g_rccl.CommInitRank(&c->comm, world, u, rank);
    if (r != 0) {
        const char *msg = g_rccl.GetErrorString(r);
        qg_comm_destroy(c);
        return fail(QG_ERR_DEVICE, "ncclCommInitRank: %s", msg);
    }
    *out = c;
    return QG_OK;
}

extern "C" int qg_comm_rollout(qg_comm *c, const float *const *actions, int32_t n_actions, float *const packed[2], float *const gathered[2],
                               int32_t steps, int32_t root) {
    if (!c || !actions || n_actions < 1 || !packed || steps < 0 || root < 0 || root >= c->world) return fail(QG_ERR_ARG, "qg_comm_rollout: bad argument");
    if (c->rank == root && !gathered) return fail(QG_ERR_ARG, "qg_comm_rollout: the root needs the gathered buffers");
    qg_sim *s = c->sim;
    HIP_TRY(hipSetDevice(s->device), QG_ERR_DEVICE);
    const size_t count = (size_t)s->n * (size_t)(s->obs_dim + 2);
    for (int k = 0; k < steps; k++) {
        const int b = k & 1;
        // the step may overwrite packed[b] only after the gather that read it (two steps ago) has finished
        if (c->consumed_valid[b]) HIP_TRY(hipStreamWaitEvent(s->stream, c->consumed[b], 0), QG_ERR_DEVICE);
        QG_TRY(qg_launch_step(s, actions[k % n_actions], nullptr, nullptr, nullptr, nullptr, packed[b], s->stream));
        HIP_TRY(hipEventRecord(c->produced[b], s->stream), QG_ERR_DEVICE);
        HIP_TRY(hipStreamWaitEvent(c->comm_stream, c->produced[b], 0), QG_ERR_DEVICE);
        RCCL_TRY(g_rccl.GroupStart());
        if (c->rank == root)
            for (int r = 0; r < c->world; r++)
                RCCL_TRY(g_rccl.Recv(gathered[b] + (size_t)r * count, count, QG_NCCL_FLOAT32, r, c->comm, c->comm_stream));
        RCCL_TRY(g_rccl.Send(packed[b], count, QG_NCCL_FLOAT32, root, c->comm, c->comm_stream));
        RCCL_TRY(g_rccl.GroupEnd());
        HIP_TRY(hipEventRecord(c->consumed[b], c->comm_stream), QG_ERR_DEVICE);
        c->consumed_valid[b] = 1;
    }
    return QG_OK;
}

extern "C" int qg_comm_synchronize(qg_comm *c) {
    if (!c) return fail(QG_ERR_ARG, "null handle");
    HIP_TRY(hipSetDevice(c->sim->device), QG_ERR_DEVICE);
    HIP_TRY(hipStreamSynchronize(c->sim->stream), QG_ERR_LAUNCH);
    HIP_TRY(hipStreamSynchronize(c->comm_stream), QG_ERR_LAUNCH);
    return QG_OK;
}
