// qg_host.h -- what every host translation unit of the library shares: the error record and the two status-forwarding macros, the
// struct_size refusal, the done vector's check and read, the finite and alignment tests, a host staging buffer, opening a device, the
// owner of a handle's device allocations and a handle's birth and death.  Internal: not installed, and nothing in here is exported (libquadgym.map).
#pragma once
#include <cstddef>
#include <cstdint>
#include <cstring>
#include <new>

#include "../../include/quadgym.h"

int qg_fail(int code, const char *fmt, ...);   // records the message for qg_last_error() and returns `code` (qg_capi.hip)
#define fail qg_fail
// a status of the library's own that is only forwarded (the message is the callee's)
#define QG_TRY(expr) do { int rc_ = (expr); if (rc_ != QG_OK) return rc_; } while (0)
// the refusal of a struct of the ABI whose struct_size is not this library's (`type` is spelled into the message)
#define QG_CHECK_STRUCT(ptr, type)                                                                                          \
    do {                                                                                                                    \
        if ((ptr)->struct_size != (int32_t)sizeof(type))                                                                    \
            return fail(QG_ERR_ARG, #type ".struct_size is %d, this library's is %d", (ptr)->struct_size, (int)sizeof(type)); \
    } while (0)

// the done vector of include/quadgym.h as an entry point `who` received it: NULL passes, whatever kind and stride say
static inline int qg_check_done(const char *who, const void *done, int32_t kind, int32_t stride) {
    if (!done) return QG_OK;
    if (kind != QG_DONE_U8 && kind != QG_DONE_F32) return fail(QG_ERR_ARG, "%s: done_kind %d is neither QG_DONE_U8 nor QG_DONE_F32", who, kind);
    if (stride < 1) return fail(QG_ERR_ARG, "%s: done_stride %d must be >= 1", who, stride);
    return QG_OK;
}

// (exponent bits, not std::isfinite: the device pass, which parses the host code too, is compiled with finite-math assumptions and
// warns about the latter)
static inline bool qg_finite32(float x) {
    uint32_t u;
    memcpy(&u, &x, sizeof u);
    return (u & 0x7f800000u) != 0x7f800000u;
}
static inline bool qg_finite64(double x) {
    uint64_t u;
    memcpy(&u, &x, sizeof u);
    return ((u >> 52) & 0x7ff) != 0x7ff;
}

#ifdef __HIPCC__   // (qg_tables.h, which the plain-C++ generator of the baked table includes, needs the lines above only)
#include <hip/hip_runtime.h>

// `p` sits at a multiple of `a` bytes (NULL does)
__host__ __device__ static inline bool qg_aligned(const void *p, size_t a) { return ((uintptr_t)p) % a == 0; }

// [n] rows of `a_width` floats at `a_stride` and [n] rows of `b_width` floats at `b_stride`: the float ranges they span intersect
static inline bool qg_rows_overlap(const float *a, int64_t a_stride, int a_width, const float *b, int64_t b_stride, int b_width, int64_t n) {
    const uintptr_t a0 = (uintptr_t)a, a1 = (uintptr_t)(a + (n - 1) * a_stride + a_width);
    const uintptr_t b0 = (uintptr_t)b, b1 = (uintptr_t)(b + (n - 1) * b_stride + b_width);
    return a0 < b1 && b0 < a1;
}

// A host staging buffer of `count` elements that frees itself on every return path.  Nothing throws: a failed allocation leaves NULL,
// which oom() turns into the library's status.
template <class T> struct QgHostBuf {
    T *p;
    explicit QgHostBuf(size_t count) : p(new (std::nothrow) T[count]) {}
    ~QgHostBuf() { delete[] p; }
    QgHostBuf(const QgHostBuf &) = delete;
    QgHostBuf &operator=(const QgHostBuf &) = delete;
    operator T *() const { return p; }
    int oom() const { return p ? QG_OK : fail(QG_ERR_ALLOC, "out of host memory"); }
};

// element i of a done vector that passed qg_check_done (not NULL; kind is one of the two, so one compare tells them apart)
__device__ __forceinline__ bool qg_done_at(const void *done, int32_t kind, int32_t stride, size_t i) {
    return kind != QG_DONE_U8 ? ((const float *)done)[i * (size_t)stride] != 0.f : ((const uint8_t *)done)[i * (size_t)stride] != 0;
}

#define HIP_TRY(expr, code)                                                                         \
    do {                                                                                            \
        hipError_t e_ = (expr);                                                                     \
        if (e_ != hipSuccess) return fail(code, "%s: %s", #expr, hipGetErrorString(e_));            \
    } while (0)

// SIMDs of a GPU (hipDeviceProp: compute units x 4); 1024, an MI355X's, where the query fails
static inline int qg_device_simds(int32_t device_id) {
    hipDeviceProp_t prop;
    if (device_id >= 0 && hipGetDeviceProperties(&prop, device_id) == hipSuccess && prop.multiProcessorCount > 0) return 4 * prop.multiProcessorCount;
    (void)hipGetLastError();
    return 1024;
}

// what every create does first: there is a device, `device_id` names one, it is the calling thread's current device
static inline int qg_open_device(int32_t device_id, int *simds) {
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev < 1) {
        (void)hipGetLastError();
        return fail(QG_ERR_DEVICE, "no HIP device is available; quadgym has no CPU backend");
    }
    if (device_id < 0 || device_id >= ndev) return fail(QG_ERR_DEVICE, "device_id %d out of range (0..%d)", device_id, ndev - 1);
    HIP_TRY(hipSetDevice(device_id), QG_ERR_DEVICE);
    if (simds) *simds = qg_device_simds(device_id);
    return QG_OK;
}

// The device allocations of one handle: alloc() records what it hands out, free_all() in the handle's destroy releases all of it --
// no list of pointers to keep in step with the allocations.  All zeros is the empty owner (the handles are zero-filled at create).
struct QgDevMem {
    void *ptr[40];
    int count;

    template <class T> int alloc(T *&p, size_t bytes, bool zero = false) {
        if (count == (int)(sizeof ptr / sizeof ptr[0])) return fail(QG_ERR_ALLOC, "hipMalloc(%zu): the handle's allocation table is full", bytes);
        hipError_t e = hipMalloc((void **)&p, bytes);
        if (e != hipSuccess) {
            p = nullptr;
            return fail(QG_ERR_ALLOC, "hipMalloc(%zu): %s", bytes, hipGetErrorString(e));
        }
        ptr[count++] = (void *)p;
        if (zero && (e = hipMemset((void *)p, 0, bytes)) != hipSuccess) return fail(QG_ERR_ALLOC, "hipMalloc(%zu): %s", bytes, hipGetErrorString(e));
        return QG_OK;
    }
    void free_all() {
        while (count > 0) (void)hipFree(ptr[--count]);
    }
};

// A handle is born zero-filled (NULL, with the message recorded, where the host is out of memory) ...
template <class T> T *qg_new_handle() {
    T *h = new (std::nothrow) T();
    if (h) memset((void *)h, 0, sizeof *h);
    else fail(QG_ERR_ALLOC, "out of host memory");
    return h;
}
// ... and dies after what is in flight on its device: the caller's comment says what that may be
template <class T> void qg_free_handle(T *h, int device) {
    (void)hipSetDevice(device);
    (void)hipDeviceSynchronize();
    h->mem.free_all();
    delete h;
}
#endif
