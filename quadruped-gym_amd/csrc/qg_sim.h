// qg_sim.h -- the simulator handle and the few functions that cross translation units: those of the simulator's own four units
// (qg_capi.hip the core, qg_sim_host.hip, qg_sim_multi.hip, qg_sim_modes.hip) and of the walking layer (qg_walk.hip) that each other
// and the layers bound to a simulator -- qg_comm.hip, qg_walk.hip, qg_po.hip -- call (what the core and the step-kernel units share
// on top of it is in qg_step_launch.h).  Internal: not installed, and nothing in here is exported (libquadgym.map).
#pragma once
#include "qg_host.h"
#include "qg_device.h"
#include "qg_walk_dev.h"     // KWalkParams / KWalkState / KWalkLaunch
#include "qg_po_dev.h"       // KPoLaunch

struct qg_sim {
    int32_t n;
    int32_t device;
    int32_t obs_dim;
    qg_model model;
    qg_task task;
    QgDevMem mem;             // every device allocation below (qg_destroy frees through it)
    KModel *d_model;
    KTask *d_task;
    KState st;
    // staging for the host-pointer entry points
    float *d_actions, *d_obs, *d_reward, *d_comps, *d_stage;
    int32_t caller_inflight;  // a device-pointer step has been enqueued on a caller's stream since the last device-wide wait
    int32_t captured_once;    // a device-pointer step of this handle has been CAPTURED into a hipGraph: replays enqueue steps the library
                              // never sees, so from then on every host-pointer call takes the device-wide wait (sticky)
    uint8_t *h_pin;           // page-locked staging of the host-pointer entry points (qg_sim_host.hip)
    size_t h_pin_cap;
    uint8_t *d_done, *d_mask;
    hipStream_t stream;       // the library's own stream (host-pointer calls, timing)
    hipEvent_t ev0, ev1;
    uint64_t seed;
    uint64_t env_index_base;
    int32_t track_ctrl;
    int32_t link_helpers;     // walking forms of the one-link-per-lane kernel run with helper waves (QG_LINK_HELPERS at qg_create; default 1)
    int32_t model_baked;      // the model equals the compiled-in default (set once by qg_create; what runs: qg_sim_baked below)
    // per-env dynamics (qg_set_dynamics_range / qg_set_dynamics)
    int32_t dyn;              // the mode is on: the per-env forms of the table-driven step kernels run
    int32_t dyn_range_set;    // QG_RESET_DYNAMICS may draw
    KDynRange dyn_range;
    float *d_dyn;             // [QG_NDYN][n]
    KModelDyn *d_model_dyn;   // the model tables and d_dyn: the per-env kernels' model pointer
    // external wrenches (qg_set_xfrc / qg_set_push): wrench mode runs the same per-env kernels (identity dynamics rows while the
    // dynamics mode is off)
    int32_t xfrc;             // wrench mode is on
    float *d_xfrc;            // [n][QG_NBODY][QG_NXFRC]
    KPush push;               // the push schedule (interval 0: off)
    int32_t mapping;         // QG_MAP_AUTO / QG_MAP_LANE / QG_MAP_QUAD (request)
    int32_t creating;
    int32_t walk_bound;       // qg_walk layers bound to this handle (qg_set_task refuses while > 0)
    int32_t po_unfused;       // env QG_PO_UNFUSED=1: keep the observation pack of qg_po_step a launch of its own (A/B, parity test)
    int32_t simds;            // SIMDs of the handle's GPU (qg_open_device; 1024 on an MI355X): AUTO's thresholds are "one wave per SIMD" sizes
    mutable uint32_t last_step_kernel;    // the step-kernel instantiation the latest launcher enqueued (step_kernel_code; 0: none yet)
    // resident form of the one-link-per-lane step (qg_resident_*, qg_kernel_resident.hip)
    struct {
        int32_t active;       // qg_resident_start has set the mailbox up (the mode is on until qg_resident_stop)
        int32_t launched;     // a resident launch has been enqueued and has not been waited for since
        KResident k;          // mailbox pointers, slots, time-outs
        void *d_mail;         // door, arrival shards, completed counter (one allocation)
        volatile unsigned long long *hstat;   // page-locked host words the kernels report into
        hipStream_t ctl_stream;
        hipStream_t last_stream;              // where the latest ring went (waited for before the kernel is retired)
        int32_t own_buffers;                  // the action / output slots are the library's (else the caller's, qg_resident_start)
        int64_t rung;         // env-steps rung through the API since qg_resident_start
        uint64_t lost_seen, gaveup_seen;
    } res;
};

// either mode that runs the per-env forms of the table-driven step kernels is on
static inline bool qg_sim_per_env(const qg_sim *s) { return s->dyn || s->xfrc; }
// the literal-constant kernel variants run: the compiled-in robot, and no per-env mode
static inline bool qg_sim_baked(const qg_sim *s) { return s->model_baked && !qg_sim_per_env(s); }
// The refusal of what the per-env modes do not cover; `fmt` takes the mode's name and the call that ends it.
static inline int qg_refuse_per_env(const qg_sim *s, const char *fmt) {
    if (s->dyn) return fail(QG_ERR_ARG, fmt, "per-env dynamics", "qg_clear_dynamics");
    if (s->xfrc) return fail(QG_ERR_ARG, fmt, "external wrenches", "qg_clear_xfrc");
    return QG_OK;
}
// hinge jitter of the envs a step auto-resets: a launch of its own behind every step
static inline bool qg_jitter_at_reset(const qg_sim *s) { return s->task.auto_reset && (s->task.reset_flags & QG_RESET_JOINT_JITTER); }

// ---- the core (qg_capi.hip) ----------------------------------------------------------------------------------------------------------
// the resident kernel hands the state back, then whatever is in flight on any stream -- a caller's included -- has run
int qg_retire_and_sync(qg_sim *s);
// a device-pointer call has been enqueued on `stream`: what the next host-pointer call has to wait for
void qg_note_caller_stream(qg_sim *s, hipStream_t stream);
// the mapping AUTO resolves to for this handle, and whether its step kernel carries the fused observation pack (KPoLaunch)
int qg_effective_mapping(const qg_sim *s);
bool qg_po_fusable(const qg_sim *s);
// One env-step enqueued on `stream`.  `walk` != NULL: the fused walking launch (the task layer folded into the step kernel);
// `po` != NULL (with `walk`): the partially observable observation pack fused in as well.
int qg_launch_step(qg_sim *s, const float *d_actions, float *d_obs, float *d_reward, uint8_t *d_done, float *d_comps, float *d_packed,
                   hipStream_t stream, const KWalkLaunch *walk = nullptr, const KPoLaunch *po = nullptr);
// src [w][n] -> dst [n][w] on the library's stream (the state's layout into the caller's), and back
int qg_transpose_out_launch(qg_sim *s, const float *src, float *dst, int w);
int qg_transpose_in_launch(qg_sim *s, const float *src, float *dst, int w);

// ---- many env-steps per launch (qg_sim_multi.hip) ---------------------------------------------------------------------------------------
// the resident kernel stores the state it holds in registers and leaves (no-op while none is launched); its mailbox released
int qg_resident_retire(qg_sim *s);
void qg_resident_free(qg_sim *s);
// the handle can run the sequence / resident forms of the one-link-per-lane kernel; else the refusal, in `who`'s name
int qg_multi_step_usable(const qg_sim *s, const char *who);

// ---- the host-pointer path (qg_sim_host.hip) ----------------------------------------------------------------------------------------------
// One host-pointer step: the actions in through the page-locked arena's first bytes, `step` enqueues the device-pointer step from
// `d_actions` on the library's stream, the four outputs (obs, reward, done, components: the caller's array, its device source, its
// size) -- and for qg_step_mirror the state snapshot -- come back through the arena behind the actions, with ONE synchronisation.
struct PinOut { void *user; size_t off, bytes; };
struct HostOut { void *user; const void *dev; size_t bytes; };
struct StateDst { float *qpos, *qvel, *act, *ctrl; int32_t *nstep; };
struct HostStep { PinOut o[4], state[5]; };
// up to the actions' transfer / from the outputs' transfers on
int qg_host_step_begin(qg_sim *s, const float *actions, float *d_actions, const HostOut (&out)[4], const StateDst *state, HostStep &h);
int qg_host_step_end(qg_sim *s, const HostOut (&out)[4], const StateDst *state, const HostStep &h);
template <class Step>
static int host_step(qg_sim *s, const float *actions, float *d_actions, const HostOut (&out)[4], Step step, const StateDst *state = nullptr) {
    HostStep h;
    int rc = qg_host_step_begin(s, actions, d_actions, out, state, h);
    if (rc == QG_OK) rc = step();
    return rc == QG_OK ? qg_host_step_end(s, out, state, h) : rc;
}

// ---- the walking layer (qg_walk.hip), read by the observation pack bound to it (qg_po.hip) -------------------------------------------
struct qg_walk {
    qg_sim *sim;
    int32_t saved_use_flip, saved_track_ctrl, bound;     // what qg_walk_create changed on the sim; restored by qg_walk_destroy
    qg_walk_params params;
    KWalkParams kp;
    KWalkState st;
    QgDevMem mem;
    float *d_obs, *d_reward, *d_comps, *d_actions, *d_tmp;
    uint8_t *d_done;
    size_t ring_slots, summary_blocks;      // allocated extent of the estimator's ring (whole blocks) and of its block summaries
    struct qg_cmdcur *cmdcur;               // the command curriculum bound to this layer (qg_cmdcur.hip), or NULL: while one is bound
                                            // the in-kernel sampler, a second curriculum and qg_walk_destroy are refused
};
// the walking env-step is one launch with the task layer fused into the step kernel (every mapping but an explicit LANE request)
bool qg_walk_fused(const qg_sim *s);
// pre + physics + post.  The commands of auto-reset envs are redrawn by the caller AFTER everything that still reads the old
// ones (the partially observable pack) has been launched.
int qg_walk_step_core(qg_walk *w, const float *actions, float *obs, float *reward, uint8_t *done, float *components, void *stream,
                      bool po_follows, const KPoLaunch *po_fused = nullptr);

// ---- task-layer snapshot / restore (checkpoint; qg_walk.hip) ----------------------------------------------------
// One opaque blob per layer: a header that pins what the bytes mean (layer, library layout version, n_envs, window) followed by the
// layer's device arrays in declaration order, byte for byte.  Restoring a blob into a layer of the same shape reproduces every later
// step bit for bit (tests/test_walking_gpu.py::test_task_state_snapshot_restores_bit_identical_rollouts).
struct QgField { void *ptr; size_t bytes; };
#define QG_MAX_FIELDS 32
int64_t qg_blob_bytes(const QgField *f, int k);
int qg_blob_out(qg_sim *s, uint32_t magic, int32_t window, const QgField *f, int k, void *blob);
int qg_blob_in(qg_sim *s, uint32_t magic, int32_t window, const QgField *f, int k, const void *blob, const char *who);
