// qg_device.h -- constant tables and launch parameters shared by the host side
// of the C ABI and the gfx950 kernels (single precision, kernarg-resident).
#pragma once
#include <stdint.h>

#define QGK_NLINK 12       // fema / shin / foot x 4 legs
#define QGK_CP_FRAME 12    // contact sample points on the FRAME
#define QGK_CP_LINK 8      // ... on every leg link
#define QGK_WAVE 64
// envs per wave of the step kernels' work mappings (the grid predicates of qg_step_launch.h and AUTO's boundaries are in these units)
#define QGK_LINK_ENVS 4     // one link per lane (qg_kernel_link.hip), in workgroups of QGK_LINK_WAVES waves
#define QGK_LINK_WAVES 4
#define QGK_QUAD_ENVS 16    // one leg per lane (qg_kernel_quad.hip)
#define QGK_PAIR_ENVS 32    // two legs per lane (qg_kernel_pair.hip)

// One leg link and the hinge that drives it (quadruped.xml:71-141, joint defaults :9,24-37,
// servo defaults :10-37).  All hinge axes are the link's local z (quadruped.xml:9), which the
// host side verifies before building this table.
struct KLink {
    float pos[3];       // link frame origin in the parent frame
    float Q[9];         // link frame orientation in the parent frame, row-major rotation matrix
    float mass;
    float ipos[3];      // centre of mass, link frame
    float inertia[6];   // xx yy zz xy xz yz about the COM, link axes
    float cp[QGK_CP_LINK][3];
    // hinge
    float ref, lo, hi, damping, armature;
    // position servo
    float kp, kv, gear, ctrl_lo, ctrl_hi, force_lo, force_hi, act_decay;  // act_decay = 1 - exp(-h/timeconst)
};

struct KModel {
    float h;            // timestep
    float g[3];         // gravity, world
    // FRAME rigid inertia about its own origin, in its own axes
    float m0, h0[3], I0[6];
    float free_damping, free_armature;
    float cp0[QGK_CP_FRAME][3];
    float contact_k, contact_c, contact_margin, contact_mu, contact_inv_ramp;
    float limit_k, limit_b, limit_inv_ramp;
    float qpos0[19];
    KLink link[QGK_NLINK];
};

// Per-env dynamics (qg_set_dynamics_range / qg_set_dynamics): QG_NDYN f32 columns per env in HBM, field-major, env-minor ([11][n],
// the state's layout).  The per-env-dynamics variants of the generic step kernels get a KModelDyn as their model pointer: the shared
// tables followed by the rows' address -- the kernel arguments (and so the existing variants' code) stay as they are.
#define QGK_NDYN 11
// External wrenches (qg_set_xfrc / qg_set_push): QG_NBODY x 6 f32 per env, env-major ([n][13][6], the ABI's layout: the device form
// is a plain copy on the caller's stream, and the six numbers a lane reads are contiguous -- three 8-byte loads, a wave's loads one
// contiguous range).  The push schedule draws a horizontal force on the FRAME per (env, episode, window) with no per-env state.
#define QGK_NXFRC 6
#define QGK_NBODY 13
struct KPush {
    int32_t interval, duration;       // env-steps per window, env-steps a push lasts (interval 0: no schedule)
    float probability, force_min, force_max;
};
struct KModelDyn {
    KModel m;
    const float *rows;        // [QGK_NDYN][n]
    const float *xfrc;        // [n][13][6] world-frame force and torque at each body's centre of mass, or NULL: wrench mode off
    float com0[3];            // the FRAME's centre of mass, body frame (the shared model's body_ipos[0]: a payload does not move it)
    KPush push;
};
// what one lane holds of its env's row: the replaced contact constants, the servo / hinge scales, the FRAME's rigid inertia about its
// origin with the payload added
struct KDyn {
    float mu, kc, cc;                         // contact friction, stiffness, damping
    float kp, kv, force, damping;             // scales of act_kp, act_kv, act_forcerange, jnt_damping
    float m0, h0[3], I0[6];
};
// the range QG_RESET_DYNAMICS draws an env's row from (qg_dyn_draw_kernel)
struct KDynRange { float lo[QGK_NDYN], hi[QGK_NDYN]; };

struct KTask {
    int32_t frame_skip;
    int32_t limit_substeps;   // substep count at which data.time >= max_time (f64 accumulation), or INT32_MAX
    int32_t use_fall;
    float fall_height;
    int32_t use_flip;         // body z axis of the (lagged) sensor pack below the horizon terminates
    float w_forward, w_ctrl, alive_bonus;
    int32_t obs_mode;         // 0: 33 sensors, 1: 21-value IMU pack
    int32_t sensor_lag;
    int32_t auto_reset;
    uint32_t reset_flags;
    float default_ctrl[12];
    float reset_joint_jitter;
};

// Struct-of-arrays state in HBM: field-major, env-minor, so that lane i of a wave
// touches address base + i*4 for every field (one 256-byte segment per wave and field).
struct KState {
    float *qpos;      // [19][n]
    float *qvel;      // [18][n]
    float *act;       // [12][n]
    float *ctrl;      // [12][n]  last env-clipped action (data.ctrl); written only when track_ctrl
    int32_t *nstep;   // [n]
    int32_t *episode; // [n]   resets this env has gone through: the counter of its reset random stream (graph-replay safe)
};

struct KStepArgs {
    KState st;
    int32_t n;
    int32_t track_ctrl;
    const float *actions;     // [n][12]
    float *obs;               // [n][obs_dim]   (separate outputs) or NULL
    float *reward;            // [n]
    uint8_t *done;            // [n]
    float *comps;             // [n][3] or NULL
    float *packed;            // [n][obs_dim+2] or NULL
    uint64_t seed;            // reset stream
    uint64_t env_index_base;
};

// The mailbox of the many-env-steps-per-launch forms of the one-link-per-lane kernel (qg_kernel_resident.hip) and the status words
// its kernels report to the host.
#define QG_RES_SHARDS 32            // arrival counters, one 128-byte line each; wave w of the grid arrives at shard w % 32
#define QG_RES_RUNNING 1ull         // hstat[0]
#define QG_RES_EXIT_STOP 2ull       // retired on request (qg_resident_stop, or any entry point that needs the state in memory)
#define QG_RES_EXIT_IDLE 3ull       // retired itself: no ring within idle_ticks
#define QG_RES_RETIRING 4ull        // no ring for idle_ticks / 2: the kernel still takes rings, and leaves at idle_ticks if none comes.  The
                                    // host does not ring a kernel in this state (it retires it and launches again): a ring it enqueues
                                    // after seeing RUNNING therefore has idle_ticks / 2 to reach the GPU before the door can shut

struct KResident {
    unsigned long long *door;       // device: env-steps rung so far | QG_DOOR_STOP
    unsigned long long *done;       // device: [QG_RES_SHARDS] arrival counters (index 16 s), cumulative env-steps x waves
    unsigned long long *completed;  // device: env-steps the previous launches have completed (where this launch starts)
    unsigned long long *hstat;      // page-locked host memory: [0] QG_RES_*, [1] env-steps completed at exit, [2] env-steps of refused
                                    // rings, [3] rings that gave up waiting
    const float *actions;           // [slots][n][12]
    float *packed;                  // [slots][n][D + 2]
    int32_t slots;
    int32_t count;                  // DOOR = false: env-steps of this launch
    uint32_t idle_ticks;            // DOOR: give up waiting for a ring after this many ticks of the 100 MHz clock
    uint32_t ring_ticks;            // ring kernel: give up after this long without an arrival
};

#ifdef __HIPCC__
// counter-based uniform in [0,1) with 24 random bits (same stream as the oracle's qgo_uniform)
__device__ __forceinline__ uint64_t mix64(uint64_t x) {
    x ^= x >> 30; x *= 0xBF58476D1CE4E5B9ull;
    x ^= x >> 27; x *= 0x94D049BB133111EBull;
    x ^= x >> 31;
    return x;
}
__device__ __forceinline__ float uniform24(uint64_t seed, uint64_t env_index, uint64_t counter) {
    uint64_t x = seed + 0x9E3779B97F4A7C15ull * (env_index + 1) + 0xD1B54A32D192ED03ull * (counter + 1);
    x = mix64(mix64(x));
    return (float)(uint32_t)(x >> 40) * (1.0f / 16777216.0f);
}
// independent streams of the same (seed, env, episode) key: 0 = reset yaw, 1..12 = hinge jitter, 13..15 = walking command
#define QG_STREAM_HINGE 1u
#define QG_STREAM_COMMAND 13u
__device__ __forceinline__ float uniform24s(uint64_t seed, uint64_t env_index, uint64_t counter, uint32_t stream) {
    return uniform24(seed + 0xA0761D6478BD642Full * (uint64_t)stream, env_index, counter);
}

// Hand-off through LDS between the lanes of ONE wave (a tile no other wave touches): the wave's LDS operations execute in order, so
// no s_barrier is needed -- in a four-wave workgroup that would also make every wave wait for the slowest of the four -- only the
// compiler has to be told that other lanes read what this lane wrote.
__device__ __forceinline__ void wave_sync() {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}
#endif
