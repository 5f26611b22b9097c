/* quadgym.h -- C ABI of the MI355X-native batched quadruped simulator.
 *
 * This is the drop-in boundary for the one hot path of antopio26/quadruped-gym:
 * QuadrupedEnv.step() / reset() (src/envs/quadruped.py:115-182) and the four
 * call sites where that file hands the arithmetic to the third-party `mujoco`
 * package (src/envs/quadruped.py:59,60,120,165).  The reference has no FFI of
 * its own (it is plain Python over the mujoco bindings); each entry point below
 * names the reference call it replaces.  Bindings: ctypes stub in INTEGRATION.md.
 *
 * Conventions: extern "C", opaque handle, int status (0 = ok, <0 = error, text
 * from qg_last_error()), no exceptions cross the boundary, caller owns every
 * buffer it passes, the library owns the per-env device state.  One handle is
 * bound to one GPU; calls on a handle are not re-entrant.  There is NO CPU
 * backend: every compute entry point fails with QG_ERR_DEVICE when no HIP device
 * is usable.
 *
 * Ordering contract.  The *_device entry points (qg_step_device, qg_step_device_packed,
 * qg_walk_step_device, qg_po_step_device) enqueue on the caller's stream and return at once;
 * consecutive calls on ONE stream are ordered by that stream, calls on different streams are the
 * caller's to order.  Every other entry point that touches the per-env state (qg_reset,
 * qg_walk_reset, qg_po_reset, the host-pointer qg_step / qg_walk_step / qg_po_step,
 * qg_get_state / qg_set_state, the task-layer snapshots, the command and estimate accessors, the destroy calls) first waits
 * for ALL work on the handle's device (hipDeviceSynchronize), runs on the library's own stream and
 * returns when it has completed -- it can therefore follow device-pointer steps on any stream
 * without further synchronisation, and must not be called while a stream is being captured.
 * (The host-pointer steps skip that device-wide wait when no device-pointer call of this handle
 * has gone to a caller's stream since the last one: their own stream is synchronised at the end
 * of every call, so there is nothing to wait for.  Once a device-pointer step of the handle has
 * been captured into a hipGraph the wait is taken on every host-pointer call: replays enqueue
 * steps the library does not see.  Device-pointer steps on the legacy NULL stream must not overlap
 * another stream's capture: the library cannot ask the NULL stream whether it is being captured.)
 *
 * Layouts at the boundary (row-major, env-major -- what NumPy / torch hand over):
 *   actions  [n_envs][12] f32      obs   [n_envs][obs_dim] f32
 *   reward   [n_envs] f32          done  [n_envs] u8
 *   reward_components [n_envs][3] f32  (forward, control_cost, alive)
 *   packed   [n_envs][obs_dim + 2] f32 (obs, reward, done as 0/1) -- one buffer
 *            for the per-step RCCL gather.
 * State arrays (qg_get_state / qg_set_state): qpos [n][19], qvel [n][18],
 * act [n][12], ctrl [n][12] f32 and nstep [n] i32 (physics substeps since
 * reset; data.time = nstep * timestep).
 */
#ifndef QUADGYM_H
#define QUADGYM_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define QG_NBODY 13      /* FRAME + 4 x (fema, shin, foot)      quadruped.xml:62-142 */
#define QG_NLEG 4
#define QG_NJNT 12       /* hinge joints = actuators            quadruped.xml:156-172 */
#define QG_NQ 19         /* 3 pos + 4 quat + 12 hinge */
#define QG_NV 18
#define QG_NU 12
#define QG_NSENSOR 33    /* model.nsensordata                   quadruped.xml:174-217 */
#define QG_MAXCP 12      /* contact sample points per body (table width) */
#define QG_NREWARD 3

/* status codes */
#define QG_OK 0
#define QG_ERR_ARG (-1)
#define QG_ERR_DEVICE (-2)
#define QG_ERR_ALLOC (-3)
#define QG_ERR_LAUNCH (-4)

/* The done vector of the device-side layers (qg_norm, qg_rollout, qg_perturb, qg_contact, qg_gait): a device [n] at done_stride elements
 * (>= 1), of the type done_kind names, nullable where the entry point says so.  Non-zero is done. */
#define QG_DONE_U8 0     /* uint8 (the walking and partially observable envs' buffer; torch.bool as well) */
#define QG_DONE_F32 1    /* f32 (the last column of the plain env's packed row) */

/* observation packs (qg_task.obs_mode) */
#define QG_OBS_FULL 0    /* the 33-value sensordata of quadruped.py:141-143 */
#define QG_OBS_IMU 1     /* jointpos 12 + accel 3 + gyro 3 + velocimeter 3 = 21 (BASELINE config 5) */

/* work mappings of the step kernel (qg_set_mapping) */
#define QG_MAP_AUTO 0    /* the measured optimum per size: LINK up to 4096 envs; above, for the compiled-in robot QUAD up to 16384 and
                            for 32769..57343, PAIR for 16385..32768 and >= 57344; QUAD for any other model numbers */
#define QG_MAP_LANE 1    /* one environment per wavefront lane (64 envs per wave), any model numbers */
#define QG_MAP_QUAD 2    /* one leg per lane, four lanes per environment (16 envs per wave), any model numbers */
#define QG_MAP_PAIR 3    /* two legs per lane as packed FP32 pairs, two lanes per environment (32 envs per wave);
                            compiled-in robot only: qg_set_mapping refuses it for other model numbers */
#define QG_MAP_LINK 4    /* one link per lane, sixteen lanes per environment (4 envs per wave), any model numbers; the reference's
                            lagged sensors only (otherwise the request falls back to QUAD) */

/* qg_reset flags */
#define QG_RESET_RANDOM_YAW 1u   /* walking_quad.py:68-75: qpos[3:7] = [cos a/2, 0, 0, sin a/2], a ~ U(0, 2 pi) */
#define QG_RESET_JOINT_JITTER 2u /* hinge j starts at qpos0 + reset_joint_jitter * U(-1, 1), clamped to its range (the reference's open
                                    "RANDOMIZE ENVIRONMENT - Starting pose, joints" item, TODO.md:8; SURVEY config 3 option) */
#define QG_RESET_DYNAMICS 4u     /* draw a new per-env dynamics row (qg_set_dynamics_range) for the envs reset; refused without a range */

/* Robot constants: what mujoco.MjModel.from_xml_path (quadruped.py:59) compiles
 * out of scene.xml.  Topology is fixed (body 0 = FRAME with the free joint, body
 * 1+3k+{0,1,2} = fema/shin/foot of leg k, joint j drives body j+1); numbers are
 * data.  Units SI, angles in radians, quaternions (w,x,y,z). */
typedef struct qg_model {
    double timestep;                       /* 0.002 (engine default, quadruped.xml:4 sets none) */
    double gravity[3];
    int32_t body_parent[QG_NBODY];         /* -1 for FRAME */
    double body_pos[QG_NBODY][3];          /* body frame in the parent body frame */
    double body_quat[QG_NBODY][4];
    double body_mass[QG_NBODY];
    double body_ipos[QG_NBODY][3];         /* centre of mass in the body frame */
    double body_inertia[QG_NBODY][6];      /* xx yy zz xy xz yz about the COM, body axes */
    double jnt_axis[QG_NJNT][3];           /* in the child body frame; anchor = body origin */
    double jnt_ref[QG_NJNT];               /* qpos0 of the hinge; rotation applied = qpos - ref */
    double jnt_range[QG_NJNT][2];
    double jnt_damping[QG_NJNT];
    double jnt_armature[QG_NJNT];
    double free_damping;                   /* applies to all 6 base DoFs (childclass, quadruped.xml:9,62-63) */
    double free_armature;
    double act_kp[QG_NU], act_kv[QG_NU], act_gear[QG_NU], act_timeconst[QG_NU];
    double act_ctrlrange[QG_NU][2], act_forcerange[QG_NU][2];
    double limit_stiffness, limit_damping; /* soft joint limits (N m/rad, N m s/rad) */
    double limit_ramp;                     /* limit damping ramps in linearly over this penetration (rad) */
    int32_t ncp[QG_NBODY];                 /* must be 12 for FRAME, 8 for every link */
    double cp[QG_NBODY][QG_MAXCP][3];      /* contact sample points, body frame */
    double contact_stiffness;              /* N/m per sample point */
    double contact_damping;                /* N s/m per body in contact (implicit) */
    double contact_margin;                 /* contact starts at this height */
    double contact_friction;               /* Coulomb mu */
    double contact_ramp;                   /* contact damping ramps in linearly over this summed penetration (m) */
    double qpos0[QG_NQ];                   /* what mj_resetData restores (quadruped.py:120) */
} qg_model;

/* Task constants: QuadrupedEnv's constructor arguments and the README reward /
 * termination set (quadruped.py:40-52,97-100,149-151; README.md:64-90). */
typedef struct qg_task {
    int32_t frame_skip;        /* quadruped.py:44, default 4 */
    double max_time;           /* quadruped.py:43, default 10.0; reported as `terminated` */
    int32_t use_time_limit;    /* use_default_termination, quadruped.py:52,99-100 */
    int32_t use_fall;          /* README.md:86-89 */
    double fall_height;        /* README literal 0.2; the base starts at 0.13 (quadruped.xml:62) */
    int32_t use_flip;          /* walking_quad.py:156-166: body z axis (sensordata[29]) < 0 terminates */
    double w_forward;          /* reward = w_forward*qvel[0] + w_ctrl*sum(ctrl^2) + alive; README.md:65-72 */
    double w_ctrl;             /* -0.1 */
    double alive_bonus;        /* 1.0 */
    int32_t obs_mode;          /* QG_OBS_FULL | QG_OBS_IMU */
    int32_t sensor_lag;        /* 1 = sensors describe the start of the last substep (mj_step order) */
    int32_t auto_reset;        /* 1 = envs that finish are reset inside the step (VecEnv semantics) */
    uint32_t reset_flags;      /* QG_RESET_* applied by auto-reset */
    double default_ctrl[QG_NU];/* quadruped.py:124: [0, 0, -0.5] * 4 */
    double reset_joint_jitter; /* [rad] half-width of the QG_RESET_JOINT_JITTER draw, default 0.1 */
} qg_task;

typedef struct qg_sim qg_sim;  /* opaque */

const char *qg_version(void);
/* 16 hex digits: hash of the sources this library was built from (kernels, C ABI, model tables).  Measurement tooling stamps
 * committed profiles with it; bench.py flags a roofline entry that was measured on other sources (roofline.profile_stale). */
const char *qg_build_id(void);
const char *qg_last_error(void);
/* The batch size at the top of the stair `n_envs` stands on: the step time is a staircase in the batch size (4096 / 16 384 / every
 * further 32 768 envs on the 1024 SIMDs of an MI355X -- one wave per SIMD of the kernel AUTO picks), so this many envs cost no more
 * per step than `n_envs` do.  4097 envs cost 55 % more per step than 4096.  device_id < 0: an MI355X. */
int32_t qg_recommended_batch(int32_t n_envs, int32_t device_id);
/* PCI bus id ("0000:05:00.0") of HIP device `device_id` into out[len >= 16] -- what bench.py's N > 1 line lists per rank, so that
 * "did RCCL see N ranks on N distinct GPUs" can be read off the line. */
int qg_device_pci_bus_id(int32_t device_id, char *out, int32_t len);

/* Fill with the constants compiled from the reference model (include/qg_model_data.h). */
int qg_default_model(qg_model *out);
int qg_default_task(qg_task *out);

/* Substep count at which `data.time >= max_time` first holds when time is
 * accumulated as the reference's engine does it (f64, time += timestep per
 * substep); quadruped.py:149-151. */
int64_t qg_time_limit_substeps(double timestep, double max_time);

/* Replaces MjModel.from_xml_path + MjData (quadruped.py:59-60).  `env_index_base`
 * is the global index of this handle's env 0 (shards of one batch get disjoint
 * ranges so per-env random streams do not depend on the sharding).  Random draws at reset come from a counter-based
 * stream keyed by (seed, global env index, number of resets that env has gone through). */
int qg_create(int32_t n_envs, int32_t device_id, const qg_model *model, const qg_task *task,
              uint64_t env_index_base, qg_sim **out);
int qg_destroy(qg_sim *sim);
int qg_num_envs(const qg_sim *sim);
int qg_obs_dim(const qg_sim *sim);

/* Replaces QuadrupedEnv.reset (quadruped.py:115-139): mj_resetData, time = 0,
 * ctrl = default.  mask == NULL resets every env, else only mask[i] != 0
 * (host pointer, n_envs bytes).  The first observation is all zeros, as in the
 * reference (no mj_forward after mj_resetData).  `seed` keys the reset random
 * streams (yaw, hinge jitter, commands) of every env of the batch, auto-resets
 * included: it is adopted by a whole-batch reset only (mask == NULL); a masked
 * reset ignores it and draws from the streams already in force. */
int qg_reset(qg_sim *sim, const uint8_t *mask, uint64_t seed, uint32_t flags);

/* Replaces QuadrupedEnv.step (quadruped.py:153-182) for the whole batch: clip to
 * [-1, 1], frame_skip x {ctrl = action; mj_step}, sensor pack, rewards,
 * terminations.  Host-pointer form (copies in and out, synchronous). */
int qg_step(qg_sim *sim, const float *actions, float *obs, float *reward, uint8_t *done,
            float *reward_components /* nullable */);

/* Device-pointer forms: every pointer is device memory on the handle's GPU,
 * `stream` is a hipStream_t (NULL = default stream); asynchronous. */
int qg_step_device(qg_sim *sim, const float *actions, float *obs, float *reward, uint8_t *done,
                   float *reward_components /* nullable */, void *stream);
int qg_step_device_packed(qg_sim *sim, const float *actions, float *packed, void *stream);

/* Snapshot / restore of data.qpos, qvel, act, ctrl and the substep counter
 * (host pointers; any may be NULL).  Used by the parity tests and checkpoints. */
int qg_get_state(qg_sim *sim, float *qpos, float *qvel, float *act, float *ctrl, int32_t *nstep);
/* qg_step followed by qg_get_state in ONE call and one synchronisation (any of the state pointers may be NULL): what an env that
 * mirrors the state on the host after every step needs -- the reference's `env.data`, which user reward / termination callables
 * read (quadruped.py:170-178). */
int qg_step_mirror(qg_sim *sim, const float *actions, float *obs, float *reward, uint8_t *done, float *reward_components, float *qpos,
                   float *qvel, float *act, float *ctrl, int32_t *nstep);
int qg_set_state(qg_sim *sim, const float *qpos, const float *qvel, const float *act, const float *ctrl,
                 const int32_t *nstep);

/* Time the step kernel alone: `iters` launches back to back on the handle's own
 * stream bracketed by HIP events on that stream; returns the mean milliseconds
 * per launch in *ms_per_launch.  State advances `iters` env-steps. */
int qg_time_step_kernel(qg_sim *sim, const float *d_actions, float *d_packed, int32_t iters, float *ms_per_launch);

/* Replace the task constants of a live handle -- what assigning env.reward_fns / env.termination_fns / env.max_time after
 * construction does in the reference (README.md:74-89): reward weights, fall / flip / time-limit terminations, auto-reset
 * and its flags, frame_skip.  obs_mode is fixed at qg_create.  Refused while a walking task layer is bound, and while the
 * resident step mode is on for a task the resident kernel cannot run (unlagged sensors, hinge jitter at auto-reset): the
 * handle keeps its task.  Takes effect from the next step; waits for steps in flight. */
int qg_set_task(qg_sim *sim, const qg_task *task);
int qg_get_task(const qg_sim *sim, qg_task *out);

/* data.ctrl (the last env-clipped action, quadruped.py:164) is written back each step only
 * while this is on (default on; bulk-throughput callers switch it off). */
int qg_set_track_ctrl(qg_sim *sim, int32_t on);
/* Development builds only (make CXXFLAGS+=-DQG_PHASE_TIMES; tools/phase_times.py): the 100 MHz clock stamps the first wave of the last
 * one-link-per-lane launch took at its phase marks.  Production builds carry no such code and return QG_ERR_ARG. */
int qg_debug_phase_times(uint64_t out[16]);
/* The step-kernel instantiation the handle's latest step launch enqueued, every template argument written out (defaults included,
 * bool as 0/1), e.g. "qg_step_kernel_quad<2,1,1,4,0,1,0>"; the many-env-steps forms are named too ("qg_step_kernel_link_multi<1,1>").
 * QG_ERR_ARG before the first step, or when `len` cannot hold the name and its terminating zero.  Host-side bookkeeping only. */
int32_t qg_debug_last_step_kernel(const qg_sim *sim, char *buf, int32_t len);

/* 1 when the handle's model equals the compiled-in default (include/qg_model_data.h) and the
 * kernel variant with those constants baked into the instruction stream runs; 0 for any other
 * numbers (generic variant, tables read from device memory). */
int qg_uses_baked_model(const qg_sim *sim);

/* Choose how environments map onto wavefront lanes (QG_MAP_*); results agree to rounding.
 * qg_get_mapping returns the mapping the next step will actually use (LANE, QUAD or PAIR). */
int qg_set_mapping(qg_sim *sim, int32_t mapping);
int qg_get_mapping(const qg_sim *sim);

/* ---- many env-steps per launch (round 4; packed rows, no task layer) -----------------------------------------------------------
 * The reference keeps an env's state in MjData across steps (quadruped.py:163-165: the hot loop re-reads nothing); the per-launch
 * step kernel re-loads and stores it around every env-step.  Two forms keep it in registers instead:
 *
 * qg_step_device_seq: ONE launch runs `count` env-steps on actions[count][n_envs][12] and writes packed[count][n_envs][obs_dim + 2]
 * (device pointers, `stream` as for qg_step_device) -- open-loop sequences (action repeat, a planned sequence, K-step graphs).
 * Results are bit-identical to `count` calls of qg_step_device_packed.  Every mapping AUTO picks has its one-launch form (one link
 * per lane up to 4096 envs, one leg per lane, two legs per lane); where none applies (the one-env-per-lane mapping, un-lagged
 * sensors, hinge jitter at auto-reset, explicit mapping requests on small grids) the call IS those `count` launches, so it means
 * the same for every handle.  The resident form below exists for the one-link-per-lane mapping (<= 4096 envs) only.
 *
 * The RESIDENT form (opt-in): qg_resident_start launches the step kernel once on the library's own stream; it stays on the GPU and
 * is handed each env-step through a mailbox in device memory -- `slots` action buffers [n_envs][12] and `slots` output buffers
 * [n_envs][obs_dim + 2] (qg_resident_buffers), env-step i of the resident sequence (counted from qg_resident_start) uses slot
 * i % slots.  qg_resident_step_device(count, stream) enqueues a RING on the caller's stream: it makes the next `count` env-steps
 * runnable and holds the stream until their rows are in memory -- a policy on the same stream stays in the loop (read the rows,
 * write the next slot's actions, ring); `count` > 1 lets the kernel run ahead through slots the caller filled beforehand.
 * Nothing in it waits without a deadline: a kernel that is not rung for `idle_timeout_us` (0 = 2000; 50 .. 100000) stores the
 * state and leaves; the next qg_resident_step_device (or qg_resident_ensure, for graph replays) launches it again.  After HALF the
 * time-out without a ring the kernel tells the host that it is about to leave (it still takes rings); the host then never rings it
 * but retires it and launches again (tens of microseconds, synchronous) -- so a ring enqueued by qg_resident_step_device has half
 * the time-out to reach the GPU before the door can shut on it.  A ring that does meet a retired kernel (a stream backlog longer
 * than that, a replayed graph without qg_resident_ensure) does NOT run its steps; the next resident call returns QG_ERR_LAUNCH and
 * says how many (the state is that of the last executed step).  Every entry point that needs the state in memory (reset, get / set_state, set_task, the per-launch
 * steps, destroy) first retires the kernel; qg_resident_stop retires it and frees the mailbox.
 * Measured: closed-loop rings cost MORE per env-step than a kernel launch; the form pays for run-ahead only. */
int qg_step_device_seq(qg_sim *sim, const float *actions, float *packed, int32_t count, void *stream);
/* actions / packed: the mailbox's slot buffers, [slots][n_envs][12] and [slots][n_envs][obs_dim + 2] f32 in device memory that the
 * caller owns and keeps alive until qg_resident_stop -- or both NULL: the library allocates them (qg_resident_buffers). */
int qg_resident_start(qg_sim *sim, int32_t slots, int32_t idle_timeout_us, float *actions, float *packed);
int qg_resident_stop(qg_sim *sim);
int qg_resident_buffers(qg_sim *sim, float **actions, float **packed, int32_t *slots);
int qg_resident_step_device(qg_sim *sim, int32_t count, void *stream);
/* Launch the resident kernel again if it has retired (idle): call before replaying a hipGraph that holds captured rings. */
int qg_resident_ensure(qg_sim *sim);
/* No synchronisation: env-steps rung through the API, whether the kernel is on the GPU, the env-steps completed when it last left,
 * env-steps of rings that met a retired kernel (cumulative).  Any output may be NULL. */
int qg_resident_status(qg_sim *sim, int64_t *rung, int32_t *running, int64_t *completed_at_exit, int64_t *not_executed);

/* ---- native per-step exchange over RCCL (opt-in) --------------------------------------------------------------
 * Env batches shard across the GPUs of a node, one process per GPU, no exchange inside the physics; once per env-step
 * the packed [n_envs][obs_dim + 2] rows are gathered to `root` over xGMI.  These entry points issue that gather from C
 * (RCCL loaded with dlopen, no link-time dependency) so that the host cost per step is a few microseconds instead of
 * torch.distributed's ~30; the unique id is created on one rank and handed to the others by whatever channel the
 * caller has (bench.py broadcasts it through torch.distributed).  Validated with a 1-rank communicator only so far. */
#define QG_COMM_ID_BYTES 128
typedef struct qg_comm qg_comm;
int qg_comm_unique_id(uint8_t id[QG_COMM_ID_BYTES]);
int qg_comm_create(qg_sim *sim, int32_t rank, int32_t world, const uint8_t id[QG_COMM_ID_BYTES], qg_comm **out);
int qg_comm_destroy(qg_comm *comm);
/* `steps` env-steps with one gather each, double-buffered and overlapped: step k reads actions[k % n_actions] (device
 * pointers, host array of n_actions pointers), writes packed[k & 1] and gathers it into gathered[k & 1]
 * ([world][n_envs][obs_dim + 2] on the root; ignored elsewhere).  Returns when everything is enqueued. */
int qg_comm_rollout(qg_comm *comm, const float *const *actions, int32_t n_actions, float *const packed[2],
                    float *const gathered[2], int32_t steps, int32_t root);
/* Block the host until the communicator's streams are idle. */
int qg_comm_synchronize(qg_comm *comm);

/* ---- walking task layer ----------------------------------------------
 * What WalkingQuadrupedEnv adds around QuadrupedEnv.step() (src/envs/walking_quad.py): the velocity /
 * heading command (src/envs/control_inputs.py), the settling-time action mask (:142-143), the online
 * frequency / amplitude estimator of the control signal (src/envs/math_utils.py:11-158), the 11-term
 * reward of input_control_reward (:352-428) and the flip termination (:156-166).  A qg_walk is bound to
 * one qg_sim (which must use the 33-value observation) and keeps the per-env task state on the device. */
#define QG_NWALKREWARD 11   /* walking_quad.py:332-351 reward_keys */

typedef struct qg_walk_params {
    double settling_time;            /* walking_quad.py:11,142-143 */
    double joint_centers[QG_NU];     /* :36-39  [0, 0, -0.5] * 4 */
    double ema_alpha, min_freq;      /* :54-59  0.8, 1 Hz (window = ceil(2 / (min_freq * dt))) */
    double control_cost_alpha;       /* :254    0.8 */
    double w[10];                    /* :362-373 weights of the ten value terms, in reward_keys order */
    double w_diff_ideal;             /* :383    -20 */
    double body_height;              /* :369    0.13 */
    double amp_target[QG_NU];        /* :279-285 [1.5, 0.5, 0] * 4 */
    double freq_target[QG_NU];       /* :272-277 [1, 1, 0] * 4 */
    int32_t unit_zero;               /* 0 (default, the reference): unit() of an exactly zero vector is NaN (math_utils.py:7-8) and that
                                        NaN reaches progress_direction_reward_local and the total (walking_quad.py:197-205,422);
                                        1: the direction term is 0 when the local xy velocity or the commanded velocity is exactly
                                        zero.  Why an option: the engine's f64 state practically never holds an exact zero there, this
                                        f32 pipeline with its exact four-fold symmetry does on the first step of EVERY episode, and a
                                        NaN reward poisons a PPO update (train_quadruped.py:132-134) -- INTEGRATION.md section 4 */
} qg_walk_params;

typedef struct qg_walk qg_walk;

int qg_walk_default_params(qg_walk_params *out);
/* Binds the task layer to `sim` (switches its flip termination and data.ctrl tracking on; qg_walk_destroy switches both back
 * to what they were).  One layer per simulator: a second qg_walk_create on the same sim is refused.  The estimator window
 * ceil(2 / (min_freq * timestep * frame_skip)) has no upper bound other than memory (math_utils.py:26-28).  Lifetime: a qg_walk borrows its qg_sim and a qg_po borrows its qg_walk -- destroy them in the order
 * po, walk, sim. */
int qg_walk_create(qg_sim *sim, const qg_walk_params *params, qg_walk **out);
int qg_walk_destroy(qg_walk *walk);
/* control_inputs.py: per-env local velocity (vx, vy) and heading unit vector (cos, sin); host pointers [n][2]. */
int qg_walk_set_commands(qg_walk *walk, const float *velocity_xy, const float *heading_xy);
/* WalkingQuadrupedEnv.reset (walking_quad.py:96-126): resets the robots (as qg_reset) and the per-episode task
 * state; the estimator is NOT reset, as in the reference (:115). */
int qg_walk_reset(qg_walk *walk, const uint8_t *mask, uint64_t seed, uint32_t flags);
/* WalkingQuadrupedEnv.step (walking_quad.py:128-148).  components: [n][11] in reward_keys order, nullable. */
int qg_walk_step(qg_walk *walk, const float *actions, float *obs, float *reward, uint8_t *done, float *components);
int qg_walk_step_device(qg_walk *walk, const float *actions, float *obs, float *reward, uint8_t *done, float *components,
                        void *stream);
/* VelocityHeadingControls.sample(options) (control_inputs.py:74-115) on the device: with a sampler installed every
 * qg_walk_reset and every in-step auto-reset draws a new command for the envs it resets (random_controls,
 * walking_quad.py:121-122), from streams 13..15 of the env's (seed, global env index, episode) key -- the reference
 * draws from the global NumPy RNG, which a batch cannot reproduce.  theta, alpha ~ U(-pi, pi), speed ~ U(min, max)
 * unless the corresponding QG_CMD_FIXED_* bit selects the fixed value.  The new command takes effect after the
 * step's reward and (PO) observation have been produced, as in the reference.  NULL removes the sampler. */
#define QG_CMD_FIXED_HEADING 1u          /* options['fixed_heading_angle'] */
#define QG_CMD_FIXED_VELOCITY_ANGLE 2u   /* options['fixed_velocity_angle'] */
#define QG_CMD_FIXED_SPEED 4u            /* options['fixed_speed'] */
typedef struct qg_command_sampler {
    uint32_t fixed;                      /* QG_CMD_FIXED_* */
    double min_speed, max_speed;         /* defaults 0, 1 */
    double fixed_heading_angle, fixed_velocity_angle, fixed_speed;
} qg_command_sampler;
int qg_walk_set_command_sampler(qg_walk *walk, const qg_command_sampler *sampler);
/* Current commands, host pointers [n][2] each (either may be NULL). */
int qg_walk_get_commands(qg_walk *walk, float *velocity_xy, float *heading_xy);
/* Snapshot of the estimator outputs (f_est, a_est: [n][12], host pointers) and the ideal position ([n][2]). */
int qg_walk_get_estimates(qg_walk *walk, float *f_est, float *a_est, float *ideal_xy);

/* Task-layer snapshot / restore (checkpoint and resume; the reference only resumes the policy,
 * src/train_quadruped.py:114-141, its env state is rebuilt by reset()).  qg_get_state / qg_set_state cover the physics; these cover what
 * the walking layer keeps per env beyond it -- commands, ideal position, previous control and its first cost, the derived-term memory,
 * the whole estimator (ring, block summaries, counters, estimates) -- as ONE opaque blob of qg_walk_state_bytes() bytes (host pointer).
 * The layout is private to the library version and to (n_envs, window); set_state refuses a blob whose header does not match. */
int64_t qg_walk_state_bytes(const qg_walk *walk);
int qg_walk_get_state(qg_walk *walk, void *blob);
int qg_walk_set_state(qg_walk *walk, const void *blob);
/* The simulator's reset streams: per-env episode counters [n] and the batch seed, which key every random draw of a (re)set
 * (random yaw, hinge jitter, commands).  Together with qg_get_state and the blobs a restored run continues bit for bit,
 * auto-resets included.  Either output may be NULL; a NULL `episode` in the setter leaves the counters as they are. */
int qg_get_reset_streams(qg_sim *sim, int32_t *episode, uint64_t *seed);
int qg_set_reset_streams(qg_sim *sim, const int32_t *episode, uint64_t seed);

/* ---- partially observable observation pack ---------------------------------
 * POWalkingQuadrupedEnv (src/envs/po_walking_quad.py:10-90): per step one 26-value frame [gyro 3, accel 3,
 * Madgwick-IMU Euler angles 3, body_vel xy 2, data.ctrl 12, command vx vy theta 3], stacked over obs_window
 * steps (FIFO).  Sits on top of a qg_walk. */
#define QG_PO_FRAME_DIM 26

typedef struct qg_po qg_po;

int qg_po_create(qg_walk *walk, int32_t obs_window, qg_po **out);          /* po_walking_quad.py:10-27 */
int qg_po_destroy(qg_po *po);
int qg_po_obs_dim(const qg_po *po);                                         /* 26 * obs_window */
/* POWalkingQuadrupedEnv.reset (:59-69); obs (nullable, host pointer [n][obs_dim]) receives the stacked reset frames */
int qg_po_reset(qg_po *po, const uint8_t *mask, uint64_t seed, uint32_t flags, float *obs);
/* POWalkingQuadrupedEnv.step (:72-90).  obs: [n][obs_dim]; terminal_obs: nullable, receives the last stacked
 * observation of envs that finished (rows of other envs are left untouched); components: [n][11], nullable.
 * Up to 4096 envs of the built-in robot the whole step is ONE kernel launch (physics, walking task layer,
 * observation pack); `obs` must not alias `actions`: the rows are written from the first instructions of the launch on. */
int qg_po_step(qg_po *po, const float *actions, float *obs, float *reward, uint8_t *done, float *components, float *terminal_obs);
int qg_po_step_device(qg_po *po, const float *actions, float *obs, float *reward, uint8_t *done, float *components,
                      float *terminal_obs, void *stream);
/* Snapshot / restore of the observation pack's own state (orientation estimate, its aliasing flag, the frame ring): as qg_walk_get_state. */
int64_t qg_po_state_bytes(const qg_po *po);
int qg_po_get_state(qg_po *po, void *blob);
int qg_po_set_state(qg_po *po, const void *blob);

/* ---- per-env dynamics randomisation -----------------------------------------------------------------------------------------
 * Every env of a handle runs one qg_model; with this mode on, each env also has a row of QG_NDYN f32 that changes the handle's model
 * for that env alone (the reference's SubprocVecEnv gives each env its own MjModel; its TODO.md:8 "RANDOMIZE ENVIRONMENT ... etc."):
 *   col  name                     effect on the handle's model for this env
 *   0    friction                 contact_friction = value (absolute Coulomb mu)
 *   1    payload_mass             point mass dm (kg, may be negative) rigidly fixed to the FRAME at ...
 *   2-4  payload_pos              ... point p, FRAME body coordinates (m): m0' = m0 + dm, h0' = h0 + dm p, I0' = I0 + dm (|p|^2 E - p p^T)
 *                                 (the FRAME's rigid inertia about its origin)
 *   5    kp_scale                 act_kp[j] x value, all 12 servos
 *   6    kv_scale                 act_kv[j] x value
 *   7    force_scale              both ends of act_forcerange[j] x value (motor strength)
 *   8    damping_scale            jnt_damping[j] x value (the 12 hinges, not the free joint)
 *   9    contact_stiffness_scale  contact_stiffness x value
 *   10   contact_damping_scale    contact_damping x value
 * The identity row is (model.contact_friction, 0, 0, 0, 0, 1, 1, 1, 1, 1, 1); with it an env computes the shared model's bits.
 * Draws (QG_RESET_DYNAMICS in qg_reset / qg_walk_reset / qg_po_reset, or in task.reset_flags for auto-resets): column k of env i for
 * episode e is lo[k] + (hi[k] - lo[k]) u, u = the uniform of stream 16 + k of the (seed, env_index_base + i, e) key -- the key the reset
 * yaw of that episode uses (streams 0..15: yaw, hinge jitter, command; unchanged).  Without the flag rows persist across resets.
 * Validation (QG_ERR_ARG): non-finite values, friction or a scale < 0, a FRAME mass m0 + dm <= 0, a rotational inertia about the new
 * centre of mass that is not positive definite (a range: at its corners).
 * While the mode is on the generic (table-driven) step kernels run in their per-env form, LINK up to 4096 envs and QUAD above (also for
 * the compiled-in robot: qg_uses_baked_model returns 0); qg_step_device_seq and the resident form are refused, as are the PAIR and LANE
 * mappings. */
#define QG_NDYN 11
#define QG_DYN_FRICTION 0
#define QG_DYN_PAYLOAD_MASS 1
#define QG_DYN_PAYLOAD_X 2
#define QG_DYN_PAYLOAD_Y 3
#define QG_DYN_PAYLOAD_Z 4
#define QG_DYN_KP_SCALE 5
#define QG_DYN_KV_SCALE 6
#define QG_DYN_FORCE_SCALE 7
#define QG_DYN_DAMPING_SCALE 8
#define QG_DYN_CONTACT_STIFFNESS_SCALE 9
#define QG_DYN_CONTACT_DAMPING_SCALE 10
typedef struct { float lo[QG_NDYN], hi[QG_NDYN]; } qg_dynamics_range;
/* Validates and stores the range QG_RESET_DYNAMICS draws from (lo <= hi per column); switches the mode on (identity rows until the
 * first draw).  Like the other entry points that touch the per-env state, these four calls first wait for all work on the handle's
 * device (the ordering contract at the top of this file). */
int qg_set_dynamics_range(qg_sim *sim, const qg_dynamics_range *range);
/* Sets rows explicitly (curricula, tests): rows is a host [n_envs][QG_NDYN] array; mask == NULL sets every env, else only
 * mask[i] != 0 (the other rows are kept).  Switches the mode on. */
int qg_set_dynamics(qg_sim *sim, const uint8_t *mask, const float *rows);
/* The current rows into a host [n_envs][QG_NDYN] array; identity rows while the mode is off. */
int qg_get_dynamics(qg_sim *sim, float *rows);
/* Back to the shared model (the range is dropped too); the compiled-in robot's baked kernels run again (unless wrench mode, below,
 * is on: it keeps the per-env kernels, with identity rows). */
int qg_clear_dynamics(qg_sim *sim);

/* ---- external body wrenches (MuJoCo's data.xfrc_applied) and random pushes -----------------------------------------------------
 * Each env has a row of QG_NBODY x QG_NXFRC f32: for body b (the numbering above: 0 = FRAME, 1+3k+i = link i of leg k) a force xyz and a
 * torque xyz, both in the WORLD frame; the force acts at body b's centre of mass (body_ipos[b] of the handle's model -- a
 * QG_DYN_PAYLOAD_* row does not move that point, as a welded payload body would not move MuJoCo's xipos).  The row is held constant
 * over the frame_skip substeps of an env-step and rotated into the FRAME's axes at every substep with that substep's orientation; it
 * adds no term to the implicit matrix (a constant force has no velocity derivative).  Rows persist across qg_reset and auto-resets, as
 * dynamics rows do (QuadrupedEnv.reset() zeroes its Python mirror, as mj_resetData does).
 * Push schedule (qg_set_push): random horizontal forces on the FRAME, drawn per env with no per-env state.  For env-step
 * s = nstep / frame_skip of an episode, window w = s / interval, offset j = s % interval: the window holds a push if
 * u_gate < probability; the push starts at o = (k_off (interval - duration + 1)) >> 24 (k_off: the 24-bit integer behind the uniform)
 * and is active while o <= j < o + duration; its force (F cos th, F sin th, 0), F = force_min + (force_max - force_min) u_mag,
 * th = 2 pi u_head, acts at the FRAME's centre of mass, added to the FRAME's row for that env-step.  Uniforms: streams
 * 32 + 4 w + {0: gate, 1: offset, 2: magnitude, 3: heading} of the (seed, env_index_base + i, episode) key (disjoint from the reset
 * streams 0..15 and the dynamics streams 16..26; the stream number wraps after 2^30 windows).
 * Either qg_set_xfrc* or qg_set_push switches the handle into wrench mode: the per-env forms of the table-driven step kernels run (as
 * with per-env dynamics, identity dynamics rows while that mode is off; qg_uses_baked_model returns 0); qg_step_device_seq, the
 * resident form and the PAIR and LANE mappings are refused, as they are with per-env dynamics.  With every row zero and no schedule an
 * env computes the bits it computes with the mode off on the same per-env kernel. */
#define QG_NXFRC 6
#define QG_XFRC_FX 0
#define QG_XFRC_FY 1
#define QG_XFRC_FZ 2
#define QG_XFRC_TX 3
#define QG_XFRC_TY 4
#define QG_XFRC_TZ 5
typedef struct {
    int32_t interval;    /* env-steps per window, >= 1 */
    int32_t duration;    /* env-steps a push lasts, 1 .. interval */
    float probability;   /* of a push in a window, [0, 1] */
    float force_min;     /* N, 0 <= force_min <= force_max */
    float force_max;
} qg_push_params;
/* Sets rows from a host [n_envs][QG_NBODY][QG_NXFRC] array; mask == NULL sets every env, else only mask[i] != 0.  Non-finite values
 * are refused (QG_ERR_ARG, nothing changes).  Waits for device work, as the other entry points that touch per-env state do. */
int qg_set_xfrc(qg_sim *sim, const uint8_t *mask, const float *rows);
/* The same from a device array of that layout, enqueued on `stream` (a copy; no validation): the ordering contract of the other
 * *_device entry points.  The call that switches the mode on waits for the device first and must not be made while a stream is
 * being captured. */
int qg_set_xfrc_device(qg_sim *sim, const float *d_rows, void *stream);
/* The rows as set (without the push) into a host [n_envs][QG_NBODY][QG_NXFRC] array; zeros while the mode is off. */
int qg_get_xfrc(qg_sim *sim, float *rows);
/* Validates and sets the push schedule (QG_ERR_ARG, nothing changes: interval < 1, duration outside 1 .. interval, probability
 * outside [0, 1], force_min < 0 or > force_max); NULL turns the schedule off. */
int qg_set_push(qg_sim *sim, const qg_push_params *push);
/* Zero rows, schedule off, wrench mode off (the baked kernels run again unless per-env dynamics are on). */
int qg_clear_xfrc(qg_sim *sim);

/* ---- fused MLP policy: actor, critic and the Gaussian log-probability in one launch -------------------------------------------------
 * A qg_policy evaluates, for n rows of observations that are already on the device (the rows a step wrote, read in place), a tanh
 * MLP policy of the kind SB3's MlpPolicy builds: action mean, optionally a sampled action and its log-probability under a diagonal
 * Gaussian with a state-independent log_std, optionally the value of a second (critic) tower.  One kernel launch per call, exact
 * f32 arithmetic (the f32-input matrix instruction: every output is a k-ordered fmaf chain), no intermediate result in global
 * memory.  The handle is independent of qg_sim: one policy can serve several simulators or both halves of a pipelined rollout.
 *
 * Network: obs_dim -> hidden[0] -> .. -> hidden[n_hidden - 1] -> act_dim, tanh after every hidden layer (the only activation), the
 * output layer linear (out_tanh = 0, SB3's action_net) or tanh (out_tanh = 1).  has_value = 1 adds a critic tower with the same hidden
 * sizes and one linear output (SB3's default, non-shared net_arch).
 *
 * Canonical flat parameter vector (f32; qg_policy_param_count floats): the actor's layers in order, each W[out][in] row-major then
 * b[out]; then log_std[act_dim]; then, with has_value, the critic's layers in the same way (its last layer is W[1][h], b[1]).
 *
 * Forward pass, per row i (it depends on row i of obs and eps and on the parameters only -- not on n, on the row's position or on
 * the other rows: results are bit-identical however a batch is cut):
 *   mean     = net(obs[i * obs_stride .. + obs_dim))
 *   actions  = mean                              (eps == NULL: predict(deterministic=True))
 *            = mean + exp(log_std) * eps[i]      (eps: caller-supplied standard-normal draws [n][act_dim]; NOT clipped)
 *   log_prob = sum_a(-eps_a^2 / 2 - log_std_a - log(2 pi) / 2)    (eps == NULL: eps = 0, the log-density at the mean)
 *   value    = critic(obs[i])
 * obs_stride is counted in floats and >= obs_dim: the first 33 columns of a packed [n][35] row, or a row of an observation stack, are
 * read where the step left them.  Outputs for non-finite observations or parameters are unspecified (the device code is compiled
 * with finite-math assumptions).
 *
 * Ordering: qg_policy_forward_device and qg_policy_set_params_device follow the contract of the other *_device entry points (they
 * enqueue on the caller's stream, return at once and may be captured into a hipGraph).  qg_policy_create, qg_policy_destroy,
 * qg_policy_set_params and qg_policy_get_params wait for the device and must not be called while a stream is being captured. */
typedef struct qg_policy qg_policy;
typedef struct qg_policy_desc {
    int32_t struct_size;       /* sizeof(qg_policy_desc): checked */
    int32_t obs_dim;           /* 1 .. 512 */
    int32_t act_dim;           /* 1 .. 16 */
    int32_t n_hidden;          /* 1 .. 3 */
    int32_t hidden[3];         /* the first n_hidden: each a multiple of 16, 16 .. 256 */
    int32_t out_tanh;          /* 0 or 1 */
    int32_t has_value;         /* 0 or 1 */
} qg_policy_desc;
/* Validation (QG_ERR_ARG) comes before the device check (QG_ERR_DEVICE: there is no CPU backend). */
int qg_policy_create(int32_t device_id, const qg_policy_desc *desc, qg_policy **out);
int qg_policy_destroy(qg_policy *policy);
/* Length of the canonical flat vector, or QG_ERR_ARG for an invalid description.  Host only. */
int qg_policy_param_count(const qg_policy_desc *desc);
/* Parameters from / to a host array in the canonical order (a new handle holds zeros).  The round trip is exact. */
int qg_policy_set_params(qg_policy *policy, const float *host_params);
int qg_policy_get_params(qg_policy *policy, float *host_params);
/* The same from a device array, enqueued on `stream` (a copy and one small repacking launch): a forward pass enqueued later on that
 * stream uses the new parameters.  The training loop's path after each update. */
int qg_policy_set_params_device(qg_policy *policy, const float *d_params, void *stream);
/* One launch.  Device pointers: obs [n] rows of obs_stride floats; eps nullable [n][act_dim]; actions [n][act_dim]; log_prob nullable
 * [n]; value nullable [n] (QG_ERR_ARG when given and has_value == 0; NULL: the critic tower is not evaluated). */
int qg_policy_forward_device(qg_policy *policy, int32_t n, const float *obs, int32_t obs_stride, const float *eps, float *actions,
                             float *log_prob, float *value, void *stream);
/* The launch shape qg_policy_forward_device picks for n rows (with_value: a value buffer is given, so the critic tower is launched):
 * waves per 16-env tile (1 or 4) and output blocks per wave (1, 4 or 16).  Results do not depend on it, only the time does; tests
 * and A/B timing read it to know which instantiation ran.  Host only, launches nothing. */
int qg_policy_launch_shape(const qg_policy *policy, int32_t n, int32_t with_value, int32_t *waves, int32_t *blocks);

/* ---- asymmetric actor-critic: a critic window ---------------------------------------------------------------------------------------------
 * A handle of qg_policy_create_asym reads TWO windows of an observation row: the actor columns [0, obs_dim) as ever, the critic columns
 * [critic_obs_offset, critic_obs_offset + critic_obs_dim) of the same row -- the joint row of qg_priv_read_device, for one:
 * (0, O + 85) shows the critic everything, (O, 85) the clean privileged state alone.
 *   value = critic(obs[i * obs_stride + critic_obs_offset .. + critic_obs_dim)),  and the v of qg_policy_ppo_grad_device likewise.
 * The canonical vector keeps its order; the critic's first layer is W[hidden[0]][critic_obs_dim].  Every entry point that takes a
 * qg_policy takes such a handle; the stride rule becomes obs_stride >= obs_dim where the critic is not launched (a forward pass without
 * a value buffer) and obs_stride >= max(obs_dim, critic_obs_offset + critic_obs_dim) where it is (a forward pass with one, every
 * qg_policy_ppo_grad_device).  A handle of qg_policy_create has the window (0, obs_dim) and computes what it always has, bit for bit.
 * QG_ERR_ARG, before the device check: desc->has_value != 1; critic_obs_dim outside 1 .. 512; critic_obs_offset < 0 or
 * critic_obs_offset + critic_obs_dim > 512; an invalid description. */
int qg_policy_create_asym(int32_t device_id, const qg_policy_desc *desc, int32_t critic_obs_offset, int32_t critic_obs_dim, qg_policy **out);
/* Length of the canonical flat vector of such a handle (the offset does not enter), or QG_ERR_ARG.  Host only. */
int qg_policy_param_count_asym(const qg_policy_desc *desc, int32_t critic_obs_dim);
/* The critic's window; (0, obs_dim) for the handles of qg_policy_create, with or without a critic tower.  Host only. */
int qg_policy_critic_window(const qg_policy *policy, int32_t *offset, int32_t *dim);

/* ---- the PPO loss and its gradient for a qg_policy (one minibatch of SB3 2.x PPO.train) ------------------------------------------------
 * With c = clip_range, cv = clip_range_vf, sigma = exp(log_std), per row of the batch:
 *   mean = actor(obs)  (tanh on it when out_tanh);  z_a = (action_a - mean_a) / sigma_a
 *   logp = sum_a(-z_a^2 / 2 - log_std_a - log(2 pi) / 2);  lr = logp - old_log_prob;  r = exp(lr)
 *   policy_loss  = -mean_rows( min(adv r, adv clamp(r, 1 - c, 1 + c)) )
 *   v = critic(obs);  vp = cv > 0 ? old_values + clamp(v - old_values, -cv, cv) : v;  value_loss = mean_rows((returns - vp)^2)
 *   entropy_loss = -sum_a(0.5 + log(2 pi) / 2 + log_std_a)          (state-independent)
 *   loss = policy_loss + ent_coef entropy_loss + vf_coef value_loss
 * Without a critic (has_value == 0) value_loss = 0 and old_values / returns are not read.  Advantages are used as given (normalise
 * them beforehand: qg_policy_normalize_advantages_device); grad is ONE flat vector, which qg_policy_adam_update_device below or the
 * caller's own optimiser takes.
 *
 * grad [qg_policy_param_count] is d loss / d parameters in the canonical order, every element overwritten (the caller need not clear
 * it).  The heads: d loss / d logp = -(adv r) / B, and 0 where (adv > 0 and r > 1 + c) or (adv < 0 and r < 1 - c);
 * d logp / d mean_a = z_a / sigma_a; d loss / d log_std_a = sum_rows(d loss / d logp (z_a^2 - 1)) - ent_coef;
 * d loss / d v = vf_coef 2 (vp - returns) / B, and 0 where cv > 0 and |v - old_values| >= cv; a factor 1 - mean^2 with out_tanh; then
 * back through the tanh layers.  stats (nullable, [8]): loss, policy_loss, value_loss, entropy_loss, approx_kl = mean((r - 1) - lr),
 * clip_fraction = mean(|r - 1| > c), 0, 0 -- summed in f64 and rounded once.
 *
 * THREE launches per call (rows: forward recomputed, heads, deltas; weights: partial sums of every dW and db; reduce), all matrix
 * products on the exact-f32 matrix instruction, the heads in f64.  No floating-point atomics and no workgroup waits for another: sums
 * over rows are taken per tile of 16 rows, over slots of 32 consecutive tiles (512 rows) in ascending order, then over the slots in
 * ascending order -- a partition that depends on B alone.  The same inputs therefore give the same bits on every run, eagerly and under
 * graph replay; bits may differ between different B.  A row with adv = 0 and no value term contributes exact zeros wherever it sits.
 * Outputs for non-finite inputs are unspecified.  The policy's parameters and its forward pass are not touched.
 *
 * qg_policy_reserve_grad allocates the scratch of the pass for up to max_batch rows (activations and deltas of every layer per row,
 * one partial gradient per 512 rows) and the transposed weight image, which every later parameter update then also repacks (a policy
 * that never reserves enqueues exactly what it did before).  Host call: it waits for the device, must not be called during a stream
 * capture, and may be called again to grow.  qg_policy_ppo_grad_device follows the *_device contract: it enqueues on the caller's
 * stream, returns at once, can be captured into a hipGraph (params are taken by value at the call: a captured graph keeps them) and
 * allocates nothing.  QG_ERR_ARG, before any device check: NULL policy / params / batch / grad, a wrong struct_size, reserved != 0,
 * B < 1, B > the rows reserved (nothing reserved included), obs_stride < obs_dim, clip_range not finite or <= 0, another parameter
 * not finite, a NULL obs / actions / old_log_prob / advantages, and with a critic a NULL returns, or a NULL old_values with cv > 0. */
typedef struct qg_ppo_params {
    int32_t struct_size;       /* sizeof(qg_ppo_params): checked */
    int32_t reserved;          /* 0 */
    float clip_range;          /* finite, > 0            (SB3: 0.2) */
    float clip_range_vf;       /* finite; <= 0: value clipping off (SB3: None) */
    float ent_coef, vf_coef;   /* finite                 (SB3: 0.0, 0.5) */
} qg_ppo_params;
typedef struct qg_ppo_batch {  /* device pointers: what qg_rollout_gather_device wrote */
    int32_t struct_size;       /* sizeof(qg_ppo_batch): checked */
    int32_t obs_stride;        /* floats, >= obs_dim */
    const float *obs;          /* [B] rows */
    const float *actions;      /* [B][act_dim] */
    const float *old_log_prob; /* [B] */
    const float *advantages;   /* [B] */
    const float *old_values;   /* [B]; may be NULL without a critic or when clip_range_vf <= 0 */
    const float *returns;      /* [B]; may be NULL without a critic */
} qg_ppo_batch;
int qg_policy_reserve_grad(qg_policy *policy, int32_t max_batch);
int qg_policy_ppo_grad_device(qg_policy *policy, const qg_ppo_params *params, int32_t B, const qg_ppo_batch *batch, float *grad,
                              float *stats, void *stream);

/* ---- teacher-student distillation: an imitation loss and its gradient for a qg_policy ---------------------------------------------------
 * The student's action mean regressed onto given target means (a teacher's: what qg_policy_forward_device of the teacher's handle
 * writes with eps = NULL), on rows the caller chooses -- in DAgger the rows the student itself visited.  Per row i of B rows, all in
 * f64:
 *   mu_i = actor(obs_i)  (tanh on it when out_tanh);  t_i = target_mean[i];  w_i = weights ? weights[i] : 1
 *   QG_DISTILL_MSE:  l_i = sum_a (mu_i[a] - t_i[a])^2
 *   QG_DISTILL_KL:   l_i = KL(N(t_i, exp(lt)) || N(mu_i, exp(ls)))
 *                        = sum_a [ ls_a - lt_a + (exp(2 lt_a) + (t_i[a] - mu_i[a])^2) / (2 exp(2 ls_a)) - 1/2 ]
 *                    ls the student's own log_std, lt = target_log_std [act_dim] in device memory (the teacher's log_std)
 *   loss = coef / B sum_i w_i l_i
 * The loss sums over the action dimensions (as the PPO log-probability does) and divides by B, NOT by sum_i w_i: a row of weight zero
 * then contributes exact zeros to every sum, and no second pass over the rows is needed.
 *
 * grad [qg_policy_param_count] is d loss / d parameters in the canonical order, every element overwritten.  The heads:
 *   d loss / d mu_i[a] = coef / B w_i 2 (mu - t)                     (MSE)       coef / B w_i (mu - t) / exp(2 ls_a)       (KL)
 *   a factor 1 - mu^2 with out_tanh, each delta rounded to f32 once; then back through the tanh layers as qg_policy_ppo_grad_device.
 *   d loss / d log_std_a = coef / B sum_i w_i (1 - (exp(2 lt_a) + (t - mu)^2) / exp(2 ls_a))   (KL);   exact +0.0   (MSE)
 * The critic's entries of a handle that has a critic are exact +0.0 and the critic tower is not launched: handles with and without
 * a critic and handles of qg_policy_create_asym are accepted alike, and only the actor's window [0, obs_dim) of a row is read
 * (obs_stride >= obs_dim suffices).  stats (nullable, [8]): loss, sq_err = 1/B sum_i w_i sum_a (mu - t)^2 (both modes), kl = 1/B sum_i
 * w_i l_i (KL mode; 0 in MSE mode), max_abs_err = max |mu - t| over the rows with w_i != 0 (0 when there is none), weight_sum =
 * sum_i w_i (B without weights), 0, 0, 0 -- the sums in f64, each statistic rounded once.
 *
 * THREE launches, the pass of qg_policy_ppo_grad_device on the actor's tower with other heads, in the same scratch
 * (qg_policy_reserve_grad; calls on one handle must be ordered by the caller).  Rounding order: the forward pass and the walk back
 * as there (f32 products in chains of 16 on the matrix instruction, the chains, the bias and tanh in f64, rounded once).  A row's l_i:
 * the actions 4g .. 4g + 3 in ascending order, then the four groups g by a fixed butterfly.  The scalar sums of a tile of 16 rows: the
 * rows in ascending order.  dW and db: a tile's 16 rows are one f32 chain in ascending row order from zero, the 32 tiles of a slot
 * of 512 rows are added in ascending order in f64 and rounded once, the slots in ascending order in f64 and rounded once.  No
 * floating-point atomics, no workgroup waits for another, and the partition depends on B alone: the same inputs give the same bits
 * on every run, eagerly and under graph replay, at any obs_stride.  A row of weight zero adds exact zeros to every chain (x + 0 is
 * exact), so moving rows of weight zero about changes no bit as long as the other rows keep their order and their tiles (a single
 * such row may sit anywhere); rows that move to another tile change the grouping of the sum, and with it, possibly, the last bit.
 * Outputs for non-finite inputs are unspecified, in rows of weight zero too: the backward products multiply that row's zero deltas
 * with its activations.  The parameters and the forward pass are not touched.
 *
 * It follows the *_device contract: enqueues on the caller's stream, returns at once, allocates nothing, can be captured into a
 * hipGraph (params and the batch's pointers are taken by value at the call).  QG_ERR_ARG, before any device call: NULL params / batch
 * / grad / policy, a wrong struct_size, reserved != 0, an unknown loss, a non-finite coef, B < 1, a NULL obs or target_mean, KL mode
 * without target_log_std, B > the rows reserved (nothing reserved included), obs_stride < obs_dim.
 * Not offered: distilling the value, recurrent students, mixing the executed action between teacher and student (torch.where does it),
 * accumulating into grad (add two flat vectors, or all-reduce them), normalising by sum_i w_i (scale coef). */
#define QG_DISTILL_MSE 0
#define QG_DISTILL_KL 1
typedef struct qg_distill_params {
    int32_t struct_size;           /* sizeof(qg_distill_params): checked */
    int32_t loss;                  /* QG_DISTILL_MSE or QG_DISTILL_KL */
    float coef;                    /* finite */
    int32_t reserved;              /* 0 */
} qg_distill_params;
typedef struct qg_distill_batch {  /* device pointers */
    int32_t struct_size;           /* sizeof(qg_distill_batch): checked */
    int32_t obs_stride;            /* floats, >= obs_dim */
    const float *obs;              /* [B] rows */
    const float *target_mean;      /* [B][act_dim] */
    const float *target_log_std;   /* [act_dim]; required in KL mode, not read in MSE mode */
    const float *weights;          /* [B], or NULL: every row has weight 1 */
} qg_distill_batch;
int qg_policy_distill_grad_device(qg_policy *policy, const qg_distill_params *params, int32_t B, const qg_distill_batch *batch,
                                  float *grad, float *stats, void *stream);

/* ---- Adam, gradient-norm clipping and advantage normalisation on the device ------------------------------------------------------------
 * What stands between the gradient and the next forward pass of SB3's PPO.train: torch.nn.utils.clip_grad_norm_ and torch.optim.Adam
 * (amsgrad off, no weight decay) on the handle's own canonical parameters, and normalize_advantage for one minibatch.  One minibatch
 * is then gather -> normalise -> ppo_grad -> adam_step: seven launches, no copy of the network, nothing of it on the host.
 *
 * qg_policy_adam_update_device, with g = grad, m and v the two moments (f32, zero after reserve) and t the step count (an integer in
 * DEVICE memory, zero after reserve: a captured step replays as t = 1, 2, 3, ..), in exactly this order and with these roundings:
 *   norm  = f32(sqrt(sum_i g_i^2))              the sum in f64 (every product is exact there) over a fixed partition, see below
 *   coef  = max_grad_norm > 0 ? min(1, max_grad_norm / (norm + 1e-6)) : 1                    f32: one addition, one division
 *   t     = t + 1;   lr = lr_device ? *lr_device : params.lr
 *   step  = f32(lr / (1 - beta_one^t));   root = f32(sqrt(1 - beta_two^t));   a1 = f32(1 - beta_one);   a2 = f32(1 - beta_two)
 *                                               each formed in f64 from the f32 arguments and rounded once
 *   per element, in f32 (fl: one rounding; fma: one rounding for product and sum):
 *   gc    = fl(coef g)
 *   m     = fma(beta_one, m, fl(a1 gc));   v = fma(beta_two, v, fl(fl(a2 gc) gc))
 *   p     = fl(p - fl(step fl(m / fl(fl(sqrt(v) / root) + eps))))                            square root and divisions correctly rounded
 * grad is not modified (a data-parallel trainer all-reduces it between ppo_grad and this call).  lr_device (nullable) points to one
 * f32 on the device that replaces params.lr: a schedule needs no re-capture; it must hold a finite value >= 0.  params_out (nullable,
 * [qg_policy_param_count]) receives a copy of the new canonical vector.  stats (nullable, [4]): norm before clipping, coef, t after
 * the step, the lr used.  The call also brings both operand images up to date -- the forward image including exp(log_std) (f64,
 * rounded once), and the transposed image once qg_policy_reserve_grad has been called --, bit for bit what
 * qg_policy_set_params_device would have produced from the new vector: the next forward / ppo_grad on the stream sees the new
 * parameters.  qg_policy_set_params and qg_policy_set_params_device leave m, v and t alone, as loading weights leaves a torch optimiser.
 *
 * TWO launches per step.  The first writes one f64 sum of squares per slot of 2048 consecutive elements of grad (a thread its eight
 * elements in ascending order, a fixed butterfly over the wave, the four waves in ascending order) and its first workgroup moves t;
 * in the second every workgroup adds the slots in ascending order itself, forms the scalars and updates its 2048 elements, writing
 * each new parameter to its places in the images.  No floating-point atomics; no workgroup waits for another; the partition depends on
 * the parameter count alone; given the scalars, element i of p, m, v depends on element i of the inputs alone.  The same inputs give
 * the same bits on every run, eagerly and under graph replay.  A zero gradient on m = 0 leaves p bit for bit; lr = 0 leaves p bit for
 * bit while m, v, t move.  Image elements that are padding are never written: they stay zero.  Outputs for non-finite inputs are
 * unspecified.  Calls on one handle must be ordered by the caller (one stream, or events).
 *
 * qg_policy_reserve_adam allocates m, v, t and the slots' sums.  Host call: it waits for the device and must not be called during a
 * stream capture; a second call is a no-op that keeps the state; it does not need qg_policy_reserve_grad.  qg_policy_adam_get_state /
 * _set_state copy m, v [qg_policy_param_count] and t (>= 0) from / to host arrays -- the round trip is exact --, wait for the device
 * and must not be called during a capture; QG_ERR_ARG before qg_policy_reserve_adam.  qg_policy_adam_update_device follows the *_device
 * contract: it enqueues on the caller's stream, returns at once, allocates nothing and can be captured into a hipGraph (params are
 * taken by value at the call; what lr_device points to is read at each replay).  QG_ERR_ARG, before any device check: NULL policy /
 * params / grad, a wrong struct_size, reserved != 0, a value outside the ranges below, params_out == grad, nothing reserved.
 *
 * qg_policy_normalize_advantages_device: out_i = f32((adv_i - mean) / (std + 1e-8)) with mean = sum(adv) / B and std =
 * sqrt(sum((adv_i - mean)^2) / (B - 1)) (the unbiased one: torch's std()), both sums and the quotient in f64, the quotient rounded
 * once.  ONE launch of one workgroup of 1024 threads: thread k adds the groups of four elements k, k + 1024, .. in ascending order,
 * a fixed butterfly adds the threads of a wave, then the waves in ascending order: an order that depends on B alone.  A constant
 * vector gives exact zeros.  out == adv (in place) is allowed; any other overlap is not.  It needs no reservation (the handle names
 * the device), follows the *_device contract and is capturable.  QG_ERR_ARG: a NULL argument, B < 2 (SB3 skips the normalisation
 * there) or B > 2^31 - 1 - 4096. */
typedef struct qg_adam_params {
    int32_t struct_size;       /* sizeof(qg_adam_params): checked */
    int32_t reserved;          /* 0 */
    float lr;                  /* finite, >= 0                       (SB3: 3e-4) */
    float beta_one, beta_two;  /* in [0, 1)                          (0.9, 0.999) */
    float eps;                 /* finite, > 0                        (1e-8; SB3's PPO passes 1e-5) */
    float max_grad_norm;       /* finite; <= 0: clipping off         (SB3: 0.5) */
} qg_adam_params;
int qg_policy_reserve_adam(qg_policy *policy);
/* (one optimiser step; "update" because every *step* entry point of this header advances the envs) */
int qg_policy_adam_update_device(qg_policy *policy, const qg_adam_params *params, const float *grad, const float *lr_device,
                               float *params_out, float *stats, void *stream);
int qg_policy_adam_get_state(qg_policy *policy, float *exp_avg, float *exp_avg_sq, int64_t *step);
int qg_policy_adam_set_state(qg_policy *policy, const float *exp_avg, const float *exp_avg_sq, int64_t step);
int qg_policy_normalize_advantages_device(qg_policy *policy, int32_t B, const float *adv, float *out, void *stream);

/* ---- running observation and reward normalisation (SB3's VecNormalize) on the device ---------------------------------------------------
 * A qg_norm keeps, in f64 on the device, a running mean and variance per observation column, a discounted return per env and the
 * running variance of those returns, and normalises the rows a step left on the device: the semantics of Stable-Baselines3 2.x
 * VecNormalize / RunningMeanStd.  Like qg_policy it is independent of qg_sim and touches no step kernel.
 *
 * A running statistic holds mean (initially 0), var (1) and count (1e-4).  update(batch of n rows), with bm the column means and bv
 * the population variances (divisor n) of the batch:
 *   delta = bm - mean;  tot = count + n
 *   mean' = mean + delta * n / tot
 *   M2    = var * count + bv * n + delta^2 * count * n / tot
 *   var'  = M2 / tot;   count' = tot
 * One training step over the n envs, in this order:
 *   1. norm_obs:     obs_rms.update(obs)
 *   2. obs_out     = f32(clip((obs - mean) / sqrt(var + epsilon), -clip_obs, clip_obs))          with the updated statistics
 *   3. returns     = returns * gamma + reward  (f64, one per env);  ret_rms.update(returns), a one-column statistic
 *   4. norm_reward: reward_out = f32(clip(reward / sqrt(ret_var + epsilon), -clip_reward, clip_reward))   with the updated ret_var
 *   5. returns[done] = 0
 * With training == 0 steps 1, 3 and 5 are skipped (no word of the state changes); 2 and 4 use the statistics as they stand.  A flag
 * that is switched off copies the value through unchanged.  The quotient is rounded to f32 once and then clipped, so a clipped
 * element is exactly +-f32(clip).
 *
 * Batch moments are accumulated in f64 (shifted sums within a tile of rows, Chan's merge above that) and combined in an order that
 * depends on (n, obs_dim) alone: no floating-point atomics, results are bit-identical from run to run and under graph replay.  A
 * row's output depends on the statistics and on that row alone.  Outputs for non-finite inputs are unspecified (the device code is
 * compiled with finite-math assumptions): a NaN reward would also poison the return statistic for good.
 *
 * Ordering: the *_device calls follow the contract of the other *_device entry points (they enqueue on the caller's stream, return
 * at once and may be captured into a hipGraph; everything that changes from call to call lives in device memory, so a captured step
 * replays correctly any number of times).  A training step is three kernel launches, an apply one, an update two.  qg_norm_create,
 * qg_norm_destroy, qg_norm_get_state and qg_norm_set_state wait for the device and must not be called during a capture. */
typedef struct qg_norm qg_norm;
typedef struct qg_norm_desc {
    int32_t struct_size;       /* sizeof(qg_norm_desc): checked */
    int32_t obs_dim;           /* 1 .. 512 */
    int32_t n_envs;            /* >= 1 */
    double gamma;              /* finite, >= 0 (SB3: 0.99) */
    double epsilon;            /* finite, >= 0 (1e-8) */
    double clip_obs;           /* > 0 (10) */
    double clip_reward;        /* > 0 (10) */
    int32_t norm_obs;          /* 0 or 1 */
    int32_t norm_reward;       /* 0 or 1 */
} qg_norm_desc;
#define QG_NORM_DONE_U8 QG_DONE_U8      /* the older names of the pair */
#define QG_NORM_DONE_F32 QG_DONE_F32
/* Validation (QG_ERR_ARG) comes before the device check (QG_ERR_DEVICE: there is no CPU backend). */
int qg_norm_create(int32_t device_id, const qg_norm_desc *desc, qg_norm **out);
int qg_norm_destroy(qg_norm *norm);
/* One step as above; n must equal n_envs.  Device pointers; strides in elements.  obs rows of obs_dim floats at in_stride /
 * out_stride >= obs_dim; obs_out == obs_in (in place) is allowed, and so is reward_out == reward_in.  reward_in nullable: NULL is an
 * observation-only step (steps 1 and 2).  done: a done vector (QG_DONE_*), nullable (no return is ever cleared).  With the strides
 * one call normalises a packed [n][obs_dim + 2] row in place: obs at column 0, reward at column obs_dim, done at obs_dim + 1, every
 * stride obs_dim + 2.  Loads and stores are 16 bytes per lane where obs_dim and both strides are multiples of 4 and both bases are
 * 16-byte aligned, 4 bytes otherwise (the packed stride of 35). */
int qg_norm_step_device(qg_norm *norm, int32_t n, const float *obs_in, int32_t in_stride, float *obs_out, int32_t out_stride,
                        const float *reward_in, int32_t reward_in_stride, float *reward_out, int32_t reward_out_stride, const void *done,
                        int32_t done_kind, int32_t done_stride, int32_t training, void *stream);
/* Step 1 alone, whatever norm_obs says, for any n >= 1: what SB3 does with the observations reset() returns. */
int qg_norm_update_obs_device(qg_norm *norm, int32_t n, const float *obs, int32_t stride, void *stream);
/* Step 2 alone with the statistics as they stand, for any n >= 1: terminal observations, evaluation, a second consumer. */
int qg_norm_apply_obs_device(qg_norm *norm, int32_t n, const float *obs_in, int32_t in_stride, float *obs_out, int32_t out_stride,
                             void *stream);
/* returns = 0 for every env (SB3's reset()). */
int qg_norm_reset_returns_device(qg_norm *norm, void *stream);
/* The whole state from / to host f64 arrays: mean[obs_dim], var[obs_dim], returns[n_envs] and the scalars.  The round trip is exact. */
int qg_norm_get_state(qg_norm *norm, double *mean, double *var, double *count, double *ret_mean, double *ret_var, double *ret_count,
                      double *returns);
int qg_norm_set_state(qg_norm *norm, const double *mean, const double *var, double count, double ret_mean, double ret_var,
                      double ret_count, const double *returns);

/* ---- PPO rollout buffer on the device: step record, fused GAE, minibatch gather (SB3's RolloutBuffer) --------------------------------
 * A qg_rollout turns the rows a collection loop leaves on the device into what PPO trains on.  The caller owns the storage (device
 * arrays it allocates and keeps alive: qg_rollout_storage); the handle owns only the small state: the cursor `pos`, two integer error
 * counters and the per-env episode accumulators, all in device memory, so that a captured call replays correctly any number of
 * times.  Like qg_policy and qg_norm it is independent of qg_sim and touches no step kernel.  With n = n_envs, K = n_steps:
 *
 * begin(obs):  pos = 0; slot 0 of storage.obs takes obs.  obs == NULL: slot `pos` (as the launch finds it: the observation after the
 *   last recorded step of the previous rollout) is copied to slot 0.  The episode accumulators are not touched.
 *
 * add(step), called after the env step; p = pos as the launch finds it.  p == K: nothing is stored, overflow += 1, pos stays.  Else
 *   1. actions[p], log_prob[p], values[p] take the arguments; dones[p][i] = (done[i] != 0) as 0 / 1
 *   2. rewards[p][i] = reward[i]                                         trunc_value == NULL
 *                    = fma(f32(gamma), trunc_value[i], reward[i])        else: ONE rounding.  The caller passes V(terminal observation)
 *      where the time limit truncated the episode and 0 elsewhere (SB3's time-limit bootstrap).
 *   3. slot p + 1 of obs takes next_obs (slot t is the observation the policy saw at step t; slot pos the one after the last step:
 *      the caller's critic turns it into last_values)
 *   4. per env i, by one thread: cur_return += f64((episode_reward ? episode_reward : reward)[i]) in f64; cur_length += 1; where
 *      done[i]: fin_return_sum += cur_return, fin_length_sum += cur_length, fin_count += 1, then cur_return = 0, cur_length = 0.
 *      No cross-env reduction happens on the device.  episode_reward lets a caller who normalises rewards log the raw returns.
 *   5. pos = p + 1
 *
 * compute(last_values): with F = pos read on the device, per env, for t = F - 1 .. 0 in this order, in f32:
 *      nnt   = 1 - dones[t]                   (the done stored with step t ends the episode: nothing flows back across it)
 *      nv    = t == F - 1 ? last_values : values[t + 1]
 *      delta = rewards[t] + gamma * nv * nnt - values[t]
 *      A[t]  = delta + gamma * gae_lambda * nnt * A[t + 1]              (A[F] = 0)
 *      returns[t] = A[t] + values[t]
 *   (RolloutBuffer.compute_returns_and_advantage of SB3 2.x with episode_starts[t + 1] written as dones[t]).  Slots >= F are not
 *   written.  Rounding order: g = f32(gamma) and gl = f32(gamma * gae_lambda), the product formed in f64 on the host; g * nnt and
 *   gl * nnt are exact (nnt is 0 or 1); then
 *      delta = fl(fma(g * nnt, nv, rewards[t]) - values[t])     A[t] = fma(gl * nnt, A[t + 1], delta)     returns[t] = fl(A[t] + values[t])
 *   -- two fused multiply-adds, one subtraction, one addition: four roundings per step.  One lane owns one env and walks time
 *   serially (no scan over time), so the results do not depend on n or on the launch shape.
 *
 * gather(idx, B): flat sample f = t * n + i is valid for 0 <= f < F * n (F = pos read on the device).  Row b of every non-NULL output
 *   takes sample idx[b]: obs slot t row i, actions, log_prob, values, advantages, returns -- copies, bit for bit.  An index outside
 *   the valid range reads nothing: its row is written as zeros and bad_index += 1 (once per such row).  idx is int64, what
 *   torch.randperm yields.
 *
 * Arithmetic: no floating-point atomics; integer atomics only for the cursor's ticket and the two counters.  Every stored float
 * depends on its own env or sample alone: results are bit-identical between runs, between eager calls and graph replay and however
 * a launch is shaped.  Outputs for non-finite inputs are unspecified (the device code is compiled with finite-math assumptions).
 * Row copies are 16 bytes per lane where obs_dim and the row stride are multiples of 4 and both bases are 16-byte aligned, 4 bytes
 * otherwise (the rule of qg_norm).
 *
 * Ordering: qg_rollout_begin_device, _add_device, _compute_device and _gather_device follow the contract of the other *_device entry
 * points (they enqueue on the caller's stream, return at once and may be captured into a hipGraph); each is ONE kernel launch, the
 * cursor's update included: every workgroup of a begin / add launch reads the cursor before it takes an integer ticket, and the
 * workgroup that draws the last ticket writes the new cursor, so no workgroup observes the cursor its own launch writes.  Calls on
 * one handle must be ordered by the caller (one stream, or events): two launches that move the cursor must not overlap.
 * qg_rollout_create, _destroy, _get_info and _episode_stats wait for the device and must not be called during a capture. */
typedef struct qg_rollout qg_rollout;
typedef struct qg_rollout_desc {
    int32_t struct_size;       /* sizeof(qg_rollout_desc): checked */
    int32_t n_envs;            /* >= 1 */
    int32_t n_steps;           /* K >= 1; (K + 1) * n_envs <= 2^31 - 1 */
    int32_t obs_dim;           /* 1 .. 512 */
    int32_t act_dim;           /* 1 .. 16 */
    int32_t reserved;          /* 0 */
    double gamma;              /* finite, in [0, 1] (SB3: 0.99) */
    double gae_lambda;         /* finite, in [0, 1] (0.95) */
} qg_rollout_desc;
/* Device pointers the caller owns and keeps alive while the handle lives; none may be NULL, the f32 ones are 4-byte aligned. */
typedef struct qg_rollout_storage {
    int32_t struct_size;       /* sizeof(qg_rollout_storage): checked */
    int32_t reserved;          /* 0 */
    float *obs;                /* [K + 1][n][obs_dim] */
    float *actions;            /* [K][n][act_dim] */
    float *log_prob;           /* [K][n], as values, rewards, advantages, returns */
    float *values;
    float *rewards;
    float *advantages;
    float *returns;
    uint8_t *dones;            /* [K][n] */
} qg_rollout_storage;
#define QG_ROLLOUT_DONE_U8 QG_DONE_U8
#define QG_ROLLOUT_DONE_F32 QG_DONE_F32
/* The rows of one env-step (device pointers; strides in elements). */
typedef struct qg_rollout_step {
    int32_t struct_size;       /* sizeof(qg_rollout_step): checked */
    int32_t next_obs_stride;   /* >= obs_dim */
    int32_t reward_stride;     /* >= 1 */
    int32_t done_kind;         /* QG_DONE_U8 or QG_DONE_F32 */
    int32_t done_stride;       /* >= 1 */
    int32_t episode_reward_stride; /* >= 1 where episode_reward is given */
    const float *next_obs;     /* [n] rows of obs_dim floats: the observation after the step */
    const float *actions;      /* [n][act_dim] */
    const float *log_prob;     /* [n] */
    const float *value;        /* [n] */
    const float *reward;       /* [n] at reward_stride */
    const void *done;          /* a done vector (QG_DONE_*), not NULL */
    const float *trunc_value;  /* nullable [n] */
    const float *episode_reward; /* nullable [n] at episode_reward_stride */
} qg_rollout_step;
/* The outputs of a gather (device pointers, each nullable: a NULL output is skipped). */
typedef struct qg_rollout_batch {
    int32_t struct_size;       /* sizeof(qg_rollout_batch): checked */
    int32_t reserved;          /* 0 */
    float *obs;                /* [B][obs_dim] */
    float *actions;            /* [B][act_dim] */
    float *old_log_prob;       /* [B], as old_values, advantages, returns */
    float *old_values;
    float *advantages;
    float *returns;
} qg_rollout_batch;
typedef struct qg_rollout_info {
    int32_t pos;               /* the cursor: slots [0, pos) are filled */
    int32_t reserved;
    int64_t overflow;          /* adds that found the buffer full (nothing stored) */
    int64_t bad_index;         /* gather rows whose index was out of range (written as zeros) */
} qg_rollout_info;
/* Validation (QG_ERR_ARG: a field out of range, a NULL or misaligned storage pointer, a wrong struct_size) comes before the device
 * check (QG_ERR_DEVICE: there is no CPU backend).  A new handle has pos = 0, both counters 0 and empty episode accumulators. */
int qg_rollout_create(int32_t device_id, const qg_rollout_desc *desc, const qg_rollout_storage *storage, qg_rollout **out);
int qg_rollout_destroy(qg_rollout *rollout);
/* One launch each, as above.  obs: [n] rows at obs_stride >= obs_dim, or NULL. */
int qg_rollout_begin_device(qg_rollout *rollout, const float *obs, int32_t obs_stride, void *stream);
int qg_rollout_add_device(qg_rollout *rollout, const qg_rollout_step *step, void *stream);
int qg_rollout_compute_device(qg_rollout *rollout, const float *last_values, void *stream);
/* B >= 1 (QG_ERR_ARG otherwise); idx [B] int64 on the device. */
int qg_rollout_gather_device(qg_rollout *rollout, const int64_t *idx, int32_t B, const qg_rollout_batch *out, void *stream);
/* Host: waits for the device, then reads pos and the counters. */
int qg_rollout_get_info(qg_rollout *rollout, qg_rollout_info *info);
/* Host: waits for the device, copies the per-env finished-episode accumulators and sums them in env order (deterministic).  clear != 0
 * zeroes them; running episodes (cur_return, cur_length) continue. */
int qg_rollout_episode_stats(qg_rollout *rollout, double *return_sum, int64_t *length_sum, int64_t *count, int32_t clear);

/* ---- sensor noise, sensor bias and actuation latency on the device ---------------------------------------------------------------------
 * A qg_perturb stands between a policy and an env: one launch before the env delays the actions by a per-episode number of env-steps
 * and adds Gaussian noise to them, one launch behind the env adds Gaussian noise and a per-episode constant bias to chosen columns of
 * the observation frames.  Like qg_norm it is independent of qg_sim and touches no step kernel; all of its state is in device memory.
 *
 * Keys.  Every draw is a pure function of (seed, env_index_base + i, episode_i, stream): shards reproduce the rows of one big handle,
 * a replayed graph draws fresh noise at every replay (age and episode advance on the device), and a frame keeps its noise while it
 * travels through the window of a stacked observation.
 *   seed_p = seed + 0x51474E4F49534531                                        (mod 2^64: a key space apart from the simulator's streams)
 *   k(s)   = the 24-bit integer of the simulator's stream hash:  x = seed_p + 0xA0761D6478BD642F * s + 0x9E3779B97F4A7C15 * (env + 1)
 *            + 0xD1B54A32D192ED03 * (episode + 1);  k = mix64(mix64(x)) >> 40  (splitmix64's finaliser, twice; s as a 64-bit integer)
 *   z(s)   = sqrt(-2 ln u1) * cos(2 pi u2),  u1 = (k(s) + 1) / 2^24,  u2 = k(s + 1) / 2^24;   |z| <= sqrt(48 ln 2) = 5.77
 *            evaluated in f32 in this order: u1 and 2 * u2 are exact; L = logf(u1); r = sqrtf(-2 * L); c = cospif(2 * u2); z = r * c.
 * Streams: 0 the delay; 2 + 2c the bias of column c (c < 64); S(f, q) = 4096 + 2 * (128 * f + q) the draws of frame f: q = c is
 * observation column c, q = 64 + j the action noise of joint j for the env-step taken at age f.  Frame 0 is the reset frame, the frame
 * the step taken at age a produces is frame a + 1.  f < 2^23.
 *
 * State per env: age (env-steps since the episode began), episode (this handle's own counter, 0 in a new handle; NOT the
 * simulator's) and an action ring [max_delay + 1][n][12].
 *   d_i = delay_lo + ((k(0) * (delay_hi - delay_lo + 1)) >> 24)              computed from the key of the running episode, not stored
 *
 * actions (before the env; reads age, does not advance it), M = max_delay + 1:
 *   ring[age mod M][i] = actions_in[i];   v = age - d_i >= 0 ? ring[(age - d_i) mod M][i] : reset_action
 *   actions_out[i][j] = v_j                                                 action_std == 0: a bit copy
 *                     = v_j + action_std * z(S(age, 64 + j))                else: one product, one add, both rounded (no fma)
 *   No clipping (the env clips).  actions_out may be actions_in.
 *
 * observe (behind the env); a row is [window][frame_dim], newest frame last; a' = age + 1.  The row of episode E with top frame t:
 *   slot k holds frame f = max(t - (window - 1 - k), 0);    out = in + e(f, c)                                     ONE f32 add
 *   e(f, c) = bias_std[c] * z(2 + 2c) + obs_std[c] * z(S(f, c))      two f32 products and their f32 sum, no fma; a term whose std is
 *   0 is left out.  A column with obs_std[c] == 0 and bias_std[c] == 0 is copied bit for bit and never touches the hash.
 *   live env:      obs row = (episode, a');  then age = a'
 *   finished env, QG_PERTURB_DONE_ROW_RESET (the partially observable env: the row already holds the new episode's reset stack):
 *                  obs row = (episode + 1, 0): frame 0 in every slot;  terminal_obs row, when given, = (episode, a')
 *   finished env, QG_PERTURB_DONE_ROW_TERMINAL (the plain and the walking env: the row is the terminal observation):
 *                  obs row = (episode, a')
 *   finished env, both: then episode += 1, age = 0.   Rows of terminal_obs that belong to live envs are not touched.
 *
 * begin (an explicit reset): for the envs of the mask (all, when NULL): episode += 1, age = 0, and, when rows are given, their row =
 * (episode + 1, 0).  Other envs' rows are not touched.
 *
 * One wave owns an env in observe and begin: it alone reads and writes that env's age and episode, so rows may be perturbed in
 * place.  No atomics; no workgroup waits for another.  Results are bit-identical between runs, between eager calls and graph replay and
 * between a handle and shards of it.  Outputs for non-finite inputs are unspecified (the device code is compiled with finite-math
 * assumptions), except that columns copied through keep their bits.
 *
 * Ordering: qg_perturb_actions_device, _observe_device and _begin_device follow the contract of the other *_device entry points (they
 * enqueue on the caller's stream, return at once, are ONE kernel launch each and may be captured into a hipGraph).  Calls on one handle
 * must be ordered by the caller.  qg_perturb_create, _destroy, _get_delays, _get_state and _set_state wait for the device and must not
 * be called during a capture. */
typedef struct qg_perturb qg_perturb;
typedef struct qg_perturb_desc {
    int32_t struct_size;       /* sizeof(qg_perturb_desc): checked */
    int32_t n_envs;            /* >= 1 */
    int32_t frame_dim;         /* 1 .. 64 */
    int32_t window;            /* 1 .. 64: an observation row is window * frame_dim floats */
    int32_t max_delay;         /* 0 .. 16 env-steps: the ring holds max_delay + 1 action rows per env */
    int32_t delay_lo;          /* 0 <= delay_lo <= delay_hi <= max_delay */
    int32_t delay_hi;
    int32_t done_row;          /* QG_PERTURB_DONE_ROW_RESET or _TERMINAL */
    float action_std;          /* finite, >= 0 */
    float obs_std[64];         /* per frame column, finite, >= 0; columns >= frame_dim are ignored */
    float bias_std[64];
    float reset_action[12];    /* what the servos hold until the first delayed action arrives (the task's default_ctrl); finite */
    int32_t reserved;          /* 0 */
    uint64_t seed;
    uint64_t env_index_base;   /* env i of this handle is env env_index_base + i of the run */
} qg_perturb_desc;
#define QG_PERTURB_DONE_ROW_RESET 0
#define QG_PERTURB_DONE_ROW_TERMINAL 1
#define QG_PERTURB_DONE_U8 QG_DONE_U8
#define QG_PERTURB_DONE_F32 QG_DONE_F32
#define QG_PERTURB_MAX_DELAY 16
/* Validation (QG_ERR_ARG) comes before the device check (QG_ERR_DEVICE: there is no CPU backend).  A new handle has age = 0,
 * episode = 0 and a ring of zeros. */
int qg_perturb_create(int32_t device_id, const qg_perturb_desc *desc, qg_perturb **out);
int qg_perturb_destroy(qg_perturb *perturb);
/* n must equal n_envs.  Device pointers, [n][12] f32, contiguous. */
int qg_perturb_actions_device(qg_perturb *perturb, int32_t n, const float *actions_in, float *actions_out, void *stream);
/* Rows of window * frame_dim floats at in_stride / out_stride (elements, >= the row length); obs_out may be obs_in.  terminal_obs
 * (nullable, in place, its own stride) only with QG_PERTURB_DONE_ROW_RESET.  done: a done vector (QG_DONE_*), nullable (no env
 * finished). */
int qg_perturb_observe_device(qg_perturb *perturb, int32_t n, const float *obs_in, int32_t in_stride, float *obs_out, int32_t out_stride,
                              float *terminal_obs, int32_t terminal_stride, const void *done, int32_t done_kind, int32_t done_stride,
                              void *stream);
/* mask: nullable device [n] u8 (non-zero selects); rows: nullable device rows at row_stride, perturbed in place. */
int qg_perturb_begin_device(qg_perturb *perturb, int32_t n, const uint8_t *mask, float *rows, int32_t row_stride, void *stream);
/* Host: delays[n_envs] = d_i of the running episodes. */
int qg_perturb_get_delays(qg_perturb *perturb, int32_t *delays);
/* Host arrays: age [n] i32, episode [n] i64 (0 <= episode < 2^62, 0 <= age < 2^23), ring [max_delay + 1][n][12] f32.  The round trip
 * is exact. */
int qg_perturb_get_state(qg_perturb *perturb, int32_t *age, int64_t *episode, float *ring);
int qg_perturb_set_state(qg_perturb *perturb, const int32_t *age, const int64_t *episode, const float *ring);

/* ---- foot-contact sensing on the device: ground reaction forces, foot kinematics, gait timers --------------------------------------
 * A qg_contact is bound to a simulator and only READS its state arrays: it adds no step kernel and changes none.  One launch
 * (qg_contact_read_device) evaluates, for every env, at the state (qpos, qvel) AS IT STANDS IN MEMORY:
 *
 * Body poses and velocities, world frame (body 0 = FRAME, body 1 + 3k + i = link i of leg k; hinge j drives body j + 1 about its z):
 *   x_0 = qpos[0:3], R_0 = R(qpos[3:7] / |qpos[3:7]|);   x_b = x_p + R_p pos_b,  R_b = R_p Q_b Rz(qpos[7 + j] - ref_j)   (p: parent)
 *   v_0 = qvel[0:3], w_0 = R_0 qvel[3:6];   v_b = v_p + w_p x (x_b - x_p),  w_b = w_p + (third column of R_b) qvel[6 + j]
 *
 * Ground reaction force of body b (plane z = 0, the contact law of the step kernels), over its sample points cp_i:
 *   r_i = R_b cp_i,  pen_i = max(0, contact_margin - (x_b.z + r_i.z)),  S = sum_i pen_i,  W = contact_stiffness * S
 *   P = x_b + (sum_i pen_i r_i) / S                      centre of pressure;   vP = v_b + w_b x (P - x_b)
 *   c = contact_damping * min(1, S / contact_ramp)       the damper ramps in with the summed penetration
 *   F_n = max(0, W - c vP.z)                             no adhesion
 *   c_t = c, or mu F_n / |vP.xy| where c |vP.xy| > mu F_n    viscous, Coulomb-limited
 *   F[b] = (-c_t vP.x, -c_t vP.y, F_n);  F[b] = 0 where no point is below the margin.
 * This is the force the NEXT substep would apply from the velocity before its update -- not the force of the substep that produced
 * the state.  After an auto-reset the row describes the new episode's first state.  A qg_step_device_seq launch shows only the state
 * after its last env-step.  The contact constants are those of the handle's model (any model); while per-env dynamics are on, friction
 * and the contact stiffness and damping scales come from the env's row.  External wrenches and pushes do not enter.
 *
 * Feet are bodies 3, 6, 9, 12 (foot f = leg f).  contact_f = F[foot].z > force_threshold.  Gait timers, per foot, in whole env-steps
 * (exact integers in device memory: prev_contact, phase_steps, last_air_steps, last_stance_steps; and one `armed` flag per env),
 * updated by a read with advance != 0:
 *   not armed, or done[env] != 0:  phase_steps = 1, last_air_steps = last_stance_steps = 0, no event, prev = contact; the env is armed
 *   armed, contact == prev:        phase_steps += 1
 *   armed, contact != prev:        touchdown (contact now): last_air_steps = phase_steps; liftoff: last_stance_steps = phase_steps;
 *                                  the event's column is 1 in this row; phase_steps = 1, prev = contact
 * With advance == 0 nothing is written: the row shows contact from the state, the timers as they stand, and no event.  Times are
 * f32(steps) * f32(dt), dt = model.timestep * task.frame_skip of the simulator's task at the call.
 *
 * Outputs (device, f32, env-major, each nullable but not both): body_force [n][13][3]; feet [n][4][12] in the columns below (48 bytes
 * per foot; `feet` must be 16-byte aligned).  Rows depend on their env alone: a handle of any size computes the same bits for a state.
 * Outputs for non-finite states are unspecified (the device code is compiled with finite-math assumptions).
 *
 * Ordering: qg_contact_read_device follows the contract of the other *_device entry points: ONE kernel launch on the caller's stream,
 * no allocation and no wait, may be captured into a hipGraph (the timers live in device memory, so a replay advances them).  The
 * caller orders it behind the step whose state it is to see.  While the resident step mode is on the state lives in registers:
 * reads are refused (qg_resident_stop first).  Every refusal is QG_ERR_ARG and comes before anything is launched.  qg_contact_create,
 * _destroy, _reset, _read, _get_state and _set_state wait for the device and must not be called during a capture; destroy the
 * qg_contact before its simulator. */
typedef struct qg_contact qg_contact;
typedef struct qg_contact_desc {
    int32_t struct_size;       /* sizeof(qg_contact_desc): checked */
    int32_t reserved;          /* 0 */
    float force_threshold;     /* N; finite, >= 0 */
} qg_contact_desc;
#define QG_CONTACT_FORCE_DIM 39    /* floats per env of body_force */
#define QG_CONTACT_FEET_DIM 48     /* floats per env of feet */
#define QG_FOOT_DIM 12             /* floats per foot */
#define QG_FOOT_POS 0              /* world position of the foot body's frame origin (3) */
#define QG_FOOT_VEL 3              /* world velocity of that origin (3) */
#define QG_FOOT_CONTACT 6          /* 0.0 or 1.0 */
#define QG_FOOT_TOUCHDOWN 7        /* 0.0 or 1.0 */
#define QG_FOOT_LIFTOFF 8          /* 0.0 or 1.0 */
#define QG_FOOT_PHASE_TIME 9       /* s in the current phase (stance or swing), this sample included */
#define QG_FOOT_LAST_AIR_TIME 10   /* s of the last completed swing (0: none yet in this episode) */
#define QG_FOOT_LAST_STANCE_TIME 11
#define QG_CONTACT_DONE_U8 QG_DONE_U8
#define QG_CONTACT_DONE_F32 QG_DONE_F32
int qg_contact_create(qg_sim *sim, const qg_contact_desc *desc, qg_contact **out);
int qg_contact_destroy(qg_contact *contact);
/* Disarms the envs of the host mask [n] (non-zero selects; NULL: every env): their next advancing read starts an episode. */
int qg_contact_reset(qg_contact *contact, const uint8_t *mask);
/* done: a done vector (QG_DONE_*), nullable; read only when advance != 0. */
int qg_contact_read_device(qg_contact *contact, const void *done, int32_t done_kind, int32_t done_stride, int32_t advance,
                           float *body_force, float *feet, void *stream);
/* The same rows into host arrays (each nullable but not both), synchronously, without advancing the timers. */
int qg_contact_read(qg_contact *contact, float *body_force, float *feet);
/* The timers and armed flags as one opaque blob (the round trip is exact; a blob fits a handle of the same n_envs). */
int64_t qg_contact_state_bytes(const qg_contact *contact);
int qg_contact_get_state(qg_contact *contact, void *blob);
int qg_contact_set_state(qg_contact *contact, const void *blob);

/* ---- reward-term monitoring on the device: the step log and per-term episode sums -----------------------------------------------------
 * A qg_monitor consumes the reward components the step kernels leave on the device (qg_walk_step_device's `components`,
 * qg_step_device's `reward_components`): what the reference's training script logs at every env-step (train_quadruped.py:86-110: the
 * mean of every reward key over the envs, the reward's mean and np.std) goes into a ring the caller owns, and every term is summed over
 * each env's episode, the finished episodes' sums over each other.  Like qg_norm and qg_rollout it is independent of qg_sim, takes
 * pointers and touches no step kernel.  With n = n_envs, C = n_terms, x[i][c] for c < C env i's term c and x[i][C] its reward, ONE
 * record does, in this order:
 *
 *   1. the log row.  row = records % capacity, records as the launch finds it in device memory.  For c <= C
 *        log[row][c] = fl(S[c] / n),  S[c] the f64 sum of f64(x[i][c]) over ALL n envs -- a finished env counts with its terminal
 *        step's terms, as the reference's infos do -- added in a fixed order: per env chunk of 256 by a butterfly over the lanes (32, 16,
 *        .. 1), ((w0 + w1) + w2) + w3 over a workgroup's waves, a tile's chunks one after the other per thread, the tiles in 4 runs
 *        and ((r0 + r1) + r2) + r3 over the runs.
 *        log[row][C + 1] = sqrt(M2 / n): the population standard deviation of the reward (np.std, ddof = 0).  M2 comes from a thread's
 *        sum(x - K) and sum((x - K)^2) with K its first reward (exact in f64), then Chan's merge over lanes, waves and tiles (the tiles in
 *        64 runs, then a butterfly) -- never E[x^2] - E[x]^2.  A constant reward and n = 1 give exactly 0.
 *        log[row][C + 2] = the number of envs whose done is set, exact.
 *   2. the episode accumulators, per env by one thread: acc[i][c] = acc[i][c] + f64(x[i][c]) -- ONE IEEE add per step and term --,
 *        len[i] += 1.
 *   3. the fold.  For the envs with done[i] != 0: totals[c] = totals[c] + F[c], F[c] the sum of their acc[i][c] in the order of S (an
 *        env that did not finish adds an exact zero: the order depends on (n, C) alone, and a step where nobody finishes leaves totals
 *        bit for bit); length_sum += len[i], episodes += 1; then acc[i][.] = 0, len[i] = 0.
 *   4. records += 1, in device memory: nothing the host bakes into a launch depends on the step number, so the hipGraph of one
 *        closed-loop step, replayed K times, fills K rows.
 *
 * Two launches, a tile pass and a combine pass of one workgroup across a kernel boundary.  No floating-point atomics, no integer ones
 * either; no workgroup reads what another workgroup of its own launch wrote.  The same inputs give the same bits on every run,
 * eagerly and under graph replay, whatever the strides and alignment of the caller's tensors; bits may differ between different n.
 * Only log[row] and the handle's own state are written.  Calls on one monitor must be ordered by the caller on one stream.  Outputs
 * for non-finite inputs are unspecified (the device code is compiled with finite-math assumptions: run the walking envs with
 * nan_direction off).  qg_monitor_record_device follows the contract of the other *_device entry points (it enqueues on the caller's
 * stream, returns at once and may be captured); every other entry point waits for the device and must not be called during a capture.
 * Validation (QG_ERR_ARG: a NULL handle or pointer, a size or stride out of range, a bad done vector) comes before any device call. */
#define QG_MONITOR_MAX_TERMS 32
typedef struct qg_monitor qg_monitor;
/* 1 <= n_terms <= QG_MONITOR_MAX_TERMS (the walking layers have 11, the plain env 3), n_envs >= 1, capacity >= 1 rows of the ring.  A
 * new handle has empty accumulators and totals and records = 0. */
int qg_monitor_create(int32_t device_id, int32_t n_envs, int32_t n_terms, int32_t capacity, qg_monitor **out);
int qg_monitor_destroy(qg_monitor *monitor);
/* components: [n] rows of n_terms floats at comp_stride >= n_terms; reward: [n] at reward_stride >= 1; done: a done vector
 * (QG_DONE_*), NULL: nobody finished; log: f64 [capacity][n_terms + 3] on the device, the caller's. */
int qg_monitor_record_device(qg_monitor *monitor, const float *components, int32_t comp_stride, const float *reward, int32_t reward_stride,
                             const void *done, int32_t done_kind, int32_t done_stride, double *log, void *stream);
/* Empties the running accumulators (acc, len) of the envs of the host mask [n] (non-zero selects; NULL: every env).  clear_totals != 0
 * also zeroes totals, episodes and length_sum; clear_log != 0 sets records = 0 (the ring itself is the caller's). */
int qg_monitor_reset(qg_monitor *monitor, const uint8_t *host_mask, int32_t clear_totals, int32_t clear_log);
/* The cursor, the finished episodes' number and lengths and totals [n_terms + 1] (the reward last).  clear != 0 then zeroes totals,
 * episodes and length_sum; the running episodes and the cursor continue. */
int qg_monitor_get_info(qg_monitor *monitor, int64_t *records, int64_t *episodes, int64_t *length_sum, double *totals, int32_t clear);
/* The whole state from / to host arrays: acc [n][n_terms + 1], len [n], totals [n_terms + 1] and the three integers.  The round trip
 * is exact: a restored monitor continues bit for bit. */
int qg_monitor_get_state(qg_monitor *monitor, double *acc, int32_t *len, double *totals, int64_t *episodes, int64_t *length_sum,
                         int64_t *records);
int qg_monitor_set_state(qg_monitor *monitor, const double *acc, const int32_t *len, const double *totals, int64_t episodes,
                         int64_t length_sum, int64_t records);

/* ---- gait-shaped reward terms from the foot-contact sensor ---------------------------------------------------------------------------------
 * A qg_gait is bound to a qg_contact.  Its launch (qg_gait_reward_device) IS that sensor's read of the env-step -- forces, foot rows,
 * timers, advance / done semantics and bits exactly as qg_contact_read_device, body_force and feet being optional outputs of it -- and
 * in the same kernel reduces seven reward terms per env, weights them and adds them to the reward.  It is the ADVANCING READ of its
 * env-step: a caller does not also call qg_contact_read_device(advance = 1) in that env-step (the timers would move twice).
 *
 * For env i and foot f = 0..3 (bodies 3, 6, 9, 12), with r = feet[i][f][.] in the QG_FOOT_* columns as this launch reports them,
 * c_f = r[CONTACT], td_f = r[TOUCHDOWN] (0.0 or 1.0 each) and Fz_b = body_force[i][b][2], the unweighted terms, in this order:
 *   0 feet_air_time       g_i * sum_f td_f (r[LAST_AIR_TIME] - air_time_target)
 *   1 feet_slip           sum_f c_f (r[VEL_X]^2 + r[VEL_Y]^2)
 *   2 feet_clearance      sum_f (1 - c_f) (r[POS_Z] - clearance_target)^2 sqrt(r[VEL_X]^2 + r[VEL_Y]^2)
 *   3 touchdown_speed     sum_f td_f r[VEL_Z]^2
 *   4 feet_contact_force  sum_f max(Fz_foot(f) - max_contact_force, 0)
 *   5 body_contact        the number of the 9 non-foot bodies with Fz_b > force_threshold (the sensor's threshold, the foot flag's
 *                         exact f32 comparison)
 *   6 flight              1 where sum_f c_f == 0, else 0
 * The gate: g_i = 1 without a command; with command [n] rows (cmd_x, cmd_y), g_i = 1 where max(|cmd_x|, |cmd_y|) > min_command_speed,
 * else 0 (the max-norm: the comparison is exact in every precision).  Sums over feet run in ascending f, in f32.
 *   components[i][base_terms + k] = f32(w_k * term_k);   shaped_i = the f32 sum of the seven in ascending k;
 *   reward_out[i] = reward[i] + shaped_i  (shaped_i alone where reward is NULL; reward_out may be reward).
 * Where done names env i, the sensor's row already describes the new episode's first state: its seven components are exact zeros and
 * its reward passes through bit for bit (done is read for this whatever `advance` says).  A launch with advance == 0 shows no
 * touchdown, so terms 0 and 3 are zero there.  Outputs for non-finite inputs are unspecified.
 *
 * base_components (nullable; f32 [n] rows of base_terms <= 25 columns): the launch copies them to components[i][0 : base_terms] and
 * writes its seven behind them, so that one [n][base_terms + 7] buffer feeds a qg_monitor (QG_MONITOR_MAX_TERMS columns).  The rows of
 * base_components and components may not overlap -- unless base_components == components at the same stride: the base columns are in
 * place already and nothing is copied.
 *
 * ONE kernel launch on the caller's stream behind the step whose state it is to see, no allocation, no wait, no LDS, no atomics;
 * capturable, and bit-reproducible eagerly and under graph replay; rows depend on their env alone.  Only the caller's outputs and
 * the sensor's timers are written.  Refused while the resident step mode is on (qg_resident_stop first); every refusal is QG_ERR_ARG
 * and comes before anything is launched.  The handle has no per-env state of its own (nothing to snapshot: the timers are the
 * sensor's); destroy the qg_gait before its qg_contact. */
#define QG_GAIT_NTERMS 7
#define QG_GAIT_FEET_AIR_TIME 0
#define QG_GAIT_FEET_SLIP 1
#define QG_GAIT_FEET_CLEARANCE 2
#define QG_GAIT_TOUCHDOWN_SPEED 3
#define QG_GAIT_FEET_CONTACT_FORCE 4
#define QG_GAIT_BODY_CONTACT 5
#define QG_GAIT_FLIGHT 6
typedef struct qg_gait qg_gait;
typedef struct qg_gait_desc {
    int32_t struct_size;               /* sizeof(qg_gait_desc): checked */
    int32_t reserved;                  /* 0 */
    float weights[QG_GAIT_NTERMS];     /* w_k, any sign; finite */
    float air_time_target;             /* s; this and the three thresholds below: finite, >= 0 */
    float clearance_target;            /* m */
    float max_contact_force;           /* N */
    float min_command_speed;           /* the command's units */
} qg_gait_desc;
int qg_gait_create(qg_contact *contact, const qg_gait_desc *desc, qg_gait **out);
int qg_gait_destroy(qg_gait *gait);
/* weights [QG_GAIT_NTERMS], host, finite: read by the launches that follow; a captured graph keeps the weights it was captured with. */
int qg_gait_set_weights(qg_gait *gait, const float *weights);
/* done: a done vector (QG_DONE_*), nullable.  reward (nullable), reward_out: f32 [n] at their strides >= 1.  components: [n] rows of
 * base_terms + 7 floats at components_stride >= base_terms + 7; components and reward_out are each nullable but not both.
 * base_components: see above (base_stride >= base_terms; NULL with base_terms = 0).  command: nullable, [n] rows of 2 floats at
 * command_stride >= 2.  body_force [n][13][3] and feet [n][4][12] (16-byte aligned): the sensor's outputs, each nullable. */
int qg_gait_reward_device(qg_gait *gait, const void *done, int32_t done_kind, int32_t done_stride, int32_t advance, const float *reward,
                        int32_t reward_stride, float *reward_out, int32_t reward_out_stride, float *components, int32_t components_stride,
                        const float *base_components, int32_t base_stride, int32_t base_terms, const float *command,
                        int32_t command_stride, float *body_force, float *feet, void *stream);

/* ---- privileged state pack: the simulator's truth as the input row of an asymmetric critic -----------------------------------------------
 * A qg_priv is bound to a simulator and only READS its state arrays: it adds no step kernel and changes none.  One launch
 * (qg_priv_read_device) writes, for every env i, the joint row
 *   out[i] = [ obs[i][0 : obs_dim]  |  QG_PRIV_DIM privileged columns ]
 * the observation an actor sees (noisy, lagged, stacked: whatever the caller's obs rows hold) copied bit for bit in front, and behind
 * it the state the sensors do not show, evaluated at (qpos, qvel, act, nstep, episode) AS THEY STAND IN MEMORY -- after an auto-reset
 * the row describes the new episode's first state.  With R0 = R(qpos[3:7] / |qpos[3:7]|), formed as the contact sensor forms it:
 *   cols   name          definition
 *   0-2    base_lin_vel  R0^T qvel[0:3]                     (the unlagged velocimeter)
 *   3-5    base_ang_vel  qvel[3:6], bit copy
 *   6-8    gravity_dir   R0^T (0, 0, -1): the negated third row of R0
 *   9      base_height   qpos[2], bit copy
 *   10-21  joint_pos     qpos[7:19], bit copy
 *   22-33  joint_vel     qvel[6:18], bit copy
 *   34-45  act           the 12 servo activation states, bit copy
 *   46-49  foot_contact  F[foot f].z > force_threshold as 0.0 / 1.0 (bodies 3, 6, 9, 12)
 *   50-61  foot_force    F[foot f], world xyz, foot-major
 *   62-65  foot_height   x_foot.z (the sensor's QG_FOOT_POS z)
 *   66     body_contact  the number of the 9 non-foot bodies with F_b.z > force_threshold, as f32
 *   67-77  dynamics      the env's QG_NDYN row, bit copy; the identity row while per-env dynamics are off
 *   78-83  frame_wrench  the FRAME's xfrc row (force, torque) plus the push schedule's force for env-step s = nstep / frame_skip of the
 *                        key (seed, env_index_base + i, episode): the wrench the NEXT env-step applies to the FRAME; zeros while wrench
 *                        mode is off
 *   84     episode_time  f32(nstep) * f32(model.timestep), one rounding
 * F[b], x_b and the threshold comparison are the contact sensor's, computed by the same device code: columns 46-65 are bit for bit what
 * qg_contact_read_device(advance = 0) with the same threshold reports for that state (and the force is the one the next substep
 * applies).  The push is drawn by the device function the step kernels draw it with, from the schedule as it stands in device memory.
 *
 * ONE kernel launch on the caller's stream behind the step whose state it is to see, no allocation, no wait, no LDS, no atomics;
 * capturable, and bit-reproducible eagerly and under graph replay; rows depend on their env alone, so a handle of any size computes
 * the same bits for a state.  Only the caller's rows are written.  Refused while the resident step mode is on (qg_resident_stop
 * first); every refusal is QG_ERR_ARG and comes before anything is launched.  The handle has no per-env state (nothing to snapshot);
 * destroy the qg_priv before its simulator. */
typedef struct qg_priv qg_priv;
typedef struct qg_priv_desc {
    int32_t struct_size;       /* sizeof(qg_priv_desc): checked */
    int32_t reserved;          /* 0 */
    float force_threshold;     /* N; finite, >= 0 */
} qg_priv_desc;
#define QG_PRIV_DIM 85
#define QG_PRIV_BASE_LIN_VEL 0
#define QG_PRIV_BASE_ANG_VEL 3
#define QG_PRIV_GRAVITY_DIR 6
#define QG_PRIV_BASE_HEIGHT 9
#define QG_PRIV_JOINT_POS 10
#define QG_PRIV_JOINT_VEL 22
#define QG_PRIV_ACT 34
#define QG_PRIV_FOOT_CONTACT 46
#define QG_PRIV_FOOT_FORCE 50
#define QG_PRIV_FOOT_HEIGHT 62
#define QG_PRIV_BODY_CONTACT 66
#define QG_PRIV_DYNAMICS 67
#define QG_PRIV_FRAME_WRENCH 78
#define QG_PRIV_EPISODE_TIME 84
int qg_priv_create(qg_sim *sim, const qg_priv_desc *desc, qg_priv **out);
int qg_priv_destroy(qg_priv *priv);
/* obs: nullable [n] rows of obs_dim floats at obs_stride >= obs_dim, copied bit for bit to out[i][0 : obs_dim] (obs == NULL: obs_dim
 * must be 0).  out: [n] rows at out_stride >= obs_dim + QG_PRIV_DIM; the 85 columns go to out[i][obs_dim : obs_dim + 85]; columns
 * behind them are not written.  obs and out may not overlap.  The obs rows are copied with 16-byte accesses where obs_dim and both
 * strides are multiples of 4 and both pointers are 16-byte aligned, element by element otherwise: the bits are the same. */
int qg_priv_read_device(qg_priv *priv, const float *obs, int32_t obs_stride, int32_t obs_dim, float *out, int32_t out_stride, void *stream);
/* Synchronous, into a host [n][QG_PRIV_DIM] array (no observation in front). */
int qg_priv_read(qg_priv *priv, float *host_out);

/* ---- commanded gait schedule: a per-env phase oscillator, clock inputs for the policy and rewards that hold the feet to it ------------------
 * A qg_sched is bound to a qg_contact.  Its launch (qg_sched_advance_device) advances, per env, a phase oscillator with a commanded gait
 * (which foot is to stand when, at which stepping frequency), writes the oscillator as ten clock columns behind the observation and
 * reduces four reward terms that compare the feet with the schedule.  The ground forces, the feet's position and velocity and the
 * contact flags are the contact sensor's, computed by its device code from the simulator's state AS IT STANDS IN MEMORY, with
 * advance == 0 semantics: THE SENSOR'S TIMERS AND ARMED FLAGS ARE NEITHER READ NOR WRITTEN.  The launch is not the advancing read of
 * its env-step: it composes with qg_gait_reward_device and qg_contact_read_device in any order.
 *
 * State per env, in device memory: phi (u32, the phase as a fraction of 2^32; it wraps by integer overflow) and episode (i64, this
 * handle's own counter, 0 in a new handle; NOT the simulator's).
 *
 * Keys.  Every draw is a pure function of (seed, env_index_base + i, episode_i, stream), through qg_perturb's k(s) -- the same mix64,
 * the same 24-bit result, the same formula -- in a key space of its own:
 *   seed_s = seed + 0x5147534348454431                                        (mod 2^64; ASCII "QGSCHED1")
 *   k(s): x = seed_s + 0xA0761D6478BD642F * s + 0x9E3779B97F4A7C15 * (env + 1) + 0xD1B54A32D192ED03 * (episode + 1);  k = mix64(mix64(x)) >> 40
 * The parameters of the running episode of env i, recomputed from the key wherever they are needed, never stored:
 *   g    = (k(0) * n_gaits) >> 24                                             the row of the gait table
 *   freq = f32(freq_lo + f32(span * f32(k(1) * 2^-24)))                       Hz; span = f32(freq_hi - freq_lo): one product, one add, no fma
 *   phi0 = random_phase ? k(2) << 8 : 0                                       the phase the episode starts at
 * Table integers, formed on the host at create from row g's (offset[4], duty):
 *   off_f = u32(rint(f64(offset_f) * 2^32)) mod 2^32;   D = u32(rint(f64(duty) * 2^32))
 * Step increment, with dt32 = f32(model.timestep * frame_skip) of the simulator's task at the call, as the sensor forms its dt:
 *   dphi = u32(rint(f64(freq) * f64(dt32) * 2^32))        a launch with freq_hi * dt32 > 0.5 is refused
 *
 * The launch, for env i, in this order:
 *   1. phi += dphi.
 *   2. For foot f = 0..3 (bodies 3, 6, 9, 12); every float below is exact in f32:
 *        q_f = phi + off_f (mod 2^32);  hard_f = q_f < D;  p_f = f32(q_f >> 8) * 2^-24;  d = f32(D >> 8) * 2^-24
 *        m_f = hard_f ? min(p_f, d - p_f) : -min(p_f - d, 1 - p_f)            the signed distance to the nearer edge of the stance
 *        s_f = kappa == 0 ? (hard_f ? 1 : 0) : clamp(0.5 + m_f * inv2k, 0, 1)  inv2k = f32(1 / (2 f64(kappa))); one product, one add, no fma
 *   3. The stand gate.  With command [n] rows (cmd_x, cmd_y): where max(|cmd_x|, |cmd_y|) <= min_command_speed every s_f = 1 and
 *      every hard_f is true (the schedule says "stand"); the phase and the clock columns keep running.  Without a command no env stands.
 *   4. F[b], the foot origin's position x and velocity v, and contact_f = F[foot f].z > force_threshold: bit for bit what
 *      qg_contact_read_device(advance = 0) reports for that state.
 *   5. The unweighted terms, f32, every product and sum rounded (no fma), sums over feet in ascending f:
 *        0 swing_force      sum_f (1 - s_f) (1 - expf(-((Fx Fx + Fy Fy) + Fz Fz) * inv_sf2))      inv_sf2 = f32(1 / f64(sigma_force)^2)
 *        1 stance_velocity  sum_f s_f (1 - expf(-((vx vx + vy vy) + vz vz) * inv_sv2))            inv_sv2 = f32(1 / f64(sigma_velocity)^2)
 *        2 swing_height     sum_f (1 - s_f) (x_z - swing_height_target)^2
 *        3 contact_match    the number of feet with contact_f == hard_f, 0..4, exact
 *   6. components[i][base_terms + k] = f32(w_k * term_k);  shaped_i = their f32 sum in ascending k;  reward_out[i] = reward[i] + shaped_i
 *      (shaped_i alone where reward is NULL; reward_out may be reward).  reward, reward_out, components, base_components (copied in
 *      front, or in place where it IS components at the same stride) and the strides follow qg_gait_reward_device's rules, with
 *      base_terms <= QG_MONITOR_MAX_TERMS - 4.  Here every output is nullable: a launch without any only advances the phase.
 *   7. The clock columns (QG_SCHED_DIM = 10), of a phase phi, gait row g and frequency freq:
 *        0-3  sinpif(2 p_f)     4-7  cospif(2 p_f)     8  freq     9  d
 *      out[i] = [ obs[i][0 : obs_dim] | the 10 columns ], the observation copied as qg_priv_read_device copies it (16-byte accesses
 *      where alignment allows, the same bits either way).  obs == out at the same stride: the observation is in place already and
 *      only the ten columns are written; any other overlap is refused.  out is nullable.
 *   8. Where done names env i (a new episode has begun in the simulator): its four components are exact zeros and its reward passes
 *      through bit for bit.
 *        QG_PERTURB_DONE_ROW_TERMINAL (the walking env): the row's clock columns are the old episode's, after its advance;
 *        QG_PERTURB_DONE_ROW_RESET (the partially observable env): the row's columns are the new episode's at its phi0, with its gait
 *          and frequency; the rows of terminal_obs / terminal_out (nullable; the same copy and in-place rules) of the FINISHED envs get
 *          the old episode's columns after its advance; rows of live envs are not touched there;
 *        both: then episode += 1 and phi = phi0 of the new episode.
 *
 * begin (an explicit reset, qg_sched_begin_device): for the envs of the mask (all, when NULL): episode += 1, phi = phi0 of the new
 * episode, and, where rows are given, rows[i][obs_dim : obs_dim + 10] = the new episode's columns at phi0.  Other rows are not touched.
 *
 * qg_sched_advance_device is ONE kernel launch on the caller's stream behind the step whose state it is to see (qg_sched_begin_device is
 * one launch of its own): no allocation, no wait, no LDS, no atomics; capturable, and a replay advances the phase; bit-reproducible
 * eagerly and under graph replay; rows depend on their env and key alone, so shards with env_index_base reproduce one big handle.
 * One lane owns an env's phi and episode: it alone reads and writes them.  Refused while the resident step mode is on
 * (qg_resident_stop first); every refusal is QG_ERR_ARG and comes before anything is launched.  Outputs for non-finite inputs are
 * unspecified.  qg_sched_create, _destroy, _set_weights, _get_gaits, _state_bytes, _get_state and _set_state wait for the device and
 * must not be called during a capture.  Destroy the qg_sched before its qg_contact. */
#define QG_SCHED_NTERMS 4
#define QG_SCHED_SWING_FORCE 0
#define QG_SCHED_STANCE_VELOCITY 1
#define QG_SCHED_SWING_HEIGHT 2
#define QG_SCHED_CONTACT_MATCH 3
#define QG_SCHED_DIM 10
#define QG_SCHED_SIN 0
#define QG_SCHED_COS 4
#define QG_SCHED_FREQ 8
#define QG_SCHED_DUTY 9
#define QG_SCHED_MAX_GAITS 8
typedef struct qg_sched qg_sched;
typedef struct qg_sched_gait {
    float offset[4];                   /* per foot, in [0, 1): the fraction of a period by which the foot leads the oscillator */
    float duty;                        /* in [1/64, 63/64]: the fraction of a period the foot is to stand */
} qg_sched_gait;
typedef struct qg_sched_desc {
    int32_t struct_size;               /* sizeof(qg_sched_desc): checked */
    int32_t reserved;                  /* 0 */
    int32_t n_gaits;                   /* 1 .. QG_SCHED_MAX_GAITS rows of `gaits` */
    int32_t random_phase;              /* 0 or 1 */
    int32_t done_row;                  /* QG_PERTURB_DONE_ROW_RESET or _TERMINAL */
    float freq_lo;                     /* Hz; 0 < freq_lo <= freq_hi, finite */
    float freq_hi;
    float kappa;                       /* half-width of the stance / swing ramp in phase units, 0 <= kappa <= 1/128 */
    float sigma_force;                 /* N; finite, > 0 */
    float sigma_velocity;              /* m/s; finite, > 0 */
    float swing_height_target;         /* m; finite */
    float min_command_speed;           /* the command's units; finite, >= 0 */
    float weights[QG_SCHED_NTERMS];    /* w_k, any sign; finite */
    qg_sched_gait gaits[QG_SCHED_MAX_GAITS];
    uint64_t seed;
    uint64_t env_index_base;           /* env i of this handle is env env_index_base + i of the run */
} qg_sched_desc;
/* Validation (QG_ERR_ARG) comes before the handle and the device are looked at.  A new handle has episode = 0 and phi = phi0 of
 * episode 0 for every env. */
int qg_sched_create(qg_contact *contact, const qg_sched_desc *desc, qg_sched **out);
int qg_sched_destroy(qg_sched *sched);
/* weights [QG_SCHED_NTERMS], host, finite: read by the launches that follow; a captured graph keeps the weights it was captured with. */
int qg_sched_set_weights(qg_sched *sched, const float *weights);
/* done: a done vector (QG_DONE_*), nullable.  reward (nullable; only with reward_out), reward_out: f32 [n] at strides >= 1.
 * components: [n] rows at components_stride >= base_terms + 4; base_components: see above (base_stride >= base_terms; NULL with
 * base_terms = 0; only with components).  command: nullable, [n] rows of 2 floats at command_stride >= 2.  obs: nullable [n] rows of
 * obs_dim floats at obs_stride >= obs_dim (NULL: obs_dim must be 0); out: nullable, [n] rows at out_stride >= obs_dim + 10.
 * terminal_obs / terminal_out: nullable, rows as obs / out at their own strides; terminal_out only with QG_PERTURB_DONE_ROW_RESET. */
int qg_sched_advance_device(qg_sched *sched, const void *done, int32_t done_kind, int32_t done_stride, const float *reward, int32_t reward_stride,
                         float *reward_out, int32_t reward_out_stride, float *components, int32_t components_stride,
                         const float *base_components, int32_t base_stride, int32_t base_terms, const float *command, int32_t command_stride,
                         const float *obs, int32_t obs_stride, int32_t obs_dim, float *out, int32_t out_stride, const float *terminal_obs,
                         int32_t terminal_obs_stride, float *terminal_out, int32_t terminal_out_stride, void *stream);
/* mask: nullable device [n] u8 (non-zero selects); rows: nullable device rows at row_stride >= obs_dim + 10 (obs_dim >= 0). */
int qg_sched_begin_device(qg_sched *sched, const uint8_t *mask, float *rows, int32_t row_stride, int32_t obs_dim, void *stream);
/* Host arrays [n], each nullable: the gait row g, freq and phi of the running episodes. */
int qg_sched_get_gaits(qg_sched *sched, int32_t *gait, float *freq, uint32_t *phi);
/* The per-env state (phi, episode) as ONE opaque blob of *bytes bytes (host pointer); restoring it into a handle of the same shape
 * reproduces every later launch bit for bit.  The round trip is exact. */
int qg_sched_state_bytes(const qg_sched *sched, int64_t *bytes);
int qg_sched_get_state(qg_sched *sched, void *blob);
int qg_sched_set_state(qg_sched *sched, const void *blob);

/* ---- command curriculum: an adaptive grid over (speed, velocity angle) that decides what the robots are asked to do -----------------------
 * A qg_cmdcur is bound to a qg_walk.  Each env runs a SEGMENT: a commanded (speed, velocity angle alpha, heading angle theta) drawn from
 * one bin of an n_speed x n_alpha grid, held until the episode ends or, with resample_steps = R > 0, for R env-steps.  The grid's integer
 * weights say how often a bin is drawn; they grow outward from the bins that start with a weight as the segments drawn from a bin
 * succeed (the grid-adaptive scheme of Margolis et al., "Rapid Locomotion via Reinforcement Learning", in exact integers).  The launches
 * of qg_cmdcur_advance_device go BEHIND the env-step (qg_walk_step_device / qg_po_step_device) on the same stream and write the walking
 * layer's command slots, as the layer's own sampler does after a step's reward and (PO) observation have been produced: the step that
 * follows rewards, and shows in its PO frames, the new command; the reset row a PO step wrote for a finished env shows, in its command
 * columns, the command of the segment that finished, as in the reference and with the in-kernel sampler.  No step kernel is involved.
 *
 * Grid.  Bin b = si * n_alpha + ai, si = 0 .. n_speed - 1, ai = 0 .. n_alpha - 1, B = n_speed * n_alpha <= 256 bins.  Formed on the host at
 * create in f64 and rounded once:  ws = f32((f64(speed_hi) - f64(speed_lo)) / n_speed);  wa = f32(2 pi / n_alpha).  Bin (si, ai) covers
 * speed from edge_s = f32(speed_lo + f32(f32(si) * ws)) and alpha from edge_a = f32(-pi32 + f32(f32(ai) * wa)), pi32 = f32(pi): one
 * product and one add each, no fma.
 *
 * State in device memory.  Per env: bin (i32), steps (i32, env-steps of the running segment), sum[4] (f32, one per criterion), segment
 * (i64, this handle's own counter, 0 in a new handle; NOT the simulator's episode).  Per handle: weight[2][B] (i32, a ping-pong pair;
 * the current half is gen & 1), gen (u32, bumped once per advance), episodes[B] and successes[B] (i64, cumulative counts of judged
 * segments by the bin they were drawn from).
 *
 * Keys.  qg_perturb's k(s), in a key space of its own, with the env's segment as the episode:
 *   seed_c = seed + 0x5147434D44435531                                        (mod 2^64; ASCII "QGCMDCU1")
 *   k(s): x = seed_c + 0xA0761D6478BD642F * s + 0x9E3779B97F4A7C15 * (env_index_base + i + 1) + 0xD1B54A32D192ED03 * (segment + 1);
 *         k = mix64(mix64(x)) >> 40
 * The draw of a new segment from weights w[0 .. B - 1]:
 *   T = sum w;  r = (k(0) * T) >> 24  (u64);  bin = the smallest b with w[0] + .. + w[b] > r, over ascending b  (a bin of weight 0 is
 *   never drawn; the share of bin b among the 2^24 values of k(0) is within one count of 2^24 w[b] / T)
 *   speed = f32(edge_s + f32(ws * f32(k(1) * 2^-24)));   alpha = f32(edge_a + f32(wa * f32(k(2) * 2^-24)))      no fma
 *   theta = fixed_heading ? heading_angle : f32(pi32 * (2 * f32(k(3) * 2^-24) - 1))
 *   then the tail of the walking layer's own sampler (one device function, shared): sincosf of theta and alpha, velocity
 *   (speed cos alpha, speed sin alpha), heading (cos theta, sin theta), global velocity = the velocity rotated by theta.
 *
 * qg_cmdcur_advance_device, for env i, in this order:
 *   1. steps += 1;  for each criterion k: sum[k] = f32(sum[k] + components[i][column_k]).  The done step's row is included.
 *   2. The segment ends where done names i or steps == R (R = 0: where done names i only).
 *   3. A segment that ends is judged: it succeeds iff steps >= min_steps and every criterion holds; criterion k holds iff
 *      sum[k] >= f32(threshold_k * f32(steps)) for sense +1, sum[k] <= that bound for sense -1; a NaN sum (or bound) fails; with
 *      n_criteria = 0 min_steps alone decides.  Then episodes[bin] += 1 and successes[bin] += success.
 *   4. Weights: with s_b the successes judged in THIS advance in bin b, every bin c gets
 *        weight[c] = min(weight_max, weight[c] + delta * sum over b in N(c) of s_b)        (i64)
 *      N(c) is a SET: c, its speed neighbours (si - 1, ai) and (si + 1, ai) where they exist (no wrap), its angle neighbours
 *      (si, ai - 1 mod n_alpha) and (si, ai + 1 mod n_alpha) (wrap); with n_alpha = 2 the two angle neighbours are one bin, counted
 *      once, and with n_alpha = 1 they are c itself.
 *   5. Every env whose segment ended: segment += 1, steps = 0, sums = 0, and a new draw from the UPDATED weights.
 *   6. command_out (nullable): row i = (vx, vy, hx, hy), the command in force after the advance, for EVERY env -- bit for bit what
 *      qg_walk_get_commands reports, without its wait.  The command of an env whose segment did not end keeps its bits.
 * It is two launches on the caller's stream and nothing else: the first judges and leaves per-block per-bin integer counts, the second
 * sums them in ascending block order in every block that needs them, forms the new weights and their prefix sums in LDS, draws, and
 * lets its first block store the new half of the ping-pong.  No floating-point atomics (no float is summed across envs), no workgroup
 * waits for another, no allocation, no wait for the device; capturable, and a replay advances the curriculum; the same inputs give the
 * same bits eagerly and under graph replay.  Refused (QG_ERR_ARG, before anything is launched): while the resident step mode is on
 * (qg_resident_stop first); a criterion column >= n_columns; criteria without components; bad strides or done kind.
 *
 * qg_cmdcur_begin_device (an explicit reset; one launch): the envs of the mask (all, when NULL) discard their running segment UNJUDGED --
 * no count, no weight changes -- and start a new one: segment += 1, steps = 0, sums = 0, a draw from the weights as they stand.
 *
 * While a curriculum is bound to a walking layer, qg_walk_set_command_sampler(non-NULL), a second qg_cmdcur_create on that layer and
 * qg_walk_destroy are refused; a layer with a sampler installed is refused at qg_cmdcur_create (the two would both redraw).  Commands
 * written by qg_walk_set_commands stand until the env's segment ends.  Shards do NOT reproduce one big handle: the weights depend on
 * every env's outcomes.  A multi-rank trainer merges its shards' weights through qg_cmdcur_get_weights / qg_cmdcur_set_weights.
 * Not covered: weight decay on failure, a curriculum over the heading, anything inside a qg_step_device_seq run.  Every entry point
 * but _advance_device and _begin_device waits for the device and must not be called during a capture.  Destroy the qg_cmdcur before
 * its qg_walk. */
#define QG_CMDCUR_MAX_SIDE 16
#define QG_CMDCUR_MAX_BINS 256
#define QG_CMDCUR_MAX_WEIGHT 65536
#define QG_CMDCUR_MAX_CRITERIA 4
typedef struct qg_cmdcur qg_cmdcur;
typedef struct qg_cmdcur_criterion {
    int32_t column;                    /* the column of `components` that is summed over the segment; >= 0, < n_columns at every advance */
    int32_t sense;                     /* +1: the mean per step must reach the threshold; -1: it must not exceed it */
    float threshold;                   /* per env-step; finite */
} qg_cmdcur_criterion;
typedef struct qg_cmdcur_desc {
    int32_t struct_size;               /* sizeof(qg_cmdcur_desc): checked */
    int32_t reserved;                  /* 0 */
    int32_t n_speed, n_alpha;          /* 1 .. QG_CMDCUR_MAX_SIDE each */
    float speed_lo, speed_hi;          /* finite, speed_lo <= speed_hi */
    int32_t fixed_heading;             /* 0: theta is drawn per segment; 1: theta = heading_angle */
    float heading_angle;               /* rad; finite */
    int32_t weight_max;                /* W: 1 .. QG_CMDCUR_MAX_WEIGHT */
    int32_t delta;                     /* 1 .. W */
    int32_t resample_steps;            /* R >= 0; 0: a segment ends with its episode only */
    int32_t min_steps;                 /* >= 1 */
    int32_t n_criteria;                /* 0 .. QG_CMDCUR_MAX_CRITERIA */
    int32_t reserved2;                 /* 0 */
    qg_cmdcur_criterion criteria[QG_CMDCUR_MAX_CRITERIA];
    int32_t initial_weights[QG_CMDCUR_MAX_BINS];     /* the first B: each in [0, W], at least one > 0 */
    uint64_t seed;
    uint64_t env_index_base;           /* env i of this handle is env env_index_base + i of the run */
} qg_cmdcur_desc;
/* Validation (QG_ERR_ARG) comes before the handle and the device are looked at.  Create draws segment 0 of every env from the initial
 * weights and writes the commands; it waits for the device. */
int qg_cmdcur_create(qg_walk *walk, const qg_cmdcur_desc *desc, qg_cmdcur **out);
int qg_cmdcur_destroy(qg_cmdcur *cur);
/* done: a done vector (QG_DONE_*), nullable.  components: [n] rows of n_columns floats at components_stride >= n_columns (nullable
 * where n_criteria is 0).  command_out: nullable, [n] rows of 4 floats at command_out_stride >= 4. */
int qg_cmdcur_advance_device(qg_cmdcur *cur, const void *done, int32_t done_kind, int32_t done_stride, const float *components,
                             int32_t components_stride, int32_t n_columns, float *command_out, int32_t command_out_stride, void *stream);
/* mask: nullable device [n] u8 (non-zero selects). */
int qg_cmdcur_begin_device(qg_cmdcur *cur, const uint8_t *mask, void *stream);
/* The current weights, host i32 [B]; set validates as create validates initial_weights and replaces the current half. */
int qg_cmdcur_get_weights(qg_cmdcur *cur, int32_t *weights);
int qg_cmdcur_set_weights(qg_cmdcur *cur, const int32_t *weights);
/* Host i64 [B] each, either nullable: judged segments and successes per bin since create (or the restored state). */
int qg_cmdcur_get_stats(qg_cmdcur *cur, int64_t *episodes, int64_t *successes);
/* Host arrays [n], each nullable: the running segments' bin, steps and segment counter. */
int qg_cmdcur_get_bins(qg_cmdcur *cur, int32_t *bin, int32_t *steps, int64_t *segment);
/* The whole state (per env and per handle) as ONE opaque blob of *bytes bytes (host pointer); the round trip is exact and a restored
 * handle of the same shape continues bit for bit.  The commands themselves are the walking layer's (qg_walk_get_state). */
int qg_cmdcur_state_bytes(const qg_cmdcur *cur, int64_t *bytes);
int qg_cmdcur_get_state(qg_cmdcur *cur, void *blob);
int qg_cmdcur_set_state(qg_cmdcur *cur, const void *blob);

#ifdef __cplusplus
}
#endif
#endif /* QUADGYM_H */
