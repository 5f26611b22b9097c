// qg_step_launch.h -- what the simulator units that enqueue steps (qg_capi.hip: one env-step; qg_sim_multi.hip: many per launch) and
// the step-kernel units (qg_kernel_link.hip, qg_kernel_quad.hip, qg_kernel_pair.hip) both read: what a launch takes, the grid predicates every step-kernel choice is made with, and the entry points
// of the units.  Each unit is a code object of its own and holds its kernels, their launchers and the leaves of its mapping: the core
// decides the mapping, the unit names the instantiation.  Internal: not installed, and nothing in here is exported (libquadgym.map).
#pragma once
#include "qg_sim.h"

// ---- step-kernel grids ------------------------------------------------------------------------------------------------------------
// The size predicates every step-kernel choice reads (po_fusable, the units' selectors, qg_step_device_seq); the launchers derive grid
// and block from the instantiation they launch, as the kernel's __launch_bounds__ does.
static int link_blocks(const qg_sim *s) { return (s->n + QGK_LINK_ENVS * QGK_LINK_WAVES - 1) / (QGK_LINK_ENVS * QGK_LINK_WAVES); }
static int quad_blocks(const qg_sim *s) { return (s->n + QGK_QUAD_ENVS - 1) / QGK_QUAD_ENVS; }    // one wave each
static int pair_blocks(const qg_sim *s) { return (s->n + QGK_PAIR_ENVS - 1) / QGK_PAIR_ENVS; }
// four-wave workgroups for grids of more than one wave per compute unit
static bool quad_wg4(const qg_sim *s) { return quad_blocks(s) > s->simds / 4; }
static bool pair_wg4(const qg_sim *s) { return pair_blocks(s) > s->simds / 4; }
// at most one wave per SIMD (256 CUs x 4 on an MI355X): give each wave the whole register file
static bool quad_one_wave(const qg_sim *s) { return quad_blocks(s) <= s->simds; }
static dim3 wave_grid(int waves, int per_group) { return dim3(per_group == 4 ? (waves + 3) / 4 : waves); }

// what every per-launch step kernel takes, and where it goes
struct StepLaunch {
    const qg_sim *s;
    const KModel *model;      // the model tables (per-env dynamics: the KModelDyn in front of the rows)
    KStepArgs P;
    hipStream_t stream;
    const KWalkLaunch *walk;
    const KPoLaunch *po;
};
template <bool WALK> static typename WalkArgT<WALK>::type walk_arg(const KWalkLaunch *w) {
    if constexpr (WALK) return *w;
    else return {};
}
template <bool PO> static typename PoArgT<PO>::type po_arg(const KPoLaunch *p) {
    if constexpr (PO) return *p;
    else return {};
}

// Which instantiation a launcher enqueued, for qg_debug_last_step_kernel: the family in the low nibble, then one nibble per template
// argument in declaration order (every argument is 0 .. 4).  A store of a constant on the launch path; the name is formatted on request.
enum StepFamily : uint32_t { KF_NONE, KF_LANE, KF_LINK, KF_QUAD, KF_PAIR, KF_LINK_MULTI, KF_QUAD_MULTI, KF_PAIR_MULTI };
template <int... A> static constexpr uint32_t step_kernel_code(StepFamily fam) {
    uint32_t code = fam, shift = 4;
    ((code |= (uint32_t)A << shift, shift += 4), ...);
    return code;
}

// ---- the units' entry points --------------------------------------------------------------------------------------------------------
// One env-step of the mapping qg_launch_step has decided on (`dyn`: per-env dynamics, which run the table-driven leaves of the LINK
// and QUAD mappings only); the launch error, if any, is left for the caller's hipGetLastError.
void qg_select_step_link(const StepLaunch &L, bool dyn);     // QG_MAP_LINK (qg_kernel_link.hip)
void qg_select_step_quad(const StepLaunch &L, bool dyn);     // QG_MAP_QUAD (qg_kernel_quad.hip)
void qg_select_step_pair(const StepLaunch &L);               // QG_MAP_PAIR (qg_kernel_pair.hip)
void qg_select_step_lane(const StepLaunch &L);               // QG_MAP_LANE (qg_kernel_quad.hip)
// `R.count` env-steps in one launch (qg_step_device_seq), each mapping's form on the grids the caller has checked
void qg_select_seq_link(const qg_sim *s, hipStream_t st, const KStepArgs &P, const KResident &R);
void qg_select_seq_quad(const qg_sim *s, hipStream_t st, const KStepArgs &P, const KResident &R);
void qg_select_seq_pair(const qg_sim *s, hipStream_t st, const KStepArgs &P, const KResident &R);
// the resident form of the one-link-per-lane kernel on the library's stream, its door control and the ring (qg_kernel_resident.hip)
void qg_select_resident(const qg_sim *s, const KStepArgs &P);
void qg_launch_resident_ctl(hipStream_t st, unsigned long long *door, int op);
void qg_launch_resident_ring(hipStream_t st, const KResident &R, unsigned count, unsigned nwaves, unsigned long long hint);

// Development builds (-DQG_PHASE_TIMES, tools/phase_times.sh): every unit's code object has a qg_phase_times[] of its own.  A unit's
// entry points leave its reader with the core, so qg_debug_phase_times copies out the stamps of the unit that launched last.
#ifdef QG_PHASE_TIMES
typedef hipError_t (*QgPhaseReader)(uint64_t out[16]);
void qg_phase_unit(QgPhaseReader reader);
// (a macro, so that a unit without device code -- qg_sim_multi.hip -- can include this file: it has no qg_phase_times to name)
#define QG_PHASE_UNIT() qg_phase_unit([](uint64_t out[16]) { return hipMemcpyFromSymbol(out, HIP_SYMBOL(qg_phase_times), 16 * sizeof(uint64_t)); })
#else
#define QG_PHASE_UNIT() ((void)0)
#endif
