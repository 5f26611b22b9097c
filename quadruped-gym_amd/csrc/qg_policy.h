// qg_policy.h -- what the translation units of the fused MLP policy share: the layer table their kernels read (qg_policy.hip: the
// forward pass; qg_policy_grad.hip: the PPO loss and gradient pass; qg_policy_distill.hip: the imitation loss and gradient pass;
// qg_policy_opt.hip: the optimiser step) and the handle.  Internal:
// not installed, nothing in here is exported.
#pragma once
#include <hip/hip_runtime.h>

#include "qg_host.h"

#define QGP_MAX_LAYERS 4          // n_hidden <= 3 hidden layers + the output layer
#define QGP_TILE 16               // envs per workgroup

struct KPolLayer {
    int32_t nq;                   // blocks of 16 input features (the input width, zero padded)
    int32_t nb;                   // blocks of 16 output features
    int32_t in_dim, out_dim;      // the real sizes (pack kernel)
    int32_t w_off, b_off;         // offsets (floats) into the packed image: W' [nb][nq][64][4], b' [nb][16]
    int32_t src_w, src_b;         // offsets (floats) into the canonical flat vector: W [out][in], b [out]
};

struct KPolicy {
    int32_t obs_dim, act_dim, n_layers, out_tanh, n_towers;
    int32_t std_off;              // packed: std[16] = exp(log_std), then log_std[16]
    int32_t src_log_std;          // canonical: log_std[act_dim]
    int32_t packed_floats;
    int32_t lds0_floats, lds1_floats;   // the two activation buffers (layer l reads buffer l & 1, writes the other)
    KPolLayer layer[2][QGP_MAX_LAYERS];
    int32_t critic_off;           // the critic's window: it reads columns [critic_off, critic_off + layer[1][0].in_dim) of a row (the
                                  // actor [0, obs_dim)); 0 and obs_dim on a handle of qg_policy_create.  Behind the table: what the
                                  // actor's launches read keeps its place in the kernel arguments
};

typedef float qgp_f32x4 __attribute__((ext_vector_type(4)));

// ---- the gradient pass (qg_policy_grad.hip) ------------------------------------------------------------------------------
#define QGG_SLOT_TILES 32         // 16-row tiles per partial-sum slot: a slot is 512 rows (FusedMlpPolicy.GRAD_SLOT_ROWS)
#define QGG_MISC 24               // f64 per tile / per slot: the log_std sums [0, 16), then the slots named below, 4 spare
#define QGG_MISC_POLICY 16        // the PPO pass: sum_rows of the policy term, of the kl estimate, of the clip count, of the value term
#define QGG_MISC_KL 17
#define QGG_MISC_CLIP 18
#define QGG_MISC_VALUE 19         // the last slot the weights launch adds, and only on a handle with a critic
#define QGD_MISC_LOSS 16          // the distillation pass, over the same slots: sum_rows w l, sum_rows w sum_a (mu - t)^2, sum_rows w
#define QGD_MISC_SQ 17
#define QGD_MISC_W 18
#define QGD_MISC_MAX 20           // tile_misc alone (the weights launch adds nothing past QGG_MISC_VALUE): max |mu - t| of the tile
#define QGG_HALF_LOG_2PI 0.91893853320467274178

struct KGradLayer {
    int32_t wt_off;               // offset (floats) into the transposed image: W^T' [nq][nb][64][4] (layers >= 1; layer 0 has none)
    int32_t h_off, d_off;         // offsets (floats) into a row's record: the layer's input [16 nq], its delta [16 nb]
    int32_t item0;                // first work item of the layer in the weight-gradient launch (ceil(nb / 4) x nq items)
};

struct KGrad {
    int32_t rec;                  // floats per row record: every layer's input and delta, both towers
    int32_t packed_t_floats;
    int32_t n_items;              // work items of the weight-gradient launch, the last one the sums of the per-tile scalars
    KGradLayer layer[2][QGP_MAX_LAYERS];
};

// ---- the optimiser step (qg_policy_opt.hip) -------------------------------------------------------------------------------
#define QGA_THREADS 256           // threads per workgroup of both launches
#define QGA_SLOT 2048             // canonical elements per workgroup: one f64 partial of the gradient norm (FusedMlpPolicy.ADAM_SLOT)
#define QGN_THREADS 1024          // the advantage normaliser's one workgroup

struct qg_policy {
    int32_t device;
    qg_policy_desc desc;
    KPolicy k;
    int32_t n_params;
    int32_t simds;
    int32_t force_waves;      // env QG_POLICY_WAVES at qg_policy_create: 1 or 4 waves per env tile whatever the size (A/B; 0: by size)
    QgDevMem mem;
    float *d_params;          // canonical flat vector (what qg_policy_get_params returns)
    float *d_packed;          // the operand image the forward kernel reads
    // qg_policy_reserve_grad: all null / zero until then
    KGrad g;
    int32_t grad_max;         // rows reserved
    float *d_packed_t;        // the transposed operand image (W_l^T delta_l)
    float *d_rec;             // [rows, padded to tiles][g.rec]: activations and deltas of a call
    double *d_tile_misc;      // [tiles][QGG_MISC]
    double *d_slot_misc;      // [slots][QGG_MISC]
    float *d_partial;         // [slots][n_params]
    // qg_policy_reserve_adam: all null / zero until then
    int32_t adam_slots;       // ceil(n_params / QGA_SLOT)
    float *d_adam_m;          // [n_params] first moment
    float *d_adam_v;          // [n_params] second moment
    long long *d_adam_t;      // the step count, in device memory: a captured step replays as t = 1, 2, 3, ..
    double *d_adam_partial;   // [adam_slots] sums of squares of the gradient
};

// the columns of an observation row the handle's launches read: obs_dim where the critic is not launched, else the farther end of
// the two towers' windows
static inline int32_t qg_policy_row_width(const qg_policy *p, bool with_critic) {
    const int32_t end = (with_critic && p->k.n_towers == 2) ? p->k.critic_off + p->k.layer[1][0].in_dim : 0;
    return end > p->desc.obs_dim ? end : p->desc.obs_dim;
}

// the transposed image from the canonical vector, on `st`; a no-op before qg_policy_reserve_grad (qg_policy_grad.hip)
int qg_policy_pack_transposed(qg_policy *p, hipStream_t st);
