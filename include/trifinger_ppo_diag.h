/* C ABI of the training diagnostics of the in-repo PPO (leibnizgym_amd/csrc/libtrifinger_ppo.so: one more compile-time variant each of the objective and of
 * the optimiser in csrc/ppo_kernels.hip, gfx950): `params.config.diagnostics`.  Conventions as in include/trifinger_ppo.h: plain pointers and sizes, every
 * pointer DEVICE memory unless stated, `stream` a hipStream_t, 0 on success, -1 invalid argument, -3 a launch failed.  tfp_api_version() stays 3: the entry
 * points below are bound by symbol.  The Python binding is leibnizgym_amd/ppo_kernels.py; the statement of the record is leibnizgym_amd/ppo.py
 * (`diag_objective_statement`, `diag_optimiser_statement`); tests/test_ppo_diagnostics_gpu.py holds both entry points against it.
 *
 * THE RECORD is `long long diag[TFP_DIAG_N]` on the device, 8-byte aligned.  It ACCUMULATES across launches; the caller clears it (every slot 0 but
 * RATIO_MIN, whose cleared state is TFP_DIAG_RATIO_MIN_CLEAR; the trainer takes and clears it once per epoch).  Counters are integers, sums are fixed point, extremes are
 * bit patterns of non-negative floats (which order as integers): the bits of the record do not depend on the order of the workgroups or of the ranks.
 *
 * Slots 0-8 (the objective) are over the LIVE ROWS of a launch: i < B; w_i != 0 in the weighted form; i < kl_rows where kl_rows > 0 (with symmetry
 * augmentation the original rows alone: an image row's ratio is against the original sample's old_nlp and says nothing about the clip).  With
 *     l_i = old_nlp_i - nlp_i,   ratio_i = expf(l_i)   (the kernel's own),   k3_i = expm1f(l_i) - l_i
 * a live row whose l_i or ratio_i is not finite adds one to NONFINITE and to nothing else; every other live row adds
 *     ROWS      1
 *     CLIPPED   ratio_i < 1 - e or ratio_i > 1 + e
 *     ZERO_GRAD the surrogate's zero-gradient branch: not (`inside` or s1 > s2), the kernel's own selection
 *     VCLIPPED  the value term's clipped branch, !unclipped; 0 without old_v
 *     MU_OUT    the number of its A entries with mu > 1.1 or mu < -1.1
 *     K3_SUM    llrint(fminf(k3_i, 64) * 2^28)
 *     RATIO_MAX / RATIO_MIN   max / min with the bit pattern of ratio_i (a finite float >= 0)
 * Fixed point: one row adds at most 64 * 2^28 = 2^34 to K3_SUM, so an epoch of 8 ranks x 65536 envs x 32 steps x 4 mini-epochs = 2^26 rows stays below
 * 2^60 < 2^63; the resolution is 2^-28 = 3.7e-9 per row, below fp32's own error on k3 (expm1f(l) - l cancels to about 1e-8 absolute for |l| <= 0.5).
 *
 * Slots 9-15 (the optimiser), one optimiser step per call, norm_q = sqrtf(sq[2 par + q]) the pre-truncation norm of group q that k_clip_adam forms:
 *     STEPS     1
 *     TRUNC_q   the step's coefficient fminf(max_norm_q / (norm_q + 1e-6), 1) is < 1
 *     GN_q_SUM  llrint(fminf(norm_q, 2^16) * 2^24)       (a non-finite norm adds 2^40: fminf drops a NaN)
 *     GN_q_MAX  max with the bit pattern of fminf(norm_q, 2^16)
 * q = 0: the actor's group (A), q = 1: the central value network's (V).  With n0 == n1 there is one group: slots 11, 13 and 15 stay 0.  With a process
 * group the norms are those of the exchanged gradient, identical on every rank; they are not reduced.
 *
 * tfp_ppo_loss_diag: tfp_ppo_loss_sym's arguments and `diag`.  ONE entry point for the four cases (old_v NULL or [B]; weighted 0: adv [B], 1: adv [B, 2]
 *   = (adv_i, w_i) interleaved, 8-byte aligned); kl_rows == 0: every row - the KL statistic over all B rows with divisor B, the bits of the entry point
 *   (old_v, weighted) selects; 1 <= kl_rows <= B: tfp_ppo_loss_sym's statistic.  d_mu and d_v come out bit for bit as from that entry point; d_logstd,
 *   the loss and stats as from it up to the order of its float atomics.  Per block at most one 64-bit atomic per slot, none for a zero.  A compile-time
 *   variant (DIAG) of the same kernel: the same float accumulators and ticket, the same contract - ONE call of any of the objective's entry points at a
 *   time per device and process; tfp_reset_state() serves all of them (it does not touch a record).
 * tfp_clip_adam_diag: tfp_clip_adam's arguments and `diag`; the same two launches, the second as its DIAG variant: block 0 thread q < 2 updates slots
 *   10-15 of its group, thread 0 STEPS as well - one writer per slot, no atomics (ONE optimiser step at a time per record, the trainer's single stream).
 *   Parameters and moments come out bit for bit as from tfp_clip_adam. */
#ifndef TRIFINGER_PPO_DIAG_H
#define TRIFINGER_PPO_DIAG_H
#include "trifinger_ppo.h"
#ifdef __cplusplus
extern "C" {
#endif

enum {
    TFP_DIAG_ROWS = 0, TFP_DIAG_CLIPPED = 1, TFP_DIAG_ZERO_GRAD = 2, TFP_DIAG_VCLIPPED = 3, TFP_DIAG_MU_OUT = 4, TFP_DIAG_NONFINITE = 5,
    TFP_DIAG_K3_SUM = 6, TFP_DIAG_RATIO_MAX = 7, TFP_DIAG_RATIO_MIN = 8, TFP_DIAG_STEPS = 9, TFP_DIAG_TRUNC_A = 10, TFP_DIAG_TRUNC_V = 11,
    TFP_DIAG_GN_A_SUM = 12, TFP_DIAG_GN_V_SUM = 13, TFP_DIAG_GN_A_MAX = 14, TFP_DIAG_GN_V_MAX = 15, TFP_DIAG_N = 16
};
#define TFP_DIAG_RATIO_MIN_CLEAR 0x7F800000LL      /* the bit pattern of +inf: the cleared state of RATIO_MIN */
#define TFP_DIAG_K3_SCALE 268435456.0f             /* 2^28 */
#define TFP_DIAG_K3_MAX 64.0f
#define TFP_DIAG_GN_SCALE 16777216.0f              /* 2^24 */
#define TFP_DIAG_GN_MAX 65536.0f                   /* 2^16 */

int tfp_ppo_loss_diag(const float* mu, const float* log_std, const float* act, const float* old_nlp, const float* adv, const float* old_mu,
                      const float* v, const float* ret, const float* old_v, int32_t weighted, int32_t kl_rows, int32_t B, int32_t A, float e_clip, float v_coef,
                      float ent_coef, float bounds_coef, float* d_mu, float* d_v, float* d_logstd, float* loss_out, float* stats, void* stream, long long* diag);
int tfp_clip_adam_diag(float* p, const float* g, float* m, float* v, int32_t n0, int32_t n1, float* sq, float* step, const float* lr,
                       float max_norm0, float max_norm1, float beta1, float beta2, float eps, void* stream, long long* diag);

#ifdef __cplusplus
}
#endif
#endif
