/* C ABI of the symmetry augmentation of the in-repo PPO (leibnizgym_amd/csrc/libtrifinger_ppo.so: csrc/ppo_symmetry.hip and one more compile-time variant
 * of the objective in csrc/ppo_kernels.hip, gfx950): `params.config.symmetry_augmentation`.  Conventions as in include/trifinger_ppo.h: plain pointers and
 * sizes, every pointer DEVICE memory unless stated, `stream` a hipStream_t, 0 on success, -1 invalid argument, -3 a launch failed, -4 declined.
 * tfp_api_version() stays 3: the entry points below are bound by symbol.  The Python binding is leibnizgym_amd/ppo_kernels.py; the statement of the map is
 * leibnizgym_amd/symmetry.py (`apply`); tests/test_symmetry_gpu.py holds both entry points against torch.
 *
 * A TABLE of a w-wide array is 2 * w entries of 16 bytes on the device, image k = 1, 2 at entries [(k - 1) w, k w): per output column j
 *     { int32 ia, int32 ib, float ca, float cb }        out[j] = ca * x[ia] + cb * x[ib]     float32, both products and the sum rounded separately, in that order;
 *                                                       out[j] = ca * x[ia]                  where cb == 0 (-0, +-inf and NaN of a permuted column stay)
 * with 0 <= ia, ib < w (the caller's duty: the kernel reads x[ia] from its staged copy of the row).
 *
 * tfp_gather_rows_sym: tfp_gather_rows_norm's arguments and `table` (host array of n device pointers, or NULL = all NULL).  For `rows` indices it writes
 *   3 * rows output rows per array: dst[k] is [3 * rows, widths[k]] and its rows [i * rows, (i + 1) * rows), i = 0, 1, 2, hold the i-th image of
 *   src[k][idx[r], :], i = 0 the plain gather; an array with table[k] == NULL is copied for every i.  Statistics, where given, are applied AFTER the
 *   transform: the bits of tfp_gather_rows_norm on the transformed rows.  idx == NULL: identity.  One launch for up to 8 arrays.  Every source row is read
 *   once into registers (two columns per lane and array) and staged in LDS; per array and image the rows of 8 consecutive indices are ONE contiguous run
 *   of the output, which a workgroup writes with consecutive threads on consecutive floats; the tables are staged in LDS once per workgroup.
 *   -4: an array wider than 128 columns, or the arrays of the launch wider than 512 columns together.
 * tfp_ppo_loss_sym: the objective (tfp_ppo_loss and its three variants) with a row count of its own for the KL statistic.  old_v NULL or [B] (the value
 *   clip of tfp_ppo_loss_vclip); weighted 0: adv [B], 1: adv [B, 2] = (adv_i, w_i) interleaved, 8-byte aligned (tfp_ppo_loss_w); 1 <= kl_rows <= B: the KL
 *   statistic stats[3] sums over the rows i < kl_rows alone and is divided by kl_rows; every other term, gradient and divisor is untouched.  With
 *   kl_rows == B: the bits of the entry point that (old_v, weighted) selects.  A compile-time variant of the same kernel: the same accumulators and
 *   ticket, the same contract - ONE call of any of the five entry points at a time per device and process; tfp_reset_state() serves all of them. */
#ifndef TRIFINGER_PPO_SYMMETRY_H
#define TRIFINGER_PPO_SYMMETRY_H
#include "trifinger_ppo.h"
#ifdef __cplusplus
extern "C" {
#endif

#define TFP_SYM_MAX_WIDTH 128      /* columns of one array */
#define TFP_SYM_MAX_COLS 512       /* columns of all arrays of one launch together */

int tfp_gather_rows_sym(const void* const* src, void* const* dst, const int32_t* widths, const void* const* mean_f, const void* const* inv_std_f,
                        const float* clip, const void* const* table, int32_t n, const void* idx, int32_t rows, void* stream);
int tfp_ppo_loss_sym(const float* mu, const float* log_std, const float* act, const float* old_nlp, const float* adv, const float* old_mu,
                     const float* v, const float* ret, const float* old_v, int32_t weighted, int32_t kl_rows, int32_t B, int32_t A, float e_clip, float v_coef,
                     float ent_coef, float bounds_coef, float* d_mu, float* d_v, float* d_logstd, float* loss_out, float* stats, void* stream);

#ifdef __cplusplus
}
#endif
#endif
