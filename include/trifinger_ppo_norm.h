/* C ABI of the input normalisation of the in-repo PPO (leibnizgym_amd/csrc/libtrifinger_ppo.so: csrc/ppo_norm.hip and the statistics variant of the forward
 * network walk in csrc/ppo_mlp_walk.hip, gfx950).  Conventions as in include/trifinger_ppo.h: plain pointers and sizes, every pointer DEVICE memory unless
 * stated, `stream` a hipStream_t, 0 on success, -1 invalid argument, -3 a launch failed, -4 declined (the caller takes another path).  The Python binding is
 * leibnizgym_amd/ppo_kernels.py; tests/test_input_norm_gpu.py holds every entry point against torch. */
#ifndef TRIFINGER_PPO_NORM_H
#define TRIFINGER_PPO_NORM_H
#include "trifinger_ppo.h"
#ifdef __cplusplus
extern "C" {
#endif

/* Input normalisation (`normalize_input` / `central_value_config.normalize_input` of asymm.yaml; csrc/ppo_norm.hip).  A statistics record of a D-wide input
 * is 1 + 2 D doubles on the device: {count, mean[D], M2[D]}, M2 = sum of squared deviations, variance = M2 / count (population).  The networks read its fp32
 * images mean_f = (float)mean and inv_std_f = (float)(1 / sqrt(M2 / count + 1e-5)) - count 0 publishes variance 1 - and the normalised input is
 *     y = min(max((x - mean_f) * inv_std_f, -clip), clip)      fp32, difference and product rounded separately: torch.clamp((x - mean_f) * inv_std_f, -clip, clip)
 * bit for bit, from every entry point below (the walk on raw rows with statistics and the plain walk on rows normalised by the gather give the same bits).
 *
 * tfp_moments: the batch records of n <= 2 row-major float arrays x[k] [rows, D[k]] into out = {record of x[0], record of x[1]} (1 + 2 D[0] + 1 + 2 D[1]
 *   doubles).  fp64 accumulation on data shifted by a value of its own slab, rows partitioned over workgroups in slabs of 256, partials merged by Chan's formula
 *   in a fixed tree, no atomics: the same input gives the same bits on every call.  `part`: the caller's scratch of tfp_moments_part_doubles(D, n, rows) doubles.
 *   -4: a row wider than 256 floats (the caller computes the moments itself).
 * tfp_norm_merge: merges the k >= 1 batch records batch[q] + j * stride (j = 0 .. k - 1, in this order; doubles) into the running record run[q] of n <= 2 inputs
 *   and publishes mean_f[q] / inv_std_f[q]; one launch.  A distributed run passes the gathered records of all ranks (stride = the length of a rank's vector).
 * tfp_gather_rows_norm: tfp_gather_rows with statistics: array k with mean_f[k] != NULL leaves normalised (clip[k] > 0; host array), any other one is copied;
 *   mean_f may be NULL (all copied).  idx == NULL: identity, dst[k][i, :] = norm(src[k][i, :]) - the standalone normaliser of the per-layer path.
 * tfp_mlp_forward_norm: tfp_mlp_forward with statistics per network (norm[i].mean == NULL: none), applied where the walk stages its input rows: the rollout
 *   reads the env's live observation buffers, no gather in between.  A compile-time variant of the forward walk; tfp_mlp_forward launches the code it always did.
 *   The backward walk needs nothing: it does not form the first layer's input gradient, and that layer's weight gradient reads the gather's normalised copy. */
typedef struct {
    const float* mean;        /* mean_f [dim[0]]; NULL: the network reads its input as it is */
    const float* inv_std;     /* inv_std_f [dim[0]] */
    float clip;               /* > 0 */
} TfpNorm;
int64_t tfp_moments_part_doubles(const int32_t* D, int32_t n, int32_t rows);
int tfp_moments(const void* const* x, const int32_t* D, int32_t n, int32_t rows, void* part, int64_t part_doubles, void* out, void* stream);
int tfp_norm_merge(void* const* run, const void* const* batch, const int32_t* D, int32_t n, int32_t k, int32_t stride, void* const* mean_f,
                   void* const* inv_std_f, void* stream);
int tfp_gather_rows_norm(const void* const* src, void* const* dst, const int32_t* widths, const void* const* mean_f, const void* const* inv_std_f,
                         const float* clip, int32_t n, const void* idx, int32_t rows, void* stream);
int tfp_mlp_forward_norm(const TfpMlp* nets, const TfpNorm* norm, int32_t n_nets, int32_t M, void* stream);

#ifdef __cplusplus
}
#endif
#endif
