/* C ABI of `params.config.mixed_precision` of the in-repo PPO: the network walk (csrc/ppo_mlp_walk.hip) and the direct weight-gradient kernel
 * (csrc/ppo_dw_direct.hip) with bf16 OPERANDS on v_mfma_f32_16x16x32_bf16 (leibnizgym_amd/csrc/libtrifinger_ppo.so, gfx950).  Conventions as in
 * include/trifinger_ppo.h: plain pointers and sizes, every pointer DEVICE memory unless stated, `stream` a hipStream_t, 0 on success, -1 invalid argument,
 * -2 / -3 a launch could not be set up / failed, -4 declined.  The Python binding is leibnizgym_amd/ppo_kernels.py; tests/test_mixed_precision_gpu.py holds
 * every entry point against float64 products of the rounded operands.  No API number changes and no existing entry point changes.
 *
 * With bf16r(t) = t rounded to bfloat16 (round to nearest even) and read back as float32, every Linear of a network becomes
 *     forward   y  = bf16r(x) bf16r(W)^T + b            products exact, accumulated in fp32; the bias added in fp32
 *     backward  gx = bf16r(gy) bf16r(W)
 *               gW = bf16r(gy)^T bf16r(x)
 *               gb = column sums of the UN-ROUNDED gy, fp32
 * (leibnizgym_amd/ppo.py: _MixedLinear is this statement in torch and the specification).  Everything else is what the fp32 entry points do, in fp32:
 * memory holds fp32 weights, inputs, saved layer outputs and dZ - nothing is stored in bf16; the rounding happens in registers where a lane assembles its
 * MFMA fragment (v_cvt_pk_bf16_f32).  Activations and their derivatives from the saved output, the input statistics (formed in fp32, then rounded as
 * the operand) and the [h | x] operand of d2rl (rounded elementwise) are unchanged.
 *
 * tfp_net_forward_bf16 / tfp_net_backward_bf16 / tfp_net_fits_bf16: arguments, limits and return codes of tfp_net_forward / tfp_net_backward / tfp_net_fits
 *     (include/trifinger_ppo_net.h: activation codes 0 .. 6, d2rl, optional statistics).  d2rl is NOT declined: the LDS operands stay fp32, so the budget is
 *     that of the fp32 walk.  backward: dZ_{l-1} = (bf16r(dZ_l) bf16r(W_l[:, :dim[l]])) * act'(h_l), the dZ_l read back from LDS un-rounded fp32 as stored.
 * tfp_gemm_tn_partials_direct_bf16: arguments and return codes of tfp_gemm_tn_partials_direct (include/trifinger_ppo.h): slabs of
 *     [bf16r(A)^T bf16r(B) | column sums of A in fp32], the same slab size (tfp_gemm_tn_partials_direct_chunk), the same fixed order of the sums through
 *     LDS, summed by tfp_sum_partials_multi as before: the same call twice gives the same bits.
 * The order of the k inside an MFMA differs from the fp32 kernels', so results agree with them to the rounding of the operands (2^-8 relative each), not
 * bit for bit. */
#ifndef TRIFINGER_PPO_MIXED_H
#define TRIFINGER_PPO_MIXED_H
#include "trifinger_ppo_net.h"
#ifdef __cplusplus
extern "C" {
#endif

int tfp_net_forward_bf16(const TfpNet* nets, int32_t n_nets, int32_t M, void* stream);
int tfp_net_backward_bf16(const TfpNet* nets, int32_t n_nets, int32_t M, void* stream);
int tfp_net_fits_bf16(const TfpNet* nets, int32_t n_nets, int32_t backward);
int tfp_gemm_tn_partials_direct_bf16(const void* const* A, const void* const* B, void* const* part, const int32_t* rows, const int32_t* N1, const int32_t* N2,
                                     int32_t n, void* stream);

#ifdef __cplusplus
}
#endif
#endif
