/* C ABI of the value side of the in-repo PPO (leibnizgym_amd/csrc/libtrifinger_ppo.so: csrc/ppo_kernels.hip, gfx950): `clip_value` and `normalize_value` of
 * the agent tree.  Conventions as in include/trifinger_ppo.h: plain pointers and sizes, every pointer DEVICE memory unless stated, `stream` a hipStream_t,
 * 0 on success, -1 invalid argument, -3 a launch failed.  tfp_api_version() stays 3: the entry points below are bound by symbol.  The Python binding is
 * leibnizgym_amd/ppo_kernels.py; tests/test_value_path_gpu.py holds both entry points against torch. */
#ifndef TRIFINGER_PPO_VALUE_H
#define TRIFINGER_PPO_VALUE_H
#include "trifinger_ppo.h"
#ifdef __cplusplus
extern "C" {
#endif

/* tfp_ppo_loss_vclip: tfp_ppo_loss with one more input, old_v [B] - the value recorded in the rollout - and the value term clipped around it, e = e_clip:
 *     vc  = old_v + clamp(v - old_v, -e, e)        L_u = (v - ret)^2        L_c = (vc - ret)^2
 *     c_i = L_u  when |v - old_v| <= e or L_u >= L_c,  L_c otherwise        (max(L_u, L_c) outside the range; inside it the two agree to rounding: L_u)
 *     d c_i / d v = 2 (v - ret) on the first branch, 0 on the second        c_loss = mean_i c_i
 *   Everything else - surrogate, bounds loss, entropy, KL, v_coef, the outputs and stats [4] - is tfp_ppo_loss.  A compile-time variant of the same kernel
 *   (tfp_ppo_loss launches the instantiation without the branch): the same reductions, the same accumulators and ticket, and therefore the same contract -
 *   ONE call of tfp_ppo_loss OR tfp_ppo_loss_vclip at a time per device and process; tfp_reset_state() serves both.
 * tfp_gae_vnorm: tfp_gae for a value network that emits NORMALISED values (`normalize_value`).  y [T + 1, n] is its raw output, mean_f / inv_std_f [1] the
 *   published floats of the returns' record (device memory: no host value enters the launch), clip > 0.  One launch, one thread per env:
 *     v       = clamp(y, -clip, clip) / inv_std_f + mean_f                  quotient and sum rounded separately
 *     adv, ret: the arithmetic of tfp_gae on v, operation for operation     (reward units)
 *     ret_n   = clamp((ret - mean_f) * inv_std_f, -clip, clip)              the critic's regression target
 *     v_old_n = clamp(y[:T], -clip, clip)                                   the old value of tfp_ppo_loss_vclip - NOT a round trip through v
 *   all four [T, n], every operation rounded as in the torch expressions above: the buffers hold the same bits. */
int tfp_ppo_loss_vclip(const float* mu, const float* log_std, const float* act, const float* old_nlp, const float* adv, const float* old_mu,
                       const float* v, const float* ret, const float* old_v, int32_t B, int32_t A, float e_clip, float v_coef, float ent_coef,
                       float bounds_coef, float* d_mu, float* d_v, float* d_logstd, float* loss_out, float* stats, void* stream);
int tfp_gae_vnorm(const float* rew, const float* done, const float* y, const float* mean_f, const float* inv_std_f, float clip, float gamma, float gamma_tau,
                  int32_t T, int32_t n, float* adv, float* ret, float* ret_n, float* v_old_n, void* stream);

#ifdef __cplusplus
}
#endif
#endif
