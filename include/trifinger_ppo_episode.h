/* C ABI of the episode-end side of the in-repo PPO (leibnizgym_amd/csrc/libtrifinger_ppo.so: csrc/ppo_kernels.hip, gfx950): `episode_ends` and
 * `value_bootstrap` of the agent tree.  Conventions as in include/trifinger_ppo.h: plain pointers and sizes, every pointer DEVICE memory unless stated,
 * `stream` a hipStream_t, 0 on success, -1 invalid argument, -3 a launch failed.  tfp_api_version() stays 3: the entry points below are bound by symbol.
 * The Python binding is leibnizgym_amd/ppo_kernels.py; the torch statement of the same definitions is leibnizgym_amd/ppo.py (gae_with_ends, the module
 * docstring); tests/test_episode_ends_gpu.py holds every entry point against torch.
 *
 * Definitions.  All arithmetic is float32, every operation rounded separately in the order written (no contraction).  Per env step t of a rollout of T
 * steps, read from the engine's buffers after the step (the reset happens at the START of the next step launch, so the observation this step returned,
 * and hence val[t + 1], is the final state of the old episode):
 *     end[t]  = float(reset_buf != 0)                                       the episode ended in this step
 *     tout[t] = float(episode_length > 0 and steps >= episode_length)       the time limit was hit (it takes precedence over a termination on the same step)
 *     term[t] = end[t] * (1 - tout[t]) with value_bootstrap, end[t] without (RL-Games' default: a time-out counts as a terminal)
 *     w[t]    = 1 - end[t - 1],  w[0] = 1 - last_end                        0 for a STALE sample: its observation belongs to an episode that had ended
 *   last_end [n] is the end row of the final step of the previous rollout (zero after a reset of the env).
 * Generalised advantage estimation, t = T - 1 .. 0, last = 0:
 *     cont  = 1 - end[t]            boot = 1 - term[t]
 *     delta = rew[t] + gamma * val[t + 1] * boot - val[t]                   = ((rew + ((gamma * val[t + 1]) * boot)) - val[t])
 *     last  = delta + (gamma * tau) * cont * last                           = delta + (((gamma tau) * cont) * last)
 *     adv[t] = last * w[t]          ret[t] = adv[t] + val[t]
 *   With end = 0 and last_end = 0 every factor is 1.0f: the outputs are the bits of tfp_gae (and of tfp_gae_vnorm, ret_n and v_old_n included).
 *
 * tfp_rollout_flags: ONE launch in place of tfp_rollout_reward.  r [n] float, reset_bytes [n] one byte per env (torch.bool / uint8; any non-zero value is an
 *   end), steps [n] int64, episode_length (<= 0: no time limit); writes rew = r * scale, end and tout into the three [n] rows given (slot t of the rollout
 *   buffers).  The engine's buffers are only read.
 * tfp_gae_ends: one launch, one thread per env, the loop above.  rew, end, tout [T, n]; val [T + 1, n]; last_end [n]; value_bootstrap 0 / 1.
 *   mean_f == inv_std_f == NULL: val holds plain values; ret_n and v_old_n are not touched (they may be NULL).  Otherwise (both given, clip > 0) val is the
 *   raw output y of a value network that works in normalised units and everything is tfp_gae_vnorm's: v = clamp(y, -clip, clip) / inv_std_f + mean_f,
 *   ret_n = clamp((ret - mean_f) * inv_std_f, -clip, clip) from the MASKED ret, v_old_n = clamp(y[:T], -clip, clip).  Outputs adv, ret, w (and ret_n,
 *   v_old_n) [T, n].
 * tfp_ppo_loss_w / tfp_ppo_loss_vclip_w: tfp_ppo_loss / tfp_ppo_loss_vclip with a weight per sample.  In place of adv [B] they read adv_w [B, 2], (adv_i, w_i)
 *   interleaved and 8-byte aligned.  Every per-sample term - surrogate, value term, bounds term, KL statistic - and every per-sample gradient - d_mu, d_v,
 *   the sample's share of d_logstd - is multiplied by w_i, as the last operation on it: with w = 1 d_mu and d_v are the bits of the unweighted entry
 *   points, with w_i = 0 the rows of d_mu and d_v are zero.  The divisor stays B (not sum w) and the batch-independent entropy term is unchanged: with
 *   w = 0 throughout d_logstd is -ent_coef and the loss -ent_coef * ent.  Compile-time variants of the same kernel: the same accumulators and ticket, and
 *   therefore the same contract - ONE call of any of the four entry points at a time per device and process; tfp_reset_state() serves all of them. */
#ifndef TRIFINGER_PPO_EPISODE_H
#define TRIFINGER_PPO_EPISODE_H
#include "trifinger_ppo.h"
#ifdef __cplusplus
extern "C" {
#endif

int tfp_rollout_flags(const float* r, const void* reset_bytes, const int64_t* steps, float scale, int64_t episode_length, int32_t n, float* b_rew, float* b_end,
                      float* b_tout, void* stream);
int tfp_gae_ends(const float* rew, const float* end, const float* tout, const float* val, const float* last_end, int32_t value_bootstrap, const float* mean_f,
                 const float* inv_std_f, float clip, float gamma, float gamma_tau, int32_t T, int32_t n, float* adv, float* ret, float* w, float* ret_n,
                 float* v_old_n, void* stream);
int tfp_ppo_loss_w(const float* mu, const float* log_std, const float* act, const float* old_nlp, const float* adv_w, const float* old_mu,
                   const float* v, const float* ret, int32_t B, int32_t A, float e_clip, float v_coef, float ent_coef, float bounds_coef,
                   float* d_mu, float* d_v, float* d_logstd, float* loss_out, float* stats, void* stream);
int tfp_ppo_loss_vclip_w(const float* mu, const float* log_std, const float* act, const float* old_nlp, const float* adv_w, const float* old_mu,
                         const float* v, const float* ret, const float* old_v, int32_t B, int32_t A, float e_clip, float v_coef, float ent_coef,
                         float bounds_coef, float* d_mu, float* d_v, float* d_logstd, float* loss_out, float* stats, void* stream);

#ifdef __cplusplus
}
#endif
#endif
