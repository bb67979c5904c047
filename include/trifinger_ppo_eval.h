/* C ABI of the checkpoint evaluator: episode statistics of a population of envs, accumulated on the device (leibnizgym_amd/csrc/libtrifinger_ppo.so:
 * csrc/tf_eval.hip, gfx950).  Conventions as in include/trifinger_ppo.h: plain pointers and sizes, every pointer DEVICE memory, `stream` a hipStream_t,
 * 0 on success, -1 invalid argument, -3 a launch failed.  The Python binding is leibnizgym_amd/ppo_kernels.py, the user leibnizgym_amd/evaluate.py;
 * tests/test_episode_stats_gpu.py holds the kernel against the plain-torch form of the same definitions.
 *
 * tfp_eval_step is ONE launch per env step, issued behind tf_step on the same stream.  It only READS the env's buffers (include/trifinger.h: TfBuffers) -
 *   state [TF_STATE_ROWS][N] (rows TF_S_CUBE_P, TF_S_CUBE_Q, TF_S_GOAL_P, TF_S_GOAL_Q), reward [N], reset_buf [N] and goal_reset_buf [N] (bytes),
 *   steps [N] (int64) - and writes two buffers of the caller, both zeroed by the caller before an evaluation:
 *     env_acc  int32 [TFP_EVAL_ENV_ROWS][N], structure of arrays, per env: the running return of the episode (the bits of a float32, summed in step
 *              order: ret = ret + reward), the number of at-goal steps, the first at-goal step (1-based, 0: none yet), the number of finished episodes;
 *     acc      int64 [TFP_EVAL_ACC], the layout below.  INTEGERS only: integer sums commute, so the vector is the same bit for bit on every run, for every
 *              order of the workgroups, and after a sum over ranks.
 *   The call allocates nothing, synchronises nothing and keeps no state in the library: two evaluations on two streams do not interfere.  Nobody may
 *   read `acc` before the stream is synchronised.
 *
 * Per env and step: e_p = |cube_p - goal_p|, e_o = quat_diff_rad(cube_q, goal_q) - the step's own device functions and expressions, compiled with the
 *   step's arithmetic flags, so pos_ok = e_p <= pos_tol and ori_ok = e_o <= ori_tol are the step's predicates bit for bit - and at_goal by `rule`:
 *   0 position, 1 both, 2 orientation (__check_termination of the reference: difficulty < 4, == 4, > 4).  An env is UNDER ITS CAP while it has finished
 *   fewer than max_episodes_per_env episodes (0: no cap).  An env under its cap adds its goal_reset_buf to GOAL_EVENTS.  An env whose reset_buf is set
 *   ends an episode at this step (the reset itself happens at the start of the next step launch: the state rows still hold the final pose, steps[i] is
 *   the episode's length).  Under its cap the episode enters the counters, sums and histograms if its return, e_p, e_o and the two quaternions are all
 *   finite, and NONFINITE alone otherwise (the quaternions are tested themselves: the step's quat_diff_rad maps a non-finite product to pi); its episode
 *   count goes up by one, and the env that thereby reaches the cap adds one to ENVS_COMPLETE.  The per-env accumulators of an ending env are cleared,
 *   capped or not; a capped env goes on running and its episodes are not counted.
 *
 * Fixed-point sums: q = __float2ll_rn(x * S), S a power of two (the product is exact), x clamped first:
 *     SUM_RETURN   S = 2^16, |x| <= 2^25 (3.3e7 reward units)   |q| <= 2^41
 *     SUM_POS_ERR  S = 2^30,  x  <= 2^10 m                        q  <= 2^40
 *     SUM_ORI_ERR  S = 2^28,  x  <= 4 rad (e_o <= pi)             q  <= 2^30
 *   so 2^21 episodes (TF_MAX_ENVS envs, one each) at the bound stay below 2^62.
 * Histograms: the bin is a function of the float32 bit pattern alone, q = bits(x) >> 21 - four bins per octave, edges at the mantissa quarters:
 *     position error     TFP_EVAL_POS_BINS = 50: bin 0 for q < 460 (x < 2^-12 m, zero included), bin 1 + q - 460 for 460 <= q < 508, bin 49 for q >= 508 (x >= 1 m)
 *     orientation error  TFP_EVAL_ORI_BINS = 42: the same with 476 (2^-8 rad) and 516 (4 rad)
 *   The lower edge of bin b >= 1 is the float with the pattern (lo + b - 1) << 21. */
#ifndef TRIFINGER_PPO_EVAL_H
#define TRIFINGER_PPO_EVAL_H
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif

enum { TFP_EVAL_ENV_RETURN = 0, TFP_EVAL_ENV_AT_GOAL_STEPS = 1, TFP_EVAL_ENV_FIRST_HIT = 2, TFP_EVAL_ENV_EPISODES = 3, TFP_EVAL_ENV_ROWS = 4 };

#define TFP_EVAL_POS_BINS 50
#define TFP_EVAL_ORI_BINS 42
#define TFP_EVAL_POS_Q_LO 460
#define TFP_EVAL_POS_Q_HI 508
#define TFP_EVAL_ORI_Q_LO 476
#define TFP_EVAL_ORI_Q_HI 516
enum {
    TFP_EVAL_EPISODES = 0,            /* finished episodes that entered the sums and histograms                        */
    TFP_EVAL_NONFINITE = 1,           /* finished episodes with a non-finite return or final error: counted here only   */
    TFP_EVAL_POS_OK = 2,              /* episodes whose final step had pos_ok                                           */
    TFP_EVAL_ORI_OK = 3,              /* ... ori_ok                                                                     */
    TFP_EVAL_SUCCESS = 4,             /* ... at_goal                                                                    */
    TFP_EVAL_REACHED = 5,             /* episodes with at least one at-goal step                                        */
    TFP_EVAL_GOAL_EVENTS = 6,         /* goal_reset_buf set, over all steps of envs under their cap                     */
    TFP_EVAL_ENVS_COMPLETE = 7,       /* envs that reached max_episodes_per_env                                         */
    TFP_EVAL_SUM_LENGTH = 8,          /* sum of steps[i] at the end of the counted episodes                             */
    TFP_EVAL_SUM_AT_GOAL_STEPS = 9,
    TFP_EVAL_SUM_FIRST_HIT = 10,      /* over the reached episodes                                                      */
    TFP_EVAL_SUM_RETURN = 11,         /* fixed point, S = 2^16                                                          */
    TFP_EVAL_SUM_POS_ERR = 12,        /* fixed point, S = 2^30                                                          */
    TFP_EVAL_SUM_ORI_ERR = 13,        /* fixed point, S = 2^28                                                          */
    TFP_EVAL_HIST_POS = 14,           /* TFP_EVAL_POS_BINS bins                                                         */
    TFP_EVAL_HIST_ORI = TFP_EVAL_HIST_POS + TFP_EVAL_POS_BINS,
    TFP_EVAL_ACC = TFP_EVAL_HIST_ORI + TFP_EVAL_ORI_BINS
};

/* rule: 0 position, 1 position and orientation, 2 orientation.  -1: NULL pointer, N outside [1, TF_MAX_ENVS], rule outside 0..2, negative cap,
 * a tolerance that is NaN */
int tfp_eval_step(const void* state, const void* reward, const void* reset_buf, const void* goal_reset_buf, const void* steps, void* env_acc, void* acc,
                  int32_t N, float pos_tol, float ori_tol, int32_t rule, int32_t max_episodes_per_env, void* stream);

/* The tests' window into the predicates (no use in the product path): adds the number of envs with pos_ok to out[0] and with ori_ok to out[1] (int64 [2],
 * zeroed by the caller), from the device code tfp_eval_step runs.  tests/test_episode_stats_gpu.py compares them with the step's own counts. */
int tfp_eval_test_predicates(const void* state, int32_t N, float pos_tol, float ori_tol, void* out, void* stream);

#ifdef __cplusplus
}
#endif
#endif
