/* trifinger_plan.h - C ABI of the planning library (libtrifinger_plan.so): a per-env fork of engine states across engines of different size, and the
 * three launches of sampling-based model-predictive control (MPPI) on a population of forked envs.
 *
 * An extension: the reference has no such interface.  The library shares no object with libtrifinger_hip.so and steps nothing itself: it reads and
 * writes the buffers the caller bound to its engines (TfBuffers of trifinger.h, handed over as TfplSide) and the caller runs tf_step between its
 * launches.  One control step of a planner over E plant envs with S samples each and horizon H is
 *     tfpl_fork (src_index[i] = i / S)  ->  H x ( tfpl_rollout_actions(h), tf_step(action) )  ->  tfpl_rollout_actions(H)  ->  tfpl_update.
 *
 * Conventions: plain C, no handle, raw device pointers, streams as void* (hipStream_t; NULL = the default stream).  Return value: TFPL_OK (0),
 * TFPL_ERR_INVALID_ARG (-1), TFPL_ERR_LAUNCH (-3: the launch failed; tfpl_last_error_string has the text).  Nothing allocates, synchronises or reads
 * device memory on the host.  Every entry point is one launch and touches rows [0, N) of its arrays only.
 *
 * WHEN A FORK EQUALS ITS SOURCE.  Env id, population size and lane position do not enter the physics of the step, so env i of the destination, stepped
 * with the action env src_index[i] of the source is stepped with, reproduces it bit for bit - as long as no env-keyed draw happens: a reset (the
 * samplers are keyed by the global env id), observation noise (dr_obs_noise) or action repeat (dr_action_repeat).  Frame-count-keyed reward
 * schedules follow the destination's frame count (tf_set_frame_count).
 *
 * THE NOISE.  Planner env i = e * S + s (group e < E, sample s < S), horizon step h < H, action component a < A:
 *     b = a / 12, k = (a % 12) / 4, j = a % 4
 *     r[0..3] = philox4x32_10(counter = (i, plan_counter, 4 h + k, b), key = (seed & 0xffffffff, seed >> 32))
 *     u[0..3] = (float)(r[.] >> 8) * 2^-24
 *     (n[0], n[1]) = box_muller(u[0], u[1]),  (n[2], n[3]) = box_muller(u[2], u[3]);   eps(i, h, a) = n[j]
 *     box_muller(ua, ub) = (rad * c, rad * s) with rad = sqrt(-2 * tf_log(1 - ua)), (s, c) = tf_sincos(6.2831855f * ub)
 * (tf_log, tf_sincos: the step's own polynomials; sqrt is IEEE).  With A = 9 the counters are (i, plan_counter, 4 h + k, 0), k = 0..2: three calls, twelve
 * normals, the first nine used.  Sample s = 0 of every group has eps = 0: it rolls out the nominal sequence.  The action of (i, h) is
 *     act(i, h, a) = min(max(U[e][h][a] + sigma * eps(i, h, a), lo), hi)              (product and sum rounded separately, fp32)
 * The noise is never stored: tfpl_update forms it again from the same counters.
 */
#ifndef TRIFINGER_PLAN_H
#define TRIFINGER_PLAN_H

#include <stdint.h>

#include "trifinger.h"

#ifdef __cplusplus
extern "C" {
#endif

#define TFPL_API_VERSION 1
#define TFPL_MAX_ACTION_DIM 24        /* two Philox blocks of twelve normals */
#define TFPL_MAX_HORIZON 256
#define TFPL_MIN_SAMPLES 64           /* S is a multiple of 64 in [64, 1024]: one workgroup of S lanes per group in tfpl_update */
#define TFPL_MAX_SAMPLES 1024
#define TFPL_STD_TINY 1e-12f          /* floor of the return's standard deviation in the weights */

enum { TFPL_OK = 0, TFPL_ERR_INVALID_ARG = -1, TFPL_ERR_LAUNCH = -3 };
/* per group, tfpl_update's stats[E][TFPL_NUM_STATS] */
enum { TFPL_STAT_BEST = 0, TFPL_STAT_MEAN = 1, TFPL_STAT_ESS = 2, TFPL_STAT_STD = 3, TFPL_NUM_STATS = 4 };

/* One engine as the library sees it: the buffers bound with tf_bind (info and scratch are not per-env and are never touched) and their widths. */
typedef struct TfplSide {
    TfBuffers buf;            /* DEVICE pointers; states may be NULL when states_dim == 0 */
    int32_t num_envs;         /* 1..TF_MAX_ENVS */
    int32_t action_dim;       /* A: action_buf is [N][A], obs [N][TF_OBS_DIM_BASE + A] */
    int32_t states_dim;       /* 0, or the width of `states` */
} TfplSide;

typedef struct TfplPlan {
    int32_t groups;           /* E >= 1 */
    int32_t samples;          /* S: multiple of 64, 64..1024;  E * S <= TF_MAX_ENVS */
    int32_t horizon;          /* H: 1..TFPL_MAX_HORIZON */
    int32_t action_dim;       /* A: 1..TFPL_MAX_ACTION_DIM */
    uint64_t seed;            /* the Philox key */
    uint32_t plan_counter;    /* counter word 1: the caller advances it once per tfpl_update, so no two plans share noise */
    float sigma;              /* >= 0 */
    float lo, hi;             /* the box every action is clamped into, lo <= hi */
    float lambda;             /* temperature of the weights, > 0 */
    int32_t normalize;        /* 1: the temperature is lambda * max(std of the group's returns, TFPL_STD_TINY); 0: lambda alone */
    int32_t shift;            /* 1: U is written back shifted by one step (receding horizon, last entry repeated); 0: as it is */
} TfplPlan;

int tfpl_api_version(void);
const char* tfpl_last_error_string(void);

/* For every destination env i < dst->num_envs with s = src_index[i]: env s's share of every per-env buffer of `src` is copied into env i of `dst` -
 * all TF_STATE_ROWS rows of the state (row r of env s is src.state[r * N_src + s]), the rows of action_buf, obs, states (when states_dim > 0) and reward,
 * the four flag bytes, steps and reset_count.  src_index: DEVICE int32 [N_dst].  An index outside [0, N_src) is not dereferenced: that env is left as it was
 * and *bad_count (DEVICE uint32, caller-zeroed, may be NULL) is incremented once for it.  The launch is laid out for src_index[i] = i / S: a wavefront
 * of 64 consecutive destination envs reads one source address per state row and stores a full line; the row-major buffers are copied element-flat
 * (consecutive lanes store consecutive floats).
 * TFPL_ERR_INVALID_ARG: a NULL side, src_index or required buffer, unequal action_dim or states_dim, num_envs outside [1, TF_MAX_ENVS].
 * ALIASING.  dst and src may be the same engine only if every source is a fixed point of the map, src_index[src_index[i]] == src_index[i] (a source env
 * is then overwritten with itself while others read it); any other map on one engine is a race, and it is the caller who must rule it out. */
int tfpl_fork(const TfplSide* dst, const TfplSide* src, const int32_t* src_index, uint32_t* bad_count, void* stream);

/* In front of horizon step h (0 <= h <= H), for every planner env i < E * S, in this order:
 *   h == 0:  G[i] = 0, alive[i] = 1
 *   h >= 1:  (closes step h - 1)  if alive[i]:  G[i] = G[i] + disc[h - 1] * reward[i]     (product and sum rounded separately)
 *                                              if reward[i] is not finite: alive[i] = 0   (G[i] is then not finite: the sample is INVALID)
 *            alive[i] = alive[i] & !reset_buf[i]
 *            so an env whose episode ended inside the horizon keeps the return it had, that step included.
 *   h <  H:  action[i][a] = act(i, h, a) for a < A (above)
 * U: DEVICE float [E][H][A].  disc: DEVICE float [H], disc[h] = gamma^h formed by the caller.  reward: DEVICE float [N], reset_buf: DEVICE uint8 [N] (the
 * rollout engine's; read for h >= 1 only).  G: DEVICE float [N], alive: DEVICE uint8 [N], action: DEVICE float [N][A] (not written for h == H). */
int tfpl_rollout_actions(const TfplPlan* plan, int32_t h, const float* U, const float* disc, const float* reward, const uint8_t* reset_buf, float* G,
                         uint8_t* alive, float* action, void* stream);

/* One workgroup of S lanes per group e.  Over the VALID samples of the group (G finite; n_valid of them), all in fp32:
 *   Gmax = max G;  mean = sum G / n_valid;  std = sqrt(sum (G - mean)^2 / n_valid)                 (population std, two passes)
 *   z_s = (G_s - Gmax) / T,  T = lambda * max(std, TFPL_STD_TINY) with normalize, else lambda
 *   w_s = exp(z_s) / sum exp(z);  w_s = 0 for an invalid sample
 *   U_new[e][h][a] = sum_s w_s * act(e S + s, h, a)                                                (the actions that were applied, noise regenerated)
 *   first[e][:] = U_new[e][0];  U[e][h] <- U_new[e][min(h + 1, H - 1)] with shift, else U_new[e][h]
 *   stats[e] = (Gmax, mean, 1 / sum w^2, std)
 * A group without a valid sample leaves U as it was, first[e] = U[e][0], w = 0, stats[e] = (0, 0, 0, 0), and invalid_count[e] = S.
 * U: DEVICE float [E][H][A], in place.  first: DEVICE float [E][A].  w: DEVICE float [E * S].  stats: DEVICE float [E][TFPL_NUM_STATS].  invalid_count:
 * DEVICE uint32 [E], the number of invalid samples of the group (written, not accumulated).  Sums run over lanes, then over wavefronts in index order. */
int tfpl_update(const TfplPlan* plan, const float* G, float* U, float* first, float* w, float* stats, uint32_t* invalid_count, void* stream);

#ifdef __cplusplus
}
#endif
#endif
