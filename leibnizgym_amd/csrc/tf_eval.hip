// tf_eval.hip - episode statistics of a population of envs, one launch per env step behind the fused step (include/trifinger_ppo_eval.h), gfx950.
//
// One env per lane, 256-thread workgroups, grid = ceil(N / 256) (TF_MAX_ENVS gives at most 8192 workgroups: no grid-stride loop).  A lane reads its env's
// cube and goal pose out of the SoA state (14 coalesced row loads: a wavefront reads one 256-byte line per row), the reward, the two flags and the step
// count, and updates its four int32 of `env_acc` - about 100 bytes per env and step against the step's ~1.5 KB.  The final errors are formed by the step's
// own device functions (tf_device_math.h) in the step's own expressions (tf_roles.h: o_dist / o_ang) and this unit is compiled with the step's
// arithmetic flags, so the predicates are the step's bit for bit.
//
// A workgroup in which nobody ends an episode and no goal event falls (one __syncthreads_or) leaves after the per-env update.  Otherwise - and after a
// reset of all envs EVERY env ends in the same launch, the burst is the normal case - the counters are popcounts of wavefront ballots, the sums 64-bit
// shuffle reductions over the wavefront, both added over the four wavefronts through LDS; the two histograms are binned with LDS integer atomics; and the
// workgroup issues ONE global 64-bit integer atomicAdd per non-zero quantity.  No float atomics, no hand-off between workgroups: nobody reads `acc`
// before the stream is synchronised.  Everything in `acc` is an integer, so the order of the workgroups does not show in its bits.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "tf_device_math.h"
#include "../../include/trifinger_ppo_eval.h"
#include "../../include/trifinger_ppo_track.h"
#include "../../include/trifinger_ppo_record.h"

#define EV_THREADS 256
#define EV_WAVES (EV_THREADS / 64)
#define EV_SCALARS TFP_EVAL_HIST_POS            // counters and sums in front of the histograms
#define EV_BINS (TFP_EVAL_POS_BINS + TFP_EVAL_ORI_BINS)

typedef unsigned long long u64;

struct EvalArgs {
    const float* state; const float* reward; const uint8_t* reset_buf; const uint8_t* goal_reset_buf; const long long* steps;
    int* env_acc; u64* acc;
    int N; float pos_tol, ori_tol; int rule, cap;
};

// final position / orientation error of env i; `qfinite`: both quaternions are finite (quat_diff_rad clamps a non-finite product to pi)
DEV void eval_errors(const float* __restrict__ state, int N, int i, float& e_p, float& e_o, bool& qfinite) {
    float cp[3], cq[4], gp[3], gq[4];
#pragma unroll
    for (int j = 0; j < 3; ++j) { cp[j] = state[(size_t)(TF_S_CUBE_P + j) * N + i]; gp[j] = state[(size_t)(TF_S_GOAL_P + j) * N + i]; }
#pragma unroll
    for (int j = 0; j < 4; ++j) { cq[j] = state[(size_t)(TF_S_CUBE_Q + j) * N + i]; gq[j] = state[(size_t)(TF_S_GOAL_Q + j) * N + i]; }
    const float dx = cp[0] - gp[0], dy = cp[1] - gp[1], dz = cp[2] - gp[2];       // norm3d(cp, gp) of tf_roles.h
    e_p = f_sqrt(dx * dx + dy * dy + dz * dz);
    e_o = quat_diff_rad(cq, gq);
    float z = 0.0f;
#pragma unroll
    for (int j = 0; j < 4; ++j) z = z + cq[j] * 0.0f + gq[j] * 0.0f;
    qfinite = z == 0.0f;
}

DEV bool finite_f(float x) { return (__float_as_uint(x) & 0x7F800000u) != 0x7F800000u; }
DEV int hist_bin(float x, int lo, int hi) {
    const int q = (int)(__float_as_uint(x) >> 21);
    return q < lo ? 0 : (q >= hi ? 1 + hi - lo : 1 + q - lo);
}
DEV long long wave_sum_ll(long long v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
    return v;
}
DEV long long wave_count(bool p) { return (long long)__popcll(__ballot(p)); }

// THE episode outcome of env i, stated once for the evaluator, the tracker and the recorder (evaluate.episode_outcome is the same statement in torch):
// the final errors, the two predicates, the at-goal rule (0 position, 1 both, 2 orientation) and the finite test of an episode whose return is `ret`.
// The caller decides which lanes load the 14 pose rows by deciding which lanes call.  `fin` takes the return when it is asked, not when the pose is
// loaded: the evaluator loads its running return behind the pose rows, and two loads held across them would cost k_eval_step two registers.
struct Outcome {
    float e_p, e_o;
    bool pos_ok, ori_ok, at_goal, pose_finite;
    DEV bool fin(float ret) const { return finite_f(ret) && pose_finite; }
};
DEV Outcome episode_outcome(const float* __restrict__ state, int N, int i, float pos_tol, float ori_tol, int rule) {
    Outcome o;
    bool qfinite;
    eval_errors(state, N, i, o.e_p, o.e_o, qfinite);
    o.pos_ok = o.e_p <= pos_tol;
    o.ori_ok = o.e_o <= ori_tol;
    o.at_goal = rule == 0 ? o.pos_ok : (rule == 1 ? (o.pos_ok && o.ori_ok) : o.ori_ok);
    o.pose_finite = finite_f(o.e_p) && finite_f(o.e_o) && qfinite;
    return o;
}
// the fixed point of the three sums of a COUNTED episode: 2^16 (return, clamped to +-2^25), 2^30 (position error, to 2^10), 2^28 (orientation error, to 4);
// zeros otherwise.  Finite: the clamps see no NaN, the products are exact, the conversions defined
DEV void fixed_sums(bool counted, float ret, float e_p, float e_o, long long& q_ret, long long& q_pos, long long& q_ori) {
    q_ret = q_pos = q_ori = 0;
    if (counted) {
        q_ret = __float2ll_rn(f_clamp(ret, -33554432.0f, 33554432.0f) * 65536.0f);
        q_pos = __float2ll_rn(f_min(e_p, 1024.0f) * 1073741824.0f);
        q_ori = __float2ll_rn(f_min(e_o, 4.0f) * 268435456.0f);
    }
}
// per-wavefront values v[K] of a 256-thread workgroup -> LDS -> ONE 64-bit integer atomicAdd per non-zero entry (two's complement: a negative sum adds as
// it should).  Uniform control flow: every thread of the workgroup calls; the barrier inside also orders whatever LDS the caller wrote before the call
template <int K>
DEV void block_add(const long long (&v)[K], long long (&s_part)[EV_WAVES][K], u64* __restrict__ acc, int t) {
    if ((t & 63) == 0) {
#pragma unroll
        for (int k = 0; k < K; ++k) s_part[t >> 6][k] = v[k];
    }
    __syncthreads();
    if (t < K) {
        long long s = 0;
#pragma unroll
        for (int w = 0; w < EV_WAVES; ++w) s += s_part[w][t];
        if (s != 0) atomicAdd(&acc[t], (u64)s);
    }
}

__global__ void __launch_bounds__(EV_THREADS) k_eval_step(const EvalArgs a) {
    __shared__ long long s_part[EV_WAVES][EV_SCALARS];
    __shared__ int s_hist[EV_BINS];
    const int t = threadIdx.x, i = (int)blockIdx.x * EV_THREADS + t, N = a.N;
    const bool valid = i < N;
    bool ends = false, goal_ev = false, counted = false, nonfin = false, complete = false, pos_ok = false, ori_ok = false, at_goal = false;
    float ret = 0.0f, e_p = 0.0f, e_o = 0.0f;
    int atg = 0, first = 0;
    long long len = 0;
    if (valid) {
        const Outcome o = episode_outcome(a.state, N, i, a.pos_tol, a.ori_tol, a.rule);
        e_p = o.e_p; e_o = o.e_o; pos_ok = o.pos_ok; ori_ok = o.ori_ok; at_goal = o.at_goal;
        int* __restrict__ ea = a.env_acc;
        ret = __int_as_float(ea[(size_t)TFP_EVAL_ENV_RETURN * N + i]) + a.reward[i];
        atg = ea[(size_t)TFP_EVAL_ENV_AT_GOAL_STEPS * N + i] + (at_goal ? 1 : 0);
        first = ea[(size_t)TFP_EVAL_ENV_FIRST_HIT * N + i];
        const int eps = ea[(size_t)TFP_EVAL_ENV_EPISODES * N + i];
        len = a.steps[i];
        if (first == 0 && at_goal) first = (int)(len < 1 ? 1 : (len > 0x7FFFFFFF ? 0x7FFFFFFF : len));
        const bool under = a.cap == 0 || eps < a.cap;
        goal_ev = under && a.goal_reset_buf[i] != 0;
        ends = a.reset_buf[i] != 0;
        if (ends) {
            const bool fin = o.fin(ret);
            counted = under && fin;
            nonfin = under && !fin;
            complete = under && a.cap != 0 && eps + 1 == a.cap;
            ea[(size_t)TFP_EVAL_ENV_RETURN * N + i] = 0;
            ea[(size_t)TFP_EVAL_ENV_AT_GOAL_STEPS * N + i] = 0;
            ea[(size_t)TFP_EVAL_ENV_FIRST_HIT * N + i] = 0;
            if (under) ea[(size_t)TFP_EVAL_ENV_EPISODES * N + i] = eps + 1;
        } else {
            ea[(size_t)TFP_EVAL_ENV_RETURN * N + i] = __float_as_int(ret);
            ea[(size_t)TFP_EVAL_ENV_AT_GOAL_STEPS * N + i] = atg;
            ea[(size_t)TFP_EVAL_ENV_FIRST_HIT * N + i] = first;
        }
    }
    if (t < EV_BINS) s_hist[t] = 0;
    if (!__syncthreads_or((ends && (counted || nonfin)) || goal_ev)) return;      // the barrier also publishes the zeroed histogram

    // ---- a workgroup with something to report: everything below is uniform control flow ----
    long long v[EV_SCALARS];
    v[TFP_EVAL_EPISODES] = wave_count(counted);
    v[TFP_EVAL_NONFINITE] = wave_count(nonfin);
    v[TFP_EVAL_POS_OK] = wave_count(counted && pos_ok);
    v[TFP_EVAL_ORI_OK] = wave_count(counted && ori_ok);
    v[TFP_EVAL_SUCCESS] = wave_count(counted && at_goal);
    v[TFP_EVAL_REACHED] = wave_count(counted && first != 0);
    v[TFP_EVAL_GOAL_EVENTS] = wave_count(goal_ev);
    v[TFP_EVAL_ENVS_COMPLETE] = wave_count(complete);
    long long q_ret, q_pos, q_ori;
    fixed_sums(counted, ret, e_p, e_o, q_ret, q_pos, q_ori);
    if (counted) {
        atomicAdd(&s_hist[hist_bin(e_p, TFP_EVAL_POS_Q_LO, TFP_EVAL_POS_Q_HI)], 1);
        atomicAdd(&s_hist[TFP_EVAL_POS_BINS + hist_bin(e_o, TFP_EVAL_ORI_Q_LO, TFP_EVAL_ORI_Q_HI)], 1);
    }
    v[TFP_EVAL_SUM_LENGTH] = wave_sum_ll(counted ? len : 0);
    v[TFP_EVAL_SUM_AT_GOAL_STEPS] = wave_sum_ll(counted ? (long long)atg : 0);
    v[TFP_EVAL_SUM_FIRST_HIT] = wave_sum_ll(counted ? (long long)first : 0);
    v[TFP_EVAL_SUM_RETURN] = wave_sum_ll(q_ret);
    v[TFP_EVAL_SUM_POS_ERR] = wave_sum_ll(q_pos);
    v[TFP_EVAL_SUM_ORI_ERR] = wave_sum_ll(q_ori);
    block_add(v, s_part, a.acc, t);
    if (t >= 64 && t < 64 + EV_BINS) {                                  // another wavefront than the scalars' takes the bins
        const int b = t - 64, c = s_hist[b];
        if (c != 0) atomicAdd(&a.acc[TFP_EVAL_HIST_POS + b], (u64)c);
    }
}

// the tests' window into the predicates: the device code above, counted
__global__ void __launch_bounds__(EV_THREADS) k_eval_predicates(const float* __restrict__ state, int N, float pos_tol, float ori_tol, u64* __restrict__ out) {
    const int i = (int)blockIdx.x * EV_THREADS + (int)threadIdx.x;
    bool pos_ok = false, ori_ok = false;
    if (i < N) {
        const Outcome o = episode_outcome(state, N, i, pos_tol, ori_tol, 0);
        pos_ok = o.pos_ok;
        ori_ok = o.ori_ok;
    }
    const long long np = wave_count(pos_ok), no = wave_count(ori_ok);
    if ((threadIdx.x & 63) == 0) {
        if (np) atomicAdd(&out[0], (u64)np);
        if (no) atomicAdd(&out[1], (u64)no);
    }
}

// ---- the training-time episode tracker (include/trifinger_ppo_track.h): the launch behind every env step of a rollout, with the bookkeeping folded in ----
// One env per lane as above.  Every lane does what k_rollout_reward (mode A: `done_bytes` given) or k_rollout_flags (mode B) of ppo_kernels.hip does - the
// same single product and the same selects, under the same contraction-free flags - and keeps its env's running return and `armed` flag (two int32).  A
// workgroup in which nobody ends an episode leaves there (one __syncthreads_or): no atomic, and the 14 pose rows are never loaded.  In a workgroup with an
// end only the lanes that end an ARMED episode load their pose; counters are ballots, sums 64-bit shuffle reductions, the four wavefronts meet in LDS and
// the workgroup issues one 64-bit integer atomicAdd per non-zero quantity.
__global__ void __launch_bounds__(EV_THREADS) k_rollout_track(const TfpTrackArgs a) {
    __shared__ long long s_part[EV_WAVES][TFP_TRACK_ACC];
    const int t = threadIdx.x, i = (int)blockIdx.x * EV_THREADS + t, N = a.N;
    bool ends = false, armed = false, tout = false;
    float ret = 0.0f;
    long long len = 0;
    if (i < N) {
        const float r = a.reward[i];
        ends = ((const uint8_t*)a.reset_buf)[i] != 0;
        len = a.steps[i];
        tout = a.episode_length > 0 && len >= a.episode_length;
        a.b_rew[i] = r * a.scale;
        if (a.done_bytes) {
            a.b_done[i] = ((const uint8_t*)a.done_bytes)[i] ? 1.0f : 0.0f;
        } else {
            a.b_end[i] = ends ? 1.0f : 0.0f;
            a.b_tout[i] = tout ? 1.0f : 0.0f;
        }
        int* __restrict__ trk = a.env_trk;
        const bool first = len == 1;
        ret = first ? r : __int_as_float(trk[(size_t)TFP_TRACK_ENV_RETURN * N + i]) + r;
        armed = first || trk[(size_t)TFP_TRACK_ENV_ARMED * N + i] != 0;
        trk[(size_t)TFP_TRACK_ENV_RETURN * N + i] = ends ? 0 : __float_as_int(ret);
        trk[(size_t)TFP_TRACK_ENV_ARMED * N + i] = (armed && !ends) ? 1 : 0;
    }
    if (!__syncthreads_or(ends)) return;

    // ---- a workgroup in which an episode ended: everything below is uniform control flow but for the pose loads ----
    bool counted = false, nonfin = false, pos_ok = false, ori_ok = false, at_goal = false;
    float e_p = 0.0f, e_o = 0.0f;
    if (ends && armed) {
        const Outcome o = episode_outcome((const float*)a.state, N, i, a.pos_tol, a.ori_tol, a.rule);
        e_p = o.e_p; e_o = o.e_o; pos_ok = o.pos_ok; ori_ok = o.ori_ok; at_goal = o.at_goal;
        counted = o.fin(ret);
        nonfin = !counted;
    }
    long long v[TFP_TRACK_ACC];
    v[TFP_TRACK_EPISODES] = wave_count(counted);
    v[TFP_TRACK_SUCCESS] = wave_count(counted && at_goal);
    v[TFP_TRACK_POS_OK] = wave_count(counted && pos_ok);
    v[TFP_TRACK_ORI_OK] = wave_count(counted && ori_ok);
    v[TFP_TRACK_TIMEOUT] = wave_count(counted && tout);
    v[TFP_TRACK_NONFINITE] = wave_count(nonfin);
    v[TFP_TRACK_UNARMED] = wave_count(ends && !armed);
    long long q_ret, q_pos, q_ori;
    fixed_sums(counted, ret, e_p, e_o, q_ret, q_pos, q_ori);
    v[TFP_TRACK_SUM_LENGTH] = wave_sum_ll(counted ? len : 0);
    v[TFP_TRACK_SUM_RETURN] = wave_sum_ll(q_ret);
    v[TFP_TRACK_SUM_POS_ERR] = wave_sum_ll(q_pos);
    v[TFP_TRACK_SUM_ORI_ERR] = wave_sum_ll(q_ori);
    block_add(v, s_part, (u64*)a.acc, t);
}

// ---- the episode flight recorder (include/trifinger_ppo_record.h): the launch behind every env step of an evaluation that records ----
// One env per lane as above, the first W envs only.  A lane reads its STATE word; a frozen lane stops there.  An armed lane whose step is recorded loads
// the 59 state rows of the record (coalesced lines of the SoA: a wavefront reads 256 bytes per row) into registers, an ending lane forms its final errors
// with eval_errors from the same lines, a lane at its first step loads the 14 TF_S_DR rows - and only then does the lane store: the record into its slot
// (unsigned)COUNT % L of the ring, the header, its env_rec words.  A lane that neither records nor ends loads none of the rows.  No index read from memory
// is used unreduced.  A workgroup with nothing to count leaves at one __syncthreads_or; otherwise the four counters are ballots, the wavefronts meet in
// LDS and the workgroup issues one 64-bit integer atomicAdd per non-zero counter.
__global__ void __launch_bounds__(EV_THREADS) k_record_step(const TfpRecordArgs a) {
    __shared__ long long s_part[EV_WAVES][TFP_REC_ACC];
    const int t = threadIdx.x, i = (int)blockIdx.x * EV_THREADS + t, N = a.N, W = a.W;
    bool rec = false, ended = false, froze = false, unarmed = false;
    if (i < W) {
        int* __restrict__ er = a.env_rec;
        const int st = er[(size_t)TFP_REC_ENV_STATE * W + i];
        if (st != TFP_REC_ST_FROZEN) {
            const float* __restrict__ state = (const float*)a.state;
            const long long s = a.steps[i];
            const int s32 = (int)(s < 0 ? 0 : (s > 0x7FFFFFFF ? 0x7FFFFFFF : s));
            const bool rb = ((const uint8_t*)a.reset_buf)[i] != 0;
            const bool first = s == 1;
            if (first || st == TFP_REC_ST_ARMED) {
                const float r = a.reward[i];
                const float ret = (first ? 0.0f : __int_as_float(er[(size_t)TFP_REC_ENV_RETURN * W + i])) + r;
                const unsigned cnt = first ? 0u : (unsigned)er[(size_t)TFP_REC_ENV_COUNT * W + i];
                rec = rb || (s32 - 1) % a.every == 0;
                // ---- loads ----
                float h[TF_NUM_DR], v[TFP_REC_STATE_ROWS];
                if (first) {
#pragma unroll
                    for (int j = 0; j < TF_NUM_DR; ++j) h[j] = state[(size_t)(TF_S_DR + j) * N + i];
                }
                int outcome = 0;
                float e_p = 0.0f, e_o = 0.0f;
                if (rec) {
#pragma unroll
                    for (int j = 0; j < TFP_REC_STATE_ROWS; ++j) v[j] = state[(size_t)(TF_S_Q + j) * N + i];
                    if (rb) {
                        const Outcome o = episode_outcome(state, N, i, a.pos_tol, a.ori_tol, a.rule);
                        const bool fin = o.fin(ret);
                        e_p = o.e_p; e_o = o.e_o;
                        const bool tout = a.episode_length > 0 && s >= a.episode_length;
                        outcome = (o.at_goal ? TFP_REC_OUT_AT_GOAL : 0) | (o.pos_ok ? TFP_REC_OUT_POS_OK : 0) | (o.ori_ok ? TFP_REC_OUT_ORI_OK : 0)
                                  | (tout ? TFP_REC_OUT_TIMEOUT : 0) | (fin ? 0 : TFP_REC_OUT_NONFINITE);
                        ended = true;
                        froze = ((a.select & TFP_REC_SEL_FAILURE) && fin && !o.at_goal) || ((a.select & TFP_REC_SEL_SUCCESS) && fin && o.at_goal)
                                || ((a.select & TFP_REC_SEL_NONFINITE) && !fin);
                    }
                }
                // ---- stores ----
                if (first) {
#pragma unroll
                    for (int j = 0; j < TF_NUM_DR; ++j) a.hdr[(size_t)j * W + i] = h[j];
                }
                if (rec) {
                    float* __restrict__ slot = a.ring + (size_t)(cnt % (unsigned)a.L) * TFP_REC_ROWS * W + i;
#pragma unroll
                    for (int j = 0; j < TFP_REC_STATE_ROWS; ++j) slot[(size_t)j * W] = v[j];
                    slot[(size_t)TFP_REC_REWARD * W] = r;
                    slot[(size_t)TFP_REC_STEP * W] = __int_as_float(s32);
                    er[(size_t)TFP_REC_ENV_COUNT * W + i] = (int)(cnt + 1u);
                } else if (first) {
                    er[(size_t)TFP_REC_ENV_COUNT * W + i] = 0;
                }
                er[(size_t)TFP_REC_ENV_RETURN * W + i] = __float_as_int(ret);
                const int nst = ended ? (froze ? TFP_REC_ST_FROZEN : TFP_REC_ST_IDLE) : TFP_REC_ST_ARMED;
                if (nst != st) er[(size_t)TFP_REC_ENV_STATE * W + i] = nst;
                if (ended) {
                    er[(size_t)TFP_REC_ENV_OUTCOME * W + i] = outcome;
                    if (froze) {
                        er[(size_t)TFP_REC_ENV_LENGTH * W + i] = s32;
                        er[(size_t)TFP_REC_ENV_E_P * W + i] = __float_as_int(e_p);
                        er[(size_t)TFP_REC_ENV_E_O * W + i] = __float_as_int(e_o);
                    }
                }
            } else {
                unarmed = rb;
            }
        }
    }
    if (!__syncthreads_or(rec || unarmed)) return;

    // ---- a workgroup with something to count: uniform control flow ----
    long long c[TFP_REC_ACC];
    c[TFP_REC_ENDED_ARMED] = wave_count(ended);
    c[TFP_REC_FROZEN] = wave_count(froze);
    c[TFP_REC_UNARMED] = wave_count(unarmed);
    c[TFP_REC_RECORDS] = wave_count(rec);
    block_add(c, s_part, (u64*)a.acc, t);
}

extern "C" {

int tfp_record_step(const TfpRecordArgs* args, void* stream) {
    if (!args) return -1;
    const TfpRecordArgs a = *args;
    if (!a.state || !a.reward || !a.reset_buf || !a.steps || !a.ring || !a.hdr || !a.env_rec || !a.acc) return -1;
    if (a.N < 1 || a.N > TF_MAX_ENVS || a.W < 1 || a.W > a.N || a.L < 1 || a.every < 1 || a.select < 1 || a.select > 7 || a.rule < 0 || a.rule > 2) return -1;
    if (a.episode_length < 0 || a.pos_tol != a.pos_tol || a.ori_tol != a.ori_tol) return -1;
    hipLaunchKernelGGL(k_record_step, dim3((unsigned)((a.W + EV_THREADS - 1) / EV_THREADS)), dim3(EV_THREADS), 0, (hipStream_t)stream, a);
    return hipGetLastError() == hipSuccess ? 0 : -3;
}

int tfp_rollout_track(const TfpTrackArgs* args, void* stream) {
    if (!args) return -1;
    const TfpTrackArgs a = *args;
    if (!a.state || !a.reward || !a.reset_buf || !a.steps || !a.b_rew || !a.env_trk || !a.acc) return -1;
    if (a.done_bytes ? !a.b_done : (!a.b_end || !a.b_tout)) return -1;
    if (a.N < 1 || a.N > TF_MAX_ENVS || a.rule < 0 || a.rule > 2 || a.pos_tol != a.pos_tol || a.ori_tol != a.ori_tol) return -1;
    hipLaunchKernelGGL(k_rollout_track, dim3((unsigned)((a.N + EV_THREADS - 1) / EV_THREADS)), dim3(EV_THREADS), 0, (hipStream_t)stream, a);
    return hipGetLastError() == hipSuccess ? 0 : -3;
}

int tfp_eval_step(const void* state, const void* reward, const void* reset_buf, const void* goal_reset_buf, const void* steps, void* env_acc, void* acc,
                  int32_t N, float pos_tol, float ori_tol, int32_t rule, int32_t max_episodes_per_env, void* stream) {
    if (!state || !reward || !reset_buf || !goal_reset_buf || !steps || !env_acc || !acc) return -1;
    if (N < 1 || N > TF_MAX_ENVS || rule < 0 || rule > 2 || max_episodes_per_env < 0 || pos_tol != pos_tol || ori_tol != ori_tol) return -1;
    EvalArgs a{};
    a.state = (const float*)state; a.reward = (const float*)reward; a.reset_buf = (const uint8_t*)reset_buf; a.goal_reset_buf = (const uint8_t*)goal_reset_buf;
    a.steps = (const long long*)steps; a.env_acc = (int*)env_acc; a.acc = (u64*)acc;
    a.N = N; a.pos_tol = pos_tol; a.ori_tol = ori_tol; a.rule = rule; a.cap = max_episodes_per_env;
    hipLaunchKernelGGL(k_eval_step, dim3((unsigned)((N + EV_THREADS - 1) / EV_THREADS)), dim3(EV_THREADS), 0, (hipStream_t)stream, a);
    return hipGetLastError() == hipSuccess ? 0 : -3;
}

int tfp_eval_test_predicates(const void* state, int32_t N, float pos_tol, float ori_tol, void* out, void* stream) {
    if (!state || !out || N < 1 || N > TF_MAX_ENVS) return -1;
    hipLaunchKernelGGL(k_eval_predicates, dim3((unsigned)((N + EV_THREADS - 1) / EV_THREADS)), dim3(EV_THREADS), 0, (hipStream_t)stream,
                       (const float*)state, (int)N, pos_tol, ori_tol, (u64*)out);
    return hipGetLastError() == hipSuccess ? 0 : -3;
}

}  // extern "C"
