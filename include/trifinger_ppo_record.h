/* C ABI of the episode flight recorder: the last L recorded steps of every watched env's current episode, kept on the device and FROZEN IN PLACE when
 * the episode ends in a selected way (leibnizgym_amd/csrc/libtrifinger_ppo.so: csrc/tf_eval.hip, gfx950).  Conventions as in
 * include/trifinger_ppo_eval.h: plain pointers and sizes, every pointer DEVICE memory, `stream` a hipStream_t, 0 on success, -1 invalid argument, -3 a
 * launch failed.  tfp_api_version() stays 3: the entry point below is bound by symbol.  The Python binding is leibnizgym_amd/ppo_kernels.py
 * (record_step), the user leibnizgym_amd/record.py (EpisodeRecorder, whose plain-torch form states the same definitions);
 * tests/test_episode_recorder_gpu.py holds the kernel against the torch statement, bit for bit.
 *
 * tfp_record_step is ONE launch per env step, issued behind tf_step on the same stream.  It only READS the env's buffers (include/trifinger.h: TfBuffers)
 * - state [TF_STATE_ROWS][N], reward [N], reset_buf [N] (bytes), steps [N] (int64) - and writes four buffers of the caller, all zeroed by the caller at
 * construction.  The first W <= N envs are WATCHED; the caller's buffers are W wide:
 *     ring     float32 [L][TFP_REC_ROWS][W]   the records; a record is the state rows TF_S_Q .. TF_S_TAU + 8 (rows 0..58: joints, cube pose and twist, goal
 *                                             pose and angular velocity, last fingertip positions, applied torque), the raw reward (TFP_REC_REWARD) and
 *                                             the step number s as an int32 bit pattern (TFP_REC_STEP; s clamped to [0, 2^31 - 1])
 *     hdr      float32 [TF_NUM_DR][W]         the episode's TF_S_DR rows, written at its first step (the renderer needs cube size, base and stage offsets)
 *     env_rec  int32 [TFP_REC_ENV_ROWS][W]    per env: STATE (0 idle, 1 armed, 2 frozen), COUNT (records written in this episode), LENGTH, OUTCOME, the
 *                                             bits of the float32 RETURN, E_P and E_O, one spare row
 *     acc      int64 [TFP_REC_ACC]            ENDED_ARMED, FROZEN, UNARMED, RECORDS.  INTEGERS only: the bits do not depend on the order of the workgroups.
 *
 * Per watched env i, after a step, with s = steps[i], rb = reset_buf[i] != 0 and r = reward[i].  The three cases are decided by STATE as it stands after
 * the arming line (an env that ends unselected goes idle and does NOT count as unarmed in the same step); a STATE other than 1 or 2 counts as 0.  Where s
 * is stored or divided (the step row, LENGTH, the `every` test) it is first clamped to [0, 2^31 - 1]; the tests s == 1 and s >= episode_length see all 64 bits:
 *     STATE == 2: nothing of this env is read or written beyond that word - the ring, hdr and env_rec column stay as frozen until the host harvests them
 *                 and sets STATE back to 0.
 *     s == 1:     STATE = 1; COUNT = 0; RETURN = 0; hdr[:, i] = state[TF_S_DR .., i]                      (arms, or re-arms without a seen end)
 *     STATE == 1:
 *         RETURN = RETURN + r                                                                               (float32, step order)
 *         if (s - 1) % every == 0 or rb:  ring[(unsigned)COUNT % L][:, i] = record; COUNT += 1; RECORDS += 1
 *         if rb:
 *             e_p, e_o, pos_ok, ori_ok, at_goal(rule): the device functions, expressions and tolerances of tfp_eval_step
 *             finite = RETURN, e_p, e_o and both quaternions finite (the test of tfp_eval_step)
 *             timeout = episode_length > 0 and s >= episode_length
 *             OUTCOME = at_goal | pos_ok << 1 | ori_ok << 2 | timeout << 3 | (!finite) << 4
 *             q = (select & 1 and finite and !at_goal) or (select & 2 and finite and at_goal) or (select & 4 and !finite)
 *             ENDED_ARMED += 1
 *             q:      STATE = 2; LENGTH = s; E_P, E_O = bits; FROZEN += 1
 *             else:   STATE = 0
 *     STATE == 0 and rb: UNARMED += 1            (the end of an episode the recorder did not see from its first step)
 * The first record of an episode is the state after its first step: the post-reset state exists only inside the step launch.  With every > 1 the records
 * fall at s = 1, 1 + every, ... and at the final step.  After an end the ring holds the last min(COUNT, L) records, the oldest at slot COUNT % L when
 * COUNT > L and at slot 0 otherwise.
 *
 * No index read from memory is used unreduced: the slot is (unsigned)COUNT % L and STATE is compared, never used as an index, so even a corrupted env_rec
 * cannot take a store outside `ring`.  The call allocates nothing, synchronises nothing and keeps no state in the library; nobody may read `acc` or a
 * frozen column before the stream is synchronised. */
#ifndef TRIFINGER_PPO_RECORD_H
#define TRIFINGER_PPO_RECORD_H
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif

#define TFP_REC_STATE_ROWS 59         /* TF_S_Q .. TF_S_TAU + 8 = TF_S_PREV_OBJ_P - 1                                        */
enum { TFP_REC_REWARD = TFP_REC_STATE_ROWS, TFP_REC_STEP = TFP_REC_STATE_ROWS + 1, TFP_REC_ROWS = TFP_REC_STATE_ROWS + 2 };

enum { TFP_REC_ENV_STATE = 0, TFP_REC_ENV_COUNT = 1, TFP_REC_ENV_LENGTH = 2, TFP_REC_ENV_OUTCOME = 3, TFP_REC_ENV_RETURN = 4, TFP_REC_ENV_E_P = 5,
       TFP_REC_ENV_E_O = 6, TFP_REC_ENV_SPARE = 7, TFP_REC_ENV_ROWS = 8 };
enum { TFP_REC_ST_IDLE = 0, TFP_REC_ST_ARMED = 1, TFP_REC_ST_FROZEN = 2 };

/* bits of OUTCOME */
enum { TFP_REC_OUT_AT_GOAL = 1, TFP_REC_OUT_POS_OK = 2, TFP_REC_OUT_ORI_OK = 4, TFP_REC_OUT_TIMEOUT = 8, TFP_REC_OUT_NONFINITE = 16 };
/* bits of `select` */
enum { TFP_REC_SEL_FAILURE = 1, TFP_REC_SEL_SUCCESS = 2, TFP_REC_SEL_NONFINITE = 4 };

enum {
    TFP_REC_ENDED_ARMED = 0,          /* ends of episodes the recorder saw from their first step                              */
    TFP_REC_FROZEN = 1,               /* ... of which were selected and frozen                                                */
    TFP_REC_UNARMED = 2,              /* ends of episodes the recorder did not see from their first step                      */
    TFP_REC_RECORDS = 3,              /* records written                                                                      */
    TFP_REC_ACC = 4
};

typedef struct TfpRecordArgs {
    const void* state;                /* float [TF_STATE_ROWS][N]                                                             */
    const float* reward;              /* [N]                                                                                  */
    const void* reset_buf;            /* [N] bytes                                                                            */
    const int64_t* steps;             /* [N]                                                                                  */
    float* ring;                      /* [L][TFP_REC_ROWS][W]                                                                 */
    float* hdr;                       /* [TF_NUM_DR][W]                                                                       */
    int32_t* env_rec;                 /* [TFP_REC_ENV_ROWS][W]                                                                */
    int64_t* acc;                     /* [TFP_REC_ACC]                                                                        */
    int64_t episode_length;           /* 0: no time limit                                                                     */
    float pos_tol, ori_tol;
    int32_t N;
    int32_t W;                        /* the first W envs are watched                                                         */
    int32_t L;                        /* ring length                                                                          */
    int32_t every;                    /* record the steps with (s - 1) % every == 0, and every final step                     */
    int32_t select;                   /* TFP_REC_SEL_* bits                                                                   */
    int32_t rule;                     /* 0 position, 1 position and orientation, 2 orientation                                */
} TfpRecordArgs;

/* -1: `args` NULL, a NULL pointer, N outside [1, TF_MAX_ENVS], W outside [1, N], L < 1, every < 1, select outside 1..7, rule outside 0..2, a negative
 * episode_length, a tolerance that is NaN */
int tfp_record_step(const TfpRecordArgs* args, void* stream);

#ifdef __cplusplus
}
#endif
#endif
