/* trifinger_kin.h - C ABI of the fingertip-space library (libtrifinger_kin.so): forward kinematics, Jacobians, damped-least-squares inverse
 * kinematics and Cartesian fingertip actions of the three 3-DoF fingers, batched over envs, one launch each.
 *
 * An extension: the reference has no such interface (its users read the Jacobian tensor of the simulator).  The library shares no object with
 * libtrifinger_hip.so; it reuses the step's device functions (fk_setup, rot_link, levers, finger_dynamics), so a fingertip position here is formed
 * by the operations that form TF_S_TIP_P in the step.  The env step is not involved: tfk_tip_action produces the env's native action [N][9], which
 * the caller hands to tf_step.
 *
 * Conventions: plain C, opaque handle, raw device pointers, streams as void* (hipStream_t; NULL = the default stream).  Return value: TFK_OK (0),
 * TFK_ERR_INVALID_ARG (-1), TFK_ERR_LAUNCH (-3: the launch failed; tfk_last_error_string has the text).  Nothing allocates or synchronises after
 * tfk_create.  Every launching entry point reads and writes rows [0, N) only, N in [1, TF_MAX_ENVS].
 *
 * ARRAY ARGUMENTS.  A per-env input is a TfkArray: a pointer and two strides in floats; element (env i, component j) is p[i * env_stride +
 * j * comp_stride].  Rows of the engine's structure-of-arrays state are {state + TF_S_Q * N, 1, N}; a row-major tensor [N][9] is {ptr, 9, 1}.
 * Strides lie in [0, 2^31) (0 broadcasts).  A required input has p != NULL; an optional one ("?") may have p == NULL.  base_off (3 components) is
 * the robot base offset of the domain randomisation, rows TF_S_DR + TF_DR_BASE_POS .. +2 of the state; NULL: no offset is added.
 * Outputs are row-major and dense.
 *
 * THE ARITHMETIC (fp32, the step's flags: no contraction, the step's own sin / cos; `/` and sqrt are IEEE).  For finger f with joints q = q[3f .. 3f+2],
 * yaw (c, s) = (base_yaw_cos[f], base_yaw_sin[f]), H = base_height:
 *   FK      (s1, c1) = sincos(q0), (s2, c2) = sincos(q1), (s23, c23) = sincos(q1 + q2);
 *           R1 u = (c1 ux + s1 uz, uy, c1 uz - s1 ux);  Rk u (k = 2, 3; a = 2, 23) = R1 (ux, ca uy - sa uz, sa uy + ca uz);
 *           p2 = R1 j2_origin, p3 = p2 + R2 j3_origin, p = p3 + R3 tip_origin              (the tip-link origin in the finger's base frame)
 *           tip_world = (c px - s py, s px + c py, pz + H) [+ base_off]                    (the point TF_S_TIP_P reports)
 *   J       axis = (c1, 0, -s1);  L1 = (pz, 0, -px), L2 = axis x (p - p2), L3 = axis x (p - p3)          (columns in the base frame)
 *           jac[i][f][r][c] = d tip_world[f][r] / d q[3f + c] = (Rz(yaw_f) Lc)[r];  block diagonal by construction: only the three 3 x 3 blocks exist
 *           tip_v = Rz(yaw_f) (L1 qd0 + L2 qd1 + L3 qd2)                                   (= J qd)
 *   DLS     one iteration towards a world target t, in the base frame:
 *             tb = Rz(yaw_f)^T (t [- base_off]) - (0, 0, H);  e = tb - p(q);  A = L L^T + lambda^2 I  (L = [L1 L2 L3]; symmetric positive definite)
 *             y = adj(A) e / max(det(A), lambda^6)                                         (adjugate, IEEE division; every eigenvalue of A is >= lambda^2,
 *                                                                                          so the floor acts only where fp32 cancellation near a singular
 *                                                                                          pose rounded det below its exact lower bound - y stays finite)
 *             dq_c = Lc . y;  dq = dq * min(1, step_max / max_c |dq_c|);  q = clamp(q + dq, q_lo, q_hi)
 *           L L^T and the error turn with Rz, so this is J^T (J J^T + lambda^2 I)^-1 (t - tip_world) of the world frame.
 *   g(q)    the bias of the step's finger_dynamics at qd = 0 under `gravity` (world frame, turned into the base frame), with the NOMINAL link masses
 *           of the model: the link-mass factor of the domain randomisation (TF_S_DR + 4) is NOT followed.
 */
#ifndef TRIFINGER_KIN_H
#define TRIFINGER_KIN_H

#include <stdint.h>

#include "trifinger.h"

#ifdef __cplusplus
extern "C" {
#endif

#define TFK_API_VERSION 1
#define TFK_MAX_IK_ITERS 64           /* upper limit of TfkIkParams.iters */
#define TFK_MAX_ACTION_ITERS 8        /* upper limit of TfkActionParams.iters */

enum { TFK_OK = 0, TFK_ERR_INVALID_ARG = -1, TFK_ERR_LAUNCH = -3 };
enum { TFK_FRAME_DELTA = 0, TFK_FRAME_ABSOLUTE = 1 };
enum { TFK_MODE_POSITION = 0, TFK_MODE_TORQUE = 1 };

typedef struct TfkArray {
    const float* p;           /* DEVICE */
    int64_t env_stride;       /* floats between consecutive envs */
    int64_t comp_stride;      /* floats between consecutive components */
} TfkArray;

typedef struct TfkIkParams {
    int32_t iters;            /* exactly this many DLS iterations, no early exit: 1..TFK_MAX_IK_ITERS */
    float lambda;             /* damping, > 0 (default 0.02; below about 1e-3 the fp32 solve near a singular pose rests on the det floor above) */
    float step_max;           /* largest joint step of one iteration, rad, > 0 */
} TfkIkParams;

typedef struct TfkActionParams {
    int32_t frame;            /* TFK_FRAME_* */
    int32_t mode;             /* TFK_MODE_*: the command_mode of the env the action is for */
    int32_t iters;            /* TFK_MODE_POSITION: DLS iterations per step, 1..TFK_MAX_ACTION_ITERS */
    int32_t normalize;        /* the env's normalize_action: the action is mapped to [-1, 1] */
    int32_t gravity_comp;     /* TFK_MODE_TORQUE: add g(q) */
    float lambda, step_max;   /* of the DLS iterations, both > 0 */
    float delta_scale;        /* TFK_FRAME_DELTA: metres per unit command, > 0 */
    float box_lo[3], box_hi[3];   /* the box every target is clamped into, world frame, stated for finger 0; box_lo <= box_hi */
    float kp[3], kd[3];       /* TFK_MODE_TORQUE: Cartesian stiffness (N/m) and damping (N s/m) per world axis, >= 0 */
    float gravity[3];         /* TFK_MODE_TORQUE with gravity_comp: the gravity vector of the env, world frame */
} TfkActionParams;

typedef struct tfk_handle_s* tfk_handle;

int tfk_api_version(void);
const char* tfk_last_error_string(void);

/* Host-side only.  Copies the kinematic chain (base_height, the base yaws, j2_origin, j3_origin, tip_origin), the inertial fields (link_mass,
 * link_com, link_inertia), q_lo, q_hi and tau_max of the model.  TFK_ERR_INVALID_ARG: a NULL argument, a non-finite field among those, q_lo >= q_hi,
 * tau_max <= 0. */
int tfk_create(const TfModel* model, tfk_handle* out);
int tfk_destroy(tfk_handle h);

/* q: 9 components.  qd? : 9 components, required when tip_v is asked for.  base_off? : 3 components.  tip_p: DEVICE float [N][9].  tip_v?: DEVICE float
 * [N][9] or NULL.  jac?: DEVICE float [N][3][3][3] or NULL.  One launch. */
int tfk_forward(tfk_handle h, TfkArray q, TfkArray qd, TfkArray base_off, float* tip_p, float* tip_v, float* jac, int32_t N, void* stream);

/* target: 9 components, world frame.  q0: 9 components, the start.  `iters` DLS iterations per finger (above).  q_out: DEVICE float [N][9].  residual:
 * DEVICE float [N][3], residual[i][f] = |target_f - tip_world_f(q_out)|.  One launch. */
int tfk_inverse(tfk_handle h, TfkArray target, TfkArray q0, TfkArray base_off, const TfkIkParams* params, float* q_out, float* residual, int32_t N,
                void* stream);

/* The env's native action [N][9] from a fingertip command cmd (9 components): one launch per env step, in front of tf_step.  With x = tip_world(q),
 * (cr, sr) the yaw of finger f relative to finger 0 (cr = c_f c_0 + s_f s_0, sr = s_f c_0 - c_f s_0) and k = clamp(cmd, -1, 1) per component:
 *   target  TFK_FRAME_DELTA:    d = x + delta_scale k;  u = Rz(cr, sr)^T d             (the box frame of finger f)
 *           TFK_FRAME_ABSOLUTE: u = box_lo + ((k + 1) / 2) (box_hi - box_lo)
 *           u = clamp(u, box_lo, box_hi);  x_des = Rz(cr, sr) u                            (target_out? [N][9] receives x_des)
 *   TFK_MODE_POSITION   q_des = `iters` DLS iterations towards x_des from q;  action = q_des, or with `normalize`
 *                       (q_des - (q_lo + q_hi) / 2) / ((q_hi - q_lo) / 2): the inverse of the map in the step's torque law
 *   TFK_MODE_TORQUE     F = kp o (x_des - x) - kd o tip_v;  Fb = Rz(yaw_f)^T F;  tau_c = Lc . Fb [+ g_c(q) with gravity_comp];
 *                       action = clamp(tau, -tau_max, tau_max), divided by tau_max with `normalize`
 * qd is read in TFK_MODE_TORQUE only (it may be NULL in TFK_MODE_POSITION).  Envs in command_mode position_impedance (18 actions) are not served. */
int tfk_tip_action(tfk_handle h, const TfkActionParams* params, TfkArray cmd, TfkArray q, TfkArray qd, TfkArray base_off, float* action,
                   float* target_out, int32_t N, void* stream);

#ifdef __cplusplus
}
#endif
#endif
