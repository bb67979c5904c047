// tf_kin.hip - the fingertip-space library (include/trifinger_kin.h, libtrifinger_kin.so): forward kinematics, Jacobians, damped-least-squares
// inverse kinematics and Cartesian fingertip actions, batched over envs.  One translation unit of its own, no object shared with the step library.
//
// One lane per (env, finger): 256-thread blocks along the envs, the finger on blockIdx.y, so the yaw of a block and every model constant is
// wave-uniform (the copied model travels by value: scalar registers) and loads from state rows coalesce along the envs.  No LDS, no atomics, counted
// loops.  The last block is ragged: every load and store is predicated on env < N.  The positions come from the step's own fk_setup chain under the
// step's arithmetic flags (Makefile: EVALFLAGS).
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdio.h>
#include <string.h>

#include "tf_device_math.h"
#include "tf_contact.h"
#include "../../include/trifinger_kin.h"

#define KIN_BLOCK 256

// what the kernels read of the model: the DevModel the step's device functions take (only the fields tfk_create copies are set) and the yaw of
// every finger relative to finger 0 (the frame the target box is stated in)
struct KinModel {
    DevModel m;
    float rel_c[3], rel_s[3];
};

struct KinArray {
    const float* p;
    int64_t es, cs;
};
DEV float ld(const KinArray& a, int i, int j) { return a.p[(int64_t)i * a.es + (int64_t)j * a.cs]; }

// the tip-link origin in the base frame and the Jacobian columns there
DEV void tip_and_levers(const DevModel& m, const float q[3], FK& k, float p[3], float L[3][3]) {
    fk_setup(m, q, k);
    link_point<3>(k, m.tip_origin, p);
    levers(k, p, L[0], L[1], L[2]);
}

// one damped-least-squares iteration towards the base-frame target tb (include/trifinger_kin.h: DLS)
DEV void dls_iteration(const DevModel& m, const float tb[3], float lam2, float step_max, float q[3]) {
    FK k;
    float p[3], L[3][3];
    tip_and_levers(m, q, k, p, L);
    const float e[3] = {tb[0] - p[0], tb[1] - p[1], tb[2] - p[2]};
    float A[6];                                                   // 00 01 02 11 12 22 of L L^T + lambda^2 I
    A[0] = FMA(L[2][0], L[2][0], FMA(L[1][0], L[1][0], L[0][0] * L[0][0])) + lam2;
    A[1] = FMA(L[2][0], L[2][1], FMA(L[1][0], L[1][1], L[0][0] * L[0][1]));
    A[2] = FMA(L[2][0], L[2][2], FMA(L[1][0], L[1][2], L[0][0] * L[0][2]));
    A[3] = FMA(L[2][1], L[2][1], FMA(L[1][1], L[1][1], L[0][1] * L[0][1])) + lam2;
    A[4] = FMA(L[2][1], L[2][2], FMA(L[1][1], L[1][2], L[0][1] * L[0][2]));
    A[5] = FMA(L[2][2], L[2][2], FMA(L[1][2], L[1][2], L[0][2] * L[0][2])) + lam2;
    const float c00 = FMA(A[3], A[5], -(A[4] * A[4]));
    const float c01 = FMA(A[2], A[4], -(A[1] * A[5]));
    const float c02 = FMA(A[1], A[4], -(A[2] * A[3]));
    const float c11 = FMA(A[0], A[5], -(A[2] * A[2]));
    const float c12 = FMA(A[1], A[2], -(A[0] * A[4]));
    const float c22 = FMA(A[0], A[3], -(A[1] * A[1]));
    // every eigenvalue of A is at least lambda^2, so det A >= lambda^6 exactly; near a singular pose with a tiny lambda the fp32 cancellation can round
    // below that (to zero or a negative value): the floor keeps y finite and the step bounded by step_max
    const float det = f_max(FMA(A[2], c02, FMA(A[1], c01, A[0] * c00)), (lam2 * lam2) * lam2);
    float y[3];
    y[0] = FMA(c02, e[2], FMA(c01, e[1], c00 * e[0])) / det;
    y[1] = FMA(c12, e[2], FMA(c11, e[1], c01 * e[0])) / det;
    y[2] = FMA(c22, e[2], FMA(c12, e[1], c02 * e[0])) / det;
    float dq[3];
#pragma unroll
    for (int c = 0; c < 3; ++c) dq[c] = dot3(L[c], y);
    const float big = f_max(f_max(f_abs(dq[0]), f_abs(dq[1])), f_abs(dq[2]));
    const float sc = f_min(1.0f, step_max / big);                 // big == 0: +inf, the minimum is 1
#pragma unroll
    for (int c = 0; c < 3; ++c) q[c] = f_min(f_max(FMA(dq[c], sc, q[c]), m.q_lo[c]), m.q_hi[c]);
}

// world target -> the finger's base frame
DEV void target_to_base(const Yaw& yw, const float t[3], const float boff[3], bool has_off, float tb[3]) {
    float w[3] = {t[0], t[1], t[2]};
    if (has_off) { w[0] = w[0] - boff[0]; w[1] = w[1] - boff[1]; w[2] = w[2] - boff[2]; }
    world_to_base(yw, w, tb);
}

DEV void tip_world(const Yaw& yw, const float p[3], const float boff[3], bool has_off, float x[3]) {
    base_to_world(yw, p, x);
    if (has_off) { x[0] = x[0] + boff[0]; x[1] = x[1] + boff[1]; x[2] = x[2] + boff[2]; }
}

__global__ __launch_bounds__(KIN_BLOCK) void k_forward(const KinModel P, KinArray q_in, KinArray qd_in, KinArray off_in, float* __restrict__ tip_p,
                                                        float* __restrict__ tip_v, float* __restrict__ jac, int N) {
    const int i = blockIdx.x * KIN_BLOCK + threadIdx.x, f = blockIdx.y;
    if (i >= N) return;
    const DevModel& m = P.m;
    const Yaw yw = {m.base_yaw_cos[f], m.base_yaw_sin[f], m.base_half_yaw_cos[f], m.base_half_yaw_sin[f], m.base_height};
    const bool has_off = off_in.p != nullptr;
    float q[3], boff[3] = {0.0f, 0.0f, 0.0f};
#pragma unroll
    for (int j = 0; j < 3; ++j) { q[j] = ld(q_in, i, 3 * f + j); if (has_off) boff[j] = ld(off_in, i, j); }
    FK k;
    float p[3], L[3][3], x[3];
    tip_and_levers(m, q, k, p, L);
    tip_world(yw, p, boff, has_off, x);
    const size_t o = (size_t)i * 9 + 3 * f;
#pragma unroll
    for (int j = 0; j < 3; ++j) tip_p[o + j] = x[j];
    if (tip_v) {
        float qd[3], vb[3], v[3];
#pragma unroll
        for (int j = 0; j < 3; ++j) qd[j] = ld(qd_in, i, 3 * f + j);
#pragma unroll
        for (int r = 0; r < 3; ++r) vb[r] = L[0][r] * qd[0] + L[1][r] * qd[1] + L[2][r] * qd[2];
        dir_base_to_world(yw, vb, v);
#pragma unroll
        for (int j = 0; j < 3; ++j) tip_v[o + j] = v[j];
    }
    if (jac) {
        float* J = jac + (size_t)i * 27 + 9 * f;
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            float w[3];
            dir_base_to_world(yw, L[c], w);
#pragma unroll
            for (int r = 0; r < 3; ++r) J[3 * r + c] = w[r];
        }
    }
}

__global__ __launch_bounds__(KIN_BLOCK) void k_inverse(const KinModel P, KinArray t_in, KinArray q0_in, KinArray off_in, int iters, float lam2, float step_max,
                                                        float* __restrict__ q_out, float* __restrict__ residual, int N) {
    const int i = blockIdx.x * KIN_BLOCK + threadIdx.x, f = blockIdx.y;
    if (i >= N) return;
    const DevModel& m = P.m;
    const Yaw yw = {m.base_yaw_cos[f], m.base_yaw_sin[f], m.base_half_yaw_cos[f], m.base_half_yaw_sin[f], m.base_height};
    const bool has_off = off_in.p != nullptr;
    float q[3], t[3], boff[3] = {0.0f, 0.0f, 0.0f}, tb[3];
#pragma unroll
    for (int j = 0; j < 3; ++j) { q[j] = ld(q0_in, i, 3 * f + j); t[j] = ld(t_in, i, 3 * f + j); if (has_off) boff[j] = ld(off_in, i, j); }
    target_to_base(yw, t, boff, has_off, tb);
#pragma unroll 1
    for (int it = 0; it < iters; ++it) dls_iteration(m, tb, lam2, step_max, q);
    FK k;
    float p[3], x[3];
    fk_setup(m, q, k);
    link_point<3>(k, m.tip_origin, p);
    tip_world(yw, p, boff, has_off, x);
    const float d[3] = {t[0] - x[0], t[1] - x[1], t[2] - x[2]};
#pragma unroll
    for (int j = 0; j < 3; ++j) q_out[(size_t)i * 9 + 3 * f + j] = q[j];
    residual[(size_t)i * 3 + f] = f_sqrt(FMA(d[2], d[2], FMA(d[1], d[1], d[0] * d[0])));
}

__global__ __launch_bounds__(KIN_BLOCK) void k_tip_action(const KinModel P, const TfkActionParams A, float lam2, KinArray cmd_in, KinArray q_in, KinArray qd_in,
                                                           KinArray off_in, float* __restrict__ action, float* __restrict__ target_out, int N) {
    const int i = blockIdx.x * KIN_BLOCK + threadIdx.x, f = blockIdx.y;
    if (i >= N) return;
    const DevModel& m = P.m;
    const Yaw yw = {m.base_yaw_cos[f], m.base_yaw_sin[f], m.base_half_yaw_cos[f], m.base_half_yaw_sin[f], m.base_height};
    const float cr = P.rel_c[f], sr = P.rel_s[f];
    const bool has_off = off_in.p != nullptr;
    float q[3], cmd[3], boff[3] = {0.0f, 0.0f, 0.0f};
#pragma unroll
    for (int j = 0; j < 3; ++j) {
        q[j] = ld(q_in, i, 3 * f + j);
        cmd[j] = f_min(f_max(ld(cmd_in, i, 3 * f + j), -1.0f), 1.0f);
        if (has_off) boff[j] = ld(off_in, i, j);
    }
    FK k;
    float p[3], L[3][3], x[3];
    tip_and_levers(m, q, k, p, L);
    tip_world(yw, p, boff, has_off, x);
    // ---- the target ----
    float u[3];
    if (A.frame == TFK_FRAME_DELTA) {
        const float d[3] = {FMA(A.delta_scale, cmd[0], x[0]), FMA(A.delta_scale, cmd[1], x[1]), FMA(A.delta_scale, cmd[2], x[2])};
        u[0] = FMA(cr, d[0], sr * d[1]);
        u[1] = FMA(cr, d[1], -(sr * d[0]));
        u[2] = d[2];
    } else {
#pragma unroll
        for (int j = 0; j < 3; ++j) u[j] = FMA((cmd[j] + 1.0f) * 0.5f, A.box_hi[j] - A.box_lo[j], A.box_lo[j]);
    }
#pragma unroll
    for (int j = 0; j < 3; ++j) u[j] = f_min(f_max(u[j], A.box_lo[j]), A.box_hi[j]);
    const float xd[3] = {FMA(cr, u[0], -(sr * u[1])), FMA(sr, u[0], cr * u[1]), u[2]};
    const size_t o = (size_t)i * 9 + 3 * f;
    if (target_out) {
#pragma unroll
        for (int j = 0; j < 3; ++j) target_out[o + j] = xd[j];
    }
    // ---- the action ----
    float a[3];
    if (A.mode == TFK_MODE_POSITION) {
        float tb[3];
        target_to_base(yw, xd, boff, has_off, tb);
#pragma unroll 1
        for (int it = 0; it < A.iters; ++it) dls_iteration(m, tb, lam2, A.step_max, q);
#pragma unroll
        for (int j = 0; j < 3; ++j) a[j] = A.normalize ? (q[j] - (m.q_lo[j] + m.q_hi[j]) * 0.5f) / ((m.q_hi[j] - m.q_lo[j]) * 0.5f) : q[j];
    } else {
        float qd[3], vb[3], v[3], F[3], Fb[3];
#pragma unroll
        for (int j = 0; j < 3; ++j) qd[j] = ld(qd_in, i, 3 * f + j);
#pragma unroll
        for (int r = 0; r < 3; ++r) vb[r] = L[0][r] * qd[0] + L[1][r] * qd[1] + L[2][r] * qd[2];
        dir_base_to_world(yw, vb, v);
#pragma unroll
        for (int j = 0; j < 3; ++j) F[j] = A.kp[j] * (xd[j] - x[j]) - A.kd[j] * v[j];
        dir_world_to_base(yw, F, Fb);
        float g[3] = {0.0f, 0.0f, 0.0f};
        if (A.gravity_comp) {
            const float zero[3] = {0.0f, 0.0f, 0.0f};
            float gb[3], M[6];
            dir_world_to_base(yw, A.gravity, gb);
            finger_dynamics(m, k, zero, gb, M, g);
        }
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            float t = dot3(L[c], Fb);
            if (A.gravity_comp) t = t + g[c];
            t = f_min(f_max(t, -m.tau_max), m.tau_max);
            a[c] = A.normalize ? t / m.tau_max : t;
        }
    }
#pragma unroll
    for (int j = 0; j < 3; ++j) action[o + j] = a[j];
}

// ------------------------------------------------------------------------------------------------------
// host
// ------------------------------------------------------------------------------------------------------
struct tfk_handle_s {
    KinModel P;
};

static thread_local char g_err[256] = "";
static int fail(int status, const char* what, const char* detail = "") {
    snprintf(g_err, sizeof(g_err), "%s%s", what, detail);
    return status;
}

static bool all_finite(const float* v, int n) {
    for (int i = 0; i < n; ++i)
        if (!isfinite(v[i])) return false;
    return true;
}

// a required (or present) array: strides in [0, 2^31)
static bool array_ok(const TfkArray& a, bool required) {
    if (!a.p) return !required;
    return a.env_stride >= 0 && a.env_stride < ((int64_t)1 << 31) && a.comp_stride >= 0 && a.comp_stride < ((int64_t)1 << 31);
}
static KinArray dev(const TfkArray& a) { return KinArray{a.p, a.env_stride, a.comp_stride}; }
static const KinArray NO_ARRAY = {nullptr, 0, 0};

static dim3 grid_of(int32_t N) { return dim3((unsigned)((N + KIN_BLOCK - 1) / KIN_BLOCK), 3); }

static int launched(const char* what) {
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return fail(TFK_ERR_LAUNCH, what, hipGetErrorString(e));
    return TFK_OK;
}

extern "C" {

int tfk_api_version(void) { return TFK_API_VERSION; }
const char* tfk_last_error_string(void) { return g_err; }

int tfk_create(const TfModel* model, tfk_handle* out) {
    if (!model || !out) return fail(TFK_ERR_INVALID_ARG, "tfk_create: NULL argument");
    const TfModel& s = *model;
    if (!(isfinite(s.base_height) && all_finite(s.base_yaw_cos, 3) && all_finite(s.base_yaw_sin, 3) && all_finite(s.base_half_yaw_cos, 3) &&
          all_finite(s.base_half_yaw_sin, 3) && all_finite(s.j2_origin, 3) && all_finite(s.j3_origin, 3) && all_finite(s.tip_origin, 3) &&
          all_finite(s.link_mass, 3) && all_finite(&s.link_com[0][0], 9) && all_finite(&s.link_inertia[0][0], 18) && all_finite(s.q_lo, 3) &&
          all_finite(s.q_hi, 3) && isfinite(s.tau_max)))
        return fail(TFK_ERR_INVALID_ARG, "tfk_create: a non-finite field of the model");
    for (int j = 0; j < 3; ++j)
        if (!(s.q_lo[j] < s.q_hi[j])) return fail(TFK_ERR_INVALID_ARG, "tfk_create: q_lo >= q_hi");
    if (!(s.tau_max > 0.0f)) return fail(TFK_ERR_INVALID_ARG, "tfk_create: tau_max <= 0");
    tfk_handle h = new tfk_handle_s;
    memset(&h->P, 0, sizeof(h->P));
    DevModel& m = h->P.m;
    m.base_height = s.base_height;
    memcpy(m.base_yaw_cos, s.base_yaw_cos, sizeof(m.base_yaw_cos));
    memcpy(m.base_yaw_sin, s.base_yaw_sin, sizeof(m.base_yaw_sin));
    memcpy(m.base_half_yaw_cos, s.base_half_yaw_cos, sizeof(m.base_half_yaw_cos));
    memcpy(m.base_half_yaw_sin, s.base_half_yaw_sin, sizeof(m.base_half_yaw_sin));
    memcpy(m.j2_origin, s.j2_origin, sizeof(m.j2_origin));
    memcpy(m.j3_origin, s.j3_origin, sizeof(m.j3_origin));
    memcpy(m.tip_origin, s.tip_origin, sizeof(m.tip_origin));
    memcpy(m.link_mass, s.link_mass, sizeof(m.link_mass));
    memcpy(m.link_com, s.link_com, sizeof(m.link_com));
    memcpy(m.link_inertia, s.link_inertia, sizeof(m.link_inertia));
    memcpy(m.q_lo, s.q_lo, sizeof(m.q_lo));
    memcpy(m.q_hi, s.q_hi, sizeof(m.q_hi));
    m.tau_max = s.tau_max;
    const float c0 = s.base_yaw_cos[0], s0 = s.base_yaw_sin[0];
    for (int f = 0; f < 3; ++f) {
        h->P.rel_c[f] = s.base_yaw_cos[f] * c0 + s.base_yaw_sin[f] * s0;
        h->P.rel_s[f] = s.base_yaw_sin[f] * c0 - s.base_yaw_cos[f] * s0;
    }
    *out = h;
    return TFK_OK;
}

int tfk_destroy(tfk_handle h) {
    if (!h) return fail(TFK_ERR_INVALID_ARG, "tfk_destroy: NULL handle");
    delete h;
    return TFK_OK;
}

int tfk_forward(tfk_handle h, TfkArray q, TfkArray qd, TfkArray base_off, float* tip_p, float* tip_v, float* jac, int32_t N, void* stream) {
    if (!h || !tip_p) return fail(TFK_ERR_INVALID_ARG, "tfk_forward: NULL handle or tip_p");
    if (N < 1 || N > TF_MAX_ENVS) return fail(TFK_ERR_INVALID_ARG, "tfk_forward: N outside [1, TF_MAX_ENVS]");
    if (!array_ok(q, true) || !array_ok(qd, tip_v != nullptr) || !array_ok(base_off, false))
        return fail(TFK_ERR_INVALID_ARG, "tfk_forward: q (and qd with tip_v) need a pointer; strides lie in [0, 2^31)");
    hipLaunchKernelGGL(k_forward, grid_of(N), dim3(KIN_BLOCK), 0, (hipStream_t)stream, h->P, dev(q), tip_v ? dev(qd) : NO_ARRAY, dev(base_off), tip_p, tip_v,
                       jac, (int)N);
    return launched("tfk_forward: ");
}

int tfk_inverse(tfk_handle h, TfkArray target, TfkArray q0, TfkArray base_off, const TfkIkParams* params, float* q_out, float* residual, int32_t N,
                void* stream) {
    if (!h || !params || !q_out || !residual) return fail(TFK_ERR_INVALID_ARG, "tfk_inverse: NULL handle, params, q_out or residual");
    if (N < 1 || N > TF_MAX_ENVS) return fail(TFK_ERR_INVALID_ARG, "tfk_inverse: N outside [1, TF_MAX_ENVS]");
    if (!array_ok(target, true) || !array_ok(q0, true) || !array_ok(base_off, false))
        return fail(TFK_ERR_INVALID_ARG, "tfk_inverse: target and q0 need a pointer; strides lie in [0, 2^31)");
    if (params->iters < 1 || params->iters > TFK_MAX_IK_ITERS) return fail(TFK_ERR_INVALID_ARG, "tfk_inverse: iters outside [1, TFK_MAX_IK_ITERS]");
    if (!(isfinite(params->lambda) && params->lambda > 0.0f)) return fail(TFK_ERR_INVALID_ARG, "tfk_inverse: lambda must be finite and > 0");
    if (!(isfinite(params->step_max) && params->step_max > 0.0f)) return fail(TFK_ERR_INVALID_ARG, "tfk_inverse: step_max must be finite and > 0");
    hipLaunchKernelGGL(k_inverse, grid_of(N), dim3(KIN_BLOCK), 0, (hipStream_t)stream, h->P, dev(target), dev(q0), dev(base_off), (int)params->iters,
                       params->lambda * params->lambda, params->step_max, q_out, residual, (int)N);
    return launched("tfk_inverse: ");
}

int tfk_tip_action(tfk_handle h, const TfkActionParams* params, TfkArray cmd, TfkArray q, TfkArray qd, TfkArray base_off, float* action,
                   float* target_out, int32_t N, void* stream) {
    if (!h || !params || !action) return fail(TFK_ERR_INVALID_ARG, "tfk_tip_action: NULL handle, params or action");
    if (N < 1 || N > TF_MAX_ENVS) return fail(TFK_ERR_INVALID_ARG, "tfk_tip_action: N outside [1, TF_MAX_ENVS]");
    const TfkActionParams& a = *params;
    if (a.frame != TFK_FRAME_DELTA && a.frame != TFK_FRAME_ABSOLUTE) return fail(TFK_ERR_INVALID_ARG, "tfk_tip_action: frame");
    if (a.mode != TFK_MODE_POSITION && a.mode != TFK_MODE_TORQUE) return fail(TFK_ERR_INVALID_ARG, "tfk_tip_action: mode");
    if (!array_ok(cmd, true) || !array_ok(q, true) || !array_ok(qd, a.mode == TFK_MODE_TORQUE) || !array_ok(base_off, false))
        return fail(TFK_ERR_INVALID_ARG, "tfk_tip_action: cmd, q (and qd in torque mode) need a pointer; strides lie in [0, 2^31)");
    if (!(all_finite(a.box_lo, 3) && all_finite(a.box_hi, 3))) return fail(TFK_ERR_INVALID_ARG, "tfk_tip_action: box not finite");
    for (int j = 0; j < 3; ++j)
        if (!(a.box_lo[j] <= a.box_hi[j])) return fail(TFK_ERR_INVALID_ARG, "tfk_tip_action: box_lo > box_hi");
    if (a.frame == TFK_FRAME_DELTA && !(isfinite(a.delta_scale) && a.delta_scale > 0.0f))
        return fail(TFK_ERR_INVALID_ARG, "tfk_tip_action: delta_scale must be finite and > 0");
    if (a.mode == TFK_MODE_POSITION) {
        if (a.iters < 1 || a.iters > TFK_MAX_ACTION_ITERS) return fail(TFK_ERR_INVALID_ARG, "tfk_tip_action: iters outside [1, TFK_MAX_ACTION_ITERS]");
        if (!(isfinite(a.lambda) && a.lambda > 0.0f)) return fail(TFK_ERR_INVALID_ARG, "tfk_tip_action: lambda must be finite and > 0");
        if (!(isfinite(a.step_max) && a.step_max > 0.0f)) return fail(TFK_ERR_INVALID_ARG, "tfk_tip_action: step_max must be finite and > 0");
    } else {
        if (!(all_finite(a.kp, 3) && all_finite(a.kd, 3))) return fail(TFK_ERR_INVALID_ARG, "tfk_tip_action: kp / kd not finite");
        for (int j = 0; j < 3; ++j)
            if (a.kp[j] < 0.0f || a.kd[j] < 0.0f) return fail(TFK_ERR_INVALID_ARG, "tfk_tip_action: kp / kd negative");
        if (a.gravity_comp && !all_finite(a.gravity, 3)) return fail(TFK_ERR_INVALID_ARG, "tfk_tip_action: gravity not finite");
    }
    const float lam2 = a.mode == TFK_MODE_POSITION ? a.lambda * a.lambda : 0.0f;
    hipLaunchKernelGGL(k_tip_action, grid_of(N), dim3(KIN_BLOCK), 0, (hipStream_t)stream, h->P, a, lam2, dev(cmd), dev(q),
                       a.mode == TFK_MODE_TORQUE ? dev(qd) : NO_ARRAY, dev(base_off), action, target_out, (int)N);
    return launched("tfk_tip_action: ");
}

}  // extern "C"
