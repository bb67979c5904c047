// tf_render.hip - offscreen renderer of the collision model (include/trifinger_render.h): libtrifinger_render.so.
//
// One workgroup = one 16 x 16 pixel tile of one view, four wavefronts of 8 x 8 pixels each: the march is a divergent loop and a wavefront runs as
// long as its slowest ray, so neighbouring rays share one.  Four lanes of wavefront 0 build the env's scene (nine link frames, nine sphere centres,
// the bounding spheres of the link shapes, object and goal pose, stage offset: 212 floats) in LDS from the state rows with the step's own kinematics (fk_setup, rot_link, base_to_world of
// tf_device_math.h), one barrier, then every lane marches its ray; the scene reads are wave-uniform LDS broadcasts, the shape constants and the
// camera scalar loads of the kernel argument.  Floor and goal are closed-form per ray.  The kernel only reads `state`; the march is bounded by
// max_steps whatever the data.
#include "tf_contact.h"
#include "../../include/trifinger_render.h"

#include <math.h>
#include <stdio.h>
#include <string.h>

// ---- what travels with every launch (kernel argument: scalar loads) ----
struct RShape {                   // a TfLinkShape with its linear quantities as (value at s = 0, difference to s = 1)
    float a[3], d[3], inv_dd;
    float rho[2], h1[2], h2[2], o1[2], o2[2];     // h = w - rho
};
struct RParams {
    DevModel m;                   // kinematics of fk_setup
    RShape sh[3];                 // shape1, shape2, shape3
    float sph_c[3][3], sph_r[3];  // sph2[0], sph2[1], sph3[0] (link 2, 2, 3)
    float bs_c[3][3], bs_r[3];    // bounding sphere of shape l: axis midpoint (link frame), half length + largest extent + a margin
    float obj_half[3];
    float wall_s[3], wall_c[3], wall_sn[3];
    // camera
    float eye[3], fw[3], rt[3], up[3], tan_x, tan_y;
    int32_t width, height, n_views, num_envs, max_steps, shading;
    float eps, relax, t_max;
    int32_t env_ids[TFR_MAX_VIEWS];
};

struct Scene {                    // LDS
    float R[9][9], o[9][3];       // frame of link l of finger f at [3 f + l]: world = R local + o (R row-major)
    float sc[9][3];               // sphere centres (world), finger f at [3 f ..]
    float bc[9][3];               // centres of the bounding spheres of the link shapes (world), as R / o
    float oR[9], op[3], oh[3];    // object
    float gR[9], gp[3];           // goal (half extents: the object's)
    float soff[2];                // stage centre
};

#define R_SQRT(x) __builtin_amdgcn_sqrtf(x)
#define R_RSQ(x) __builtin_amdgcn_rsqf(x)
#define R_RCP(x) __builtin_amdgcn_rcpf(x)
#define R_INF __builtin_inff()

__device__ static const uint8_t PALETTE[TFR_NUM_IDS + 1][3] = {
    {24, 24, 28},
    {230, 60, 60}, {200, 40, 40}, {255, 100, 100}, {170, 30, 30}, {150, 20, 20}, {130, 10, 10},
    {60, 230, 60}, {40, 200, 40}, {100, 255, 100}, {30, 170, 30}, {20, 150, 20}, {10, 130, 10},
    {60, 60, 230}, {40, 40, 200}, {100, 100, 255}, {30, 30, 170}, {20, 20, 150}, {10, 10, 130},
    {0, 0, 0},
    {235, 200, 40}, {120, 122, 126}, {176, 150, 118},
    {60, 220, 220},               // [TFR_NUM_IDS]: the goal ghost
};

// ---- scene construction: one lane per finger, one for object / goal / stage ----
template <int LINK> DEV void store_frame(Scene& S, int idx, const Yaw& yw, const FK& k, const float boff[3]) {
#pragma unroll
    for (int j = 0; j < 3; ++j) {
        const float e[3] = {j == 0 ? 1.0f : 0.0f, j == 1 ? 1.0f : 0.0f, j == 2 ? 1.0f : 0.0f};
        float cb[3], cw[3];
        rot_link<LINK>(k, e, cb);
        dir_base_to_world(yw, cb, cw);
        S.R[idx][j] = cw[0]; S.R[idx][3 + j] = cw[1]; S.R[idx][6 + j] = cw[2];
    }
    const float zero[3] = {0.0f, 0.0f, 0.0f};
    float ob[3], ow[3];
    link_point<LINK>(k, zero, ob);
    base_to_world(yw, ob, ow);
#pragma unroll
    for (int j = 0; j < 3; ++j) S.o[idx][j] = ow[j] + boff[j];
}
template <int LINK> DEV void store_point(float out[3], const Yaw& yw, const FK& k, const float boff[3], const float c[3]) {
    float pb[3], pw[3];
    link_point<LINK>(k, c, pb);
    base_to_world(yw, pb, pw);
#pragma unroll
    for (int j = 0; j < 3; ++j) out[j] = pw[j] + boff[j];
}
DEV void build_scene(const RParams& P, const float* __restrict__ state, int env, int lane, Scene& S) {
    const int N = P.num_envs;
    auto LD = [&](int row) { return state[(size_t)row * (size_t)N + (size_t)env]; };
    if (lane < 3) {
        const int f = lane;
        const DevModel& m = P.m;
        const Yaw yw = {m.base_yaw_cos[f], m.base_yaw_sin[f], m.base_half_yaw_cos[f], m.base_half_yaw_sin[f], m.base_height};
        const float q[3] = {LD(TF_S_Q + 3 * f), LD(TF_S_Q + 3 * f + 1), LD(TF_S_Q + 3 * f + 2)};
        const float boff[3] = {LD(TF_S_DR + TF_DR_BASE_POS), LD(TF_S_DR + TF_DR_BASE_POS + 1), LD(TF_S_DR + TF_DR_BASE_POS + 2)};
        FK k;
        fk_setup(m, q, k);
        store_frame<1>(S, 3 * f, yw, k, boff);
        store_frame<2>(S, 3 * f + 1, yw, k, boff);
        store_frame<3>(S, 3 * f + 2, yw, k, boff);
        store_point<2>(S.sc[3 * f], yw, k, boff, P.sph_c[0]);
        store_point<2>(S.sc[3 * f + 1], yw, k, boff, P.sph_c[1]);
        store_point<3>(S.sc[3 * f + 2], yw, k, boff, P.sph_c[2]);
        store_point<1>(S.bc[3 * f], yw, k, boff, P.bs_c[0]);
        store_point<2>(S.bc[3 * f + 1], yw, k, boff, P.bs_c[1]);
        store_point<3>(S.bc[3 * f + 2], yw, k, boff, P.bs_c[2]);
    } else if (lane == 3) {
        const float size = LD(TF_S_DR + TF_DR_CUBE_SIZE);
        float q[4], R[9];
#pragma unroll
        for (int j = 0; j < 4; ++j) q[j] = LD(TF_S_CUBE_Q + j);
        quat_to_rot(q, R);
#pragma unroll
        for (int j = 0; j < 9; ++j) S.oR[j] = R[j];
#pragma unroll
        for (int j = 0; j < 4; ++j) q[j] = LD(TF_S_GOAL_Q + j);
        quat_to_rot(q, R);
#pragma unroll
        for (int j = 0; j < 9; ++j) S.gR[j] = R[j];
#pragma unroll
        for (int j = 0; j < 3; ++j) { S.op[j] = LD(TF_S_CUBE_P + j); S.gp[j] = LD(TF_S_GOAL_P + j); S.oh[j] = P.obj_half[j] * size; }
        S.soff[0] = LD(TF_S_DR + TF_DR_STAGE_POS); S.soff[1] = LD(TF_S_DR + TF_DR_STAGE_POS + 1);
    }
}

// ---- fields ----
template <int LK> DEV float shape_dist(const RShape& c, const float* R, const float* o, const float p[3]) {
    const float dd[3] = {p[0] - o[0], p[1] - o[1], p[2] - o[2]};
    float pl[3];
    mat3T_mul(R, dd, pl);
    const float e0[3] = {pl[0] - c.a[0], pl[1] - c.a[1], pl[2] - c.a[2]};
    const float s = f_clamp(dot3(e0, c.d) * c.inv_dd, 0.0f, 1.0f);
    const float e[3] = {e0[0] - s * c.d[0], e0[1] - s * c.d[1], e0[2] - s * c.d[2]};
    const float D2 = f_max(dot3(e, e), 1e-24f);
    const float inv = R_RSQ(D2);
    const float D = D2 * inv;
    const float u1 = e[0] * inv, u2 = ((LK == 1) ? e[2] : e[1]) * inv;
    const float rho = c.rho[0] + s * c.rho[1], h1 = c.h1[0] + s * c.h1[1], h2 = c.h2[0] + s * c.h2[1];
    const float o1 = c.o1[0] + s * c.o1[1], o2 = c.o2[0] + s * c.o2[1];
    return D - (rho + h1 * f_abs(u1) + h2 * f_abs(u2) + o1 * u1 + o2 * u2);
}
DEV float sphere_dist(const float* c, float radius, const float p[3]) {
    const float e[3] = {p[0] - c[0], p[1] - c[1], p[2] - c[2]};
    return R_SQRT(dot3(e, e)) - radius;
}
DEV float box_dist(const float* R, const float* c, const float* h, const float p[3]) {
    const float dd[3] = {p[0] - c[0], p[1] - c[1], p[2] - c[2]};
    float l[3];
    mat3T_mul(R, dd, l);
    const float q0 = f_abs(l[0]) - h[0], q1 = f_abs(l[1]) - h[1], q2 = f_abs(l[2]) - h[2];
    const float a0 = f_max(q0, 0.0f), a1 = f_max(q1, 0.0f), a2 = f_max(q2, 0.0f);
    return R_SQRT(a0 * a0 + a1 * a1 + a2 * a2) + f_min(f_max(q0, f_max(q1, q2)), 0.0f);
}
// Minimum over link shapes, spheres and object; ties to the lower id.  The cheap exact fields (spheres, object) come first; a link shape is
// evaluated only where its bounding sphere is not farther than the minimum so far: its field is at least the distance to that sphere (the
// closest axis point lies within half a length of the midpoint, the extent is at most its largest value), so a skipped shape can neither be
// the minimum nor tie it - the result is the one of visiting everything in id order.
template <bool WANT_ID> DEV float scene_dist(const RParams& P, const Scene& S, const float p[3], int& id) {
    float best = R_INF;
    int bid = 0;
    auto take = [&](float d, int i) {
        if (WANT_ID) { bid = ((d < best) || (d == best && i < bid)) ? i : bid; }
        best = f_min(best, d);
    };
#pragma unroll 1
    for (int f = 0; f < 3; ++f) {
        const int b = 3 * f, i0 = 1 + 6 * f;
        take(sphere_dist(S.sc[b], P.sph_r[0], p), i0 + 3);
        take(sphere_dist(S.sc[b + 1], P.sph_r[1], p), i0 + 4);
        take(sphere_dist(S.sc[b + 2], P.sph_r[2], p), i0 + 5);
    }
    take(box_dist(S.oR, S.op, S.oh, p), TFR_ID_OBJECT);
#pragma unroll 1
    for (int f = 0; f < 3; ++f) {
        const int b = 3 * f, i0 = 1 + 6 * f;
        if (sphere_dist(S.bc[b], P.bs_r[0], p) <= best) take(shape_dist<1>(P.sh[0], S.R[b], S.o[b], p), i0);
        if (sphere_dist(S.bc[b + 1], P.bs_r[1], p) <= best) take(shape_dist<2>(P.sh[1], S.R[b + 1], S.o[b + 1], p), i0 + 1);
        if (sphere_dist(S.bc[b + 2], P.bs_r[2], p) <= best) take(shape_dist<3>(P.sh[2], S.R[b + 2], S.o[b + 2], p), i0 + 2);
    }
    id = bid;
    return best;
}
// the boundary field; nrm (optional): the inward surface normal there
template <bool WANT_N> DEV float boundary_dist(const RParams& P, const Scene& S, const float p[3], float nrm[3]) {
    const DevModel& m = P.m;
    const float x = p[0] - S.soff[0], y = p[1] - S.soff[1], z = p[2];
    const float rho = R_SQRT(x * x + y * y);
    const bool b0 = z > m.wall_z[0], b1 = z > m.wall_z[1], b2 = z > m.wall_z[2];
    float r = m.wall_r[0], c = 1.0f, sn = 0.0f;
    r = b0 ? m.wall_r[0] + (z - m.wall_z[0]) * P.wall_s[0] : r;  c = b0 ? P.wall_c[0] : c;  sn = b0 ? P.wall_sn[0] : sn;
    r = b1 ? m.wall_r[1] + (z - m.wall_z[1]) * P.wall_s[1] : r;  c = b1 ? P.wall_c[1] : c;  sn = b1 ? P.wall_sn[1] : sn;
    r = b2 ? m.wall_r[2] + (z - m.wall_z[2]) * P.wall_s[2] : r;  c = b2 ? P.wall_c[2] : c;  sn = b2 ? P.wall_sn[2] : sn;
    const bool below = z < m.wall_z[3];
    const float er = rho - m.wall_r[3], ez = z - m.wall_z[3];
    const float drim = R_SQRT(er * er + ez * ez);
    if (WANT_N) {
        const float ir = R_RCP(f_max(rho, 1e-12f)), nx = x * ir, ny = y * ir;
        const float id = R_RCP(f_max(drim, 1e-12f));
        nrm[0] = below ? -(c * nx) : (er * id) * nx;
        nrm[1] = below ? -(c * ny) : (er * id) * ny;
        nrm[2] = below ? sn : ez * id;
    }
    return below ? f_abs((r - rho) * c) : drim;
}

// closed-form ray / box (slab method in the box frame): entry parameter (0 from inside), +inf for a miss
DEV float ray_box(const float* R, const float* c, const float* h, const float eye[3], const float d[3]) {
    const float eo[3] = {eye[0] - c[0], eye[1] - c[1], eye[2] - c[2]};
    float o[3], dl[3];
    mat3T_mul(R, eo, o);
    mat3T_mul(R, d, dl);
    float tn = -R_INF, tf = R_INF;
    bool miss = false;
#pragma unroll
    for (int i = 0; i < 3; ++i) {
        const bool par = f_abs(dl[i]) < 1e-12f;
        const float inv = 1.0f / (par ? 1.0f : dl[i]);
        const float t1 = (-h[i] - o[i]) * inv, t2 = (h[i] - o[i]) * inv;
        miss = miss || (par && f_abs(o[i]) > h[i]);
        tn = par ? tn : f_max(tn, f_min(t1, t2));
        tf = par ? tf : f_min(tf, f_max(t1, t2));
    }
    const bool hit = !miss && tn <= tf && tf > 0.0f;
    return hit ? f_max(tn, 0.0f) : R_INF;
}

DEV void pixel_ray(const RParams& P, int px, int py, float d[3]) {
    const float x = (((float)px + 0.5f) / (float)P.width * 2.0f - 1.0f) * P.tan_x;
    const float y = (1.0f - ((float)py + 0.5f) / (float)P.height * 2.0f) * P.tan_y;
    float v[3];
#pragma unroll
    for (int j = 0; j < 3; ++j) v[j] = P.fw[j] + x * P.rt[j] + y * P.up[j];
    const float inv = 1.0f / __builtin_sqrtf(dot3(v, v));
#pragma unroll
    for (int j = 0; j < 3; ++j) d[j] = v[j] * inv;
}

__global__ __launch_bounds__(256) void k_render(const RParams P, const float* __restrict__ state, uint32_t* __restrict__ color,
                                                float* __restrict__ depth, uint8_t* __restrict__ seg) {
    __shared__ Scene S;
    const int tid = (int)threadIdx.x, wave = tid >> 6, lane = tid & 63;
    const int view = (int)blockIdx.z;
    if (wave == 0) build_scene(P, state, P.env_ids[view], lane, S);
    __syncthreads();
    const int px = (int)blockIdx.x * 16 + (wave & 1) * 8 + (lane & 7);
    const int py = (int)blockIdx.y * 16 + (wave >> 1) * 8 + (lane >> 3);
    if (px >= P.width || py >= P.height) return;

    const float eye[3] = {P.eye[0], P.eye[1], P.eye[2]};
    float d[3];
    pixel_ray(P, px, py, d);
    // closed forms of the ray: floor-plane crossing, whether it lies on the disc, closest approach to the stage axis
    const float tfl = (d[2] < 0.0f) ? -eye[2] / f_min(d[2], -1e-9f) : R_INF;
    const float ex = eye[0] - S.soff[0], ey = eye[1] - S.soff[1];
    const float tc = -(ex * d[0] + ey * d[1]) / f_max(d[0] * d[0] + d[1] * d[1], 1e-12f);
    const float fx = ex + tfl * d[0], fy = ey + tfl * d[1];
    const bool on_disc = (fx * fx + fy * fy) <= P.m.wall_r[0] * P.m.wall_r[0];

    float t = 0.0f;
    int hit = 0;
    float p[3];
    for (int it = 0; it < P.max_steps; ++it) {
#pragma unroll
        for (int j = 0; j < 3; ++j) p[j] = eye[j] + t * d[j];
        int id;
        const float ds = scene_dist<true>(P, S, p, id);
        const bool after = t >= tc;
        const float db = after ? boundary_dist<false>(P, S, p, nullptr) : R_INF;
        if (ds < P.eps) { hit = id; break; }
        if (db < P.eps) { hit = TFR_ID_BOUNDARY; break; }
        t = after ? t + P.relax * f_min(ds, db) : f_min(t + P.relax * ds, f_max(tc, t + P.eps));
        if (t >= tfl) { t = tfl; hit = on_disc ? TFR_ID_FLOOR : -1; break; }
        if (t > P.t_max) break;
    }
    const bool solid = hit > 0;
    const int id = solid ? hit : 0;
    const float z = solid ? t : R_INF;

    float shade = 1.0f;
    if (P.shading == TFR_SHADING_LIT && solid) {
        float n[3] = {0.0f, 0.0f, 1.0f};
#pragma unroll
        for (int j = 0; j < 3; ++j) p[j] = eye[j] + t * d[j];
        if (id <= TFR_ID_OBJECT) {
            const float h = 5e-4f;
            int dummy;
#pragma unroll 1
            for (int j = 0; j < 3; ++j) {
                float pa[3] = {p[0], p[1], p[2]}, pb[3] = {p[0], p[1], p[2]};
                pa[j] += h; pb[j] -= h;
                n[j] = scene_dist<false>(P, S, pa, dummy) - scene_dist<false>(P, S, pb, dummy);
            }
            const float inv = R_RSQ(f_max(dot3(n, n), 1e-30f));
            n[0] *= inv; n[1] *= inv; n[2] *= inv;
        } else if (id == TFR_ID_BOUNDARY) {
            boundary_dist<true>(P, S, p, n);
        }
        const float L[3] = {0.35080324f, 0.25057375f, 0.90206549f};       // (0.35, 0.25, 0.9) / |.|
        shade = 0.35f + 0.65f * f_max(dot3(n, L), 0.0f);
    }
    uint32_t c[3];
#pragma unroll
    for (int j = 0; j < 3; ++j) {
        const float v = (float)PALETTE[id][j] * shade;
        c[j] = (uint32_t)f_min(__builtin_floorf(v + 0.5f), 255.0f);
    }
    // the goal ghost: over whatever lies behind it
    const float tg = ray_box(S.gR, S.gp, S.oh, eye, d);
    if (tg < z) {
#pragma unroll
        for (int j = 0; j < 3; ++j) c[j] = (c[j] + (uint32_t)PALETTE[TFR_NUM_IDS][j] + 1u) >> 1;
    }
    const size_t pix = ((size_t)view * (size_t)P.height + (size_t)py) * (size_t)P.width + (size_t)px;
    color[pix] = c[0] | (c[1] << 8) | (c[2] << 16) | 0xff000000u;
    if (depth) depth[pix] = z;
    if (seg) seg[pix] = (uint8_t)id;
}

__global__ __launch_bounds__(256) void k_test_field(const RParams P, const float* __restrict__ state, int env, const float* __restrict__ points,
                                                    float* __restrict__ dist, uint8_t* __restrict__ ids, float* __restrict__ bdist, int n) {
    __shared__ Scene S;
    const int tid = (int)threadIdx.x;
    if (tid < 64) build_scene(P, state, env, tid, S);
    __syncthreads();
    const int i = (int)blockIdx.x * 256 + tid;
    if (i >= n) return;
    const float p[3] = {points[3 * (size_t)i], points[3 * (size_t)i + 1], points[3 * (size_t)i + 2]};
    int id;
    const float ds = scene_dist<true>(P, S, p, id);
    if (dist) dist[i] = ds;
    if (ids) ids[i] = (uint8_t)id;
    if (bdist) bdist[i] = boundary_dist<false>(P, S, p, nullptr);
}

// ------------------------------------------------------------------------------------------------------
// host
// ------------------------------------------------------------------------------------------------------
struct tfr_handle_s {
    RParams P;
    int32_t max_views;
    bool bound;
};

static thread_local char g_err[512] = "";
static int fail(int status, const char* what, const char* detail = "") {
    snprintf(g_err, sizeof(g_err), "%s%s", what, detail);
    return status;
}

static void set_shape(RShape& r, const TfLinkShape& s) {
    double dd = 0.0;
    for (int j = 0; j < 3; ++j) { r.a[j] = s.a[j]; r.d[j] = s.b[j] - s.a[j]; dd += (double)r.d[j] * (double)r.d[j]; }
    r.inv_dd = (float)(1.0 / dd);
    const float h1a = s.w1[0] - s.rho[0], h1b = s.w1[1] - s.rho[1], h2a = s.w2[0] - s.rho[0], h2b = s.w2[1] - s.rho[1];
    r.rho[0] = s.rho[0]; r.rho[1] = s.rho[1] - s.rho[0];
    r.h1[0] = h1a; r.h1[1] = h1b - h1a;
    r.h2[0] = h2a; r.h2[1] = h2b - h2a;
    r.o1[0] = s.o1[0]; r.o1[1] = s.o1[1] - s.o1[0];
    r.o2[0] = s.o2[0]; r.o2[1] = s.o2[1] - s.o2[0];
}
// bounding sphere of a link shape: every point of its surface and its outside has a field >= |p - c| - r
static void set_bound(float c[3], float& r, const TfLinkShape& s) {
    double half = 0.0, ext = 0.0;
    for (int j = 0; j < 3; ++j) { c[j] = 0.5f * (s.a[j] + s.b[j]); const double d = 0.5 * ((double)s.b[j] - (double)s.a[j]); half += d * d; }
    for (int e = 0; e < 2; ++e)
        ext = fmax(ext, (double)s.rho[e] + fabs((double)s.w1[e] - s.rho[e]) + fabs((double)s.w2[e] - s.rho[e]) + fabs((double)s.o1[e]) + fabs((double)s.o2[e]));
    r = (float)(sqrt(half) + ext + 1e-5);          // the margin covers the fp32 rounding of both sides, a thousand times over
}
static bool shape_ok(const TfLinkShape& s) {
    double dd = 0.0;
    for (int j = 0; j < 3; ++j) { const double d = (double)s.b[j] - (double)s.a[j]; dd += d * d; }
    return std::isfinite(dd) && dd > 1e-12;
}

static int camera(RParams& P, const float eye[3], const float target[3], float fov) {
    if (!(fov > 1e-3f && fov < 3.1f)) return fail(TF_ERR_INVALID_ARG, "tfr_set_camera: fov_y_rad outside (0.001, 3.1)");
    double f[3], r[3], u[3], n = 0.0;
    for (int j = 0; j < 3; ++j) { if (!std::isfinite(eye[j]) || !std::isfinite(target[j])) return fail(TF_ERR_INVALID_ARG, "tfr_set_camera: non-finite"); }
    for (int j = 0; j < 3; ++j) { f[j] = (double)target[j] - (double)eye[j]; n += f[j] * f[j]; }
    if (!(n > 1e-12)) return fail(TF_ERR_INVALID_ARG, "tfr_set_camera: eye == target");
    n = sqrt(n);
    for (int j = 0; j < 3; ++j) f[j] /= n;
    r[0] = f[1]; r[1] = -f[0]; r[2] = 0.0;                     // f x (0, 0, 1)
    n = sqrt(r[0] * r[0] + r[1] * r[1]);
    if (!(n > 1e-6)) return fail(TF_ERR_INVALID_ARG, "tfr_set_camera: the view direction is vertical (z is up)");
    r[0] /= n; r[1] /= n;
    u[0] = r[1] * f[2] - r[2] * f[1]; u[1] = r[2] * f[0] - r[0] * f[2]; u[2] = r[0] * f[1] - r[1] * f[0];      // r x f
    for (int j = 0; j < 3; ++j) { P.eye[j] = eye[j]; P.fw[j] = (float)f[j]; P.rt[j] = (float)r[j]; P.up[j] = (float)u[j]; }
    const double th = tan(0.5 * (double)fov);
    P.tan_y = (float)th;
    P.tan_x = (float)(th * (double)P.width / (double)P.height);
    return TF_OK;
}

extern "C" {

int tfr_api_version(void) { return TFR_API_VERSION; }
const char* tfr_last_error_string(void) { return g_err; }

void tfr_default_config(TfrConfig* c) {
    if (!c) return;
    c->api_version = TFR_API_VERSION;
    c->width = 256; c->height = 256; c->max_views = 16;
    c->max_steps = 160; c->shading = TFR_SHADING_LIT;
    c->eps = 1e-4f; c->relax = 0.9f; c->t_max = 2.0f;
}

int tfr_create(const TfModel* model, const TfrConfig* cfg, tfr_handle* out) {
    if (!model || !cfg || !out) return fail(TF_ERR_INVALID_ARG, "tfr_create: NULL argument");
    if (cfg->api_version != TFR_API_VERSION) return fail(TF_ERR_INVALID_ARG, "tfr_create: api_version");
    if (cfg->width < 1 || cfg->width > TFR_MAX_SIZE || cfg->height < 1 || cfg->height > TFR_MAX_SIZE)
        return fail(TF_ERR_INVALID_ARG, "tfr_create: width / height outside [1, 4096]");
    if (cfg->max_views < 1 || cfg->max_views > TFR_MAX_VIEWS) return fail(TF_ERR_INVALID_ARG, "tfr_create: max_views outside [1, 64]");
    if (cfg->max_steps < 1 || cfg->max_steps > 4096) return fail(TF_ERR_INVALID_ARG, "tfr_create: max_steps outside [1, 4096]");
    if (cfg->shading != TFR_SHADING_FLAT && cfg->shading != TFR_SHADING_LIT) return fail(TF_ERR_INVALID_ARG, "tfr_create: shading");
    if (!(cfg->eps > 0.0f && cfg->eps < 1.0f) || !(cfg->relax > 0.0f && cfg->relax <= 1.0f) || !(cfg->t_max > 0.0f && cfg->t_max < 1e6f))
        return fail(TF_ERR_INVALID_ARG, "tfr_create: eps in (0, 1), relax in (0, 1], t_max in (0, 1e6)");
    if (!shape_ok(model->shape1) || !shape_ok(model->shape2) || !shape_ok(model->shape3))
        return fail(TF_ERR_INVALID_ARG, "tfr_create: a link shape has no axis");
    for (int i = 0; i < 4; ++i)
        if (!std::isfinite(model->wall_r[i]) || !std::isfinite(model->wall_z[i]) || (i > 0 && !(model->wall_z[i] > model->wall_z[i - 1])))
            return fail(TF_ERR_INVALID_ARG, "tfr_create: boundary knots must be finite and rise strictly");
    tfr_handle h = new tfr_handle_s();
    memset(h, 0, sizeof(*h));
    RParams& P = h->P;
    memcpy(&P.m, model, sizeof(DevModel));
    set_shape(P.sh[0], model->shape1); set_shape(P.sh[1], model->shape2); set_shape(P.sh[2], model->shape3);
    set_bound(P.bs_c[0], P.bs_r[0], model->shape1); set_bound(P.bs_c[1], P.bs_r[1], model->shape2); set_bound(P.bs_c[2], P.bs_r[2], model->shape3);
    const TfSphere* sp[3] = {&model->sph2[0], &model->sph2[1], &model->sph3[0]};
    for (int i = 0; i < 3; ++i) { for (int j = 0; j < 3; ++j) P.sph_c[i][j] = sp[i]->c[j]; P.sph_r[i] = sp[i]->radius; }
    for (int j = 0; j < 3; ++j) P.obj_half[j] = model->box ? model->box_half[j] : model->cube_half;
    for (int i = 0; i < 3; ++i) {                                  // as tf_create derives them
        const double sl = ((double)model->wall_r[i + 1] - (double)model->wall_r[i]) / ((double)model->wall_z[i + 1] - (double)model->wall_z[i]);
        P.wall_s[i] = (float)sl;
        P.wall_c[i] = (float)(1.0 / sqrt(1.0 + sl * sl));
        P.wall_sn[i] = (float)(sl / sqrt(1.0 + sl * sl));
    }
    P.width = cfg->width; P.height = cfg->height;
    P.max_steps = cfg->max_steps; P.shading = cfg->shading;
    P.eps = cfg->eps; P.relax = cfg->relax; P.t_max = cfg->t_max;
    h->max_views = cfg->max_views;
    const float eye[3] = {0.55f, 0.35f, 0.50f}, target[3] = {0.0f, 0.0f, 0.10f};
    camera(P, eye, target, 0.78539816339744831f);
    *out = h;
    return TF_OK;
}

int tfr_destroy(tfr_handle h) {
    if (!h) return fail(TF_ERR_INVALID_ARG, "tfr_destroy: NULL handle");
    delete h;
    return TF_OK;
}

int tfr_set_camera(tfr_handle h, const float eye[3], const float target[3], float fov_y_rad) {
    if (!h || !eye || !target) return fail(TF_ERR_INVALID_ARG, "tfr_set_camera: NULL argument");
    RParams P = h->P;
    const int rc = camera(P, eye, target, fov_y_rad);
    if (rc == TF_OK) h->P = P;
    return rc;
}

int tfr_set_views(tfr_handle h, const int32_t* env_ids, int32_t n_views, int32_t num_envs) {
    if (!h || !env_ids) return fail(TF_ERR_INVALID_ARG, "tfr_set_views: NULL argument");
    if (num_envs < 1 || num_envs > TF_MAX_ENVS) return fail(TF_ERR_INVALID_ARG, "tfr_set_views: num_envs outside [1, TF_MAX_ENVS]");
    if (n_views < 1 || n_views > h->max_views) return fail(TF_ERR_INVALID_ARG, "tfr_set_views: n_views outside [1, max_views]");
    for (int i = 0; i < n_views; ++i)
        if (env_ids[i] < 0 || env_ids[i] >= num_envs) return fail(TF_ERR_INVALID_ARG, "tfr_set_views: env id outside [0, num_envs)");
    for (int i = 0; i < TFR_MAX_VIEWS; ++i) h->P.env_ids[i] = (i < n_views) ? env_ids[i] : 0;
    h->P.n_views = n_views;
    h->P.num_envs = num_envs;
    h->bound = true;
    return TF_OK;
}

int tfr_render(tfr_handle h, const float* state, uint8_t* color, float* depth, uint8_t* segmentation, void* stream) {
    if (!h || !state || !color) return fail(TF_ERR_INVALID_ARG, "tfr_render: NULL argument");
    if (!h->bound) return fail(TF_ERR_NOT_BOUND, "tfr_render before tfr_set_views");
    const RParams& P = h->P;
    const dim3 grid((unsigned)((P.width + 15) / 16), (unsigned)((P.height + 15) / 16), (unsigned)P.n_views);
    hipLaunchKernelGGL(k_render, grid, dim3(256), 0, (hipStream_t)stream, P, state, (uint32_t*)color, depth, segmentation);
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return fail(TF_ERR_DEVICE, "tfr_render: ", hipGetErrorString(e));
    return TF_OK;
}

int tfr_test_field(tfr_handle h, const float* state, int32_t env, const float* points, float* dist, uint8_t* id, float* boundary_dist,
                   int32_t n, void* stream) {
    if (!h || !state || !points) return fail(TF_ERR_INVALID_ARG, "tfr_test_field: NULL argument");
    if (!h->bound) return fail(TF_ERR_NOT_BOUND, "tfr_test_field before tfr_set_views");
    if (env < 0 || env >= h->P.num_envs) return fail(TF_ERR_INVALID_ARG, "tfr_test_field: env outside [0, num_envs)");
    if (n < 1 || n > (1 << 26)) return fail(TF_ERR_INVALID_ARG, "tfr_test_field: n outside [1, 2^26]");
    hipLaunchKernelGGL(k_test_field, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, (hipStream_t)stream, h->P, state, (int)env, points, dist, id,
                       boundary_dist, (int)n);
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return fail(TF_ERR_DEVICE, "tfr_test_field: ", hipGetErrorString(e));
    return TF_OK;
}

}  // extern "C"
