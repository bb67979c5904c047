/* trifinger_render.h - C ABI of the offscreen renderer of the TriFinger COLLISION MODEL (libtrifinger_render.so).
 *
 * A picture of exactly what the contact code collides: the implicit surfaces of the contact queries of the step (include/trifinger.h: TfLinkShape,
 * TfSphere, the object box, the floor disc and the boundary profile), ray-marched on the GPU from the resident state[TF_STATE_ROWS][num_envs] rows.
 * No meshes, no textures, no window.  The library shares no object with libtrifinger_hip.so; the kernel only READS the state.
 *
 * Conventions: plain C, opaque handle, POD structs, raw device pointers, streams as void* (hipStream_t), TfStatus return codes
 * (tfr_last_error_string has the text).  Nothing allocates or synchronises after tfr_create.
 *
 * THE SCENE of one env (from its state rows and the TfModel given at tfr_create):
 *   finger links   frames as the step builds them: world = Rz(yaw_f) base + (0, 0, base_height) + state[TF_S_DR + TF_DR_BASE_POS ..+2];
 *                  bodies shape1, shape2, shape3 and the spheres sph2[0], sph2[1], sph3[0] of every finger, always.  Field of a TfLinkShape at a
 *                  point p of the link frame: the step's gap formula against a point - s the parameter of the closest point x(s) of the axis,
 *                  D = |p - x|, u = (p - x) / D,  D - [(w1 - rho) |u1| + (w2 - rho) |u2| + rho + o1 u1 + o2 u2]  with (u1, u2) along (x, z) for the
 *                  upper link and (x, y) for the other two (u = 0 where D < 1e-12).  Sphere: |p - c| - radius.
 *   object         exact box distance (negative inside); half extents cube_half (or box_half[] when model.box != 0) x state[TF_S_DR + TF_DR_CUBE_SIZE]
 *                  at TF_S_CUBE_P, TF_S_CUBE_Q (xyzw)
 *   floor          the disc z = 0, rho <= wall_r[0] about the stage centre state[TF_S_DR + TF_DR_STAGE_POS ..+1], intersected in closed form; a ray
 *                  that crosses z = 0 outside the disc ends there as background
 *   boundary       the profile r(z) through (wall_z[i], wall_r[i]) about the stage centre: field |(r(z) - rho) c| below wall_z[3] (c the cosine of
 *                  the slope angle of the segment, 1 on the vertical ring), distance to the rim circle (wall_r[3], wall_z[3]) above.  Drawn as its
 *                  INNER surface only: it exists for t >= t_c, the ray's closest approach to the stage axis
 *   goal           TF_S_GOAL_P, TF_S_GOAL_Q with the object's half extents: no collider - a ghost (closed-form ray / box), blended over the colour
 *                  behind it as (ghost + behind + 1) >> 1 per channel where it is nearer than the scene hit; writes neither depth nor segmentation
 *
 * THE MARCH of one ray, from the eye, t = 0.  At each sample: (ds, id) = minimum field over link shapes, spheres and object (ties to the lower id);
 * for t >= t_c the boundary field db.  ds < eps: hit id; else t >= t_c and db < eps: hit 22.  Otherwise t advances to t + relax min(ds, db) when
 * t >= t_c, and to min(t + relax ds, max(t_c, t + eps)) before.  A ray whose t then reaches its floor-plane crossing takes the floor there (id 21)
 * or ends as background outside the disc; a ray beyond t_max, or after max_steps samples, ends as background ("unresolved").
 *
 * IDS (segmentation):  0 background,  1 + 6 f + {0, 1, 2} upper / middle / distal shape of finger f,  1 + 6 f + {3, 4, 5} spheres sph2[0], sph2[1],
 * sph3[0],  20 object,  21 floor,  22 boundary.
 *
 * COLOUR (RGBA8, alpha 255).  Shading 0: palette[id] exactly.  Shading 1: palette[id] x (0.35 + 0.65 max(n . l, 0)), rounded to nearest, with
 * l = (0.35, 0.25, 0.9) / |.| and n: ids 1..20 the normalised central difference (h = 5e-4 m) of the scene field at the hit, floor (0, 0, 1),
 * boundary the inward surface normal (-c n_h, sin) of its segment (towards the point from the rim circle above wall_z[3]).
 *   palette (R, G, B):  background (24, 24, 28);  ghost (60, 220, 220);  object (235, 200, 40);  floor (120, 122, 126);  boundary (176, 150, 118);
 *   finger 0 red, finger 1 green, finger 2 blue - the six bodies of a finger in id order, with (a, b) = (main, other) channel values:
 *   upper (230, 60)  middle (200, 40)  distal (255, 100)  sph2[0] (170, 30)  sph2[1] (150, 20)  sph3[0] (130, 10);  id 19 is unused (0, 0, 0).
 *
 * CAMERA: z-up, right-handed, pinhole; forward f = (target - eye) / |.|, right r = f x z / |.|, up = r x f; the ray of pixel (col i, row j) is
 * f + x r + y up normalised, x = ((i + 0.5) / W 2 - 1) tan(fov_y / 2) W / H, y = (1 - (j + 0.5) / H 2) tan(fov_y / 2): pixel centres, square pixels,
 * row 0 at the top.  depth is the ray parameter t of the hit in metres (distance from the eye), +inf where nothing was hit.
 */
#ifndef TRIFINGER_RENDER_H
#define TRIFINGER_RENDER_H

#include <stdint.h>

#include "trifinger.h"

#ifdef __cplusplus
extern "C" {
#endif

#define TFR_API_VERSION 1
#define TFR_MAX_VIEWS 64          /* upper limit of TfrConfig.max_views: the checked env ids travel with the launch */
#define TFR_MAX_SIZE 4096         /* upper limit of width and height */

enum { TFR_ID_BACKGROUND = 0, TFR_ID_OBJECT = 20, TFR_ID_FLOOR = 21, TFR_ID_BOUNDARY = 22, TFR_NUM_IDS = 23 };
enum { TFR_SHADING_FLAT = 0, TFR_SHADING_LIT = 1 };

typedef struct TfrConfig {
    int32_t api_version;      /* TFR_API_VERSION */
    int32_t width, height;    /* pixels, 1..TFR_MAX_SIZE */
    int32_t max_views;        /* 1..TFR_MAX_VIEWS */
    int32_t max_steps;        /* samples per ray, 1..4096 (default 160) */
    int32_t shading;          /* TFR_SHADING_* (default TFR_SHADING_LIT) */
    float eps;                /* hit threshold, metres (default 1e-4) */
    float relax;              /* step = relax x field, (0, 1] (default 0.9: the shape field is not an exact distance - do not raise it) */
    float t_max;              /* metres (default 2) */
} TfrConfig;

typedef struct tfr_handle_s* tfr_handle;

int tfr_api_version(void);
const char* tfr_last_error_string(void);
void tfr_default_config(TfrConfig* cfg);      /* 256 x 256, 16 views, the march defaults above */

/* Host-side only: validates, derives the constants of the shapes and keeps them in the handle.  The default camera is
 * eye (0.55, 0.35, 0.50) -> target (0, 0, 0.10), fov_y 45 degrees. */
int tfr_create(const TfModel* model, const TfrConfig* cfg, tfr_handle* out);
int tfr_destroy(tfr_handle h);
int tfr_set_camera(tfr_handle h, const float eye[3], const float target[3], float fov_y_rad);
/* env_ids: HOST memory.  Every id is checked against [0, num_envs) and n_views against [1, max_views] (TF_ERR_INVALID_ARG) and copied into the
 * handle: the kernel never indexes the state with a value nobody checked.  Binds the renderer to state[TF_STATE_ROWS][num_envs]. */
int tfr_set_views(tfr_handle h, const int32_t* env_ids, int32_t n_views, int32_t num_envs);
/* state: DEVICE float [TF_STATE_ROWS][num_envs], read only.  color: DEVICE uint8 [V][H][W][4].  depth: DEVICE float [V][H][W] or NULL.
 * segmentation: DEVICE uint8 [V][H][W] or NULL.  One launch on `stream`; TF_ERR_NOT_BOUND before tfr_set_views. */
int tfr_render(tfr_handle h, const float* state, uint8_t* color, float* depth, uint8_t* segmentation, void* stream);
/* Leaf entry of the parity tests: the fields at n world points (DEVICE float [n][3]) of env `env` (checked against the num_envs of tfr_set_views):
 * dist / id the scene minimum and its id (1..20), boundary_dist the boundary field.  Any output may be NULL. */
int tfr_test_field(tfr_handle h, const float* state, int32_t env, const float* points, float* dist, uint8_t* id, float* boundary_dist,
                   int32_t n, void* stream);

#ifdef __cplusplus
}
#endif
#endif
