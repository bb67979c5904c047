// tf_plan.hip - the planning library (include/trifinger_plan.h, libtrifinger_plan.so): the per-env fork of engine states across engines and the launches of
// sampling-based MPC (MPPI) around the env step.  One translation unit of its own, no object shared with the step library; the noise is the step's own
// Philox / Box-Muller chain under the step's arithmetic flags (Makefile: EVALFLAGS), so the torch statement of leibnizgym_amd/planning.py forms the same bits.
//
// k_fork            grid (256-env blocks, slots): a slot is a chunk of state rows, the per-env scalars, or a chunk of columns of a row-major buffer.  With
//                   src_index[i] = i / S (S a multiple of 64) the source address of a state row is wave-uniform and the store is one full line per
//                   wavefront; the row-major buffers are walked element-flat so consecutive lanes store consecutive floats.
// k_rollout_actions one lane per (planner env, block of four action components): one Philox call, two Box-Muller pairs, up to four stores; the lane of
//                   block 0 also closes the previous horizon step.
// k_update          one workgroup of S lanes per group: xor-butterfly sums inside a wavefront, partials through LDS, summed in wavefront order by every
//                   lane (so every lane holds the same bits without a broadcast).
// Every load and store is predicated on its row index; nothing is read through an index that was not range-checked.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdio.h>

#include "tf_device_math.h"
#include "../../include/trifinger_plan.h"

#define FORK_BLOCK 256
#define FORK_ROWS 8                       // state rows per slot
#define FORK_COLS 16                      // passes of 256 consecutive elements of a row-major buffer per slot
#define ACT_BLOCK 256
#define UPD_MAX_WAVES (TFPL_MAX_SAMPLES / 64)

// ---- fork ------------------------------------------------------------------------------------------------------------------------------------------------
struct ForkArgs {
    TfBuffers d, s;
    const int32_t* idx;
    uint32_t* bad;
    int nd, ns, A, SD;
    int slot_scalars, slot_action, slot_obs, slot_states;       // first slot of each part; the state chunks are slots [0, slot_scalars)
};

// passes [k0, k1) of the element-flat copy of a row-major buffer of width W: block bx owns the elements of envs [256 bx, 256 bx + 256)
DEV void fork_flat(float* dst, const float* src, const int32_t* idx, int nd, int ns, int W, int k0) {
    const size_t total = (size_t)nd * (size_t)W;
    const size_t base = (size_t)blockIdx.x * FORK_BLOCK * (size_t)W;
    const int k1 = k0 + FORK_COLS < W ? k0 + FORK_COLS : W;
    for (int k = k0; k < k1; ++k) {
        const size_t e = base + (size_t)k * FORK_BLOCK + threadIdx.x;
        if (e >= total) return;
        const int i = (int)(e / (size_t)W);
        const int c = (int)(e - (size_t)i * (size_t)W);
        const int s = idx[i];
        if ((unsigned)s < (unsigned)ns) dst[e] = src[(size_t)s * (size_t)W + c];
    }
}

__global__ __launch_bounds__(FORK_BLOCK) void k_fork(const ForkArgs a) {
    const int slot = blockIdx.y;
    if (slot >= a.slot_action) {
        if (slot < a.slot_obs) fork_flat(a.d.action_buf, a.s.action_buf, a.idx, a.nd, a.ns, a.A, (slot - a.slot_action) * FORK_COLS);
        else if (slot < a.slot_states) fork_flat(a.d.obs, a.s.obs, a.idx, a.nd, a.ns, TF_OBS_DIM_BASE + a.A, (slot - a.slot_obs) * FORK_COLS);
        else fork_flat(a.d.states, a.s.states, a.idx, a.nd, a.ns, a.SD, (slot - a.slot_states) * FORK_COLS);
        return;
    }
    const int i = blockIdx.x * FORK_BLOCK + threadIdx.x;
    if (i >= a.nd) return;
    const int s = a.idx[i];
    if ((unsigned)s >= (unsigned)a.ns) {
        if (slot == a.slot_scalars && a.bad) atomicAdd(a.bad, 1u);      // once per env: a vector atomic
        return;
    }
    if (slot < a.slot_scalars) {
        const int r0 = slot * FORK_ROWS;
        const int r1 = r0 + FORK_ROWS < TF_STATE_ROWS ? r0 + FORK_ROWS : TF_STATE_ROWS;
        const float* sp = a.s.state + (size_t)r0 * (size_t)a.ns + s;
        float* dp = a.d.state + (size_t)r0 * (size_t)a.nd + i;
        float v[FORK_ROWS];
#pragma unroll
        for (int r = 0; r < FORK_ROWS; ++r)
            if (r0 + r < r1) v[r] = sp[(size_t)r * (size_t)a.ns];
#pragma unroll
        for (int r = 0; r < FORK_ROWS; ++r)
            if (r0 + r < r1) dp[(size_t)r * (size_t)a.nd] = v[r];
        return;
    }
    a.d.reward[i] = a.s.reward[s];
    a.d.reset_buf[i] = a.s.reset_buf[s];
    a.d.goal_reset_buf[i] = a.s.goal_reset_buf[s];
    a.d.successes[i] = a.s.successes[s];
    a.d.dones[i] = a.s.dones[s];
    a.d.steps[i] = a.s.steps[s];
    a.d.reset_count[i] = a.s.reset_count[s];
}

// ---- the noise ---------------------------------------------------------------------------------------------------------------------------------------------
struct PlanArgs {
    int E, S, H, A, N;
    uint32_t k0, k1, counter;
    float sigma, lo, hi, lambda;
    int normalize, shift;
};

// the four normals of block q = a / 4 of (env i, horizon step h): include/trifinger_plan.h, THE NOISE
DEV void noise4(const PlanArgs& p, int i, int h, int q, float n[4]) {
    const uint32_t b = (uint32_t)q / 3u, k = (uint32_t)q % 3u;
    uint32_t r[4];
    philox4x32_10((uint32_t)i, p.counter, 4u * (uint32_t)h + k, b, p.k0, p.k1, r);
    box_muller(u01(r[0]), u01(r[1]), n[0], n[1]);
    box_muller(u01(r[2]), u01(r[3]), n[2], n[3]);
}

DEV float applied(const PlanArgs& p, float u, float eps) {
    const float t = p.sigma * eps;
    return f_min(f_max(u + t, p.lo), p.hi);
}

__global__ __launch_bounds__(ACT_BLOCK) void k_rollout_actions(const PlanArgs p, int h, const float* __restrict__ U, const float* __restrict__ disc,
                                                                const float* __restrict__ reward, const uint8_t* __restrict__ reset_buf,
                                                                float* __restrict__ G, uint8_t* __restrict__ alive, float* __restrict__ action) {
    const int i = blockIdx.x * ACT_BLOCK + threadIdx.x, q = blockIdx.y;
    if (i >= p.N) return;
    if (q == 0) {
        if (h == 0) {
            G[i] = 0.0f;
            alive[i] = 1;
        } else {
            uint8_t al = alive[i];
            if (al) {
                const float r = reward[i];
                const float t = disc[h - 1] * r;
                G[i] = G[i] + t;
                if (!isfinite(r)) al = 0;
            }
            if (reset_buf[i]) al = 0;
            alive[i] = al;
        }
    }
    if (h >= p.H) return;
    const int e = i / p.S, s = i - e * p.S;
    float n[4] = {0.0f, 0.0f, 0.0f, 0.0f};
    if (s != 0) noise4(p, i, h, q, n);
    const float* u = U + ((size_t)e * p.H + h) * p.A;
    float* out = action + (size_t)i * p.A;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const int a = 4 * q + j;
        if (a < p.A) out[a] = applied(p, u[a], n[j]);
    }
}

// ---- the update -------------------------------------------------------------------------------------------------------------------------------------------
DEV float wave_sum(float v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v = v + __shfl_xor(v, o, 64);
    return v;
}
DEV float wave_max(float v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v = f_max(v, __shfl_xor(v, o, 64));
    return v;
}

// the sum (or maximum) of v over the workgroup, the same bits in every lane; `part` holds one float per wavefront
template <bool MAX> DEV float block_reduce(float v, float* part, int nw) {
    v = MAX ? wave_max(v) : wave_sum(v);
    if ((threadIdx.x & 63) == 0) part[threadIdx.x >> 6] = v;
    __syncthreads();
    float r = part[0];
    for (int k = 1; k < nw; ++k) r = MAX ? f_max(r, part[k]) : r + part[k];
    __syncthreads();
    return r;
}

__global__ __launch_bounds__(TFPL_MAX_SAMPLES) void k_update(const PlanArgs p, const float* __restrict__ G, float* U, float* __restrict__ first,
                                                             float* __restrict__ w_out, float* __restrict__ stats, uint32_t* __restrict__ invalid_count) {
    __shared__ float part[UPD_MAX_WAVES];
    __shared__ float acc[UPD_MAX_WAVES][TFPL_MAX_ACTION_DIM];
    const int e = blockIdx.x, s = threadIdx.x, i = e * p.S + s, nw = p.S >> 6, wave = s >> 6, lane = s & 63;
    const float g = G[i];
    const bool valid = isfinite(g);
    const float nv = block_reduce<false>(valid ? 1.0f : 0.0f, part, nw);
    float* Ue = U + (size_t)e * p.H * p.A;
    if (nv == 0.0f) {                                                    // uniform: every lane holds the same count
        w_out[i] = 0.0f;
        if (s < p.A) first[(size_t)e * p.A + s] = Ue[s];
        if (s < TFPL_NUM_STATS) stats[(size_t)e * TFPL_NUM_STATS + s] = 0.0f;
        if (s == 0) invalid_count[e] = (uint32_t)p.S;
        return;
    }
    const float gmax = block_reduce<true>(valid ? g : -INFINITY, part, nw);
    const float mean = block_reduce<false>(valid ? g : 0.0f, part, nw) / nv;
    const float dev = valid ? g - mean : 0.0f;
    const float sd = f_sqrt(block_reduce<false>(dev * dev, part, nw) / nv);
    const float T = p.normalize ? p.lambda * f_max(sd, TFPL_STD_TINY) : p.lambda;
    const float ez = valid ? expf((g - gmax) / T) : 0.0f;
    const float w = ez / block_reduce<false>(ez, part, nw);              // the best sample contributes exp(0) = 1: the sum is >= 1
    const float w2 = block_reduce<false>(w * w, part, nw);
    w_out[i] = w;
    if (s == 0) {
        float* st = stats + (size_t)e * TFPL_NUM_STATS;
        st[TFPL_STAT_BEST] = gmax;
        st[TFPL_STAT_MEAN] = mean;
        st[TFPL_STAT_ESS] = 1.0f / w2;
        st[TFPL_STAT_STD] = sd;
        invalid_count[e] = (uint32_t)p.S - (uint32_t)nv;
    }
    const int Q = (p.A + 3) >> 2;
#pragma unroll 1
    for (int h = 0; h < p.H; ++h) {
        const float* u = Ue + (size_t)h * p.A;
#pragma unroll 1
        for (int q = 0; q < Q; ++q) {
            float n[4] = {0.0f, 0.0f, 0.0f, 0.0f};
            if (s != 0) noise4(p, i, h, q, n);
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const int a = 4 * q + j;
                const float v = wave_sum(a < p.A ? w * applied(p, u[a], n[j]) : 0.0f);
                if (lane == 0 && a < p.A) acc[wave][a] = v;
            }
        }
        __syncthreads();                                                 // every lane has read U[e][h]; the partials are in LDS
        if (s < p.A) {
            float r = acc[0][s];
            for (int k = 1; k < nw; ++k) r = r + acc[k][s];
            if (h == 0) first[(size_t)e * p.A + s] = r;
            if (!p.shift) Ue[(size_t)h * p.A + s] = r;
            else {
                if (h > 0) Ue[(size_t)(h - 1) * p.A + s] = r;            // U[e][h - 1] was read in the iteration before
                if (h == p.H - 1) Ue[(size_t)h * p.A + s] = r;           // the last entry is repeated
            }
        }
        __syncthreads();                                                 // the partials are free again
    }
}

// ------------------------------------------------------------------------------------------------------
// host
// ------------------------------------------------------------------------------------------------------
static thread_local char g_err[256] = "";
static int fail(int status, const char* what, const char* detail = "") {
    snprintf(g_err, sizeof(g_err), "%s%s", what, detail);
    return status;
}

static int launched(const char* what) {
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return fail(TFPL_ERR_LAUNCH, what, hipGetErrorString(e));
    return TFPL_OK;
}

static bool side_ok(const TfplSide* s) {
    if (!s || s->num_envs < 1 || s->num_envs > TF_MAX_ENVS || s->action_dim < 1 || s->action_dim > TFPL_MAX_ACTION_DIM || s->states_dim < 0) return false;
    const TfBuffers& b = s->buf;
    return b.state && b.action_buf && b.obs && (b.states || s->states_dim == 0) && b.reward && b.reset_buf && b.goal_reset_buf && b.successes && b.dones &&
           b.steps && b.reset_count;
}

static int plan_args(const TfplPlan* plan, const char* who, PlanArgs* out) {
    if (!plan) return fail(TFPL_ERR_INVALID_ARG, who, ": NULL plan");
    const TfplPlan& c = *plan;
    if (c.groups < 1 || c.samples < TFPL_MIN_SAMPLES || c.samples > TFPL_MAX_SAMPLES || c.samples % 64 != 0)
        return fail(TFPL_ERR_INVALID_ARG, who, ": groups >= 1, samples a multiple of 64 in [64, 1024]");
    if ((int64_t)c.groups * c.samples > TF_MAX_ENVS) return fail(TFPL_ERR_INVALID_ARG, who, ": groups * samples > TF_MAX_ENVS");
    if (c.horizon < 1 || c.horizon > TFPL_MAX_HORIZON) return fail(TFPL_ERR_INVALID_ARG, who, ": horizon outside [1, TFPL_MAX_HORIZON]");
    if (c.action_dim < 1 || c.action_dim > TFPL_MAX_ACTION_DIM) return fail(TFPL_ERR_INVALID_ARG, who, ": action_dim outside [1, TFPL_MAX_ACTION_DIM]");
    if (!(isfinite(c.sigma) && c.sigma >= 0.0f)) return fail(TFPL_ERR_INVALID_ARG, who, ": sigma must be finite and >= 0");
    if (!(isfinite(c.lo) && isfinite(c.hi) && c.lo <= c.hi)) return fail(TFPL_ERR_INVALID_ARG, who, ": lo <= hi, both finite");
    if (!(isfinite(c.lambda) && c.lambda > 0.0f)) return fail(TFPL_ERR_INVALID_ARG, who, ": lambda must be finite and > 0");
    PlanArgs p;
    p.E = c.groups; p.S = c.samples; p.H = c.horizon; p.A = c.action_dim; p.N = c.groups * c.samples;
    p.k0 = (uint32_t)(c.seed & 0xffffffffu); p.k1 = (uint32_t)(c.seed >> 32); p.counter = c.plan_counter;
    p.sigma = c.sigma; p.lo = c.lo; p.hi = c.hi; p.lambda = c.lambda;
    p.normalize = c.normalize != 0; p.shift = c.shift != 0;
    *out = p;
    return TFPL_OK;
}

extern "C" {

int tfpl_api_version(void) { return TFPL_API_VERSION; }
const char* tfpl_last_error_string(void) { return g_err; }

int tfpl_fork(const TfplSide* dst, const TfplSide* src, const int32_t* src_index, uint32_t* bad_count, void* stream) {
    if (!side_ok(dst) || !side_ok(src)) return fail(TFPL_ERR_INVALID_ARG, "tfpl_fork: a NULL side or buffer, or num_envs / action_dim / states_dim out of range");
    if (!src_index) return fail(TFPL_ERR_INVALID_ARG, "tfpl_fork: NULL src_index");
    if (dst->action_dim != src->action_dim || dst->states_dim != src->states_dim)
        return fail(TFPL_ERR_INVALID_ARG, "tfpl_fork: the two engines differ in action_dim or states_dim");
    ForkArgs a;
    a.d = dst->buf; a.s = src->buf; a.idx = src_index; a.bad = bad_count;
    a.nd = dst->num_envs; a.ns = src->num_envs; a.A = dst->action_dim; a.SD = dst->states_dim;
    const auto slots = [](int w) { return (w + FORK_COLS - 1) / FORK_COLS; };
    a.slot_scalars = (TF_STATE_ROWS + FORK_ROWS - 1) / FORK_ROWS;
    a.slot_action = a.slot_scalars + 1;
    a.slot_obs = a.slot_action + slots(a.A);
    a.slot_states = a.slot_obs + slots(TF_OBS_DIM_BASE + a.A);
    const int total = a.slot_states + slots(a.SD);
    hipLaunchKernelGGL(k_fork, dim3((unsigned)((a.nd + FORK_BLOCK - 1) / FORK_BLOCK), (unsigned)total), dim3(FORK_BLOCK), 0, (hipStream_t)stream, a);
    return launched("tfpl_fork: ");
}

int tfpl_rollout_actions(const TfplPlan* plan, int32_t h, const float* U, const float* disc, const float* reward, const uint8_t* reset_buf, float* G,
                         uint8_t* alive, float* action, void* stream) {
    PlanArgs p;
    const int rc = plan_args(plan, "tfpl_rollout_actions", &p);
    if (rc) return rc;
    if (h < 0 || h > p.H) return fail(TFPL_ERR_INVALID_ARG, "tfpl_rollout_actions: h outside [0, H]");
    if (!G || !alive) return fail(TFPL_ERR_INVALID_ARG, "tfpl_rollout_actions: NULL G or alive");
    if (h >= 1 && (!disc || !reward || !reset_buf)) return fail(TFPL_ERR_INVALID_ARG, "tfpl_rollout_actions: h >= 1 needs disc, reward and reset_buf");
    if (h < p.H && (!U || !action)) return fail(TFPL_ERR_INVALID_ARG, "tfpl_rollout_actions: h < H needs U and action");
    const unsigned Q = h < p.H ? (unsigned)((p.A + 3) / 4) : 1u;
    hipLaunchKernelGGL(k_rollout_actions, dim3((unsigned)((p.N + ACT_BLOCK - 1) / ACT_BLOCK), Q), dim3(ACT_BLOCK), 0, (hipStream_t)stream, p, (int)h, U, disc,
                       reward, reset_buf, G, alive, action);
    return launched("tfpl_rollout_actions: ");
}

int tfpl_update(const TfplPlan* plan, const float* G, float* U, float* first, float* w, float* stats, uint32_t* invalid_count, void* stream) {
    PlanArgs p;
    const int rc = plan_args(plan, "tfpl_update", &p);
    if (rc) return rc;
    if (!G || !U || !first || !w || !stats || !invalid_count) return fail(TFPL_ERR_INVALID_ARG, "tfpl_update: NULL argument");
    hipLaunchKernelGGL(k_update, dim3((unsigned)p.E), dim3((unsigned)p.S), 0, (hipStream_t)stream, p, G, U, first, w, stats, invalid_count);
    return launched("tfpl_update: ");
}

}  // extern "C"
