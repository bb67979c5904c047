// ppo_norm.hip - input normalisation of the in-repo PPO (`normalize_input` of the reference's resources/config/rlg/asymm.yaml), gfx950.
//
// A statistics RECORD of a D-wide input is {count, mean[D], M2[D]} in fp64 (M2 = sum of squared deviations, variance = M2 / count); what the networks
// read are its fp32 images mean_f = (float)mean and inv_std_f = (float)(1 / sqrt(M2 / count + 1e-5)), and the normalised input is
//     y = clamp((x - mean_f) * inv_std_f, -clip, clip)           (fp32, the difference and the product rounded separately: the torch expression, bit for bit)
// Three entry points live here (the fourth consumer, the forward network walk, stages its input through the same expression: ppo_mlp_walk.hip):
//
//   tfp_moments          batch moments of up to two row-major fp32 arrays [rows, D] = the rollout buffers of an epoch, one bandwidth-bound pass.
//                        A workgroup owns a SLAB of 256 consecutive rows; thread t < g D, g = 256 / D, owns column t % D of row group t / D, so that in
//                        every iteration the threads 0 .. g D - 1 read g D consecutive floats whatever D is (41 and 113 are odd: a thread-per-column
//                        layout would use 41 lanes of 256) and every thread keeps ONE column's sums in registers.  The sums are taken of d = x - c with
//                        c = the column's value in the first row of the slab (fp64, exact difference of two floats up to the 53 bits): s1 += d,
//                        s2 += d d, then mean = c + s1 / n, M2 = s2 - s1 s1 / n.  On data shifted by one of its own values the cancellation in that
//                        last difference is harmless: its rounding error is at most ~2 n eps (x - c)^2 summed, while the slab's true M2 is at least
//                        (x - c)^2 / 2 for the element farthest from c - a relative error of 4 n eps = 1e-13 for n = 256, for ANY data (a column at
//                        1e4 +- 1e-2 and a column with one outlier of 1e6 included; a constant column gives d = 0 and M2 = 0 exactly).
//                        A second small launch merges the slab partials per column with Chan's pairwise formula in a FIXED tree: every thread its run
//                        of consecutive slabs in slab order, then a binary tree over the threads.  No atomics anywhere: the same input gives the same bits.
//   tfp_norm_merge       merges k >= 1 batch records, in the order given, into the running record of up to two inputs and publishes mean_f / inv_std_f.
//   tfp_gather_rows_norm tfp_gather_rows with an optional (mean_f, inv_std_f, clip) per array and an optional index (NULL: identity = a plain normaliser).
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "../../include/trifinger_ppo.h"
#include "../../include/trifinger_ppo_norm.h"

#define MOM_SLAB 256          // rows per slab (and per workgroup)
#define MOM_UNROLL 8          // loads in flight per thread

struct MomArgs { const float* x[2]; int D[2]; int first[2]; int base[2]; int n, rows, Dtot, slabs; };   // first: first column in the concatenation; base: offset of the record in `out`

// Chan's pairwise merge of (na, ma, Ma) <- (nb, mb, Mb); an empty side leaves the other one untouched, bit for bit
__device__ __forceinline__ void chan_merge(double& na, double& ma, double& Ma, double nb, double mb, double Mb) {
#pragma clang fp contract(off)
    if (nb <= 0.0) return;
    if (na <= 0.0) { na = nb; ma = mb; Ma = Mb; return; }
    const double n = na + nb, delta = mb - ma;
    const double w = nb / n, dm = delta * w;
    const double dd = delta * delta, f = na * nb / n, t = dd * f;
    ma = ma + dm;
    Ma = (Ma + Mb) + t;
    na = n;
}

__global__ void __launch_bounds__(256) k_moments_slab(const MomArgs a, double* __restrict__ part) {
    __shared__ double s1s[256], s2s[256];
    const int k = blockIdx.y, D = a.D[k], g = 256 / D;
    const int row0 = (int)blockIdx.x * MOM_SLAB, ns = min(MOM_SLAB, a.rows - row0);
    const int t = threadIdx.x, rg = t / D, col = t - rg * D;
    const float* __restrict__ p = a.x[k] + (size_t)row0 * D + col;          // col < D also for the idle threads (rg == g): p[0] stays inside the slab
    const double c = (double)p[0];
    double s1 = 0.0, s2 = 0.0;
    if (rg < g) {
        const size_t st = (size_t)g * D;
        int r = rg;
        for (; r + (MOM_UNROLL - 1) * g < ns; r += MOM_UNROLL * g) {
            float v[MOM_UNROLL];
#pragma unroll
            for (int u = 0; u < MOM_UNROLL; ++u) v[u] = p[(size_t)r * D + u * st];
#pragma unroll
            for (int u = 0; u < MOM_UNROLL; ++u) { const double d = (double)v[u] - c; s1 += d; s2 = fma(d, d, s2); }
        }
        for (; r < ns; r += g) { const double d = (double)p[(size_t)r * D] - c; s1 += d; s2 = fma(d, d, s2); }
    }
    s1s[t] = s1; s2s[t] = s2;
    __syncthreads();
    if (t < D) {                                                             // the row groups share the shift c: their sums add, in group order
        double S1 = 0.0, S2 = 0.0;
        for (int q = 0; q < g; ++q) { S1 += s1s[q * D + t]; S2 += s2s[q * D + t]; }
        const double n = (double)ns;
        double M2 = S2 - S1 * S1 / n;
        if (M2 < 0.0) M2 = 0.0;
        double* o = part + ((size_t)blockIdx.x * a.Dtot + a.first[k] + t) * 2;
        o[0] = c + S1 / n;
        o[1] = M2;
    }
}

// one workgroup per column of the concatenation: thread t merges the slabs [t per, (t + 1) per) in order, then a binary tree over the threads (left = earlier slabs)
__global__ void __launch_bounds__(256) k_moments_merge(const MomArgs a, const double* __restrict__ part, double* __restrict__ out) {
    __shared__ double sn[256], sm[256], sM[256];
    const int cg = blockIdx.x, k = (a.n > 1 && cg >= a.first[1]) ? 1 : 0, c = cg - a.first[k], D = a.D[k];
    const int t = threadIdx.x, per = (a.slabs + 255) / 256;
    double n = 0.0, m = 0.0, M = 0.0;
    for (int s = t * per; s < min((t + 1) * per, a.slabs); ++s) {
        const double* q = part + ((size_t)s * a.Dtot + cg) * 2;
        chan_merge(n, m, M, (double)min(MOM_SLAB, a.rows - s * MOM_SLAB), q[0], q[1]);
    }
    sn[t] = n; sm[t] = m; sM[t] = M;
    __syncthreads();
    for (int st = 1; st < 256; st <<= 1) {
        if ((t & (2 * st - 1)) == 0) {
            chan_merge(n, m, M, sn[t + st], sm[t + st], sM[t + st]);
            sn[t] = n; sm[t] = m; sM[t] = M;
        }
        __syncthreads();
    }
    if (t == 0) {
        double* o = out + a.base[k];
        if (c == 0) o[0] = n;
        o[1 + c] = m;
        o[1 + D + c] = M;
    }
}

struct MergeArgs { double* run[2]; const double* batch[2]; float* mean_f[2]; float* inv_f[2]; int D[2]; int k, stride; };
// one workgroup per record: the count is read by every thread before the barrier and written by thread 0 behind it
__global__ void __launch_bounds__(256) k_norm_merge(const MergeArgs a) {
    const int q = blockIdx.x, D = a.D[q];
    double* run = a.run[q];
    const double n0 = run[0];
    double nn = n0;
    for (int c0 = 0; c0 < D; c0 += 256) {
        const int c = c0 + (int)threadIdx.x;
        if (c < D) {
            double n = n0, m = run[1 + c], M = run[1 + D + c];
            for (int j = 0; j < a.k; ++j) {
                const double* b = a.batch[q] + (size_t)j * a.stride;
                chan_merge(n, m, M, b[0], b[1 + c], b[1 + D + c]);
            }
            run[1 + c] = m; run[1 + D + c] = M;
            a.mean_f[q][c] = (float)m;
            a.inv_f[q][c] = n > 0.0 ? (float)(1.0 / sqrt(M / n + 1e-5)) : (float)(1.0 / sqrt(1.0 + 1e-5));      // count 0: variance 1
            nn = n;
        }
    }
    __syncthreads();
    if (threadIdx.x == 0) run[0] = nn;                                       // D >= 1: thread 0 always owns a column
}

struct GatherNormArgs { const float* src[8]; float* dst[8]; const float* mean[8]; const float* inv[8]; float clip[8]; int width[8]; int n; };
// one wavefront per row, as k_gather_rows (ppo_kernels.hip); an array with statistics leaves normalised
__global__ void __launch_bounds__(256) k_gather_rows_norm(const GatherNormArgs ga, const long long* __restrict__ idx, int rows) {
#pragma clang fp contract(off)
    const int r = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (r >= rows) return;
    const long long i = idx ? idx[r] : (long long)r;
#pragma unroll 1
    for (int k = 0; k < ga.n; ++k) {
        const int w = ga.width[k];
        const float* __restrict__ s = ga.src[k] + (size_t)i * w;
        float* __restrict__ d = ga.dst[k] + (size_t)r * w;
        const float* __restrict__ mean = ga.mean[k];
        if (!mean) {
            for (int c = lane; c < w; c += 64) d[c] = s[c];
        } else {
            const float* __restrict__ inv = ga.inv[k];
            const float hi = ga.clip[k], lo = -hi;
            for (int c = lane; c < w; c += 64) {
                const float df = s[c] - mean[c], y = df * inv[c];
                d[c] = y < lo ? lo : (y > hi ? hi : y);                      // a NaN passes through, as in torch.clamp
            }
        }
    }
}

extern "C" {

// doubles of scratch tfp_moments needs for these shapes (0: invalid)
int64_t tfp_moments_part_doubles(const int32_t* D, int32_t n, int32_t rows) {
    if (!D || n < 1 || n > 2 || rows <= 0) return 0;
    int64_t dt = 0;
    for (int k = 0; k < n; ++k) { if (D[k] <= 0) return 0; dt += D[k]; }
    return 2 * dt * (int64_t)((rows + MOM_SLAB - 1) / MOM_SLAB);
}

int tfp_moments(const void* const* x, const int32_t* D, int32_t n, int32_t rows, void* part, int64_t part_doubles, void* out, void* stream) {
    if (!x || !D || !part || !out || n < 1 || n > 2 || rows <= 0) return -1;
    MomArgs a{};
    int dt = 0, base = 0;
    for (int k = 0; k < n; ++k) {
        if (!x[k] || D[k] <= 0) return -1;
        if (D[k] > 256) return -4;                                           // a row wider than a workgroup: the caller computes the moments itself
        a.x[k] = (const float*)x[k]; a.D[k] = D[k]; a.first[k] = dt; a.base[k] = base;
        dt += D[k]; base += 1 + 2 * D[k];
    }
    a.n = n; a.rows = rows; a.Dtot = dt; a.slabs = (rows + MOM_SLAB - 1) / MOM_SLAB;
    if (part_doubles < 2 * (int64_t)dt * a.slabs) return -1;
    hipStream_t s = (hipStream_t)stream;
    hipLaunchKernelGGL(k_moments_slab, dim3((unsigned)a.slabs, (unsigned)n), dim3(256), 0, s, a, (double*)part);
    if (hipGetLastError() != hipSuccess) return -3;
    hipLaunchKernelGGL(k_moments_merge, dim3((unsigned)dt), dim3(256), 0, s, a, (const double*)part, (double*)out);
    return hipGetLastError() == hipSuccess ? 0 : -3;
}

int tfp_norm_merge(void* const* run, const void* const* batch, const int32_t* D, int32_t n, int32_t k, int32_t stride, void* const* mean_f,
                   void* const* inv_std_f, void* stream) {
    if (!run || !batch || !D || !mean_f || !inv_std_f || n < 1 || n > 2 || k < 1) return -1;
    MergeArgs a{};
    for (int q = 0; q < n; ++q) {
        if (!run[q] || !batch[q] || !mean_f[q] || !inv_std_f[q] || D[q] <= 0 || stride < 1 + 2 * D[q]) return -1;
        a.run[q] = (double*)run[q]; a.batch[q] = (const double*)batch[q]; a.mean_f[q] = (float*)mean_f[q]; a.inv_f[q] = (float*)inv_std_f[q]; a.D[q] = D[q];
    }
    a.k = k; a.stride = stride;
    hipLaunchKernelGGL(k_norm_merge, dim3((unsigned)n), dim3(256), 0, (hipStream_t)stream, a);
    return hipGetLastError() == hipSuccess ? 0 : -3;
}

int tfp_gather_rows_norm(const void* const* src, void* const* dst, const int32_t* widths, const void* const* mean_f, const void* const* inv_std_f,
                         const float* clip, int32_t n, const void* idx, int32_t rows, void* stream) {
    if (!src || !dst || !widths || n <= 0 || n > 8 || rows <= 0) return -1;
    GatherNormArgs ga{};
    for (int k = 0; k < n; ++k) {
        if (!src[k] || !dst[k] || widths[k] <= 0) return -1;
        ga.src[k] = (const float*)src[k]; ga.dst[k] = (float*)dst[k]; ga.width[k] = widths[k];
        if (mean_f && mean_f[k]) {
            if (!inv_std_f || !inv_std_f[k] || !clip || !(clip[k] > 0.0f)) return -1;
            ga.mean[k] = (const float*)mean_f[k]; ga.inv[k] = (const float*)inv_std_f[k]; ga.clip[k] = clip[k];
        }
    }
    ga.n = n;
    hipLaunchKernelGGL(k_gather_rows_norm, dim3((unsigned)((rows + 3) / 4)), dim3(256), 0, (hipStream_t)stream, ga, (const long long*)idx, rows);
    return hipGetLastError() == hipSuccess ? 0 : -3;
}

}  // extern "C"
