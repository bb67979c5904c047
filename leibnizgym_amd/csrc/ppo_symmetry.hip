// ppo_symmetry.hip - the augmenting gather of the in-repo PPO (`params.config.symmetry_augmentation`; include/trifinger_ppo_symmetry.h), gfx950.
//
// tfp_gather_rows_sym is tfp_gather_rows_norm (ppo_norm.hip) writing, per gathered row, the row and its two images under the robot's three-fold symmetry
// (leibnizgym_amd/symmetry.py: `apply` is the specification, bit for bit).  An image is a signed linear map with at most two source columns per output
// column, stated as a table entry {ia, ib, ca, cb}: out[j] = ca x[ia] + cb x[ib], both products and the sum rounded separately (this unit is built with
// -ffp-contract=off: a fused multiply-add would lose the bits of the statement), or ca x[ia] alone where cb == 0.
//
// Memory-bound: per source row one read and three writes.  The rows are narrow and odd (41, 113, 9, 1 floats), so a store instruction of a wavefront that
// owns ONE row covers 4 to 256 bytes; what the three images of consecutive output rows offer instead is that they are CONTIGUOUS per array and image.  A
// workgroup of four wavefronts therefore takes SYM_ROWS = 8 consecutive output rows per trip of a grid-stride loop:
//   1. every wavefront reads its two source rows - the indices, then the rows of EVERY array, lanes along the columns (rows are at most 128 columns: two
//      registers per lane, array and row; all loads in flight before the first use) - and stages them in LDS, one [cols] row of all arrays per source row;
//   2. per array the 8 x w floats of each image are one contiguous run of the output: the 256 threads walk it element by element - row = e / w (exact in
//      float for these sizes), column = e - row w -, read the staged value (image 0, and all three copies of an array without a table) or form the image
//      column from two LDS reads with the entry of the LDS table, normalise where statistics are given (after the transform: the bits of
//      tfp_gather_rows_norm on the transformed rows) and store: every store instruction covers 256 consecutive bytes.
// The tables are staged in LDS once per workgroup (16 bytes per image and column; the trainer's four tables are 5.5 KB).  Vector stores only; no atomics.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "../../include/trifinger_ppo_symmetry.h"

#define SYM_WAVES 4
#define SYM_WROWS 2                               // source rows per wavefront and trip
#define SYM_ROWS (SYM_WAVES * SYM_WROWS)          // consecutive output rows per workgroup and trip
#define SYM_MAX_BLOCKS 2048

struct GatherSymArgs {
    const float* src[8]; float* dst[8]; const float* mean[8]; const float* inv[8]; const int4* table[8];
    float clip[8]; float rinv[8];                     // rinv: 1 / width
    int width[8]; int off[8]; int toff[8];            // off: first column of the array in a staged row; toff: in the LDS tables (arrays with a table)
    int n, cols, tcols;                               // cols: columns of all arrays together; tcols: of those with a table
};

__device__ __forceinline__ float sym_norm(float x, const float* __restrict__ mean, const float* __restrict__ inv, int c, float hi) {
    if (!mean) return x;
    const float df = x - mean[c], y = df * inv[c];
    return y < -hi ? -hi : (y > hi ? hi : y);                               // a NaN passes through, as in torch.clamp
}

__global__ void __launch_bounds__(64 * SYM_WAVES) k_gather_rows_sym(const GatherSymArgs ga, const long long* __restrict__ idx, int rows) {
    extern __shared__ int4 smem[];                                          // tables [2][tcols] of 16 bytes, then the staged rows [SYM_ROWS][cols] floats
    int4* __restrict__ tab = smem;
    float* __restrict__ stage = reinterpret_cast<float*>(smem + 2 * ga.tcols);
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    for (int k = 0; k < ga.n; ++k) {
        const int4* __restrict__ t = ga.table[k];
        if (!t) continue;
        const int w = ga.width[k];
        for (int e = threadIdx.x; e < 2 * w; e += 64 * SYM_WAVES) tab[(e >= w ? ga.tcols + e - w : e) + ga.toff[k]] = t[e];
    }
    // the trip count is the same for every wavefront of the workgroup: the barriers below are reached by all of them (the first one also covers the tables)
    for (int r0 = blockIdx.x * SYM_ROWS; r0 < rows; r0 += gridDim.x * SYM_ROWS) {
        const int nr = min(SYM_ROWS, rows - r0);
        long long i[SYM_WROWS];
#pragma unroll
        for (int j = 0; j < SYM_WROWS; ++j) {
            const int rl = wave * SYM_WROWS + j;
            i[j] = rl < nr ? (idx ? idx[r0 + rl] : (long long)(r0 + rl)) : -1;
        }
        float x[SYM_WROWS][8][2];
#pragma unroll
        for (int j = 0; j < SYM_WROWS; ++j) {
#pragma unroll
            for (int k = 0; k < 8; ++k) {
                if (k < ga.n && i[j] >= 0) {
                    const int w = ga.width[k];
                    const float* __restrict__ s = ga.src[k] + (size_t)i[j] * w;
                    x[j][k][0] = lane < w ? s[lane] : 0.0f;
                    x[j][k][1] = lane + 64 < w ? s[lane + 64] : 0.0f;
                }
            }
        }
#pragma unroll
        for (int j = 0; j < SYM_WROWS; ++j) {
            float* __restrict__ st = stage + (wave * SYM_WROWS + j) * ga.cols;
#pragma unroll
            for (int k = 0; k < 8; ++k) {
                if (k < ga.n && i[j] >= 0) {
                    const int w = ga.width[k];
                    if (lane < w) st[ga.off[k] + lane] = x[j][k][0];
                    if (lane + 64 < w) st[ga.off[k] + lane + 64] = x[j][k][1];
                }
            }
        }
        __syncthreads();
#pragma unroll 1
        for (int k = 0; k < ga.n; ++k) {
            const int w = ga.width[k], off = ga.off[k], total = nr * w;
            const float rinv = ga.rinv[k];
            const float* __restrict__ mean = ga.mean[k];
            const float* __restrict__ inv = ga.inv[k];
            const float hi = ga.clip[k];
            const size_t image = (size_t)rows * w;
            float* __restrict__ d0 = ga.dst[k] + (size_t)r0 * w;            // the run of image 0; images 1 and 2 lie `image` and 2 `image` floats behind it
            const int4* __restrict__ t1 = ga.table[k] ? tab + ga.toff[k] : nullptr;
            for (int e = threadIdx.x; e < total; e += 64 * SYM_WAVES) {
                // e < 8 * 128 and w <= 128: (e + 0.5) / w lies at least 0.5 / 128 from an integer, the float product errs by less than 1e-4
                const int rl = (int)(((float)e + 0.5f) * rinv), c = e - rl * w;
                const float* __restrict__ st = stage + rl * ga.cols + off;
                const float y0 = sym_norm(st[c], mean, inv, c, hi);
                d0[e] = y0;
                if (!t1) { d0[image + e] = y0; d0[2 * image + e] = y0; continue; }
#pragma unroll
                for (int g = 0; g < 2; ++g) {
                    const int4 en = t1[g * ga.tcols + c];
                    const float ca = __int_as_float(en.z), cb = __int_as_float(en.w);
                    const float pa = ca * st[en.x];
                    const float pb = cb * st[en.y];
                    const float v = cb == 0.0f ? pa : pa + pb;
                    d0[(size_t)(g + 1) * image + e] = sym_norm(v, mean, inv, c, hi);
                }
            }
        }
        __syncthreads();                                                    // the staged rows are free for the next trip
    }
}

extern "C" {

int tfp_gather_rows_sym(const void* const* src, void* const* dst, const int32_t* widths, const void* const* mean_f, const void* const* inv_std_f,
                        const float* clip, const void* const* table, int32_t n, const void* idx, int32_t rows, void* stream) {
    if (!src || !dst || !widths || n <= 0 || n > 8 || rows <= 0) return -1;
    GatherSymArgs ga{};
    int cols = 0, tcols = 0;
    for (int k = 0; k < n; ++k) {
        if (!src[k] || !dst[k] || widths[k] <= 0) return -1;
        if (widths[k] > TFP_SYM_MAX_WIDTH) return -4;                       // a lane holds two columns of every array
        ga.src[k] = (const float*)src[k]; ga.dst[k] = (float*)dst[k]; ga.width[k] = widths[k]; ga.rinv[k] = 1.0f / (float)widths[k];
        ga.off[k] = cols;
        cols += widths[k];
        if (mean_f && mean_f[k]) {
            if (!inv_std_f || !inv_std_f[k] || !clip || !(clip[k] > 0.0f)) return -1;
            ga.mean[k] = (const float*)mean_f[k]; ga.inv[k] = (const float*)inv_std_f[k]; ga.clip[k] = clip[k];
        }
        if (table && table[k]) {
            if (((uintptr_t)table[k] & 15) != 0) return -1;                 // entries are read 16 bytes at a time
            ga.table[k] = (const int4*)table[k]; ga.toff[k] = tcols;
            tcols += widths[k];
        }
    }
    if (cols > TFP_SYM_MAX_COLS) return -4;                                 // 8 staged rows of 512 floats and two tables of 512 entries: 32 KB of LDS
    ga.n = n; ga.cols = cols; ga.tcols = tcols;
    const int groups = (rows + SYM_ROWS - 1) / SYM_ROWS;
    const size_t lds = (size_t)tcols * 2 * sizeof(int4) + (size_t)SYM_ROWS * cols * sizeof(float);
    hipLaunchKernelGGL(k_gather_rows_sym, dim3((unsigned)(groups < SYM_MAX_BLOCKS ? groups : SYM_MAX_BLOCKS)), dim3(64 * SYM_WAVES), lds, (hipStream_t)stream, ga,
                       (const long long*)idx, rows);
    return hipGetLastError() == hipSuccess ? 0 : -3;
}

}  // extern "C"
