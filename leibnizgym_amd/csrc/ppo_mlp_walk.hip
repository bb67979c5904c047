// ppo_mlp_walk.hip - the trainer's two MLPs as ONE launch per direction ("network walk"), gfx950, fp32 MFMA.
//
// The per-layer products of ppo_kernels.hip (k_gemm / k_gemm_group) pay, for every layer, a launch, a cold first tile, a tail, a round trip of
// the activations through memory, and 64-wide tiles that pad N = 200 to 256 and N = 100 to 128.  Here a workgroup owns 32 ROWS of the minibatch
// and walks ALL layers of one network with them:
//
//   forward   x [32, D0] -> LDS;  y1 = elu(x W1^T + b1) -> LDS (+ memory);  y2 = elu(y1 W2^T + b2) -> LDS (+ memory);  ...;  y4 -> memory
//   backward  g [32, D4] -> LDS;  dZ3 = (g W4) * elu'(y3) -> LDS + memory;  dZ2 = (dZ3 W3) * elu'(y2) -> LDS + memory;  dZ1 = (dZ2 W2) * elu'(y1) -> memory
//
// (the weight gradients dW_l = dZ_l^T y_{l-1} stay a split-K product over the whole minibatch: tfp_gemm_tn_partials_group).  M = 8192 rows and two
// networks are 512 workgroups = two per CU, one round; the activations of a row block never leave the CU (two LDS buffers used alternately: 27 + 52 KB
// for 41/113 -> 400 -> 200 -> 100 -> 9/1, so two workgroups share a CU's 160 KB), the weights stream from L2 (1 MB for both networks).
// Two INDEPENDENT workgroups per CU = two wavefronts per SIMD that are not tied by each other's barriers: the epilogue, the barrier waits and the memory
// latencies of one run in the shadow of the other's MFMAs (a first form with 64 rows and one wavefront per SIMD spent half its time in exactly those:
// docs/HISTORY.md section 12).
//
// Inside a layer the four wavefronts of a workgroup split the [32, N] output by columns: a wavefront owns all 32 rows (two 16-row tiles) and a quarter
// of the 16-column tiles (N = 400: 7 / 6 / 6 / 6 tiles, 200: 4 / 3 / 3 / 3, 100: 2 / 2 / 2 / 1), i.e. up to 14 accumulators of v_mfma_f32_16x16x4_f32.
// A wavefront's weights need no LDS: the B fragment of a 16 x 16 tile is loaded from memory straight in MFMA layout -
//   forward  (W [N, K], k contiguous): lane (n = l % 16, kk = l / 16) reads W[n][k0 + 4 kk .. + 3] with one dwordx4 load and feeds the four values
//            to four MFMAs; the A fragment is the same shape out of LDS (one ds_read_b128), so MFMA s of a 16-k step sums k0 + 4 kk + s, kk = 0..3:
//            the order of the k inside a step is free as long as both operands use the same one;
//   backward (W [K, N], n contiguous): the same lane reads W[k0 + 4 kk + s][n], s = 0..3, with four dword loads (a wave instruction = 4 rows x 64 B).
// A step visits the column tiles in turn: the 8 MFMAs of tile j (4 k-groups x 2 row tiles), then the load of tile j's fragment for the NEXT step into
// the registers those MFMAs have just released.  LDS rows have a pitch of 16 q + 4 floats: conflict-free for the b128 fragment reads (16 rows x 4
// k-groups) and for the epilogue's column writes.
//
// The epilogue of a layer adds the bias, applies ELU (forward) or multiplies by elu'(y) = y > 0 ? 1 : y + 1 of the saved output (backward) and writes
// the tile to LDS as the next layer's A operand (zero in the padding columns).  Hidden outputs reach memory FROM LDS, as dwordx4 rows, one chunk per
// thread and K step of the NEXT layer (the buffer is that layer's A operand and stays intact throughout): 46 MB of stores per forward pass are spread
// over the whole launch instead of arriving in bursts at the layer boundaries.  ELU is x > 0 ? x : exp(x) - 1 with exp on v_exp_f32 (the form torch's
// kernel uses: exp - 1, not expm1; absolute error <= 1.2e-7).
//
// The extended walk (EXT; include/trifinger_ppo_net.h: tfp_net_forward / tfp_net_backward) is a compile-time variant of the same kernel, added the way
// NORM was - the plain kernels keep their code and their argument block.  It knows the activation codes 0 .. 6 (the epilogue branches once per layer on
// the wave-uniform code; backward: the derivative from the saved output) and d2rl: the operand of a hidden layer l >= 1 is [h | x], K = dim[l] + dim[0] -
// the epilogue writes h as ever, the workgroup copies the row block's x columns behind it from the operand of the running layer, and the saved outputs go to
// memory as these wide rows (the weight gradients stay plain products on them; rows of 441 / 513 floats miss StreamOut's dwordx4 path and leave at the layer
// boundary).  The backward chain reads W with that leading dimension and N = dim[l], and the saved output with a row stride of its own.  The forward operands
// of a d2rl walk are 110 KB at the trainer's shapes: that call may take the whole CU's LDS, one workgroup per CU.
//
// bf16 operands (BF; include/trifinger_ppo_mixed.h: tfp_net_forward_bf16 / tfp_net_backward_bf16, `mixed_precision`) is one more compile-time variant of the
// extended walk: walk_layer_bf16 below stands where walk_layer stands, everything else - staging, statistics, d2rl (not declined: LDS stays fp32, so the
// budget is the fp32 form's), epilogues, StreamOut - is the same code.  The fp32 kernels keep their code and their argument blocks.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <string.h>
#include "../../include/trifinger_ppo.h"
#include "../../include/trifinger_ppo_norm.h"
#include "../../include/trifinger_ppo_net.h"
#include "../../include/trifinger_ppo_mixed.h"

typedef float w4 __attribute__((ext_vector_type(4)));
typedef float w4u __attribute__((ext_vector_type(4), aligned(4)));      // a dwordx4 load needs dword alignment only (rows of 41 / 113 floats)

#ifndef WALK_DBG
#define WALK_DBG 0     // developer builds (timing only, wrong results): 1 = the B loads do not advance along K (every step re-reads the first one: L1 hits),
#endif                 // 2 = no MFMAs (loads, LDS traffic and epilogues only)
#ifdef WALK_TIMING     // developer build: s_memtime stamps of one workgroup (per wavefront: start, input staged, then per layer: K loop done, epilogue done, barrier passed)
__device__ unsigned long long g_walk_t[4 * 32];
#ifndef WALK_TIMING_WG
#define WALK_TIMING_WG 0
#endif
#define WSTAMP(i_) do { if (blockIdx.x == WALK_TIMING_WG && (threadIdx.x & 63) == 0) g_walk_t[(threadIdx.x >> 6) * 32 + (i_)] = __builtin_readcyclecounter(); } while (0)
#else
#define WSTAMP(i_)
#endif
#define WALK_ROWS 32
#define WALK_MAXL 4

struct WalkNet {
    const float* x;                    // forward: network input [M, dim[0]]; backward: gradient of the network output [M, dim[nl]]
    const float* W[WALK_MAXL];         // W[l]: [dim[l + 1], dim[l]] row-major (torch.nn.Linear.weight)
    const float* b[WALK_MAXL];         // forward: bias [dim[l + 1]]
    const float* yin[WALK_MAXL];       // backward: yin[l] = saved output of layer l, [M, dim[l + 1]]
    float* y[WALK_MAXL];               // forward: output of layer l (NULL: not stored; the last one must be given); backward: y[l] = dZ of layer l (l < nl - 1)
    int dim[WALK_MAXL + 1];
    int act[WALK_MAXL];                // 1: ELU behind layer l
    int nl;
};
struct WalkArgs { WalkNet net[2]; int n_nets, M, blocks_per_net, p_floats; };

__device__ __forceinline__ int pitch_of(int d) { return ((d + 15) & ~15) + 4; }

__device__ __forceinline__ float elu_fast(float v) {
    // exp(v) - 1 for v <= 0 through v_exp_f32 (2^x): |error| <= 1.2e-7 absolute
    const float e = __builtin_amdgcn_exp2f(v * 1.44269504088896340736f) - 1.0f;
    return v > 0.0f ? v : e;
}

// The other activations of include/trifinger_ppo_net.h (the extended walk only: EXT).  CODE is a template argument: the epilogue branches ONCE per layer on
// the wave-uniform code and runs a loop compiled for it.  exp / log through v_exp_f32 / v_log_f32 (2^x, log2), the quotients through v_rcp_f32 (1 ulp).
#define WALK_SELU_L 1.0507009873554805f
#define WALK_SELU_LA (1.0507009873554805f * 1.6732632423543772f)
__device__ __forceinline__ float exp_fast(float v) { return __builtin_amdgcn_exp2f(v * 1.44269504088896340736f); }
// tanh, intended to stay within a few ulp (the formula with exact exp and quotient: 2.5e-7 relative, tests/test_net_shape.py): 1 - 2 / (exp(2 |v|) + 1) with the sign of v from |v| = 0.625 on (exp = inf gives exactly 1, no NaN); below that the difference cancels
// (an absolute 1e-7 on a result near 0 - which Adam, scale-free, turns into visibly different steps), so the odd polynomial v + v^3 P(v^2) of Cephes' tanhf
__device__ __forceinline__ float tanh_fast(float v) {
    const float a = __builtin_fabsf(v), z = v * v;
    const float big = __builtin_copysignf(1.0f - 2.0f * __builtin_amdgcn_rcpf(exp_fast(2.0f * a) + 1.0f), v);
    const float p = ((((-5.70498872745e-3f * z + 2.06390887954e-2f) * z - 5.37397155531e-2f) * z + 1.33314422036e-1f) * z - 3.33332819422e-1f) * z * v + v;
    return a < 0.625f ? p : big;
}
template <int CODE>
__device__ __forceinline__ float act_fwd(float v) {
    if (CODE == TFP_ACT_ELU) return elu_fast(v);
    if (CODE == TFP_ACT_RELU) return v > 0.0f ? v : 0.0f;
    if (CODE == TFP_ACT_TANH) return tanh_fast(v);
    if (CODE == TFP_ACT_SIGMOID) return __builtin_amdgcn_rcpf(1.0f + exp_fast(-v));                               // exp = inf: 0
    if (CODE == TFP_ACT_SELU) return v > 0.0f ? WALK_SELU_L * v : WALK_SELU_LA * (exp_fast(v) - 1.0f);
    if (CODE == TFP_ACT_SOFTPLUS) return v > 20.0f ? v : 0.69314718055994530942f * __builtin_amdgcn_logf(1.0f + exp_fast(v));
    return v;
}
// the derivative from the saved OUTPUT y of the layer
template <int CODE>
__device__ __forceinline__ float act_der(float y) {
    if (CODE == TFP_ACT_ELU) return y > 0.0f ? 1.0f : y + 1.0f;
    if (CODE == TFP_ACT_RELU) return y > 0.0f ? 1.0f : 0.0f;
    if (CODE == TFP_ACT_TANH) return 1.0f - y * y;
    if (CODE == TFP_ACT_SIGMOID) return y * (1.0f - y);
    if (CODE == TFP_ACT_SELU) return y > 0.0f ? WALK_SELU_L : y + WALK_SELU_LA;
    if (CODE == TFP_ACT_SOFTPLUS) return 1.0f - exp_fast(-y);
    return 1.0f;
}
template <int CODE, bool BWD, int NCT>
__device__ __forceinline__ void act_tiles(w4 (&acc)[2][NCT], const float (&bv)[NCT], const w4 (&e)[2][BWD ? NCT : 1]) {
#pragma unroll
    for (int j = 0; j < NCT; ++j) {
#pragma unroll
        for (int i = 0; i < 2; ++i) {
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                if (BWD) acc[i][j][r] *= act_der<CODE>(e[i][BWD ? j : 0][r]);
                else acc[i][j][r] = act_fwd<CODE>(acc[i][j][r] + bv[j]);
            }
        }
    }
}

typedef unsigned u4 __attribute__((ext_vector_type(4)));
typedef __attribute__((address_space(1))) float gfloat;           // a pointer the compiler must treat as global memory (a flat access counts in vmcnt AND lgkmcnt)
// Buffer addressing (raw buffer, stride 0): a load takes the matrix as a 128-bit resource in scalar registers, a 32-bit per-lane byte offset and a scalar
// byte offset - the K position of the step - so the K loop holds no address arithmetic at all; what lies past the end of the matrix reads as zero and
// stores past the end are dropped (the range check of the hardware), which is what the ragged edges need.
__device__ __forceinline__ __amdgpu_buffer_rsrc_t make_rsrc(const void* p, unsigned bytes) {
    return __builtin_amdgcn_make_buffer_rsrc(const_cast<void*>(p), 0, (int)bytes, 0x00020000);
}
__device__ __forceinline__ w4 buf_load4(__amdgpu_buffer_rsrc_t r, unsigned voff, unsigned soff) {
    return __builtin_bit_cast(w4, __builtin_amdgcn_raw_buffer_load_b128(r, (int)voff, (int)soff, 0));
}
__device__ __forceinline__ float buf_load1(__amdgpu_buffer_rsrc_t r, unsigned voff, unsigned soff) {
    return __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(r, (int)voff, (int)soff, 0));
}

// What the step before left in the LDS operand of this one (a hidden output / dZ, [32][pitch], width W, W % 4 == 0) on its way to memory [M, W]: every
// thread owns the 16-byte chunks tid, tid + 256, ... of the row block (memory is linear in the chunk index) and moves ONE of them per K step of the
// running layer - read from LDS at the top of the step, stored at its end, no branch: a thread that has run out of chunks stores out of range.
struct StreamOut {
    u4 dst;                            // buffer resource of the row block in memory (base, 0, bytes, format word)
    const float* src;                  // the LDS operand
    int pitch, cpr, total, dr, dc;     // chunks per row, chunks of the block, the (row, chunk-in-row) advance of 256 chunks
    int idx, row, c4;
    unsigned woff;
    __device__ __forceinline__ void init(float* G, const float* Xs, int pitch_, int W, int row0, int M) {
        const int rows = min(WALK_ROWS, M - row0);
        const uintptr_t base = (uintptr_t)(G + (size_t)row0 * W);
        dst = u4{(unsigned)base, (unsigned)(base >> 32) & 0xffffu, (unsigned)(rows * W) * 4u, 0x00020000u};
        src = Xs; pitch = pitch_;
        cpr = W >> 2;
        total = rows * cpr;
        dr = 256 / cpr; dc = 256 - dr * cpr;
        row = (int)threadIdx.x / cpr; c4 = (int)threadIdx.x - row * cpr;
        idx = threadIdx.x;
    }
    __device__ __forceinline__ w4 read() {
        const bool ok = idx < total;
        woff = ok ? (unsigned)idx * 16u : (unsigned)total * 16u;      // = num_records: just past the end (a huge offset could wrap in the range check)
        return *(const w4*)(src + (ok ? row : 0) * pitch + 4 * (ok ? c4 : 0));
    }
    __device__ __forceinline__ void write(const w4& v) {
        // The store is written as inline assembly ON PURPOSE: on gfx9 loads and stores share vmcnt, and with a store pending the compiler's wait-count
        // pass treats the counter as out of order - every wait for a B fragment in the K loop becomes vmcnt(0), i.e. the wavefront sits out the latency of
        // the load it issued last, in every step.  Hidden from that pass the store only makes the hardware counter larger than the compiler's model, so
        // its waits stay safe (loads return in order among themselves), and the data registers are read in issue order (no expcnt on gfx9).
        const u4 rs = u4{(unsigned)__builtin_amdgcn_readfirstlane((int)dst[0]), (unsigned)__builtin_amdgcn_readfirstlane((int)dst[1]),
                         (unsigned)__builtin_amdgcn_readfirstlane((int)dst[2]), (unsigned)__builtin_amdgcn_readfirstlane((int)dst[3])};
        // (s_nop 4: a vector instruction that writes a scalar register - the v_readfirstlane above - needs 5 wait states before a memory instruction reads
        // that register; the compiler inserts them for its own instructions, not in front of an asm: without them the store ran with a stale descriptor)
        asm volatile("s_nop 4\n\tbuffer_store_dwordx4 %0, %1, %2, 0 offen" : : "v"(v), "v"(woff), "s"(rs) : "memory");
        idx += 256; c4 += dc; row += dr;
        if (c4 >= cpr) { c4 -= cpr; row += 1; }
    }
    // what is left when the K loop is over (or for a wavefront without tiles in this layer): ordinary stores, the compiler's own
    __device__ __forceinline__ void flush() {
        const unsigned d0 = (unsigned)__builtin_amdgcn_readfirstlane((int)dst[0]), d1 = (unsigned)__builtin_amdgcn_readfirstlane((int)dst[1]);
        const __amdgpu_buffer_rsrc_t rd = __builtin_amdgcn_make_buffer_rsrc((void*)(((uintptr_t)d0) | ((uintptr_t)(d1 & 0xffffu) << 32)), 0,
                                                                             __builtin_amdgcn_readfirstlane((int)dst[2]), 0x00020000);
        while (__builtin_amdgcn_ballot_w64(idx < total) != 0ull) {
            const w4 v = read();
            __builtin_amdgcn_raw_buffer_store_b128(__builtin_bit_cast(u4, v), rd, (int)woff, 0, 0);
            idx += 256; c4 += dc; row += dr;
            if (c4 >= cpr) { c4 -= cpr; row += 1; }
        }
    }
};

// after the last MFMA of a layer, before anything but an MFMA touches the accumulators.  The compiler inserts the wait states an 8-pass MFMA needs before a
// vector instruction reads its result; the explicit ones and the empty asm ties date from the inline-assembly form of the loop and are kept because they
// keep the epilogue's reads behind the whole K loop (64 cycles per layer, under 0.5% of the walk) - the shape the parity tests and profiles were taken on.
template <int NCT>
__device__ __forceinline__ void walk_mfma_drain(w4 (&acc)[2][NCT]) {
    asm volatile("s_nop 15\n\ts_nop 15" ::: "memory");
    // every accumulator passes through an (empty) volatile asm behind the wait states: a vector instruction that reads one cannot be scheduled above them
#pragma unroll
    for (int i = 0; i < 2; ++i) {
#pragma unroll
        for (int j = 0; j < NCT; ++j) asm volatile("" : "+v"(acc[i][j]));
    }
}

// One layer for this wavefront: acc[i][j] += X[16 i .., :] . op(W)[:, 16 (ct0 + j) ..] over K, NCT column tiles (exact: no guards inside).
//   Xs: LDS [32][px], columns K .. ceil16(K) are zero.  KMAJ = false: W[n * ldw + k] (forward); true: W[k * ldw + n] (backward).  SO: a stream-out
//   rides along (one chunk per step).
// K = 16 nfull + tail.  Every step is the same code: a fragment that reaches past the end of the matrix reads zeros, one that reaches past the end of a
// row (forward) reads the next row's finite values against A values that are zero.  Only a forward K that is no multiple of 4 (the first layer: 41, 113)
// has a dwordx4 fragment straddling the end of the LAST row with values that count: that ragged step loads every element on its own.
template <int NCT, bool KMAJ, bool SO, class EpiLoad>
__device__ __forceinline__ void walk_layer(const float* Xs, int px, const float* __restrict__ W, int ldw, int K, int N, int ct0, int nct, StreamOut& so,
                                           w4 (&acc)[2][NCT], EpiLoad&& epi_load) {
    const int lane = threadIdx.x & 63, lr = lane & 15, kk = lane >> 4;
    // (measured on gfx950: the range check of a raw buffer covers vector offset + scalar offset - with num_records reduced by the scalar offset the last
    // row of W came back as zeros one step early - so one resource serves every step and the K position rides in the scalar offset)
    const __amdgpu_buffer_rsrc_t rw = make_rsrc(W, (unsigned)(KMAJ ? K * ldw : N * ldw) * 4u);
    unsigned boff[NCT];                                            // this lane's fragment of tile j at k0 = 0: byte offset into W
#pragma unroll
    for (int j = 0; j < NCT; ++j) {
        const int n = min((ct0 + min(j, nct - 1)) * 16 + lr, N - 1);                   // columns past N / tiles past nct: copies (discarded in the epilogue)
        boff[j] = 4u * (KMAJ ? (unsigned)(n + 4 * kk * ldw) : (unsigned)(n * ldw + 4 * kk));
    }
    const float* xa = Xs + lr * px + 4 * kk;
    const bool ragged = !KMAJ && (K & 3) != 0;
    const int nvec = ragged ? (K >> 4) : ((K + 15) >> 4), tail = ragged ? (K & 15) : 0;     // steps of the uniform form; elements of the ragged step
    // The MFMAs are builtins and the order of a step is pinned with sched_group_barrier (the LDS reads of the next A fragments, then per column tile its
    // 8 MFMAs followed by the load of its next B fragment).  Left to itself the scheduler hoisted all loads to the top of the step, which made every wait
    // a vmcnt(0); sched_barrier(0) between tiles cut the region and brought accumulator copies (v_accvgpr shuffles) with it.  Writing the MFMAs as volatile
    // inline assembly was tried and dropped: the hazard recogniser does not see them, and the compiler placed vector copies of accumulators behind MFMAs
    // that had not finished (docs/HISTORY.md section 12).
    auto loadb = [&](int t, int j, w4& b) __attribute__((always_inline)) {
        const int k0 = WALK_DBG == 1 ? 0 : 16 * t;
        if (KMAJ) {
            const unsigned s0 = (unsigned)(k0 * ldw) * 4u, sl = (unsigned)ldw * 4u;      // rows k0 + s (the lane's 4 kk rows are in boff)
            b = w4{buf_load1(rw, boff[j], s0), buf_load1(rw, boff[j], s0 + sl), buf_load1(rw, boff[j], s0 + 2u * sl), buf_load1(rw, boff[j], s0 + 3u * sl)};
        } else {
            b = buf_load4(rw, boff[j], (unsigned)k0 * 4u);
        }
    };
    auto loadb_ragged = [&](int j, w4& b) __attribute__((always_inline)) {
#pragma unroll
        for (int s = 0; s < 4; ++s) {
            const int k = min(16 * nvec + 4 * kk + s, K - 1);
            b[s] = buf_load1(rw, boff[j] + 4u * (unsigned)(k - 4 * kk), 0u);             // boff holds the 4 kk part
        }
    };
    auto loada = [&](int t, w4 (&a)[2]) __attribute__((always_inline)) {
#pragma unroll
        for (int i = 0; i < 2; ++i) a[i] = *(const w4*)(xa + i * 16 * px + 16 * t);
    };
    auto mma_tile = [&](const w4 (&a)[2], const w4& b, int j, int smax) __attribute__((always_inline)) {
#pragma unroll
        for (int s = 0; s < 4; ++s) {
            if (s < smax) {
#pragma unroll
                for (int i = 0; i < 2; ++i) {
                    if (WALK_DBG == 2) { acc[i][j][0] += a[i][s] + b[s]; continue; }
                    acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x4f32(a[i][s], b[s], acc[i][j], 0, 0, 0);
                }
            }
        }
    };
    w4 a[2], an[2], b[NCT];
    if (nvec == 0) {                                                // K < 16 and ragged: the ragged step alone
        loada(0, a);
#pragma unroll
        for (int j = 0; j < NCT; ++j) loadb_ragged(j, b[j]);
        if (SO) so.flush();
#pragma unroll
        for (int j = 0; j < NCT; ++j) { mma_tile(a, b[j], j, tail); epi_load(j); }
        return;
    }
    loada(0, a);
#pragma unroll
    for (int j = 0; j < NCT; ++j) loadb(0, j, b[j]);
    for (int t = 0; t + 1 < nvec; ++t) {
        w4 sv;
        if (SO) sv = so.read();
        loada(t + 1, an);
#pragma unroll
        for (int j = 0; j < NCT; ++j) {
            mma_tile(a, b[j], j, 4);
            loadb(t + 1, j, b[j]);
        }
        if (SO) so.write(sv);
        __builtin_amdgcn_sched_group_barrier(0x100, SO ? 3 : 2, 0);
#pragma unroll
        for (int j = 0; j < NCT; ++j) {
            __builtin_amdgcn_sched_group_barrier(0x008, 8, 0);
            __builtin_amdgcn_sched_group_barrier(0x020, KMAJ ? 4 : 1, 0);
        }
        a[0] = an[0]; a[1] = an[1];
    }
    if (tail) {
        loada(nvec, an);
#pragma unroll
        for (int j = 0; j < NCT; ++j) {
            mma_tile(a, b[j], j, 4);
            loadb_ragged(j, b[j]);
        }
        if (SO) so.flush();
#pragma unroll
        for (int j = 0; j < NCT; ++j) { mma_tile(an, b[j], j, tail); epi_load(j); }     // MFMA s covers k0 + 4 kk + s: needed while s < tail
    } else {
        if (SO) so.flush();
#pragma unroll
        for (int j = 0; j < NCT; ++j) { mma_tile(a, b[j], j, 4); epi_load(j); }         // the last step has no fragment to fetch: the epilogue's loads go there
    }
}

// The same layer with bf16 OPERANDS (include/trifinger_ppo_mixed.h; the BF variant of the extended walk): acc += bf16r(X) . bf16r(op(W)), the products exact
// and the sums in fp32 on v_mfma_f32_16x16x32_bf16.  LDS and the weights stay fp32: a lane assembles the 8-k fragments of a 32-k step from the very
// fragments the fp32 form reads in two of its 16-k steps ("halves") - element j of lane (lr, kk) is k = k0 + 16 (j / 4) + 4 kk + j % 4 for BOTH operands
// (the order of the k inside a step is free as long as both use the same one) - and packs them with v_cvt_pk_bf16_f32 (round to nearest even) in registers.
// So the A fragment is two ds_read_b128 at columns k0 + 4 kk and k0 + 16 + 4 kk, conflict-free on the 16 q + 4 pitch like the fp32 form's (8 CONSECUTIVE
// k per lane, columns k0 + 8 kk and + 4, would be 2-way on every pitch in use), and the B fragment is two dwordx4 (forward) or eight dword loads (backward:
// rows k0 + 4 kk + s and k0 + 16 + 4 kk + s).  The C/D layout is that of the 16 x 16 fp32 form: epilogues, StreamOut and pitches are shared.
// K = 16 n16 halves.  A half past ceil16(K) is zero in both operands (registers); the forward half that holds the end of a row of K % 4 != 0 floats
// (41, 113) is loaded element by element with clamped k, against A values the staging zeroed; everything else is the uniform loader of the fp32 form.
typedef __bf16 h8 __attribute__((ext_vector_type(8)));
__device__ __forceinline__ h8 pack_bf16(const w4& lo, const w4& hi) {
    return __builtin_convertvector(__builtin_shufflevector(lo, hi, 0, 1, 2, 3, 4, 5, 6, 7), h8);
}
template <int NCT, bool KMAJ, bool SO, class EpiLoad>
__device__ __forceinline__ void walk_layer_bf16(const float* Xs, int px, const float* __restrict__ W, int ldw, int K, int N, int ct0, int nct, StreamOut& so,
                                                w4 (&acc)[2][NCT], EpiLoad&& epi_load) {
    const int lane = threadIdx.x & 63, lr = lane & 15, kk = lane >> 4;
    const __amdgpu_buffer_rsrc_t rw = make_rsrc(W, (unsigned)(KMAJ ? K * ldw : N * ldw) * 4u);
    unsigned boff[NCT];
#pragma unroll
    for (int j = 0; j < NCT; ++j) {
        const int n = min((ct0 + min(j, nct - 1)) * 16 + lr, N - 1);
        boff[j] = 4u * (KMAJ ? (unsigned)(n + 4 * kk * ldw) : (unsigned)(n * ldw + 4 * kk));
    }
    const float* xa = Xs + lr * px + 4 * kk;
    const bool ragged = !KMAJ && (K & 3) != 0;
    const int n16 = (K + 15) >> 4, nuni = ragged ? n16 - 1 : n16;  // halves in all; halves the uniform loader serves
    const int nfull = nuni >> 1, rem = n16 - 2 * nfull;             // 32-k steps of two uniform halves; halves of the last step (0: there is none)
    const bool lo_ragged = ragged && rem == 1, hi_there = rem == 2; // the last step: (ragged | zero), (uniform | zero) or (uniform | ragged)
    auto loadb16 = [&](int h, int j, w4& b) __attribute__((always_inline)) {
        const int k0 = 16 * h;
        if (KMAJ) {
            const unsigned s0 = (unsigned)(k0 * ldw) * 4u, sl = (unsigned)ldw * 4u;
            b = w4{buf_load1(rw, boff[j], s0), buf_load1(rw, boff[j], s0 + sl), buf_load1(rw, boff[j], s0 + 2u * sl), buf_load1(rw, boff[j], s0 + 3u * sl)};
        } else {
            b = buf_load4(rw, boff[j], (unsigned)k0 * 4u);
        }
    };
    auto loadb_ragged = [&](int h, int j, w4& b) __attribute__((always_inline)) {
#pragma unroll
        for (int s = 0; s < 4; ++s) {
            const int k = min(16 * h + 4 * kk + s, K - 1);         // k >= K: a copy of the row's last element, against an A value that is zero
            b[s] = buf_load1(rw, boff[j] + 4u * (unsigned)(k - 4 * kk), 0u);
        }
    };
    auto loada16 = [&](int h, w4 (&a)[2]) __attribute__((always_inline)) {
#pragma unroll
        for (int i = 0; i < 2; ++i) a[i] = *(const w4*)(xa + i * 16 * px + 16 * h);
    };
    const w4 zero4 = w4{0.0f, 0.0f, 0.0f, 0.0f};
    auto tail_a = [&](w4 (&a)[2][2]) __attribute__((always_inline)) {
        loada16(2 * nfull, a[0]);
        if (hi_there) loada16(2 * nfull + 1, a[1]); else { a[1][0] = zero4; a[1][1] = zero4; }
    };
    auto tail_b = [&](int j, w4 (&b)[2]) __attribute__((always_inline)) {
        if (lo_ragged) loadb_ragged(2 * nfull, j, b[0]); else loadb16(2 * nfull, j, b[0]);
        if (hi_there) loadb_ragged(2 * nfull + 1, j, b[1]); else b[1] = zero4;
    };
    auto pack_a = [&](const w4 (&a)[2][2], h8 (&pa)[2]) __attribute__((always_inline)) {
#pragma unroll
        for (int i = 0; i < 2; ++i) pa[i] = pack_bf16(a[0][i], a[1][i]);
    };
    auto mma_tile = [&](const h8 (&pa)[2], const w4 (&b)[2], int j) __attribute__((always_inline)) {
        const h8 pb = pack_bf16(b[0], b[1]);
#pragma unroll
        for (int i = 0; i < 2; ++i) acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(pa[i], pb, acc[i][j], 0, 0, 0);
    };
    w4 a[2][2], an[2][2], b[NCT][2];                                // [half][row tile], [tile][half]
    h8 pa[2];
    if (nfull == 0) {                                               // K <= 16, or K <= 32 and ragged: the last step alone
        tail_a(a);
#pragma unroll
        for (int j = 0; j < NCT; ++j) tail_b(j, b[j]);
        if (SO) so.flush();
        pack_a(a, pa);
#pragma unroll
        for (int j = 0; j < NCT; ++j) { mma_tile(pa, b[j], j); epi_load(j); }
        return;
    }
    loada16(0, a[0]); loada16(1, a[1]);
#pragma unroll
    for (int j = 0; j < NCT; ++j) { loadb16(0, j, b[j][0]); loadb16(1, j, b[j][1]); }
    for (int t = 0; t + 1 < nfull; ++t) {
        w4 sv;
        if (SO) sv = so.read();
        loada16(2 * t + 2, an[0]); loada16(2 * t + 3, an[1]);
        pack_a(a, pa);
#pragma unroll
        for (int j = 0; j < NCT; ++j) {
            mma_tile(pa, b[j], j);
            loadb16(2 * t + 2, j, b[j][0]); loadb16(2 * t + 3, j, b[j][1]);
        }
        if (SO) so.write(sv);
        // the pinned order of a step, restated for this form: the 4 LDS reads of the next A fragments (5 with a stream-out), then per column tile its
        // 2 MFMAs followed by the loads of its next B fragment (2 dwordx4 forward, 8 dwords backward); the packing goes where its MFMAs need it
        __builtin_amdgcn_sched_group_barrier(0x100, SO ? 5 : 4, 0);
#pragma unroll
        for (int j = 0; j < NCT; ++j) {
            __builtin_amdgcn_sched_group_barrier(0x008, 2, 0);
            __builtin_amdgcn_sched_group_barrier(0x020, KMAJ ? 8 : 2, 0);
        }
#pragma unroll
        for (int h = 0; h < 2; ++h) { a[h][0] = an[h][0]; a[h][1] = an[h][1]; }
    }
    if (rem) {
        tail_a(an);
        pack_a(a, pa);
#pragma unroll
        for (int j = 0; j < NCT; ++j) {
            mma_tile(pa, b[j], j);
            tail_b(j, b[j]);
        }
        if (SO) so.flush();
        pack_a(an, pa);
#pragma unroll
        for (int j = 0; j < NCT; ++j) { mma_tile(pa, b[j], j); epi_load(j); }
    } else {
        if (SO) so.flush();
        pack_a(a, pa);
#pragma unroll
        for (int j = 0; j < NCT; ++j) { mma_tile(pa, b[j], j); epi_load(j); }
    }
}

// layer + epilogue for a wavefront with NCT column tiles.  Ys: LDS output [32][py] or nullptr (last product).  G: memory output [M, N], written here only
// for the last product (the others leave through StreamOut during the next step).
//   BWD = false: v = acc + bias, ELU when act;  BWD = true: v = acc * elu'(E[row, col]) when E (the saved output of the layer this is the dZ of)
//   EXT (the extended walk, include/trifinger_ppo_net.h): `act` is an activation code, forwards and backwards; ldw / lde are the leading dimensions of W and E
//   (the plain walk passes BWD ? N : K and N); xcols: the columns of Ys behind N belong to the row block's input (d2rl) and are not written here.
template <int NCT, bool BWD, bool SO, bool EXT, bool BF = false>
__device__ __forceinline__ void walk_run(const float* Xs, int px, const float* __restrict__ W, int ldw, int K, int N, const float* __restrict__ bias, int act,
                                         const float* __restrict__ E, int lde, bool xcols, float* Ys, int py, float* __restrict__ G, int row0, int M, int ct0,
                                         int nct, StreamOut& so, int stamp) {
    const int lane = threadIdx.x & 63, lr = lane & 15, kk = lane >> 4;
    const int colb = ct0 * 16 + lr;                                // + 16 j
    const int rowb = 4 * kk;                                       // + 16 i + r: C layout of the 16 x 16 forms, column = lane % 16, row = 4 (lane / 16) + register
    // Every store issued so far (a stream-out fallback, the previous walk step) is waited for HERE, explicitly: on gfx9 loads and stores share vmcnt, and a
    // store that MAY be pending at the head of the K loop (the compiler merges the paths into it) turns the first wait of every step into vmcnt(0).
    // (lgkmcnt too: a FLAT access that may be pending - the compiler does not always prove a pointer out of the argument block global - forces both to 0)
    __builtin_amdgcn_s_waitcnt(0);
    // what the epilogue needs from memory is requested BEFORE the K loop (a round trip to memory is 2 - 3 thousand cycles; a lone wavefront would sit it out)
    float bv[NCT];
    w4 e[2][BWD ? NCT : 1];
    unsigned eoff[2][4];
    if (BWD) {
        if (E) {                                                    // rows past M / columns past N: clamped copies, never stored
#pragma unroll
            for (int i = 0; i < 2; ++i) {
#pragma unroll
                for (int r = 0; r < 4; ++r) eoff[i][r] = (unsigned)min(row0 + rowb + 16 * i + r, M - 1) * (unsigned)lde;
            }
        }
    } else {
#pragma unroll
        for (int j = 0; j < NCT; ++j) bv[j] = bias ? ((const gfloat*)bias)[min(colb + 16 * min(j, nct - 1), N - 1)] : 0.0f;
    }
    // backward: the 8 saved outputs a tile's epilogue needs are requested in the LAST K step, where the tile has no next fragment to fetch (before the
    // loop they would be 56 more loads in flight than the 6-bit vmcnt can count)
    auto epi_load = [&](int j) __attribute__((always_inline)) {
        if (BWD) {
            if (E) {
                const unsigned c = (unsigned)min(colb + 16 * min(j, nct - 1), N - 1);
#pragma unroll
                for (int i = 0; i < 2; ++i) {
#pragma unroll
                    for (int r = 0; r < 4; ++r) e[i][BWD ? j : 0][r] = ((const gfloat*)E)[eoff[i][r] + c];
                }
            }
        }
    };
    w4 acc[2][NCT];
#pragma unroll
    for (int i = 0; i < 2; ++i) {
#pragma unroll
        for (int j = 0; j < NCT; ++j) acc[i][j] = w4{0.0f, 0.0f, 0.0f, 0.0f};
    }
#pragma unroll
    for (int i = 0; i < 2; ++i) {
#pragma unroll
        for (int j = 0; j < NCT; ++j) asm volatile("" : "+v"(acc[i][j]));       // the zeroing instructions stay in front of ...
    }
    asm volatile("s_nop 7" ::: "memory");                          // ... the wait states before the first MFMA reads an accumulator as srcC
    if constexpr (BF) walk_layer_bf16<NCT, BWD, SO>(Xs, px, W, ldw, K, N, ct0, nct, so, acc, epi_load);
    else walk_layer<NCT, BWD, SO>(Xs, px, W, ldw, K, N, ct0, nct, so, acc, epi_load);
    walk_mfma_drain<NCT>(acc);
    WSTAMP(2 + 3 * stamp);
    if (EXT) {
        if (!BWD || E) {
            switch (act) {                                          // uniform per layer
                case TFP_ACT_ELU: act_tiles<TFP_ACT_ELU, BWD, NCT>(acc, bv, e); break;
                case TFP_ACT_RELU: act_tiles<TFP_ACT_RELU, BWD, NCT>(acc, bv, e); break;
                case TFP_ACT_TANH: act_tiles<TFP_ACT_TANH, BWD, NCT>(acc, bv, e); break;
                case TFP_ACT_SIGMOID: act_tiles<TFP_ACT_SIGMOID, BWD, NCT>(acc, bv, e); break;
                case TFP_ACT_SELU: act_tiles<TFP_ACT_SELU, BWD, NCT>(acc, bv, e); break;
                case TFP_ACT_SOFTPLUS: act_tiles<TFP_ACT_SOFTPLUS, BWD, NCT>(acc, bv, e); break;
                default: act_tiles<TFP_ACT_NONE, BWD, NCT>(acc, bv, e); break;
            }
        }
    } else if (BWD) {
        if (E) {
#pragma unroll
            for (int j = 0; j < NCT; ++j) {
#pragma unroll
                for (int i = 0; i < 2; ++i) {
#pragma unroll
                    for (int r = 0; r < 4; ++r) { const float yv = e[i][j][r]; acc[i][j][r] *= (yv > 0.0f ? 1.0f : yv + 1.0f); }
                }
            }
        }
    } else {
#pragma unroll
        for (int j = 0; j < NCT; ++j) {
#pragma unroll
            for (int i = 0; i < 2; ++i) {
#pragma unroll
                for (int r = 0; r < 4; ++r) { const float v = acc[i][j][r] + bv[j]; acc[i][j][r] = act ? elu_fast(v) : v; }
            }
        }
    }
    const bool rows_in = row0 + WALK_ROWS <= M;                    // uniform: every row of the block exists
#pragma unroll
    for (int j = 0; j < NCT; ++j) {
        if (j < nct) {
            const int col = colb + 16 * j;
            const bool full = (ct0 + j) * 16 + 16 <= N;            // uniform: the tile lies wholly inside the matrix (all but possibly the last one)
            if (Ys) {                                              // next step's A operand; zero in the padding columns
                float* yp = Ys + rowb * py + col;
                if (EXT && xcols) {                                 // the columns behind N hold the input: nothing is written there
                    if (full || col < N) {
#pragma unroll
                        for (int i = 0; i < 2; ++i) {
#pragma unroll
                            for (int r = 0; r < 4; ++r) yp[(16 * i + r) * py] = acc[i][j][r];
                        }
                    }
                    continue;
                }
#pragma unroll
                for (int i = 0; i < 2; ++i) {
#pragma unroll
                    for (int r = 0; r < 4; ++r) yp[(16 * i + r) * py] = (full || col < N) ? acc[i][j][r] : 0.0f;
                }
            } else if (G) {                                        // last product of the walk: straight to memory
                gfloat* gp = (gfloat*)(G + (size_t)(row0 + rowb) * N + col);
                if (full && rows_in) {
#pragma unroll
                    for (int i = 0; i < 2; ++i) {
#pragma unroll
                        for (int r = 0; r < 4; ++r) gp[(16 * i + r) * N] = acc[i][j][r];
                    }
                } else {
#pragma unroll
                    for (int i = 0; i < 2; ++i) {
#pragma unroll
                        for (int r = 0; r < 4; ++r) { if (col < N && row0 + rowb + 16 * i + r < M) gp[(16 * i + r) * N] = acc[i][j][r]; }
                    }
                }
            }
        }
    }
}

// this wavefront's share of a layer: all 32 rows and a quarter of the 16-column tiles (the first `nct_all % 4` wavefronts take one more); the tile count
// selects the instantiation with exactly that many accumulator columns
template <bool BWD, bool EXT, bool BF = false>
__device__ __forceinline__ void walk_dispatch(const float* Xs, int px, const float* __restrict__ W, int ldw, int K, int N, const float* __restrict__ bias,
                                              int act, const float* __restrict__ E, int lde, bool xcols, float* Ys, int py, float* __restrict__ G, int row0,
                                              int M, StreamOut& so, bool has_so, int stamp) {
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int nct_all = (N + 15) >> 4, base = nct_all >> 2, rem = nct_all & 3;
    const int nct = base + (wave < rem ? 1 : 0), ct0 = wave * base + min(wave, rem);
    if (nct <= 0) { if (has_so) so.flush(); return; }
#define WALK_CASE(n_) do { if (has_so) walk_run<n_, BWD, true, EXT, BF>(Xs, px, W, ldw, K, N, bias, act, E, lde, xcols, Ys, py, G, row0, M, ct0, nct, so, stamp); \
                           else walk_run<n_, BWD, false, EXT, BF>(Xs, px, W, ldw, K, N, bias, act, E, lde, xcols, Ys, py, G, row0, M, ct0, nct, so, stamp); } while (0)
    switch (nct) {
        case 1: WALK_CASE(1); break;
        case 2: WALK_CASE(2); break;
        case 3: WALK_CASE(3); break;
        case 4: WALK_CASE(4); break;
        case 5: WALK_CASE(5); break;
        case 6: WALK_CASE(6); break;
        default: WALK_CASE(7); break;
    }
#undef WALK_CASE
}

// Input statistics of the forward walk (tfp_mlp_forward_norm; csrc/ppo_norm.hip holds the record they are published from): a network with mean != NULL
// reads clamp((x - mean) * inv_std, -clip, clip) instead of x - formed where the row block's input is staged into LDS, so the rollout normalises the env's live
// observation buffers without a launch or a copy of its own.  The statistics travel behind WalkArgs: the plain kernels keep their argument block.
struct WalkNorm { const float* mean[2]; const float* inv[2]; float clip[2]; };
struct WalkArgsNorm : WalkArgs { WalkNorm nm; };
// The extended walk (include/trifinger_ppo_net.h; EXT): activation codes in WalkNet.act, and kin[ni][l] = the width of layer l's INPUT OPERAND - dim[l], or
// dim[l] + dim[0] where a d2rl network concatenates its input behind the hidden output (1 <= l <= nl - 2).  That width is the K of the forward product, the
// leading dimension of W[l] and the row stride of the saved output yin[l - 1]; the backward chain reads the first dim[l] columns of each.  Like the statistics
// it travels behind WalkArgs: the plain kernels keep their argument block and their code.
struct WalkArgsExt : WalkArgsNorm { int kin[2][WALK_MAXL]; };
template <bool NORM, bool EXT> struct walk_args { typedef WalkArgs type; };
template <> struct walk_args<true, false> { typedef WalkArgsNorm type; };
template <bool NORM> struct walk_args<NORM, true> { typedef WalkArgsExt type; };

// two workgroups of four wavefronts per CU: two wavefronts per SIMD, 256 registers each.  NORM (forward only): the staged input passes through a.nm.
// EXT forward is always NORM (a network without statistics has mean NULL); with the wide rows of a d2rl network its LDS may exceed half a CU's: then one
// workgroup per CU runs, with the same code.
template <bool BWD, bool NORM = false, bool EXT = false, bool BF = false>
__global__ void __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(2, 2))) k_mlp_walk(const typename walk_args<NORM, EXT>::type a) {
    extern __shared__ __attribute__((aligned(16))) float lds[];
    const int ni = (int)blockIdx.x / a.blocks_per_net;
    if (ni >= a.n_nets) return;
    const WalkNet& net = a.net[ni];
    const int row0 = ((int)blockIdx.x - ni * a.blocks_per_net) * WALK_ROWS;
    if (row0 >= a.M) return;
    float* P = lds;
    float* Q = lds + a.p_floats;
    WSTAMP(0);
    const int nl = net.nl;
    // ---- the row block's input -> P: the block is one contiguous piece of memory (rows past M: zero), read linearly, sixteen loads in flight per thread;
    // the padding columns D .. ceil16(D) are zeroed by the threads that own them ----
    {
        const int D = BWD ? net.dim[nl] : net.dim[0], D16 = (D + 15) & ~15, px = D16 + 4;
        const int rows = min(WALK_ROWS, a.M - row0), total = rows * D;
        const gfloat* src = (const gfloat*)(net.x + (size_t)row0 * D);
        const int dr = 256 / D, dc = 256 - dr * D;
        int row = (int)threadIdx.x / D, col = (int)threadIdx.x - row * D;
        for (int c = threadIdx.x; c < WALK_ROWS * D; c += 16 * 256) {
            float v[16];
#pragma unroll
            for (int u = 0; u < 16; ++u) v[u] = src[min(c + 256 * u, total - 1)];
#pragma unroll
            for (int u = 0; u < 16; ++u) {
                if constexpr (NORM) {
#pragma clang fp contract(off)                               // the difference and the product rounded separately: torch.clamp((x - mean) * inv_std, -clip, clip) bit for bit
                    const gfloat* nmean = (const gfloat*)a.nm.mean[ni];
                    if (nmean) {                                    // uniform: a network of the call may come without statistics
                        const float hi = a.nm.clip[ni], lo = -hi;
                        const float df = v[u] - nmean[col], y = df * ((const gfloat*)a.nm.inv[ni])[col];
                        v[u] = y < lo ? lo : (y > hi ? hi : y);
                    }
                }
                if (c + 256 * u < WALK_ROWS * D) P[row * px + col] = (c + 256 * u < total) ? v[u] : 0.0f;
                col += dc; row += dr;
                if (col >= D) { col -= D; row += 1; }
            }
        }
        const int pad = D16 - D;
        for (int e = threadIdx.x; e < WALK_ROWS * pad; e += 256) { const int r = e / pad; P[r * px + D + (e - r * pad)] = 0.0f; }
    }
    __syncthreads();
    WSTAMP(1);
    float* cur = P;
    float* nxt = Q;
    float* pend = nullptr;                                         // memory destination of what `cur` holds (the hidden output / dZ of the step before)
#pragma unroll 1
    for (int s = 0; s < nl; ++s) {
        // forward: layer l = s maps dim[l] -> dim[l + 1]; backward: step s undoes layer l = nl - 1 - s: K = dim[l + 1] -> N = dim[l]; the product of the
        // first layer's input gradient is not formed
        const int l = BWD ? nl - 1 - s : s;
        if (BWD && l == 0) break;
        int K = BWD ? net.dim[l + 1] : net.dim[l];
        const int N = BWD ? net.dim[l] : net.dim[l + 1];
        int px = pitch_of(K), py = pitch_of(N), ldw = BWD ? N : K, lde = N;
        const bool lastp = BWD ? (l == 1) : (l == nl - 1);
        float* Ys = lastp ? nullptr : nxt;
        bool xcols = false;
        if constexpr (EXT) {
            const int kin = a.kin[ni][l];
            ldw = kin;
            if (BWD) {
                lde = kin;                                          // yin[l - 1] = [h_l | x] where the forward kept the operand of layer l
            } else {
                K = kin; px = pitch_of(K);
                const int kn = lastp ? N : a.kin[ni][l + 1], D0 = kn - N;
                if (D0 > 0) {
                    // d2rl: the next operand is [h | x].  The input columns are copied from this step's operand (x itself, or [h' | x]), the epilogue below
                    // writes the N columns in front of them; nxt was last read as the operand of the step before (a barrier ago)
                    xcols = true;
                    py = pitch_of(kn);
                    const int xoff = K - D0, pad = py - 4 - kn;
                    for (int e = threadIdx.x; e < WALK_ROWS * D0; e += 256) { const int r = e / D0, c = e - r * D0; nxt[r * py + N + c] = cur[r * px + xoff + c]; }
                    for (int e = threadIdx.x; e < WALK_ROWS * pad; e += 256) { const int r = e / pad; nxt[r * py + kn + (e - r * pad)] = 0.0f; }
                }
            }
        }
        StreamOut so;
        bool has_so = false;
        if (pend) {
            if ((K & 3) == 0 && (((uintptr_t)pend) & 15) == 0) {
                so.init(pend, cur, px, K, row0, a.M);
                has_so = true;
            } else {                                                // rows that are no multiple of 16 bytes: element by element, here and now
                const int rows = min(WALK_ROWS, a.M - row0), total = rows * K;
                gfloat* g0 = (gfloat*)(pend + (size_t)row0 * K);
                const int dr = 256 / K, dc = 256 - dr * K;
                int row = (int)threadIdx.x / K, col = (int)threadIdx.x - row * K;
                for (int c = threadIdx.x; c < total; c += 256) {
                    g0[c] = cur[row * px + col];
                    col += dc; row += dr;
                    if (col >= K) { col -= K; row += 1; }
                }
            }
        }
        const float* E = BWD ? (net.act[l - 1] ? net.yin[l - 1] : nullptr) : nullptr;
        float* G = BWD ? net.y[l - 1] : net.y[l];
        const int act = BWD ? (EXT ? net.act[l - 1] : 0) : net.act[l];
        const float* bias = BWD ? nullptr : net.b[l];
        walk_dispatch<BWD, EXT, BF>(cur, px, net.W[l], ldw, K, N, bias, act, E, lde, xcols, Ys, py, G, row0, a.M, so, has_so, s);
        WSTAMP(3 + 3 * s);
        if (!lastp) __syncthreads();
        WSTAMP(4 + 3 * s);
        pend = lastp ? nullptr : G;
        float* t = cur; cur = nxt; nxt = t;
    }
}

// kin (the extended walk): the operand widths of the forward walk, see WalkArgsExt; limit: the LDS a workgroup may take
static int walk_prepare(WalkArgs& a, int M, bool bwd, size_t* lds_bytes, const int (*kin)[WALK_MAXL] = nullptr, size_t limit = 80 * 1024, bool shapes_only = false) {
    // the two LDS buffers are used alternately: the input and every second product in P, the others in Q
    int p = 0, q = 0;
    for (int ni = 0; ni < a.n_nets; ++ni) {
        const WalkNet& n = a.net[ni];
        if (n.nl < 1 || n.nl > WALK_MAXL) return -1;
        for (int l = 0; l <= n.nl; ++l) if (n.dim[l] <= 0) return -1;
        if (!shapes_only) {
            for (int l = 0; l < n.nl; ++l) if (!n.W[l] && !(bwd && l == 0)) return -1;
            if (!n.x) return -1;
        }
        for (int l = 1; l <= n.nl; ++l) if (n.dim[l] > 416) return -4;                 // 26 column tiles: 7 + 7 + 6 + 6 accumulator columns
        if (n.dim[0] > 416) return -4;
        int seq[WALK_MAXL + 1], cnt = 0;
        if (!bwd) { for (int l = 0; l < n.nl; ++l) seq[cnt++] = kin ? kin[ni][l] : n.dim[l]; }   // operands that live in LDS: input and all but the last output
        else { for (int l = n.nl; l >= 2; --l) seq[cnt++] = n.dim[l]; if (n.nl == 1) seq[cnt++] = n.dim[1]; }
        for (int i = 0; i < cnt; ++i) {
            const int fl = WALK_ROWS * ((((seq[i] + 15) & ~15)) + 4);
            if (i & 1) { if (fl > q) q = fl; } else { if (fl > p) p = fl; }
        }
    }
    a.p_floats = p;
    a.M = M;
    a.blocks_per_net = (M + WALK_ROWS - 1) / WALK_ROWS;
    *lds_bytes = (size_t)(p + q) * sizeof(float);
    return *lds_bytes <= limit ? 0 : -4;                           // half a CU's LDS: two workgroups per CU (the forward walk of a d2rl network: up to all of it)
}

extern "C" {

static int walk_launch(const TfpMlp* nets, int32_t n_nets, int32_t M, bool bwd, void* stream, const TfpNorm* norm = nullptr) {
    if (!nets || n_nets < 1 || n_nets > 2 || M <= 0) return -1;
    WalkNorm nm; memset(&nm, 0, sizeof(nm));
    bool with_norm = false;
    for (int ni = 0; norm && ni < n_nets; ++ni) {
        if (!norm[ni].mean) continue;
        if (bwd || !norm[ni].inv_std || !(norm[ni].clip > 0.0f)) return -1;
        nm.mean[ni] = norm[ni].mean; nm.inv[ni] = norm[ni].inv_std; nm.clip[ni] = norm[ni].clip;
        with_norm = true;
    }
    WalkArgs a; memset(&a, 0, sizeof(a));
    a.n_nets = n_nets;
    for (int ni = 0; ni < n_nets; ++ni) {
        WalkNet& d = a.net[ni]; const TfpMlp& s = nets[ni];
        if (s.n_layers < 1 || s.n_layers > WALK_MAXL) return -1;
        d.x = s.x; d.nl = s.n_layers;
        for (int l = 0; l < WALK_MAXL; ++l) { d.W[l] = s.W[l]; d.b[l] = s.b[l]; d.yin[l] = s.yin[l]; d.y[l] = s.y[l]; d.act[l] = s.act[l]; }
        for (int l = 0; l <= WALK_MAXL; ++l) d.dim[l] = s.dim[l];
        if (!bwd && !s.y[s.n_layers - 1]) return -1;
        if (bwd) for (int l = 0; l + 1 < s.n_layers; ++l) { if (!s.y[l]) return -1; if (s.act[l] && !s.yin[l]) return -1; }
    }
    size_t lds = 0;
    const int rc = walk_prepare(a, M, bwd, &lds);
    if (rc) return rc;
    static bool attr_set[3] = {false, false, false};
    const int which = with_norm ? 2 : (bwd ? 1 : 0);
    if (!attr_set[which]) {
        const void* f = with_norm ? (const void*)k_mlp_walk<false, true> : bwd ? (const void*)k_mlp_walk<true> : (const void*)k_mlp_walk<false>;
        if (hipFuncSetAttribute(f, hipFuncAttributeMaxDynamicSharedMemorySize, 80 * 1024) != hipSuccess) return -2;
        attr_set[which] = true;
    }
    const dim3 grid(a.blocks_per_net * n_nets), block(256);
    hipStream_t s = (hipStream_t)stream;
    if (with_norm) { WalkArgsNorm an; static_cast<WalkArgs&>(an) = a; an.nm = nm; hipLaunchKernelGGL((k_mlp_walk<false, true>), grid, block, lds, s, an); }
    else if (bwd) hipLaunchKernelGGL(k_mlp_walk<true>, grid, block, lds, s, a);
    else hipLaunchKernelGGL(k_mlp_walk<false>, grid, block, lds, s, a);
    return hipGetLastError() == hipSuccess ? 0 : -3;
}

// forward of n_nets <= 2 Linear / ELU stacks over the same M rows in ONE launch; -4: the shapes do not fit the walk (a layer wider than 416, LDS):
// the caller runs the layers one by one (tfp_linear_fwd[_group])
int tfp_mlp_forward(const TfpMlp* nets, int32_t n_nets, int32_t M, void* stream) { return walk_launch(nets, n_nets, M, false, stream); }
// ... with optional input statistics per network (norm[i].mean == NULL: network i reads its input as it is; norm == NULL or no statistics at all: tfp_mlp_forward)
int tfp_mlp_forward_norm(const TfpMlp* nets, const TfpNorm* norm, int32_t n_nets, int32_t M, void* stream) {
    return walk_launch(nets, n_nets, M, false, stream, norm);
}
// the input-gradient chain of the same stacks in ONE launch: x = gradient of the network output, yin[l] = saved output of layer l, y[l] = dZ of layer l
// (l < n_layers - 1; the dZ of the last layer is x itself)
int tfp_mlp_backward(const TfpMlp* nets, int32_t n_nets, int32_t M, void* stream) { return walk_launch(nets, n_nets, M, true, stream); }

// ---- the extended walk (include/trifinger_ppo_net.h): activation codes 0 .. 6, d2rl, optional statistics ----
static int net_setup(const TfpNet* nets, int32_t n_nets, bool bwd, bool shapes_only, WalkArgsExt& a, bool* any_d2rl) {
    if (!nets || n_nets < 1 || n_nets > 2) return -1;
    memset(&a, 0, sizeof(a));
    a.n_nets = n_nets;
    *any_d2rl = false;
    for (int ni = 0; ni < n_nets; ++ni) {
        WalkNet& d = a.net[ni]; const TfpMlp& s = nets[ni].mlp;
        if (s.n_layers < 1 || s.n_layers > WALK_MAXL) return -1;
        d.x = s.x; d.nl = s.n_layers;
        for (int l = 0; l < WALK_MAXL; ++l) { d.W[l] = s.W[l]; d.b[l] = s.b[l]; d.yin[l] = s.yin[l]; d.y[l] = s.y[l]; d.act[l] = s.act[l]; }
        for (int l = 0; l <= WALK_MAXL; ++l) d.dim[l] = s.dim[l];
        for (int l = 0; l < s.n_layers; ++l) {
            if (s.dim[l] <= 0) return -1;
            if (s.act[l] < TFP_ACT_NONE || s.act[l] > TFP_ACT_SOFTPLUS) return -1;
            const bool wide = nets[ni].d2rl && l >= 1 && l <= s.n_layers - 2;
            a.kin[ni][l] = s.dim[l] + (wide ? s.dim[0] : 0);
            if (wide) *any_d2rl = true;
        }
        if (shapes_only) continue;
        if (!bwd && !s.y[s.n_layers - 1]) return -1;
        if (bwd) for (int l = 0; l + 1 < s.n_layers; ++l) { if (!s.y[l]) return -1; if (s.act[l] && !s.yin[l]) return -1; }
        if (nets[ni].mean) {
            if (bwd || !nets[ni].inv_std || !(nets[ni].clip > 0.0f)) return -1;
            a.nm.mean[ni] = nets[ni].mean; a.nm.inv[ni] = nets[ni].inv_std; a.nm.clip[ni] = nets[ni].clip;
        }
    }
    return 0;
}
static int net_launch(const TfpNet* nets, int32_t n_nets, int32_t M, bool bwd, void* stream, bool shapes_only, bool bf16 = false) {
    if (M <= 0) return -1;
    WalkArgsExt a; bool d2rl = false;
    int rc = net_setup(nets, n_nets, bwd, shapes_only, a, &d2rl);
    if (rc) return rc;
    // the wide operand rows of a d2rl network exist in the forward walk only (the backward chain runs over the hidden part): that call alone may take a whole CU
    const size_t limit = (!bwd && d2rl) ? 160 * 1024 : 80 * 1024;
    size_t lds = 0;
    rc = walk_prepare(a, M, bwd, &lds, a.kin, limit, shapes_only);
    if (rc || shapes_only) return rc;
    // (bf16: the BF instantiations of the same kernel - LDS, limits and argument block are those of the fp32 form, d2rl included)
    static bool attr_set[4] = {false, false, false, false};
    const int which = (bf16 ? 2 : 0) + (bwd ? 1 : 0);
    const void* f = bf16 ? (bwd ? (const void*)k_mlp_walk<true, false, true, true> : (const void*)k_mlp_walk<false, true, true, true>)
                         : (bwd ? (const void*)k_mlp_walk<true, false, true> : (const void*)k_mlp_walk<false, true, true>);
    if (!attr_set[which]) {
        if (hipFuncSetAttribute(f, hipFuncAttributeMaxDynamicSharedMemorySize, bwd ? 80 * 1024 : 160 * 1024) != hipSuccess) return -2;
        attr_set[which] = true;
    }
    const dim3 grid(a.blocks_per_net * n_nets), block(256);
    hipStream_t s = (hipStream_t)stream;
    if (bf16) {
        if (bwd) hipLaunchKernelGGL((k_mlp_walk<true, false, true, true>), grid, block, lds, s, a);
        else hipLaunchKernelGGL((k_mlp_walk<false, true, true, true>), grid, block, lds, s, a);
    } else if (bwd) hipLaunchKernelGGL((k_mlp_walk<true, false, true>), grid, block, lds, s, a);
    else hipLaunchKernelGGL((k_mlp_walk<false, true, true>), grid, block, lds, s, a);
    return hipGetLastError() == hipSuccess ? 0 : -3;
}
int tfp_net_forward(const TfpNet* nets, int32_t n_nets, int32_t M, void* stream) { return net_launch(nets, n_nets, M, false, stream, false); }
int tfp_net_backward(const TfpNet* nets, int32_t n_nets, int32_t M, void* stream) { return net_launch(nets, n_nets, M, true, stream, false); }
int tfp_net_fits(const TfpNet* nets, int32_t n_nets, int32_t backward) { return net_launch(nets, n_nets, 1, backward != 0, nullptr, true); }
// ---- `mixed_precision` (include/trifinger_ppo_mixed.h): the same walk with bf16 operands on v_mfma_f32_16x16x32_bf16 ----
int tfp_net_forward_bf16(const TfpNet* nets, int32_t n_nets, int32_t M, void* stream) { return net_launch(nets, n_nets, M, false, stream, false, true); }
int tfp_net_backward_bf16(const TfpNet* nets, int32_t n_nets, int32_t M, void* stream) { return net_launch(nets, n_nets, M, true, stream, false, true); }
int tfp_net_fits_bf16(const TfpNet* nets, int32_t n_nets, int32_t backward) { return net_launch(nets, n_nets, 1, backward != 0, nullptr, true, true); }

#ifdef WALK_TIMING
int tfp_walk_debug_read(unsigned long long* out) { return hipMemcpyFromSymbol(out, HIP_SYMBOL(g_walk_t), sizeof(unsigned long long) * 128) == hipSuccess ? 0 : -3; }
#endif
}  // extern "C"
