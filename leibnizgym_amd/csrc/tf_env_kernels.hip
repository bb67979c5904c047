// tf_env_kernels.hip - the fused TriFinger step kernel (roles: tf_roles.h) and the EnvUnit of ONE translation unit (tf_launch.h).
//
// Compiled once per unit of the Makefile's UNITS (-DTF_EXT=0|1|2 -DTF_WIDE=0|1|2, and -DTF_SURF=1 / -DTF_DR=1 below): EXT 0 the headline kernels, 1 the extended domain
// randomisation, 2 the general box object; WIDE 0 the 128-register instantiation (four workgroups per CU), 1 the 256-register one for populations of at
// most 32768 envs, 2 the 256-register one with four helper wavefronts per workgroup (one workgroup per CU: at most 16384 envs; the launches that
// simulate only - the others are served by the WIDE = 1 unit).
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "tf_roles.h"
#include "tf_launch.h"

#ifndef TF_EXT
#error "compile with -DTF_EXT=0|1|2 -DTF_WIDE=0|1|2"
#endif
// -DTF_SURF=1: the instantiations with the surface normal of the cube corners on the flared part of the boundary (TfModel.cube_wall_surface; EXT 0 and 1,
// WIDE 1 and 2 only).  Their kernel (k_env_surf) and unit (tf_unit_s<EXT>_<WIDE>) have names of their own; they carry the launches that simulate.
#ifndef TF_SURF
#define TF_SURF 0
#endif
// -DTF_DR=1: the EXT 0 and EXT 2 kernels with the base domain randomisation (cube mass and size, friction, motor strength, link mass, restitution; observation
// noise and action repeat) as a run-time flag of the parameter block.  Their kernel (k_env_dr) and unit (tf_unit_d<EXT>_<WIDE>) have names of their own: the
// plain EXT 0 and EXT 2 units are built WITHOUT domain randomisation (DR_RT false: the factors are constants, no TF_S_DR row, L_DR0 slot or previous torque is
// touched, the noise blocks and their barriers are not in the code object) - dr_enable is fixed at tf_create, and the host picks the unit from it (unit_for).
// The EXT 1 kernels (only ever launched with dr_enable set) and the surface-normal kernels keep the run-time flag under their own names.
#ifndef TF_DR
#define TF_DR 0
#endif
#if TF_DR && (TF_EXT == 1 || TF_SURF)
#error "TF_DR: the EXT 0 and EXT 2 kernels without the surface normal only (-DTF_EXT=0|2 -DTF_WIDE=0|1|2)"
#endif
#define DR_RT (TF_DR || TF_EXT == 1 || TF_SURF)
#if TF_SURF
#if TF_EXT == 2 || TF_WIDE == 0
#error "TF_SURF: the 256-register cube kernels only (-DTF_EXT=0|1 -DTF_WIDE=1|2)"
#endif
#define K_ENV k_env_surf
#define TF_UNIT_PREFIX tf_unit_s
#elif TF_DR
#define K_ENV k_env_dr
#define TF_UNIT_PREFIX tf_unit_d
#else
#define K_ENV k_env
#define TF_UNIT_PREFIX tf_unit_
#endif

// One launch = one or more hooks of the reference step (MODE) for every env of the handle.
// WIDE = false: 128 registers, 4 workgroups per CU (4 wavefronts per SIMD) - populations that fill the chip; WIDE = true: 256 registers, no spills,
// nothing parked in LDS between substeps, the cube role's contact-space records in registers - populations of at most 32768 envs, which never put
// more than two workgroups on a CU, so the occupancy the narrow build buys is not used (tf_create picks).  Same arithmetic.
// HELP: the WIDE kernel in workgroups of eight wavefronts - 0..2 fingers, 3 cube, 4..7 helpers (tf_roles.h: helper_role) - for populations that leave a CU to
// one workgroup: the second wavefront slot of every SIMD, empty otherwise, carries the finger-finger rows (middle-distal: 4..6, distal pass: 7).  Same arithmetic again.
template <int A, bool IS_RESET, bool ASYM, int MODE, int EXT, bool WIDE, bool HELP = false>
__global__ void __launch_bounds__(HELP ? NT_HELP : NT, HELP ? 1 : (WIDE ? 2 : 4)) K_ENV(const DevParams* __restrict__ Pp, const StepArgs sa, const float* __restrict__ action) {
    __shared__ __attribute__((aligned(16))) float lds[(TF_SURF ? LDS_SLOTS_SURF : (EXT == 2) ? (WIDE ? LDS_SLOTS_BOX_WIDE : LDS_SLOTS_BOX) : (HELP ? LDS_SLOTS_HELP : LDS_SLOTS)) * WAVE];
    const DevParams& P = *Pp;
    {   // Warm the scalar cache with the parameter block (one dword per 64-byte line) BEFORE the state loads of every workgroup of the
        // launch saturate the L2: the model constants the free motion needs then come out of the constant cache instead of queueing
        // behind that burst.
        const unsigned* pw = reinterpret_cast<const unsigned*>(Pp);
        unsigned touch = 0u;
        // (the host-formed invariants at the end of the block are read by the 128-register kernels without domain randomisation only: the others stop in front of them)
        constexpr unsigned warm = (WIDE || DR_RT) ? (unsigned)offsetof(DevParams, inv_cube_inertia) : (unsigned)sizeof(DevParams);
#pragma unroll
        for (unsigned k = 0; k < warm / 64u; ++k) touch |= pw[16u * k];
        asm volatile("" ::"s"(touch));
    }
    Ctx cx;
    cx.tid = (int)threadIdx.x;
    cx.lane = (int)threadIdx.x & (WAVE - 1);
    cx.role = __builtin_amdgcn_readfirstlane((int)threadIdx.x >> 6);
    cx.wave_first = (int)blockIdx.x * WAVE;
    const int i_raw = cx.wave_first + cx.lane;
    cx.valid = i_raw < P.N;
    cx.i = cx.valid ? i_raw : (P.N - 1);
    cx.n_valid = (P.N - cx.wave_first < WAVE) ? (P.N - cx.wave_first) : WAVE;
    if (cx.role == 3) cube_role<A, IS_RESET, ASYM, MODE, EXT, WIDE, HELP, TF_SURF != 0, DR_RT != 0>(P, sa, action, lds, cx);
    else if (HELP && cx.role > 3) helper_role<ASYM, MODE, EXT, DR_RT != 0>(P, sa, lds, cx);
    else finger_role<A, IS_RESET, ASYM, MODE, EXT, WIDE, HELP, DR_RT != 0>(P, sa, action, lds, cx);
}


using EnvKernel = void (*)(const DevParams*, StepArgs, const float*);

// the instantiation of (MODE, action_dim, asym) in this unit, or nullptr
template <int MODE, bool IS_RESET>
static EnvKernel kernel(int action_dim, bool asym) {
    constexpr int EXT = TF_EXT;
    constexpr bool WIDE = TF_WIDE != 0, HELP = TF_WIDE == 2;
    if (action_dim == 9) return asym ? K_ENV<9, IS_RESET, true, MODE, EXT, WIDE, HELP> : K_ENV<9, IS_RESET, false, MODE, EXT, WIDE, HELP>;
#if !defined(TF_DEV_MIN)      // developer builds carry A = 9 only
    if (action_dim == 18) return asym ? K_ENV<18, IS_RESET, true, MODE, EXT, WIDE, HELP> : K_ENV<18, IS_RESET, false, MODE, EXT, WIDE, HELP>;
#endif
    return nullptr;
}

// the kernel of launch mode lm, or nullptr where this unit does not instantiate it (the kernels land in the code object in the order of the cases)
static EnvKernel kernel_for(int lm, int action_dim, bool asym) {
    switch (lm) {
    case TF_LM_STEP: return kernel<M_FUSED_STEP, false>(action_dim, asym);
    case TF_LM_RESET: return kernel<M_FUSED_RESET, true>(action_dim, asym);
#if !defined(TF_DEV_MIN)      // developer builds carry the fused launches only
    case TF_LM_SIM: return kernel<M_SIM, false>(action_dim, asym);
#if TF_WIDE != 2 && !TF_SURF   // (the helper and surface units carry the launches that simulate; the host sends the others to the WIDE = 1 unit)
    case TF_LM_RESETS: return kernel<M_RESETS, false>(action_dim, asym);
    case TF_LM_TORQUE: return kernel<M_TORQUE, false>(action_dim, asym);
    case TF_LM_POST: return kernel<M_POST, false>(action_dim, asym);
    case TF_LM_FINISH: return kernel<M_FINISH, false>(action_dim, asym);
#endif
#endif
    case TF_LM_STEP_RAND: return kernel<M_FUSED_STEP_RAND, false>(action_dim, asym);
    }
    return nullptr;
}

static int launch(int lm, const EnvLaunch& a) {
    const EnvKernel k = kernel_for(lm, a.action_dim, a.asym);
    if (!k) return TF_ERR_UNSUPPORTED;
    hipLaunchKernelGGL(k, dim3(a.grid), dim3(TF_WIDE == 2 ? NT_HELP : NT), 0, a.stream, a.d_params, a.sa, a.action);
    return TF_OK;
}

static int occupancy(int action_dim, bool asym) {
    const EnvKernel k = kernel_for(TF_LM_STEP_RAND, action_dim, asym);
    int n = -1;
    return (k && hipOccupancyMaxActiveBlocksPerMultiprocessor(&n, k, TF_WIDE == 2 ? NT_HELP : NT, 0) == hipSuccess) ? n : -1;
}

#define TF_CAT3_(a, b, c) a##b##_##c
#define TF_CAT3(a, b, c) TF_CAT3_(a, b, c)
EnvUnit TF_CAT3(TF_UNIT_PREFIX, TF_EXT, TF_WIDE) = {launch, occupancy};
