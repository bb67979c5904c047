// tf_launch.h - the seam between the C ABI host half (trifinger_hip.hip) and the fused step kernel (tf_env_kernels.hip).
//
// k_env<A, IS_RESET, ASYM, MODE, EXT, WIDE, HELP> (k_env_surf with the surface normal of the cube corners, k_env_dr the EXT 0 / 2 kernels with the base domain
// randomisation as a run-time flag) is split into translation units ("units"):
// tf_env_kernels.hip is compiled once per (EXT, WIDE) pair, once per (EXT, WIDE) pair of the surface-normal kernels and once per (EXT, WIDE) pair of the k_env_dr kernels
// (Makefile: UNITS), so that the nineteen units build in parallel (make -j: ~1 min instead of ~4 for one translation unit).  Each unit exports one EnvUnit object; the host picks one
// from its table (trifinger_hip.hip: unit_for).  Host side only: plain pointers and a stream.
#pragma once
#include <hip/hip_runtime.h>

#include "tf_params.h"

struct EnvLaunch {
    unsigned grid;               // workgroups = ceil(num_envs / 64)
    int action_dim;              // 9 or 18
    bool asym;                   // asymmetric observations: the states tile is emitted too
    const DevParams* d_params;   // device copy of the parameter block
    StepArgs sa;                 // what changes per launch, by value
    const float* action;         // [N][A] device tensor, or nullptr
    hipStream_t stream;
};

// which hooks of the reference step a launch performs (MODE of tf_roles.h)
enum { TF_LM_STEP = 0, TF_LM_STEP_RAND, TF_LM_RESET, TF_LM_RESETS, TF_LM_TORQUE, TF_LM_SIM, TF_LM_POST, TF_LM_FINISH };

struct EnvUnit {
    // enqueues launch mode lm: TF_OK (launch errors: hipGetLastError), or TF_ERR_UNSUPPORTED where the unit does not instantiate (lm, action_dim)
    int (*launch)(int lm, const EnvLaunch& a);
    // workgroups of the fused step (actions drawn in the launch) that fit a CU at once, as the HIP runtime computes it from registers and LDS; -1 on failure
    int (*occupancy)(int action_dim, bool asym);
};

// tf_unit_<EXT>_<WIDE>: WIDE 0 the 128-register kernels, 1 the 256-register ones, 2 those with helper wavefronts (the launches that simulate only:
// TF_LM_STEP, _STEP_RAND, _RESET, _SIM); tf_unit_s<EXT>_<WIDE>: with the surface normal of the cube corners (TfModel.cube_wall_surface, -DTF_SURF=1),
// the launches that simulate; tf_unit_d<EXT>_<WIDE>: EXT 0 / 2 with the base domain randomisation as a run-time flag (-DTF_DR=1; tf_unit_0_<WIDE> and
// tf_unit_2_<WIDE> are built without any: configs with dr_enable == 0).  Developer builds (-DTF_DEV_MIN) carry tf_unit_0_<WIDE> with the fused launches of A = 9 only.  (Not const: hipcc would
// emit a const one for the device as well, where its host functions do not exist.)
extern EnvUnit tf_unit_0_0, tf_unit_0_1, tf_unit_0_2, tf_unit_1_0, tf_unit_1_1, tf_unit_1_2, tf_unit_2_0, tf_unit_2_1, tf_unit_2_2;
extern EnvUnit tf_unit_s0_1, tf_unit_s0_2, tf_unit_s1_1, tf_unit_s1_2;
extern EnvUnit tf_unit_d0_0, tf_unit_d0_1, tf_unit_d0_2, tf_unit_d2_0, tf_unit_d2_1, tf_unit_d2_2;
