/* C ABI of the network-shape keys of the in-repo PPO (`network.mlp.activation`, `network.mlp.d2rl` of asymm.yaml, per network): the extended form of the
 * network walk in csrc/ppo_mlp_walk.hip (leibnizgym_amd/csrc/libtrifinger_ppo.so, gfx950).  Conventions as in include/trifinger_ppo.h: plain pointers and
 * sizes, every pointer DEVICE memory unless stated, `stream` a hipStream_t, 0 on success, -1 invalid argument, -2 / -3 a launch could not be set up / failed,
 * -4 declined (the shapes do not fit the walk).  The Python binding is leibnizgym_amd/ppo_kernels.py; tests/test_net_shape_gpu.py holds every entry point
 * against fp64 torch.
 *
 * Activation codes (TfpMlp.act[l], uniform per layer): 0 none and 1 ELU as ever (tfp_mlp_forward / tfp_mlp_backward know these two only and launch what they
 * always launched); the entry points below also take
 *     code  name      forward y(v), fp32, exp / log on v_exp_f32 / v_log_f32      derivative, formed from the SAVED OUTPUT y
 *     2     relu      max(v, 0)                                                   y > 0 ? 1 : 0
 *     3     tanh      sign(v) (1 - 2 / (exp(2 |v|) + 1)) from |v| = 0.625 on            1 - y^2
 *                     (saturates to +-1, no NaN), an odd polynomial below; the formula is
 *                     within 2.5e-7 relative of tanh (tests/test_net_shape.py), v_exp_f32 and
 *                     v_rcp_f32 add their 1 ulp each: intended, not pinned on the hardware
 *     4     sigmoid   1 / (1 + exp(-v))                                           y (1 - y)
 *     5     selu      L (v > 0 ? v : A (exp(v) - 1)), L = 1.0507009873554805,     y > 0 ? L : y + L A
 *                     A = 1.6732632423543772
 *     6     softplus  v > 20 ? v : log(1 + exp(v))   (torch: beta 1, threshold 20) 1 - exp(-y)
 * The backward walk reads the saved layer outputs and nothing else (no pre-activations are stored), which is why swish and gelu - not monotone, no
 * derivative from the output - have no code: a trainer that is asked for them runs on plain torch.
 *
 * d2rl (TfpNet.d2rl != 0; the skip width is dim[0]): with hidden outputs h_1 .. h_H (H = n_layers - 1) and input x,
 *     h_1 = act(x W_0^T + b_0),  h_{l+1} = act([h_l | x] W_l^T + b_l) for 1 <= l < H,  out = h_H W_H^T + b_H
 * i.e. W[l] is [dim[l+1], dim[l] + dim[0]] row-major for 1 <= l <= n_layers - 2 and [dim[l+1], dim[l]] otherwise: the hidden output first, x behind it (the
 * order of torch.cat([h, x], 1)); the output layer reads h_H alone; a network with one hidden layer has no wide layer at all.  With statistics the x that is
 * concatenated is the normalised one.  No gradient flows to x.
 *   forward:  y[l] for l <= n_layers - 3 receives the INPUT OPERAND of layer l + 1, [M, dim[l+1] + dim[0]] = [h_{l+1} | x] with the x columns in place
 *             (so that the weight gradient dZ_{l+1}^T [input | 1] is a plain product on it); y[n_layers - 2] is [M, dim[n_layers - 1]], the last one the
 *             network output.  Hidden ones may be NULL (not stored).
 *   backward: yin[l] as the forward stored them (row stride dim[l+1] + dim[0] for l <= n_layers - 3); the chain runs over the hidden part only,
 *             dZ_{l-1} = (dZ_l W_l[:, :dim[l]]) * act'(h_l); y[l] receives dZ_l as [M, dim[l+1]].
 * Limits: as the plain walk (n_layers <= 4, every dim <= 416); the two LDS operand buffers of the forward d2rl walk hold the wide rows (110 KB at
 * 41/113 -> 400 -> 200 -> 100), so that call may take up to a whole CU's 160 KiB - one workgroup per CU instead of two - and declines beyond; every other
 * call keeps the 80 KB of the plain walk.
 *
 * mean != NULL (forward only): the network reads clamp((x - mean) * inv_std, -clip, clip), formed where the rows are staged - TfpNorm's semantics, the bits of
 * the call without statistics on rows normalised beforehand.
 * tfp_net_fits: whether the SHAPES (n_layers, dim, d2rl; pointers are not looked at) fit the walk in the given direction, 0 or -4, without a launch.
 * For act in {0, 1}, d2rl == 0 and no statistics tfp_net_forward / tfp_net_backward return the bits of tfp_mlp_forward / tfp_mlp_backward. */
#ifndef TRIFINGER_PPO_NET_H
#define TRIFINGER_PPO_NET_H
#include "trifinger_ppo.h"
#ifdef __cplusplus
extern "C" {
#endif

#define TFP_ACT_NONE 0
#define TFP_ACT_ELU 1
#define TFP_ACT_RELU 2
#define TFP_ACT_TANH 3
#define TFP_ACT_SIGMOID 4
#define TFP_ACT_SELU 5
#define TFP_ACT_SOFTPLUS 6

typedef struct {
    TfpMlp mlp;               /* as for tfp_mlp_forward / tfp_mlp_backward, act[l] in 0 .. 6, widths of W / y / yin as described above */
    int32_t d2rl;             /* != 0: the input is concatenated behind every hidden output but the last */
    float clip;               /* > 0 when mean is given */
    const float* mean;        /* mean_f [dim[0]] or NULL */
    const float* inv_std;     /* inv_std_f [dim[0]] */
} TfpNet;
int tfp_net_forward(const TfpNet* nets, int32_t n_nets, int32_t M, void* stream);
int tfp_net_backward(const TfpNet* nets, int32_t n_nets, int32_t M, void* stream);
int tfp_net_fits(const TfpNet* nets, int32_t n_nets, int32_t backward);

#ifdef __cplusplus
}
#endif
#endif
