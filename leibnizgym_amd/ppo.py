"""Minimal asymmetric-actor-critic PPO for the TriFinger env (BASELINE config 5 when `rl_games` is absent).

Follows the agent configuration the reference ships for RL-Games (resources/config/rlg/asymm.yaml): continuous
A2C/PPO, actor MLP [400, 200, 100] ELU on `obs`, central value MLP [400, 200, 100] ELU on `states` (the defaults of `activation` / `d2rl`, below), state-independent
log-std (`fixed_sigma`), horizon `steps_num` 32, 4 mini-epochs, minibatch = num_envs, gamma 0.99, GAE tau 0.95,
actor lr 3e-4 adaptive on a KL threshold of 0.008, e_clip 0.2, reward scale 0.01, grad-norm 1.0, bounds loss 1e-4,
normalised advantages; the central value network has its OWN optimiser state (asymm.yaml:70-90): lr 5e-4 constant, its
own gradient-norm truncation, unweighted MSE loss (RL-Games drops `critic_coef` from the actor loss when a central value
network exists); initialisers as asymm.yaml:16-18,31-33,84-86 (`variance_scaling_initializer`: truncated normal with
variance scale / fan_in; biases zero).  `PPOConfig.from_rlg` reads all of it from the `rlg` tree of the launcher.
Checkpoints (`save` / `restore`: networks, optimiser moments, learning rates, frame and epoch counters), periodic and
best-so-far saving and a deterministic `play` mode mirror what the reference gets from RL-Games (`args.checkpoint`,
`args.play`, `save_frequency`, `save_best_after`).
`normalize_input` (the actor's `obs`) and `central_value_config.normalize_input` (the value network's `states`) are honoured by running moments
modelled on RL-Games' RunningMeanStd (`InputNorm`): fp64 {count, mean, M2} per input on the device, frozen for a whole epoch (rollout and every
minibatch of the update that follows read the same record), updated ONCE at the end of `update()` with the moments of the epoch's raw rollout buffer.
The value side of the tree: `clip_value` (the critic's, without a central value network) / `central_value_config.clip_value` (the central value network's)
clip the value loss around the value recorded in the rollout with the surrogate's e_clip - c_i = (v - ret)^2 inside the range or where it is the larger
term, (v_old + clamp(v - v_old, -e, e) - ret)^2 otherwise (`clipped_value_loss`: a `where`, so that the gradient is 2 (v - ret) or 0 and never halves on a
tie as torch.max's does; the kernel makes the same selection).  `normalize_value` keeps ONE more `InputNorm(dim=1)`, of the returns: the value network's
output is read as a NORMALISED value; rollout values enter GAE de-normalised, v = clamp(y, -5, 5) / inv_std_f + mean_f; the critic regresses on
ret_n = clamp((ret - mean_f) * inv_std_f, -5, 5) and clips around clamp(y_old, -5, 5), so c_loss and its clip range are in normalised units; advantages,
`mean_reward` and the KL statistic are what they were.  The record is frozen for the epoch like the input records and merged with them at the end of
`update()` (the same single all_gather) with the moments of the epoch's de-normalised returns buf["ret"], T n samples.  Deliberately NOT RL-Games here:
it merges values as well as returns, and before it normalises; its de-normalisation multiplies by sqrt(var + eps) where this divides by the published
inv_std_f (no third published quantity).  `act()` / `play()` neither read nor move the record; `ActorCritic.value_denorm` gives a value in reward units.
The shape of the networks follows the tree as well, per network (`params.network.mlp` for the actor, `central_value_config.network.mlp` for the central value
network; without one the critic takes the actor's keys).  RL-Games is not installed here, so the definitions in this module ARE the specification; they follow
RL-Games' network builder and D2RLNet as far as can be stated without it.  `activation`: relu, tanh, sigmoid, elu, selu, swish, gelu, softplus or None (`ACTIVATIONS`),
behind every hidden layer and never behind the output layer; anything else raises a ValueError naming the key.  `d2rl: True` (`D2RLMLP`): h_1 = act(x W_1^T + b_1),
h_l = act([h_{l-1} | x] W_l^T + b_l) with W_l [u_l, u_{l-1} + D0] (torch.cat([h, x], 1): the hidden output first), the output layer reads h_last alone, the
concatenated x is the normalised one, the initialisers see the real fan-in; `d2rl: False` keeps FusedMLP and the state-dict keys checkpoints have.  Which tier runs a network on a GPU - the
network walk, the per-layer kernels, plain torch - is decided in ppo_kernels.forward_nets / backward_nets and, once per trainer with ONE message, in
PPOTrainer.__init__ (`_fused_refusal`: swish, gelu and shapes the walk declines put the whole update on plain torch, as with `fused_kernels=False`).
`truncate_grads: False` / `central_value_config.truncate_grads: False`: no gradient-norm truncation for that optimiser.  `lr_schedule`: adaptive (the KL rule),
identity / None (the actor's rate stays; the KL statistic is still logged), linear (1e-6 + (learning_rate - 1e-6) * max(0, max_epochs - epoch) / max_epochs, set once
per epoch); the central value network's rate is constant throughout.  Not built and refused by name (ValueError): `fixed_sigma: False`, `mu_activation` /
`sigma_activation` other than None.
Episode ends (`params.config.episode_ends`, `params.config.value_bootstrap`; both off by default, and off is the reference bit for bit).  The reference's
`dones` is `reset_buf & goal_reset_buf`, which the shipped `success.activate: False` never sets although every env times out after `episode_length` steps
and is reset inside the next step launch: by default GAE never sees an episode end.  With `episode_ends` the trainer resolves the engine
behind the env once (evaluate.engine_of; an env without one is refused) and reads, after every env step t of a rollout, the engine's own buffers:
    end[t]  = float(reset_buf != 0)                                       the episode ended in this step; the reset happens at the start of the NEXT step
                                                                          launch, so the observation this step returned - and val[t + 1] - is the old episode's final state
    tout[t] = float(episode_length > 0 and steps >= episode_length)       the time limit was hit (it takes precedence over a termination on the same step)
    term[t] = end[t] * (1 - tout[t]) with `value_bootstrap`, end[t] without (RL-Games' default: a time-out counts as a terminal)
    w[t]    = 1 - end[t - 1],  w[0] = 1 - last_end                        0 for a STALE sample: the policy acted on the final state of an episode that had ended, the
                                                                          env was reset underneath it, reward and successor belong to the new episode
`last_end` is the end row of the final step of the previous rollout, kept by the trainer; zero after construction, at the end of `evaluate` and in `restore`.
GAE (`gae_with_ends`, the specification; float32, every operation rounded separately in the order written), t = T - 1 .. 0, last = 0:
    cont = 1 - end[t];  boot = 1 - term[t];  delta = rew[t] + gamma * val[t + 1] * boot - val[t];  last = delta + (gamma * tau) * cont * last
    adv[t] = last * w[t];  ret[t] = adv[t] + val[t]
so a stale sample has adv = 0 and ret = val (neutral for the returns' record of `normalize_value`), and with end = 0 the buffers hold the bits they hold with
the mode off (ret_n and v_old_n of `normalize_value` are formed from the masked ret as before).  Deliberately NOT RL-Games: its `value_bootstrap` adds gamma V of
the observation BEFORE the step, this uses V of the final state, which the buffers hold.  buf["done"] does not exist with the mode on: `end` replaces it.
Advantages are normalised over the samples with w = 1: mean = sum(w adv) / sum(w), std = sqrt(sum(w (adv - mean)^2) / (sum(w) - 1)),
adv_n = w (adv - mean) / (std + 1e-8) (`masked_advantage_norm`: torch, once per epoch, no host sync).  In the objective every per-sample term - surrogate,
value term, bounds term, KL statistic - and with it every per-sample gradient is multiplied by w_i; the divisor stays B, not sum(w) (the stale share is
1 / episode_length, 0.13 % at 750 steps; a constant divisor needs no pre-pass over the minibatch); the batch-independent entropy term is unchanged.  The input
records keep reading the whole rollout buffer (a stale observation is still a real observation).  `update()` reports `episodes_ended` = end.sum() of the epoch.
On the GPU: include/trifinger_ppo_episode.h - one launch in place of the reward launch (`rollout_flags`), one in place of GAE (`ppo_kernels.gae_ends`), the weighted
instantiation of the objective kernel reading (adv, w) interleaved, so that the gather still carries at most eight arrays.
Episode tracking (`params.config.track_episodes`, off by default; `games_to_track` and `score_to_win` are RL-Games' keys): what an EPISODE is worth, in the
statistics of every epoch.  The trainer resolves the engine once (an env without one is refused) and keeps an `evaluate.EpisodeTracker` on it.  After every env
step of a rollout, per env i, from the engine's buffers: r = reward[i] (raw, before reward_scale), rb = reset_buf[i] != 0, s = steps[i] (after a step the number
of steps taken in the current episode: s == 1 marks an episode's first step), and the cube and goal pose rows of `state`.  Per-env state `env_trk`, int32 [2][N],
zero at construction: the bits of the running float32 return, and `armed`.
    if s == 1: ret = r; armed = 1          else: ret = ret + r        (float32, step order)
    if rb:
        if armed:
            e_p, e_o, pos_ok, ori_ok, at_goal(rule): the device functions and tolerances of the evaluator (include/trifinger_ppo_eval.h)
            finite = ret, e_p, e_o and both quaternions finite
            finite:     EPISODES += 1; SUCCESS += at_goal; POS_OK += pos_ok; ORI_OK += ori_ok; TIMEOUT += (episode_length > 0 and s >= episode_length);
                        SUM_LENGTH += s; SUM_RETURN, SUM_POS_ERR, SUM_ORI_ERR += fixed point (2^16, 2^30, 2^28, the evaluator's clamps)
            not finite: NONFINITE += 1
        else: UNARMED += 1                 (an episode the tracker did not see from its first step: not counted)
        ret = 0; armed = 0
The accumulator is int64 [11] in that order - integers only, so the bits do not depend on the order of the workgroups or of the ranks.  The arming rule makes
the tracker self-synchronising: after `restore()` and at the end of `evaluate()` `env_trk` is zeroed and every partial episode is discarded, with no protocol.
On the GPU the tracker's launch (include/trifinger_ppo_track.h: `rollout_track`) stands where `rollout_reward` / `rollout_flags` stand and writes their bits: one
launch per step either way; otherwise the torch statement runs behind the step.  `update()` takes the epoch's vector - one SUM all-reduce with a process group,
counted in `n_track_allreduce` - and reads it with the other statistics at the end.  The WINDOW is the most recent epoch vectors with EPISODES > 0, newest
first, taken whole until their EPISODES reach `games_to_track` (8192 envs that time out in step: the last epoch in which episodes ended).  Reported:
`episode_return`, `episode_length`, `success_rate`, `pos_ok_rate`, `ori_ok_rate`, `timeout_rate`, `final_pos_err`, `final_ori_err` over the window (absent
before any episode has ended: no NaN goes into a log), `episodes` (the window's count), and the cumulative `episodes_total`, `episodes_nonfinite`,
`episodes_unarmed`.  `train()` then judges `<name>_best.pth` by `episode_return` and stops above `score_to_win` (its docstring).  Checkpoints carry the window and
the cumulative counts; one written without tracking restores with an empty window and best_reward = -inf (a reward per step and an episode return are different
units; likewise the other way round).  With the key off no tracker exists and every launch, buffer and statistic is what it was.
Symmetry augmentation (`params.config.symmetry_augmentation`, the project's own key like `episode_ends`; off by default).  The robot has an exact three-fold
symmetry - three copies of one finger at base yaw 0, -120 and -240 degrees, floor and boundary bodies of revolution, goals and resets from rotation-invariant
distributions, a reward built from distances - so the turn G of a sample by -120 degrees about z, with finger f renamed f + 1, is another sample of the same
MDP (leibnizgym_amd/symmetry.py states G on obs, states and actions as tables and `apply` as their torch expression).  With the key on every minibatch of B
rows is trained as 3B rows: rows [k B, (k + 1) B) hold G^k of obs / states and P^k of act and old_mu (the finger permutation), k = 0, 1, 2, and keep the
original sample's old_nlp, adv, ret, old_v and w; input statistics are applied AFTER the transform.  Surrogate, value, bounds and entropy terms run over all
3B rows with divisor 3B; the KL statistic, which drives the adaptive learning rate, runs over the FIRST B rows with divisor B - an asymmetric policy would
otherwise read as a large KL and the rate collapse to its floor.  Advantage normalisation, the input and return records, `mean_reward`, episode tracking and
checkpoints are untouched; the networks' shapes do not change, so checkpoints move freely between on and off.  Per epoch the statistics gain `symmetry_gap`:
the mean over i and k = 1, 2 of |P^-k mu[k B + i] - mu[i]| on the last minibatch's forward (torch, read with the epoch's other statistics; rank-local).  The
trainer resolves the engine once and refuses by name (ValueError): an env without an engine; an obs / states width other than 32 + A / obs + 72 (or 0) with
A in {9, 18}; an engine with `dr_enable` and a non-zero `dr_base_pos` or `dr_stage_pos` (such a scene is not invariant).  On the GPU: include/
trifinger_ppo_symmetry.h - the augmenting gather writes the three images in the ONE gather launch (`ppo_kernels.gather_rows_sym`), the objective takes
the KL row count (`tfp_ppo_loss_sym`); the step keeps its launch count on three times the rows.  With the key off no table is built and every launch, buffer
and statistic is what it was.
Training diagnostics (`params.config.diagnostics`, the project's own key; off by default, and off every launch, buffer, statistic and log line is what it
was).  THE RECORD is int64 [16] on the device (include/trifinger_ppo_diag.h; `D_*` below): integers and fixed-point sums, so its bits do not depend on the
order of the workgroups or of the ranks.  Every minibatch step adds to it: the objective slots 0-8 over its LIVE rows (w_i != 0 with `episode_ends`, the
original B rows with `symmetry_augmentation`; a row with a non-finite log-ratio or ratio counts in NONFINITE alone) - ROWS, CLIPPED (ratio outside 1 +- e_clip),
ZERO_GRAD (the surrogate's zero-gradient branch), VCLIPPED (the value term's clipped branch), MU_OUT (entries of mu beyond +-1.1), K3_SUM
(round(min(expm1(l) - l, 64) * 2^28), l = old_nlp - nlp), RATIO_MAX / RATIO_MIN (bit patterns) -, the optimiser slots 9-15 - STEPS, and per group TRUNC (its
coefficient max_norm / (norm + 1e-6) is < 1), GN_SUM (round(min(norm, 2^16) * 2^24)), GN_MAX, norm the pre-truncation gradient norm.  `diag_objective_statement`
and `diag_optimiser_statement` ARE the specification: float32 torch with the kernel's predicates in the kernel's order, what the torch path runs; on the GPU
the same two launches run as their DIAG instantiations (`tfp_ppo_loss_diag`, `tfp_clip_adam_diag`) - no quantity of the loss, of a gradient or of the update
is formed differently, no launch and no host sync is added to the minibatch loop.  `update()` takes and clears the record once per epoch - with a process
group slots 0-6 through ONE SUM all-reduce and (RATIO_MAX, -RATIO_MIN) through ONE MAX all-reduce, both counted in `n_diag_allreduce`; the norms are those of
the exchanged gradient, the same on every rank - and reports, a key whose divisor is 0 being absent: `clip_frac`, `zero_grad_frac`, `value_clip_frac` (with a
clipped value term), `mu_out_frac` = MU_OUT / (ROWS A), `approx_kl` = K3_SUM / 2^28 / ROWS, `ratio_max`, `ratio_min`, `nonfinite_rows`, `grad_norm` (the mean
over the steps), `grad_norm_max`, `grad_trunc_frac` and the same three with suffix `_value` for a central value network; and once per epoch in torch,
rank-local like `symmetry_gap`: `explained_variance` = 1 - Var(ret - val) / Var(ret) over the rollout's samples with w = 1 in reward units (ret - val is the
advantage estimate as GAE filed it; population variances; absent when Var(ret) = 0), `entropy` = sum_a (log sigma_a + 0.5 + 0.5 log 2 pi), `sigma_mean`.
`last_diag` keeps the epoch's record.  Checkpoints do not carry it.
Mixed precision (`params.config.mixed_precision`, RL-Games' key; off by default, and off every launch, buffer, statistic and bit is what it was).  With
bf16r(t) = t.to(bfloat16).to(float32) (round to nearest even) every Linear of both networks - hidden layers, the mu head, the value head - becomes
    forward   y  = bf16r(x) @ bf16r(W).T + b           products accumulated in fp32, the bias added in fp32
    backward  gx = bf16r(gy) @ bf16r(W);   gW = bf16r(gy).T @ bf16r(x);   gb = gy.sum(0)   (the un-rounded gy)
with the rounding straight-through for autograd: `_MixedLinear` IS the specification - what the CPU path and `fused_kernels=False` run and what the kernels
are held to.  Everything else stays fp32 and unchanged: master weights, biases and log_std; activations and their derivatives from the saved output; the
saved layer outputs and dZ in memory; input normalisation (formed in fp32, then rounded as the operand); the [h | x] operand of d2rl (rounded elementwise);
the objective, GAE, the records and Adam; checkpoints (the same keys: they move freely between on and off); the gradient exchange (fp32).  The rollout
forward, `act()`, `play()` and `evaluate()` use the same arithmetic as the update - otherwise the probability ratio of the first minibatch would not be 1.
Deliberately NOT RL-Games: it autocasts to fp16 under a gradient scaler; this build rounds to bf16, which has fp32's range, and needs no scaler (DESIGN.md
section 6).  On the GPU: include/trifinger_ppo_mixed.h - the network walk and the direct weight-gradient kernel with bf16 operands on
v_mfma_f32_16x16x32_bf16, packed in registers at the fragment (memory and LDS stay fp32).  There is no per-layer bf16 tier: shapes the bf16 walk declines put
the trainer on the torch statement, said once (`_fused_refusal`); a weight-gradient group the direct kernel declines at run time is formed as torch products of
the rounded operands.  ppo_kernels.n_calls counts the launches per entry point.

This is host-side training glue, NOT part of the measured hot path.  On a GPU the minibatch step runs on the hand-written kernels of
csrc/ppo_kernels.hip (leibnizgym_amd/ppo_kernels.py): one gather launch, the Linear / ELU layers on fp32 MFMA, the objective with all
its gradients in one launch, the chunk sums of the weight gradients in one launch, truncation + Adam over one flat buffer - about 30
launches per step, launched eagerly (a HIP-graph replay of the step existed in round 2; it was slower than eager launches and its
learning curves were never explained, so it was removed in round 3 - DESIGN.md section 8).
On the CPU (tests) and with `fused_kernels=False` the same step is plain torch.
Data parallelism: every rank owns an env shard (leibnizgym_amd.sharding) and its own rollout; gradients are averaged
with ONE all-reduce of a flat buffer per minibatch (`torch.distributed`, backend nccl = RCCL over xGMI on the GPU
box, gloo in the CPU tests) - ~1 MB, latency-bound, so a single fused collective is the right shape.
"""
import math
import os
from dataclasses import dataclass, field
from typing import List

import torch
import torch.nn as nn


@dataclass
class PPOConfig:
    units: List[int] = field(default_factory=lambda: [400, 200, 100])
    horizon: int = 32                 # steps_num
    mini_epochs: int = 4
    minibatches: int = 32             # minibatch_size = num_envs  ->  horizon minibatches per epoch
    gamma: float = 0.99
    tau: float = 0.95
    lr: float = 3e-4
    lr_value: float = 5e-4            # central_value_config.lr
    kl_threshold: float = 0.008       # lr_schedule: adaptive
    e_clip: float = 0.2
    critic_coef: float = 4.0
    reward_scale: float = 0.01
    grad_norm: float = 1.0
    bounds_loss_coef: float = 1e-4
    entropy_coef: float = 0.0
    normalize_advantage: bool = True
    value_mini_epochs: int = 0        # central_value_config.mini_epochs; 0 = as mini_epochs (they must be equal: one fused pass serves both)
    value_grad_norm: float = 1.0      # central_value_config.grad_norm
    mu_init_scale: float = 0.02       # network.space.continuous.mu_init (variance scaling)
    actor_init: str = "default"       # network.mlp.initializer.name
    value_init: str = "variance_scaling_initializer"   # central_value_config.network.mlp.initializer
    value_init_scale: float = 2.0
    save_frequency: int = 100
    save_best_after: int = 500
    max_epochs: int = 100000
    name: str = "trifinger"
    seed: int = 7
    fused_kernels: bool = True        # hand-written HIP kernel for the objective, forward and backward in one launch (GPU only)
    normalize_input: bool = False     # params.config.normalize_input: running mean / std of `obs` in front of the actor (and of a critic that reads obs)
    normalize_input_value: bool = False   # central_value_config.normalize_input: the same for `states` in front of the central value network
    clip_value: bool = False          # params.config.clip_value: the critic's value loss clipped around the rollout's value (no central value network)
    clip_value_central: bool = False  # central_value_config.clip_value: the same for the central value network (when there is one)
    normalize_value: bool = False     # params.config.normalize_value: running mean / std of the returns; the value network works in normalised units
    activation: str = "elu"           # params.network.mlp.activation: behind every hidden layer of the actor (ACTIVATIONS)
    value_activation: str = ""        # central_value_config.network.mlp.activation; "" = the actor's
    d2rl: bool = False                # params.network.mlp.d2rl: the input concatenated behind every hidden output but the last (D2RLMLP)
    value_d2rl: bool = False          # central_value_config.network.mlp.d2rl
    truncate_grads: bool = True       # params.config.truncate_grads: False = no gradient-norm truncation for the actor's optimiser
    value_truncate_grads: bool = True     # central_value_config.truncate_grads: the same for the central value network's
    lr_schedule: str = "adaptive"     # params.config.lr_schedule: adaptive | identity / None (constant) | linear (to 1e-6 at max_epochs, per epoch)
    episode_ends: bool = False        # params.config.episode_ends: GAE and the objective see the engine's episode ends (module docstring); off = the reference
    value_bootstrap: bool = False     # params.config.value_bootstrap (RL-Games' key): a time-out bootstraps from the final state's value; needs episode_ends
    track_episodes: bool = False      # params.config.track_episodes: episode returns, lengths and success in the statistics (module docstring); off = as before
    games_to_track: int = 100         # params.config.games_to_track (RL-Games' key): the episodes the reported window holds at least, once that many have ended
    score_to_win: float = float("inf")    # params.config.score_to_win (RL-Games' key): train() stops when episode_return exceeds it; needs track_episodes
    symmetry_augmentation: bool = False   # params.config.symmetry_augmentation: every minibatch with its two images under the robot's 120-degree turn (module docstring)
    diagnostics: bool = False         # params.config.diagnostics: clip fraction, approx_kl, gradient norms, explained variance in the statistics (module docstring)
    mixed_precision: bool = False     # params.config.mixed_precision (RL-Games' key): every Linear's products take bf16 operands, fp32 sums (module docstring)

    def __post_init__(self):
        if self.value_bootstrap and not self.episode_ends:
            raise ValueError("params.config.value_bootstrap: True needs params.config.episode_ends: True - without episode ends there is no time-out to "
                             "bootstrap from")

    @classmethod
    def from_rlg(cls, rlg: dict, num_envs: int = None, **overrides):
        """Hyper-parameters from the launcher's `rlg` tree (leibnizgym_amd/config.py:RLG_ASYMM, i.e. the reference's
        resources/config/rlg/asymm.yaml).  `minibatch_size` is given in samples there; the trainer counts minibatches per
        epoch: horizon * num_envs / minibatch_size."""
        p = rlg["params"]
        c, net = p["config"], p["network"]
        cv = c.get("central_value_config", {})
        # keys that are not built are refused by name, never ignored
        cont = net.get("space", {}).get("continuous", {})
        if not bool(cont.get("fixed_sigma", True)):
            raise ValueError("params.network.space.continuous.fixed_sigma: False (a state-dependent sigma head) is not built; the in-repo PPO keeps a "
                             "state-independent log-std")
        for key in ("mu_activation", "sigma_activation"):
            if cont.get(key, "None") not in (None, "None"):
                raise ValueError(f"params.network.space.continuous.{key}: {cont[key]!r} is not built; only None")
        kw = dict(units=list(net["mlp"]["units"]), horizon=int(c["steps_num"]), mini_epochs=int(c["mini_epochs"]),
                  gamma=float(c["gamma"]), tau=float(c["tau"]), lr=float(c["learning_rate"]),
                  kl_threshold=float(c["lr_threshold"]), e_clip=float(c["e_clip"]), critic_coef=float(c["critic_coef"]),
                  reward_scale=float(c["reward_shaper"]["scale_value"]), grad_norm=float(c["grad_norm"]),
                  bounds_loss_coef=float(c["bounds_loss_coef"]), entropy_coef=float(c["entropy_coef"]),
                  normalize_advantage=bool(c["normalize_advantage"]),
                  mu_init_scale=float(net["space"]["continuous"]["mu_init"].get("scale", 0.02)),
                  actor_init=str(net["mlp"]["initializer"]["name"]),
                  save_frequency=int(c.get("save_frequency", 100)), save_best_after=int(c.get("save_best_after", 500)),
                  max_epochs=int(c.get("max_epochs", 100000)), name=str(c.get("name", "trifinger")),
                  seed=int(rlg.get("seed", 7)), normalize_input=bool(c.get("normalize_input", False)),
                  clip_value=bool(c.get("clip_value", False)), normalize_value=bool(c.get("normalize_value", False)),
                  activation=activation_name(net["mlp"].get("activation", "elu"), "params.network.mlp.activation"),
                  d2rl=bool(net["mlp"].get("d2rl", False)), truncate_grads=bool(c.get("truncate_grads", True)),
                  lr_schedule=lr_schedule_name(c.get("lr_schedule", "adaptive")),
                  episode_ends=bool(c.get("episode_ends", False)), value_bootstrap=bool(c.get("value_bootstrap", False)),
                  track_episodes=bool(c.get("track_episodes", False)), games_to_track=int(c.get("games_to_track", 100)),
                  score_to_win=float(c.get("score_to_win", float("inf"))), symmetry_augmentation=bool(c.get("symmetry_augmentation", False)),
                  diagnostics=bool(c.get("diagnostics", False)), mixed_precision=bool(c.get("mixed_precision", False)))
        # without a central value network the critic takes the actor's keys
        kw.update(value_activation=kw["activation"], value_d2rl=kw["d2rl"], value_truncate_grads=kw["truncate_grads"])
        if cv:
            cmlp = cv["network"]["mlp"]
            kw.update(value_activation=activation_name(cmlp.get("activation", "elu"), "central_value_config.network.mlp.activation"),
                      value_d2rl=bool(cmlp.get("d2rl", False)), value_truncate_grads=bool(cv.get("truncate_grads", True)))
            init = cv["network"]["mlp"]["initializer"]
            kw.update(lr_value=float(cv["lr"]), value_mini_epochs=int(cv["mini_epochs"]),
                      value_grad_norm=float(cv["grad_norm"]), value_init=str(init["name"]),
                      value_init_scale=float(init.get("scale", 2.0)), normalize_input_value=bool(cv.get("normalize_input", False)),
                      clip_value_central=bool(cv.get("clip_value", False)))
        if num_envs:
            kw["minibatches"] = max(1, kw["horizon"] * int(num_envs) // int(c["minibatch_size"]))
        kw.update(overrides)
        return cls(**kw)


class _SplitKLinear(torch.autograd.Function):
    """y = x W^T + b with a weight gradient that is parallel over the batch: dW = dY^T X has a tiny output (e.g. 400 x 41)
    and the whole minibatch (8192) as its reduction dimension, which rocBLAS runs as ~80 workgroups of a 256-CU chip
    (55 us per call, the largest single item of the update).  Splitting the batch into S slices turns it into one batched
    GEMM with S times the workgroups plus a sum over S."""
    SLICES = 16

    @staticmethod
    def forward(ctx, x, w, b):
        ctx.save_for_backward(x, w)
        return torch.addmm(b, x, w.t())

    @staticmethod
    def backward(ctx, gy):
        x, w = ctx.saved_tensors
        gx = gy @ w if ctx.needs_input_grad[0] else None
        n = x.shape[0]
        s = _SplitKLinear.SLICES
        if n % s == 0 and n >= 64 * s:
            gw = torch.bmm(gy.view(s, n // s, -1).transpose(1, 2), x.view(s, n // s, -1)).sum(0)
        else:
            gw = gy.t() @ x
        return gx, gw, gy.sum(0)


def bf16r(t):
    """t rounded to bfloat16 (round to nearest even) and read back in its own type (float32 in the trainer; a float64 reference stays float64)"""
    return t.to(torch.bfloat16).to(t.dtype)


class _MixedLinear(torch.autograd.Function):
    """`mixed_precision`, THE STATEMENT of a Linear with bf16 operands (module docstring; include/trifinger_ppo_mixed.h): y = bf16r(x) bf16r(W)^T + b with the
    products accumulated in fp32 and the bias added in fp32; gx = bf16r(gy) bf16r(W), gW = bf16r(gy)^T bf16r(x), gb = the column sums of the UN-ROUNDED gy.
    The rounding is straight-through: no derivative of bf16r appears.  x may carry leading dimensions; they are rows."""

    @staticmethod
    def forward(ctx, x, w, b):
        xr, wr = bf16r(x), bf16r(w)
        ctx.save_for_backward(xr, wr)
        return torch.matmul(xr, wr.t()) + b

    @staticmethod
    def backward(ctx, gy):
        xr, wr = ctx.saved_tensors
        gr = bf16r(gy)
        gx = torch.matmul(gr, wr) if ctx.needs_input_grad[0] else None
        g2, x2 = gr.reshape(-1, gr.shape[-1]), xr.reshape(-1, xr.shape[-1])
        return gx, g2.t() @ x2, gy.reshape(-1, gy.shape[-1]).sum(0)


class SplitKLinear(nn.Linear):
    mixed = False              # `mixed_precision`: the layer is _MixedLinear (set by ActorCritic, a plain attribute: the state_dict keeps its keys)

    def forward(self, x):
        if self.mixed:
            return _MixedLinear.apply(x, self.weight, self.bias)
        if x.dim() == 2 and x.is_cuda and torch.is_grad_enabled():
            return _SplitKLinear.apply(x, self.weight, self.bias)
        return super().forward(x)


# `network.mlp.activation`: name -> (module, activation code of include/trifinger_ppo_net.h; -1: no kernel - swish and gelu are not monotone, their derivative
# cannot be formed from the saved output, which is all the backward walk reads).  RL-Games is not installed here: this table and D2RLMLP below ARE the
# specification, following RL-Games' network builder and D2RLNet as far as can be stated without it.
ACTIVATIONS = {"relu": (nn.ReLU, 2), "tanh": (nn.Tanh, 3), "sigmoid": (nn.Sigmoid, 4), "elu": (nn.ELU, 1), "selu": (nn.SELU, 5), "swish": (nn.SiLU, -1),
               "gelu": (nn.GELU, -1), "softplus": (nn.Softplus, 6), "None": (nn.Identity, 0)}
_ACT_CODE_OF = {mod: code for mod, code in ACTIVATIONS.values()}


def activation_name(name, key="network.mlp.activation"):
    """the canonical name of an activation key's value (None -> "None"); anything unknown raises a ValueError that names the key"""
    name = "None" if name is None else str(name)
    if name not in ACTIVATIONS:
        raise ValueError(f"{key}: unknown activation {name!r}; accepted: {', '.join(ACTIVATIONS)}")
    return name


def lr_schedule_name(name, key="params.config.lr_schedule"):
    name = "identity" if name in (None, "None", "identity") else str(name)
    if name not in ("adaptive", "identity", "linear"):
        raise ValueError(f"{key}: unknown schedule {name!r}; accepted: adaptive, identity, None, linear")
    return name


class FusedMLP(nn.Sequential):
    """Linear / activation stack (same modules and state-dict keys as the nn.Sequential it is).  With `mfma` set (the trainer does it on a
    GPU when `fused_kernels` is on) every layer runs on the hand-written fp32 MFMA kernels of csrc/ppo_kernels.hip: bias and ELU
    fused into the forward product, the ELU derivative formed in the operand loads of the two backward products, the bias gradient
    as an extra column of the weight-gradient product (those per-layer kernels know ELU only: any other activation runs as its torch module behind
    a plain product)."""
    mfma = False
    d2rl = False
    mixed = False              # `mixed_precision`: the Linear layers are _MixedLinear; on the hand-written path the walk with bf16 operands runs the network

    def layer_list(self):
        """[(weight, bias, act, grad_out)] of the Linear layers (a ppo_kernels.LayerList: it carries `d2rl`), act = the activation code behind the layer"""
        from .ppo_kernels import LayerList
        mods, out = list(self), LayerList()
        out.d2rl, out.mixed = self.d2rl, self.mixed
        other = False
        for i, m in enumerate(mods):
            if isinstance(m, nn.Linear):
                act = _ACT_CODE_OF.get(type(mods[i + 1]), 0) if i + 1 < len(mods) else 0
                other = other or act > 1 or act < 0
                out.append((m.weight, m.bias, act, getattr(m, "_grad_out", None)))
        out.ext = other or (self.d2rl and len(out) >= 3)            # what ppo_kernels.needs_net_walk() would find
        return out

    def forward(self, x):
        if self.mixed or not (self.mfma and x.is_cuda and x.dim() == 2 and x.dtype == torch.float32):
            return super().forward(x)                               # (mixed: the torch statement - the per-layer kernels are fp32, there is no bf16 tier of them)
        from .ppo_kernels import mfma_linear
        mods = list(self)
        i = 0
        while i < len(mods):
            m = mods[i]
            if isinstance(m, nn.Linear):
                act = i + 1 < len(mods) and isinstance(mods[i + 1], nn.ELU)
                x = mfma_linear(x, m.weight, m.bias, 1 if act else 0, getattr(m, "_grad_out", None) if torch.is_grad_enabled() else None)
                i += 2 if act else 1
            else:
                x = m(x)
                i += 1
        return x


class D2RLMLP(FusedMLP):
    """`network.mlp.d2rl: True`: h_1 = act(x W_1^T + b_1), h_l = act([h_{l-1} | x] W_l^T + b_l) for l >= 2 (W_l: [u_l, u_{l-1} + D0], the hidden output first
    and x behind it: torch.cat([h, x], dim=1)), the output layer reads h_last alone.  The same Sequential layout and state-dict keys as FusedMLP with wider
    hidden weights; the forward is plain torch (the trainer's fused path runs the network on the walk, ppo_kernels.mlp_forward_pair)."""
    d2rl = True

    def forward(self, x):
        lin = [m for m in self if isinstance(m, nn.Linear)]
        acts = [m for m in self if not isinstance(m, nn.Linear)]
        h = acts[0](lin[0](x))
        for l in range(1, len(lin) - 1):
            h = acts[l](lin[l](torch.cat([h, x], dim=-1)))
        return lin[-1](h)


def mlp(inp, units, out, activation="elu", d2rl=False):
    """the stack `network.mlp` describes: the activation behind every hidden layer, never behind the output layer; d2rl: D2RLMLP"""
    act = ACTIVATIONS[activation_name(activation)][0]
    layers, last = [], inp
    for i, u in enumerate(units):
        layers += [SplitKLinear(last + (inp if (d2rl and i > 0) else 0), u), act()]
        last = u
    layers.append(SplitKLinear(last, out))
    return (D2RLMLP if d2rl else FusedMLP)(*layers)


def variance_scaling_(w: torch.Tensor, scale: float) -> torch.Tensor:
    """RL-Games' `variance_scaling_initializer` (fan_in mode): normal with variance scale / fan_in, truncated at two
    standard deviations."""
    std = math.sqrt(scale / w.shape[1])
    return nn.init.trunc_normal_(w, mean=0.0, std=std, a=-2.0 * std, b=2.0 * std)


class InputNorm:
    """Running statistics of one network input (`normalize_input`), modelled on RL-Games' RunningMeanStd.
    State: ONE float64 vector `state` = [count, mean[D], M2[D]] on the device (M2 = sum of squared deviations; variance = M2 / count, population).
    Published: `mean_f` = float(mean), `inv_std_f` = float(1 / sqrt(M2 / count + 1e-5)), float32 [D], updated IN PLACE (the kernels keep their addresses);
    count 0 publishes mean 0 and variance 1.  `normalize(x)` = clamp((x - mean_f) * inv_std_f, -clip, clip) in float32 - the torch expression, which the
    kernels reproduce bit for bit.  Nothing here moves by itself: `merge` is called by the trainer once per epoch.
    `fused`: the merge and (for contiguous float32 rows on the GPU) the normaliser run on csrc/ppo_norm.hip; otherwise, and for anything the kernels
    decline, plain torch of the same semantics (the merge may differ from the kernel's in the last bits of the float64 record)."""
    EPS = 1e-5

    def __init__(self, dim, device, clip=5.0, fused=False):
        self.dim, self.clip, self.fused = int(dim), float(clip), bool(fused)
        self.state = torch.zeros(1 + 2 * self.dim, dtype=torch.float64, device=device)
        self.mean_f = torch.zeros(self.dim, dtype=torch.float32, device=device)
        self.inv_std_f = torch.empty(self.dim, dtype=torch.float32, device=device)
        self.publish()

    count = property(lambda self: self.state[0])
    mean = property(lambda self: self.state[1:1 + self.dim])
    m2 = property(lambda self: self.state[1 + self.dim:])

    def stats(self):
        """what the kernels take: (mean_f, inv_std_f, clip)"""
        return self.mean_f, self.inv_std_f, self.clip

    def publish(self):
        n = float(self.state[0])
        var = self.m2 / n if n > 0 else torch.ones_like(self.m2)
        self.mean_f.copy_(self.mean.float())
        self.inv_std_f.copy_((1.0 / torch.sqrt(var + self.EPS)).float())

    def normalize(self, x):
        if self.fused and x.is_cuda and x.dtype == torch.float32 and x.dim() == 2 and x.is_contiguous() and x.shape[1] == self.dim and not torch.is_grad_enabled():
            from . import ppo_kernels as pk
            return pk.normalize_rows(x, self.mean_f, self.inv_std_f, self.clip)
        return torch.clamp((x - self.mean_f) * self.inv_std_f, -self.clip, self.clip)

    @staticmethod
    def batch_record(x):
        """[count, mean, M2] of the rows of x, two passes in float64 (the reference form; the GPU path is ppo_kernels.moments)"""
        xd = x.reshape(-1, x.shape[-1]).double()
        mean = xd.mean(0)
        return torch.cat([torch.tensor([float(xd.shape[0])], dtype=torch.float64, device=x.device), mean, ((xd - mean) ** 2).sum(0)])

    def merge(self, records):
        """Chan's pairwise merge of the batch records `records` [k, 1 + 2 D] (float64), in the order given, into the running record; publishes.
        (torch form; the trainer's fused path merges all its inputs in one launch: ppo_kernels.norm_merge)"""
        D = self.dim
        na, ma, Ma = float(self.state[0]), self.mean.clone(), self.m2.clone()
        for r in records.reshape(-1, 1 + 2 * D):
            nb, mb, Mb = float(r[0]), r[1:1 + D], r[1 + D:]
            if nb <= 0:
                continue
            if na <= 0:
                na, ma, Ma = nb, mb.clone(), Mb.clone()
                continue
            n = na + nb
            delta = mb - ma
            ma = ma + delta * (nb / n)
            Ma = (Ma + Mb) + (delta * delta) * (na * nb / n)
            na = n
        self.state[0] = na
        self.state[1:1 + D] = ma
        self.state[1 + D:] = Ma
        self.publish()

    def state_dict(self):
        return {"state": self.state.clone(), "mean_f": self.mean_f.clone(), "inv_std_f": self.inv_std_f.clone()}

    def check_state_dict(self, sd, what, kind="input_norm"):
        for k, t in (("state", self.state), ("mean_f", self.mean_f), ("inv_std_f", self.inv_std_f)):
            if not isinstance(sd, dict) or k not in sd or tuple(sd[k].shape) != tuple(t.shape):
                raise ValueError(f"checkpoint {kind} record '{what}': '{k}' missing or of another width (this trainer: {self.dim} columns)")

    def load_state_dict(self, sd):
        self.state.copy_(sd["state"]); self.mean_f.copy_(sd["mean_f"]); self.inv_std_f.copy_(sd["inv_std_f"])   # the published bits as they were saved


def clipped_value_loss(v, ret, old_v, e):
    """per sample: (v - ret)^2 inside |v - old_v| <= e or where it is the larger term, (old_v + clamp(v - old_v, -e, e) - ret)^2 otherwise.  A `where`
    on purpose: the gradient is 2 (v - ret) or 0, the selection of tfp_ppo_loss_vclip (torch.max would halve it on a tie)"""
    lu = (v - ret).pow(2)
    lc = (old_v + (v - old_v).clamp(-e, e) - ret).pow(2)
    return torch.where(((v - old_v).abs() <= e) | (lu >= lc), lu, lc)


def denormalize_value(y, rec: "InputNorm"):
    """a normalised value -> reward units: clamp(y, -clip, clip) / inv_std_f + mean_f, float32, quotient and sum rounded separately"""
    return torch.clamp(y, -rec.clip, rec.clip) / rec.inv_std_f + rec.mean_f


def gae_spec(rew, val, gamma, tau, done=None, ends=None):
    """Generalised advantage estimation - the SPECIFICATION of the loop in both its modes, what the torch path runs and what ppo_kernels.gae_buffers reproduces bit
    for bit; float32, every operation rounded separately in the order written.  rew [T, n]; val [T + 1, n] in reward units; either `done` [T, n] (the
    public flag stops the estimate and the bootstrap alike) or `ends` = (end [T, n], tout [T, n], last_end [n], value_bootstrap) (`episode_ends`; the
    module docstring has the definitions; last_end: the end row of the final step of the previous rollout).  Returns adv and ret, and w with `ends`,
    each [T, n]."""
    T = rew.shape[0]
    if ends is None:
        stop, term, w = done, done, None
    else:
        stop, tout, last_end, value_bootstrap = ends
        term = stop * (1.0 - tout) if value_bootstrap else stop
        w = torch.cat([(1.0 - last_end).unsqueeze(0), 1.0 - stop[:T - 1]], dim=0)
    adv, last = torch.zeros_like(rew), torch.zeros_like(rew[0])
    for t in reversed(range(T)):
        cont = 1.0 - stop[t]
        boot = 1.0 - term[t]
        delta = rew[t] + gamma * val[t + 1] * boot - val[t]
        last = delta + gamma * tau * cont * last
        adv[t] = last if w is None else last * w[t]
    out = dict(adv=adv, ret=adv + val[:T])
    return out if w is None else dict(out, w=w)


def gae_with_ends(rew, end, tout, val, last_end, gamma, tau, value_bootstrap):
    """`gae_spec` with episode ends, as (adv, ret, w): the specification tfp_gae_ends names (include/trifinger_ppo_episode.h)"""
    out = gae_spec(rew, val, gamma, tau, ends=(end, tout, last_end, value_bootstrap))
    return out["adv"], out["ret"], out["w"]


def gae_torch(rew, val, gamma, tau, done=None, ends=None, vnorm=None):
    """ppo_kernels.gae_buffers in plain torch: the same arguments, the same named buffers, the same bits.  With `vnorm` (the returns' record) val is the value
    network's raw NORMALISED output y: GAE runs on v = clamp(y, -clip, clip) / inv_std_f + mean_f (`denormalize_value`), which replaces y as `val` among
    the buffers, next to v_old_n = clamp(y[:T], -clip, clip) and ret_n = clamp((ret - mean_f) * inv_std_f, -clip, clip)"""
    out = {}
    if vnorm is not None:
        out["v_old_n"] = torch.clamp(val[:rew.shape[0]], -vnorm.clip, vnorm.clip)
        out["val"] = val = denormalize_value(val, vnorm)
    out.update(gae_spec(rew, val, gamma, tau, done, ends))
    if vnorm is not None:
        out["ret_n"] = torch.clamp((out["ret"] - vnorm.mean_f) * vnorm.inv_std_f, -vnorm.clip, vnorm.clip)
    return out


def masked_advantage_norm(adv, w):
    """advantage normalisation over the samples with w = 1 (`episode_ends`): mean and unbiased std of those samples alone, stale samples leave as 0.
    Sums only - no boolean indexing, no host sync"""
    sw = w.sum()
    mean = (w * adv).sum() / sw
    std = torch.sqrt((w * (adv - mean) ** 2).sum() / (sw - 1.0))
    return w * (adv - mean) / (std + 1e-8)


# ---- training diagnostics (`params.config.diagnostics`; include/trifinger_ppo_diag.h has the record, the module docstring the keys) ----------------------
DIAG_N = 16
(D_ROWS, D_CLIPPED, D_ZERO_GRAD, D_VCLIPPED, D_MU_OUT, D_NONFINITE, D_K3_SUM, D_RATIO_MAX, D_RATIO_MIN, D_STEPS, D_TRUNC_A, D_TRUNC_V, D_GN_A_SUM, D_GN_V_SUM,
 D_GN_A_MAX, D_GN_V_MAX) = range(DIAG_N)
DIAG_RATIO_MIN_CLEAR = 0x7F800000                # the bit pattern of +inf: the cleared state of RATIO_MIN
DIAG_K3_SCALE, DIAG_K3_MAX, DIAG_GN_SCALE, DIAG_GN_MAX = 2.0 ** 28, 64.0, 2.0 ** 24, 2.0 ** 16


def new_diag_record(device):
    """a cleared record: int64 [DIAG_N], every slot 0 but RATIO_MIN"""
    rec = torch.zeros(DIAG_N, dtype=torch.int64, device=device)
    rec[D_RATIO_MIN] = DIAG_RATIO_MIN_CLEAR
    return rec


def _float_bits(x):
    """the bit pattern of a float32 tensor as int64 (of a non-negative float: an integer that orders as the float does)"""
    return x.float().contiguous().view(torch.int32).to(torch.int64)


def diag_objective_statement(l, ratio, adv, mu, e_clip, v=None, ret=None, old_v=None, w=None, kl_rows=None):
    """slots 0-8 of the record for ONE launch of the objective - the SPECIFICATION of what tfp_ppo_loss_diag adds, with the kernel's predicates in the
    kernel's order, on the tensors `_mb_backward` has: l = old_nlp - nlp [B], ratio = exp(l) [B], adv [B], mu [B, A], and with a clipped value term v, ret,
    old_v [B]; w [B] with `episode_ends`, kl_rows with `symmetry_augmentation`.  float32 in, int64 [DIAG_N] out (slots 9-15 zero, RATIO_MIN in its
    cleared state when no row is live); sums and masks only - no boolean indexing, no host sync.
    A row is LIVE when w_i != 0 (where w is given) and i < kl_rows (where given); a live row with a non-finite l or ratio counts in NONFINITE alone."""
    e = torch.as_tensor(e_clip, dtype=ratio.dtype, device=ratio.device)
    one = torch.ones((), dtype=ratio.dtype, device=ratio.device)
    lo, hi = one - e, one + e
    live = torch.ones_like(ratio, dtype=torch.bool)
    if w is not None:
        live = live & (w != 0)
    if kl_rows is not None:
        live = live & (torch.arange(ratio.numel(), device=ratio.device) < int(kl_rows))
    fin = torch.isfinite(l) & torch.isfinite(ratio)
    row, nonf = live & fin, live & ~fin
    s1, s2 = -adv * ratio, -adv * torch.minimum(torch.maximum(ratio, lo), hi)
    inside = (ratio >= lo) & (ratio <= hi)
    clipped = (ratio < lo) | (ratio > hi)
    zero = ~(inside | (s1 > s2))
    if old_v is not None:
        dlt = v - old_v
        lu, lc = (v - ret) ** 2, ((old_v + torch.minimum(torch.maximum(dlt, -e), e)) - ret) ** 2
        vclipped = ~(((dlt >= -e) & (dlt <= e)) | (lu >= lc))
    else:
        vclipped = torch.zeros_like(row)
    mu_out = ((mu > 1.1) | (mu < -1.1)).sum(-1)
    k3 = torch.round(torch.clamp(torch.expm1(l) - l, max=DIAG_K3_MAX) * DIAG_K3_SCALE)
    k3 = torch.where(row, k3, torch.zeros_like(k3)).to(torch.int64)          # a non-finite value never reaches the integer conversion
    bits = _float_bits(torch.where(row, ratio, torch.zeros_like(ratio)))
    cnt = lambda p: (p & row).sum()                                           # noqa: E731
    zero64 = torch.zeros((), dtype=torch.int64, device=ratio.device)
    return torch.stack([row.sum(), cnt(clipped), cnt(zero), cnt(vclipped), torch.where(row, mu_out, torch.zeros_like(mu_out)).sum(), nonf.sum(), k3.sum(),
                        bits.max(), torch.where(row, bits, torch.full_like(bits, DIAG_RATIO_MIN_CLEAR)).min()] + [zero64] * (DIAG_N - 9)).to(torch.int64)


def total_grad_norm(params):
    """the 2-norm of the gradients of `params` as torch.nn.utils.clip_grad_norm_ forms and returns it (for an optimiser that does not truncate)"""
    return torch.linalg.vector_norm(torch.stack([torch.linalg.vector_norm(p.grad) for p in params if p.grad is not None]))


def diag_optimiser_statement(norms, max_norms):
    """slots 9-15 of the record for ONE optimiser step - the SPECIFICATION of what tfp_clip_adam_diag adds.  `norms`: the pre-truncation gradient norm per
    optimiser group (one or two float32 scalars: what clip_grad_norm_ returns), `max_norms`: the group's max_norm, inf where it does not truncate.  A group is
    TRUNCATED when its coefficient max_norm / (norm + 1e-6) is < 1; the norm enters the sum as round(fmin(norm, 2^16) * 2^24) and the maximum by its bit
    pattern.  int64 [DIAG_N], slots 0-8 zero (RATIO_MIN too: `diag_merge` takes the minimum of slot 8 from objective statements alone)."""
    out = torch.zeros(DIAG_N, dtype=torch.int64, device=norms[0].device)
    out[D_STEPS] = 1
    for q, (nrm, mx) in enumerate(zip(norms, max_norms)):
        nrm = nrm.detach().float()
        coef = torch.as_tensor(float(mx), dtype=torch.float32, device=nrm.device) / (nrm + 1e-6)
        nb = torch.fmin(nrm, torch.as_tensor(DIAG_GN_MAX, dtype=torch.float32, device=nrm.device))
        out[D_TRUNC_A + q] = (coef < 1.0).to(torch.int64)
        out[D_GN_A_SUM + q] = torch.round(nb * DIAG_GN_SCALE).to(torch.int64)
        out[D_GN_A_MAX + q] = _float_bits(nb)
    return out


def diag_merge(rec, add, objective):
    """accumulate one statement into the record, in place, as the kernels do: sums add, maxima take the larger, RATIO_MIN the smaller"""
    if objective:
        rec[:D_RATIO_MAX] += add[:D_RATIO_MAX]
        rec[D_RATIO_MAX] = torch.maximum(rec[D_RATIO_MAX], add[D_RATIO_MAX])
        rec[D_RATIO_MIN] = torch.minimum(rec[D_RATIO_MIN], add[D_RATIO_MIN])
    else:
        rec[D_STEPS:D_GN_A_MAX] += add[D_STEPS:D_GN_A_MAX]
        rec[D_GN_A_MAX:] = torch.maximum(rec[D_GN_A_MAX:], add[D_GN_A_MAX:])


def _bits_float(b):
    import struct
    return struct.unpack("<f", struct.pack("<I", int(b) & 0xFFFFFFFF))[0]


def diagnostic_stats(vec, act_dim, value_clip, central):
    """the record of an epoch (a list of DIAG_N integers) as the statistics `update()` reports; a key whose divisor is 0 is absent (no NaN goes into a log)"""
    out = {"nonfinite_rows": int(vec[D_NONFINITE])}
    rows, steps = int(vec[D_ROWS]), int(vec[D_STEPS])
    if rows > 0:
        out["clip_frac"], out["zero_grad_frac"] = vec[D_CLIPPED] / rows, vec[D_ZERO_GRAD] / rows
        if value_clip:
            out["value_clip_frac"] = vec[D_VCLIPPED] / rows
        out["mu_out_frac"] = vec[D_MU_OUT] / (rows * int(act_dim))
        out["approx_kl"] = vec[D_K3_SUM] / DIAG_K3_SCALE / rows
        out["ratio_max"], out["ratio_min"] = _bits_float(vec[D_RATIO_MAX]), _bits_float(vec[D_RATIO_MIN])
    if steps > 0:
        for q, sfx in enumerate(("", "_value") if central else ("",)):
            out["grad_norm" + sfx] = vec[D_GN_A_SUM + q] / DIAG_GN_SCALE / steps
            out["grad_norm_max" + sfx] = _bits_float(vec[D_GN_A_MAX + q])
            out["grad_trunc_frac" + sfx] = vec[D_TRUNC_A + q] / steps
    return out


class ActorCritic(nn.Module):
    obs_norm = None            # InputNorm of `obs` / of `states` (plain attributes, not modules: the model's state_dict keeps its keys); set by the trainer
    state_norm = None
    value_norm = None          # InputNorm(1) of the returns (`normalize_value`): `value` then returns NORMALISED values, `value_denorm` reward units

    def __init__(self, obs_dim, state_dim, act_dim, units, cfg: "PPOConfig" = None):
        super().__init__()
        self.central = state_dim > 0
        a_act, a_d2rl = (cfg.activation, cfg.d2rl) if cfg is not None else ("elu", False)
        c_act, c_d2rl = ((cfg.value_activation or a_act, cfg.value_d2rl) if self.central else (a_act, a_d2rl)) if cfg is not None else ("elu", False)
        self.actor = mlp(obs_dim, units, act_dim, a_act, a_d2rl)
        self.critic = mlp(state_dim if state_dim > 0 else obs_dim, units, 1, c_act, c_d2rl)
        self.log_std = nn.Parameter(torch.zeros(act_dim))          # sigma_init const 0, fixed_sigma
        self.mixed = bool(cfg is not None and cfg.mixed_precision)
        if self.mixed:                                              # `mixed_precision`: every Linear of both networks, the heads included
            for net in (self.actor, self.critic):
                net.mixed = True
                for m in net:
                    if isinstance(m, nn.Linear):
                        m.mixed = True
        if cfg is not None:
            self.init_like_rl_games(cfg)

    def init_like_rl_games(self, cfg: "PPOConfig"):
        """asymm.yaml:12-18,31-33,84-86 through RL-Games' network builder: every Linear gets its MLP initialiser
        (`default` leaves torch's) and a zero bias; the mu head gets `mu_init`."""
        for net, kind, scale in ((self.actor, cfg.actor_init, 2.0), (self.critic, cfg.value_init if self.central else cfg.actor_init, cfg.value_init_scale)):
            for m in net:
                if isinstance(m, nn.Linear):
                    if kind == "variance_scaling_initializer":
                        variance_scaling_(m.weight.data, scale)
                    nn.init.zeros_(m.bias)
        variance_scaling_(self.actor[-1].weight.data, cfg.mu_init_scale)

    def actor_parameters(self):
        return list(self.actor.parameters()) + [self.log_std]

    def critic_parameters(self):
        return list(self.critic.parameters())

    def critic_norm(self):
        """the record in front of the critic: the central value network's own; without one the critic reads `obs` and shares the actor's"""
        return self.state_norm if self.central else self.obs_norm

    def _forward(self, xs, nets, runner=False):
        """the ONE place that answers, for a call: which record stands in front of which network of `nets` ("actor" / "critic", inputs `xs`), and whether the
        hand-written path may take it - every network on the MFMA kernels, float32 rows on the GPU, no autograd.  Returns the networks' outputs.
        `runner`: the hand-written path is ONE call of ppo_kernels.forward_nets - the walk, else the per-layer kernels (its docstring has the order) - on the
        raw rows with the records' statistics, no hidden output stored.  Otherwise, and whenever that path may not take the call, each network's own forward
        (FusedMLP.forward: the per-layer kernels, or torch) behind InputNorm.normalize"""
        recs = [self.obs_norm if n == "actor" else self.critic_norm() for n in nets]
        mods, x = [getattr(self, n) for n in nets], xs[0]
        # (`mixed_precision`: every call without autograd takes that ONE call - the walk with bf16 operands is the only kernel tier of the mode)
        if (runner or self.mixed) and all(m.mfma for m in mods) and x.is_cuda and x.dtype == torch.float32 and not torch.is_grad_enabled() and all(x.dim() == 2 for x in xs):
            from . import ppo_kernels as pk
            ys = pk.forward_nets([(x.contiguous(), m.layer_list()) for x, m in zip(xs, mods)], store_hidden=False,
                                 norms=[r.stats() if r is not None else None for r in recs])
            return [y[-1] for y in ys]
        return [m(r.normalize(x) if r is not None else x) for x, m, r in zip(xs, mods, recs)]

    def value(self, obs, states):
        return self._forward([states if self.central else obs], ["critic"])[0].squeeze(-1)

    def value_denorm(self, obs, states):
        """the value in reward units, whether or not the network works in normalised ones"""
        y = self.value(obs, states)
        return denormalize_value(y, self.value_norm) if self.value_norm is not None else y

    def dist(self, obs):
        mu = self._forward([obs], ["actor"])[0]
        return mu, self.log_std.expand_as(mu)

    def dist_and_value(self, obs, states):
        """(mu, log_std, value) of one batch: on the hand-written kernels and without autograd (the rollout) both networks are ONE launch of the walk,
        else layer k of the two is one (ppo_kernels.forward_nets)"""
        mu, v = self._forward([obs, states if self.central else obs], ["actor", "critic"], runner=True)
        return mu, self.log_std.expand_as(mu), v.squeeze(-1)

    def mean_action(self, obs):
        """the deterministic action: bit for bit the `mu` of dist_and_value.  On the hand-written kernels and without autograd it is ONE launch of the
        network walk with the actor alone (no hidden output stored, the actor's input record applied where the walk stages its rows); a shape the walk
        declines runs on the per-layer kernels; plain torch otherwise."""
        return self._forward([obs], ["actor"], runner=True)[0]


def neglogp(x, mu, log_std):
    return (0.5 * ((x - mu) / log_std.exp()).pow(2) + log_std + 0.5 * math.log(2 * math.pi)).sum(-1)


class PPOTrainer:
    """`env` is an RlGamesGpuEnvAdapter-like object: reset() -> {"obs","states"} or obs; step(a) -> (same, r, d, info).  Contract on the tensors it
    returns: with the attribute `buffers_stable_until_next_step = True` they may be the env's live buffers (valid until its next step / reset, on the
    calling stream) and the fused rollout reads them in place; without it every step's observation is cloned before it is used."""

    def __init__(self, env, obs_dim, state_dim, act_dim, cfg: PPOConfig = None, device="cuda:0", group=None):
        self.env, self.cfg, self.device, self.group = env, cfg or PPOConfig(), torch.device(device), group
        c = self.cfg
        if state_dim > 0 and c.value_mini_epochs not in (0, c.mini_epochs):
            raise ValueError("central_value_config.mini_epochs must equal mini_epochs: actor and central value network "
                             "are updated in one fused pass over the same minibatches")
        self.lr_schedule = lr_schedule_name(c.lr_schedule)
        torch.manual_seed(c.seed)              # identical initial weights on every rank (and a broadcast below)
        self.net = ActorCritic(obs_dim, state_dim, act_dim, c.units, c).to(self.device)
        # fused multi-tensor Adam on the GPU: the update is launch-bound (tiny MLPs), one kernel instead of ~60.
        # Two parameter groups = RL-Games' two optimisers: the actor's learning rate follows the KL schedule, the
        # central value network keeps central_value_config.lr; moments are per parameter, so nothing else is shared.
        fused = self.device.type == "cuda"
        lr_v = c.lr_value if self.net.central else c.lr
        groups = [{"params": self.net.actor_parameters(), "lr": c.lr},
                  {"params": self.net.critic_parameters(), "lr": lr_v}]
        kw = {"fused": True} if fused else {}
        self.opt = torch.optim.Adam(groups, eps=1e-8, **kw)
        self.lr = c.lr
        # The hand-written kernels serve a network the walk can run (module docstring): decided ONCE, here, with one message - otherwise the whole update
        # runs on plain torch, as with fused_kernels=False; no ELU kernel is ever applied to a network that asked for something else.  `fk` is the one
        # answer everything below takes: the objective kernel and the minibatch step, the MFMA layers, the records, the flat optimiser, the tracker
        fk = bool(fused and c.fused_kernels)
        self.torch_path_reason = self._fused_refusal() if fk else None
        if self.torch_path_reason:
            print(f"[ppo] {self.torch_path_reason}: this trainer runs on the plain torch path (as with fused_kernels=False)", flush=True)
            fk = False
        self.fused_loss = self.net.actor.mfma = self.net.critic.mfma = fk
        if fk:
            self._mb_backward = self._mb_backward_fused
        norm = lambda dim: InputNorm(dim, self.device, fused=fk)  # noqa: E731
        # which optimiser truncates its gradient norm (`truncate_grads` / central_value_config.truncate_grads; one optimiser without a central value network)
        self.trunc = (bool(c.truncate_grads), bool(c.value_truncate_grads if self.net.central else c.truncate_grads))
        # normalize_input / central_value_config.normalize_input: one record per normalised input, frozen during an epoch (module docstring)
        if c.normalize_input:
            self.net.obs_norm = norm(obs_dim)
        if c.normalize_input_value and self.net.central:
            self.net.state_norm = norm(state_dim)
        # the value side: which clip_value key applies depends on who is the critic; the returns' record exists only when normalize_value is on
        self.clip_v = bool(c.clip_value_central if self.net.central else c.clip_value)
        self.value_norm = None
        if c.normalize_value:
            self.value_norm = self.net.value_norm = norm(1)
        self.dist_on = False
        self.n_grad_allreduce = self.n_kl_allreduce = 0       # collectives issued so far (what a test of the distributed path counts)
        self.n_norm_allgather = 0
        self.n_eval_allreduce = 0
        self.last_recording = None                           # the episodes the last evaluate(record=...) harvested (leibnizgym_amd/record.py)
        rank = 0
        try:
            import torch.distributed as dist
            self.dist = dist
            # a process group that exists is used - also a world of one (`torch.distributed.run --nproc-per-node 1`): the collectives then run exactly
            # as in a multi-GPU job (that is how the RCCL path is exercised on a one-GPU box); without a group nothing is exchanged
            self.dist_on = dist.is_available() and dist.is_initialized()
        except Exception:
            self.dist = None
        if self.dist_on:                       # identical initial weights on every rank
            for p in self.net.parameters():
                self.dist.broadcast(p.data, src=0, group=group)
            rank = self.dist.get_rank(group)
        # GPU + fused kernels: truncation + Adam of both groups as two hand-written launches over one flat buffer
        self.flat_opt = None
        if fk:
            from .ppo_kernels import FlatClipAdam
            # no truncation = an infinite max_norm: the kernel's coefficient fminf(max_norm / (norm + 1e-6), 1) is then exactly 1 (inf / finite = inf; an
            # overflowed norm gives inf / inf = NaN, and fminf returns its other operand), and g * 1.0f is g
            inf = float("inf")
            gn0 = c.grad_norm if self.trunc[0] else inf
            if self.net.central:
                self.flat_opt = FlatClipAdam(self.net.actor_parameters(), self.net.critic_parameters(), c.lr, lr_v, gn0, c.value_grad_norm if self.trunc[1] else inf)
            else:
                self.flat_opt = FlatClipAdam(list(self.net.parameters()), [], c.lr, c.lr, gn0, gn0)
            for net in (self.net.actor, self.net.critic):      # the MFMA layers write dW / db straight into the flat gradient buffer
                for m in net:
                    if isinstance(m, nn.Linear):
                        m._grad_out = (self.flat_opt.grad_view(m.weight), self.flat_opt.grad_view(m.bias))
            # the minibatch step's view of the two networks, built ONCE: the parameters and their gradient slots stay where they are from here on
            self._layer_lists = (self.net.actor.layer_list(), self.net.critic.layer_list())
        # exploration noise and minibatch order must differ between ranks (the same env index of two shards would
        # otherwise receive the same noise sequence): re-seed with the rank after the weights are in place
        torch.manual_seed(c.seed + 7919 * rank)
        self.last = self._unpack(env.reset())
        # `episode_ends`: the engine behind the env, resolved ONCE (its ValueError for an env without one), its episode length read where `evaluate` reads
        # it (none = no time-outs), and the end row of the previous rollout's final step.  Off: none of it exists
        self.ends = bool(c.episode_ends)
        self.ends_engine, self.ends_ep_len, self.last_end = None, 0, None
        if self.ends:
            from .evaluate import engine_of
            self.ends_engine = engine_of(env)
            self.ends_ep_len = int(getattr(getattr(self.ends_engine, "cfg", None), "episode_length", 0) or 0)
            self.last_end = torch.zeros(self.last[0].shape[0], device=self.device)
        # `track_episodes`: the tracker on the engine behind the env (resolved once, like `episode_ends`: an env without one is refused by name), the
        # window of epoch vectors (integers, time order) and the cumulative counts.  Off: none of it exists
        self.tracker, self.track_window, self.track_totals = None, [], [0, 0, 0]       # totals: episodes, non-finite, unarmed
        self.n_track_allreduce = 0
        if c.track_episodes:
            from .evaluate import EpisodeTracker, engine_of
            eng = self.ends_engine if self.ends_engine is not None else engine_of(env)
            self.tracker = EpisodeTracker(eng, fused=bool(fk and eng.state.is_cuda))
        # `symmetry_augmentation`: the tables of the map, built ONCE for this env's widths (the refusals: module docstring).  Off: none of it exists
        self.sym = self._symmetry_tables(obs_dim, state_dim, act_dim, fk) if c.symmetry_augmentation else None
        self._sym_mu = None                                  # the last minibatch's mu [3B, A] (a reference, no launch): `symmetry_gap` is formed from it once per epoch
        # `diagnostics`: the record (int64 [DIAG_N] on the device), which the objective and the optimiser of every minibatch step add to and `update()` takes
        # and clears once per epoch.  Off: none of it exists
        self.diag = new_diag_record(self.device) if c.diagnostics else None
        self.n_diag_allreduce = 0
        self.last_diag = None                                # the last epoch's record as `update()` read it (a list of DIAG_N integers; reduced over the ranks)
        self.frames = 0
        self.epoch = 0
        self.last_info = {}
        self.best_reward = -float("inf")

    def _symmetry_tables(self, obs_dim, state_dim, act_dim, fused):
        """`symmetry_augmentation`: refuse by name what the map is not stated for, then the tables of G and G^2 for obs, states and actions on the trainer's
        device, and on the hand-written path their packed form per gathered array (symmetry.pack)"""
        from .evaluate import engine_of
        from . import symmetry as sy
        eng = engine_of(self.env)
        A = int(act_dim)
        if A not in (9, 18) or int(obs_dim) != 32 + A or int(state_dim) not in (0, int(obs_dim) + 72):
            raise ValueError(f"params.config.symmetry_augmentation: the map is stated for obs [32 + A], states [obs + 72] (or none) and A in (9, 18); this "
                             f"trainer has obs {obs_dim}, states {state_dim}, actions {act_dim}")
        ec = getattr(eng, "cfg", None)
        if ec is not None and int(getattr(ec, "dr_enable", 0)) and any(float(x) != 0.0 for x in list(ec.dr_base_pos) + list(ec.dr_stage_pos)):
            raise ValueError("params.config.symmetry_augmentation: domain_randomization.robot_base_position / stage_position are non-zero - a scene with a "
                             "shifted robot base or stage is not invariant under the 120-degree turn")
        tabs = sy.tables_to(sy.trifinger_symmetry(A, int(state_dim) > 0), self.device)
        if fused:
            pa = sy.pack(tabs["action"])
            tabs["packed"] = {"obs": sy.pack(tabs["obs"]), "act": pa, "old_mu": pa}
            if tabs["states"] is not None:
                tabs["packed"]["states"] = sy.pack(tabs["states"])
        return tabs

    def _symmetry_gap(self):
        """mean over i and k = 1, 2 of |P^-k mu[k B + i] - mu[i]| on the last minibatch's forward (P^-1 = P^2, P^-2 = P); a device scalar"""
        from .symmetry import apply
        mu = self._sym_mu
        B = mu.shape[0] // 3
        t = self.sym["action"]
        return 0.5 * ((apply(mu[B:2 * B], t[1]) - mu[:B]).abs().mean() + (apply(mu[2 * B:], t[0]) - mu[:B]).abs().mean())

    def _fused_refusal(self):
        """None, or why this network cannot run on the hand-written kernels: an activation without a kernel (swish, gelu), or a network only the extended
        walk runs (another activation than ELU, d2rl) whose shapes the walk declines - the per-layer fallback is ELU only"""
        from . import ppo_kernels as pk
        la, lc = self.net.actor.layer_list(), self.net.critic.layer_list()
        if any(l[2] == pk.ACT_NO_KERNEL for l in la + lc):
            return ("network.mlp.activation: swish / gelu have no kernel (not monotone: the derivative cannot be formed from the layer output, which is all the "
                    "backward walk keeps)")
        if (pk.needs_net_walk(la) or pk.needs_net_walk(lc)) and not (pk.net_fits([la, lc], False) and pk.net_fits([la, lc], True)):
            return ("network.mlp.activation / d2rl: the network walk declines these shapes (a layer wider than 416 or rows beyond the LDS of a CU) and the "
                    "per-layer kernels know ELU only")
        if self.cfg.mixed_precision and not (pk.net_fits([la, lc], False, mixed=True) and pk.net_fits([la, lc], True, mixed=True)):
            return ("params.config.mixed_precision: the network walk with bf16 operands declines these shapes (more than 4 layers, a layer wider than 416 or "
                    "rows beyond the LDS of a CU) and there is no per-layer bf16 tier")
        return None

    def _set_actor_lr(self, lr):
        """the actor's learning rate (the only one without a central value network) into whichever optimiser runs"""
        self.lr = float(lr)
        if self.flat_opt is not None:
            self.flat_opt.set_lr(0, self.lr)
            if not self.net.central:
                self.flat_opt.set_lr(1, self.lr)
        for g in (self.opt.param_groups[:1] if self.net.central else self.opt.param_groups):
            g["lr"] = self.lr

    def scheduled_lr(self, epoch):
        """`lr_schedule: linear`: 1e-6 + (learning_rate - 1e-6) * max(0, max_epochs - epoch) / max_epochs"""
        c = self.cfg
        return 1e-6 + (c.lr - 1e-6) * max(0, c.max_epochs - epoch) / c.max_epochs

    # ---- checkpoints (what RL-Games' save / restore / `args.checkpoint` give the reference launcher) ----
    def _optimizer_state(self):
        """Adam state in ONE format whichever optimiser runs (the flat hand-written one on a GPU, torch's otherwise): first and
        second moments per parameter NAME, the step counter, the two learning rates - so that a checkpoint written by one path
        restores into the other (CPU <-> GPU, fused_kernels on <-> off)."""
        names = {id(p): n for n, p in self.net.named_parameters()}
        m, v, step = {}, {}, 0.0
        if self.flat_opt is not None:
            fo = self.flat_opt
            for p, o in zip(fo.params, fo.offsets):
                m[names[id(p)]] = fo.m[o:o + p.numel()].view_as(p).clone()
                v[names[id(p)]] = fo.v[o:o + p.numel()].view_as(p).clone()
            step = float(fo.step_count[1].item())             # completed steps
            lrs = [float(x) for x in fo.lr.tolist()]
        else:
            for g in self.opt.param_groups:
                for p in g["params"]:
                    st = self.opt.state.get(p, {})
                    m[names[id(p)]] = st["exp_avg"].detach().clone() if "exp_avg" in st else torch.zeros_like(p)
                    v[names[id(p)]] = st["exp_avg_sq"].detach().clone() if "exp_avg_sq" in st else torch.zeros_like(p)
                    step = max(step, float(st["step"]) if "step" in st else 0.0)
            lrs = [float(g["lr"]) for g in self.opt.param_groups]
        return {"kind": "adam_per_parameter", "exp_avg": m, "exp_avg_sq": v, "step": step, "lrs": lrs}

    def _parse_optimizer_state(self, sd):
        """Any of the three optimiser-state formats -> (first moments by parameter name, second moments by name, step, learning rates),
        VALIDATED against this network (unknown names, wrong shapes, wrong total size raise ValueError) and without touching the
        trainer: restore() calls this before it overwrites a single weight.  Formats: 'adam_per_parameter' (what `_optimizer_state`
        writes), 'flat_clip_adam' (round 2, GPU path: the flat buffers of FlatClipAdam, every parameter padded to 4 floats, actor
        group then critic group for a central-value net, net.parameters() order otherwise) and torch.optim.Adam.state_dict() (round 2,
        CPU path: moments by parameter index in the order of the optimiser's groups)."""
        named = dict(self.net.named_parameters())
        names = {id(p): n for n, p in named.items()}
        kind = sd.get("kind")
        if kind == "adam_per_parameter":
            m, v, step, lrs = dict(sd["exp_avg"]), dict(sd["exp_avg_sq"]), float(sd["step"]), list(sd.get("lrs", []))
        elif kind == "flat_clip_adam":
            order = self.net.actor_parameters() + self.net.critic_parameters() if self.net.central else list(self.net.parameters())
            if sum((p.numel() + 3) & ~3 for p in order) != sd["m"].numel() or sd["v"].numel() != sd["m"].numel():
                raise ValueError("checkpoint optimizer state belongs to a network of another size")
            m, v, off = {}, {}, 0
            for p in order:
                m[names[id(p)]] = sd["m"][off:off + p.numel()].view_as(p)
                v[names[id(p)]] = sd["v"][off:off + p.numel()].view_as(p)
                off += (p.numel() + 3) & ~3
            step, lrs = float(sd["step"].item()), [float(x) for x in sd["lr"].tolist()]
        elif "state" in sd and "param_groups" in sd:
            order = [p for g in self.opt.param_groups for p in g["params"]]     # actor group (log_std last), then critic group
            n_ck = sum(len(g["params"]) for g in sd["param_groups"])
            if n_ck != len(order):
                raise ValueError(f"checkpoint optimizer state holds {n_ck} parameters, this network {len(order)}")
            st = sd["state"]
            m = {names[id(p)]: st[i]["exp_avg"] for i, p in enumerate(order) if i in st}
            v = {names[id(p)]: st[i]["exp_avg_sq"] for i, p in enumerate(order) if i in st}
            step = max([float(x["step"]) for x in st.values()] or [0.0])
            lrs = [float(g["lr"]) for g in sd["param_groups"]]
        else:
            raise ValueError(f"unknown optimizer state format (kind = {kind!r})")
        for which in (m, v):
            for n, t in which.items():
                if n not in named:
                    raise ValueError(f"checkpoint optimizer state names a parameter this network does not have: {n}")
                if tuple(t.shape) != tuple(named[n].shape):
                    raise ValueError(f"checkpoint optimizer moment of '{n}': shape {tuple(t.shape)}, parameter {tuple(named[n].shape)}")
        return m, v, step, lrs

    def _load_optimizer_state(self, sd, lr, parsed=None):
        """inverse of `_optimizer_state` (and of the two round-2 formats: `_parse_optimizer_state`)"""
        named = dict(self.net.named_parameters())
        m, v, step, lrs = parsed if parsed is not None else self._parse_optimizer_state(sd)
        lr_actor = float(lr) if lr is not None else (lrs[0] if lrs else self.lr)
        lr_value = lrs[1] if len(lrs) > 1 else None
        if self.flat_opt is not None:
            fo = self.flat_opt
            names = {id(p): n for n, p in named.items()}
            fo.m.zero_(); fo.v.zero_()
            for p, o in zip(fo.params, fo.offsets):                  # every moment into its own (padded) slot
                n = names[id(p)]
                if n in m:
                    fo.m[o:o + p.numel()].copy_(m[n].reshape(-1).to(fo.m.device))
                    fo.v[o:o + p.numel()].copy_(v[n].reshape(-1).to(fo.v.device))
            fo._set_step(torch.tensor([float(step)]))
            fo.set_lr(0, lr_actor)
            if lr_value is not None:
                fo.set_lr(1, lr_value if self.net.central else lr_actor)
        else:
            fused = self.device.type == "cuda"
            for gi, g in enumerate(self.opt.param_groups):
                for p in g["params"]:
                    n = next(k for k, q in named.items() if q is p)
                    self.opt.state[p] = {
                        "step": torch.tensor(step, dtype=torch.float32, device=p.device if fused else "cpu"),
                        "exp_avg": (m[n].to(p.device).clone().view_as(p) if n in m else torch.zeros_like(p)),
                        "exp_avg_sq": (v[n].to(p.device).clone().view_as(p) if n in v else torch.zeros_like(p))}
                g["lr"] = lr_actor if (gi == 0 or not self.net.central) else (lr_value if lr_value is not None else g["lr"])

    def _norm_records(self):
        """{"obs": InputNorm, "states": InputNorm} of the inputs that are normalised (empty: normalisation is off)"""
        out = {}
        if self.net.obs_norm is not None:
            out["obs"] = self.net.obs_norm
        if self.net.state_norm is not None:
            out["states"] = self.net.state_norm
        return out

    def state_dict(self):
        sd = {"model": self.net.state_dict(), "optimizer": self._optimizer_state(), "lr": self.lr, "frames": self.frames,
              "epoch": self.epoch, "best_reward": self.best_reward, "config": dict(self.cfg.__dict__)}
        recs = self._norm_records()
        if recs:                                                     # the key exists only when normalisation is on
            sd["input_norm"] = {k: r.state_dict() for k, r in recs.items()}
        if self.value_norm is not None:                              # likewise
            sd["value_norm"] = self.value_norm.state_dict()
        if self.tracker is not None:                                 # likewise: the window (integer vectors, time order) and the cumulative counts
            sd["track"] = {"window": [list(v) for v in self.track_window], "totals": list(self.track_totals)}
        return sd

    def save(self, path: str):
        os.makedirs(os.path.dirname(os.path.abspath(path)) or ".", exist_ok=True)
        torch.save(self.state_dict(), path)
        return path

    def restore(self, path: str):
        ck = torch.load(path, map_location=self.device, weights_only=False)
        parsed = None
        mine = self.net.state_dict()                                 # validate EVERYTHING before anything is overwritten
        for k, t in mine.items():
            if k not in ck["model"] or tuple(ck["model"][k].shape) != tuple(t.shape):
                raise ValueError(f"checkpoint model entry '{k}' missing or of another shape")
        recs, ck_recs = self._norm_records(), ck.get("input_norm") or {}
        if sorted(recs) != sorted(ck_recs):
            raise ValueError(f"checkpoint normalises {sorted(ck_recs) or 'no input'}, this trainer {sorted(recs) or 'no input'} "
                             "(normalize_input / central_value_config.normalize_input differ)")
        for k, r in recs.items():
            r.check_state_dict(ck_recs[k], k)
        if (ck.get("value_norm") is not None) != (self.value_norm is not None):
            raise ValueError(f"checkpoint {'normalises' if ck.get('value_norm') is not None else 'does not normalise'} the value, this trainer "
                             f"{'does' if self.value_norm is not None else 'does not'} (normalize_value differs)")
        if self.value_norm is not None:
            self.value_norm.check_state_dict(ck["value_norm"], "returns", kind="value_norm")
        if "optimizer" in ck:
            parsed = self._parse_optimizer_state(ck["optimizer"])
        with torch.no_grad():                                        # in place: the parameters may be views of a flat buffer
            for k, v in self.net.state_dict().items():
                v.copy_(ck["model"][k])
            for k, r in recs.items():
                r.load_state_dict(ck_recs[k])
            if self.value_norm is not None:
                self.value_norm.load_state_dict(ck["value_norm"])
            if "optimizer" in ck:
                self._load_optimizer_state(ck["optimizer"], ck.get("lr"), parsed)
        self.lr = float(ck.get("lr", self.lr))
        self.frames, self.epoch = int(ck.get("frames", 0)), int(ck.get("epoch", 0))
        self.best_reward = float(ck.get("best_reward", -float("inf")))
        if self.last_end is not None:
            self.last_end.zero_()
        trk = ck.get("track")
        if (trk is not None) != (self.tracker is not None):          # best_reward is an episode return with tracking and a reward per step without: the
            self.best_reward = -float("inf")                         # units differ, the best so far starts again
        if self.tracker is not None:
            self.tracker.reset_envs()                                # the env is where it is, not where the checkpoint's episodes were: they re-arm at their next first step
            self.tracker.acc.zero_()
            self.track_window = [[int(x) for x in v] for v in trk["window"]] if trk is not None else []
            self.track_totals = [int(x) for x in trk["totals"]] if trk is not None else [0, 0, 0]
        return ck

    @torch.no_grad()
    def act(self, obs, deterministic=True):
        mu, ls = self.net.dist(obs)
        return mu if deterministic else mu + ls.exp() * torch.randn_like(mu)

    @torch.no_grad()
    def play(self, steps: int, deterministic=True):
        """`args.play`: roll the policy without learning; returns the mean reward per step and the last info dict."""
        obs, _ = self.last
        total, info = 0.0, {}
        for _ in range(steps):
            out, r, _, extra = self.env.step(self.act(obs, deterministic))
            obs, states = self._unpack(out)
            total += float(r.mean())
            if isinstance(extra, (list, tuple)) and len(extra) > 1 and isinstance(extra[1], dict):
                info = extra[1]
        self.last = (obs, states)
        return total / max(steps, 1), info

    @torch.no_grad()
    def evaluate(self, episodes_per_env=1, deterministic=True, max_steps=None, pos_tol=None, ori_tol=None, check_every=32, record=None):
        """Episode statistics of the current policy over `episodes_per_env` whole episodes of every env (leibnizgym_amd/evaluate.py: EpisodeStats, whose
        result dict this returns, with the number of env steps taken as "steps").  The env is reset first - every env starts at step 0, there are no
        partial episodes -, then stepped with the deterministic action (ActorCritic.mean_action) or with mu + sigma * randn, the statistics updated on the
        device behind every step.  The host reads ONE counter every `check_every` steps and stops when every env has finished its episodes, at
        episodes_per_env * episode_length steps (no episode is longer) or at `max_steps`, whichever comes first; an env without an episode length
        needs `max_steps` (ValueError).  Tolerances default to the env's.  With a process group the accumulators of all ranks are summed in one
        all-reduce (`n_eval_allreduce` counts them) and every rank returns the statistics of the whole population.
        Nothing of the trainer moves: no weight, no normalisation record, no counter (frames, epoch).  The env does: at the end it is reset again and
        `self.last` is that fresh observation - TRAINING CONTINUES FROM A RESET, not from where the last rollout stopped.
        `record`: None, or a dict (`select`, `every`, `length`, `watch`, `max_episodes`) - a flight recorder (leibnizgym_amd/record.py: EpisodeRecorder,
        with the evaluation's tolerances) is updated behind the statistics, one more launch per step and no host synchronisation; at the end this rank's
        selected episodes (at most `max_episodes`, ascending env id) are harvested into `self.last_recording` and the result gains
        "episodes_recorded", their number.  With None no recorder exists: every launch, buffer and result key is as without the argument."""
        from .evaluate import EpisodeStats, engine_of
        k = int(episodes_per_env)
        if k < 1:
            raise ValueError(f"episodes_per_env = {episodes_per_env}: need at least one episode per env")
        eng = engine_of(self.env)
        ep_len = int(getattr(getattr(eng, "cfg", None), "episode_length", 0) or 0)
        if ep_len <= 0 and max_steps is None:
            raise ValueError("this env has no episode length (its episodes never time out): evaluate() needs max_steps")
        limit = k * ep_len if ep_len > 0 else int(max_steps)
        if max_steps is not None:
            limit = min(limit, int(max_steps))
        stats = EpisodeStats(eng, pos_tol=pos_tol, ori_tol=ori_tol, max_episodes_per_env=k)
        recorder = None
        if record is not None:
            from .record import EpisodeRecorder
            unknown = sorted(set(record) - {"select", "every", "length", "watch", "max_episodes"})
            if unknown:
                raise ValueError(f"record: unknown key(s) {unknown}; known: select, every, length, watch, max_episodes")
            length = record.get("length")
            if length is None and ep_len <= 0:
                length = limit // max(1, int(record.get("every", 1))) + 2          # no episode length: the ring takes the whole evaluation
            recorder = EpisodeRecorder(eng, select=record.get("select", "failure"), every=record.get("every", 1), length=length,
                                       watch=record.get("watch"), pos_tol=pos_tol, ori_tol=ori_tol)
        live = getattr(self.env, "buffers_stable_until_next_step", False)      # the observation is consumed before the next step overwrites it

        def obs_of(o):
            o = o["obs"] if isinstance(o, dict) else o
            return o if live else o.clone()
        obs = obs_of(self.env.reset())
        sigma = self.net.log_std.detach().exp()
        every, steps = max(1, int(check_every)), 0
        while steps < limit:
            mu = self.net.mean_action(obs)
            out = self.env.step(mu if deterministic else mu + sigma * torch.randn_like(mu))[0]
            stats.update()
            if recorder is not None:
                recorder.update()
            obs = obs_of(out)
            steps += 1
            if steps % every == 0 and steps < limit and stats.envs_complete() == stats.num_envs:
                break
        if self.dist_on:
            stats.merge(self.group)
            self.n_eval_allreduce += 1
        res = stats.result()
        res["steps"] = steps
        if recorder is not None:
            self.last_recording = recorder.take(record.get("max_episodes"))
            res["episodes_recorded"] = len(self.last_recording)
        self.last = self._unpack(self.env.reset())
        if self.last_end is not None:                        # every env starts a fresh episode: no sample of the next rollout is stale
            self.last_end.zero_()
        if self.tracker is not None:                         # the evaluation's episodes are not the training run's: every env re-arms at its next first step
            self.tracker.reset_envs()
        return res

    @staticmethod
    def _unpack(o):
        if isinstance(o, dict):
            return o["obs"].clone(), o["states"].clone()
        return o.clone(), None

    @torch.no_grad()
    def rollout(self):
        c, T = self.cfg, self.cfg.horizon
        obs, states = self.last
        n = obs.shape[0]
        dev = self.device
        # with the hand-written kernels the bookkeeping of a step is two launches (ppo_kernels.rollout_record / rollout_reward) and the advantage
        # estimate one (ppo_kernels.gae_buffers) instead of ~25 + 8 T elementwise launches; same arithmetic, same random numbers (torch.randn_like)
        fused, pk = self.fused_loss and obs.is_cuda and obs.dtype == torch.float32, None
        if fused:
            from . import ppo_kernels as pk
        A = self.net.log_std.numel()
        sigma = self.net.log_std.detach().exp()              # constant over the rollout
        buf = dict(obs=torch.zeros(T, n, obs.shape[1], device=dev),
                   states=torch.zeros(T, n, states.shape[1], device=dev) if states is not None else None,
                   act=torch.zeros(T, n, A, device=dev), nlp=torch.zeros(T, n, device=dev), val=torch.zeros(T + 1, n, device=dev),
                   rew=torch.zeros(T, n, device=dev), mu=torch.zeros(T, n, A, device=dev))
        if self.ends:                                        # `end` replaces `done` (module docstring)
            buf["end"], buf["tout"] = torch.zeros(T, n, device=dev), torch.zeros(T, n, device=dev)
        else:
            buf["done"] = torch.zeros(T, n, device=dev)
        for t in range(T):
            mu, ls, val_t = self.net.dist_and_value(obs, states)
            if fused:
                a = pk.rollout_record(obs, states, mu, self.net.log_std, sigma, torch.randn_like(mu), val_t, buf, t)
            else:
                a = mu + ls.exp() * torch.randn_like(mu)
                buf["obs"][t], buf["act"][t], buf["mu"][t] = obs, a, mu
                if states is not None:
                    buf["states"][t] = states
                buf["nlp"][t] = neglogp(a, mu, ls)
                buf["val"][t] = val_t
            out, r, d, extra = self.env.step(a)
            last_step = t == T - 1
            # an env that DECLARES its buffers stable until its next step (`buffers_stable_until_next_step`: RlGamesGpuEnvAdapter hands out the
            # engine's own tensors) is read in place - they are filed above before the next step overwrites them, only what outlives the loop is cloned;
            # any other env gets a snapshot per step (it may refresh its observation asynchronously or on another stream)
            live = fused and not last_step and getattr(self.env, "buffers_stable_until_next_step", False)
            obs, states = ((out["obs"], out["states"]) if isinstance(out, dict) else (out, None)) if live else self._unpack(out)
            if isinstance(extra, (list, tuple)) and len(extra) > 1 and isinstance(extra[1], dict):
                self.last_info = extra[1]                   # RL-Games convention: [[], info] (direct logging from the env)
            self._file_step(pk, buf, t, r, d)
        buf["val"][T] = self.net.value(obs, states)
        self.last = (obs, states)
        self._advantages(pk, buf)
        self.frames += T * n
        return buf

    def _file_step(self, pk, buf, t, r, d):
        """file what env step t returned into slot t of the rollout buffers: rew = r * reward_scale and the public `done` as a float or, with
        `episode_ends`, `end` / `tout` from the engine's own buffers behind the step (stable until its next step, read in place).  ONE launch where the
        kernels can read the tensors (ppo_kernels.rollout_reward / rollout_flags), torch expressions otherwise.  `track_episodes`: the tracker's launch
        stands where that launch stands - one launch either way - when it reads the very reward the env returned; otherwise its own update() follows.
        `pk`: ppo_kernels on the hand-written path, None on the torch path"""
        c, dev, ends, eng, trk = self.cfg, self.device, self.ends, self.ends_engine, self.tracker
        fused = pk is not None and pk.readable(r, r, torch.float32) and (
            (pk.readable(eng.reset_buf, r, torch.bool, torch.uint8) and pk.readable(eng.steps, r, torch.int64)) if ends
            else pk.readable(d, r, torch.bool, torch.uint8))
        tracked = bool(fused and trk is not None and trk.fused and r.data_ptr() == trk.engine.reward.data_ptr() and dev == r.device)
        if tracked and ends:
            trk.step_fused(c.reward_scale, buf["rew"][t], end_t=buf["end"][t], tout_t=buf["tout"][t])
        elif tracked:
            trk.step_fused(c.reward_scale, buf["rew"][t], done=d, done_t=buf["done"][t])
        elif fused and ends:
            pk.rollout_flags(r, eng.reset_buf, eng.steps, c.reward_scale, self.ends_ep_len, buf["rew"][t], buf["end"][t], buf["tout"][t])
        elif fused:
            pk.rollout_reward(r, d, c.reward_scale, buf["rew"][t], buf["done"][t])
        else:
            buf["rew"][t] = r.to(dev) * c.reward_scale
            if ends:
                buf["end"][t] = (eng.reset_buf != 0).to(dev).float()
                if self.ends_ep_len > 0:
                    buf["tout"][t] = (eng.steps >= self.ends_ep_len).to(dev).float()
            else:
                buf["done"][t] = d.to(dev).float()
        if trk is not None and not tracked:                 # the tracker's launch could not stand in: its own update (the torch statement on CPU tensors)
            trk.update()

    def _advantages(self, pk, buf):
        """the advantage pass over a filled rollout: adv and ret, w with `episode_ends`, ret_n and v_old_n with `normalize_value` - ONE launch
        (ppo_kernels.gae_buffers; buf["val"] keeps the network's raw normalised output y there) or the torch statement (`gae_torch`, which replaces it by v)"""
        c = self.cfg
        mode = dict(ends=(buf["end"], buf["tout"], self.last_end, c.value_bootstrap)) if self.ends else dict(done=buf["done"])
        buf.update((pk.gae_buffers if pk is not None else gae_torch)(buf["rew"], buf["val"], c.gamma, c.tau, vnorm=self.value_norm, **mode))
        if self.ends:
            self.last_end = buf["end"][c.horizon - 1].clone()       # w[0] of the next rollout

    # ---- one minibatch step, split at the gradient exchange ----
    def _mb_backward(self, d, idx, acc):
        """gather the minibatch, forward, losses, backward; returns nothing - gradients sit in p.grad, the running
        sums of the logged quantities in `acc` (device tensors, no host sync).  The torch statement; a trainer on the hand-written kernels binds
        `_mb_backward_fused` under this name at construction"""
        c = self.cfg
        if self.sym is not None:                   # the 3B minibatch (module docstring); everything below reads it through `d` and `idx` as before
            d, idx, B = self._sym_minibatch(d, idx), slice(None), idx.numel()
        obs = d["obs"][idx]
        mu, ls = self.net.dist(obs)
        nlp = neglogp(d["act"][idx], mu, ls)
        ratio = (d["old_nlp"][idx] - nlp).exp()
        a = d["adv"][idx]
        # `episode_ends`: every per-sample term times w_i, the divisor stays B (module docstring); off: the expressions as they were
        w = d["w"][idx] if self.ends else None
        wmean = (lambda x: (w * x).mean()) if self.ends else (lambda x: x.mean())
        a_loss = wmean(torch.max(-a * ratio, -a * ratio.clamp(1 - c.e_clip, 1 + c.e_clip)))
        v = self.net.value(obs, d["states"][idx] if d["states"] is not None else None)
        if self.clip_v:
            c_loss = wmean(clipped_value_loss(v, d["ret"][idx], d["old_v"][idx], c.e_clip))
        else:
            c_loss = wmean((v - d["ret"][idx]).pow(2))
        b_loss = wmean(((mu - 1.1).clamp(min=0).pow(2) + (-1.1 - mu).clamp(min=0).pow(2)).sum(-1))
        ent = (ls + 0.5 + 0.5 * math.log(2 * math.pi)).sum(-1).mean()
        # with a central value network RL-Games trains it on its own unweighted MSE and drops the critic term from the
        # actor loss; the two gradients do not overlap (separate parameters), so one backward serves both
        v_coef = 1.0 if self.net.central else 0.5 * c.critic_coef
        loss = a_loss + v_coef * c_loss - c.entropy_coef * ent + c.bounds_loss_coef * b_loss
        for p in self.net.parameters():
            p.grad = None
        loss.backward()
        with torch.no_grad():      # KL between the old and new diagonal Gaussians (same sigma)
            kl_i = (0.5 * ((mu - d["old_mu"][idx]) / ls.exp()).pow(2)).sum(-1)
            if self.sym is not None:               # over the original rows alone, divisor B
                kl = (w[:B] * kl_i[:B]).mean() if self.ends else kl_i[:B].mean()
                self._sym_mu = mu.detach()
            else:
                kl = wmean(kl_i)
            acc["kl"] += kl
            acc["loss"] += loss.detach(); acc["a_loss"] += a_loss.detach(); acc["c_loss"] += c_loss.detach()
            if self.diag is not None:              # the torch statement of what tfp_ppo_loss_diag counts
                vk = dict(v=v, ret=d["ret"][idx], old_v=d["old_v"][idx]) if self.clip_v else {}
                diag_merge(self.diag, diag_objective_statement(d["old_nlp"][idx] - nlp, ratio, a, mu, c.e_clip, w=w, kl_rows=B if self.sym is not None else None,
                                                               **vk), objective=True)

    def _sym_minibatch(self, d, idx):
        """the 3B minibatch of `symmetry_augmentation` in plain torch: rows [k B, (k + 1) B) = G^k of obs / states, P^k of act and old_mu, the rest repeated"""
        from .symmetry import apply
        t = self.sym
        img = lambda x, tabs: torch.cat([x, apply(x, tabs[0]), apply(x, tabs[1])])        # noqa: E731
        out = {k: (img(d[k][idx], t[name]) if d[k] is not None else None) for k, name in (("obs", "obs"), ("states", "states"), ("act", "action"), ("old_mu", "action"))}
        for k in ("old_nlp", "adv", "ret", "old_v", "w"):
            if k in d:
                out[k] = d[k][idx].repeat(3)
        return out

    def _mb_backward_fused(self, d, idx, acc):
        """the same step on the hand-written kernels: one gather launch for the seven minibatch arrays (eight with `clip_value`: old_v), the MFMA layers, the objective
        and its gradients in ONE launch (ppo_kernels.ppo_loss_and_grads), the backward pass started at the network outputs with those
        gradients (no loss node), the chunk sums of all weight gradients in one launch.  Every parameter gradient lands in its slot of
        the flat gradient buffer directly (the log-std gradient too), so that the optimiser reads nothing but that buffer; the
        statistics accumulate on the device in `acc["_fused"]` = (loss, a_loss, c_loss, kl)"""
        from . import ppo_kernels as pk
        c = self.cfg
        na, ns = self.net.obs_norm, self.net.state_norm
        # what the ONE gather launch carries, in order: (key, source, statistics or None) - with statistics the same launch writes obs / states normalised: what
        # the forward AND the first layers' weight gradients read.  adv is (adv_i, w_i) interleaved with `episode_ends`, ret is ret_n with `normalize_value`
        ent = [("obs", d["obs"], na.stats() if na is not None else None), ("act", d["act"], None), ("old_nlp", d["old_nlp"], None),
               ("adv", d["adv_w"] if self.ends else d["adv"], None), ("ret", d["ret"], None), ("old_mu", d["old_mu"], None)]
        if self.clip_v:
            ent.append(("old_v", d["old_v"], None))
        if d["states"] is not None:
            ent.append(("states", d["states"], ns.stats() if ns is not None else None))
        assert len(ent) <= pk.GATHER_MAX                   # with every option on exactly one launch's worth
        if self.sym is not None:                           # the same ONE launch writes the three images: 3B rows per array, statistics behind the transform
            g = dict(zip([e[0] for e in ent], pk.gather_rows_sym([e[1] for e in ent], idx, [self.sym["packed"].get(e[0]) for e in ent], norm=[e[2] for e in ent])))
            kl_rows = {"kl_rows": idx.numel()}             # the KL statistic: the original rows alone
        else:
            g = dict(zip([e[0] for e in ent], pk.gather_rows([e[1] for e in ent], idx, norm=[e[2] for e in ent])))
            kl_rows = {}
        for p in self.net.parameters():
            p.grad = None
        # no autograd: the structure is fixed (two Linear / ELU stacks), so the step is a straight sequence of kernel launches from this
        # thread - forward of both networks, the objective with its gradients, the two backward walks, one launch for all chunk sums
        with torch.no_grad():
            la, lc = self._layer_lists
            obs = g["obs"]
            xc = g["states"] if self.net.central else obs
            ya, yc = pk.mlp_forward_pair(obs, la, xc, lc)        # layer k of both networks in one launch
            mu, v = ya[-1], yc[-1].squeeze(-1)
            v_coef = 1.0 if self.net.central else 0.5 * c.critic_coef
            kw = {"old_v": g["old_v"]} if self.clip_v else {}
            if self.ends:                                  # the gathered array is (adv_i, w_i): the weighted instantiation of the objective
                kw["adv_w"] = g.pop("adv")
            kw.update(kl_rows)
            if self.diag is not None:                      # the DIAG instantiation of the same launch adds to the record
                kw["diag"] = self.diag
            if self.sym is not None:
                self._sym_mu = mu
            _, d_mu, d_v, _ = pk.ppo_loss_and_grads(mu, self.net.log_std, v, g["act"], g["old_nlp"], g.get("adv"), g["ret"], g["old_mu"], acc["_fused"], c.e_clip,
                                                    v_coef, c.entropy_coef, c.bounds_loss_coef, d_ls_out=self.flat_opt.grad_view(self.net.log_std), **kw)
            try:
                pk.mlp_backward_pair(obs, ya, d_mu, la, xc, yc, d_v.unsqueeze(-1), lc)
                pk.flush_partial_sums()
            finally:
                pk.discard_partial_sums()                  # nothing stale survives a launch that raised

    @staticmethod
    def _new_acc(dev):
        """running sums of the logged quantities, device side: views of ONE buffer (loss, a_loss, c_loss, kl), which is also
        what the fused objective kernel accumulates into"""
        buf = torch.zeros(4, device=dev)
        return {"loss": buf[0], "a_loss": buf[1], "c_loss": buf[2], "kl": buf[3], "_fused": buf}

    def _mb_apply(self, gathered=False):
        if self.flat_opt is not None:
            self.flat_opt.step(gathered, **({"diag": self.diag} if self.diag is not None else {}))
            return
        # (parameters, max_norm, truncates) per optimiser: truncate_grads of each on its own network
        if self.net.central:
            groups = [(self.net.actor_parameters(), self.cfg.grad_norm, self.trunc[0]), (self.net.critic_parameters(), self.cfg.value_grad_norm, self.trunc[1])]
        else:
            groups = [(list(self.net.parameters()), self.cfg.grad_norm, self.trunc[0])]
        norms = [nn.utils.clip_grad_norm_(ps, mx, foreach=True) if on else None for ps, mx, on in groups]
        if self.diag is not None:              # the torch statement of what tfp_clip_adam_diag files: the pre-truncation norms, clip_grad_norm_'s return value
            with torch.no_grad():
                norms = [nrm if nrm is not None else total_grad_norm(ps) for nrm, (ps, _, _) in zip(norms, groups)]
                diag_merge(self.diag, diag_optimiser_statement(norms, [mx if on else float("inf") for _, mx, on in groups]), objective=False)
        self.opt.step()

    def _flatten_grads(self, out=None):
        if self.flat_opt is not None:
            return self.flat_opt.gather_grads()
        grads = [p.grad for p in self.net.parameters()]
        return torch.cat([g.reshape(-1) for g in grads], out=out)

    def _unflatten_grads(self, flat):
        if self.flat_opt is not None:
            return                                 # the optimiser reads the flat buffer itself
        off = 0
        for p in self.net.parameters():
            p.grad.copy_(flat[off:off + p.numel()].view_as(p.grad))
            off += p.numel()

    def _exchange(self, flat):
        self.n_grad_allreduce += 1
        self.dist.all_reduce(flat, op=self.dist.ReduceOp.SUM, group=self.group)
        flat /= self.dist.get_world_size(self.group)

    def update(self, buf):
        c = self.cfg
        T, n = buf["nlp"].shape
        flat = lambda x: x.reshape(T * n, *x.shape[2:]) if x is not None else None  # noqa: E731
        adv = flat(buf["adv"])
        w = flat(buf["w"]) if self.ends else None
        if c.normalize_advantage:
            adv = masked_advantage_norm(adv, w) if self.ends else (adv - adv.mean()) / (adv.std() + 1e-8)
        vn = self.value_norm
        src = dict(obs=flat(buf["obs"]), states=flat(buf["states"]), act=flat(buf["act"]), old_nlp=flat(buf["nlp"]),
                   ret=flat(buf["ret_n"] if vn is not None else buf["ret"]), adv=adv, old_mu=flat(buf["mu"]))
        if self.clip_v:                            # the value the loss is clipped around, in the units the network works in
            src["old_v"] = flat(buf["v_old_n"] if vn is not None else buf["val"][:T])
        if self.ends:
            src["w"] = w
            if self.fused_loss:                    # (adv_i, w_i) interleaved, stacked once per epoch: ONE gathered array, the gather keeps its eight
                src["adv_w"] = torch.stack([adv, w], dim=1)
            ended = buf["end"].sum()               # device side; fetched with the other statistics below
        if self.tracker is not None:               # the epoch's vector: summed over the ranks (ONE all-reduce), taken and cleared on the device; read below
            if self.dist_on:
                self.tracker.merge(self.group)
                self.n_track_allreduce += 1
            track_vec = self.tracker.take()
        if self.diag is not None:                  # once per epoch in torch, rank-local like symmetry_gap: the rollout's samples with w = 1, in reward units.
            # ret = adv + val (GAE), so ret - val is the advantage estimate as filed: [Var(ret - val), Var(ret)] (population), read below
            wv = w if self.ends else torch.ones_like(adv)
            err, rets, sw = flat(buf["adv"]), flat(buf["ret"]), wv.sum()
            pvar = lambda x: (wv * (x - (wv * x).sum() / sw) ** 2).sum() / sw  # noqa: E731
            ev_pair = torch.stack([pvar(err), pvar(rets)])
        total = T * n
        mb = max(1, total // c.minibatches)
        dev = src["obs"].device
        d = src
        acc = self._new_acc(dev)
        for v in acc.values():
            v.zero_()
        stats = {"kl": 0.0}
        count = 0
        if self.lr_schedule == "linear":           # once per epoch
            self._set_actor_lr(self.scheduled_lr(self.epoch))
        for _ in range(c.mini_epochs):
            perm = torch.randperm(total, device=dev)
            acc["kl"].zero_()
            nmb = 0
            for s in range(0, total - mb + 1, mb):
                self._mb_backward(d, perm[s:s + mb], acc)
                if self.dist_on:
                    fl = self._flatten_grads()
                    self._exchange(fl)
                    self._unflatten_grads(fl)
                self._mb_apply(gathered=self.dist_on)
                nmb += 1
            count += nmb
            kl = acc["kl"] / max(nmb, 1)
            if self.dist_on:
                self.n_kl_allreduce += 1
                self.dist.all_reduce(kl, op=self.dist.ReduceOp.SUM, group=self.group)
                kl /= self.dist.get_world_size(self.group)
            kl = float(kl)                     # the one host sync per mini-epoch (adaptive learning rate)
            stats["kl"] = kl
            if self.lr_schedule == "adaptive":      # rl_games AdaptiveScheduler; identity / linear: the statistic is logged, the rate is not moved here
                lr = self.lr
                if kl > 2.0 * c.kl_threshold:
                    lr = max(lr / 1.5, 1e-6)
                elif kl < 0.5 * c.kl_threshold:
                    lr = min(lr * 1.5, 1e-2)
                self._set_actor_lr(lr)
        # `normalize_value`: the epoch's de-normalised returns buf["ret"] (T n samples) join the end-of-epoch merge of the input records
        self._update_input_norm(src, returns=buf["ret"].reshape(-1, 1) if vn is not None else None)
        for k in ("loss", "a_loss", "c_loss"):
            stats[k] = float(acc[k]) / max(count, 1)
        stats["lr"] = self.lr
        stats["mean_reward"] = float(buf["rew"].mean() / c.reward_scale)
        if self.ends:
            stats["episodes_ended"] = int(ended)
        if self.tracker is not None:
            stats.update(self._track_stats(track_vec.tolist()))
        if self.sym is not None and self._sym_mu is not None:
            stats["symmetry_gap"] = float(self._symmetry_gap())
        if self.diag is not None:
            stats.update(self._diag_stats(ev_pair))
        return stats

    @torch.no_grad()
    def _diag_stats(self, ev_pair):
        """`diagnostics`: take the epoch's record and clear it; with a process group slots 0-6 through ONE SUM all-reduce and (RATIO_MAX, -RATIO_MIN) through
        ONE MAX all-reduce (`n_diag_allreduce` counts both; the gradient norms are those of the exchanged gradient, the same on every rank, and stay), then
        the keys of the module docstring - the record's, and explained_variance / entropy / sigma_mean of this rank in torch"""
        vec = self.diag.clone()
        self.diag.copy_(new_diag_record(self.device))
        if self.dist_on:
            sums = vec[:D_RATIO_MAX].clone()
            ext = torch.stack([vec[D_RATIO_MAX], -vec[D_RATIO_MIN]])
            self.dist.all_reduce(sums, op=self.dist.ReduceOp.SUM, group=self.group)
            self.dist.all_reduce(ext, op=self.dist.ReduceOp.MAX, group=self.group)
            self.n_diag_allreduce += 2
            vec[:D_RATIO_MAX], vec[D_RATIO_MAX], vec[D_RATIO_MIN] = sums, ext[0], -ext[1]
        ls = self.net.log_std.detach()
        extra = torch.cat([ev_pair.double(), torch.stack([(ls + 0.5 + 0.5 * math.log(2 * math.pi)).sum(), ls.exp().mean()]).double()]).tolist()
        self.last_diag = vec.tolist()
        out = diagnostic_stats(self.last_diag, ls.numel(), self.clip_v, self.net.central)
        if extra[1] > 0.0:                         # absent when the returns do not vary
            out["explained_variance"] = 1.0 - extra[0] / extra[1]
        out["entropy"], out["sigma_mean"] = extra[2], extra[3]
        return out

    def _track_stats(self, vec):
        """file the epoch's vector (a list of integers, the same on every rank) and return the episode keys of the statistics: the window's means and rates
        (absent before any episode has ended), its count `episodes`, and the cumulative counts"""
        from .evaluate import EpisodeTracker, T_EPISODES, T_NONFINITE, T_UNARMED
        for k, j in enumerate((T_EPISODES, T_NONFINITE, T_UNARMED)):
            self.track_totals[k] += int(vec[j])
        if int(vec[T_EPISODES]) > 0:
            self.track_window = EpisodeTracker.window(self.track_window + [[int(x) for x in vec]], self.cfg.games_to_track)
        out = EpisodeTracker.window_stats(self.track_window)
        out["episodes_total"], out["episodes_nonfinite"], out["episodes_unarmed"] = self.track_totals
        return out

    @torch.no_grad()
    def _update_input_norm(self, src, returns=None):
        """the end of an epoch: the moments of its RAW rollout buffer (T n rows) merged into the running records, which then serve the next epoch.
        One pass over the buffer (ppo_kernels.moments: both inputs in one call) and one merge launch; a distributed run gathers every rank's batch vector
        [1 + 2 Do (+ 1 + 2 Ds)] (float64) with ONE all_gather and merges them in rank order, so that all ranks keep the same record bit for bit.
        `returns` [T n, 1] (`normalize_value`: the epoch's de-normalised returns): the returns' record [3] is appended to the vector - one more moments call and one more merge
        launch (the kernels take up to two arrays per call), the same single all_gather."""
        recs = dict(self._norm_records())
        n_in = len(recs)
        if returns is not None:
            recs["returns"], src = self.value_norm, dict(src, returns=returns)
        if not recs:
            return
        keys = list(recs)                                            # "obs" before "states" before "returns"
        xs = [src[k] for k in keys]
        fused = self.fused_loss and all(x.is_cuda and x.dtype == torch.float32 and x.is_contiguous() for x in xs)
        groups = [g for g in (keys[:n_in], keys[n_in:]) if g]        # one moments call / one merge launch each
        if fused:
            from . import ppo_kernels as pk
        parts = []
        for g in groups:
            gx = [src[k] for k in g]
            v = pk.moments(gx) if fused else None                    # None: declined (a row wider than 256)
            parts.append(v if v is not None else torch.cat([InputNorm.batch_record(x) for x in gx]))
        vec = parts[0] if len(parts) == 1 else torch.cat(parts)
        L, k = vec.numel(), 1
        if self.dist_on:
            k = self.dist.get_world_size(self.group)
            parts = [torch.empty_like(vec) for _ in range(k)]
            self.n_norm_allgather += 1
            self.dist.all_gather(parts, vec, group=self.group)
            vec = torch.cat(parts)
        offs, off = [], 0
        for key in keys:
            offs.append(off)
            off += 1 + 2 * recs[key].dim
        if fused:
            at = dict(zip(keys, offs))
            for g in groups:
                pk.norm_merge([recs[key].state for key in g], [vec[at[key]:] for key in g], k, L, [recs[key].mean_f for key in g],
                              [recs[key].inv_std_f for key in g])
        else:
            rows = vec.view(k, L)
            for key, o in zip(keys, offs):
                recs[key].merge(rows[:, o:o + 1 + 2 * recs[key].dim])

    def train(self, epochs, log=None, checkpoint_dir=None):
        """`epochs` PPO iterations.  With `checkpoint_dir` (rank 0 only): `<name>.pth` every `save_frequency` epochs and
        at the end, `<name>_best.pth` whenever the mean reward improves after `save_best_after` epochs.  With `track_episodes` the best is judged by
        `episode_return` once a window exists (RL-Games' criterion), and an `episode_return` above `score_to_win` saves `<name>.pth`, marks `won` in the
        epoch's statistics and stops - on every rank in the same epoch, since every rank holds the all-reduced vector."""
        out = []
        for _ in range(epochs):
            st = self.update(self.rollout())
            self.epoch += 1
            st["epoch"], st["frames"] = self.epoch - 1, self.frames
            won = self.tracker is not None and st.get("episode_return", -float("inf")) > self.cfg.score_to_win
            if won:
                st["won"] = True
            out.append(st)
            if log:
                log(st)
            if checkpoint_dir:
                if self.epoch % max(self.cfg.save_frequency, 1) == 0:
                    self.save(os.path.join(checkpoint_dir, f"{self.cfg.name}.pth"))
                score = st["mean_reward"] if self.tracker is None else st.get("episode_return")
                if self.epoch >= self.cfg.save_best_after and score is not None and score > self.best_reward:
                    self.best_reward = score
                    self.save(os.path.join(checkpoint_dir, f"{self.cfg.name}_best.pth"))
            if won or self.epoch >= self.cfg.max_epochs:     # won: the final save below writes <name>.pth
                break
        if checkpoint_dir:
            self.save(os.path.join(checkpoint_dir, f"{self.cfg.name}.pth"))
        return out
