"""Episode statistics of a population of envs, accumulated on the device: what answers "how good is this checkpoint?".

`EpisodeStats` binds to the buffers of a `TrifingerEngine` and is updated once per env step, behind the step, with no host synchronisation.  Episode ends
are taken from the engine's own `reset_buf` (the public `dones` is `reset_buf & goal_reset_buf`, which the shipped configuration never sets although every
env times out), the final errors from the state rows, which hold the final pose until the reset at the start of the next step.  On the GPU an update is one
launch of csrc/tf_eval.hip (include/trifinger_ppo_eval.h has the definitions and the layout of the accumulator); the plain-torch form below has the same
semantics, the same accumulator layout, the same bit-pattern bins, final errors (`step_errors`) and fixed-point conversions - the same bits -, and serves CPU tensors (the tests' oracle engines) and
`fused=False`.  The accumulator holds integers only: integer sums commute, so the vector is bitwise the same on every run and after `merge` over ranks.
"""
import math
import struct

import torch

from . import _capi as capi

# include/trifinger_ppo_eval.h
ENV_RETURN, ENV_AT_GOAL_STEPS, ENV_FIRST_HIT, ENV_EPISODES, ENV_ROWS = 0, 1, 2, 3, 4
POS_BINS, ORI_BINS = 50, 42
POS_Q = (460, 508)            # bits >> 21 of 2^-12 m and of 1 m
ORI_Q = (476, 516)            # ... of 2^-8 rad and of 4 rad
(EPISODES, NONFINITE, POS_OK, ORI_OK, SUCCESS, REACHED, GOAL_EVENTS, ENVS_COMPLETE, SUM_LENGTH, SUM_AT_GOAL_STEPS, SUM_FIRST_HIT, SUM_RETURN, SUM_POS_ERR,
 SUM_ORI_ERR, HIST_POS) = range(15)
HIST_ORI = HIST_POS + POS_BINS
ACC = HIST_ORI + ORI_BINS
S_RETURN, S_POS_ERR, S_ORI_ERR = 2.0 ** 16, 2.0 ** 30, 2.0 ** 28
RETURN_MAX, POS_ERR_MAX, ORI_ERR_MAX = 2.0 ** 25, 2.0 ** 10, 4.0

_BUFFERS = ("state", "reward", "reset_buf", "goal_reset_buf", "steps")


def engine_of(env):
    """the TrifingerEngine behind an env: RlGamesGpuEnvAdapter (.env) -> VecTaskPython (._task) -> TrifingerEnv (._engine); an object that has the engine's
    buffer attributes itself is returned as it is.  ValueError for an env without one."""
    obj = env
    for _ in range(8):
        if all(hasattr(obj, k) for k in _BUFFERS):
            return obj
        nxt = next((getattr(obj, k) for k in ("_engine", "_task", "env") if getattr(obj, k, None) is not None), None)
        if nxt is None:
            break
        obj = nxt
    raise ValueError(f"{type(env).__name__}: no native engine behind this env (episode statistics are taken from the engine's buffers: "
                     f"{', '.join(_BUFFERS)})")


def rule_of_difficulty(d):
    """which predicate is `at goal`: 0 position (difficulty < 4), 1 both (== 4), 2 orientation (> 4) - __check_termination of the reference"""
    return 0 if d < 4 else (1 if d == 4 else 2)


def bin_edge(q):
    """the float32 with the bit pattern q << 21: the lower edge of the histogram bin that starts at q"""
    return struct.unpack("<f", struct.pack("<I", q << 21))[0]


def bin_bounds(b, q_lo, q_hi):
    """(lower edge, upper edge) of bin b of a histogram with the bounds (q_lo, q_hi): bin 0 is [0, edge(q_lo)), the last one [edge(q_hi), inf)"""
    if b == 0:
        return 0.0, bin_edge(q_lo)
    if b == 1 + q_hi - q_lo:
        return bin_edge(q_hi), math.inf
    return bin_edge(q_lo + b - 1), bin_edge(q_lo + b)


def quantile_bin(hist, num, den, q_lo, q_hi):
    """bounds of the bin that holds the ceil(num / den * n)-th smallest of the n samples of `hist` (integers); (nan, nan) without samples"""
    n = int(sum(hist))
    if n <= 0:
        return math.nan, math.nan
    k, c = max(1, -(-num * n // den)), 0
    for b, h in enumerate(hist):
        c += int(h)
        if c >= k:
            return bin_bounds(b, q_lo, q_hi)
    raise AssertionError("unreachable: the bins sum to n")


def _bins(x, q_lo, q_hi):
    q = x.contiguous().view(torch.int32).to(torch.int64) >> 21          # x >= 0 where it is used: the pattern is a non-negative int32
    return torch.where(q < q_lo, torch.zeros_like(q), torch.where(q >= q_hi, torch.full_like(q, 1 + q_hi - q_lo), 1 + q - q_lo))


# what a kernel of csrc/tf_eval.hip reads a per-env engine buffer as, one element per env (`state` is float32 [TF_STATE_ROWS, N])
_KERNEL_READS = {"reward": (torch.float32,), "reset_buf": (torch.bool, torch.uint8), "goal_reset_buf": (torch.bool, torch.uint8), "steps": (torch.int64,)}


class EngineObserver:
    """What EpisodeStats, EpisodeTracker and record.EpisodeRecorder share: they bind to the buffers of an engine (`engine_of`), judge an episode's end by
    the same tolerances and at-goal rule (defaults: the engine's config, as the episode length), run ONE launch of csrc/tf_eval.hip behind an env step
    where the buffers live on a GPU and the plain-torch statement of the same definitions otherwise (`fused`: None decides by the device), and keep an
    int64 accumulator `acc` that sums over ranks.  A subclass names the per-env buffers its kernel reads besides `state` (`buffers`), the length of its
    accumulator (`acc_size`), and provides `_launch()` and `_update_torch()`."""
    buffers = ()
    acc_size = 0

    def __init__(self, engine, pos_tol=None, ori_tol=None, rule=None, fused=None, episode_length=None):
        self.engine = engine = engine_of(engine)
        cfg = getattr(engine, "cfg", None)
        if (pos_tol is None or ori_tol is None or rule is None) and cfg is None:
            raise ValueError("an engine without a config needs pos_tol, ori_tol and rule")
        self.pos_tol = float(cfg.position_tolerance if pos_tol is None else pos_tol)
        self.ori_tol = float(cfg.orientation_tolerance if ori_tol is None else ori_tol)
        self.rule = int(rule_of_difficulty(int(cfg.task_difficulty)) if rule is None else rule)
        self.ep_len = int((getattr(cfg, "episode_length", 0) or 0) if episode_length is None else episode_length)
        if self.rule not in (0, 1, 2) or math.isnan(self.pos_tol) or math.isnan(self.ori_tol) or self.ep_len < 0:
            raise ValueError(f"rule {self.rule} (0, 1, 2), tolerances {self.pos_tol}, {self.ori_tol}, episode_length {self.ep_len} (>= 0)")
        st = engine.state
        self.num_envs = n = int(st.shape[1])
        self.fused = st.is_cuda if fused is None else bool(fused)
        if self.fused and not st.is_cuda:
            raise ValueError("fused=True: the kernel reads device buffers, this engine lives on the CPU")
        if self.fused:
            if tuple(st.shape) != (capi.TF_STATE_ROWS, n) or st.dtype != torch.float32 or not st.is_contiguous():
                raise ValueError("engine buffer 'state' of another layout than include/trifinger.h: contiguous float32 [TF_STATE_ROWS, N]")
            for k in self.buffers:
                t, ok = getattr(engine, k), _KERNEL_READS[k]
                if t.dtype not in ok or tuple(t.shape) != (n,) or not t.is_contiguous() or t.device != st.device:
                    raise ValueError(f"engine buffer '{k}': {t.dtype} {tuple(t.shape)} on {t.device}, the kernel reads contiguous "
                                     f"{' / '.join(str(d) for d in ok)} [{n}] on {st.device}")
        self.acc = torch.zeros((self.acc_size,), dtype=torch.int64, device=st.device)
        self.n_allreduce = 0

    def update(self):
        """account for the env step that has just run (on the stream it ran on); no host synchronisation"""
        if not self.fused:
            self._update_torch()
        elif torch.cuda.current_device() != self.acc.device.index:
            with torch.cuda.device(self.acc.device):
                self._launch()
        else:
            self._launch()

    def merge(self, group=None):
        """sum the accumulator over the ranks of `group`: ONE all-reduce of the int64 vector, after which every rank holds the same bits"""
        import torch.distributed as dist
        dist.all_reduce(self.acc, op=dist.ReduceOp.SUM, group=group)
        self.n_allreduce += 1


class EpisodeStats(EngineObserver):
    """Episode statistics of the envs of `engine` (a TrifingerEngine, or anything with its buffer attributes state / reward / reset_buf /
    goal_reset_buf / steps): `reset()`, then `update()` after every env step - no host synchronisation -, `merge(group)` once in a distributed run,
    `result()` for the one synchronising read.  Tolerances and the at-goal rule default to the engine's config.  `max_episodes_per_env`: an env that has
    finished that many episodes goes on running, its further episodes are not counted (0: no cap).  `fused`: None = the kernel where the buffers live on
    a GPU, plain torch otherwise."""

    buffers = ("reward", "reset_buf", "goal_reset_buf", "steps")
    acc_size = ACC

    def __init__(self, engine, pos_tol=None, ori_tol=None, max_episodes_per_env=0, fused=None, rule=None):
        super().__init__(engine, pos_tol, ori_tol, rule, fused)
        self.cap = int(max_episodes_per_env)
        if self.cap < 0:
            raise ValueError(f"max_episodes_per_env {self.cap} (>= 0)")
        self.env_acc = torch.zeros((ENV_ROWS, self.num_envs), dtype=torch.int32, device=self.acc.device)

    def reset(self):
        self.env_acc.zero_()
        self.acc.zero_()

    def _launch(self):
        from . import ppo_kernels as pk
        e = self.engine
        pk.eval_step(e.state, e.reward, e.reset_buf, e.goal_reset_buf, e.steps, self.env_acc, self.acc, self.pos_tol, self.ori_tol, self.rule, self.cap)

    @torch.no_grad()
    def _update_torch(self):
        e, ea, acc = self.engine, self.env_acc, self.acc
        ret = ea[ENV_RETURN].view(torch.float32) + e.reward
        e_p, e_o, pos_ok, ori_ok, at_goal, fin = episode_outcome(e.state, ret, self.pos_tol, self.ori_tol, self.rule)
        atg = ea[ENV_AT_GOAL_STEPS] + at_goal.to(torch.int32)
        length = e.steps.to(torch.int64)
        first = torch.where((ea[ENV_FIRST_HIT] == 0) & at_goal, length.clamp(1, 2 ** 31 - 1).to(torch.int32), ea[ENV_FIRST_HIT])
        eps = ea[ENV_EPISODES]
        under = (eps < self.cap) if self.cap else torch.ones_like(at_goal)
        ends = e.reset_buf.to(torch.bool)
        counted, nonfin = ends & under & fin, ends & under & ~fin
        i64 = torch.int64
        zero = torch.zeros_like(length)
        acc[EPISODES] += counted.sum()
        acc[NONFINITE] += nonfin.sum()
        acc[POS_OK] += (counted & pos_ok).sum()
        acc[ORI_OK] += (counted & ori_ok).sum()
        acc[SUCCESS] += (counted & at_goal).sum()
        acc[REACHED] += (counted & (first != 0)).sum()
        acc[GOAL_EVENTS] += (under & e.goal_reset_buf.to(torch.bool)).sum()
        if self.cap:
            acc[ENVS_COMPLETE] += (ends & under & (eps + 1 == self.cap)).sum()
        acc[SUM_LENGTH] += torch.where(counted, length, zero).sum()
        acc[SUM_AT_GOAL_STEPS] += torch.where(counted, atg.to(i64), zero).sum()
        acc[SUM_FIRST_HIT] += torch.where(counted, first.to(i64), zero).sum()
        acc[SUM_RETURN:SUM_ORI_ERR + 1] += torch.stack(fixed_sums(counted, ret, e_p, e_o))
        acc[HIST_POS:HIST_POS + POS_BINS] += torch.bincount(_bins(e_p, *POS_Q)[counted], minlength=POS_BINS)
        acc[HIST_ORI:HIST_ORI + ORI_BINS] += torch.bincount(_bins(e_o, *ORI_Q)[counted], minlength=ORI_BINS)
        izero = torch.zeros_like(atg)
        ea[ENV_RETURN] = torch.where(ends, torch.zeros_like(ret), ret).view(torch.int32)
        ea[ENV_AT_GOAL_STEPS] = torch.where(ends, izero, atg)
        ea[ENV_FIRST_HIT] = torch.where(ends, izero, first)
        ea[ENV_EPISODES] = torch.where(ends & under, eps + 1, eps)

    def envs_complete(self):
        """the number of envs that have reached the cap; synchronises (one int64)"""
        return int(self.acc[ENVS_COMPLETE])

    def result(self):
        """the statistics as a dict of Python numbers (the one synchronising read); a rate or mean over zero episodes is nan"""
        return summarize(self.acc.cpu().tolist())


def summarize(raw):
    """the result dict of an accumulator vector (a list of TFP_EVAL_ACC integers)"""
    raw = [int(x) for x in raw]
    if len(raw) != ACC:
        raise ValueError(f"an accumulator has {ACC} entries, got {len(raw)}")
    n = raw[EPISODES]

    def per(x, d=n):
        return x / d if d > 0 else math.nan
    hp, ho = raw[HIST_POS:HIST_POS + POS_BINS], raw[HIST_ORI:HIST_ORI + ORI_BINS]
    return {
        "episodes": n, "nonfinite_episodes": raw[NONFINITE],
        "success_rate": per(raw[SUCCESS]), "success_rate_position": per(raw[POS_OK]), "success_rate_orientation": per(raw[ORI_OK]),
        "reached_goal_rate": per(raw[REACHED]),
        "steps_to_goal_mean": per(raw[SUM_FIRST_HIT], raw[REACHED]),
        "time_at_goal_fraction": per(raw[SUM_AT_GOAL_STEPS], raw[SUM_LENGTH]),
        "goals_reached": raw[GOAL_EVENTS],
        "episode_reward_mean": per(raw[SUM_RETURN] / S_RETURN), "episode_length_mean": per(raw[SUM_LENGTH]),
        "final_position_error_mean": per(raw[SUM_POS_ERR] / S_POS_ERR), "final_orientation_error_mean": per(raw[SUM_ORI_ERR] / S_ORI_ERR),
        "final_position_error_median": quantile_bin(hp, 1, 2, *POS_Q), "final_position_error_p90": quantile_bin(hp, 9, 10, *POS_Q),
        "final_orientation_error_median": quantile_bin(ho, 1, 2, *ORI_Q), "final_orientation_error_p90": quantile_bin(ho, 9, 10, *ORI_Q),
        "envs_complete": raw[ENVS_COMPLETE],
        "raw": raw,
    }


# ---- the training-time episode tracker (include/trifinger_ppo_track.h) -------------------------------------------------------------------------------
TRK_RETURN, TRK_ARMED, TRK_ROWS = 0, 1, 2
(T_EPISODES, T_SUCCESS, T_POS_OK, T_ORI_OK, T_TIMEOUT, T_SUM_LENGTH, T_SUM_RETURN, T_SUM_POS_ERR, T_SUM_ORI_ERR, T_NONFINITE, T_UNARMED, TRACK_ACC) = range(12)


def _fma32(a, b, c):
    """float32 fma(a, b, c), rounded ONCE, out of float64 operations: the product of two float32 is exact in float64; the sum is rounded to odd (the
    error of the float64 addition is recovered with TwoSum, and an inexact sum with an even last bit moves to its odd neighbour on the side of the
    error), after which the rounding to float32 is the rounding of the exact value (53 >= 2 * 24 + 2 bits)"""
    p, c = a.double() * b.double(), c.double()
    s = p + c
    bb = s - p
    err = (p - (s - bb)) + (c - bb)
    even = (s.view(torch.int64) & 1) == 0
    odd = torch.nextafter(s, torch.where(err > 0, torch.full_like(s, math.inf), torch.full_like(s, -math.inf)))
    return torch.where((err != 0) & even & torch.isfinite(s), odd, s).float()


def _sqrt32(x):
    """the correctly rounded float32 square root (the device's IEEE sqrt), whatever torch's own float32 sqrt does on this backend: through float64,
    whose 53 bits make the second rounding harmless for a square root"""
    return x.double().sqrt().float()


def step_asin(x):
    """tf_asin of csrc/tf_device_math.h operation for operation in float32 - the arcsine the step, the evaluator's kernel and the tracker's kernel use -,
    for x >= 0"""
    f = lambda v: torch.full_like(x, v)                                    # noqa: E731
    a = torch.where(x < 1.0, x, f(1.0))                                    # fminf: a NaN becomes 1
    big = a > 0.5
    z = torch.where(big, 0.5 * (1.0 - a), a * a)
    y = torch.where(big, _sqrt32(z), a)
    p = f(4.2163199048e-2)
    for k in (2.4181311049e-2, 4.5470025998e-2, 7.4953002686e-2, 1.6666752422e-1):
        p = _fma32(p, z, f(k))
    p = _fma32(p * z, y, y)
    return torch.where(big, 1.5707963267948966 - (p + p), p)


def step_errors(state):
    """(e_p, e_o, both quaternions finite) per env from the state rows, in the step's own expressions (csrc/tf_eval.hip: eval_errors, behind episode_outcome) - float32, every
    operation rounded separately in the device code's order, the arcsine the step's polynomial (step_asin), so that the values are the kernel's"""
    from .utils.torch_utils import quat_conjugate, quat_mul
    cp, gp = state[capi.S_CUBE_P:capi.S_CUBE_P + 3], state[capi.S_GOAL_P:capi.S_GOAL_P + 3]
    cq, gq = state[capi.S_CUBE_Q:capi.S_CUBE_Q + 4].t().contiguous(), state[capi.S_GOAL_Q:capi.S_GOAL_Q + 4].t().contiguous()
    d = cp - gp
    e_p = _sqrt32(d[0] * d[0] + d[1] * d[1] + d[2] * d[2])
    m = quat_mul(cq, quat_conjugate(gq))
    nrm = _sqrt32(m[:, 0] * m[:, 0] + m[:, 1] * m[:, 1] + m[:, 2] * m[:, 2])
    e_o = 2.0 * step_asin(nrm)
    return e_p, e_o, torch.isfinite(cq).all(1) & torch.isfinite(gq).all(1)


def episode_outcome(state, ret, pos_tol, ori_tol, rule):
    """THE episode outcome per env, stated once for the three `_update_torch` (csrc/tf_eval.hip: episode_outcome is the same statement on the device):
    (e_p, e_o, pos_ok, ori_ok, at_goal, fin) - the final errors of `step_errors`, the two predicates, the at-goal rule (0 position, 1 both,
    2 orientation) and the finite test of an episode whose return is `ret`"""
    e_p, e_o, qfinite = step_errors(state)
    pos_ok, ori_ok = e_p <= pos_tol, e_o <= ori_tol
    at_goal = pos_ok if rule == 0 else ((pos_ok & ori_ok) if rule == 1 else ori_ok)
    return e_p, e_o, pos_ok, ori_ok, at_goal, torch.isfinite(ret) & torch.isfinite(e_p) & torch.isfinite(e_o) & qfinite


def fixed_sums(counted, ret, e_p, e_o):
    """the three fixed-point sums over the `counted` envs, int64 scalars: the return in 2^-16 (clamped to +-2^25), the position error in 2^-30 (to 2^10),
    the orientation error in 2^-28 (to 4).  A non-finite value never reaches a conversion"""
    clean = torch.zeros_like(ret)

    def fixed(x, lo, hi, scale):
        return torch.round(torch.where(counted, x, clean).clamp(lo, hi) * scale).to(torch.int64).sum()
    return fixed(ret, -RETURN_MAX, RETURN_MAX, S_RETURN), fixed(e_p, 0.0, POS_ERR_MAX, S_POS_ERR), fixed(e_o, 0.0, ORI_ERR_MAX, S_ORI_ERR)


class EpisodeTracker(EngineObserver):
    """What an EPISODE is worth while the policy trains (`params.config.track_episodes`): returns, lengths and success of the episodes that end during
    the rollouts, accumulated on the device behind every env step with no host synchronisation.  include/trifinger_ppo_track.h has the definitions; in
    short, per env: the float32 return is summed in step order from the step with steps == 1 (which ARMS the env), and at a step with reset_buf set an
    armed env's episode enters the integer accumulator `acc` [TRACK_ACC] - with the final errors, predicates and finite test of `EpisodeStats` - while an
    env that was never armed (the tracker did not see the episode's first step) adds to UNARMED alone.  So a tracker created in the middle of episodes, or
    whose envs were reset underneath it, needs no protocol with the caller.
    `update()` accounts for the env step that has just run.  On the GPU the trainer calls `step_fused(...)` instead: ONE launch that also does the work of
    the launch it replaces (ppo_kernels.rollout_track).  The plain-torch statement serves CPU tensors and `fused=False`: the integers are identical and
    the return is summed in the same order.  `merge(group)` sums the accumulator over ranks, `take()` hands it out and clears it (no sync),
    `window_stats` turns integer vectors into the reported dict.  `episode_length` (for TIMEOUT) defaults to the engine's config; 0: no time limit."""

    buffers = ("reward", "reset_buf", "steps")
    acc_size = TRACK_ACC

    def __init__(self, engine, pos_tol=None, ori_tol=None, rule=None, fused=None, episode_length=None):
        super().__init__(engine, pos_tol, ori_tol, rule, fused, episode_length)
        n, dev = self.num_envs, self.acc.device
        if self.fused:
            self._scratch = torch.empty((3, n), dtype=torch.float32, device=dev)       # the outputs of a launch nobody asked outputs of (`update`)
        self.env_trk = torch.zeros((TRK_ROWS, n), dtype=torch.int32, device=dev)

    def reset_envs(self):
        """forget every running episode (the accumulator stays): after `restore()` and at the end of `evaluate()`"""
        self.env_trk.zero_()

    def step_fused(self, scale, rew_t, done=None, done_t=None, end_t=None, tout_t=None):
        """the ONE launch behind an env step: rew_t = reward * scale and, with `done`, done_t = float(done) (in place of ppo_kernels.rollout_reward) or
        end_t / tout_t (in place of ppo_kernels.rollout_flags) - and the tracker's update.  Fused trackers only."""
        if not self.fused:
            raise ValueError("step_fused on a tracker that runs the torch statement: call update()")
        from . import ppo_kernels as pk
        e = self.engine
        pk.rollout_track(e.state, e.reward, e.reset_buf, e.steps, self.env_trk, self.acc, scale, self.ep_len, self.pos_tol, self.ori_tol, self.rule,
                         rew_t, done=done, done_t=done_t, end_t=end_t, tout_t=tout_t)

    def _launch(self):
        s = self._scratch
        self.step_fused(1.0, s[0], end_t=s[1], tout_t=s[2])

    @torch.no_grad()
    def _update_torch(self):
        """the statement of include/trifinger_ppo_track.h in plain torch"""
        e, trk, acc = self.engine, self.env_trk, self.acc
        r = e.reward
        s = e.steps.to(torch.int64)
        ends = e.reset_buf.to(torch.bool)
        first = s == 1
        ret = torch.where(first, r, trk[TRK_RETURN].view(torch.float32) + r)
        armed = first | (trk[TRK_ARMED] != 0)
        e_p, e_o, pos_ok, ori_ok, at_goal, fin = episode_outcome(e.state, ret, self.pos_tol, self.ori_tol, self.rule)
        counted, nonfin, unarmed = ends & armed & fin, ends & armed & ~fin, ends & ~armed
        tout = (s >= self.ep_len) if self.ep_len > 0 else torch.zeros_like(ends)
        acc[T_EPISODES] += counted.sum()
        acc[T_SUCCESS] += (counted & at_goal).sum()
        acc[T_POS_OK] += (counted & pos_ok).sum()
        acc[T_ORI_OK] += (counted & ori_ok).sum()
        acc[T_TIMEOUT] += (counted & tout).sum()
        acc[T_SUM_LENGTH] += torch.where(counted, s, torch.zeros_like(s)).sum()
        acc[T_SUM_RETURN:T_SUM_ORI_ERR + 1] += torch.stack(fixed_sums(counted, ret, e_p, e_o))
        acc[T_NONFINITE] += nonfin.sum()
        acc[T_UNARMED] += unarmed.sum()
        trk[TRK_RETURN] = torch.where(ends, torch.zeros_like(ret), ret).view(torch.int32)
        trk[TRK_ARMED] = (armed & ~ends).to(torch.int32)

    def take(self):
        """the accumulator since the last take (int64 [TRACK_ACC], a device tensor of its own), cleared behind it; no host synchronisation"""
        v = self.acc.clone()
        self.acc.zero_()
        return v

    @staticmethod
    def window(vectors, games_to_track):
        """of epoch vectors in time order, the most recent ones with EPISODES > 0, taken whole, until their EPISODES reach `games_to_track`
        (returned in time order; empty before any episode has ended)"""
        out, n = [], 0
        for v in reversed(vectors):
            if int(v[T_EPISODES]) > 0:
                out.append([int(x) for x in v])
                n += out[-1][T_EPISODES]
                if n >= int(games_to_track):
                    break
        return out[::-1]

    @staticmethod
    def window_stats(vectors):
        """the reported dict of a window of integer vectors: their sum, as means and rates over its EPISODES.  Without an episode only
        {"episodes": 0}: no NaN goes into a log."""
        raw = [sum(int(v[k]) for v in vectors) for k in range(TRACK_ACC)]
        n = raw[T_EPISODES]
        if n <= 0:
            return {"episodes": 0}
        return {"episodes": n, "episode_return": raw[T_SUM_RETURN] / S_RETURN / n, "episode_length": raw[T_SUM_LENGTH] / n,
                "success_rate": raw[T_SUCCESS] / n, "pos_ok_rate": raw[T_POS_OK] / n, "ori_ok_rate": raw[T_ORI_OK] / n,
                "timeout_rate": raw[T_TIMEOUT] / n, "final_pos_err": raw[T_SUM_POS_ERR] / S_POS_ERR / n,
                "final_ori_err": raw[T_SUM_ORI_ERR] / S_ORI_ERR / n}
