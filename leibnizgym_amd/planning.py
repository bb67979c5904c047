"""Planning on the simulator: ctypes binding of include/trifinger_plan.h (libtrifinger_plan.so), its torch front end and the torch statements of its laws.

`fork_envs` copies the state of chosen envs of one engine into the envs of another (or the same) engine, whatever the two sizes; `MPPIPlanner` forks
the envs it controls into a population of scratch envs, rolls every copy forward under its own action sequence, weights the sequences by their
returns and returns the first action of the weighted mean: sampling-based model-predictive control (MPPI).  On a HIP engine the fork, the action
sampling and the update are one launch each around the engine's own step.

`fork_statement`, `noise_statement`, `rollout_actions_statement` and `update_statement` state the same laws in plain torch, with the operations of the
header in the header's order (integer Philox, the step's log / sin / cos polynomials with single-rounded fused multiply-adds): the specification the
kernels are held to (tests/test_planning_gpu.py) and what runs on a CPU engine.  An extension: the reference has no such interface.
"""
import ctypes as C
import os

import torch

from . import _capi as capi
from .engine import TrifingerEngine, fill_reward_terms
from .evaluate import _fma32, _sqrt32, engine_of

TFPL_API_VERSION = 1
TFPL_MAX_ACTION_DIM = 24
TFPL_MAX_HORIZON = 256
TFPL_MIN_SAMPLES, TFPL_MAX_SAMPLES = 64, 1024
TFPL_STD_TINY = 1e-12
TFPL_OK, TFPL_ERR_INVALID_ARG, TFPL_ERR_LAUNCH = 0, -1, -3
STAT_BEST, STAT_MEAN, STAT_ESS, STAT_STD, NUM_STATS = 0, 1, 2, 3, 4
TF_MAX_ENVS = 2097152
TF_OBS_DIM_BASE = 32

# the per-env buffers of an engine, in the order of TfBuffers (`info` and `scratch` are not per-env: a fork leaves them alone)
FORK_BUFFERS = ("state", "action_buf", "obs", "states", "reward", "reset_buf", "goal_reset_buf", "successes", "dones", "steps", "reset_count")


class TfplSide(C.Structure):
    _fields_ = [("buf", capi.TfBuffers), ("num_envs", C.c_int32), ("action_dim", C.c_int32), ("states_dim", C.c_int32)]


class TfplPlan(C.Structure):
    _fields_ = [("groups", C.c_int32), ("samples", C.c_int32), ("horizon", C.c_int32), ("action_dim", C.c_int32), ("seed", C.c_uint64),
                ("plan_counter", C.c_uint32), ("sigma", C.c_float), ("lo", C.c_float), ("hi", C.c_float), ("lam", C.c_float),
                ("normalize", C.c_int32), ("shift", C.c_int32)]


_P = C.c_void_p

# every symbol include/trifinger_plan.h declares: name -> (restype, argtypes)
SYMBOLS = {
    "tfpl_api_version": (C.c_int, []),
    "tfpl_last_error_string": (C.c_char_p, []),
    "tfpl_fork": (C.c_int, [C.POINTER(TfplSide), C.POINTER(TfplSide), _P, _P, _P]),
    "tfpl_rollout_actions": (C.c_int, [C.POINTER(TfplPlan), C.c_int32, _P, _P, _P, _P, _P, _P, _P, _P]),
    "tfpl_update": (C.c_int, [C.POINTER(TfplPlan), _P, _P, _P, _P, _P, _P, _P]),
}

_LIB = None


def library_path():
    return os.path.join(os.path.dirname(os.path.abspath(__file__)), "csrc", "libtrifinger_plan.so")


def load():
    """Load libtrifinger_plan.so (cached); works without a GPU.  Fails loudly when it has not been built."""
    global _LIB
    if _LIB is None:
        path = library_path()
        if not os.path.isfile(path):
            raise capi.TfLibraryError(f"native library not found: {path}. Build it with `make -C leibnizgym_amd/csrc`. There is no fallback path.")
        lib = C.CDLL(path)
        for name, (res, args) in SYMBOLS.items():
            try:
                fn = getattr(lib, name)
            except AttributeError as exc:
                raise capi.TfLibraryError(f"{path} does not export `{name}` declared in include/trifinger_plan.h") from exc
            fn.restype = res
            fn.argtypes = args
        if lib.tfpl_api_version() != TFPL_API_VERSION:
            raise capi.TfLibraryError(f"{path}: API version {lib.tfpl_api_version()} != {TFPL_API_VERSION}")
        _LIB = lib
    return _LIB


def _check(lib, rc, what):
    if rc == TFPL_OK:
        return
    text = (lib.tfpl_last_error_string() or b"").decode()
    exc = ValueError if rc == TFPL_ERR_INVALID_ARG else RuntimeError
    raise exc(f"{what}: status {rc} ({text})")


def side_of(engine):
    """the TfplSide of an engine: the addresses of its buffers as they are now (an engine whose buffers were re-bound is followed)"""
    s = TfplSide()
    for k in FORK_BUFFERS:
        t = getattr(engine, k)
        setattr(s.buf, k, t.data_ptr() if t.numel() else None)
    s.num_envs, s.action_dim, s.states_dim = engine.num_envs, engine.action_dim, engine.states_dim
    return s


def _stream(index):
    return _P(torch.cuda.current_stream(index).cuda_stream)


# ---- the fork ------------------------------------------------------------------------------------------------------------------------------------------
def fork_statement(dst, src, src_index):
    """THE fork in plain torch: env src_index[i] of `src` is copied into env i of `dst`, buffer by buffer (eleven gathers and eleven scatters); an index
    outside [0, N_src) leaves its env as it was.  -> the number of such indices (an int: this form synchronises)"""
    idx = src_index.to(torch.int64)
    ok = (idx >= 0) & (idx < src.num_envs)
    di = torch.nonzero(ok).reshape(-1)
    si = idx[di]
    for k in FORK_BUFFERS:
        d, s = getattr(dst, k), getattr(src, k)
        if d.numel() == 0:
            continue
        if k == "state":
            d[:, di] = s[:, si]
        else:
            d[di] = s[si]
    return int(idx.numel() - di.numel())


def fork_envs(dst, src, src_index, *, fused=None, validate=True, bad_count=None):
    """Copy env src_index[i] of `src` into env i of `dst`, for every env of `dst`: the state with the solver's warm start, the last action, observation,
    privileged state and reward, the four flags, the step and reset counters.  `dst`, `src`: engines, or envs with one behind them; their sizes may
    differ, their action and states widths may not.  src_index: int32 [N_dst] on the engines' device.

    fused None: the HIP launch (tfpl_fork) on a GPU engine, the torch statement on a CPU one; False forces the statement.  The launch reads nothing on
    the host: an index outside [0, N_src) skips its env and increments `bad_count` (an int32 tensor of one element on the device, or None).  The
    statement returns the count.

    `dst` and `src` may be the same engine only if every source is a fixed point of the map (src_index[src_index[i]] == src_index[i]); `validate`
    checks that with one torch expression (a synchronisation) and is the caller's to switch off.

    A fork equals its source only while no env-keyed draw happens: see MPPIPlanner."""
    dst, src = engine_of(dst), engine_of(src)
    if dst.action_dim != src.action_dim or dst.states_dim != src.states_dim:
        raise ValueError(f"fork: the engines differ in width: action_dim {dst.action_dim} / {src.action_dim}, states_dim {dst.states_dim} / {src.states_dim}")
    if dst.device != src.device:
        raise ValueError(f"fork: dst lives on {dst.device}, src on {src.device}")
    if not isinstance(src_index, torch.Tensor) or src_index.dtype != torch.int32 or tuple(src_index.shape) != (dst.num_envs,) \
            or src_index.device != dst.device or not src_index.is_contiguous():
        raise ValueError(f"src_index: a contiguous int32 tensor [{dst.num_envs}] on {dst.device}")
    if validate and dst.state.data_ptr() == src.state.data_ptr():
        idx = src_index.to(torch.int64)
        ok = (idx >= 0) & (idx < src.num_envs)
        if not bool((idx[idx.clamp(0, src.num_envs - 1)] == idx)[ok].all()):
            raise ValueError("fork within one engine: every source must be a fixed point of the map, src_index[src_index[i]] == src_index[i]")
    if fused is None:
        fused = dst.device.type == "cuda"
    if not fused:
        bad = fork_statement(dst, src, src_index)
        if bad_count is not None:
            bad_count += bad
        return bad
    if dst.device.type != "cuda":
        raise RuntimeError(f"the fork kernel runs only on an MI355X (got '{dst.device}'); fused=False runs the torch statement")
    lib = load()
    a, b = side_of(dst), side_of(src)
    with torch.cuda.device(dst.device.index):
        rc = lib.tfpl_fork(C.byref(a), C.byref(b), src_index.data_ptr(), None if bad_count is None else bad_count.data_ptr(), _stream(dst.device.index))
    _check(lib, rc, "tfpl_fork")
    return None


# ---- the noise -----------------------------------------------------------------------------------------------------------------------------------------
_M0, _M1, _W0, _W1, _MASK = 0xD2511F53, 0xCD9E8D57, 0x9E3779B9, 0xBB67AE85, 0xFFFFFFFF


def _mulhilo(m, c):
    """(high, low) 32-bit halves of m * c for a constant m < 2^32 and an int64 tensor c of values < 2^32, without leaving int64"""
    lo16, hi16 = c & 0xFFFF, c >> 16
    a, b = m * lo16, m * hi16                                           # both < 2^48
    mid = ((b & 0xFFFF) << 16) + a                                      # < 2^49
    return (b >> 16) + (mid >> 32), mid & _MASK


def philox4x32_10(c0, c1, c2, c3, k0, k1):
    """Philox4x32-10 on int64 tensors holding 32-bit words (k0, k1: Python ints) -> four int64 tensors: csrc/tf_device_math.h, word for word"""
    for _ in range(10):
        hi0, lo0 = _mulhilo(_M0, c0)
        hi1, lo1 = _mulhilo(_M1, c2)
        c0, c1, c2, c3 = hi1 ^ c1 ^ k0, lo1, hi0 ^ c3 ^ k1, lo0
        k0, k1 = (k0 + _W0) & _MASK, (k1 + _W1) & _MASK
    return c0, c1, c2, c3


def _u01(r):
    return (r >> 8).to(torch.float32) * 5.9604644775390625e-8


def step_log(x):
    """tf_log of csrc/tf_device_math.h operation for operation in float32, for positive normal x"""
    f = lambda v: torch.full_like(x, v)                                  # noqa: E731
    u = x.contiguous().view(torch.int32).to(torch.int64)
    e = ((u >> 23) & 0xFF) - 126
    m = ((u & 0x007FFFFF) | 0x3F000000).to(torch.int32).view(torch.float32)
    small = m < 0.707106781186547524
    e = torch.where(small, e - 1, e)
    m = torch.where(small, m + m - 1.0, m - 1.0)
    z = m * m
    y = f(7.0376836292e-2)
    for k in (-1.1514610310e-1, 1.1676998740e-1, -1.2420140846e-1, 1.4249322787e-1, -1.6668057665e-1, 2.0000714765e-1, -2.4999993993e-1, 3.3333331174e-1):
        y = _fma32(y, m, f(k))
    y = (y * m) * z
    fe = e.to(torch.float32)
    y = _fma32(fe, f(-2.12194440e-4), y)
    y = _fma32(f(-0.5), z, y)
    return _fma32(fe, f(0.693359375), m + y)


def step_sincos(x):
    """tf_sincos of csrc/tf_device_math.h operation for operation in float32 -> (sin, cos)"""
    f = lambda v: torch.full_like(x, v)                                  # noqa: E731
    k = torch.round(x * 0.63661977236758134)                              # rintf: ties to even
    n = k.to(torch.int64)
    r = _fma32(-k, f(1.5703125), x)
    r = _fma32(-k, f(4.837512969970703125e-4), r)
    r = _fma32(-k, f(7.54978995489188216e-8), r)
    z = r * r
    ps = _fma32(_fma32(f(-1.9515295891e-4), z, f(8.3321608736e-3)), z, f(-1.6666654611e-1))
    ps = _fma32(ps * z, r, r)
    pc = _fma32(_fma32(f(2.443315711809948e-5), z, f(-1.388731625493765e-3)), z, f(4.166664568298827e-2))
    pc = _fma32(pc * z, z, _fma32(f(-0.5), z, f(1.0)))
    q = n & 3
    odd = (q & 1) != 0
    s, c = torch.where(odd, pc, ps), torch.where(odd, ps, pc)
    return torch.where((q & 2) != 0, -s, s), torch.where((q == 1) | (q == 2), -c, c)


def _box_muller(ua, ub):
    rad = _sqrt32(-2.0 * step_log(1.0 - ua))
    s, c = step_sincos(6.2831855 * ub)
    return rad * c, rad * s


def noise_statement(env_index, h, action_dim, seed, plan_counter, samples):
    """eps(i, h, a) of include/trifinger_plan.h for the planner envs `env_index` (an integer tensor [n]) and the horizon step(s) `h` (an int, or an integer
    tensor [n]) -> float32 [n, action_dim]; sample 0 of every group (i % samples == 0) has eps = 0"""
    i = env_index.to(torch.int64)
    h = h.to(torch.int64) if isinstance(h, torch.Tensor) else torch.full_like(i, int(h))
    k0, k1 = int(seed) & _MASK, (int(seed) >> 32) & _MASK
    cols = []
    for q in range((action_dim + 3) // 4):
        b, k = divmod(q, 3)
        r = philox4x32_10(i, torch.full_like(i, int(plan_counter) & _MASK), 4 * h + k, torch.full_like(i, b), k0, k1)
        u = [_u01(x) for x in r]
        cols += list(_box_muller(u[0], u[1])) + list(_box_muller(u[2], u[3]))
    eps = torch.stack(cols[:action_dim], dim=1)
    return torch.where((i % samples == 0).unsqueeze(1), torch.zeros_like(eps), eps)


def applied_actions(p, U, h=None):
    """act(i, h, :) of the header for every planner env -> float32 [N, A]; h None: every horizon step at once, [N, H, A].  p: the parameter dict of
    `plan_params`; U: float32 [E, H, A]"""
    n, H, A = p["groups"] * p["samples"], p["horizon"], p["action_dim"]
    i = torch.arange(n, device=U.device)
    e = torch.div(i, p["samples"], rounding_mode="floor")
    if h is not None:
        eps = noise_statement(i, h, A, p["seed"], p["plan_counter"], p["samples"])
        return torch.clamp(U[e, h] + p["sigma"] * eps, p["lo"], p["hi"])
    ii, hh = i.repeat_interleave(H), torch.arange(H, device=U.device).repeat(n)
    eps = noise_statement(ii, hh, A, p["seed"], p["plan_counter"], p["samples"]).reshape(n, H, A)
    return torch.clamp(U[e] + p["sigma"] * eps, p["lo"], p["hi"])


def rollout_actions_statement(p, h, U, disc, reward, reset_buf, G, alive, action, acts=None):
    """tfpl_rollout_actions in plain torch, in place on G, alive (bool or uint8 [N]) and action.  acts: `applied_actions(p, U)` formed earlier from this U
    (the statement of a whole plan forms the noise once)"""
    if h == 0:
        G.zero_()
        alive.fill_(1)
    else:
        al = alive.to(torch.bool)
        G.copy_(torch.where(al, G + disc[h - 1] * reward, G))
        al = al & torch.isfinite(reward) & ~reset_buf.to(torch.bool)
        alive.copy_(al.to(alive.dtype))
    if h < p["horizon"]:
        action.copy_(applied_actions(p, U, h) if acts is None else acts[:, h])


def update_statement(p, G, U, dtype=torch.float32, acts=None):
    """tfpl_update in plain torch with the sums in `dtype` (the applied actions are the float32 bits in any case); U [E, H, A] is updated in place (rounded
    to its own dtype).  acts: as in rollout_actions_statement.  -> (first [E, A], w [E * S], stats [E, NUM_STATS], invalid [E]) in `dtype`"""
    E, S, H, A = p["groups"], p["samples"], p["horizon"], p["action_dim"]
    g = G.reshape(E, S).to(dtype)
    valid = torch.isfinite(g)
    nv = valid.sum(1).to(dtype)
    some = nv > 0
    nvs = torch.where(some, nv, torch.ones_like(nv))
    zero = torch.zeros_like(g)
    gmax = torch.where(valid, g, torch.full_like(g, -float("inf"))).max(1).values
    gmax = torch.where(some, gmax, torch.zeros_like(gmax))
    mean = torch.where(valid, g, zero).sum(1) / nvs
    dev = torch.where(valid, g - mean[:, None], zero)
    sd = torch.sqrt((dev * dev).sum(1) / nvs)
    T = p["lam"] * torch.clamp(sd, min=TFPL_STD_TINY) if p["normalize"] else torch.full_like(sd, p["lam"])
    ez = torch.where(valid, torch.exp((torch.where(valid, g, zero) - gmax[:, None]) / T[:, None]), zero)
    w = ez / torch.where(some, ez.sum(1), torch.ones_like(nv))[:, None]
    acts = (applied_actions(p, U.to(torch.float32)) if acts is None else acts).reshape(E, S, H, A).to(dtype)
    new = (w[:, :, None, None] * acts).sum(1)                                                     # [E, H, A]
    old = U.to(dtype)
    new = torch.where(some[:, None, None], new, old)
    first = new[:, 0].clone()
    out = torch.cat([new[:, 1:], new[:, -1:]], dim=1) if p["shift"] else new
    U.copy_(torch.where(some[:, None, None], out, old).to(U.dtype))
    ess = torch.where(some, 1.0 / torch.where(some, (w * w).sum(1), torch.ones_like(nv)), torch.zeros_like(nv))
    stats = torch.stack([gmax, torch.where(some, mean, torch.zeros_like(mean)), ess, torch.where(some, sd, torch.zeros_like(sd))], dim=1)
    return first, w.reshape(-1), stats, (S - valid.sum(1)).to(torch.int32)


def plan_params(groups, samples, horizon, action_dim, *, sigma, lam, seed=0, plan_counter=0, lo=-1.0, hi=1.0, normalize=True, shift=True):
    """A TfplPlan and the same values as a dict for the statements (the float32 values the kernels see); ValueError by name"""
    if not (isinstance(samples, int) and TFPL_MIN_SAMPLES <= samples <= TFPL_MAX_SAMPLES and samples % 64 == 0):
        raise ValueError(f"samples: a multiple of 64 in [{TFPL_MIN_SAMPLES}, {TFPL_MAX_SAMPLES}], got {samples!r}")
    if not (isinstance(groups, int) and groups >= 1 and groups * samples <= TF_MAX_ENVS):
        raise ValueError(f"groups: >= 1 with groups * samples <= {TF_MAX_ENVS}, got {groups!r}")
    if not (isinstance(horizon, int) and 1 <= horizon <= TFPL_MAX_HORIZON):
        raise ValueError(f"horizon: 1..{TFPL_MAX_HORIZON}, got {horizon!r}")
    if not 1 <= action_dim <= TFPL_MAX_ACTION_DIM:
        raise ValueError(f"action_dim: 1..{TFPL_MAX_ACTION_DIM}, got {action_dim!r}")
    if not float(sigma) >= 0.0:
        raise ValueError(f"sigma: >= 0, got {sigma!r}")
    if not float(lam) > 0.0:
        raise ValueError(f"lam: > 0, got {lam!r}")
    if not float(lo) <= float(hi):
        raise ValueError(f"lo <= hi, got {(lo, hi)}")
    c = TfplPlan(groups, samples, horizon, int(action_dim), int(seed) & 0xFFFFFFFFFFFFFFFF, int(plan_counter) & _MASK, float(sigma), float(lo), float(hi),
                 float(lam), int(bool(normalize)), int(bool(shift)))
    d = dict(groups=groups, samples=samples, horizon=horizon, action_dim=int(action_dim), seed=int(c.seed), plan_counter=int(c.plan_counter),
             sigma=float(c.sigma), lo=float(c.lo), hi=float(c.hi), lam=float(c.lam), normalize=bool(normalize), shift=bool(shift))
    return c, d


# ---- the planner -----------------------------------------------------------------------------------------------------------------------------------------
ROLLOUT_ENV_ID_OFFSET = 1 << 24          # the planner's scratch envs carry ids of their own, away from any plant's


class MPPIPlanner:
    """Sampling-based model-predictive control on a population of forked envs.

    For E plant envs the planner owns a rollout engine of E * `samples` envs built from the plant's configuration: the same model, command mode,
    observation layout and domain-randomisation ranges, with `episode_length` 0, no observation noise, no action repeat and env ids of its own;
    `rollout_overrides` (``{"reward_terms": {...}, "success": {...}}``) replaces the reward terms or the success bonus there - the planner's cost is the
    planner's own affair.  `plan()` forks every plant env into its `samples` copies, rolls them `horizon` steps forward under the nominal sequence
    plus Gaussian noise of deviation `sigma` (sample 0: the nominal sequence itself), weights the samples of each plant env by
    softmax((G - max G) / (lam * std G)) of their discounted returns (`normalize` False: lam alone) and returns the weighted mean of the first
    actions, [E, A]; the rest of the mean, shifted by one step, is the next nominal sequence.  `iterations` > 1 repeats that on the same state.
    Everything runs on the engine's stream without a host synchronisation: one launch each for the fork, the sampling in front of every step
    and the update (`fused`; the torch statements on a CPU engine or with fused=False).  `lib`: the step library of the rollout engine (default:
    the plant's).

    Two limits.  A fork equals its source only while no env-keyed draw happens: a reset, observation noise or action repeat are drawn per env id,
    so the rollout engine switches the latter two off, and a copy whose episode ends inside the horizon stops collecting reward there instead of
    living through a reset the plant would not see.  And the action planned for a plant env that is already flagged for reset is wasted: the
    plant resets that env at the start of its next step."""

    def __init__(self, plant, *, samples, horizon, sigma, lam, gamma=1.0, normalize=True, iterations=1, seed=0, rollout_overrides=None, fused=None,
                 lib=None, action_low=-1.0, action_high=1.0):
        self._plant_obj = plant
        self.plant = engine_of(plant)
        pe = self.plant
        self.device = pe.device
        self.fused = (self.device.type == "cuda") if fused is None else bool(fused)
        if self.fused and self.device.type != "cuda":
            raise RuntimeError(f"the planning kernels run only on an MI355X (got '{self.device}'); fused=False runs the torch statements")
        if not (isinstance(iterations, int) and iterations >= 1):
            raise ValueError(f"iterations: an integer >= 1, got {iterations!r}")
        if not 0.0 < float(gamma) <= 1.0:
            raise ValueError(f"gamma: in (0, 1], got {gamma!r}")
        self.groups, self.samples, self.horizon, self.iterations, self.gamma = pe.num_envs, samples, horizon, iterations, float(gamma)
        self._cfg_args = dict(sigma=sigma, lam=lam, seed=seed, lo=action_low, hi=action_high, normalize=normalize)
        plan_params(self.groups, samples, horizon, pe.action_dim, **self._cfg_args)                # validates
        n = self.groups * samples
        cfg = capi.TfConfig.from_buffer_copy(pe.cfg)
        cfg.num_envs = n
        cfg.env_id_offset = ROLLOUT_ENV_ID_OFFSET
        cfg.seed = (int(seed) ^ 0x9E3779B97F4A7C15) & 0xFFFFFFFFFFFFFFFF
        cfg.episode_length = 0
        cfg.dr_obs_noise = 0.0
        cfg.dr_action_repeat = 0.0
        over = dict(rollout_overrides or {})
        unknown = sorted(set(over) - {"reward_terms", "success"})
        if unknown:
            raise ValueError(f"rollout_overrides: unknown key(s) {unknown}; known: ['reward_terms', 'success']")
        if "reward_terms" in over:
            fill_reward_terms(cfg, over["reward_terms"])
        for k, v in dict(over.get("success", {})).items():
            field = {"activate": "success_activate", "bonus": "success_bonus", "position_tolerance": "position_tolerance",
                     "orientation_tolerance": "orientation_tolerance"}[k]
            setattr(cfg, field, int(bool(v)) if k == "activate" else float(v))
        self.rollout = TrifingerEngine(cfg, device=self.device, lib=lib if lib is not None else pe.lib)
        dev, f32 = self.device, dict(dtype=torch.float32, device=self.device)
        A = pe.action_dim
        self.src_index = torch.div(torch.arange(n, device=dev), samples, rounding_mode="floor").to(torch.int32)
        self.U = torch.zeros((self.groups, horizon, A), **f32)
        self.disc = torch.tensor([self.gamma ** h for h in range(horizon)], **f32)
        self.G = torch.zeros((n,), **f32)
        self.alive = torch.zeros((n,), dtype=torch.uint8, device=dev)
        self.action = torch.zeros((n, A), **f32)
        self.first = torch.zeros((self.groups, A), **f32)
        self.weights = torch.zeros((n,), **f32)
        self._stats = torch.zeros((self.groups, NUM_STATS), **f32)
        self.invalid = torch.zeros((self.groups,), dtype=torch.int32, device=dev)
        self.bad_forks = torch.zeros((1,), dtype=torch.int32, device=dev)
        self.plan_counter = 0
        self._lib = load() if self.fused else None

    def close(self):
        self.rollout.close()

    def _params(self, shift):
        return plan_params(self.groups, self.samples, self.horizon, self.plant.action_dim, plan_counter=self.plan_counter, shift=shift, **self._cfg_args)

    def _rollout_actions(self, c, d, h):
        r = self.rollout
        if not self.fused:
            if h == 0:
                self._acts = applied_actions(d, self.U)
            rollout_actions_statement(d, h, self.U, self.disc, r.reward, r.reset_buf, self.G, self.alive, self.action, acts=self._acts)
            return
        rc = self._lib.tfpl_rollout_actions(C.byref(c), h, self.U.data_ptr(), self.disc.data_ptr(), r.reward.data_ptr(), r.reset_buf.data_ptr(),
                                            self.G.data_ptr(), self.alive.data_ptr(), self.action.data_ptr(), _stream(self.device.index))
        _check(self._lib, rc, "tfpl_rollout_actions")

    def _update(self, c, d):
        if not self.fused:
            first, w, stats, invalid = update_statement(d, self.G, self.U, acts=self._acts)
            self.first.copy_(first)
            self.weights.copy_(w)
            self._stats.copy_(stats)
            self.invalid.copy_(invalid)
            return
        rc = self._lib.tfpl_update(C.byref(c), self.G.data_ptr(), self.U.data_ptr(), self.first.data_ptr(), self.weights.data_ptr(), self._stats.data_ptr(),
                                   self.invalid.data_ptr(), _stream(self.device.index))
        _check(self._lib, rc, "tfpl_update")

    def plan(self):
        """-> [E, A]: the action to apply to every plant env now (the planner's own tensor: copy it to keep it across calls)"""
        ctx = torch.cuda.device(self.device.index) if self.fused else _NO_CTX
        with ctx:
            for it in range(self.iterations):
                c, d = self._params(shift=it == self.iterations - 1)
                fork_envs(self.rollout, self.plant, self.src_index, fused=self.fused, validate=False, bad_count=self.bad_forks if self.fused else None)
                self.rollout.frame_count = self.plant.frame_count                 # reward schedules are keyed by the frame count
                for h in range(self.horizon):
                    self._rollout_actions(c, d, h)
                    self.rollout.step(self.action)
                self._rollout_actions(c, d, self.horizon)
                self._update(c, d)
                self.plan_counter += 1
        return self.first

    def act(self):
        """plan, then step the plant with the planned action -> (the action, what the plant's `step` returned)"""
        a = self.plan()
        return a, self._plant_obj.step(a)

    def stats(self):
        """per plant env, of the last update: best and mean return of its samples, effective sample size 1 / sum w^2, std of the returns, the number of
        invalid samples; and the weights and returns of all samples, [E, S].  Device tensors: nothing synchronises until they are read."""
        s = self._stats
        return dict(best=s[:, STAT_BEST], mean=s[:, STAT_MEAN], ess=s[:, STAT_ESS], std=s[:, STAT_STD], invalid=self.invalid,
                    weights=self.weights.view(self.groups, self.samples), returns=self.G.view(self.groups, self.samples))

    def reset_plan(self, mask=None):
        """zero the nominal sequence of the plant envs in `mask` (bool [E]; default: those whose episode just ended, the plant's reset_buf)"""
        mask = self.plant.reset_buf if mask is None else mask
        self.U.copy_(torch.where(mask.to(torch.bool).view(-1, 1, 1), torch.zeros_like(self.U), self.U))


class _NoCtx:
    def __enter__(self):
        return None

    def __exit__(self, *exc):
        return False


_NO_CTX = _NoCtx()
