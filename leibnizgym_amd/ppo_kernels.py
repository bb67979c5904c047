"""ctypes binding and autograd wrapper of the trainer's hand-written HIP kernel (leibnizgym_amd/csrc/ppo_kernels.hip).

`fused_ppo_loss` evaluates the whole PPO objective and its gradients in ONE launch (the eager form is ~60 elementwise and
reduction launches forwards and backwards).  It launches on torch's current stream.  GPU only: the CPU tests of the trainer run its plain-torch form, which is also the fp32
reference the GPU tests compare the kernel with (tests/test_ppo_kernels.py).

Tried and dropped (measured on MI355X, batch 8192): a fused ELU-derivative + bias-gradient backward kernel - the column sums
need either ~50 k atomics on 400 addresses (28 us, twice torch's two launches) or a second pass; not worth 2 % of the step."""
import ctypes as C
import os

import torch

_LIB = None
_F = C.POINTER(C.c_float)


def library_path():
    return os.path.join(os.path.dirname(os.path.abspath(__file__)), "csrc", "libtrifinger_ppo.so")


_P, _I, _L, _R = C.c_void_p, C.c_int32, C.c_int64, C.c_float
_LOSS = [_P] * 8 + [_I, _I] + [_R] * 4 + [_P] * 6          # the objective; its clip variants take old_v behind `ret`
_WALK = [_P, _I, _I, _P]
# every entry point the binding calls: name -> argument types (include/trifinger_ppo*.h).  All return int but tfp_moments_part_doubles (int64)
_ARGTYPES = {
    # include/trifinger_ppo.h
    "tfp_api_version": [], "tfp_reset_state": [_P], "tfp_ppo_loss": _LOSS,
    "tfp_clip_adam": [_P] * 4 + [_I, _I] + [_P] * 3 + [_R] * 5 + [_P],
    "tfp_linear_fwd": [_P] * 4 + [_I] * 4 + [_P], "tfp_gemm_nn": [_P] * 4 + [_I] * 3 + [_P], "tfp_gemm_nn_dz": [_P] * 5 + [_I] * 3 + [_P],
    "tfp_gemm_tn_bias": [_P] * 6 + [_I] * 4 + [_P], "tfp_gemm_tn_partials": [_P] * 4 + [_I] * 4 + [_P],
    "tfp_linear_fwd_group": [_P] * 7 + [_I, _I, _P], "tfp_gemm_nn_group": [_P] * 7 + [_I, _P], "tfp_gemm_nn_dz_group": [_P] * 8 + [_I, _P],
    "tfp_gemm_tn_partials_group": [_P] * 7 + [_I, _I, _P], "tfp_sum_partials_multi": [_P] * 6 + [_I, _P],
    "tfp_gemm_tn_partials_direct_chunk": [], "tfp_gemm_tn_partials_direct": [_P] * 6 + [_I, _P],
    "tfp_rollout_record": [_P, _I, _P, _I] + [_P] * 5 + [_I, _I] + [_P] * 7, "tfp_rollout_reward": [_P, _P, _R, _I, _P, _P, _P],
    "tfp_gae": [_P] * 3 + [_R, _R, _I, _I, _P, _P, _P], "tfp_gather_rows": [_P] * 3 + [_I, _P, _I, _P],
    "tfp_mlp_forward": _WALK, "tfp_mlp_backward": _WALK,
    # input normalisation (include/trifinger_ppo_norm.h: csrc/ppo_norm.hip and the walk variant)
    "tfp_moments_part_doubles": [_P, _I, _I], "tfp_moments": [_P, _P, _I, _I, _P, _L, _P, _P], "tfp_norm_merge": [_P] * 3 + [_I] * 3 + [_P] * 3,
    "tfp_gather_rows_norm": [_P] * 6 + [_I, _P, _I, _P], "tfp_mlp_forward_norm": [_P, _P, _I, _I, _P],
    # the value side (include/trifinger_ppo_value.h)
    "tfp_ppo_loss_vclip": [_P] + _LOSS, "tfp_gae_vnorm": [_P] * 5 + [_R, _R, _R, _I, _I] + [_P] * 5,
    # the network-shape keys (include/trifinger_ppo_net.h: activation codes, d2rl)
    "tfp_net_forward": _WALK, "tfp_net_backward": _WALK, "tfp_net_fits": [_P, _I, _I],
    # the checkpoint evaluator (include/trifinger_ppo_eval.h: csrc/tf_eval.hip)
    "tfp_eval_step": [_P] * 7 + [_I, _R, _R, _I, _I, _P], "tfp_eval_test_predicates": [_P, _I, _R, _R, _P, _P],
    # episode ends (include/trifinger_ppo_episode.h)
    "tfp_rollout_flags": [_P] * 3 + [_R, _L, _I] + [_P] * 4, "tfp_gae_ends": [_P] * 5 + [_I, _P, _P, _R, _R, _R, _I, _I] + [_P] * 6,
    "tfp_ppo_loss_w": _LOSS, "tfp_ppo_loss_vclip_w": [_P] + _LOSS,
    # the training-time episode tracker and the episode flight recorder (include/trifinger_ppo_track.h, include/trifinger_ppo_record.h: csrc/tf_eval.hip)
    "tfp_rollout_track": [_P, _P], "tfp_record_step": [_P, _P],
    # symmetry augmentation (include/trifinger_ppo_symmetry.h: csrc/ppo_symmetry.hip and the KL-row variant of the objective)
    "tfp_gather_rows_sym": [_P] * 7 + [_I, _P, _I, _P], "tfp_ppo_loss_sym": [_P] * 9 + [_I] * 4 + [_R] * 4 + [_P] * 6,
    # training diagnostics (include/trifinger_ppo_diag.h: the DIAG variants of the objective and of the optimiser, the record behind their arguments)
    "tfp_ppo_loss_diag": [_P] * 9 + [_I] * 4 + [_R] * 4 + [_P] * 7, "tfp_clip_adam_diag": [_P] * 4 + [_I, _I] + [_P] * 3 + [_R] * 5 + [_P, _P],
    # `mixed_precision` (include/trifinger_ppo_mixed.h: the walk and the direct weight-gradient kernel with bf16 operands)
    "tfp_net_forward_bf16": _WALK, "tfp_net_backward_bf16": _WALK, "tfp_net_fits_bf16": [_P, _I, _I], "tfp_gemm_tn_partials_direct_bf16": [_P] * 6 + [_I, _P],
}
# launches per entry point of the three product kernels - the walk forwards and backwards, the direct weight gradients - since import: which tier ran a
# network (the tests of `mixed_precision` read them: the bf16 names advance, the fp32 walk's do not); `n_mixed_dw_torch`: weight-gradient groups the direct
# bf16 kernel declined, formed as torch products of the rounded operands
n_calls = {}


def _count(name):
    n_calls[name] = n_calls.get(name, 0) + 1


def bf16r(t):
    """t rounded to bfloat16 (round to nearest even) and read back in its own type: the operand rounding of `mixed_precision` (ppo._MixedLinear)"""
    return t.to(torch.bfloat16).to(t.dtype)


def load():
    """the library with every entry point of `_ARGTYPES` bound BY SYMBOL: a library built before one of them fails here, not with a fall-back"""
    global _LIB
    if _LIB is None:
        path = library_path()
        if not os.path.isfile(path):
            raise RuntimeError(f"{path} is missing: build it with `make -C leibnizgym_amd/csrc` (python __graft_entry__.py)")
        lib = C.CDLL(path)
        for name, argtypes in _ARGTYPES.items():
            fn = getattr(lib, name)
            fn.restype, fn.argtypes = (C.c_int64 if name == "tfp_moments_part_doubles" else C.c_int), argtypes
        _LIB = lib
    return _LIB


def _stream(t):
    return C.c_void_p(torch.cuda.current_stream(t.device).cuda_stream)


def _chk(rc, what):
    if rc != 0:
        raise RuntimeError(f"{what} failed with status {rc}")


class _FusedPPOLoss(torch.autograd.Function):
    @staticmethod
    def forward(ctx, mu, log_std, v, act, old_nlp, adv, ret, old_mu, stats, e_clip, v_coef, ent_coef, bounds_coef):
        loss, d_mu, d_v, d_ls = ppo_loss_and_grads(mu, log_std, v, act, old_nlp, adv, ret, old_mu, stats, e_clip, v_coef, ent_coef, bounds_coef)
        ctx.save_for_backward(d_mu, d_v, d_ls)
        return loss

    @staticmethod
    def backward(ctx, g):
        d_mu, d_v, d_ls = ctx.saved_tensors
        return d_mu * g, d_ls * g, d_v * g, None, None, None, None, None, None, None, None, None, None


# the objective's entry point by (old_v given, adv_w given); the clip variants take old_v behind `ret`
_LOSS_ENTRY = {(False, False): "tfp_ppo_loss", (True, False): "tfp_ppo_loss_vclip", (False, True): "tfp_ppo_loss_w", (True, True): "tfp_ppo_loss_vclip_w"}


DIAG_N, DIAG_RATIO_MIN, DIAG_RATIO_MIN_CLEAR = 16, 8, 0x7F800000        # include/trifinger_ppo_diag.h: the record, and the one slot whose cleared state is not 0


def new_diag(device):
    """a cleared diagnostics record: int64 [DIAG_N] on the device"""
    rec = torch.zeros(DIAG_N, dtype=torch.int64, device=device)
    rec[DIAG_RATIO_MIN] = DIAG_RATIO_MIN_CLEAR
    return rec


def _diag_ok(diag, like):
    return diag.dtype == torch.int64 and diag.is_contiguous() and diag.numel() == DIAG_N and diag.device == like.device


def ppo_loss_and_grads(mu, log_std, v, act, old_nlp, adv, ret, old_mu, stats, e_clip, v_coef, ent_coef, bounds_coef, d_ls_out=None, old_v=None, adv_w=None,
                       kl_rows=None, diag=None):
    """(loss, d loss / d mu, d loss / d v, d loss / d log_std) straight from the kernel - for a caller that starts the backward pass at
    the network outputs itself (`torch.autograd.backward((mu, v), (d_mu, d_v))`), without a loss node multiplying them by one.
    `old_v` [B] (the value recorded in the rollout): the value term is clipped around it with the surrogate's `e_clip` (tfp_ppo_loss_vclip: `clip_value`).
    `adv_w` [B, 2] = (adv_i, w_i) interleaved (`episode_ends`; `adv` is then None): every per-sample term and gradient times w_i, the divisor stays B
    (tfp_ppo_loss_w / tfp_ppo_loss_vclip_w, include/trifinger_ppo_episode.h).
    `kl_rows` (`symmetry_augmentation`; 1 .. B): the KL statistic sums over the first kl_rows rows alone and is divided by kl_rows, everything else is
    untouched (tfp_ppo_loss_sym, include/trifinger_ppo_symmetry.h: ONE entry point for the four cases above; with kl_rows == B their bits).
    `diag` (`diagnostics`; int64 [DIAG_N] on the device, `new_diag`): the launch is tfp_ppo_loss_diag (include/trifinger_ppo_diag.h: ONE entry point for
    all of the above) and adds what it saw to slots 0-8 of the record; every output is what it is without the record"""
    lib = load()
    mu, v = mu.contiguous(), v.contiguous()
    B, A = mu.shape
    if adv_w is not None:
        assert adv is None and adv_w.dtype == torch.float32 and adv_w.is_contiguous() and tuple(adv_w.shape) == (B, 2) and adv_w.device == mu.device
        adv = adv_w
    if old_v is not None:
        assert old_v.dtype == torch.float32 and old_v.is_contiguous() and old_v.numel() == B and old_v.device == mu.device
    d_mu, d_v = torch.empty_like(mu), torch.empty_like(v)
    out = torch.empty(A + 1, device=mu.device, dtype=torch.float32)      # d_logstd [A] and the loss
    d_ls, loss = (out[:A] if d_ls_out is None else d_ls_out), out[A]      # d_ls_out: e.g. the parameter's slot of a flat gradient buffer
    if kl_rows is not None and not 1 <= int(kl_rows) <= B:
        raise ValueError(f"kl_rows = {kl_rows}: the KL statistic needs between 1 and B = {B} rows")
    if diag is not None:
        assert _diag_ok(diag, mu), "the diagnostics record is int64 [16], contiguous, on the device of the minibatch"
        _chk(lib.tfp_ppo_loss_diag(mu.data_ptr(), log_std.data_ptr(), act.data_ptr(), old_nlp.data_ptr(), adv.data_ptr(), old_mu.data_ptr(), v.data_ptr(),
                                   ret.data_ptr(), old_v.data_ptr() if old_v is not None else None, 1 if adv_w is not None else 0,
                                   int(kl_rows) if kl_rows is not None else 0, B, A, float(e_clip), float(v_coef), float(ent_coef), float(bounds_coef),
                                   d_mu.data_ptr(), d_v.data_ptr(), d_ls.data_ptr(), loss.data_ptr(), stats.data_ptr(), _stream(mu), diag.data_ptr()),
             "tfp_ppo_loss_diag")
        return loss, d_mu, d_v, d_ls
    if kl_rows is not None:
        _chk(lib.tfp_ppo_loss_sym(mu.data_ptr(), log_std.data_ptr(), act.data_ptr(), old_nlp.data_ptr(), adv.data_ptr(), old_mu.data_ptr(), v.data_ptr(),
                                  ret.data_ptr(), old_v.data_ptr() if old_v is not None else None, 1 if adv_w is not None else 0, int(kl_rows), B, A,
                                  float(e_clip), float(v_coef), float(ent_coef), float(bounds_coef), d_mu.data_ptr(), d_v.data_ptr(), d_ls.data_ptr(),
                                  loss.data_ptr(), stats.data_ptr(), _stream(mu)), "tfp_ppo_loss_sym")
        return loss, d_mu, d_v, d_ls
    name = _LOSS_ENTRY[old_v is not None, adv_w is not None]
    _chk(getattr(lib, name)(mu.data_ptr(), log_std.data_ptr(), act.data_ptr(), old_nlp.data_ptr(), adv.data_ptr(), old_mu.data_ptr(), v.data_ptr(), ret.data_ptr(),
                            *((old_v.data_ptr(),) if old_v is not None else ()), B, A, float(e_clip), float(v_coef), float(ent_coef), float(bounds_coef),
                            d_mu.data_ptr(), d_v.data_ptr(), d_ls.data_ptr(), loss.data_ptr(), stats.data_ptr(), _stream(mu)), name)
    return loss, d_mu, d_v, d_ls


def reset_state(device="cuda:0"):
    """the zero state of the objective kernel's accumulators (only after a launch of it was aborted: a completed one leaves them clean)"""
    _chk(load().tfp_reset_state(C.c_void_p(torch.cuda.current_stream(torch.device(device)).cuda_stream)), "tfp_reset_state")


def fused_ppo_loss(mu, log_std, v, act, old_nlp, adv, ret, old_mu, stats, e_clip, v_coef, ent_coef, bounds_coef):
    """loss (0-d tensor with grad); `stats` [4] accumulates (loss, a_loss, c_loss, kl) of the call.  All float32, contiguous,
    on one GPU; `act`, `old_nlp`, `adv`, `ret`, `old_mu` are data (no gradient)."""
    return _FusedPPOLoss.apply(mu, log_std, v, act, old_nlp, adv, ret, old_mu, stats, float(e_clip), float(v_coef), float(ent_coef),
                               float(bounds_coef))


class FlatClipAdam:
    """Gradient-norm truncation + Adam for two parameter groups over ONE flat buffer, two hand-written launches per step
    (csrc/ppo_kernels.hip: tfp_clip_adam) instead of torch's multi-tensor clip + two fused-Adam launches (~110 us for the 32
    small tensors of the two MLPs).  Same arithmetic as `torch.nn.utils.clip_grad_norm_` per group followed by `torch.optim.Adam`
    (no weight decay, no amsgrad).  The parameters are re-pointed to views of the flat buffer (their values are kept); learning
    rates and the step counter live on the device (no host value enters a launch)."""

    def __init__(self, group0, group1, lr0, lr1, max_norm0, max_norm1, betas=(0.9, 0.999), eps=1e-8):
        params = list(group0) + list(group1)
        dev = params[0].device
        self.params = params
        # every parameter starts on a 16-byte boundary of the flat buffer (the forward GEMM reads weight rows with dwordx4 loads); the
        # padding floats are zero, receive zero gradients and are never read by the networks
        al = lambda n: (n + 3) & ~3  # noqa: E731
        self.offsets, off = [], 0
        for k, p in enumerate(params):
            if k == len(list(group0)):
                self.n0 = off
            self.offsets.append(off)
            off += al(p.numel())
        if not list(group1):
            self.n0 = off
        self.n1 = off
        self.flat_p = torch.zeros(off, device=dev, dtype=torch.float32)
        for p, o in zip(params, self.offsets):             # parameters become views of the flat buffer
            self.flat_p[o:o + p.numel()].copy_(p.detach().reshape(-1))
            p.data = self.flat_p[o:o + p.numel()].view_as(p)
        self.flat_g = torch.zeros_like(self.flat_p)
        self.m, self.v = torch.zeros_like(self.flat_p), torch.zeros_like(self.flat_p)
        self.step_count = torch.zeros(2, device=dev)            # (this step, completed steps): include/trifinger_ppo.h
        self.lr = torch.tensor([float(lr0), float(lr1)], device=dev)
        self.sq = torch.zeros(4, device=dev)                    # two halves used by alternate steps; the kernels keep the next one clear
        self.max_norms, self.betas, self.eps = (float(max_norm0), float(max_norm1)), betas, float(eps)

    def set_lr(self, group, value):
        self.lr[group] = float(value)

    def grad_view(self, p):
        """the slot of parameter `p` in the flat gradient buffer, shaped like `p` (the MFMA linear layers write their weight and bias
        gradients straight into it)"""
        k = next(i for i, q in enumerate(self.params) if q is p)
        return self.flat_g[self.offsets[k]:self.offsets[k] + p.numel()].view_as(p)

    def gather_grads(self):
        """gradients that autograd left in `.grad` -> their slots (one multi-tensor copy); the layers that wrote their slots
        themselves have `.grad` None"""
        dst, src = [], []
        for p, o in zip(self.params, self.offsets):
            if p.grad is not None:
                dst.append(self.flat_g[o:o + p.numel()])
                src.append(p.grad.reshape(-1))
        if dst:
            torch._foreach_copy_(dst, src)
        return self.flat_g

    def step(self, gathered=False, diag=None):
        """`diag` (int64 [DIAG_N] on the device): tfp_clip_adam_diag - the same two launches, slots 9-15 of the record updated on the side"""
        if not gathered:
            self.gather_grads()
        if diag is not None:
            assert _diag_ok(diag, self.flat_p), "the diagnostics record is int64 [16], contiguous, on the optimiser's device"
            _chk(load().tfp_clip_adam_diag(self.flat_p.data_ptr(), self.flat_g.data_ptr(), self.m.data_ptr(), self.v.data_ptr(), self.n0, self.n1,
                                           self.sq.data_ptr(), self.step_count.data_ptr(), self.lr.data_ptr(), self.max_norms[0], self.max_norms[1],
                                           self.betas[0], self.betas[1], self.eps, _stream(self.flat_p), diag.data_ptr()), "tfp_clip_adam_diag")
            return
        _chk(load().tfp_clip_adam(self.flat_p.data_ptr(), self.flat_g.data_ptr(), self.m.data_ptr(), self.v.data_ptr(), self.n0, self.n1,
                                  self.sq.data_ptr(), self.step_count.data_ptr(), self.lr.data_ptr(), self.max_norms[0], self.max_norms[1],
                                  self.betas[0], self.betas[1], self.eps, _stream(self.flat_p)), "tfp_clip_adam")

    def snapshot(self):
        return self.m.clone(), self.v.clone(), self.step_count.clone()

    def restore_snapshot(self, snap):
        self.m.copy_(snap[0]); self.v.copy_(snap[1]); self._set_step(snap[2])

    def state_dict(self):
        return {"kind": "flat_clip_adam", "m": self.m.clone(), "v": self.v.clone(), "step": self.step_count[1:2].clone(), "lr": self.lr.clone()}

    def _set_step(self, t):
        """continue from `t` completed steps (a 1-element tensor, or the two-slot counter of a snapshot)"""
        self.step_count.fill_(float(t.reshape(-1)[-1]))
        self.sq.zero_()

    def load_state_dict(self, sd):
        if sd.get("kind") != "flat_clip_adam" or sd["m"].numel() != self.m.numel():
            raise ValueError("optimizer state of another kind / size")
        self.m.copy_(sd["m"]); self.v.copy_(sd["v"]); self._set_step(sd["step"]); self.lr.copy_(sd["lr"])


# ---- fp32 MFMA GEMMs of the two MLPs (csrc/ppo_kernels.hip: k_gemm) --------------------------------------------------------------
def linear_fwd(x, w, b, act):
    """act(x @ w.T + b) for contiguous float32 x [M, K], w [N, K], b [N]; act: 0 none, 1 ELU (the per-layer launches know no other activation)"""
    if int(act) not in (0, 1):
        raise ValueError(f"the per-layer kernels apply ELU or nothing, not activation code {act}: such a network runs on the network walk or on torch")
    M, K = x.shape
    N = w.shape[0]
    y = torch.empty(M, N, device=x.device, dtype=torch.float32)
    _chk(load().tfp_linear_fwd(x.data_ptr(), w.data_ptr(), b.data_ptr(), y.data_ptr(), M, N, K, int(act), _stream(x)), "tfp_linear_fwd")
    return y


def gemm_nn(a, b, y=None, y_out=None):
    """((a * elu'(y)) @ b) * elu'(y_out)  (y: the ELU output the gradient a belongs to, or None; y_out: the ELU output of the layer the product is the
    gradient of, or None - with it the result is that layer's dZ, ready for its own two products without a factor in their operand loads)"""
    M, K = a.shape
    N = b.shape[1]
    c = torch.empty(M, N, device=a.device, dtype=torch.float32)
    _chk(load().tfp_gemm_nn_dz(a.data_ptr(), y.data_ptr() if y is not None else None, b.data_ptr(), y_out.data_ptr() if y_out is not None else None,
                               c.data_ptr(), M, N, K, _stream(a)), "tfp_gemm_nn_dz")
    return c


_PENDING_SUMS = []        # (part, gw, gb, splits, N1, N2) of the layers whose chunk products wait for flush_partial_sums()


def discard_partial_sums():
    """drop whatever is still queued (a launch raised between `mlp_backward` and `flush_partial_sums`)"""
    global _PENDING_SUMS
    _PENDING_SUMS = []


def flush_partial_sums():
    """the chunk sums of every layer queued by `gemm_tn_bias(..., defer=True)` since the last call, in ONE launch per eight layers
    (the trainer calls it once after the backward pass: eight launches become one)"""
    global _PENDING_SUMS
    pend, _PENDING_SUMS = _PENDING_SUMS, []
    for i in range(0, len(pend), 8):
        grp = pend[i:i + 8]
        n = len(grp)
        vp = lambda k: (C.c_void_p * n)(*[g[k].data_ptr() for g in grp])     # noqa: E731
        ip = lambda k: (C.c_int32 * n)(*[g[k] for g in grp])                 # noqa: E731
        _chk(load().tfp_sum_partials_multi(vp(0), vp(1), vp(2), ip(3), ip(4), ip(5), n, _stream(grp[0][0])), "tfp_sum_partials_multi")


GATHER_MAX = 8        # arrays per tfp_gather_rows launch; the trainer's minibatch with every option on is exactly that many (ppo.PPOTrainer._mb_backward_fused)


def gather_rows(srcs, idx, outs=None, norm=None):
    """[s[idx] for s in srcs] for up to 8 row-major float32 arrays (1-D arrays count as width 1) in ONE launch.  `norm`: None, or one entry per array -
    None (copied) or (mean_f, inv_std_f, clip): that array leaves as clamp((s[idx] - mean_f) * inv_std_f, -clip, clip) (tfp_gather_rows_norm), and `idx`
    may then be None (every row in place: a plain normaliser)."""
    if norm is not None and any(e is not None for e in norm):
        return _gather_rows_norm(srcs, idx, outs, norm)
    assert 0 < len(srcs) <= GATHER_MAX and idx.dtype == torch.long and idx.is_contiguous()
    rows = idx.numel()
    widths = [int(s[0].numel()) for s in srcs]
    if outs is None:
        outs = [torch.empty((rows,) + tuple(s.shape[1:]), device=s.device, dtype=torch.float32) for s in srcs]
    n = len(srcs)
    _chk(load().tfp_gather_rows((C.c_void_p * n)(*[s.data_ptr() for s in srcs]), (C.c_void_p * n)(*[o.data_ptr() for o in outs]),
                                (C.c_int32 * n)(*widths), n, idx.data_ptr(), rows, _stream(idx)), "tfp_gather_rows")
    return outs


# ---- input normalisation (csrc/ppo_norm.hip; the holder of the records is ppo.InputNorm) -----------------------------------------------------
def _norm_ok(e, width, dev):
    mean, inv, clip = e
    return (mean.dtype == torch.float32 and inv.dtype == torch.float32 and mean.is_contiguous() and inv.is_contiguous() and mean.device == dev
            and inv.device == dev and mean.numel() == width and inv.numel() == width and float(clip) > 0.0)


def _gather_rows_norm(srcs, idx, outs, norm):
    assert 0 < len(srcs) <= GATHER_MAX and len(norm) == len(srcs) and all(s.dtype == torch.float32 and s.is_contiguous() for s in srcs)
    assert idx is None or (idx.dtype == torch.long and idx.is_contiguous())
    rows = idx.numel() if idx is not None else srcs[0].shape[0]
    assert idx is not None or all(s.shape[0] == rows for s in srcs)
    widths = [int(s[0].numel()) for s in srcs]
    assert all(e is None or _norm_ok(e, w, s.device) for e, w, s in zip(norm, widths, srcs)), "statistics of another width, type or device"
    if outs is None:
        outs = [torch.empty((rows,) + tuple(s.shape[1:]), device=s.device, dtype=torch.float32) for s in srcs]
    n = len(srcs)
    _chk(load().tfp_gather_rows_norm(_vp(srcs), _vp(outs), _ip(widths), _vp([e[0] if e is not None else None for e in norm]),
                                     _vp([e[1] if e is not None else None for e in norm]),
                                     (C.c_float * n)(*[float(e[2]) if e is not None else 0.0 for e in norm]), n,
                                     idx.data_ptr() if idx is not None else None, rows, _stream(srcs[0])), "tfp_gather_rows_norm")
    return outs


SYM_MAX_WIDTH, SYM_MAX_COLS = 128, 512        # include/trifinger_ppo_symmetry.h: columns of one array / of all arrays of one launch together


def gather_rows_sym(srcs, idx, tables, outs=None, norm=None):
    """the augmenting gather (`symmetry_augmentation`): per array [3 rows, ...] - rows [k rows, (k + 1) rows) hold the k-th image of s[idx], k = 0 the plain
    gather - for up to 8 row-major float32 arrays in ONE launch (tfp_gather_rows_sym).  `tables`: one entry per array - None (copied for every k) or the
    packed tables of that array (symmetry.pack: int32 [2, width, 4] on the device); `norm` as in gather_rows, applied after the transform: the bits of
    gather_rows(norm=...) on symmetry.apply of the gathered rows.  `idx` may be None (every row in place)."""
    n = len(srcs)
    assert 0 < n <= GATHER_MAX and len(tables) == n and all(s.dtype == torch.float32 and s.is_contiguous() and s.is_cuda for s in srcs)
    assert idx is None or (idx.dtype == torch.long and idx.is_contiguous() and idx.device == srcs[0].device)
    rows = idx.numel() if idx is not None else srcs[0].shape[0]
    assert idx is not None or all(s.shape[0] == rows for s in srcs)
    widths = [int(s[0].numel()) for s in srcs]
    norm = norm if norm is not None else [None] * n
    assert len(norm) == n and all(e is None or _norm_ok(e, w, s.device) for e, w, s in zip(norm, widths, srcs)), "statistics of another width, type or device"
    for t, w, s in zip(tables, widths, srcs):
        if t is not None and not (t.dtype == torch.int32 and t.is_contiguous() and tuple(t.shape) == (2, w, 4) and t.device == s.device):
            raise ValueError(f"a symmetry table of another shape, type or device than its array (width {w})")
    if any(w > SYM_MAX_WIDTH for w in widths) or sum(widths) > SYM_MAX_COLS:
        raise ValueError(f"the augmenting gather takes rows of at most {SYM_MAX_WIDTH} columns, and {SYM_MAX_COLS} columns over the arrays of one launch")
    if outs is None:
        outs = [torch.empty((3 * rows,) + tuple(s.shape[1:]), device=s.device, dtype=torch.float32) for s in srcs]
    assert all(o.dtype == torch.float32 and o.is_contiguous() and o.numel() == 3 * rows * w and o.device == s.device for o, w, s in zip(outs, widths, srcs))
    _chk(load().tfp_gather_rows_sym(_vp(srcs), _vp(outs), _ip(widths), _vp([e[0] if e is not None else None for e in norm]),
                                    _vp([e[1] if e is not None else None for e in norm]),
                                    (C.c_float * n)(*[float(e[2]) if e is not None else 0.0 for e in norm]), _vp(tables), n,
                                    idx.data_ptr() if idx is not None else None, rows, _stream(srcs[0])), "tfp_gather_rows_sym")
    return outs


def normalize_rows(x, mean_f, inv_std_f, clip):
    """clamp((x - mean_f) * inv_std_f, -clip, clip) of a contiguous float32 [rows, D] in one launch (the gather with the identity index)"""
    return _gather_rows_norm([x], None, None, [(mean_f, inv_std_f, clip)])[0]


def moments(xs):
    """the batch records {count, mean[D], M2[D]} (float64) of one or two contiguous float32 arrays [rows, D] over the same rows, concatenated into one vector
    [1 + 2 D0 (+ 1 + 2 D1)], in two launches (tfp_moments: fp64, deterministic); None when the kernel declines the shapes (a row wider than 256)"""
    assert 0 < len(xs) <= 2 and all(x.dim() == 2 and x.dtype == torch.float32 and x.is_contiguous() and x.shape[0] == xs[0].shape[0] for x in xs)
    rows, D = xs[0].shape[0], [x.shape[1] for x in xs]
    if rows <= 0 or rows >= 2 ** 31:
        return None
    lib = load()
    need = int(lib.tfp_moments_part_doubles(_ip(D), len(xs), rows))
    part = torch.empty(max(need, 1), device=xs[0].device, dtype=torch.float64)
    out = torch.empty(sum(1 + 2 * d for d in D), device=xs[0].device, dtype=torch.float64)
    rc = lib.tfp_moments(_vp(xs), _ip(D), len(xs), rows, part.data_ptr(), need, out.data_ptr(), _stream(xs[0]))
    if rc == -4:
        return None
    _chk(rc, "tfp_moments")
    return out


def norm_merge(runs, batches, k, stride, mean_fs, inv_std_fs):
    """merge, per record q (one or two), the k batch records batches[q][j * stride : ...], j = 0 .. k - 1 in this order, into the running record runs[q]
    (float64 [1 + 2 D], in place) and publish mean_fs[q] / inv_std_fs[q] (float32 [D], in place); ONE launch.  `batches[q]` is a float64 view whose
    first element is record 0 of input q - e.g. a slice of the gathered vectors of all ranks."""
    n = len(runs)
    assert 0 < n <= 2 and all(r.dtype == torch.float64 and r.is_contiguous() for r in runs)
    D = [(r.numel() - 1) // 2 for r in runs]
    assert all(b.dtype == torch.float64 and b.is_contiguous() and b.numel() >= (k - 1) * stride + 1 + 2 * d for b, d in zip(batches, D))
    assert all(m.dtype == torch.float32 and m.numel() == d and i.dtype == torch.float32 and i.numel() == d for m, i, d in zip(mean_fs, inv_std_fs, D))
    _chk(load().tfp_norm_merge(_vp(runs), _vp(batches), _ip(D), n, int(k), int(stride), _vp(mean_fs), _vp(inv_std_fs), _stream(runs[0])), "tfp_norm_merge")


# ---- the rollout's bookkeeping (ppo.PPOTrainer.rollout) -----------------------------------------------------------------------------------
def rollout_record(obs, states, mu, log_std, sigma, eps, val, buf, t):
    """a = mu + sigma * eps (sigma = log_std.exp(), formed once per rollout), its negative log-likelihood, and the step filed into slot t of the rollout buffers (obs, states, act, mu, nlp, val) in
    ONE launch; returns the action (a view of buf["act"][t])"""
    n, A = mu.shape
    f = lambda x: x if x.is_contiguous() else x.contiguous()          # noqa: E731
    obs, mu, eps, val = f(obs), f(mu), f(eps), f(val)
    states = f(states) if states is not None else None
    _chk(load().tfp_rollout_record(obs.data_ptr(), obs.shape[1], states.data_ptr() if states is not None else None, states.shape[1] if states is not None else 0,
                                   mu.data_ptr(), log_std.data_ptr(), sigma.data_ptr(), eps.data_ptr(), val.data_ptr(), n, A, buf["obs"][t].data_ptr(),
                                   buf["states"][t].data_ptr() if states is not None else None, buf["act"][t].data_ptr(), buf["mu"][t].data_ptr(),
                                   buf["nlp"][t].data_ptr(), buf["val"][t].data_ptr(), _stream(mu)), "tfp_rollout_record")
    return buf["act"][t]


def eval_step(state, reward, reset_buf, goal_reset_buf, steps, env_acc, acc, pos_tol, ori_tol, rule, max_episodes_per_env):
    """one launch of the episode statistics behind an env step (include/trifinger_ppo_eval.h: tfp_eval_step) on torch's current stream: reads the env's
    buffers, updates `env_acc` (int32 [4, N]) and `acc` (int64 [TFP_EVAL_ACC]) in place; no allocation, no synchronisation"""
    _chk(load().tfp_eval_step(state.data_ptr(), reward.data_ptr(), reset_buf.data_ptr(), goal_reset_buf.data_ptr(), steps.data_ptr(), env_acc.data_ptr(),
                              acc.data_ptr(), reward.shape[0], float(pos_tol), float(ori_tol), int(rule), int(max_episodes_per_env), _stream(state)),
         "tfp_eval_step")


def eval_test_predicates(state, pos_tol, ori_tol):
    """int64 [2]: the number of envs with pos_ok / ori_ok from the evaluator's device code (tfp_eval_test_predicates: the tests' window into the predicates)"""
    out = torch.zeros(2, dtype=torch.int64, device=state.device)
    _chk(load().tfp_eval_test_predicates(state.data_ptr(), state.shape[1], float(pos_tol), float(ori_tol), out.data_ptr(), _stream(state)),
         "tfp_eval_test_predicates")
    return out


def readable(t, like, *dtypes):
    """the kernels can read `t` in place: a contiguous GPU tensor of one of `dtypes` on the device of `like`"""
    return t.is_cuda and t.device == like.device and t.dtype in dtypes and t.is_contiguous()


def rollout_reward(r, d, scale, rew_t, done_t):
    """rew_t = r * scale, done_t = float(d) in one launch; d: torch.bool / uint8"""
    assert d.dtype in (torch.bool, torch.uint8) and d.is_contiguous() and r.is_contiguous() and r.dtype == torch.float32
    _chk(load().tfp_rollout_reward(r.data_ptr(), d.data_ptr(), float(scale), r.numel(), rew_t.data_ptr(), done_t.data_ptr(), _stream(r)), "tfp_rollout_reward")


def _gae_launch(rew, end, val, gamma, tau, tout=None, last_end=None, boot=None, mean_f=None, inv_std_f=None, clip=0.0):
    """the checks, the allocation and the launch behind `gae`, `gae_vnorm` and `gae_ends` (`boot` None: the `done` instantiations, `end` holds the done
    rows; mean_f None: plain values); the outputs in the order adv, ret, [w], [ret_n, v_old_n]"""
    T, n = rew.shape
    ends, vnorm = boot is not None, mean_f is not None
    ins = (rew, val, end) + ((tout, last_end) if ends else ()) + ((mean_f, inv_std_f) if vnorm else ())
    assert all(t.dtype == torch.float32 and t.is_contiguous() and t.device == rew.device for t in ins)
    assert val.shape == (T + 1, n) and end.shape == (T, n) and (not ends or (tout.shape == (T, n) and last_end.shape == (n,)))
    assert not vnorm or (mean_f.numel() == 1 and inv_std_f.numel() == 1 and float(clip) > 0.0)
    out = {k: torch.empty_like(rew) for k in ("adv", "ret") + (("w",) if ends else ()) + (("ret_n", "v_old_n") if vnorm else ())}
    p = {k: t.data_ptr() for k, t in out.items()}
    g, gt, st = float(gamma), float(gamma * tau), _stream(rew)
    norm = (mean_f.data_ptr(), inv_std_f.data_ptr(), float(clip)) if vnorm else (None, None, float(clip))
    if ends:
        _chk(load().tfp_gae_ends(rew.data_ptr(), end.data_ptr(), tout.data_ptr(), val.data_ptr(), last_end.data_ptr(), 1 if boot else 0, *norm, g, gt, T, n,
                                 p["adv"], p["ret"], p["w"], p.get("ret_n"), p.get("v_old_n"), st), "tfp_gae_ends")
    elif vnorm:
        _chk(load().tfp_gae_vnorm(rew.data_ptr(), end.data_ptr(), val.data_ptr(), *norm, g, gt, T, n, p["adv"], p["ret"], p["ret_n"], p["v_old_n"], st), "tfp_gae_vnorm")
    else:
        _chk(load().tfp_gae(rew.data_ptr(), end.data_ptr(), val.data_ptr(), g, gt, T, n, p["adv"], p["ret"], st), "tfp_gae")
    return tuple(out.values())


# the three entry points of k_gae, one binding each (the tests and the cost tools call and count them by name); `gae_buffers` is what the trainer calls
def gae(rew, done, val, gamma, tau):
    """tfp_gae: (adv, ret), each [T, n], from rew, done [T, n] and val [T + 1, n]"""
    return _gae_launch(rew, done, val, gamma, tau)


def gae_vnorm(rew, done, y, mean_f, inv_std_f, clip, gamma, tau):
    """tfp_gae_vnorm: (adv, ret, ret_n, v_old_n) for a value network whose raw output y [T + 1, n] is in normalised units (`normalize_value`);
    mean_f / inv_std_f: the float32 [1] device tensors a ppo.InputNorm(1) publishes"""
    return _gae_launch(rew, done, y, gamma, tau, mean_f=mean_f, inv_std_f=inv_std_f, clip=clip)


def gae_ends(rew, end, tout, val, last_end, gamma, tau, value_bootstrap, mean_f=None, inv_std_f=None, clip=0.0):
    """tfp_gae_ends (`episode_ends`): (adv, ret, w), and with mean_f / inv_std_f / clip (adv, ret, w, ret_n, v_old_n); last_end [n]"""
    return _gae_launch(rew, end, val, gamma, tau, tout, last_end, bool(value_bootstrap), mean_f, inv_std_f, clip)


def gae_buffers(rew, val, gamma, tau, done=None, ends=None, vnorm=None):
    """Generalised advantage estimation over the horizon in ONE launch (ppo.gae_spec is the specification, bit for bit) - the ONE wrapper of the trainer:
    rew [T, n], val [T + 1, n], and either `done` [T, n] or `ends` = (end [T, n], tout [T, n], last_end [n], value_bootstrap) (`episode_ends`).  `vnorm`:
    the returns' record (ppo.InputNorm(1): mean_f, inv_std_f, clip) - val is then the value network's raw normalised output.  Returns the named buffers
    of the rollout, each [T, n], so that the caller can `buf.update()` them: adv and ret, w with `ends`, ret_n and v_old_n with `vnorm`."""
    assert (done is None) != (ends is None)
    norm = (vnorm.mean_f, vnorm.inv_std_f, vnorm.clip) if vnorm is not None else ()
    if ends is not None:
        end, tout, last_end, boot = ends
        return dict(zip(("adv", "ret", "w", "ret_n", "v_old_n"), gae_ends(rew, end, tout, val, last_end, gamma, tau, boot, *norm)))
    if vnorm is not None:
        return dict(zip(("adv", "ret", "ret_n", "v_old_n"), gae_vnorm(rew, done, val, *norm, gamma, tau)))
    return dict(zip(("adv", "ret"), gae(rew, done, val, gamma, tau)))


# ---- episode ends (include/trifinger_ppo_episode.h; ppo.PPOTrainer with `episode_ends`) --------------------------------------------------------
def rollout_flags(r, reset_buf, steps, scale, episode_length, rew_t, end_t, tout_t):
    """rew_t = r * scale, end_t = float(reset_buf != 0), tout_t = float(episode_length > 0 and steps >= episode_length) in ONE launch (it stands where
    `rollout_reward` does); reset_buf: torch.bool / uint8 [n], steps: int64 [n] - the engine's own buffers, only read"""
    n = r.numel()
    assert r.dtype == torch.float32 and r.is_contiguous() and reset_buf.dtype in (torch.bool, torch.uint8) and reset_buf.is_contiguous() and reset_buf.numel() == n
    assert steps.dtype == torch.int64 and steps.is_contiguous() and steps.numel() == n and reset_buf.device == r.device and steps.device == r.device
    for t in (rew_t, end_t, tout_t):
        assert t.dtype == torch.float32 and t.is_contiguous() and t.numel() == n and t.device == r.device
    _chk(load().tfp_rollout_flags(r.data_ptr(), reset_buf.data_ptr(), steps.data_ptr(), float(scale), int(episode_length), n, rew_t.data_ptr(), end_t.data_ptr(),
                                  tout_t.data_ptr(), _stream(r)), "tfp_rollout_flags")


# ---- the training-time episode tracker (include/trifinger_ppo_track.h; evaluate.EpisodeTracker, ppo.PPOTrainer with `track_episodes`) ---------------------
TRACK_ENV_ROWS, TRACK_ACC = 2, 11


class TfpTrackArgs(C.Structure):
    """include/trifinger_ppo_track.h: TfpTrackArgs"""
    _fields_ = [("state", C.c_void_p), ("reward", C.c_void_p), ("reset_buf", C.c_void_p), ("steps", C.c_void_p), ("done_bytes", C.c_void_p),
                ("b_rew", C.c_void_p), ("b_done", C.c_void_p), ("b_end", C.c_void_p), ("b_tout", C.c_void_p), ("env_trk", C.c_void_p), ("acc", C.c_void_p),
                ("episode_length", C.c_int64), ("scale", C.c_float), ("pos_tol", C.c_float), ("ori_tol", C.c_float), ("rule", C.c_int32), ("N", C.c_int32)]


def rollout_track(state, reward, reset_buf, steps, env_trk, acc, scale, episode_length, pos_tol, ori_tol, rule, rew_t, done=None, done_t=None, end_t=None,
                  tout_t=None):
    """ONE launch behind an env step of a rollout, on torch's current stream (tfp_rollout_track): with `done` / `done_t` it stands where `rollout_reward`
    does (rew_t = reward * scale, done_t = float(done)), with `end_t` / `tout_t` where `rollout_flags` does - the same bits -, and either way it updates the
    tracker's per-env state `env_trk` (int32 [2, N]) and its accumulator `acc` (int64 [TRACK_ACC]) from the engine's buffers, which are only read.
    No allocation, no synchronisation."""
    n = reward.numel()
    dev = reward.device
    mode_a = done is not None
    outs = (rew_t, done_t) if mode_a else (rew_t, end_t, tout_t)
    assert reward.dtype == torch.float32 and reward.is_contiguous() and state.dtype == torch.float32 and state.is_contiguous() and state.shape[1] == n
    assert reset_buf.dtype in (torch.bool, torch.uint8) and reset_buf.is_contiguous() and reset_buf.numel() == n
    assert steps.dtype == torch.int64 and steps.is_contiguous() and steps.numel() == n
    assert not mode_a or (done.dtype in (torch.bool, torch.uint8) and done.is_contiguous() and done.numel() == n and done.device == dev)
    assert all(t is not None and t.dtype == torch.float32 and t.is_contiguous() and t.numel() == n and t.device == dev for t in outs)
    assert env_trk.dtype == torch.int32 and env_trk.is_contiguous() and tuple(env_trk.shape) == (TRACK_ENV_ROWS, n)
    assert acc.dtype == torch.int64 and acc.is_contiguous() and acc.numel() == TRACK_ACC
    assert all(t.device == dev for t in (state, reset_buf, steps, env_trk, acc))
    a = TfpTrackArgs()
    a.state, a.reward, a.reset_buf, a.steps = state.data_ptr(), reward.data_ptr(), reset_buf.data_ptr(), steps.data_ptr()
    a.done_bytes = done.data_ptr() if mode_a else None
    a.b_rew = rew_t.data_ptr()
    a.b_done = done_t.data_ptr() if mode_a else None
    a.b_end, a.b_tout = (None, None) if mode_a else (end_t.data_ptr(), tout_t.data_ptr())
    a.env_trk, a.acc = env_trk.data_ptr(), acc.data_ptr()
    a.episode_length, a.scale, a.pos_tol, a.ori_tol, a.rule, a.N = int(episode_length), float(scale), float(pos_tol), float(ori_tol), int(rule), n
    _chk(load().tfp_rollout_track(C.byref(a), _stream(reward)), "tfp_rollout_track")


# ---- the episode flight recorder (include/trifinger_ppo_record.h; record.EpisodeRecorder) -------------------------------------------------------------
REC_STATE_ROWS, REC_ROWS, REC_ENV_ROWS, REC_ACC = 59, 61, 8, 4


class TfpRecordArgs(C.Structure):
    """include/trifinger_ppo_record.h: TfpRecordArgs"""
    _fields_ = [("state", C.c_void_p), ("reward", C.c_void_p), ("reset_buf", C.c_void_p), ("steps", C.c_void_p), ("ring", C.c_void_p), ("hdr", C.c_void_p),
                ("env_rec", C.c_void_p), ("acc", C.c_void_p), ("episode_length", C.c_int64), ("pos_tol", C.c_float), ("ori_tol", C.c_float),
                ("N", C.c_int32), ("W", C.c_int32), ("L", C.c_int32), ("every", C.c_int32), ("select", C.c_int32), ("rule", C.c_int32)]


def record_step(state, reward, reset_buf, steps, ring, hdr, env_rec, acc, every, select, episode_length, pos_tol, ori_tol, rule):
    """ONE launch of the episode flight recorder behind an env step, on torch's current stream (tfp_record_step): reads the engine's buffers, writes the
    caller's `ring` (float32 [L, REC_ROWS, W]), `hdr` (float32 [TF_NUM_DR, W]), `env_rec` (int32 [REC_ENV_ROWS, W]) and `acc` (int64 [REC_ACC]); the
    ring's shape gives L and W.  No allocation, no synchronisation."""
    n = reward.numel()
    dev = reward.device
    assert ring.dim() == 3 and ring.shape[1] == REC_ROWS
    L, w = int(ring.shape[0]), int(ring.shape[2])
    assert 1 <= w <= n and L >= 1
    assert reward.dtype == torch.float32 and reward.is_contiguous() and state.dtype == torch.float32 and state.is_contiguous() and state.dim() == 2
    assert state.shape[1] == n and state.shape[0] >= 98                                  # rows up to TF_S_DR + TF_NUM_DR are read
    assert reset_buf.dtype in (torch.bool, torch.uint8) and reset_buf.is_contiguous() and reset_buf.numel() == n
    assert steps.dtype == torch.int64 and steps.is_contiguous() and steps.numel() == n
    assert ring.dtype == torch.float32 and ring.is_contiguous() and hdr.dtype == torch.float32 and hdr.is_contiguous() and tuple(hdr.shape) == (14, w)
    assert env_rec.dtype == torch.int32 and env_rec.is_contiguous() and tuple(env_rec.shape) == (REC_ENV_ROWS, w)
    assert acc.dtype == torch.int64 and acc.is_contiguous() and acc.numel() == REC_ACC
    assert all(t.device == dev for t in (state, reset_buf, steps, ring, hdr, env_rec, acc))
    a = TfpRecordArgs()
    a.state, a.reward, a.reset_buf, a.steps = state.data_ptr(), reward.data_ptr(), reset_buf.data_ptr(), steps.data_ptr()
    a.ring, a.hdr, a.env_rec, a.acc = ring.data_ptr(), hdr.data_ptr(), env_rec.data_ptr(), acc.data_ptr()
    a.episode_length, a.pos_tol, a.ori_tol = int(episode_length), float(pos_tol), float(ori_tol)
    a.N, a.W, a.L, a.every, a.select, a.rule = n, w, L, int(every), int(select), int(rule)
    _chk(load().tfp_record_step(C.byref(a), _stream(reward)), "tfp_record_step")


def gemm_tn_bias(a, b, y=None, chunk=256, out=None, defer=False):
    """dz = a * elu'(y) (or a); returns (dz.T @ b, dz.sum(0)): products of [b | 1] over row chunks (one workgroup set per chunk),
    then their sum in a fixed order - the bias gradient is the extra column"""
    rows, N1 = a.shape
    N2 = b.shape[1]
    splits = (rows + chunk - 1) // chunk
    part = torch.empty(splits * N1 * (N2 + 1), device=a.device, dtype=torch.float32)
    if out is not None:
        gw, gb = out
    else:
        gw = torch.empty(N1, N2, device=a.device, dtype=torch.float32)
        gb = torch.empty(N1, device=a.device, dtype=torch.float32)
    if defer:                                             # products now, the chunk sums with the other layers' in flush_partial_sums()
        _chk(load().tfp_gemm_tn_partials(a.data_ptr(), y.data_ptr() if y is not None else None, b.data_ptr(), part.data_ptr(), rows, N1, N2, chunk,
                                         _stream(a)), "tfp_gemm_tn_partials")
        _PENDING_SUMS.append((part, gw, gb, splits, N1, N2))
        return gw, gb
    _chk(load().tfp_gemm_tn_bias(a.data_ptr(), y.data_ptr() if y is not None else None, b.data_ptr(), part.data_ptr(), gw.data_ptr(), gb.data_ptr(),
                                 rows, N1, N2, chunk, _stream(a)), "tfp_gemm_tn_bias")
    return gw, gb


# ---- the same products for several independent problems in one launch (tfp_*_group) -------------------------------------------------
def _vp(ts):
    return (C.c_void_p * len(ts))(*[(t.data_ptr() if t is not None else None) for t in ts])


def _ip(vals):
    return (C.c_int32 * len(vals))(*[int(v) for v in vals])


def linear_fwd_group(xs, ws, bs, act):
    """[act(x @ w.T + b)] for up to 8 independent (x, w, b) in ONE launch; None when the problems are not of one kind (the caller falls back)"""
    n = len(xs)
    ys = [torch.empty(x.shape[0], w.shape[0], device=x.device, dtype=torch.float32) for x, w in zip(xs, ws)]
    rc = load().tfp_linear_fwd_group(_vp(xs), _vp(ws), _vp(bs), _vp(ys), _ip([x.shape[0] for x in xs]), _ip([w.shape[0] for w in ws]),
                                     _ip([x.shape[1] for x in xs]), int(act), n, _stream(xs[0]))
    if rc == -4:
        return None
    _chk(rc, "tfp_linear_fwd_group")
    return ys


def gemm_nn_group(as_, bs, ys=None, y_outs=None):
    """[((a * elu'(y)) @ b) * elu'(y_out)] for up to 8 independent problems in ONE launch (ys: all given or None; y_outs: a list with None entries
    allowed, or None); None when they are not of one kind"""
    n = len(as_)
    cs = [torch.empty(a.shape[0], b.shape[1], device=a.device, dtype=torch.float32) for a, b in zip(as_, bs)]
    eo = None
    if y_outs is not None and any(e is not None for e in y_outs):
        eo = (C.c_void_p * n)(*[e.data_ptr() if e is not None else None for e in y_outs])
    rc = load().tfp_gemm_nn_dz_group(_vp(as_), _vp(ys) if ys is not None else None, _vp(bs), eo, _vp(cs), _ip([a.shape[0] for a in as_]),
                                     _ip([b.shape[1] for b in bs]), _ip([a.shape[1] for a in as_]), n, _stream(as_[0]))
    if rc == -4:
        return None
    _chk(rc, "tfp_gemm_nn_dz_group")
    return cs


def gemm_tn_bias_group(as_, bs, ys, outs, chunk=256):
    """the chunk products of up to 8 weight / bias gradients in ONE launch, their sums deferred to flush_partial_sums() (as gemm_tn_bias(defer=True));
    ys: all given or None.  Returns False when the problems are not of one kind (nothing is queued then)"""
    n = len(as_)
    rows = [a.shape[0] for a in as_]
    n1 = [a.shape[1] for a in as_]
    n2 = [b.shape[1] for b in bs]
    parts = [torch.empty(((r + chunk - 1) // chunk) * a1 * (b2 + 1), device=as_[0].device, dtype=torch.float32) for r, a1, b2 in zip(rows, n1, n2)]
    rc = load().tfp_gemm_tn_partials_group(_vp(as_), _vp(ys) if ys is not None else None, _vp(bs), _vp(parts), _ip(rows), _ip(n1), _ip(n2), int(chunk), n,
                                           _stream(as_[0]))
    if rc == -4:
        return False
    _chk(rc, "tfp_gemm_tn_partials_group")
    for k in range(n):
        _PENDING_SUMS.append((parts[k], outs[k][0], outs[k][1], (rows[k] + chunk - 1) // chunk, n1[k], n2[k]))
    return True


def gemm_tn_bias_direct(as_, bs, outs, mixed=False):
    """the chunk slabs of up to 8 weight / bias gradients [a.T @ b | a.sum(0)] in ONE launch of the direct kernel (csrc/ppo_dw_direct.hip: 64 x 64 blocks,
    operands straight from memory), their sums deferred to flush_partial_sums().  a: dZ [rows, N1] (plain: no activation factor), b: [rows, N2].
    Returns False when the call does not fit (nothing is queued then).  `mixed`: tfp_gemm_tn_partials_direct_bf16 - [bf16r(a).T @ bf16r(b) | a.sum(0)]."""
    n = len(as_)
    name = "tfp_gemm_tn_partials_direct_bf16" if mixed else "tfp_gemm_tn_partials_direct"
    as_ = [a if a.is_contiguous() else a.contiguous() for a in as_]
    bs = [b if b.is_contiguous() else b.contiguous() for b in bs]
    rows = [a.shape[0] for a in as_]
    n1 = [a.shape[1] for a in as_]
    n2 = [b.shape[1] for b in bs]
    chunk = load().tfp_gemm_tn_partials_direct_chunk()          # rows per slab of the build
    splits = [(r + chunk - 1) // chunk for r in rows]
    parts = [torch.empty(sp * a1 * (b2 + 1), device=as_[0].device, dtype=torch.float32) for sp, a1, b2 in zip(splits, n1, n2)]
    rc = getattr(load(), name)(_vp(as_), _vp(bs), _vp(parts), _ip(rows), _ip(n1), _ip(n2), n, _stream(as_[0]))
    if rc == -4:
        return False
    _chk(rc, name)
    _count(name)
    for k in range(n):
        _PENDING_SUMS.append((parts[k], outs[k][0], outs[k][1], splits[k], n1[k], n2[k]))
    return True


USE_DIRECT_DW = True


class _MfmaLinear(torch.autograd.Function):
    """act(x W^T + b) with every matrix product on the hand-written fp32 MFMA kernels: forward with bias and ELU fused into the
    store; backward with the ELU derivative formed in the operand loads and the bias gradient as an extra column of the weight
    gradient product - three launches (+ one reduction of the batch chunks) where the eager form takes nine.  With `grad_out` =
    (dW buffer, db buffer) the parameter gradients are WRITTEN there (not accumulated, not returned to autograd) - complete only
    after `flush_partial_sums()`, which sums the row chunks of every such layer of the backward pass in one launch: the trainer
    passes the parameters' slots of its flat gradient buffer and flushes once per minibatch step."""

    @staticmethod
    def forward(ctx, x, w, b, act, grad_out):
        x = x.contiguous()
        y = linear_fwd(x, w, b, act)
        ctx.act, ctx.grad_out = act, grad_out
        ctx.save_for_backward(x, w, y)
        return y

    @staticmethod
    def backward(ctx, gy):
        x, w, y = ctx.saved_tensors
        gy = gy.contiguous()
        yy = y if ctx.act else None
        gx = gemm_nn(gy, w, yy) if ctx.needs_input_grad[0] else None
        if ctx.grad_out is not None:                      # the trainer's path: sums deferred to one launch after the backward pass
            gemm_tn_bias(gy, x, yy, out=ctx.grad_out, defer=True)
            return gx, None, None, None, None
        gw, gb = gemm_tn_bias(gy, x, yy)
        return gx, gw, gb, None, None


def mfma_linear(x, w, b, act, grad_out=None):
    return _MfmaLinear.apply(x, w, b, int(act), grad_out)


# ---- the two MLPs without autograd: forward keeps the layer outputs, backward walks them in reverse --------------------------------
def mlp_forward(x, layers):
    """`layers`: [(weight, bias, act, grad_out)] in order.  Returns the list of layer outputs (the last one is the network output);
    the inputs of the layers are `x` and the outputs before them.  The per-layer tier itself: one launch per layer, ELU / none only."""
    ys = []
    for w, b, act, _ in layers:
        x = linear_fwd(x, w, b, act)
        ys.append(x)
    return ys


# ---- the network walk (csrc/ppo_mlp_walk.hip): all layers of up to two networks in ONE launch per direction ------------------------------------
WALK_MAXL = 4


class TfpMlp(C.Structure):
    """include/trifinger_ppo.h: TfpMlp"""
    _fields_ = [("x", C.c_void_p), ("W", C.c_void_p * WALK_MAXL), ("b", C.c_void_p * WALK_MAXL), ("yin", C.c_void_p * WALK_MAXL),
                ("y", C.c_void_p * WALK_MAXL), ("dim", C.c_int32 * (WALK_MAXL + 1)), ("act", C.c_int32 * WALK_MAXL), ("n_layers", C.c_int32)]


class TfpNet(C.Structure):
    """include/trifinger_ppo_net.h: TfpNet"""
    _fields_ = [("mlp", TfpMlp), ("d2rl", C.c_int32), ("clip", C.c_float), ("mean", C.c_void_p), ("inv_std", C.c_void_p)]


class TfpNorm(C.Structure):
    """include/trifinger_ppo_norm.h: TfpNorm"""
    _fields_ = [("mean", C.c_void_p), ("inv_std", C.c_void_p), ("clip", C.c_float)]


# activation codes of include/trifinger_ppo_net.h (0 and 1 are the ones every kernel knows); swish and gelu have none (ACT_NO_KERNEL)
ACT_CODES = {"none": 0, "elu": 1, "relu": 2, "tanh": 3, "sigmoid": 4, "selu": 5, "softplus": 6}
ACT_NO_KERNEL = -1


class LayerList(list):
    """[(weight, bias, act, grad_out)] of a network's Linear layers, act an activation code.  `d2rl`: the input x is concatenated behind every hidden
    output but the last - weight l is [out, in + D0] for 1 <= l <= len - 2 - and the walk keeps / expects the hidden outputs of those layers as the wide
    rows [h | x] (include/trifinger_ppo_net.h).  `ext`: what needs_net_walk() answers, when the builder of the list already knows it (None: computed per call;
    the trainer's lists carry it so that a minibatch step does not walk the layers again).  `mixed`: `mixed_precision` - every product of the network takes
    bf16 operands (include/trifinger_ppo_mixed.h); forward_nets / backward_nets read the mode from here"""
    d2rl = False
    ext = None
    mixed = False


def _d2rl(layers):
    return bool(getattr(layers, "d2rl", False)) and len(layers) >= 3      # with one hidden layer there is no wide layer: the plain network


def needs_net_walk(layers):
    """True for a network only the extended walk (tfp_net_*) runs: an activation other than ELU / none, or d2rl"""
    known = getattr(layers, "ext", None)
    if known is not None:
        return known
    return _d2rl(layers) or any(int(l[2]) not in (0, 1) for l in layers)


def _out_width(layers, l):
    """columns of what the walk stores for layer l: [h | x] where the next layer of a d2rl network reads it"""
    return layers[l][0].shape[0] + (layers[0][0].shape[1] if (_d2rl(layers) and l <= len(layers) - 3) else 0)


def _walk_blocks(nets, ext, norms=None, check=False):
    """the walk's argument blocks, the ONE place that fills them: nets = [(x or gy or None, layers, y, yin)] with y / yin the per-layer tensors (or None)
    behind TfpMlp.y / .yin.  An array of TfpMlp, each wrapped in a TfpNet (d2rl, the statistics `norms[i]`) when the extended entry point is taken.
    `check`: the weights' widths against the network description (a ValueError)"""
    arr = ((TfpNet if ext else TfpMlp) * len(nets))()
    for i, (x, layers, y, yin) in enumerate(nets):
        net = arr[i]
        m = net.mlp if ext else net
        m.x = x.data_ptr() if x is not None else None
        m.n_layers = len(layers)
        m.dim[0] = layers[0][0].shape[1]
        for l, (w, b, act, _) in enumerate(layers):
            m.W[l], m.b[l] = w.data_ptr(), (b.data_ptr() if b is not None else None)
            m.dim[l + 1], m.act[l] = w.shape[0], int(act)
            if y is not None and l < len(y) and y[l] is not None:
                m.y[l] = y[l].data_ptr()
            if yin is not None and l < len(yin):
                m.yin[l] = yin[l].data_ptr()
            if check and w.shape[1] != (_out_width(layers, l - 1) if l > 0 else m.dim[0]):
                raise ValueError(f"weight of layer {l} has {w.shape[1]} columns, the network description gives {_out_width(layers, l - 1) if l > 0 else m.dim[0]}")
        if ext:
            net.d2rl = 1 if _d2rl(layers) else 0
            if norms is not None and norms[i] is not None:
                net.mean, net.inv_std, net.clip = norms[i][0].data_ptr(), norms[i][1].data_ptr(), float(norms[i][2])
    return arr


# the walk's entry point by (direction, extended, statistics given).  The plain kernels keep their own argument block and entry points on purpose: their
# timing is what DESIGN.md section 9 item 1 rests on
_WALK_ENTRY_MIXED = {"forward": "tfp_net_forward_bf16", "backward": "tfp_net_backward_bf16"}      # `mixed_precision`: the extended block, whatever the network
_WALK_ENTRY = {("forward", False, False): "tfp_mlp_forward", ("forward", False, True): "tfp_mlp_forward_norm", ("forward", True, False): "tfp_net_forward",
               ("forward", True, True): "tfp_net_forward", ("backward", False, False): "tfp_mlp_backward", ("backward", True, False): "tfp_net_backward"}


def _walk_launch(direction, nets, ext, norms, M, stream, mixed=False):
    """ONE launch of the walk over `nets` (as _walk_blocks takes them); False when the kernel declines the shapes.  `mixed`: the bf16 entry point (ext is True)"""
    name = _WALK_ENTRY_MIXED[direction] if mixed else _WALK_ENTRY[direction, bool(ext), norms is not None]
    args = [C.cast(_walk_blocks(nets, ext, norms, check=ext and direction == "forward"), C.c_void_p)]
    if norms is not None and not ext:                               # the plain walk takes the statistics as a block of their own
        nm = (TfpNorm * len(nets))()
        for i, e in enumerate(norms):
            if e is not None:
                nm[i].mean, nm[i].inv_std, nm[i].clip = e[0].data_ptr(), e[1].data_ptr(), float(e[2])
        args.append(C.cast(nm, C.c_void_p))
    rc = getattr(load(), name)(*args, len(nets), M, stream)
    if rc == -4:
        return False
    _chk(rc, name)
    _count(name)
    return True


def net_fits(layer_lists, backward=False, mixed=False):
    """whether the SHAPES of one or two networks (LayerLists; activation codes 0 .. 6) fit the network walk in the given direction: tfp_net_fits
    (`mixed`: tfp_net_fits_bf16), no launch"""
    if not (0 < len(layer_lists) <= 2) or any(not (0 < len(l) <= WALK_MAXL) or any(not (0 <= int(e[2]) <= 6) for e in l) for l in layer_lists):
        return False
    arr = _walk_blocks([(None, layers, None, None) for layers in layer_lists], True, check=True)
    name = "tfp_net_fits_bf16" if mixed else "tfp_net_fits"
    rc = getattr(load(), name)(C.cast(arr, C.c_void_p), len(layer_lists), 1 if backward else 0)
    if rc == -4:
        return False
    _chk(rc, name)
    return True


def _walkable(nets):
    return (0 < len(nets) <= 2 and all(0 < len(layers) <= WALK_MAXL for _, layers in nets)
            and all(x.dim() == 2 and x.is_contiguous() and x.shape[0] == nets[0][0].shape[0] for x, _ in nets))


def mlp_walk_forward(nets, store_hidden=True, norms=None, ext=None, mixed=False, outs=None):
    """nets: [(x, layers)] for one or two Linear / ELU stacks over the same rows (`layers` as in mlp_forward).  ONE launch; returns the list of layer
    outputs per network (hidden outputs None with store_hidden = False: the rollout needs the network outputs only), or None when the shapes do not
    fit the walk (the caller then runs the layers one by one).  `norms`: None, or per network None / (mean_f, inv_std_f, clip): that network reads
    clamp((x - mean_f) * inv_std_f, -clip, clip), formed while the rows are staged (tfp_mlp_forward_norm) - the bits of the plain walk on normalize_rows(x).
    A network with another activation than ELU / none or with d2rl (`layers` a LayerList) takes the call to tfp_net_forward (`ext` = True forces that entry
    point, which for plain networks returns the same bits); of a d2rl network the outputs of the layers 0 .. len - 3 come back as the wide rows [h | x].
    `mixed`: tfp_net_forward_bf16 - every product with bf16 operands, everything else as the extended entry point.
    `outs`: preallocated tensors to write instead of new ones, per network one per layer (None where nothing is stored); they are what is returned."""
    if not _walkable(nets):
        return None
    if ext is None:
        ext = any(needs_net_walk(layers) for _, layers in nets)
    ext = bool(ext or mixed)
    if norms is not None and not any(e is not None for e in norms):
        norms = None
    if norms is not None and not (len(norms) == len(nets) and all(e is None or _norm_ok(e, x.shape[1], x.device) for e, (x, _) in zip(norms, nets))):
        return None
    M = nets[0][0].shape[0]
    shapes = [[(M, _out_width(layers, l) if ext else w.shape[0]) if (store_hidden or l == len(layers) - 1) else None for l, (w, _, _, _) in enumerate(layers)]
              for _, layers in nets]
    if outs is None:
        outs = [[None if sh is None else torch.empty(sh, device=x.device, dtype=torch.float32) for sh in net] for net, (x, _) in zip(shapes, nets)]
    elif len(outs) != len(nets) or any(len(o) != len(net) or any((t is None) != (sh is None) or (t is not None and (
            t.dtype != torch.float32 or not t.is_contiguous() or tuple(t.shape) != sh or t.device != x.device)) for t, sh in zip(o, net))
            for o, net, (x, _) in zip(outs, shapes, nets)):
        raise ValueError(f"outs: per network one contiguous float32 tensor per stored layer output, shapes {shapes}, on the device of the input")
    blocks = [(x, layers, ys, None) for (x, layers), ys in zip(nets, outs)]
    return outs if _walk_launch("forward", blocks, ext, norms, M, _stream(nets[0][0]), mixed) else None


def mlp_walk_backward(nets, ext=None, mixed=False, outs=None):
    """nets: [(gy, ys, layers)]: gy = gradient of the network output, ys = the layer outputs the forward kept.  ONE launch for the whole input-gradient
    chain; returns per network the list dz with dz[l] = gradient of layer l's pre-activation (dz[-1] is gy itself), or None when the shapes do not fit.
    `outs`: preallocated dz tensors to write instead of new ones, per network one per layer but the last."""
    if not (0 < len(nets) <= 2) or any(len(layers) > WALK_MAXL or any(y is None for y in ys) for _, ys, layers in nets):
        return None
    if ext is None:
        ext = any(needs_net_walk(layers) for _, _, layers in nets)
    ext = bool(ext or mixed)
    M = nets[0][0].shape[0]
    given, outs, blocks = outs, [], []
    if given is not None and len(given) != len(nets):
        raise ValueError("outs: one list of dz tensors per network")
    for ni, (gy, ys, layers) in enumerate(nets):
        gy = gy if gy.is_contiguous() else gy.contiguous()
        for l in range(len(layers) - 1 if ext else 0):               # dZ covers the hidden part only; ys[l] may be the wide rows [h | x]
            if tuple(ys[l].shape) != (M, _out_width(layers, l)) or not ys[l].is_contiguous():
                raise ValueError(f"saved output of layer {l}: {tuple(ys[l].shape)}, contiguous {ys[l].is_contiguous()}; the walk stored and reads "
                                 f"({M}, {_out_width(layers, l)}) contiguous")
        shapes = [(M, layers[l][0].shape[0]) if ext else tuple(ys[l].shape) for l in range(len(layers) - 1)]
        if given is None:
            dz = [torch.empty(sh, device=gy.device, dtype=torch.float32) if ext else torch.empty_like(ys[l]) for l, sh in enumerate(shapes)]
        else:
            dz = list(given[ni])
            if len(dz) != len(shapes) or any(d.dtype != torch.float32 or not d.is_contiguous() or tuple(d.shape) != sh or d.device != gy.device
                                             for d, sh in zip(dz, shapes)):
                raise ValueError(f"outs: network {ni} takes contiguous float32 dz tensors of shapes {shapes} on the device of the gradient")
        blocks.append((gy, layers, dz, ys[:len(layers) - 1]))
        outs.append(dz + [gy])
    return outs if _walk_launch("backward", blocks, ext, None, M, _stream(nets[0][0]), mixed) else None


USE_WALK = True       # tools / tests switch it off to time or check the per-layer launches


# ---- the ONE place that decides how networks run: the walk, else grouped or per-layer launches (plain torch is decided by the caller: ppo.ActorCritic) ----
_WALK_ONLY = "a network with an activation other than ELU or with d2rl runs on the network walk only, and the walk declined these shapes"


_MIXED_ONLY = ("mixed_precision: a network with bf16 operands runs on the network walk only (there is no per-layer bf16 tier), and the walk declined these "
               "shapes or is switched off")


def _mixed_of(layer_lists):
    return any(bool(getattr(layers, "mixed", False)) for layers in layer_lists)


def _pairable(la, lc):
    return len(la) == len(lc) and all(a[2] == c[2] for a, c in zip(la, lc))


def forward_nets(nets, store_hidden=True, norms=None, mixed=None):
    """the forward of one or two networks [(x, layers)] over the same rows; returns the list of layer outputs per network.  In this order: ONE launch on the
    network walk (any activation code, d2rl: LayerLists); a network that needs the walk and was declined raises - the per-layer launches are ELU / none
    stacks and are never applied to a network that asked for something else (the trainer asks net_fits() once and runs such a network on torch); else the
    per-layer tier - two Linear / ELU stacks of the same depth and activations one grouped launch per layer (4 launches instead of 8 for the trainer's
    MLPs), anything else layer by layer.  `norms`: per network None or (mean_f, inv_std_f, clip): the inputs are RAW and normalised on the way in - inside
    the walk, or by one normalize_rows launch per network in front of the per-layer tier.  `mixed` (None: what the LayerLists say): `mixed_precision` - ONE
    launch of the walk with bf16 operands (tfp_net_forward_bf16) or a RuntimeError: there is no per-layer bf16 tier, the trainer asks net_fits(mixed=True)
    once and runs a network the walk declines on the torch statement."""
    if norms is not None and not any(e is not None for e in norms):
        norms = None
    if mixed is None:
        mixed = _mixed_of([layers for _, layers in nets])
    if mixed:
        out = mlp_walk_forward(nets, store_hidden, norms, mixed=True) if USE_WALK else None
        if out is None:
            raise RuntimeError(_MIXED_ONLY)
        return out
    if USE_WALK:
        out = mlp_walk_forward(nets, store_hidden, norms)
        if out is not None:
            return out
    if any(needs_net_walk(layers) for _, layers in nets):
        raise RuntimeError(_WALK_ONLY)
    if norms is not None:
        nets = [(normalize_rows(x, *e) if e is not None else x, layers) for (x, layers), e in zip(nets, norms)]
    if len(nets) != 2 or not _pairable(nets[0][1], nets[1][1]):
        return [mlp_forward(x, layers) for x, layers in nets]
    (xa, la), (xc, lc) = nets
    ya, yc = [], []
    for (wa, ba, act, _), (wc, bc, _, _) in zip(la, lc):
        out = linear_fwd_group([xa, xc], [wa, wc], [ba, bc], act)
        if out is None:
            out = [linear_fwd(xa, wa, ba, act), linear_fwd(xc, wc, bc, act)]
        xa, xc = out
        ya.append(xa); yc.append(xc)
    return [ya, yc]


def mlp_forward_pair(xa, la, xc, lc, store_hidden=True, norms=None):
    """forward_nets of the actor and the central value network side by side; `norms` = (actor's, critic's)"""
    ya, yc = forward_nets([(xa, la), (xc, lc)], store_hidden, norms)
    return ya, yc


def _weight_grads(gys, inps, ys, outs, direct=False, grouped=True, mixed=False):
    """the tail of a backward pass: the weight / bias gradient products (gy or dZ, layer input, grad_out) of the parallel lists, eight per launch - the
    direct kernel (`direct`: every dZ is plain) -> one grouped launch -> one by one.  ys: None, or per product the ELU output whose derivative the operand
    load forms.  Chunk sums deferred: flush_partial_sums().  `mixed`: the direct kernel with bf16 operands (every dZ is plain), and for a group it declines
    at run time the torch products of the rounded operands, written at once: gw = bf16r(gy).T @ bf16r(x), gb = gy.sum(0)"""
    for i in range(0, len(gys), 8):
        sl = slice(i, i + 8)
        if mixed:
            if not (USE_DIRECT_DW and gemm_tn_bias_direct(gys[sl], inps[sl], outs[sl], mixed=True)):
                _count("n_mixed_dw_torch")
                for gy, x, (gw, gb) in zip(gys[sl], inps[sl], outs[sl]):
                    torch.matmul(bf16r(gy).t(), bf16r(x), out=gw)
                    torch.sum(gy, 0, out=gb)
            continue
        if direct and USE_DIRECT_DW and gemm_tn_bias_direct(gys[sl], inps[sl], outs[sl]):
            continue
        if not (grouped and gemm_tn_bias_group(gys[sl], inps[sl], ys[sl] if ys is not None else None, outs[sl])):
            for k in range(i, min(i + 8, len(gys))):
                gemm_tn_bias(gys[k], inps[k], ys[k] if ys is not None else None, out=outs[k], defer=True)


def _backward_per_layer(nets):
    """the per-layer tier of backward_nets for one network or two pairable ones: the input-gradient product of layer k (of both in one launch), and the
    weight / bias gradient products behind them in two groups - operand load with elu', and without: their bits differ"""
    # gy is the gradient of layer k's OUTPUT at the top of the walk and the dZ of layer k - already times elu'(ys[k]) - below it: every input-gradient
    # product leaves multiplied by the activation derivative of the layer it is the gradient of (tfp_gemm_nn_dz), so the two products that consume it
    # stage plain operands.  Same bits as multiplying in their operand loads (one fp32 product either way).
    pair, acts = len(nets) == 2, [l[2] for l in nets[0][3]]
    gys = [gy for _, _, gy, _ in nets]
    dw = {True: ([], [], [], []), False: ([], [], [], [])}          # the operand load multiplies by elu' -> (gy, input, y, grad_out)
    is_dz = False
    for k in range(len(acts) - 1, -1, -1):
        act = bool(acts[k] and not is_dz)
        for (x, ys, _, layers), gy in zip(nets, gys):
            slot = dw[act]
            slot[0].append(gy); slot[1].append(ys[k - 1] if k > 0 else x); slot[2].append(ys[k]); slot[3].append(layers[k][3])
        if k > 0:
            ws = [layers[k][0] for _, _, _, layers in nets]
            yy = [ys[k] if act else None for _, ys, _, _ in nets]
            eo = [ys[k - 1] if acts[k - 1] else None for _, ys, _, _ in nets]
            out = gemm_nn_group(gys, ws, yy if act else None, eo if acts[k - 1] else None) if pair else None
            if out is None:
                out = [gemm_nn(gy, w, y, y_out=e) for gy, w, y, e in zip(gys, ws, yy, eo)]
            gys, is_dz = out, True
    for has_elu, (g, inps, ys, outs) in dw.items():
        _weight_grads(g, inps, ys if has_elu else None, outs, grouped=pair)


def backward_nets(nets, walk=True, mixed=None):
    """gradients of every layer's weight and bias of one or two networks [(x, ys, gy, layers)] into the layers' `grad_out` buffers, given the gradient
    `gy` of each network output; the input gradient of the first layer is not formed.  The counterpart of forward_nets, same order: the walk - ONE launch
    for every dZ, then all weight / bias gradients of the step as plain products dZ_l^T [input_l | 1] -, the refusal, the per-layer tier (5 launches
    instead of 14 for the trainer's MLPs).  Chunk sums deferred: call flush_partial_sums() afterwards.  `mixed` (None: what the LayerLists say): the walk
    and the direct weight gradients with bf16 operands, or a RuntimeError (no per-layer bf16 tier)."""
    if mixed is None:
        mixed = _mixed_of([layers for _, _, _, layers in nets])
    if mixed and not (walk and USE_WALK):
        raise RuntimeError(_MIXED_ONLY)
    if walk and USE_WALK:
        dz = mlp_walk_backward([(gy, ys, layers) for _, ys, gy, layers in nets], mixed=mixed)
        if dz is None and mixed:
            raise RuntimeError(_MIXED_ONLY)
        if dz is not None:
            gys, inps, outs = [], [], []
            for (x, ys, _, layers), d in zip(nets, dz):
                for k in range(len(layers) - 1, -1, -1):
                    gys.append(d[k]); inps.append(ys[k - 1] if k > 0 else x); outs.append(layers[k][3])
            _weight_grads(gys, inps, None, outs, direct=True, mixed=mixed)
            return
    if any(needs_net_walk(layers) for _, _, _, layers in nets):
        raise RuntimeError(_WALK_ONLY)
    if len(nets) == 2 and not _pairable(nets[0][3], nets[1][3]):
        for net in nets:
            _backward_per_layer([net])
        return
    _backward_per_layer(nets)


def mlp_backward_pair(xa, ya, gya, la, xc, yc, gyc, lc):
    """backward_nets of the actor and the central value network side by side"""
    backward_nets([(xa, ya, gya, la), (xc, yc, gyc, lc)])


def mlp_backward(x, ys, gy, layers):
    """backward_nets of one network on the per-layer launches (the walk is not asked)"""
    backward_nets([(x, ys, gy, layers)], walk=False)
