"""The episode-end kernels (include/trifinger_ppo_episode.h: tfp_rollout_flags, tfp_gae_ends, tfp_ppo_loss_w, tfp_ppo_loss_vclip_w) on the GPU and the
trainer with `episode_ends` / `value_bootstrap` on the HIP env.  References: the torch expressions of the trainer's torch path run on the same GPU tensors
(bit for bit for the rollout kernels; ppo.gae_with_ends is the specification), the existing kernels for the cases in which the new ones must be them
(tfp_gae, tfp_gae_vnorm; tfp_ppo_loss / tfp_ppo_loss_vclip for w = 1), and the float64 torch objective with weights at the tolerances of
tests/test_value_path_gpu.py, whose inputs (`objective_inputs`) and records these tests share."""
import math

import numpy as np
import pytest
import torch

import leibnizgym_amd.ppo as ppo
import test_value_path_gpu as vp
from leibnizgym_amd import ppo_kernels as pk
from leibnizgym_amd.ppo import InputNorm, PPOConfig, PPOTrainer, denormalize_value, gae_with_ends, masked_advantage_norm, neglogp
from value_path_util import E_CLIP

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
CLIP = 5.0
GAMMA, TAU = 0.99, 0.95
SIZES = [1, 63, 64, 65, 257]


# ---- tfp_rollout_flags -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", SIZES)
def test_rollout_flags_holds_the_bits_of_the_torch_expressions(hip, n):
    g = torch.Generator().manual_seed(n)
    L = 5
    r = torch.randn(n, generator=g).to(DEV)
    steps = torch.randint(0, 2 * L, (n,), generator=g)
    steps[0] = L                                                          # the limit itself is a time-out
    reset = torch.tensor([0, 1, 2, 255], dtype=torch.uint8)[torch.randint(0, 4, (n,), generator=g)]
    if n >= 63:
        steps[1], steps[2], steps[3] = L - 1, 2 ** 33, 0                  # below the limit; beyond int32
        assert bool((steps < L).any()) and bool((steps >= L).any()) and all(bool((reset == k).any()) for k in (0, 1, 2, 255))
    steps, reset = steps.to(DEV), reset.to(DEV)
    scale = 0.01
    for rb in (reset, reset != 0):                                        # uint8 with values other than 0 and 1; torch.bool
        for ep_len in (L, 0, -3):
            out = torch.full((3, n), 7.0, device=DEV)
            pk.rollout_flags(r, rb, steps, scale, ep_len, out[0], out[1], out[2])
            assert torch.equal(out[0], r * scale), "rew"
            assert torch.equal(out[1], (rb != 0).float()), "end"
            assert torch.equal(out[2], (steps >= ep_len).float() if ep_len > 0 else torch.zeros(n, device=DEV)), "tout"
    assert torch.equal(steps.cpu()[:1], torch.tensor([L])) and reset.dtype == torch.uint8          # the engine's buffers are only read


# ---- tfp_gae_ends ----------------------------------------------------------------------------------------------------------------------------
def flags(T, n):
    """seeded flags, P(end) = 0.2, half of the ends time-outs, with the cases a rollout of this size can hold planted into env 0; the presence of every
    case is asserted on the inputs.  (end, tout, last_end) on the CPU"""
    g = torch.Generator().manual_seed(1000 * T + n)
    end = (torch.rand(T, n, generator=g) < 0.2).float()
    tout = end * (torch.rand(T, n, generator=g) < 0.5).float()
    last_end = (torch.rand(n, generator=g) < 0.2).float()
    last_end[0] = 1.0                                                     # a stale t = 0
    if T >= 3:
        end[0, 0], tout[0, 0] = 1.0, 0.0                                  # a termination, behind last_end = 1: two ends in a row, and again with t = 1
        end[1, 0], tout[1, 0] = 1.0, 1.0
    end[T - 1, 0], tout[T - 1, 0] = 1.0, 1.0                              # a time-out, at T - 1
    prev = torch.cat([last_end.unsqueeze(0), end[:-1]])
    assert bool(((end == 1) & (tout == 1)).any()) and bool((last_end == 1).any()) and bool((end[T - 1] == 1).any()) and bool(((end == 1) & (prev == 1)).any())
    if T >= 3:
        assert bool(((end == 1) & (tout == 0)).any())
    assert bool((tout <= end).all())
    return end, tout, last_end


def records():
    return (("count 0", InputNorm(1, DEV)), ("std 1e-3", vp.record(10, 0.5, 1e-3)), ("std 1e3", vp.record(10, -2.0, 1e3)), ("mean 1e4", vp.record(10, 1e4, 1.0)))


@pytest.mark.parametrize("T", [1, 3, 32])
@pytest.mark.parametrize("n", SIZES)
def test_gae_ends_holds_the_bits_of_gae_with_ends(hip, T, n):
    end, tout, last_end = (t.to(DEV) for t in flags(T, n))
    g = torch.Generator(device=DEV).manual_seed(100 * T + n)
    y = torch.randn(T + 1, n, device=DEV, generator=g) * 3
    y[0, 0], y[T, n - 1] = 7.5, -6.25                                     # beyond the clip on both sides, the bootstrap row included
    zero, zero_n = torch.zeros(T, n, device=DEV), torch.zeros(n, device=DEV)
    rew = torch.randn(T, n, device=DEV, generator=g) * 0.3
    for boot in (False, True):
        got = pk.gae_ends(rew, end, tout, y, last_end, GAMMA, TAU, boot)
        want = gae_with_ends(rew, end, tout, y, last_end, GAMMA, TAU, boot)
        for what, a, b in zip(("adv", "ret", "w"), got, want):
            assert a.shape == (T, n) and torch.equal(a, b), (boot, what, float((a - b).abs().max()))
        assert bool((got[0][got[2] == 0] == 0).all()) and torch.equal(got[1][got[2] == 0], y[:T][got[2] == 0])
        # no end anywhere: tfp_gae
        adv, ret, w = pk.gae_ends(rew, zero, tout, y, zero_n, GAMMA, TAU, boot)
        a0, r0 = pk.gae(rew, zero, y, GAMMA, TAU)
        assert torch.equal(adv, a0) and torch.equal(ret, r0) and bool((w == 1).all())
    live_tout = bool(((tout == 1) & (got[2] == 1)).any())                 # a time-out on a sample that is not stale: there the two settings differ
    assert live_tout or n == 1
    if live_tout:
        assert not torch.equal(pk.gae_ends(rew, end, tout, y, last_end, GAMMA, TAU, False)[0], pk.gae_ends(rew, end, tout, y, last_end, GAMMA, TAU, True)[0])
    for name, rec in records():
        rew = torch.randn(T, n, device=DEV, generator=g) * (0.3 / float(rec.inv_std_f))      # rewards of the size of the values they meet
        v = denormalize_value(y, rec)
        for boot in (False, True):
            got = pk.gae_ends(rew, end, tout, y, last_end, GAMMA, TAU, boot, rec.mean_f, rec.inv_std_f, CLIP)
            adv, ret, w = gae_with_ends(rew, end, tout, v, last_end, GAMMA, TAU, boot)
            want = (adv, ret, w, torch.clamp((ret - rec.mean_f) * rec.inv_std_f, -CLIP, CLIP), torch.clamp(y[:T], -CLIP, CLIP))
            for what, a, b in zip(("adv", "ret", "w", "ret_n", "v_old_n"), got, want):
                assert a.shape == (T, n) and torch.equal(a, b), (name, boot, what, float((a - b).abs().max()))
            # no end anywhere: tfp_gae_vnorm
            got = pk.gae_ends(rew, zero, tout, y, zero_n, GAMMA, TAU, boot, rec.mean_f, rec.inv_std_f, CLIP)
            want = pk.gae_vnorm(rew, zero, y, rec.mean_f, rec.inv_std_f, CLIP, GAMMA, TAU)
            for what, a, b in zip(("adv", "ret", "ret_n", "v_old_n"), (got[0], got[1], got[3], got[4]), want):
                assert torch.equal(a, b), (name, boot, what)
            assert bool((got[2] == 1).all())


# ---- tfp_ppo_loss_w / tfp_ppo_loss_vclip_w ---------------------------------------------------------------------------------------------------
ARGS = dict(e_clip=E_CLIP, v_coef=2.0, ent_coef=0.003, bounds_coef=1e-4)


def weighted_reference(mu, ls, v, act, old_nlp, adv, ret, old_mu, old_v, w, e_clip, v_coef, ent_coef, bounds_coef):
    """the objective of csrc/ppo_kernels.hip with every per-sample term times w_i and the divisor B; float64 when the inputs are.  old_v None: no value clip"""
    wm = lambda x: (w * x).mean()                                         # noqa: E731
    nlp = neglogp(act, mu, ls.expand_as(mu))
    ratio = (old_nlp - nlp).exp()
    a_loss = wm(torch.max(-adv * ratio, -adv * ratio.clamp(1 - e_clip, 1 + e_clip)))
    c_loss = wm(ppo.clipped_value_loss(v, ret, old_v, e_clip) if old_v is not None else (v - ret).pow(2))
    b_loss = wm(((mu - 1.1).clamp(min=0).pow(2) + (-1.1 - mu).clamp(min=0).pow(2)).sum(-1))
    ent = (ls + 0.5 + 0.5 * math.log(2 * math.pi)).sum()
    kl = wm((0.5 * ((mu - old_mu) / ls.exp()).pow(2)).sum(-1))
    return a_loss + v_coef * c_loss - ent_coef * ent + bounds_coef * b_loss, a_loss, c_loss, kl


@pytest.mark.parametrize("A", [9, 18])
@pytest.mark.parametrize("B", [1, 255, 256, 257, 1000])
@pytest.mark.parametrize("vclip", [False, True], ids=["plain", "vclip"])
def test_weighted_objective(hip, B, A, vclip):
    """tolerances: those of tests/test_value_path_gpu.py::test_clipped_objective_matches_torch_fp32, quantity for quantity"""
    mu0, ls0, v0, act, old_nlp, adv, ret, old_mu, old_v = vp.objective_inputs(B, A)
    kw = {"old_v": old_v} if vclip else {}
    run = lambda w: (lambda s: pk.ppo_loss_and_grads(mu0, ls0, v0, act, old_nlp, None, ret, old_mu, s, adv_w=torch.stack([adv, w], 1).contiguous(),   # noqa: E731
                                                     **kw, **ARGS) + (s,))(torch.zeros(4, device=DEV))
    # w = 1: the unweighted entry point - d_mu and d_v bit for bit, the sums (atomics over the blocks) within the tolerances
    s0 = torch.zeros(4, device=DEV)
    loss0, d_mu0, d_v0, d_ls0 = pk.ppo_loss_and_grads(mu0, ls0, v0, act, old_nlp, adv, ret, old_mu, s0, **kw, **ARGS)
    loss1, d_mu1, d_v1, d_ls1, s1 = run(torch.ones(B, device=DEV))
    assert torch.equal(d_mu0, d_mu1) and torch.equal(d_v0, d_v1)
    assert torch.allclose(loss0, loss1, rtol=2e-5, atol=1e-6) and torch.allclose(s0, s1, rtol=2e-5, atol=1e-6) and torch.allclose(d_ls0, d_ls1, rtol=2e-4, atol=1e-7)
    # a seeded mask, about a quarter zeros, against the float64 objective with weights
    w = (torch.rand(B, generator=torch.Generator().manual_seed(B + A)) >= 0.25).float().to(DEV)
    if B >= 255:
        assert 0.15 <= 1.0 - float(w.mean()) <= 0.35
    d = lambda t: t.double()                                              # noqa: E731
    print(f"B {B} A {A}: conditioning of the weighted log-std gradient {vp.conditioning(mu0, ls0, act, old_nlp, adv * w, E_CLIP):.2f}")
    mu, ls, v = (d(t).clone().requires_grad_(True) for t in (mu0, ls0, v0))
    loss, a_loss, c_loss, kl = weighted_reference(mu, ls, v, d(act), d(old_nlp), d(adv), d(ret), d(old_mu), d(old_v) if vclip else None, d(w), **ARGS)
    loss.backward()
    want_stats = torch.stack([loss.detach(), a_loss.detach(), c_loss.detach(), kl.detach()]).float()
    got_loss, d_mu, d_v, d_ls, stats = run(w)
    assert torch.allclose(loss.detach().float(), got_loss, rtol=2e-5, atol=1e-6)
    assert torch.allclose(want_stats, stats, rtol=2e-5, atol=1e-6)
    assert torch.allclose(mu.grad.float(), d_mu, rtol=1e-4, atol=1e-9) and torch.allclose(v.grad.float(), d_v, rtol=1e-5, atol=1e-10)
    assert torch.allclose(ls.grad.float(), d_ls, rtol=2e-4, atol=1e-7)
    assert bool((d_mu[w == 0] == 0).all()) and bool((d_v[w == 0] == 0).all())                     # a stale row: exactly zero
    if B >= 255:                                                          # (a live row may still be all zero: the clipped branch of the surrogate has no gradient)
        assert bool((d_mu[w == 1] != 0).any()) and bool((d_v[w == 1] != 0).any())
    # w = 0 throughout: the batch-independent entropy term is all that is left, exactly
    got_loss, d_mu, d_v, d_ls, stats = run(torch.zeros(B, device=DEV))
    assert bool((d_mu == 0).all()) and bool((d_v == 0).all())
    ec = np.float32(ARGS["ent_coef"])
    assert torch.equal(d_ls, torch.full((A,), -float(ec), device=DEV))
    ent = np.float32(0.0)
    for x in ls0.cpu().numpy():                                           # the kernel's order: ent += ls[a] + 1.4189385...f, one rounding each
        ent = np.float32(ent + np.float32(x + np.float32(1.4189385332046727)))
    want = np.float32(-(np.float64(ec) * np.float64(ent)))                # one rounding of the exact product, whether or not it is contracted into the sum
    assert float(got_loss) == float(want), (float(got_loss), float(want))
    assert float(stats[0]) == float(want) and stats[1:].tolist() == [0.0, 0.0, 0.0]


def test_reset_state_serves_the_weighted_variants(hip):
    """after the variants ran, tfp_reset_state leaves the zero state: the next call gives the bits of the first (257 samples, two blocks: the order of the
    atomics cannot matter)"""
    mu, ls, v, act, old_nlp, adv, ret, old_mu, old_v = vp.objective_inputs(257, 9)
    aw = torch.stack([adv, (torch.arange(257, device=DEV) % 4 != 0).float()], 1).contiguous()

    def run(**kw):
        s = torch.zeros(4, device=DEV)
        return pk.ppo_loss_and_grads(mu, ls, v, act, old_nlp, None, ret, old_mu, s, adv_w=aw, **kw, **ARGS) + (s,)
    first = [run(), run(old_v=old_v)]
    pk.reset_state(DEV)
    again = [run(), run(old_v=old_v)]
    for a, b in zip(first, again):
        assert all(torch.equal(x, y) for x, y in zip(a, b))
    s = torch.zeros(4, device=DEV)
    plain = pk.ppo_loss_and_grads(mu, ls, v, act, old_nlp, adv, ret, old_mu, s, **ARGS)           # ... and the unweighted entry point behind them
    pk.reset_state(DEV)
    s2 = torch.zeros(4, device=DEV)
    assert all(torch.equal(x, y) for x, y in zip(plain, pk.ppo_loss_and_grads(mu, ls, v, act, old_nlp, adv, ret, old_mu, s2, **ARGS))) and torch.equal(s, s2)
    lib = pk.load()
    p = 4096                                                              # never dereferenced: refused on the host
    assert lib.tfp_ppo_loss_w(p, p, p, p, p + 4, p, p, p, 8, 9, 0.2, 1.0, 0.0, 0.0, p, p, p, p, p, None) == -1      # (adv, w) pairs must be 8-byte aligned
    assert lib.tfp_ppo_loss_w(p, p, p, p, p, p, p, p, 8, 10, 0.2, 1.0, 0.0, 0.0, p, p, p, p, p, None) == -1
    assert lib.tfp_ppo_loss_vclip_w(p, p, p, p, p, p, p, p, None, 8, 9, 0.2, 1.0, 0.0, 0.0, p, p, p, p, p, None) == -1
    assert lib.tfp_gae_ends(p, p, p, p, p, 0, p, None, 5.0, 0.99, 0.94, 4, 4, p, p, p, p, p, None) == -1
    assert lib.tfp_gae_ends(p, p, p, p, p, 0, None, None, 0.0, 0.99, 0.94, 0, 4, p, p, p, None, None, None) == -1
    assert lib.tfp_rollout_flags(p, p, p, 0.01, 5, 0, p, p, p, None) == -1


# ---- the trainer on the HIP env --------------------------------------------------------------------------------------------------------------
N, EP_LEN, T = 65, 5, 8


def hip_trainer(**kw):
    from leibnizgym_amd.config import gym_config
    from leibnizgym_amd.envs import TrifingerEnv
    from leibnizgym_amd.utils.rlg_train import RlGamesGpuEnvAdapter
    from leibnizgym_amd.wrappers import VecTaskPython
    cfg = gym_config("trifinger_difficulty_4")
    cfg.update(num_instances=N, seed=1, physics_engine="physx", asymmetric_obs=True, episode_length=EP_LEN)
    env = TrifingerEnv(config=cfg, device=DEV, verbose=False)
    ad = RlGamesGpuEnvAdapter("rlgpu", N, env=VecTaskPython(env, rl_device=DEV))
    return PPOTrainer(ad, 41, 113, 9, PPOConfig(horizon=T, minibatches=4, mini_epochs=2, **kw), device=DEV)


@pytest.mark.parametrize("boot", [False, True], ids=["terminal", "value_bootstrap"])
def test_trainer_with_episode_ends_on_the_hip_env(hip, monkeypatch, boot):
    """65 envs, episode_length 5, horizon 8, normalize_value and central_value_config.clip_value on: the gather carries its full eight arrays"""
    calls = []
    for name in ("rollout_flags", "gae_ends", "rollout_reward", "gae", "gae_vnorm"):
        monkeypatch.setattr(pk, name, lambda *a, _f=getattr(pk, name), _n=name, **k: (calls.append(_n), _f(*a, **k))[1])
    loss, gather = pk.ppo_loss_and_grads, pk.gather_rows
    monkeypatch.setattr(pk, "ppo_loss_and_grads", lambda *a, **k: (calls.append("loss_w" if k.get("adv_w") is not None else "loss"), loss(*a, **k))[1])
    monkeypatch.setattr(pk, "gather_rows", lambda srcs, *a, **k: (calls.append(f"gather{len(srcs)}"), gather(srcs, *a, **k))[1])
    keys = dict(episode_ends=True, value_bootstrap=boot, normalize_value=True, clip_value_central=True)
    tr = hip_trainer(**keys)
    ref = hip_trainer(fused_kernels=False, **keys)                        # the same seed: the same initial weights
    assert tr.fused_loss and not ref.fused_loss and all(torch.equal(a, b) for a, b in zip(tr.net.parameters(), ref.net.parameters()))
    vn = tr.value_norm
    last_end = tr.last_end.clone()
    buf = tr.rollout()
    assert calls.count("rollout_flags") == T and calls.count("gae_ends") == 1 and not {"rollout_reward", "gae", "gae_vnorm"} & set(calls)
    assert torch.equal(buf["end"][EP_LEN - 1], torch.ones(N, device=DEV)) and float(buf["end"].sum()) == N and torch.equal(buf["end"], buf["tout"])
    adv, ret, w = gae_with_ends(buf["rew"], buf["end"], buf["tout"], denormalize_value(buf["val"], vn), last_end, GAMMA, TAU, boot)
    assert torch.equal(buf["adv"], adv) and torch.equal(buf["ret"], ret) and torch.equal(buf["w"], w)
    assert torch.equal(buf["ret_n"], torch.clamp((ret - vn.mean_f) * vn.inv_std_f, -vn.clip, vn.clip))
    assert float((w == 0).sum()) == N and torch.equal(tr.last_end, buf["end"][T - 1])
    # one minibatch step of all T n samples, kernels against the torch path: the tolerance of tests/test_ppo_kernels.py::test_trainer_with_and_without_the_kernels
    flat = lambda x: x.reshape(T * N, *x.shape[2:])                       # noqa: E731
    a_n, wf = masked_advantage_norm(flat(buf["adv"]), flat(buf["w"])), flat(buf["w"])
    d = dict(obs=flat(buf["obs"]), states=flat(buf["states"]), act=flat(buf["act"]), old_nlp=flat(buf["nlp"]), ret=flat(buf["ret_n"]), adv=a_n,
             old_mu=flat(buf["mu"]), old_v=flat(buf["v_old_n"]), w=wf, adv_w=torch.stack([a_n, wf], dim=1))
    idx = torch.randperm(T * N, device=DEV)
    before = [p.detach().clone() for p in tr.net.parameters()]
    accs = []
    for t in (tr, ref):
        accs.append(t._new_acc(DEV))
        t._mb_backward(d, idx, accs[-1])
        t._mb_apply()
    assert calls.count("loss_w") == 1 and "loss" not in calls and calls.count("gather8") == 1
    for a, b, c in zip(tr.net.parameters(), ref.net.parameters(), before):
        assert torch.allclose(a, b, atol=3e-5, rtol=1e-3) and not torch.equal(a, c)
    for k in ("loss", "a_loss", "c_loss", "kl"):
        x, y = float(accs[0][k]), float(accs[1][k])
        assert abs(x - y) < 1e-3 * max(1.0, abs(y)), (k, x, y)
    # two epochs: finite, the ends counted, and no collective in a world of one process
    stats = tr.train(2)
    assert all(math.isfinite(st[k]) for st in stats for k in ("loss", "a_loss", "c_loss", "kl")) and all(st["episodes_ended"] >= N for st in stats)
    assert (tr.n_grad_allreduce, tr.n_kl_allreduce, tr.n_norm_allgather, tr.n_eval_allreduce) == (0, 0, 0, 0) and not tr.dist_on
    assert "loss" not in calls and not {"rollout_reward", "gae", "gae_vnorm"} & set(calls)
