"""The value-side kernels (include/trifinger_ppo_value.h: tfp_gae_vnorm, tfp_ppo_loss_vclip) on the GPU and the trainer with `clip_value`,
`central_value_config.clip_value` and `normalize_value` on the HIP env.  References: the float32 torch expressions of the trainer's torch path (bit for bit
for tfp_gae_vnorm), the torch objective with the `where` form of the clipped value term, tfp_ppo_loss itself for an unreachable clip range."""
import math

import pytest
import torch

import leibnizgym_amd.ppo as ppo
from leibnizgym_amd import ppo_kernels as pk
from leibnizgym_amd.ppo import InputNorm, PPOConfig, PPOTrainer, neglogp
from value_path_util import E_CLIP, planted

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
CLIP = 5.0
GAMMA, TAU = 0.99, 0.95


# ---- tfp_gae_vnorm ---------------------------------------------------------------------------------------------------------------------------
def record(count, mean, std):
    rec = InputNorm(1, DEV)
    rec.state.copy_(torch.tensor([count, mean, std * std * count], dtype=torch.float64))
    rec.publish()
    return rec


def gae_vnorm_torch(rew, done, y, mean_f, inv_std_f, clip, gamma, tau):
    """the trainer's torch path, expression for expression"""
    T, n = rew.shape
    v = torch.clamp(y, -clip, clip) / inv_std_f + mean_f
    adv, last = torch.zeros(T, n, device=rew.device), torch.zeros(n, device=rew.device)
    for t in reversed(range(T)):
        nd = 1.0 - done[t]
        delta = rew[t] + gamma * v[t + 1] * nd - v[t]
        last = delta + gamma * tau * nd * last
        adv[t] = last
    ret = adv + v[:T]
    return adv, ret, torch.clamp((ret - mean_f) * inv_std_f, -clip, clip), torch.clamp(y[:T], -clip, clip)


@pytest.mark.parametrize("T", [1, 3, 32])
@pytest.mark.parametrize("n", [1, 63, 64, 65, 257, 1000])
def test_gae_vnorm_holds_the_bits_of_the_torch_expressions(hip, T, n):
    g = torch.Generator(device=DEV).manual_seed(100 * T + n)
    y = torch.randn(T + 1, n, device=DEV, generator=g) * 3
    y[0, 0], y[T, n - 1] = 7.5, -6.25                                     # beyond the clip on both sides, the bootstrap row included
    assert bool((y.abs() > CLIP).any())
    dones = {"none": torch.zeros(T, n, device=DEV), "all": torch.ones(T, n, device=DEV), "last step": torch.zeros(T, n, device=DEV)}
    dones["last step"][T - 1] = 1.0
    for name, rec in (("count 0", InputNorm(1, DEV)), ("std 1e-3", record(10, 0.5, 1e-3)), ("std 1e3", record(10, -2.0, 1e3)), ("mean 1e4", record(10, 1e4, 1.0))):
        scale = 1.0 / float(rec.inv_std_f)
        rew = torch.randn(T, n, device=DEV, generator=g) * scale * 0.3   # rewards of the size of the values they meet
        for dname, done in dones.items():
            want = gae_vnorm_torch(rew, done, y, rec.mean_f, rec.inv_std_f, CLIP, GAMMA, TAU)
            got = pk.gae_vnorm(rew, done, y, rec.mean_f, rec.inv_std_f, CLIP, GAMMA, TAU)
            for what, a, b in zip(("adv", "ret", "ret_n", "v_old_n"), got, want):
                assert a.shape == (T, n) and torch.equal(a, b), (name, dname, what, float((a - b).abs().max()))
    assert float(InputNorm(1, DEV).mean_f) == 0.0                         # count 0 published mean 0 / variance 1


# ---- tfp_ppo_loss_vclip ----------------------------------------------------------------------------------------------------------------------
def objective_inputs(B, A):
    """The tolerances below are those of a test whose log-std gradient has no component that cancels; a sum of B float32 terms carries an error of the
    order of 2^-24 * sum |terms|, so they can only be asked of sums whose terms do not cancel.  d_logstd[a] = sum_i g_i (1 - z_ia^2) with g_i proportional to
    adv_i: the inputs are built so that both factors keep a sign on average - z = (act - mu) / sigma ~ N(0, 0.5^2) for EVERY action (noise in units of that
    action's sigma), advantages with mean 1.5 and unit spread (7 % negative: both sides of the surrogate's clip are there).  `conditioning` states the
    property in float64 and the tests assert it: by construction of the inputs, not from anything the kernel returns."""
    g = torch.Generator(device=DEV).manual_seed(B + A)
    r = lambda *s: torch.randn(*s, device=DEV, generator=g)               # noqa: E731
    mu, ls = r(B, A) * 0.8, r(A) * 0.3 - 0.5
    act, old_mu = mu + r(B, A) * 0.5 * ls.exp(), mu + r(B, A) * 0.05
    adv = r(B) + 1.5
    old_nlp = neglogp(act, old_mu, ls.expand_as(old_mu)) + r(B) * 0.05
    v, ret, old_v = planted(B, DEV, seed=B)                               # the four regimes of the value term, cycled over the batch
    return mu, ls, v, act, old_nlp, adv, ret, old_mu, old_v


def conditioning(mu, ls, act, old_nlp, adv, e_clip):
    """max over the actions of sum_i |t_ia| / |sum_i t_ia|, t_ia = the term sample i adds to d_logstd[a] (float64, from the definition of the surrogate)"""
    mu, ls, act, old_nlp, adv = (t.double() for t in (mu, ls, act, old_nlp, adv))
    z = (act - mu) / ls.exp()
    ratio = (old_nlp - (0.5 * z * z + ls + 0.5 * math.log(2 * math.pi)).sum(-1)).exp()
    s1, s2 = -adv * ratio, -adv * ratio.clamp(1 - e_clip, 1 + e_clip)
    live = ((ratio >= 1 - e_clip) & (ratio <= 1 + e_clip)) | (s1 > s2)
    t = (torch.where(live, adv, torch.zeros_like(adv)) * ratio).unsqueeze(-1) * (1 - z * z)
    return float((t.abs().sum(0) / t.sum(0).abs()).max())


def reference(mu, ls, v, act, old_nlp, adv, ret, old_mu, old_v, e_clip, v_coef, ent_coef, bounds_coef):
    """the trainer's torch objective (tests/test_ppo_kernels.py: reference_loss) with the `where` form of the clipped value term"""
    nlp = neglogp(act, mu, ls.expand_as(mu))
    ratio = (old_nlp - nlp).exp()
    a_loss = torch.max(-adv * ratio, -adv * ratio.clamp(1 - e_clip, 1 + e_clip)).mean()
    c_loss = ppo.clipped_value_loss(v, ret, old_v, e_clip).mean()
    b_loss = ((mu - 1.1).clamp(min=0).pow(2) + (-1.1 - mu).clamp(min=0).pow(2)).sum(-1).mean()
    ent = (ls + 0.5 + 0.5 * math.log(2 * math.pi)).sum()
    kl = (0.5 * ((mu - old_mu) / ls.exp()).pow(2)).sum(-1).mean()
    return a_loss + v_coef * c_loss - ent_coef * ent + bounds_coef * b_loss, a_loss, c_loss, kl


@pytest.mark.parametrize("A", [9, 18])
@pytest.mark.parametrize("B", [1, 63, 64, 65, 255, 256, 257, 1000])
def test_clipped_objective_matches_torch_fp32(hip, B, A):
    """tolerances: those of tests/test_ppo_kernels.py::test_fused_objective_matches_torch_fp32 (the same reductions)"""
    mu0, ls0, v0, act, old_nlp, adv, ret, old_mu, old_v = objective_inputs(B, A)
    args = dict(e_clip=E_CLIP, v_coef=2.0, ent_coef=0.003, bounds_coef=1e-4)
    assert conditioning(mu0, ls0, act, old_nlp, adv, E_CLIP) <= 4.0 or B < 63      # the sums the tolerances are asked of do not cancel (a lone sample has no sum)
    mu, ls, v = (t.clone().requires_grad_(True) for t in (mu0, ls0, v0))
    loss, a_loss, c_loss, kl = reference(mu, ls, v, act, old_nlp, adv, ret, old_mu, old_v, **args)
    loss.backward()
    want_stats = torch.stack([loss.detach(), a_loss.detach(), c_loss.detach(), kl.detach()])
    stats = torch.zeros(4, device=DEV)
    got_loss, d_mu, d_v, d_ls = pk.ppo_loss_and_grads(mu0, ls0, v0, act, old_nlp, adv, ret, old_mu, stats, old_v=old_v, **args)
    assert torch.allclose(loss.detach(), got_loss, rtol=2e-5, atol=1e-6)
    assert torch.allclose(want_stats, stats, rtol=2e-5, atol=1e-6)
    assert torch.allclose(mu.grad, d_mu, rtol=1e-4, atol=1e-9) and torch.allclose(v.grad, d_v, rtol=1e-5, atol=1e-10)
    assert torch.allclose(ls.grad, d_ls, rtol=2e-4, atol=1e-7)
    if B >= 7:                                                            # the clipped branch was there: samples without a value gradient, in both paths
        assert bool((d_v == 0).any()) and torch.equal(d_v == 0, v.grad == 0)


@pytest.mark.parametrize("A", [9, 18])
@pytest.mark.parametrize("B", [1, 63, 64, 65, 255, 256, 257, 1000])
def test_unreachable_clip_range_is_the_unclipped_objective_bit_for_bit(hip, B, A):
    """old_v given, e = 1e30 (every ratio and every value inside the range in BOTH calls): the results of tfp_ppo_loss on the same inputs, bit for bit.
    d_mu and d_v are per sample: the same bits at every size.  loss, d_logstd and stats are sums over the blocks of 256 samples, added with one atomic per
    block in the order the blocks arrive (csrc/ppo_kernels.hip: "results as before up to the order of the atomic sums") - the same bits up to two blocks,
    where the order cannot matter (B <= 512: every size but the last).  At B = 1000, four blocks, tfp_ppo_loss is not bit-reproducible against ITSELF by
    contract; there the sums of the two kernels may differ by what reordering four addends can do and by no more: three additions per order, each
    rounding at most half an ulp of a partial sum bounded by S = the sum of the magnitudes of the terms: |difference| <= 2 * 3 * 2^-24 * S."""
    mu, ls, v, act, old_nlp, adv, ret, old_mu, old_v = objective_inputs(B, A)
    args = dict(v_coef=2.0, ent_coef=0.003, bounds_coef=1e-4)
    s0, s1 = torch.zeros(4, device=DEV), torch.zeros(4, device=DEV)
    plain = pk.ppo_loss_and_grads(mu, ls, v, act, old_nlp, adv, ret, old_mu, s0, e_clip=1e30, **args)
    clip = pk.ppo_loss_and_grads(mu, ls, v, act, old_nlp, adv, ret, old_mu, s1, e_clip=1e30, old_v=old_v, **args)
    assert torch.equal(plain[1], clip[1]) and torch.equal(plain[2], clip[2])                       # d_mu, d_v
    sums = (("loss", plain[0], clip[0]), ("d_logstd", plain[3], clip[3]), ("stats", s0, s1))
    if (B + 255) // 256 <= 2:
        for what, a, b in sums:
            assert torch.equal(a, b), (what, float((a - b).abs().max()))
        return
    # the magnitudes of the terms each sum is made of (float64 from the float32 inputs; the bound needs no more than their size)
    d = lambda t: t.double()                                              # noqa: E731
    z = (d(act) - d(mu)) / d(ls).exp()
    ratio = (d(old_nlp) - (0.5 * z * z + d(ls) + 0.5 * math.log(2 * math.pi)).sum(-1)).exp()
    a_abs, c_abs = (d(adv) * ratio).abs().mean(), ((d(v) - d(ret)) ** 2).mean()
    b_abs = ((d(mu) - 1.1).clamp(min=0) ** 2 + (-1.1 - d(mu)).clamp(min=0) ** 2).sum(-1).mean()
    kl_abs = (0.5 * ((d(mu) - d(old_mu)) / d(ls).exp()) ** 2).sum(-1).mean()
    ent_abs = args["ent_coef"] * (d(ls) + 0.5 + 0.5 * math.log(2 * math.pi)).sum().abs()
    loss_abs = a_abs + args["v_coef"] * c_abs + args["bounds_coef"] * b_abs + ent_abs
    dls_abs = ((d(adv) * ratio).abs().unsqueeze(-1) * (1 - z * z).abs()).mean(0) + args["ent_coef"]
    slack = 2 * 3 * 2.0 ** -24
    for what, a, b, S in (("loss", plain[0], clip[0], loss_abs), ("d_logstd", plain[3], clip[3], dls_abs),
                          ("stats", s0, s1, torch.stack([loss_abs, a_abs, c_abs, kl_abs]))):
        diff = (d(a) - d(b)).abs()
        print(f"B {B} A {A} {what}: max |difference| {float(diff.max()):.3e}, bound {float((slack * S).min()):.3e}")
        assert bool((diff <= slack * S).all()), what


# ---- the trainer on the HIP env --------------------------------------------------------------------------------------------------------------
def hip_trainer(n, T=4, **kw):
    from leibnizgym_amd.config import gym_config
    from leibnizgym_amd.envs import TrifingerEnv
    from leibnizgym_amd.utils.rlg_train import RlGamesGpuEnvAdapter
    from leibnizgym_amd.wrappers import VecTaskPython
    cfg = gym_config("trifinger_difficulty_4")
    cfg.update(num_instances=n, seed=1, physics_engine="physx", asymmetric_obs=True, episode_length=20)
    env = TrifingerEnv(config=cfg, device=DEV, verbose=False)
    ad = RlGamesGpuEnvAdapter("rlgpu", n, env=VecTaskPython(env, rl_device=DEV))
    return PPOTrainer(ad, 41, 113, 9, PPOConfig(horizon=T, minibatches=4, mini_epochs=2, **kw), device=DEV)


def test_trainer_with_every_key_on_with_and_without_the_kernels(hip, monkeypatch):
    """256 envs, horizon 4, 2 epochs, from the same seed.  The records of the two runs are moments of float32 buffers that the two runs fill through different
    GEMMs (the MFMA kernels / torch's), so beside the relative bound of 1e-9 they get the absolute one the parameters of the same two runs get in
    tests/test_ppo_kernels.py::test_trainer_with_and_without_the_kernels (3e-5), applied to mean and variance (M2 / count); the counts are equal."""
    n, T = 256, 4
    calls = []
    gae_vnorm, loss = pk.gae_vnorm, pk.ppo_loss_and_grads
    monkeypatch.setattr(pk, "gae_vnorm", lambda *a, **k: (calls.append("gae_vnorm"), gae_vnorm(*a, **k))[1])
    monkeypatch.setattr(pk, "ppo_loss_and_grads", lambda *a, **k: (calls.append("vclip" if k.get("old_v") is not None else "plain"), loss(*a, **k))[1])

    def run(fused):
        tr = hip_trainer(n, T, fused_kernels=fused, clip_value=True, clip_value_central=True, normalize_value=True, normalize_input=True,
                         normalize_input_value=True)
        torch.manual_seed(11)
        stats = tr.train(2)
        assert tr.frames == 2 * T * n
        return tr, stats
    t0, s0 = run(False)
    assert calls == []
    t1, s1 = run(True)
    assert calls.count("gae_vnorm") == 2 and calls.count("vclip") == 2 * 2 * 4 and "plain" not in calls       # the fused path was taken
    for st in s0 + s1:
        assert all(math.isfinite(st[k]) for k in ("loss", "a_loss", "c_loss", "kl"))
    for a, b in zip(t0.net.parameters(), t1.net.parameters()):
        assert torch.allclose(a, b, atol=3e-5, rtol=1e-3)
    for k in ("loss", "a_loss", "c_loss", "kl"):
        assert abs(s0[-1][k] - s1[-1][k]) < 1e-3 * max(1.0, abs(s0[-1][k])), (k, s0[-1][k], s1[-1][k])
    for name, a, b in (("returns", t0.value_norm, t1.value_norm), ("obs", t0.net.obs_norm, t1.net.obs_norm), ("states", t0.net.state_norm, t1.net.state_norm)):
        assert float(a.count) == float(b.count) == 2 * T * n
        va, vb = a.m2 / a.count, b.m2 / b.count
        print(f"record {name}: max |mean diff| {float((a.mean - b.mean).abs().max()):.3e}  max |var diff| {float((va - vb).abs().max()):.3e}")
        assert torch.allclose(a.mean, b.mean, rtol=1e-9, atol=3e-5), name
        assert torch.allclose(va, vb, rtol=1e-9, atol=3e-5), name


def test_off_is_off_on_the_gpu(hip, monkeypatch):
    def boom(*a, **k):
        raise AssertionError("a function of the value path ran with its keys off")
    loss = pk.ppo_loss_and_grads
    monkeypatch.setattr(pk, "gae_vnorm", boom)
    monkeypatch.setattr(pk, "ppo_loss_and_grads", lambda *a, **k: boom() if "old_v" in k else loss(*a, **k))
    merge = PPOTrainer._update_input_norm                  # the returns join the end-of-epoch merge through its `returns` argument
    monkeypatch.setattr(PPOTrainer, "_update_input_norm", lambda self, src, returns=None: boom() if returns is not None else merge(self, src))
    tr = hip_trainer(256)
    stats = tr.train(2)
    assert tr.frames == 2 * 4 * 256 and all(math.isfinite(st["loss"]) for st in stats)
    assert "value_norm" not in tr.state_dict() and tr.value_norm is None
