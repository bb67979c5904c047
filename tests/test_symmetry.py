"""`symmetry_augmentation` of the in-repo PPO on the CPU (leibnizgym_amd/symmetry.py, leibnizgym_amd/ppo.py: the module docstrings have the definitions): the
tables as matrices, the map against one step of the oracle (tests/symmetry_util.py restates it in float64 on the engine's state rows), the torch-path
minibatch against three explicitly transformed minibatches, the trainer on the oracle env, the refusals and the key off.  The kernels' side is
tests/test_symmetry_gpu.py.

Equivariance, measured on the oracle in the scenario of symmetry_util.scenario (69 of the 128 pairs have no live finger contact row on either side), max
|apply(first half) - second half| per block; the bounds are ten times these (symmetry_util.MEASURED / BOUNDS):
    obs 5.6e-6; object linear velocity 1.5e-4, angular velocity 4.9e-3 (the cube rests on its floor corners with friction rows along world x / y: the
    solver's pyramid, not an error of the map); fingertip position 3.0e-8, quaternion 2.1e-7, linear velocity 3.6e-7, angular velocity 1.9e-6; joint torque
    and fingertip wrench 0 (exact); reward 1.3e-4 relative.  The turn taken the other way: 1.7 in obs."""
import copy
import math

import numpy as np
import pytest
import torch

import leibnizgym_amd.ppo as ppo
import symmetry_util as su
from leibnizgym_amd import symmetry as sy
from leibnizgym_amd.config import RLG_ASYMM
from leibnizgym_amd.ppo import PPOConfig, PPOTrainer
from minibatch_step_util import StubEnv, objective


# ---- the tables ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("asym", [False, True], ids=["obs", "obs+states"])
@pytest.mark.parametrize("A", [9, 18])
def test_tables_are_orthogonal_and_of_order_three(A, asym):
    tabs = sy.trifinger_symmetry(A, asym)
    assert (tabs["states"] is None) == (not asym)
    widths = {"obs": 32 + A, "states": 32 + A + 72, "action": A}
    for key, pair in tabs.items():
        if pair is None:
            continue
        w = widths[key]
        for ia, ib, ca, cb in pair:
            assert ia.dtype == ib.dtype == torch.int64 and ca.dtype == cb.dtype == torch.float32 and all(t.shape == (w,) for t in (ia, ib, ca, cb))
            assert int(ia.min()) >= 0 and int(ib.min()) >= 0 and int(ia.max()) < w and int(ib.max()) < w
        M1, M2 = sy.table_matrix(pair[0]), sy.table_matrix(pair[1])
        eye = np.eye(w)
        assert np.abs(M1.T @ M1 - eye).max() <= 1e-6 and np.abs(M2.T @ M2 - eye).max() <= 1e-6
        assert np.abs(M2 - M1 @ M1).max() <= 1e-7                           # G^2 is the composition (rounded once)
        want = eye.copy()
        if key != "action":                                                 # -1 on the object and goal quaternion: the same rotation
            for q0 in (21, 28):
                want[q0:q0 + 4, q0:q0 + 4] *= -1.0
        assert np.abs(M2 @ M1 - want).max() <= 1e-6, key
        # `apply` is the table read as a matrix
        x = torch.randn(5, w, generator=torch.Generator().manual_seed(w), dtype=torch.float64)
        assert np.abs(sy.apply(x, pair[0]).numpy() - x.numpy() @ M1.T).max() <= 1e-12
    # a permuted column keeps -0, inf and NaN; the action map is the finger permutation per block of 9
    a = torch.arange(A, dtype=torch.float32).unsqueeze(0)
    assert torch.equal(sy.apply(a, tabs["action"][0]), su.perm_action(a)) and torch.equal(sy.apply(a, tabs["action"][1]), su.perm_action(su.perm_action(a)))
    x = torch.zeros(1, 32 + A)
    x[0, 0], x[0, 1], x[0, 2] = -0.0, float("inf"), float("nan")
    y = sy.apply(x, tabs["obs"][0])
    assert math.copysign(1.0, float(y[0, 3])) == -1.0 and float(y[0, 3]) == 0.0 and float(y[0, 4]) == float("inf") and math.isnan(float(y[0, 5]))
    assert bool(torch.isfinite(torch.cat([y[0, :3], y[0, 6:]])).all())


def test_the_action_width_is_refused_by_name():
    with pytest.raises(ValueError, match="action width 12"):
        sy.trifinger_symmetry(12, True)


# ---- equivariance against the step ---------------------------------------------------------------------------------------------------------
def test_the_step_is_equivariant_on_the_oracle(oracle):
    tabs = sy.trifinger_symmetry(9, True)
    obs, states, rew, ok = su.scenario(oracle, "cpu")
    assert int(ok.sum()) >= su.HALF // 4, int(ok.sum())
    err = su.errors(obs, states, rew, ok, tabs)
    print("equivariance on the oracle:", int(ok.sum()), "pairs", err)
    for key, bound in su.BOUNDS.items():
        assert err[key] <= bound, (key, err[key], bound)
    # the turn taken the other way is not a symmetry
    obs, states, rew, ok = su.scenario(oracle, "cpu", sense=+1.0)
    assert int(ok.sum()) >= su.HALF // 4
    assert su.errors(obs, states, rew, ok, tabs)["obs"] > 0.05


# ---- the trainer on the oracle env -----------------------------------------------------------------------------------------------------------
T, N = 4, 32


def trainer(oracle, n=N, domain_randomization=None, **kw):
    from leibnizgym_amd.config import gym_config
    from leibnizgym_amd.envs import TrifingerEnv
    from leibnizgym_amd.utils.rlg_train import RlGamesGpuEnvAdapter
    from leibnizgym_amd.wrappers import VecTaskPython
    cfg = gym_config("trifinger_difficulty_4")
    cfg.update(num_instances=n, seed=1, physics_engine="physx", asymmetric_obs=True, episode_length=6)
    if domain_randomization is not None:
        cfg["domain_randomization"] = domain_randomization
    env = TrifingerEnv(config=cfg, device="cpu", verbose=False, lib=oracle)
    ad = RlGamesGpuEnvAdapter("rlgpu", n, env=VecTaskPython(env, rl_device="cpu"))
    return PPOTrainer(ad, 41, 113, 9, PPOConfig(horizon=T, minibatches=2, mini_epochs=2, **kw), device="cpu"), env


def test_the_key():
    assert PPOConfig().symmetry_augmentation is False and PPOConfig.from_rlg(RLG_ASYMM, num_envs=64).symmetry_augmentation is False
    assert "symmetry_augmentation" not in RLG_ASYMM["params"]["config"]     # the project's own key: the default tree does not change
    tree = copy.deepcopy(RLG_ASYMM)
    tree["params"]["config"]["symmetry_augmentation"] = True
    assert PPOConfig.from_rlg(tree, num_envs=64).symmetry_augmentation is True


@pytest.mark.parametrize("keys", [{}, dict(episode_ends=True, clip_value_central=True)], ids=["plain", "ends+vclip"])
def test_minibatch_gradients_are_the_mean_over_three_transformed_minibatches(oracle, keys):
    """float64 throughout: the trainer's own torch step with the key on, against the mean of the gradients of the minibatch, its image under G and its
    image under G^2, each through the objective of tests/minibatch_step_util.py; the KL reported is that of the untransformed minibatch alone"""
    B, rows = 64, 96
    tr, _ = trainer(oracle, symmetry_augmentation=True, **keys)
    assert tr.sym is not None and "packed" not in tr.sym
    tr.net.double()
    g = torch.Generator().manual_seed(5)
    r = lambda *s: torch.randn(*s, generator=g, dtype=torch.float64)      # noqa: E731
    with torch.no_grad():
        tr.net.log_std.copy_(0.3 * r(9) - 0.5)
        tr.net.actor[-1].weight.mul_(20.0)                                  # an asymmetric policy with a spread: the images' gradients differ
    d = dict(obs=r(rows, 41) * 0.5, states=r(rows, 113) * 0.5, act=r(rows, 9) * 0.5, old_nlp=r(rows) * 0.1 + 9.0, adv=r(rows) + 0.5, ret=r(rows),
             old_mu=r(rows, 9) * 0.3, old_v=r(rows) * 0.2)
    w = (torch.rand(rows, generator=g, dtype=torch.float64) > 0.2).double()
    if tr.ends:
        d["w"] = w
    idx = torch.randperm(rows, generator=g)[:B]
    acc = {k: torch.zeros((), dtype=torch.float64) for k in ("loss", "a_loss", "c_loss", "kl")}
    tr._mb_backward(d, idx, acc)
    got = {n: p.grad.clone() for n, p in tr.net.named_parameters()}
    assert tuple(tr._sym_mu.shape) == (3 * B, 9)

    tabs = tr.sym
    ref = copy.deepcopy(tr.net)
    want, stats = {n: torch.zeros_like(p) for n, p in ref.named_parameters()}, []
    for k in range(3):
        img = (lambda x, key: x) if k == 0 else (lambda x, key: sy.apply(x, tabs[key][k - 1]))       # noqa: E731
        dk = dict(d, obs=img(d["obs"], "obs"), states=img(d["states"], "states"), act=img(d["act"], "action"), old_mu=img(d["old_mu"], "action"))
        for p in ref.parameters():
            p.grad = None
        if tr.ends:                                                         # every per-sample term times w_i, the divisor stays B
            st = weighted_objective(ref, tr.cfg, tr.clip_v, dk, idx)
        else:
            st, _ = objective(ref, tr.cfg, tr.clip_v, dk, idx)
        st[0].backward()
        stats.append([float(x.detach()) for x in st])
        for n, p in ref.named_parameters():
            want[n] += p.grad / 3.0
    for n in want:
        assert float(want[n].abs().max()) > 0 and torch.allclose(got[n], want[n], rtol=1e-5, atol=0.0), (n, float((got[n] - want[n]).abs().max()))
    mean = [sum(s[q] for s in stats) / 3.0 for q in range(3)]
    assert [float(acc[k]) for k in ("loss", "a_loss", "c_loss")] == pytest.approx(mean, rel=1e-9)
    assert float(acc["kl"]) == pytest.approx(stats[0][3], rel=1e-12)
    assert abs(stats[1][3] - stats[0][3]) > 1e-3 * stats[0][3]              # ... which the images' KL is not
    gap = float(tr._symmetry_gap())
    mu = tr._sym_mu
    by_hand = 0.5 * float((su.perm_action(su.perm_action(mu[B:2 * B])) - mu[:B]).abs().mean() + (su.perm_action(mu[2 * B:]) - mu[:B]).abs().mean())
    assert gap == pytest.approx(by_hand, rel=1e-12) and gap > 0.01


def weighted_objective(net, cfg, clip_v, d, idx):
    """minibatch_step_util.objective with a weight per sample (`episode_ends`): every per-sample term times w_i, the divisor stays B"""
    e, w = cfg.e_clip, d["w"][idx]
    obs = d["obs"][idx]
    mu, ls = net.dist(obs)
    v = net.value(obs, d["states"][idx])
    ratio = (d["old_nlp"][idx] - ppo.neglogp(d["act"][idx], mu, ls)).exp()
    adv, ret = d["adv"][idx], d["ret"][idx]
    a_loss = (w * torch.maximum(-adv * ratio, -adv * ratio.clamp(1 - e, 1 + e))).mean()
    c_loss = (w * (ppo.clipped_value_loss(v, ret, d["old_v"][idx], e) if clip_v else (v - ret) ** 2)).mean()
    b_loss = (w * ((mu - 1.1).clamp(min=0) ** 2 + (-1.1 - mu).clamp(min=0) ** 2).sum(-1)).mean()
    ent = (net.log_std + 0.5 + 0.5 * math.log(2 * math.pi)).sum()
    loss = a_loss + (1.0 if net.central else 0.5 * cfg.critic_coef) * c_loss - cfg.entropy_coef * ent + cfg.bounds_loss_coef * b_loss
    kl = (w * (0.5 * ((mu - d["old_mu"][idx]) / net.log_std.exp()) ** 2).sum(-1)).mean()
    return loss, a_loss, c_loss, kl


def test_trainer_trains_with_the_key_on(oracle, tmp_path):
    tr, _ = trainer(oracle, symmetry_augmentation=True, normalize_input=True, normalize_input_value=True)
    before = [p.detach().clone() for p in tr.net.parameters()]
    stats = tr.train(2)
    assert len(stats) == 2
    for st in stats:
        assert all(math.isfinite(st[k]) for k in ("loss", "a_loss", "c_loss", "kl", "mean_reward", "symmetry_gap")) and st["symmetry_gap"] >= 0.0
    assert all(bool(torch.isfinite(p).all()) and not torch.equal(a, p) for a, p in zip(before, tr.net.parameters()))
    assert tr.frames == 2 * T * N
    # the networks' shapes do not change: a checkpoint moves between on and off
    path = tr.save(str(tmp_path / "ck.pth"))
    off, _ = trainer(oracle, normalize_input=True, normalize_input_value=True)
    off.restore(path)
    assert all(torch.equal(a, b) for a, b in zip(tr.net.parameters(), off.net.parameters()))
    assert "symmetry_gap" not in off.train(1)[0]


def test_refusals_name_the_key(oracle):
    with pytest.raises(ValueError, match="no native engine"):
        PPOTrainer(StubEnv(41, 113, "cpu"), 41, 113, 9, PPOConfig(symmetry_augmentation=True), device="cpu")
    tr, env = trainer(oracle)
    for od, sd, A in ((40, 112, 9), (41, 100, 9), (44, 116, 12)):
        with pytest.raises(ValueError, match="symmetry_augmentation") as e:
            PPOTrainer(tr.env, od, sd, A, PPOConfig(symmetry_augmentation=True), device="cpu")
        assert f"obs {od}" in str(e.value) and f"states {sd}" in str(e.value)
    assert PPOTrainer(tr.env, 41, 0, 9, PPOConfig(symmetry_augmentation=True), device="cpu").sym["states"] is None      # no central value network: fine
    # a shifted robot base or stage: the scene is not invariant; any other randomisation is
    dr = {"activate": True, "stage_position": (0.01, 0.0)}
    with pytest.raises(ValueError, match="stage_position"):
        trainer(oracle, domain_randomization=dr, symmetry_augmentation=True)
    with pytest.raises(ValueError, match="robot_base_position"):
        trainer(oracle, domain_randomization={"activate": True, "robot_base_position": (0.0, 0.0, 0.002)}, symmetry_augmentation=True)
    assert trainer(oracle, domain_randomization={"activate": True, "cube_mass": (0.8, 1.2)}, symmetry_augmentation=True)[0].sym is not None
    assert trainer(oracle, domain_randomization=dr)[0].sym is None          # ... and only with the key on


def test_off_is_off(oracle, monkeypatch):
    def boom(*a, **k):
        raise AssertionError("a function of the symmetry path ran with the key off")
    for name in ("trifinger_symmetry", "apply", "pack", "tables_to"):
        monkeypatch.setattr(sy, name, boom)
    monkeypatch.setattr(PPOTrainer, "_symmetry_tables", boom)
    monkeypatch.setattr(PPOTrainer, "_sym_minibatch", boom)
    tr, _ = trainer(oracle)
    assert tr.sym is None and tr._sym_mu is None
    stats = tr.train(1)[0]
    assert "symmetry_gap" not in stats and math.isfinite(stats["loss"]) and tr._sym_mu is None
    assert tr.state_dict()["config"]["symmetry_augmentation"] is False
