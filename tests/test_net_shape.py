"""The network-shape keys of the agent tree on the in-repo PPO (CPU): `network.mlp.activation`, `network.mlp.d2rl`, `truncate_grads`, `lr_schedule`, and the
keys that are refused by name (`fixed_sigma: False`, `mu_activation` / `sigma_activation`).  The kernels' side is tests/test_net_shape_gpu.py."""
import copy

import pytest
import torch
import torch.nn as nn

from leibnizgym_amd.config import RLG_ASYMM, gym_config
from leibnizgym_amd.envs import TrifingerEnv
from leibnizgym_amd.ppo import ActorCritic, D2RLMLP, FusedMLP, PPOConfig, PPOTrainer, mlp
from leibnizgym_amd.utils.rlg_train import RlGamesGpuEnvAdapter
from leibnizgym_amd.wrappers import VecTaskPython


def tree(**edits):
    """the default agent tree with `a/b/c=value` edits"""
    t = copy.deepcopy(RLG_ASYMM)
    for path, v in edits.items():
        node = t
        keys = path.split("/")
        for k in keys[:-1]:
            node = node[k]
        node[keys[-1]] = v
    return t


A_MLP, V_MLP = "params/network/mlp/", "params/config/central_value_config/network/mlp/"


def make(oracle, n=32):
    cfg = gym_config("trifinger_difficulty_4")
    cfg.update(num_instances=n, seed=1, physics_engine="physx", asymmetric_obs=True, episode_length=20)
    env = TrifingerEnv(config=cfg, device="cpu", verbose=False, lib=oracle)
    return RlGamesGpuEnvAdapter("rlgpu", n, env=VecTaskPython(env, rl_device="cpu"))


def test_the_network_follows_the_tree():
    c = PPOConfig.from_rlg(tree())
    assert (c.activation, c.value_activation, c.d2rl, c.value_d2rl) == ("elu", "elu", False, False)
    assert (c.truncate_grads, c.value_truncate_grads, c.lr_schedule) == (True, True, "adaptive")
    net = ActorCritic(41, 113, 9, c.units, c)
    assert all(isinstance(m, nn.ELU) for m in list(net.actor)[1::2] + list(net.critic)[1::2]) and type(net.actor) is FusedMLP

    c = PPOConfig.from_rlg(tree(**{A_MLP + "activation": "tanh", V_MLP + "activation": "selu", A_MLP + "d2rl": True, V_MLP + "d2rl": True,
                                   "params/config/truncate_grads": False, "params/config/lr_schedule": "linear"}))
    assert (c.activation, c.value_activation, c.d2rl, c.value_d2rl) == ("tanh", "selu", True, True)
    assert (c.truncate_grads, c.value_truncate_grads, c.lr_schedule) == (False, True, "linear")
    net = ActorCritic(41, 113, 9, c.units, c)
    assert all(isinstance(m, nn.Tanh) for m in list(net.actor)[1::2]) and all(isinstance(m, nn.SELU) for m in list(net.critic)[1::2])
    assert len(net.actor) == 7 and isinstance(net.actor[-1], nn.Linear)              # no activation behind the output layer
    assert net.actor[2].in_features == 400 + 41 and net.critic[2].in_features == 400 + 113
    assert net.actor[4].in_features == 200 + 41 and net.critic[4].in_features == 200 + 113
    assert net.actor[-1].in_features == 100 and net.critic[-1].in_features == 100
    assert [l[2] for l in net.actor.layer_list()] == [3, 3, 3, 0] and [l[2] for l in net.critic.layer_list()] == [5, 5, 5, 0]
    assert net.actor.layer_list().d2rl and net.critic.layer_list().d2rl
    # None, in both of YAML's spellings, is the identity
    for none in (None, "None"):
        c = PPOConfig.from_rlg(tree(**{A_MLP + "activation": none}))
        assert c.activation == "None" and isinstance(ActorCritic(41, 113, 9, c.units, c).actor[1], nn.Identity)
    # without a central value network the critic takes the actor's keys
    t = tree(**{A_MLP + "activation": "relu", A_MLP + "d2rl": True, "params/config/truncate_grads": False})
    del t["params"]["config"]["central_value_config"]
    c = PPOConfig.from_rlg(t)
    assert (c.value_activation, c.value_d2rl, c.value_truncate_grads) == ("relu", True, False)
    net = ActorCritic(41, 0, 9, c.units, c)
    assert isinstance(net.critic[1], nn.ReLU) and net.critic[2].in_features == 400 + 41


@pytest.mark.parametrize("units", [[24, 16, 8], [12]])
@pytest.mark.parametrize("act", ["tanh", "softplus"])
def test_d2rl_module_is_the_cat_formula(units, act):
    torch.manual_seed(3)
    net = mlp(7, units, 3, activation=act, d2rl=True).double()
    assert isinstance(net, D2RLMLP)
    x = torch.randn(5, 7, dtype=torch.float64)
    f = {"tanh": torch.tanh, "softplus": nn.functional.softplus}[act]
    lin = [m for m in net if isinstance(m, nn.Linear)]
    h = f(x @ lin[0].weight.t() + lin[0].bias)
    for l in lin[1:-1]:
        assert l.weight.shape[1] == h.shape[1] + 7
        h = f(torch.cat([h, x], dim=1) @ l.weight.t() + l.bias)
    assert lin[-1].weight.shape[1] == units[-1]
    assert torch.equal(net(x), h @ lin[-1].weight.t() + lin[-1].bias)
    (g,) = torch.autograd.grad(net(x).sum(), lin[0].weight)
    assert torch.isfinite(g).all()


def test_without_d2rl_the_state_dict_is_the_old_one():
    """keys and shapes of the plain Linear / ELU Sequential a checkpoint of before holds; such a checkpoint loads"""
    old_actor = nn.Sequential(nn.Linear(41, 400), nn.ELU(), nn.Linear(400, 200), nn.ELU(), nn.Linear(200, 100), nn.ELU(), nn.Linear(100, 9))
    old_critic = nn.Sequential(nn.Linear(113, 400), nn.ELU(), nn.Linear(400, 200), nn.ELU(), nn.Linear(200, 100), nn.ELU(), nn.Linear(100, 1))
    old = {"log_std": torch.full((9,), 0.25)}
    old.update({"actor." + k: v for k, v in old_actor.state_dict().items()})
    old.update({"critic." + k: v for k, v in old_critic.state_dict().items()})
    for cfg in (None, PPOConfig(), PPOConfig(activation="tanh", value_activation="None")):
        net = ActorCritic(41, 113, 9, [400, 200, 100], cfg)
        assert sorted(net.state_dict()) == sorted(old) and all(net.state_dict()[k].shape == v.shape for k, v in old.items())
        net.load_state_dict(old)
        assert torch.equal(net.actor[2].weight, old_actor[2].weight) and torch.equal(net.log_std, old["log_std"])


def test_truncate_grads_false_is_plain_adam(oracle):
    def run(trunc, scale):
        tr = PPOTrainer(make(oracle), 41, 113, 9, PPOConfig(horizon=4, minibatches=1, mini_epochs=1, truncate_grads=trunc, value_truncate_grads=trunc), device="cpu")
        torch.manual_seed(5)
        grads = [torch.randn_like(p) * scale for p in tr.net.parameters()]
        ref = copy.deepcopy(tr.net)
        opt = torch.optim.Adam([{"params": list(ref.actor.parameters()) + [ref.log_std], "lr": tr.cfg.lr}, {"params": list(ref.critic.parameters()), "lr": tr.cfg.lr_value}],
                               eps=1e-8)
        for p, q, g in zip(tr.net.parameters(), ref.parameters(), grads):
            p.grad, q.grad = g.clone(), g.clone()
        tr._mb_apply()
        opt.step()
        return all(torch.equal(p, q) for p, q in zip(tr.net.parameters(), ref.parameters()))
    # a huge gradient (norm ~ 5e5, truncated by a factor ~ 2e-6): Adam's first step is lr g / (|g| + eps), so truncation shows through eps = 1e-8 against
    # elements ~ 1e-3 (a relative 1e-5, far above fp32 rounding) - the control below sees it, the untruncated step must not
    assert run(False, 1e3)                  # no truncation: plain Adam, bit for bit
    assert not run(True, 1e3)               # the control: with truncation the same step differs


def test_lr_schedules(oracle):
    tr = PPOTrainer(make(oracle), 41, 113, 9, PPOConfig(horizon=4, minibatches=2, mini_epochs=2, lr_schedule="identity"), device="cpu")
    stats = tr.train(3)
    assert [s["lr"] for s in stats] == [tr.cfg.lr] * 3 and tr.opt.param_groups[0]["lr"] == tr.cfg.lr and tr.opt.param_groups[1]["lr"] == tr.cfg.lr_value
    assert all(s["kl"] >= 0.0 for s in stats)                                        # the statistic is still computed and logged
    tr = PPOTrainer(make(oracle), 41, 113, 9, PPOConfig(horizon=4, minibatches=2, mini_epochs=1, lr_schedule="linear", max_epochs=4), device="cpu")
    f = lambda e: 1e-6 + (3e-4 - 1e-6) * max(0, 4 - e) / 4  # noqa: E731
    stats = tr.train(2)
    assert [s["lr"] for s in stats] == [f(0), f(1)] and f(0) == 3e-4
    assert tr.opt.param_groups[0]["lr"] == f(1) and tr.opt.param_groups[1]["lr"] == tr.cfg.lr_value      # the central value network's rate stays constant
    tr.epoch = 4
    assert tr.update(tr.rollout())["lr"] == f(4) == 1e-6
    c = PPOConfig.from_rlg(tree(**{"params/config/lr_schedule": "None"}))
    assert c.lr_schedule == "identity"


def test_unknown_and_unbuilt_keys_are_refused_by_name(oracle):
    for edits, key in (({A_MLP + "activation": "mish"}, "params.network.mlp.activation"),
                       ({V_MLP + "activation": "mish"}, "central_value_config.network.mlp.activation"),
                       ({"params/config/lr_schedule": "cosine"}, "lr_schedule"),
                       ({"params/network/space/continuous/fixed_sigma": False}, "fixed_sigma"),
                       ({"params/network/space/continuous/mu_activation": "tanh"}, "mu_activation"),
                       ({"params/network/space/continuous/sigma_activation": "tanh"}, "sigma_activation")):
        with pytest.raises(ValueError, match=key.replace(".", r"\.")):
            PPOConfig.from_rlg(tree(**edits))
    with pytest.raises(ValueError, match="activation") as e:
        ActorCritic(41, 113, 9, [8], PPOConfig(activation="mish"))
    assert "relu" in str(e.value) and "softplus" in str(e.value)                      # the accepted values are listed
    with pytest.raises(ValueError, match="lr_schedule"):
        PPOTrainer(make(oracle), 41, 113, 9, PPOConfig(lr_schedule="cosine"), device="cpu")


def test_swish_and_d2rl_train_on_the_cpu_path(oracle):
    tr = PPOTrainer(make(oracle), 41, 113, 9, PPOConfig(horizon=8, minibatches=4, mini_epochs=2, activation="swish", value_activation="gelu", d2rl=True,
                                                        value_d2rl=True), device="cpu")
    assert isinstance(tr.net.actor[1], nn.SiLU) and isinstance(tr.net.critic[1], nn.GELU)
    before = [p.detach().clone() for p in tr.net.parameters()]
    stats = tr.train(2)
    assert len(stats) == 2 and all(torch.isfinite(torch.tensor([s["loss"], s["kl"]])).all() for s in stats)
    assert any(not torch.equal(a, b) for a, b in zip(before, tr.net.parameters()))


def test_an_override_of_the_tree_reaches_the_trainer(oracle):
    """what scripts/rlg_hydra.py does with `rlg.params.network.mlp.activation=tanh`: the tree goes through PPOConfig.from_rlg into the trainer"""
    c = PPOConfig.from_rlg(tree(**{A_MLP + "activation": "tanh", V_MLP + "d2rl": True}), num_envs=32, horizon=4)
    tr = PPOTrainer(make(oracle), 41, 113, 9, c, device="cpu")
    assert isinstance(tr.net.actor[1], nn.Tanh) and type(tr.net.actor) is FusedMLP and isinstance(tr.net.critic, D2RLMLP) and isinstance(tr.net.critic[1], nn.ELU)
    assert tr.state_dict()["config"]["activation"] == "tanh" and tr.state_dict()["config"]["value_d2rl"] is True


def test_the_tanh_formula_of_the_walk_is_within_two_ulp():
    """the formula of csrc/ppo_mlp_walk.hip:tanh_fast in float32 torch (exp and quotient correctly rounded; the hardware's v_exp_f32 / v_rcp_f32 add 1 ulp
    each) against float64 tanh: relative error <= 2.5e-7 (2 ulp = 2.4e-7) over the polynomial range, the switch at 0.625 and the saturated range; +-1, finite"""
    v = torch.cat([torch.linspace(-40, 40, 400001), torch.linspace(-0.7, 0.7, 200001), torch.tensor([1e-6, -1e-6, 1e-20, 0.625, -0.625, 100.0, -100.0])]).float()
    a, z = v.abs(), v * v
    big = torch.copysign(1 - 2 / (torch.exp2((2 * a) * 1.44269504088896340736) + 1), v)
    p = ((((-5.70498872745e-3 * z + 2.06390887954e-2) * z - 5.37397155531e-2) * z + 1.33314422036e-1) * z - 3.33332819422e-1) * z * v + v
    y = torch.where(a < 0.625, p, big)
    ref = torch.tanh(v.double())
    nz = v != 0
    assert torch.isfinite(y).all() and float(y.abs().max()) <= 1.0
    assert float(((y.double() - ref).abs() / ref.abs())[nz].max()) <= 2.5e-7
