"""`episode_ends` / `value_bootstrap` of the in-repo PPO on the CPU (leibnizgym_amd/ppo.py: the module docstring has the definitions): the keys, the torch
specification `gae_with_ends` against hand-computed float64 values and against the backward loop the trainer runs with the mode off, and the trainer on the
oracle env (injected through `lib=`) with the mode on and off.  The kernels' side of the same definitions is tests/test_episode_ends_gpu.py."""
import copy
import math

import pytest
import torch

import leibnizgym_amd.ppo as ppo
from leibnizgym_amd.config import RLG_ASYMM
from leibnizgym_amd.ppo import InputNorm, PPOConfig, PPOTrainer, denormalize_value, gae_with_ends, masked_advantage_norm

GAMMA, TAU = 0.99, 0.95
EP_LEN, T, N = 5, 8, 3


# ---- the keys --------------------------------------------------------------------------------------------------------------------------------
def test_from_rlg_reads_both_keys():
    c = PPOConfig.from_rlg(RLG_ASYMM, num_envs=64)
    assert (c.episode_ends, c.value_bootstrap) == (False, False) and (PPOConfig().episode_ends, PPOConfig().value_bootstrap) == (False, False)
    assert "episode_ends" not in RLG_ASYMM["params"]["config"] and "value_bootstrap" not in RLG_ASYMM["params"]["config"]     # the default tree does not change
    tree = copy.deepcopy(RLG_ASYMM)
    tree["params"]["config"]["episode_ends"] = True
    c = PPOConfig.from_rlg(tree, num_envs=64)
    assert (c.episode_ends, c.value_bootstrap) == (True, False)
    tree["params"]["config"]["value_bootstrap"] = True
    c = PPOConfig.from_rlg(tree, num_envs=64)
    assert (c.episode_ends, c.value_bootstrap) == (True, True)
    tree["params"]["config"]["episode_ends"] = False
    with pytest.raises(ValueError) as e:
        PPOConfig.from_rlg(tree, num_envs=64)
    assert "value_bootstrap" in str(e.value) and "episode_ends" in str(e.value)
    with pytest.raises(ValueError, match="episode_ends"):
        PPOConfig(value_bootstrap=True)


# ---- gae_with_ends against hand-computed float64 values ------------------------------------------------------------------------------------
VAL = [0.5, -1.25, 2.0, 0.75, -3.0]            # val[0 .. 4]; rew = 1 throughout: every case below differs from every other
G, GT = GAMMA, GAMMA * TAU


def run(end, tout, last_end, boot):
    f = lambda x: torch.tensor(x, dtype=torch.float32).unsqueeze(1)       # noqa: E731
    adv, ret, w = gae_with_ends(torch.ones(4, 1), f(end), f(tout), f(VAL), torch.tensor([float(last_end)]), GAMMA, TAU, boot)
    assert adv.dtype == ret.dtype == w.dtype == torch.float32 and adv.shape == ret.shape == w.shape == (4, 1)
    return adv[:, 0].tolist(), ret[:, 0].tolist(), w[:, 0].tolist()


def close(got, want):
    # float32 against float64: values of magnitude < 8, at most ten roundings of 2^-24 relative each
    assert got == pytest.approx(want, abs=8 * 10 * 2.0 ** -24), (got, want)


def test_gae_with_ends_by_hand():
    v = VAL
    d = [1 + G * v[t + 1] - v[t] for t in range(4)]                      # the deltas that bootstrap
    # no end anywhere: plain GAE
    l3 = d[3]; l2 = d[2] + GT * l3; l1 = d[1] + GT * l2; l0 = d[0] + GT * l1
    adv, ret, w = run([0, 0, 0, 0], [0, 0, 0, 0], 0, True)
    close(adv, [l0, l1, l2, l3]); close(ret, [l0 + v[0], l1 + v[1], l2 + v[2], l3 + v[3]]); assert w == [1, 1, 1, 1]
    plain = (adv, ret, w)
    # an end at t = 1 as a time-out, with bootstrap: delta_1 holds gamma val[2], the trace is cut at t = 1, t = 2 is stale
    l1 = d[1]; l0 = d[0] + GT * l1
    adv, ret, w = run([0, 1, 0, 0], [0, 1, 0, 0], 0, True)
    close(adv, [l0, l1, 0.0, l3]); close(ret, [l0 + v[0], l1 + v[1], v[2], l3 + v[3]])
    assert w == [1, 1, 0, 1] and adv[2] == 0.0 and ret[2] == v[2]
    boot = adv
    # the same end without bootstrap: delta_1 does not hold it
    l1 = 1 - v[1]; l0 = d[0] + GT * l1
    for end, tout, b in (([0, 1, 0, 0], [0, 1, 0, 0], False),            # a time-out, bootstrap off
                         ([0, 1, 0, 0], [0, 0, 0, 0], True),             # a termination never bootstraps
                         ([0, 1, 0, 0], [0, 0, 0, 0], False)):
        adv, ret, w = run(end, tout, 0, b)
        close(adv, [l0, l1, 0.0, l3]); close(ret, [l0 + v[0], l1 + v[1], v[2], l3 + v[3]]); assert w == [1, 1, 0, 1]
        assert abs(adv[1] - boot[1]) > 1.0 and abs(adv[0] - boot[0]) > 1.0                          # the cases differ
    # last_end = 1 makes t = 0 stale, and nothing else moves
    adv, ret, w = run([0, 0, 0, 0], [0, 0, 0, 0], 1, True)
    assert w == [0, 1, 1, 1] and adv[0] == 0.0 and ret[0] == v[0] and adv[1:] == plain[0][1:] and ret[1:] == plain[1][1:]
    # an end at t = T - 1 (a time-out that bootstraps) changes nothing in this rollout: the stale sample is the next rollout's first
    assert run([0, 0, 0, 1], [0, 0, 0, 1], 0, True) == plain
    # ... and as a terminal it takes gamma val[4] out of delta_3
    l3 = 1 - v[3]; l2 = d[2] + GT * l3; l1 = d[1] + GT * l2; l0 = d[0] + GT * l1
    adv, ret, w = run([0, 0, 0, 1], [0, 0, 0, 1], 0, False)
    close(adv, [l0, l1, l2, l3]); assert w == [1, 1, 1, 1]


def test_masked_advantage_norm():
    g = torch.Generator().manual_seed(3)
    adv, w = torch.randn(200, generator=g) * 3 + 1, (torch.rand(200, generator=g) > 0.25).float()
    adv = adv * w
    got = masked_advantage_norm(adv, w)
    live = adv[w == 1]
    assert torch.allclose(got[w == 1], (live - live.mean()) / (live.std() + 1e-8), rtol=1e-5, atol=1e-6) and bool((got[w == 0] == 0).all())
    one = torch.ones(200)
    assert torch.allclose(masked_advantage_norm(adv, one), (adv - adv.mean()) / (adv.std() + 1e-8), rtol=1e-5, atol=1e-6)


# ---- bit identity with the loop the trainer runs with the mode off ---------------------------------------------------------------------------
def parent_loop(rew, done, val, gamma, tau):
    """PPOTrainer.rollout's torch form with the mode off, expression for expression"""
    Tn, n = rew.shape
    adv, last = torch.zeros(Tn, n), torch.zeros(n)
    for t in reversed(range(Tn)):
        nd = 1.0 - done[t]
        delta = rew[t] + gamma * val[t + 1] * nd - val[t]
        last = delta + gamma * tau * nd * last
        adv[t] = last
    return adv, adv + val[:Tn]


@pytest.mark.parametrize("vnorm", [False, True], ids=["plain", "normalize_value"])
def test_without_ends_the_bits_of_the_existing_loop(vnorm):
    g = torch.Generator().manual_seed(5)
    Tn, n = 32, 67
    rew, y = torch.randn(Tn, n, generator=g), torch.randn(Tn + 1, n, generator=g) * 3
    zero = torch.zeros(Tn, n)
    if vnorm:
        rec = InputNorm(1, "cpu")
        rec.state.copy_(torch.tensor([10.0, 0.5, 4.0 * 10], dtype=torch.float64))
        rec.publish()
        val = denormalize_value(y, rec)
    else:
        val = y
    want_adv, want_ret = parent_loop(rew, zero, val, GAMMA, TAU)
    for boot in (False, True):
        for tout in (zero, torch.ones(Tn, n)):                            # a time-out flag without an end is no end
            adv, ret, w = gae_with_ends(rew, zero, tout, val, torch.zeros(n), GAMMA, TAU, boot)
            assert torch.equal(adv, want_adv) and torch.equal(ret, want_ret) and bool((w == 1).all())
    # and `done` of the mode off is `end` without a stale sample: the same cut of the trace, the same missing bootstrap
    done = (torch.rand(Tn, n, generator=g) < 0.2).float()
    adv, ret, w = gae_with_ends(rew, done, zero, val, torch.zeros(n), GAMMA, TAU, False)
    a0, r0 = parent_loop(rew, done, val, GAMMA, TAU)
    assert torch.equal(adv, a0 * w) and torch.equal(w[1:], 1.0 - done[:-1]) and torch.equal(ret, a0 * w + val[:Tn])


# ---- the trainer on the oracle env -----------------------------------------------------------------------------------------------------------
def trainer(oracle, n=N, episode_length=EP_LEN, **kw):
    from leibnizgym_amd.config import gym_config
    from leibnizgym_amd.envs import TrifingerEnv
    from leibnizgym_amd.utils.rlg_train import RlGamesGpuEnvAdapter
    from leibnizgym_amd.wrappers import VecTaskPython
    cfg = gym_config("trifinger_difficulty_4")
    cfg.update(num_instances=n, seed=1, physics_engine="physx", asymmetric_obs=True, episode_length=episode_length)
    env = TrifingerEnv(config=cfg, device="cpu", verbose=False, lib=oracle)
    ad = RlGamesGpuEnvAdapter("rlgpu", n, env=VecTaskPython(env, rl_device="cpu"))
    return PPOTrainer(ad, 41, 113, 9, PPOConfig(horizon=T, minibatches=4, mini_epochs=2, **kw), device="cpu"), env


def record_steps(tr, eng):
    """what the engine's buffers hold after every step of the trainer's env, and what the step returned"""
    seen, step = [], tr.env.step

    def wrapped(a):
        out = step(a)
        seen.append(dict(reset=eng.reset_buf.clone(), steps=eng.steps.clone(), r=out[1].clone(), d=out[2].clone()))
        return out
    tr.env.step = wrapped
    return seen


@pytest.mark.parametrize("boot", [False, True], ids=["terminal", "value_bootstrap"])
def test_trainer_with_episode_ends(oracle, boot):
    tr, env = trainer(oracle, episode_ends=True, value_bootstrap=boot)
    eng = env._engine
    assert tr.ends and tr.ends_engine is eng and tr.ends_ep_len == EP_LEN and torch.equal(tr.last_end, torch.zeros(N))
    seen = record_steps(tr, eng)
    bufs = []
    for k in range(6):
        last_end = tr.last_end.clone()
        buf = tr.rollout()
        rec = seen[k * T:(k + 1) * T]
        assert len(rec) == T and "done" not in buf
        end = torch.stack([(r["reset"] != 0).float() for r in rec])
        tout = torch.stack([(r["steps"] >= EP_LEN).float() for r in rec])
        assert torch.equal(buf["end"], end) and torch.equal(buf["tout"], tout)
        assert torch.equal(buf["rew"], torch.stack([r["r"] * tr.cfg.reward_scale for r in rec]))
        assert torch.equal(buf["w"][0], 1.0 - last_end) and torch.equal(buf["w"][1:], 1.0 - end[:-1]) and torch.equal(tr.last_end, end[T - 1])
        adv, ret, w = gae_with_ends(buf["rew"], buf["end"], buf["tout"], buf["val"], last_end, GAMMA, TAU, boot)
        assert torch.equal(buf["adv"], adv) and torch.equal(buf["ret"], ret) and torch.equal(buf["w"], w)
        assert bool((buf["adv"][buf["w"] == 0] == 0).all()) and torch.equal(buf["ret"][buf["w"] == 0], buf["val"][:T][buf["w"] == 0])
        bufs.append(buf)
    # by construction: a time limit of 5 steps in rollouts of 8 - every env ends in every rollout, each end is a time-out, the public `done` never fires
    assert all(bool((b["end"].sum(0) >= 1).all()) for b in bufs) and all(torch.equal(b["end"], b["tout"]) for b in bufs)
    assert not any(bool(r["d"].any()) for r in seen)
    want = torch.zeros(6 * T, N)
    want[EP_LEN - 1::EP_LEN] = 1.0                                        # global steps 5, 10, 15, ...
    assert torch.equal(torch.cat([b["end"] for b in bufs]), want)
    # w[0] of the second rollout is 1 - end[T - 1] of the first; global step 40 is the last step of the fifth rollout: the sixth starts stale
    assert torch.equal(bufs[1]["w"][0], 1.0 - bufs[0]["end"][T - 1])
    assert bool((bufs[4]["end"][T - 1] == 1).all()) and bool((bufs[5]["w"][0] == 0).all()) and bool((bufs[5]["adv"][0] == 0).all())

    # a minibatch made of stale samples only: every gradient is exactly zero (the entropy term is batch-independent and the only thing left)
    buf = bufs[5]
    flat = lambda x: x.reshape(T * N, *x.shape[2:])                       # noqa: E731
    d = dict(obs=flat(buf["obs"]), states=flat(buf["states"]), act=flat(buf["act"]), old_nlp=flat(buf["nlp"]), ret=flat(buf["ret"]),
             adv=masked_advantage_norm(flat(buf["adv"]), flat(buf["w"])), old_mu=flat(buf["mu"]), w=flat(buf["w"]))
    stale = torch.nonzero(d["w"] == 0).squeeze(1)
    assert stale.numel() == 2 * N and bool((d["adv"][stale] == 0).all())
    tr._mb_backward(d, stale, tr._new_acc("cpu"))
    assert all(p.grad is not None and bool((p.grad == 0).all()) for p in tr.net.parameters())
    tr.cfg.entropy_coef = 0.01
    acc = tr._new_acc("cpu")
    tr._mb_backward(d, stale, acc)
    tr.cfg.entropy_coef = 0.0
    for name, p in tr.net.named_parameters():
        if name == "log_std":
            assert torch.allclose(p.grad, torch.full_like(p.grad, -0.01), rtol=1e-6, atol=0)
        else:
            assert bool((p.grad == 0).all()), name
    ent = float((tr.net.log_std.detach() + 0.5 + 0.5 * math.log(2 * math.pi)).sum())
    assert float(acc["loss"]) == pytest.approx(-0.01 * ent, rel=1e-6) and float(acc["kl"]) == 0.0 and float(acc["a_loss"]) == 0.0 and float(acc["c_loss"]) == 0.0
    live = torch.nonzero(d["w"] == 1).squeeze(1)
    tr._mb_backward(d, live, tr._new_acc("cpu"))
    assert all(float(p.grad.abs().max()) > 0 for p in tr.net.parameters())

    # one update: finite, moves the parameters, counts the ends
    before = [p.detach().clone() for p in tr.net.parameters()]
    stats = tr.update(buf)
    assert all(math.isfinite(stats[k]) for k in ("loss", "a_loss", "c_loss", "kl", "mean_reward"))
    assert stats["episodes_ended"] == int(buf["end"].sum()) == N             # global step 45
    assert all(bool(torch.isfinite(p).all()) for p in tr.net.parameters()) and all(not torch.equal(a, p) for a, p in zip(before, tr.net.parameters()))
    # whenever the trainer resets the env, no sample of the next rollout is stale
    tr.last_end.fill_(1.0)
    tr.evaluate(max_steps=2)
    assert torch.equal(tr.last_end, torch.zeros(N)) and bool((tr.rollout()["w"][0] == 1).all())


def test_trainer_with_every_value_key_and_episode_ends(oracle, tmp_path):
    """normalize_value + clip_value_central with the mode on, on the torch path: ret_n and v_old_n from the masked ret, two epochs finite, restore zeroes last_end"""
    tr, _ = trainer(oracle, episode_ends=True, value_bootstrap=True, normalize_value=True, clip_value_central=True, normalize_input=True)
    vn = tr.value_norm
    buf = tr.rollout()
    adv, ret, w = gae_with_ends(buf["rew"], buf["end"], buf["tout"], buf["val"], torch.zeros(N), GAMMA, TAU, True)
    assert torch.equal(buf["adv"], adv) and torch.equal(buf["ret"], ret)
    assert torch.equal(buf["ret_n"], torch.clamp((ret - vn.mean_f) * vn.inv_std_f, -vn.clip, vn.clip))
    stats = [tr.update(buf)] + tr.train(2)
    assert all(math.isfinite(s[k]) for s in stats for k in ("loss", "a_loss", "c_loss", "kl")) and all(s["episodes_ended"] >= N for s in stats)
    assert float(vn.count) == 3 * T * N                                   # every sample, stale ones as ret = val
    path = tr.save(str(tmp_path / "ck.pth"))
    tr.last_end.fill_(1.0)
    tr.restore(path)
    assert torch.equal(tr.last_end, torch.zeros(N))


def test_no_time_limit_is_still_valid(oracle):
    tr, _ = trainer(oracle, episode_length=0, episode_ends=True, value_bootstrap=True)
    assert tr.ends_ep_len == 0
    buf = tr.rollout()
    assert float(buf["tout"].sum()) == 0 and float(buf["end"].sum()) == 0 and bool((buf["w"] == 1).all())
    assert tr.update(buf)["episodes_ended"] == 0


# ---- the mode off ----------------------------------------------------------------------------------------------------------------------------
def test_off_is_off(oracle, monkeypatch):
    """none of the new functions runs, none of the new buffers exists, and the rollout buffers are the expressions they were"""
    def boom(*a, **k):
        raise AssertionError("a function of the episode-end path ran with its keys off")
    import leibnizgym_amd.evaluate as ev
    monkeypatch.setattr(ppo, "gae_with_ends", boom)
    monkeypatch.setattr(ppo, "masked_advantage_norm", boom)
    monkeypatch.setattr(ev, "engine_of", boom)
    tr, env = trainer(oracle)
    assert not tr.ends and tr.last_end is None and tr.ends_engine is None
    seen = record_steps(tr, env._engine)
    torch.manual_seed(3)
    buf = tr.rollout()
    assert not {"end", "tout", "w"} & set(buf)
    assert torch.equal(buf["rew"], torch.stack([r["r"] * tr.cfg.reward_scale for r in seen]))
    assert torch.equal(buf["done"], torch.stack([r["d"].float() for r in seen]))
    adv, ret = parent_loop(buf["rew"], buf["done"], buf["val"], GAMMA, TAU)
    assert torch.equal(buf["adv"], adv) and torch.equal(buf["ret"], ret)
    stats = tr.update(buf)
    assert "episodes_ended" not in stats and math.isfinite(stats["loss"])
    assert "episode_ends" in tr.state_dict()["config"]


def test_an_env_without_a_native_engine_is_refused():
    from minibatch_step_util import StubEnv
    with pytest.raises(ValueError, match="no native engine"):
        PPOTrainer(StubEnv(41, 113, "cpu"), 41, 113, 9, PPOConfig(episode_ends=True), device="cpu")
    PPOTrainer(StubEnv(41, 113, "cpu"), 41, 113, 9, PPOConfig(), device="cpu")        # ... and only with the mode on


# ---- data parallel: no collective is added -----------------------------------------------------------------------------------------------------
def test_a_world_of_one_issues_the_same_collectives(oracle, tmp_path):
    import torch.distributed as dist
    counts = {}
    dist.init_process_group("gloo", store=dist.FileStore(str(tmp_path / "store"), 1), rank=0, world_size=1)
    try:
        for on in (False, True):
            tr, _ = trainer(oracle, episode_ends=on, value_bootstrap=on, normalize_input=True)
            assert tr.dist_on
            tr.train(1)
            counts[on] = (tr.n_grad_allreduce, tr.n_kl_allreduce, tr.n_norm_allgather, tr.n_eval_allreduce)
    finally:
        dist.destroy_process_group()
    assert counts[True] == counts[False] == (2 * 4, 2, 1, 0)
