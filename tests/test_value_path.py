"""`clip_value`, `central_value_config.clip_value` and `normalize_value` in the in-repo PPO (leibnizgym_amd/ppo.py), CPU side, torch path on the oracle env:
the three keys arrive, nothing new runs when they are off, the clipped value loss against a float64 restatement, the returns' record frozen for an epoch and
merged at its end, the buffers against the stated expressions bit for bit, checkpoints, two gloo ranks.  The kernels are held in tests/test_value_path_gpu.py."""
import copy
import os
import socket

import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

import leibnizgym_amd.ppo as ppo
from leibnizgym_amd import ppo_kernels as pk
from leibnizgym_amd.config import RLG_ASYMM, compose
from leibnizgym_amd.ppo import PPOConfig, PPOTrainer
from test_ppo import make
from value_path_util import E_CLIP, planted, restated, restated_with_grad

RTOL, ATOL = 1e-9, 1e-12            # the record against two-pass float64 moments: the tolerances of tests/test_input_norm.py
T, N = 8, 32


def trainer(oracle, state_dim=113, n=N, **kw):
    env, ad = make(oracle, n=n)
    cfg = PPOConfig(horizon=T, minibatches=4, mini_epochs=2, **kw)
    return PPOTrainer(ad, 41, state_dim, 9, cfg, device="cpu")


def plant(tr, mean=3.0, std=2.0, count=100.0):
    rec = tr.value_norm
    rec.state.copy_(torch.tensor([count, mean, std * std * count], dtype=torch.float64))
    rec.publish()
    return rec


def denorm(y, rec):
    return torch.clamp(y, -5.0, 5.0) / rec.inv_std_f + rec.mean_f


def raw_values(tr, buf):
    """the critic's raw output recomputed on the rows the rollout stored (and on the observation it stopped at), [T + 1, n]"""
    with torch.no_grad():
        st = buf["states"]
        rows = [tr.net.value(buf["obs"][t], st[t] if st is not None else None) for t in range(buf["obs"].shape[0])]
        rows.append(tr.net.value(*tr.last))
    return torch.stack(rows)


# ---- config ----------------------------------------------------------------------------------------------------------------------------------
def test_from_rlg_reads_the_three_keys():
    c = PPOConfig()
    assert (c.clip_value, c.clip_value_central, c.normalize_value) == (False, False, False)
    c = PPOConfig.from_rlg(RLG_ASYMM, num_envs=64)                        # the reference's tree
    assert (c.clip_value, c.clip_value_central, c.normalize_value) == (False, False, False)
    for path, want in ((("clip_value",), (True, False, False)), (("central_value_config", "clip_value"), (False, True, False)),
                       (("normalize_value",), (False, False, True))):
        t = copy.deepcopy(RLG_ASYMM)
        node = t["params"]["config"]
        for k in path[:-1]:
            node = node[k]
        node[path[-1]] = True
        c = PPOConfig.from_rlg(t, num_envs=64)
        assert (c.clip_value, c.clip_value_central, c.normalize_value) == want, path


def test_launcher_overrides_reach_from_rlg():
    """what scripts/train_ppo.py and scripts/rlg_hydra.py (utils/rlg_train.py) do with their command line: compose(), then from_rlg on the `rlg` tree"""
    cfg = compose(["gym=trifinger_difficulty_4", "rlg.params.config.clip_value=True", "rlg.params.config.central_value_config.clip_value=True",
                   "rlg.params.config.normalize_value=True"])
    c = PPOConfig.from_rlg(cfg["rlg"], num_envs=64)
    assert (c.clip_value, c.clip_value_central, c.normalize_value) == (True, True, True)
    c = PPOConfig.from_rlg(compose(["gym=trifinger_difficulty_4", "rlg.params.config.normalize_value=True"])["rlg"], num_envs=64)
    assert (c.clip_value, c.clip_value_central, c.normalize_value) == (False, False, True)
    c = PPOConfig.from_rlg(compose(["gym=trifinger_difficulty_4"])["rlg"], num_envs=64)
    assert (c.clip_value, c.clip_value_central, c.normalize_value) == (False, False, False)


def test_which_clip_key_applies_depends_on_who_is_the_critic(oracle):
    assert trainer(oracle, clip_value_central=True).clip_v and not trainer(oracle, clip_value=True).clip_v
    assert trainer(oracle, state_dim=0, clip_value=True).clip_v and not trainer(oracle, state_dim=0, clip_value_central=True).clip_v


# ---- off is off ------------------------------------------------------------------------------------------------------------------------------
def test_off_is_off(oracle, monkeypatch):
    def boom(*a, **k):
        raise AssertionError("a function of the value path ran with its keys off")
    monkeypatch.setattr(pk, "gae_vnorm", boom)
    monkeypatch.setattr(ppo, "clipped_value_loss", boom)
    monkeypatch.setattr(ppo, "denormalize_value", boom)
    merge = PPOTrainer._update_input_norm                  # the returns join the end-of-epoch merge through its `returns` argument
    monkeypatch.setattr(PPOTrainer, "_update_input_norm", lambda self, src, returns=None: boom() if returns is not None else merge(self, src))
    tr = trainer(oracle)
    assert tr.value_norm is None and tr.net.value_norm is None and not tr.clip_v
    seen = []
    inner = tr._mb_backward
    tr._mb_backward = lambda d, idx, acc: (seen.append(sorted(d)), inner(d, idx, acc))[1]
    stats = tr.train(2)
    assert len(stats) == 2 and tr.frames == 2 * T * N
    assert seen and all("old_v" not in keys for keys in seen)
    sd = tr.state_dict()
    assert "value_norm" not in sd and "input_norm" not in sd


# ---- the clipped loss ------------------------------------------------------------------------------------------------------------------------
def test_clipped_value_loss_against_the_float64_restatement():
    """float32 `clipped_value_loss` and its autograd gradient against the restatement.  Tolerance: all values lie in [-2, 2] (ulp <= 2.4e-7), a term is the
    square of x = (v_old + clamp(v - v_old)) - ret, three rounded operations, |x| <= 0.8: |error of x| <= 4e-7, of x^2 <= 2 * 0.8 * 4e-7 + 6e-8 * 0.64 < 1e-6;
    the gradient 2 (v - ret) carries one rounding: < 5e-7."""
    v, ret, v_old = planted(700, seed=1)
    want_c, want_g = restated_with_grad(v, ret, v_old)
    vv = v.clone().requires_grad_(True)
    c = ppo.clipped_value_loss(vv, ret, v_old, E_CLIP)
    c.sum().backward()
    assert c.dtype == torch.float32
    assert torch.allclose(c.double(), want_c, rtol=0, atol=1e-6)
    assert torch.allclose(vv.grad.double(), want_g, rtol=0, atol=5e-7)
    # the four regimes did what the definition says: no gradient exactly where the clipped term is the larger one
    dd = v.double() - v_old.double()
    lu, lc = (v.double() - ret.double()) ** 2, (v_old.double() + dd.clamp(-E_CLIP, E_CLIP) - ret.double()) ** 2
    dead = (dd.abs() > E_CLIP) & (lc > lu)
    assert bool(dead.any()) and bool((vv.grad[dead] == 0).all()) and bool((vv.grad[~dead] == (2 * (v - ret))[~dead]).all())
    assert torch.equal(c[dd == 0], ((v - ret) ** 2)[dd == 0])             # v = v_old: the unclipped term, as written


def test_clip_value_reaches_the_minibatch_loss(oracle):
    """clip on, normalisation off: the value term of the first minibatch is the restated loss around the rollout's own values buf["val"][:T]"""
    tr = trainer(oracle, clip_value_central=True)
    buf = tr.rollout()
    got = first_minibatch_value_term(tr, buf)
    assert torch.equal(got["d"]["old_v"], buf["val"][:T].reshape(-1)) and torch.equal(got["d"]["ret"], buf["ret"].reshape(-1))
    assert abs(got["c_loss"] - got["want"]) <= 1e-5 * max(1.0, abs(got["want"]))


def first_minibatch_value_term(tr, buf):
    """runs update(); returns the first minibatch's source arrays, its c_loss as the trainer accumulated it, and the float64 restatement on the same rows"""
    out = {}
    inner = tr._mb_backward

    def spy(d, idx, acc):
        first = not out
        if first:
            with torch.no_grad():
                v = tr.net.value(d["obs"][idx], d["states"][idx] if d["states"] is not None else None)
            out.update(d=d, want=float(restated(v, d["ret"][idx], d["old_v"][idx]).mean()))
        inner(d, idx, acc)
        if first:
            out["c_loss"] = float(acc["c_loss"])
    tr._mb_backward = spy
    tr.update(buf)
    tr._mb_backward = inner
    return out


# ---- the returns' record ---------------------------------------------------------------------------------------------------------------------
def test_record_is_frozen_for_an_epoch_and_holds_the_moments_of_the_returns(oracle):
    tr = trainer(oracle, normalize_value=True)
    rec = tr.value_norm
    assert rec is not None and rec.dim == 1 and rec.clip == 5.0 and tr.net.value_norm is rec
    assert float(rec.count) == 0 and float(rec.mean_f) == 0.0            # count 0 publishes mean 0, variance 1
    assert torch.equal(rec.inv_std_f, torch.full((1,), 1.0 / (1.0 + 1e-5) ** 0.5, dtype=torch.float64).float())
    rets, k = [], 3
    for epoch in range(1, k + 1):
        start = [t.clone() for t in (rec.state, rec.mean_f, rec.inv_std_f)]
        same = lambda: all(torch.equal(a, b) for a, b in zip(start, (rec.state, rec.mean_f, rec.inv_std_f)))      # noqa: E731
        seen = []
        inner = tr._mb_backward
        tr._mb_backward = lambda d, idx, acc: (seen.append(same()), inner(d, idx, acc))[1]
        buf = tr.rollout()
        assert same()
        st = tr.update(buf)
        tr._mb_backward = inner
        assert len(seen) == 2 * 4 and all(seen)                           # unchanged up to the last minibatch ...
        assert not torch.equal(start[0], rec.state)                       # ... and merged behind it
        assert all(torch.isfinite(torch.tensor([st["loss"], st["c_loss"], st["kl"]])))
        rets.append(buf["ret"].reshape(-1))
        assert float(rec.count) == epoch * T * N
        x = torch.cat(rets).double()
        mean = x.mean()
        assert torch.allclose(rec.mean[0], mean, rtol=RTOL, atol=ATOL)
        assert torch.allclose(rec.m2[0] / rec.count, ((x - mean) ** 2).sum() / x.numel(), rtol=RTOL, atol=ATOL)
        assert torch.equal(rec.mean_f, rec.mean.float()) and torch.equal(rec.inv_std_f, (1.0 / torch.sqrt(rec.m2 / rec.count + 1e-5)).float())


@pytest.mark.parametrize("state_dim", [113, 0])
def test_planted_record_buffers_hold_the_stated_expressions(oracle, state_dim):
    """mean 3, standard deviation 2; with a central value network and without one (the critic on `obs`)"""
    tr = trainer(oracle, state_dim=state_dim, normalize_value=True, clip_value=True, clip_value_central=True)
    rec = plant(tr)
    assert float(rec.mean_f) == 3.0 and abs(float(rec.inv_std_f) - 0.5) < 1e-6
    buf = tr.rollout()
    y = raw_values(tr, buf)
    assert torch.equal(buf["val"], denorm(y, rec))                        # de-normalised, bit for bit - the bootstrap value of step T included
    assert torch.equal(buf["v_old_n"], torch.clamp(y[:T], -5.0, 5.0))     # not a round trip through v
    assert torch.equal(buf["ret"], buf["adv"] + buf["val"][:T])
    assert torch.equal(buf["ret_n"], torch.clamp((buf["ret"] - rec.mean_f) * rec.inv_std_f, -5.0, 5.0))
    # GAE ran on the de-normalised values: the backward loop of the trainer, restated
    adv, last = torch.zeros(T, N), torch.zeros(N)
    for t in reversed(range(T)):
        nd = 1.0 - buf["done"][t]
        last = buf["rew"][t] + 0.99 * buf["val"][t + 1] * nd - buf["val"][t] + 0.99 * 0.95 * nd * last
        adv[t] = last
    assert torch.equal(buf["adv"], adv)
    assert float((buf["val"] - 3.0).abs().max()) < 10.0 + 1e-3 and float(buf["val"].mean()) > 1.0      # values live around the planted mean
    got = first_minibatch_value_term(tr, buf)
    assert torch.equal(got["d"]["ret"], buf["ret_n"].reshape(-1)) and torch.equal(got["d"]["old_v"], buf["v_old_n"].reshape(-1))
    assert abs(got["c_loss"] - got["want"]) <= 1e-5 * max(1.0, abs(got["want"]))                      # the loss, and its clip range, in normalised units
    assert float(rec.count) == 100 + T * N                                # merged once, behind the minibatches


def test_act_play_and_value_denorm(oracle):
    tr = trainer(oracle, normalize_value=True)
    plant(tr)
    tr.train(1)
    rec = tr.value_norm
    before = [rec.state.clone(), rec.mean_f.clone(), rec.inv_std_f.clone()]
    a = tr.act(torch.randn(5, 41))
    tr.play(3)
    obs, states = torch.randn(6, 41), torch.randn(6, 113)
    with torch.no_grad():
        assert torch.equal(tr.net.value_denorm(obs, states), denorm(tr.net.value(obs, states), rec))
    assert all(torch.equal(x, y) for x, y in zip(before, (rec.state, rec.mean_f, rec.inv_std_f)))
    assert a.shape == (5, 9)
    off = trainer(oracle)                                                 # without the record value_denorm is value
    with torch.no_grad():
        assert torch.equal(off.net.value_denorm(obs, states), off.net.value(obs, states))


# ---- checkpoints -----------------------------------------------------------------------------------------------------------------------------
def test_checkpoint_round_trip_and_mismatches(oracle, tmp_path):
    a = trainer(oracle, normalize_value=True, clip_value_central=True)
    a.train(2)
    path = a.save(os.path.join(tmp_path, "v.pth"))
    assert sorted(torch.load(path, weights_only=False)["value_norm"]) == ["inv_std_f", "mean_f", "state"]
    b = trainer(oracle, normalize_value=True, clip_value_central=True)
    b.restore(path)
    ra, rb = a.value_norm, b.value_norm
    assert torch.equal(ra.state, rb.state) and torch.equal(ra.mean_f, rb.mean_f) and torch.equal(ra.inv_std_f, rb.inv_std_f)
    assert float(rb.count) == 2 * T * N

    def rejected(reader, p):
        before = {k: v.clone() for k, v in reader.net.state_dict().items()}
        rec = reader.value_norm.state_dict() if reader.value_norm is not None else None
        with pytest.raises(ValueError, match="value_norm|normalize_value"):
            reader.restore(p)
        for k, v in reader.net.state_dict().items():
            assert torch.equal(v, before[k]), k
        if rec is not None:
            assert all(torch.equal(rec[k], v) for k, v in reader.value_norm.state_dict().items())
    rejected(trainer(oracle), path)                                       # on in the checkpoint, off here
    plain = trainer(oracle)
    plain.train(1)
    plain_path = plain.save(os.path.join(tmp_path, "p.pth"))
    moved = trainer(oracle, normalize_value=True)
    moved.train(1)                                                        # a record that is not the initial one
    rejected(moved, plain_path)                                           # off in the checkpoint, on here
    ck = torch.load(path, weights_only=False)
    for key in ("state", "mean_f", "inv_std_f"):                          # a truncated record
        bad = copy.deepcopy(ck)
        bad["value_norm"][key] = bad["value_norm"][key][:-1].clone()
        bad_path = os.path.join(tmp_path, "bad.pth")
        torch.save(bad, bad_path)
        rejected(moved, bad_path)
    bad = copy.deepcopy(ck)
    del bad["value_norm"]["state"]                                        # a missing one
    torch.save(bad, bad_path)
    rejected(moved, bad_path)


# ---- two ranks -------------------------------------------------------------------------------------------------------------------------------
EPOCHS = 2


def _worker(rank, world, port, out):
    os.environ["MASTER_ADDR"], os.environ["MASTER_PORT"] = "127.0.0.1", str(port)
    import sys
    sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
    from oracle_util import load_oracle
    torch.set_num_threads(1)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    env, ad = make(load_oracle(), n=16, env_id_offset=rank * 16, global_num_instances=32)
    cfg = PPOConfig(horizon=4, minibatches=2, mini_epochs=1, seed=5, normalize_input=True, normalize_input_value=True, normalize_value=True,
                    clip_value_central=True)
    tr = PPOTrainer(ad, 41, 113, 9, cfg, device="cpu")
    rets = []
    for _ in range(EPOCHS):
        buf = tr.rollout()
        tr.update(buf)
        rets.append(buf["ret"].reshape(-1))
    torch.save({"ret": torch.cat(rets), "value": tr.value_norm.state_dict(), "obs": tr.net.obs_norm.state_dict(), "states": tr.net.state_norm.state_dict(),
                "n_norm_allgather": tr.n_norm_allgather}, os.path.join(out, f"r{rank}.pt"))
    dist.destroy_process_group()


def test_two_ranks_hold_the_same_records_with_one_gather_per_epoch(tmp_path):
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        port = s.getsockname()[1]
    mp.spawn(_worker, args=(2, port, str(tmp_path)), nprocs=2, join=True)
    r0, r1 = (torch.load(os.path.join(tmp_path, f"r{r}.pt")) for r in range(2))
    assert r0["n_norm_allgather"] == EPOCHS and r1["n_norm_allgather"] == EPOCHS
    for key in ("value", "obs", "states"):
        for k in ("state", "mean_f", "inv_std_f"):
            assert torch.equal(r0[key][k], r1[key][k]), (key, k)
    assert not torch.equal(r0["ret"], r1["ret"])                          # different shards, one record: the moments of their union
    x = torch.cat([r0["ret"], r1["ret"]]).double()
    st = r0["value"]["state"]
    assert float(st[0]) == x.numel() == EPOCHS * 2 * 4 * 16
    assert torch.allclose(st[1], x.mean(), rtol=RTOL, atol=ATOL)
    assert torch.allclose(st[2] / st[0], ((x - x.mean()) ** 2).sum() / x.numel(), rtol=RTOL, atol=ATOL)
