"""`normalize_input` / `central_value_config.normalize_input` in the in-repo PPO (leibnizgym_amd/ppo.py: InputNorm), CPU side: the two
config keys arrive, the merge formula against two-pass float64 moments, statistics frozen for an epoch, nothing new when the keys are off,
checkpoints, and two gloo ranks that end with the same record.  The kernels are held in tests/test_input_norm_gpu.py."""
import copy
import os
import socket

import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

from leibnizgym_amd import ppo_kernels as pk
from leibnizgym_amd.config import RLG_ASYMM, compose
from leibnizgym_amd.ppo import InputNorm, PPOConfig, PPOTrainer, neglogp
from test_ppo import make

RTOL, ATOL = 1e-9, 1e-12
NEW_KERNEL_FUNCTIONS = ("moments", "norm_merge", "normalize_rows", "_gather_rows_norm")


def two_pass(x):
    """(count, mean, population variance) of the rows of x, two passes in float64"""
    xd = x.reshape(-1, x.shape[-1]).double()
    mean = xd.mean(0)
    return xd.shape[0], mean, ((xd - mean) ** 2).sum(0) / xd.shape[0]


def assert_record(rec: InputNorm, x):
    n, mean, var = two_pass(x)
    assert float(rec.count) == n
    assert torch.allclose(rec.mean, mean, rtol=RTOL, atol=ATOL)
    assert torch.allclose(rec.m2 / rec.count, var, rtol=RTOL, atol=ATOL)
    assert torch.equal(rec.mean_f, rec.mean.float())
    assert torch.equal(rec.inv_std_f, (1.0 / torch.sqrt(rec.m2 / rec.count + 1e-5)).float())


def trainer(oracle, state_dim=113, n=32, **kw):
    env, ad = make(oracle, n=n)
    cfg = PPOConfig(horizon=8, minibatches=4, mini_epochs=2, **kw)
    return PPOTrainer(ad, 41, state_dim, 9, cfg, device="cpu")


# ---- config ----------------------------------------------------------------------------------------------------------------------
def test_from_rlg_reads_both_keys():
    c = PPOConfig.from_rlg(RLG_ASYMM, num_envs=64)
    assert c.normalize_input is False and c.normalize_input_value is False
    t = copy.deepcopy(RLG_ASYMM)
    t["params"]["config"]["normalize_input"] = True
    c = PPOConfig.from_rlg(t, num_envs=64)
    assert c.normalize_input is True and c.normalize_input_value is False
    t = copy.deepcopy(RLG_ASYMM)
    t["params"]["config"]["central_value_config"]["normalize_input"] = True
    c = PPOConfig.from_rlg(t, num_envs=64)
    assert c.normalize_input is False and c.normalize_input_value is True


def test_launcher_overrides_reach_from_rlg():
    """what scripts/train_ppo.py and utils/rlg_train.py do with their command line: compose(), then from_rlg on the `rlg` tree"""
    cfg = compose(["gym=trifinger_difficulty_4", "rlg.params.config.normalize_input=True",
                   "rlg.params.config.central_value_config.normalize_input=True"])
    c = PPOConfig.from_rlg(cfg["rlg"], num_envs=64)
    assert c.normalize_input is True and c.normalize_input_value is True
    c = PPOConfig.from_rlg(compose(["gym=trifinger_difficulty_4"])["rlg"], num_envs=64)
    assert c.normalize_input is False and c.normalize_input_value is False


# ---- the merge formula ---------------------------------------------------------------------------------------------------------------
def test_merge_of_batches_is_the_moments_of_their_concatenation():
    g = torch.Generator().manual_seed(3)
    D = 7
    scale = torch.tensor([1.0, 1e-2, 30.0, 1.0, 1.0, 1e3, 1.0])
    shift = torch.tensor([0.0, 1e4, -5.0, 0.0, 2.0, 0.0, 0.0])
    batches = [torch.randn(r, D, generator=g) * scale + shift for r in (1, 17, 256, 3, 1000)]
    for b in batches:
        b[:, 3] = 0.25                                     # a constant column
    rec = InputNorm(D, "cpu")
    assert float(rec.count) == 0 and torch.equal(rec.mean_f, torch.zeros(D))
    assert torch.equal(rec.inv_std_f, torch.full((D,), 1.0 / (1.0 + 1e-5) ** 0.5, dtype=torch.float64).float())
    # from count 0: the batch's own moments
    rec.merge(InputNorm.batch_record(batches[2]).unsqueeze(0))
    assert_record(rec, batches[2])
    # one by one, and several records in one call: both are the moments of everything seen
    rec = InputNorm(D, "cpu")
    for b in batches[:2]:
        rec.merge(InputNorm.batch_record(b).unsqueeze(0))
    rec.merge(torch.stack([InputNorm.batch_record(b) for b in batches[2:]]))
    assert_record(rec, torch.cat(batches))
    assert float(rec.m2[3]) == 0.0 and float(rec.mean[3]) == 0.25
    # normalize is the stated expression
    x = batches[4]
    assert torch.equal(rec.normalize(x), torch.clamp((x - rec.mean_f) * rec.inv_std_f, -5.0, 5.0))


# ---- frozen for an epoch ---------------------------------------------------------------------------------------------------------------
def test_statistics_are_frozen_for_an_epoch_and_updated_at_its_end(oracle):
    tr = trainer(oracle, normalize_input=True, normalize_input_value=True)
    ro, rs = tr.net.obs_norm, tr.net.state_norm
    assert ro is not None and rs is not None and ro.dim == 41 and rs.dim == 113
    T, n = 8, 32
    for epoch in range(1, 3):
        start = [t.clone() for t in (ro.mean_f, ro.inv_std_f, rs.mean_f, rs.inv_std_f, ro.state, rs.state)]
        seen = []
        inner = tr._mb_backward

        def spy(d, idx, acc):
            seen.append(all(torch.equal(a, b) for a, b in zip(start, (ro.mean_f, ro.inv_std_f, rs.mean_f, rs.inv_std_f, ro.state, rs.state))))
            return inner(d, idx, acc)
        tr._mb_backward = spy
        buf = tr.rollout()
        assert all(torch.equal(a, b) for a, b in zip(start, (ro.mean_f, ro.inv_std_f, rs.mean_f, rs.inv_std_f, ro.state, rs.state)))
        if epoch == 2:
            # the rollout buffers keep RAW observations, and the stored likelihoods belong to the frozen record: recomputed on the first minibatch
            # before any optimiser step they are old_nlp
            idx = torch.arange(64)
            flat = lambda x: x.reshape(T * n, *x.shape[2:])     # noqa: E731
            with torch.no_grad():
                mu, ls = tr.net.dist(flat(buf["obs"])[idx])
                again = neglogp(flat(buf["act"])[idx], mu, ls)
            assert torch.allclose(again, flat(buf["nlp"])[idx], rtol=1e-5, atol=1e-6)
            assert not torch.equal(ro.mean_f, torch.zeros(41))          # ... with statistics that are not the initial ones
        st = tr.update(buf)
        tr._mb_backward = inner
        assert len(seen) == 2 * 4 and all(seen)              # unchanged up to the last minibatch
        assert all(torch.isfinite(torch.tensor([st["loss"], st["kl"]])))
        assert float(ro.count) == epoch * T * n and float(rs.count) == epoch * T * n
        assert not torch.equal(start[4], ro.state)           # ... and merged behind it
        if epoch == 1:                                        # from count 0: the record is the epoch's own buffer
            assert_record(ro, buf["obs"])
            assert_record(rs, buf["states"])


def test_act_and_play_do_not_move_the_record(oracle):
    tr = trainer(oracle, normalize_input=True, normalize_input_value=True)
    tr.train(1)
    before = [tr.net.obs_norm.state.clone(), tr.net.state_norm.state.clone(), tr.net.obs_norm.inv_std_f.clone()]
    tr.act(torch.randn(5, 41))
    tr.play(3)
    assert torch.equal(before[0], tr.net.obs_norm.state) and torch.equal(before[1], tr.net.state_norm.state)
    assert torch.equal(before[2], tr.net.obs_norm.inv_std_f)


def test_without_a_central_value_network_the_critic_shares_the_actors_record(oracle):
    tr = trainer(oracle, state_dim=0, normalize_input=True, normalize_input_value=True)
    assert tr.net.state_norm is None and tr.net.critic_norm() is tr.net.obs_norm
    buf = tr.rollout()
    tr.update(buf)
    assert_record(tr.net.obs_norm, buf["obs"])
    assert sorted(tr.state_dict()["input_norm"]) == ["obs"]
    x = torch.randn(6, 41) * 3
    with torch.no_grad():
        assert torch.equal(tr.net.value(x, None), tr.net.critic(tr.net.obs_norm.normalize(x)).squeeze(-1))


# ---- off is off --------------------------------------------------------------------------------------------------------------------------
def test_off_is_off(oracle, monkeypatch):
    calls = []
    for name in NEW_KERNEL_FUNCTIONS:
        monkeypatch.setattr(pk, name, lambda *a, _n=name, **k: calls.append(_n))
    tr = trainer(oracle)
    assert tr.net.obs_norm is None and tr.net.state_norm is None
    tr.train(1)
    tr.act(torch.randn(3, 41))
    assert "input_norm" not in tr.state_dict()
    assert calls == [] and tr.n_norm_allgather == 0


# ---- checkpoints ---------------------------------------------------------------------------------------------------------------------------
def test_checkpoint_round_trip_and_mismatches(oracle, tmp_path):
    a = trainer(oracle, normalize_input=True, normalize_input_value=True)
    a.train(2)
    path = a.save(os.path.join(tmp_path, "n.pth"))
    b = trainer(oracle, normalize_input=True, normalize_input_value=True)
    b.restore(path)
    obs = torch.randn(32, 41) * 2
    assert torch.equal(a.act(obs), b.act(obs))
    for ra, rb in ((a.net.obs_norm, b.net.obs_norm), (a.net.state_norm, b.net.state_norm)):
        assert torch.equal(ra.state, rb.state) and torch.equal(ra.mean_f, rb.mean_f) and torch.equal(ra.inv_std_f, rb.inv_std_f)
    assert float(b.net.obs_norm.count) == 2 * 8 * 32

    def rejected(reader, p):
        before = {k: v.clone() for k, v in reader.net.state_dict().items()}
        recs = [r.state.clone() for r in reader._norm_records().values()]
        with pytest.raises(ValueError):
            reader.restore(p)
        for k, v in reader.net.state_dict().items():
            assert torch.equal(v, before[k]), k
        for r, s in zip(reader._norm_records().values(), recs):
            assert torch.equal(r.state, s)
    # the checkpoint and the trainer disagree about normalisation, in both directions and in one key only
    rejected(trainer(oracle), path)
    rejected(trainer(oracle, normalize_input=True), path)
    plain = trainer(oracle)
    plain.train(1)
    plain_path = plain.save(os.path.join(tmp_path, "p.pth"))
    rejected(trainer(oracle, normalize_input=True, normalize_input_value=True), plain_path)
    # a record of another width
    ck = torch.load(path, weights_only=False)
    for key in ("state", "mean_f"):
        bad = copy.deepcopy(ck)
        bad["input_norm"]["obs"][key] = bad["input_norm"]["obs"][key][:-2].clone()
        bad_path = os.path.join(tmp_path, "bad.pth")
        torch.save(bad, bad_path)
        rejected(trainer(oracle, normalize_input=True, normalize_input_value=True), bad_path)


# ---- two ranks -------------------------------------------------------------------------------------------------------------------------------
def _worker(rank, world, port, out):
    os.environ["MASTER_ADDR"], os.environ["MASTER_PORT"] = "127.0.0.1", str(port)
    import sys
    sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
    from oracle_util import load_oracle
    torch.set_num_threads(1)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    env, ad = make(load_oracle(), n=16, env_id_offset=rank * 16, global_num_instances=32)
    tr = PPOTrainer(ad, 41, 113, 9, PPOConfig(horizon=4, minibatches=2, mini_epochs=1, seed=5, normalize_input=True, normalize_input_value=True),
                    device="cpu")
    buf = tr.rollout()
    tr.update(buf)
    torch.save({"obs": buf["obs"], "states": buf["states"], "rec_obs": tr.net.obs_norm.state_dict(), "rec_states": tr.net.state_norm.state_dict(),
                "n_norm_allgather": tr.n_norm_allgather, "weights": [p.detach().clone() for p in tr.net.parameters()]},
               os.path.join(out, f"r{rank}.pt"))
    dist.destroy_process_group()


def test_two_ranks_hold_the_same_record(tmp_path):
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        port = s.getsockname()[1]
    mp.spawn(_worker, args=(2, port, str(tmp_path)), nprocs=2, join=True)
    r0, r1 = (torch.load(os.path.join(tmp_path, f"r{r}.pt")) for r in range(2))
    assert r0["n_norm_allgather"] == 1 and r1["n_norm_allgather"] == 1
    for key in ("rec_obs", "rec_states"):
        for k in ("state", "mean_f", "inv_std_f"):
            assert torch.equal(r0[key][k], r1[key][k]), (key, k)
    assert not torch.equal(r0["obs"], r1["obs"])                       # different shards ...
    for key, buf in (("rec_obs", "obs"), ("rec_states", "states")):    # ... one record: the moments of their union
        n, mean, var = two_pass(torch.cat([r0[buf].reshape(-1, r0[buf].shape[-1]), r1[buf].reshape(-1, r1[buf].shape[-1])]))
        st = r0[key]["state"]
        D = mean.numel()
        assert float(st[0]) == n == 2 * 4 * 16
        assert torch.allclose(st[1:1 + D], mean, rtol=RTOL, atol=ATOL)
        assert torch.allclose(st[1 + D:] / st[0], var, rtol=RTOL, atol=ATOL)
    assert all(torch.allclose(a, b, atol=1e-6) for a, b in zip(r0["weights"], r1["weights"]))
