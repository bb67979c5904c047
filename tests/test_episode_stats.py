"""Episode statistics (leibnizgym_amd/evaluate.py) on the CPU: the plain-torch path over rollouts of the oracle (injected through `lib=`) against the numpy
reference of tests/episode_stats_ref.py, the cap, non-finite episodes, the result dict, two ranks over gloo, and PPOTrainer.evaluate / mean_action on the
torch path.  The kernel's side of the same definitions is tests/test_episode_stats_gpu.py."""
import math
import os
import socket
import sys

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

import parity_util as pu
from episode_stats_ref import RefStats, compare
from leibnizgym_amd import evaluate as ev
from leibnizgym_amd.evaluate import EpisodeStats

N, EP_LEN, STEPS = 70, 20, 65            # every env ends three episodes (steps 20, 40, 60) and is five steps into a fourth
PLANT_BEFORE = (3, 10, 19, 25, 39, 47, 59)        # 0-based indices of the steps in front of which goals are planted; 19, 39 and 59 are ending steps
YAW = 0.5


def engine(lib, n=N, success=False, off=0, total=None, episode_length=EP_LEN):
    from leibnizgym_amd.engine import TrifingerEngine, make_config
    kw = dict(pu.CONFIGS["d4_torque_asym"])
    kw["success"] = dict(kw["success"], activate=success)
    return TrifingerEngine(make_config(lib, n, seed=3, episode_length=episode_length, env_id_offset=off, global_num_envs=total or n, **kw), device="cpu", lib=lib)


def plant(eng, ids):
    """goals into the state views by GLOBAL env id: id % 3 == 0 at the cube's pose, == 1 3 cm and 0.5 rad (about z) off it, == 2 untouched"""
    cube, goal = eng.cube, eng.goal
    ids = torch.as_tensor(ids)
    a, b = ids % 3 == 0, ids % 3 == 1
    goal[0:7, a] = cube[0:7, a]
    goal[0:3, b] = cube[0:3, b] + torch.tensor([0.03, 0.0, 0.0]).unsqueeze(1)
    x, y, z, w = cube[3:7, b]
    s, c = math.sin(YAW / 2), math.cos(YAW / 2)                 # cube_q (x) (0, 0, s, c)
    goal[3:7, b] = torch.stack([x * c + y * s, y * c - x * s, z * c + w * s, w * c - z * s])


def rollout(eng, observers, off=0, total=N, steps=STEPS, poke=None):
    """`steps` steps under the fixed action function of (global env id, step); after every step each observer sees the engine"""
    cnt = eng.num_envs
    eng.reset()
    for t in range(steps):
        if t in PLANT_BEFORE:
            plant(eng, torch.arange(off, off + cnt))
        eng.step(pu.actions_for(t, total, eng.action_dim, 3)[off:off + cnt].contiguous())
        if poke is not None:
            poke(t, eng)
        for o in observers:
            o(eng)


def ref_observer(ref):
    return lambda e: ref.update(e.state.numpy(), e.reward.numpy(), e.reset_buf.numpy(), e.goal_reset_buf.numpy(), e.steps.numpy())


@pytest.mark.parametrize("success", [True, False], ids=["success-on", "success-off"])
def test_torch_path_against_the_numpy_reference(oracle, success):
    """A: 70 envs, episode_length 20, 65 steps, planted goals; counters, integer sums, the return sum and both histograms exactly, the error sums within
    episodes + 2^-20 sum|q| fixed-point units.  The planted offsets (0, 3 cm / 0.5 rad) keep every sample of every step away from the tolerances, so
    every counter and integer sum is asked EXACTLY.  0.5 rad is itself an edge of the orientation histogram (bits(0.5) >> 21 == 504), which a cube at
    rest through its last step keeps: 48 of the 9520 tested samples (0.5 %) sit at that one edge, and only there - between the bins [0.4375, 0.5) and
    [0.5, 0.625) of the orientation histogram - may a sample be in either bin (episode_stats_ref.compare); the position histogram is exact."""
    eng = engine(oracle, success=success)
    st = EpisodeStats(eng)
    assert (st.pos_tol, st.ori_tol, st.rule, st.fused) == (pytest.approx(0.02), pytest.approx(0.25), 1, False)
    ref = RefStats(N, st.pos_tol, st.ori_tol, st.rule)
    rollout(eng, [lambda e: st.update(), ref_observer(ref)])
    r = st.result()
    frac = compare(r["raw"], ref, f"success={success}")
    print(f"undecidable samples: {100 * frac:.3f} % ({ref.undecidable} of {ref.samples}), near a tolerance {ref.near_tol}")
    assert ref.near_tol == 0 and int(ref.near_edge[ev.HIST_POS].sum()) == 0
    edge = 504 - ev.ORI_Q[0]                                      # the edge at 0.5 rad
    assert int(ref.near_edge[ev.HIST_ORI].sum()) == int(ref.near_edge[ev.HIST_ORI][edge])
    assert r["episodes"] == 3 * N and r["nonfinite_episodes"] == 0 and r["episode_length_mean"] == EP_LEN
    assert r["raw"][ev.SUCCESS] >= N // 3 and r["raw"][ev.REACHED] >= r["raw"][ev.SUCCESS]          # the goals planted in front of the ending steps
    assert (r["goals_reached"] > 0) == success                    # goal events exist only where success termination is on
    assert st.env_acc[ev.ENV_EPISODES].tolist() == [3] * N
    assert 0 < r["success_rate"] < 1 and 0 < r["time_at_goal_fraction"] < 1 and r["steps_to_goal_mean"] >= 1


def test_the_cap(oracle):
    """B: with max_episodes_per_env = 2 only two episodes per env count, ENVS_COMPLETE == 70 after step 40, and the steps 41-65 change nothing but per-env state"""
    eng = engine(oracle)
    st = EpisodeStats(eng, max_episodes_per_env=2)
    ref = RefStats(N, st.pos_tol, st.ori_tol, st.rule, cap=2)
    seen = []
    rollout(eng, [lambda e: st.update(), ref_observer(ref), lambda e: seen.append((st.acc.clone(), st.env_acc.clone()))])
    compare(st.result()["raw"], ref, "cap")
    assert int(seen[38][0][ev.ENVS_COMPLETE]) == 0 and int(seen[39][0][ev.ENVS_COMPLETE]) == N and st.envs_complete() == N
    assert all(torch.equal(a, seen[39][0]) for a, _ in seen[40:])
    assert int(seen[39][0][ev.EPISODES]) == 2 * N
    assert not torch.equal(seen[45][1][ev.ENV_RETURN], seen[44][1][ev.ENV_RETURN])            # capped envs still run
    assert seen[-1][1][ev.ENV_EPISODES].tolist() == [2] * N


def test_a_nonfinite_episode_is_counted_apart(oracle):
    """C: a NaN in one env's cube row at its ending step gives NONFINITE == 1, and that episode is in no sum or bin.  The NaN is written behind the step
    and in front of the update: a NaN the step itself reads is caught by its guard, which parks the env at a finite pose."""
    eng = engine(oracle)
    st = EpisodeStats(eng)
    ref = RefStats(N, st.pos_tol, st.ori_tol, st.rule)

    def poke(t, e):
        if t == 19:
            e.state[18, 7] = float("nan")
    rollout(eng, [lambda e: st.update(), ref_observer(ref)], poke=poke)
    r = st.result()
    compare(r["raw"], ref, "nonfinite")
    assert r["nonfinite_episodes"] == 1
    assert sum(r["raw"][ev.HIST_POS:ev.HIST_POS + ev.POS_BINS]) == r["episodes"] == sum(r["raw"][ev.HIST_ORI:])
    assert math.isfinite(r["final_position_error_mean"]) and math.isfinite(r["episode_reward_mean"])
    q = float("nan")                                  # a non-finite quaternion: the step's quat_diff_rad would report pi for it
    eng2 = engine(oracle)
    st2 = EpisodeStats(eng2)
    rollout(eng2, [lambda e: st2.update()], steps=20, poke=lambda t, e: e.state.__setitem__((21, 5), q) if t == 19 else None)
    assert st2.result()["nonfinite_episodes"] == 1 and st2.result()["episodes"] == N - 1


def test_result_of_a_hand_made_vector():
    """D: rates, means and the quantile bins from a hand-made vector; zero episodes give nan, not an exception"""
    raw = [0] * ev.ACC
    r = ev.summarize(raw)
    assert r["episodes"] == 0 and all(math.isnan(r[k]) for k in ("success_rate", "episode_reward_mean", "steps_to_goal_mean", "time_at_goal_fraction"))
    assert all(math.isnan(x) for x in r["final_position_error_median"] + r["final_orientation_error_p90"])
    raw[ev.EPISODES], raw[ev.SUCCESS], raw[ev.POS_OK], raw[ev.ORI_OK], raw[ev.REACHED] = 10, 4, 6, 5, 8
    raw[ev.SUM_LENGTH], raw[ev.SUM_AT_GOAL_STEPS], raw[ev.SUM_FIRST_HIT], raw[ev.GOAL_EVENTS], raw[ev.NONFINITE] = 200, 50, 24, 3, 1
    raw[ev.SUM_RETURN], raw[ev.SUM_POS_ERR], raw[ev.SUM_ORI_ERR] = -15 * 2 ** 16, 2 ** 30 // 4, 5 * 2 ** 28
    raw[ev.HIST_POS + 0], raw[ev.HIST_POS + 1], raw[ev.HIST_POS + 49] = 5, 4, 1          # ranks 5 and 9: bins 0 and 1
    raw[ev.HIST_ORI + 41], raw[ev.HIST_ORI + 9] = 2, 8                                      # ranks 5 and 9: bins 9 and 41
    r = ev.summarize(raw)
    assert (r["success_rate"], r["success_rate_position"], r["success_rate_orientation"], r["reached_goal_rate"]) == (0.4, 0.6, 0.5, 0.8)
    assert (r["steps_to_goal_mean"], r["time_at_goal_fraction"], r["goals_reached"], r["nonfinite_episodes"]) == (3.0, 0.25, 3, 1)
    assert (r["episode_reward_mean"], r["episode_length_mean"], r["final_position_error_mean"], r["final_orientation_error_mean"]) == (-1.5, 20.0, 0.025, 0.5)
    assert r["final_position_error_median"] == (0.0, 2.0 ** -12) and r["final_position_error_p90"] == (2.0 ** -12, 1.25 * 2.0 ** -12)
    assert r["final_orientation_error_median"] == (2.0 ** -6, 1.25 * 2.0 ** -6) and r["final_orientation_error_p90"] == (4.0, math.inf)
    raw[ev.HIST_POS + 49], raw[ev.HIST_POS + 48] = 6, 0
    raw[ev.HIST_POS + 0] = 0
    assert ev.summarize(raw)["final_position_error_median"] == (1.0, math.inf)
    assert ev.bin_edge(460) == 2.0 ** -12 and ev.bin_edge(508) == 1.0 and ev.bin_edge(476) == 2.0 ** -8 and ev.bin_edge(516) == 4.0
    x = torch.tensor([0.0, 2.0 ** -12, 0.99999994, 1.0, 1.25 * 2.0 ** -12, 3.0e38])
    assert ev._bins(x, *ev.POS_Q).tolist() == [0, 1, 48, 49, 2, 49]
    with pytest.raises(ValueError):
        ev.summarize([0] * 5)
    with pytest.raises(ValueError):
        ev.engine_of(object())


def test_library_binding_and_refusals():
    """the new header's names are exported and bound (argtypes and restype), and bad arguments are refused before any launch: no GPU needed"""
    import ctypes as C
    import re
    from leibnizgym_amd import ppo_kernels as pk
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(os.path.dirname(pk.library_path()), "..", "..", "include", "trifinger_ppo_eval.h")).read(), flags=re.S)
    names = sorted(set(re.findall(r"\b(tfp_[a-z0-9_]+)\s*\(", src)))
    assert names == ["tfp_eval_step", "tfp_eval_test_predicates"]
    lib = pk.load()
    for n in names:
        assert getattr(lib, n).restype is C.c_int and getattr(lib, n).argtypes
    for k, v in (("TFP_EVAL_ACC", ev.ACC), ("TFP_EVAL_POS_BINS", ev.POS_BINS), ("TFP_EVAL_ORI_BINS", ev.ORI_BINS)):
        assert k in src
    assert (ev.HIST_POS, ev.HIST_ORI, ev.ACC) == (14, 64, 106)
    p = 4096                                              # never dereferenced: every call below is refused on the host
    assert lib.tfp_eval_step(p, p, p, p, p, p, p, 0, 0.02, 0.2, 1, 0, None) == -1
    assert lib.tfp_eval_step(p, p, p, p, p, p, p, 2097153, 0.02, 0.2, 1, 0, None) == -1
    assert lib.tfp_eval_step(p, p, p, p, p, p, p, 4, 0.02, 0.2, 3, 0, None) == -1
    assert lib.tfp_eval_step(p, p, p, p, p, p, p, 4, 0.02, 0.2, 1, -1, None) == -1
    for k in range(7):
        assert lib.tfp_eval_step(*[None if j == k else p for j in range(7)], 4, 0.02, 0.2, 1, 0, None) == -1
    assert lib.tfp_eval_test_predicates(None, 4, 0.02, 0.2, p, None) == -1


def _rank(rank, world, port, out_dir):
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
    from oracle_util import load_oracle
    import test_episode_stats as me
    torch.set_num_threads(1)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    seen = []                                             # every collective this process issues, observed at torch.distributed itself
    for name in ("all_reduce", "all_gather", "all_gather_into_tensor", "broadcast", "reduce", "reduce_scatter", "barrier", "all_to_all", "gather", "scatter"):
        def wrapped(*a, _f=getattr(dist, name), _n=name, **k):
            seen.append(_n)
            return _f(*a, **k)
        setattr(dist, name, wrapped)
    cnt = N // world
    eng = me.engine(load_oracle(), n=cnt, success=True, off=rank * cnt, total=N)
    st = EpisodeStats(eng)
    me.rollout(eng, [lambda e: st.update()], off=rank * cnt, total=N)
    local = st.acc.clone()
    st.merge()
    np.savez(os.path.join(out_dir, f"rank{rank}.npz"), raw=st.acc.numpy(), local=local.numpy(), n_allreduce=st.n_allreduce, collectives=np.array(seen))
    dist.destroy_process_group()


def test_two_ranks_give_the_vector_of_one_engine(oracle, tmp_path):
    """E: two shards of 35 envs (env_id_offset) and one engine of 70 envs give the same vector bit for bit after merge; one collective per rank"""
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        port = s.getsockname()[1]
    mp.spawn(_rank, args=(2, port, str(tmp_path)), nprocs=2, join=True)
    eng = engine(oracle, success=True)
    st = EpisodeStats(eng)
    rollout(eng, [lambda e: st.update()])
    want = st.acc.numpy()
    parts = [np.load(os.path.join(tmp_path, f"rank{r}.npz")) for r in range(2)]
    for p in parts:
        assert np.array_equal(p["raw"], want) and int(p["n_allreduce"]) == 1 and p["collectives"].tolist() == ["all_reduce"]
    assert not np.array_equal(parts[0]["local"], parts[1]["local"]) and np.array_equal(parts[0]["local"] + parts[1]["local"], want)
    assert want[ev.EPISODES] == 3 * N


def _trainer(oracle, n=32, episode_length=EP_LEN, **kw):
    from leibnizgym_amd.config import gym_config
    from leibnizgym_amd.envs import TrifingerEnv
    from leibnizgym_amd.ppo import PPOConfig, PPOTrainer
    from leibnizgym_amd.utils.rlg_train import RlGamesGpuEnvAdapter
    from leibnizgym_amd.wrappers import VecTaskPython
    cfg = gym_config("trifinger_difficulty_4")
    cfg.update(num_instances=n, seed=1, physics_engine="physx", asymmetric_obs=True, episode_length=episode_length)
    env = TrifingerEnv(config=cfg, device="cpu", verbose=False, lib=oracle)
    ad = RlGamesGpuEnvAdapter("rlgpu", n, env=VecTaskPython(env, rl_device="cpu"))
    return PPOTrainer(ad, 41, 113, 9, PPOConfig(horizon=8, minibatches=4, mini_epochs=2, **kw), device="cpu"), env


@pytest.mark.parametrize("deterministic", [True, False], ids=["deterministic", "stochastic"])
def test_trainer_evaluate_on_the_torch_path(oracle, deterministic):
    """F: episodes == N K; parameters, frames, epoch and the input records unchanged; self.last is a reset observation; mean_action is dist_and_value's mu"""
    tr, env = _trainer(oracle, normalize_input=True, normalize_input_value=True)
    tr.train(1)
    before = {k: v.clone() for k, v in tr.net.state_dict().items()}
    recs = {k: {a: b.clone() for a, b in r.state_dict().items()} for k, r in tr._norm_records().items()}
    frames, epoch = tr.frames, tr.epoch
    assert ev.engine_of(tr.env) is env._engine and ev.engine_of(env) is env._engine
    r = tr.evaluate(episodes_per_env=2, deterministic=deterministic)
    assert r["episodes"] + r["nonfinite_episodes"] == 32 * 2 and r["envs_complete"] == 32 and r["steps"] == 2 * EP_LEN
    assert r["episode_length_mean"] == EP_LEN and math.isfinite(r["episode_reward_mean"]) and len(r["raw"]) == ev.ACC
    assert (tr.frames, tr.epoch, tr.n_eval_allreduce) == (frames, epoch, 0)
    assert all(torch.equal(v, before[k]) for k, v in tr.net.state_dict().items())
    assert recs and all(torch.equal(b, recs[k][a]) for k, rec in tr._norm_records().items() for a, b in rec.state_dict().items())
    eng = env._engine
    assert int(eng.steps.abs().sum()) == 0 and torch.equal(tr.last[0], eng.obs) and torch.equal(tr.last[1], eng.states)
    obs, states = tr.last
    with torch.no_grad():
        assert torch.equal(tr.net.mean_action(obs), tr.net.dist_and_value(obs, states)[0])
    assert tr.evaluate(episodes_per_env=3, max_steps=25)["steps"] == 25
    assert math.isfinite(tr.train(1)[-1]["loss"])                   # training goes on from the reset


def test_trainer_evaluate_needs_an_end(oracle):
    tr, _ = _trainer(oracle, n=8, episode_length=0)
    with pytest.raises(ValueError, match="max_steps"):
        tr.evaluate()
    assert tr.evaluate(max_steps=3)["episodes"] == 0
    with pytest.raises(ValueError, match="episodes_per_env"):
        tr.evaluate(episodes_per_env=0)
