"""`track_episodes` of the in-repo PPO on the CPU (include/trifinger_ppo_track.h, leibnizgym_amd/evaluate.py: EpisodeTracker, leibnizgym_amd/ppo.py): the
torch statement against a naive per-env loop over a scripted sequence, the binding and its refusals, the engine's step counter on the oracle, and the
trainer on the oracle env (injected through `lib=`): reported sums, parameters with the key on and off, score_to_win, the best checkpoint, save / restore and
two gloo ranks.  The kernel's side of the same definitions is tests/test_track_episodes_gpu.py."""
import copy
import math
import os
import socket
import sys

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

import track_episodes_util as tu
from leibnizgym_amd import evaluate as ev
from leibnizgym_amd.config import RLG_ASYMM
from leibnizgym_amd.evaluate import EpisodeTracker
from leibnizgym_amd.ppo import PPOConfig, PPOTrainer

EP_LEN, N, T = 6, 32, 4
PARENT_KEYS = {"kl", "loss", "a_loss", "c_loss", "lr", "mean_reward"}
MEAN_KEYS = {"episode_return", "episode_length", "success_rate", "pos_ok_rate", "ori_ok_rate", "timeout_rate", "final_pos_err", "final_ori_err"}
COUNT_KEYS = {"episodes", "episodes_total", "episodes_nonfinite", "episodes_unarmed"}


# ---- the torch statement against the naive loop -----------------------------------------------------------------------------------------------
def test_torch_statement_against_the_naive_loop():
    n = 19
    recs = tu.script(n)
    assert len(recs) == 40
    eng = tu.fake_engine(n, "cpu")
    trk = EpisodeTracker(eng, tu.POS_TOL, tu.ORI_TOL, rule=tu.RULE, episode_length=tu.EP_LEN)
    assert not trk.fused and trk.acc.dtype == torch.int64 and tuple(trk.env_trk.shape) == (2, n) and int(trk.env_trk.abs().sum()) == 0
    naive = tu.Naive(n)
    for t, rec in enumerate(recs):
        tu.load(eng, rec)
        trk.update()
        naive.update(rec)
        assert trk.acc.tolist() == naive.acc, t
        assert torch.equal(trk.env_trk, naive.env_trk()), t
    # what the scripted data holds, asserted on the data itself
    kinds = [e[0] for e in naive.events]
    assert kinds.count("counted") >= 1 and kinds.count("unarmed") == sum(1 for i in range(n) if i % 8 in (0, 6, 7)) and kinds.count("nonfinite") >= 2
    assert any(k == "counted" and s == 1 for k, s, _ in naive.events)                        # an episode of length 1
    assert any(k == "counted" and 1 < s < tu.EP_LEN and not to for k, s, to in naive.events)  # a termination that is not a time-out
    assert any(to for _, _, to in naive.events)
    a = naive.acc
    assert 0 < a[ev.T_SUCCESS] < a[ev.T_POS_OK] < a[ev.T_EPISODES] and 0 < a[ev.T_ORI_OK] < a[ev.T_EPISODES] and 0 < a[ev.T_TIMEOUT] < a[ev.T_EPISODES]
    inf_envs = [i for i in range(n) if i % 8 == tu.INF_AT[1]]
    assert all(math.isinf(float(recs[tu.INF_AT[0]]["reward"][i])) for i in inf_envs) and a[ev.T_NONFINITE] == len(inf_envs) + len([i for i in range(n) if i % 8 == 5])
    # take() hands the vector out and clears it; the per-env state stays
    trk_env = trk.env_trk.clone()
    v = trk.take()
    assert v.tolist() == naive.acc and int(trk.acc.abs().sum()) == 0 and torch.equal(trk.env_trk, trk_env)
    trk.reset_envs()
    assert int(trk.env_trk.abs().sum()) == 0


def test_window_and_its_statistics():
    def vec(n, ret=0, length=0, **kw):
        v = [0] * ev.TRACK_ACC
        v[ev.T_EPISODES], v[ev.T_SUM_RETURN], v[ev.T_SUM_LENGTH] = n, int(ret * 2 ** 16), length
        for k, x in kw.items():
            v[getattr(ev, k)] = x
        return v
    assert EpisodeTracker.window_stats([]) == {"episodes": 0} and EpisodeTracker.window([], 100) == [] and EpisodeTracker.window([vec(0)], 100) == []
    vs = [vec(60, -30, 600), vec(0), vec(50, 25, 250, T_SUCCESS=10, T_POS_OK=20, T_ORI_OK=25, T_TIMEOUT=40, T_SUM_POS_ERR=2 ** 30, T_SUM_ORI_ERR=2 ** 28), vec(0),
          vec(70, 35, 700, T_SUCCESS=50, T_SUM_POS_ERR=2 ** 29)]
    assert EpisodeTracker.window(vs, 100) == [vs[2], vs[4]]                    # newest first, whole vectors, until 100 episodes: 70 + 50
    assert EpisodeTracker.window(vs, 70) == [vs[4]] and EpisodeTracker.window(vs, 121) == [vs[0], vs[2], vs[4]] and EpisodeTracker.window(vs, 10 ** 6) == [vs[0], vs[2], vs[4]]
    st = EpisodeTracker.window_stats([vs[2], vs[4]])
    assert set(st) == MEAN_KEYS | {"episodes"} and st["episodes"] == 120
    assert (st["episode_return"], st["episode_length"], st["success_rate"], st["timeout_rate"]) == (0.5, 950 / 120, 0.5, 40 / 120)
    assert (st["pos_ok_rate"], st["ori_ok_rate"], st["final_pos_err"], st["final_ori_err"]) == (20 / 120, 25 / 120, 1.5 / 120, 1 / 120)


def test_the_statement_forms_the_steps_arcsine():
    """step_asin is tf_asin of csrc/tf_device_math.h: exact at the ends, within 4 ulp of the float64 arcsine inside (the polynomial's own error), and the
    single-rounding fma it is built on agrees with an fma formed in exact rational arithmetic"""
    from fractions import Fraction
    x = torch.tensor([0.0, 1.0, 0.5, 2.0, float("inf"), float("nan")])
    got = ev.step_asin(x)
    half_pi = torch.tensor(math.pi / 2).float()
    assert got[0] == 0 and bool((got[1] == half_pi) & (got[3] == half_pi) & (got[4] == half_pi) & (got[5] == half_pi))
    g = torch.Generator().manual_seed(0)
    x = torch.rand(20000, generator=g)
    err = (ev.step_asin(x).double() - torch.asin(x.double())).abs()
    assert float((err / torch.asin(x.double()).clamp_min(1e-30)).max()) < 4 * 2.0 ** -23
    a, b, c = (torch.randn(300, generator=g) for _ in range(3))
    c = -(a * b) + c * 1e-7                                               # heavy cancellation: where a double rounding would show
    got = ev._fma32(a, b, c)
    for x, y, z, r in zip(a.tolist(), b.tolist(), c.tolist(), got.tolist()):
        exact = Fraction(x) * Fraction(y) + Fraction(z)
        near = np.float32(float(exact))                                   # float(Fraction) and float32(double) both round to nearest: check r against its neighbours
        cands = [np.nextafter(near, np.float32(-np.inf)), near, np.nextafter(near, np.float32(np.inf))]
        best = min(cands, key=lambda q: abs(Fraction(float(q)) - exact))
        assert abs(Fraction(r) - exact) == abs(Fraction(float(best)) - exact), (x, y, z, r)


# ---- the binding ------------------------------------------------------------------------------------------------------------------------------
def test_library_binding_and_refusals():
    """the new header's one name is exported and bound, the old header keeps its names, and bad arguments are refused before any launch: no GPU needed"""
    import ctypes as C
    import re
    from leibnizgym_amd import ppo_kernels as pk
    inc = os.path.join(os.path.dirname(pk.library_path()), "..", "..", "include")
    strip = lambda name: re.sub(r"/\*.*?\*/", "", open(os.path.join(inc, name)).read(), flags=re.S)      # noqa: E731
    src = strip("trifinger_ppo_track.h")
    assert sorted(set(re.findall(r"\b(tfp_[a-z0-9_]+)\s*\(", src))) == ["tfp_rollout_track"]
    assert len(set(re.findall(r"\b(tfp_[a-z0-9_]+)\s*\(", strip("trifinger_ppo.h")))) == 22
    lib = pk.load()
    assert lib.tfp_api_version() == 3
    assert lib.tfp_rollout_track.restype is C.c_int and lib.tfp_rollout_track.argtypes == [C.c_void_p, C.c_void_p]
    assert "TFP_TRACK_ACC = 11" in src and (ev.TRACK_ACC, pk.TRACK_ACC, pk.TRACK_ENV_ROWS, ev.TRK_ROWS) == (11, 11, 2, 2)
    order = re.findall(r"TFP_TRACK_([A-Z_]+) = (\d+)", src)
    assert [(k, int(v)) for k, v in order if k not in ("ENV_RETURN", "ENV_ARMED", "ENV_ROWS")] == [
        ("EPISODES", 0), ("SUCCESS", 1), ("POS_OK", 2), ("ORI_OK", 3), ("TIMEOUT", 4), ("SUM_LENGTH", 5), ("SUM_RETURN", 6), ("SUM_POS_ERR", 7),
        ("SUM_ORI_ERR", 8), ("NONFINITE", 9), ("UNARMED", 10), ("ACC", 11)]
    assert (ev.T_EPISODES, ev.T_SUCCESS, ev.T_POS_OK, ev.T_ORI_OK, ev.T_TIMEOUT, ev.T_SUM_LENGTH, ev.T_SUM_RETURN, ev.T_SUM_POS_ERR, ev.T_SUM_ORI_ERR,
            ev.T_NONFINITE, ev.T_UNARMED) == tuple(range(11))
    p = 4096                                              # never dereferenced: every call below is refused on the host
    ptrs_a = ("state", "reward", "reset_buf", "steps", "b_rew", "env_trk", "acc", "done_bytes", "b_done")
    ptrs_b = ("state", "reward", "reset_buf", "steps", "b_rew", "env_trk", "acc", "b_end", "b_tout")

    def args(ptrs, **kw):
        a = pk.TfpTrackArgs()
        for k in ptrs:
            setattr(a, k, p)
        a.N, a.rule, a.pos_tol, a.ori_tol, a.scale, a.episode_length = 4, 1, 0.02, 0.2, 0.01, 6
        for k, v in kw.items():
            setattr(a, k, v)
        return C.byref(a)
    assert lib.tfp_rollout_track(None, None) == -1
    for ptrs in (ptrs_a, ptrs_b):
        for k in ptrs:
            if k == "done_bytes":                         # without it the call is mode B, which then misses b_end and b_tout
                assert lib.tfp_rollout_track(args([q for q in ptrs if q != k]), None) == -1
            else:
                assert lib.tfp_rollout_track(args(ptrs, **{k: None}), None) == -1, k
        for bad in (dict(N=0), dict(N=-1), dict(N=2097153), dict(rule=-1), dict(rule=3), dict(pos_tol=float("nan")), dict(ori_tol=float("nan"))):
            assert lib.tfp_rollout_track(args(ptrs, **bad), None) == -1, bad
    eng = tu.fake_engine(4, "cpu")
    with pytest.raises(ValueError, match="CPU"):
        EpisodeTracker(eng, 0.02, 0.2, rule=1, fused=True)
    with pytest.raises(ValueError, match="step_fused"):
        EpisodeTracker(eng, 0.02, 0.2, rule=1).step_fused(1.0, torch.zeros(4))
    with pytest.raises(ValueError):
        EpisodeTracker(eng, 0.02, 0.2, rule=3)
    with pytest.raises(ValueError, match="pos_tol"):
        EpisodeTracker(eng)                               # an engine without a config needs the tolerances


# ---- the keys ---------------------------------------------------------------------------------------------------------------------------------
def test_from_rlg_reads_the_keys():
    c = PPOConfig.from_rlg(RLG_ASYMM, num_envs=64)
    conf = RLG_ASYMM["params"]["config"]
    assert "track_episodes" not in conf and c.track_episodes is False and PPOConfig().track_episodes is False       # the default tree does not change
    assert c.games_to_track == int(conf.get("games_to_track", 100)) and c.score_to_win == float(conf.get("score_to_win", math.inf))
    assert PPOConfig().games_to_track == 100 and PPOConfig().score_to_win == math.inf
    tree = copy.deepcopy(RLG_ASYMM)
    tree["params"]["config"].update(track_episodes=True, games_to_track=7, score_to_win=123.5)
    c = PPOConfig.from_rlg(tree, num_envs=64)
    assert (c.track_episodes, c.games_to_track, c.score_to_win) == (True, 7, 123.5)
    for k in ("track_episodes", "games_to_track", "score_to_win"):
        tree["params"]["config"].pop(k, None)
    c = PPOConfig.from_rlg(tree, num_envs=64)
    assert (c.track_episodes, c.games_to_track, c.score_to_win) == (False, 100, math.inf)


# ---- the engine's step counter ----------------------------------------------------------------------------------------------------------------
def trainer(oracle, n=N, episode_length=EP_LEN, horizon=T, **kw):
    from leibnizgym_amd.config import gym_config
    from leibnizgym_amd.envs import TrifingerEnv
    from leibnizgym_amd.utils.rlg_train import RlGamesGpuEnvAdapter
    from leibnizgym_amd.wrappers import VecTaskPython
    cfg = gym_config("trifinger_difficulty_4")
    cfg.update(num_instances=n, seed=1, physics_engine="physx", asymmetric_obs=True, episode_length=episode_length)
    env = TrifingerEnv(config=cfg, device="cpu", verbose=False, lib=oracle)
    ad = RlGamesGpuEnvAdapter("rlgpu", n, env=VecTaskPython(env, rl_device="cpu"))
    return PPOTrainer(ad, 41, 113, 9, PPOConfig(horizon=horizon, minibatches=4, mini_epochs=2, **kw), device="cpu"), env


def test_steps_is_one_in_the_first_step_of_an_episode(oracle):
    """after tf_reset and after a reset inside a step alike: s == 1 marks the first step, s == episode_length the step in which reset_buf is set"""
    tr, env = trainer(oracle, n=4)
    eng = env._engine
    assert int(eng.steps.abs().sum()) == 0                                # the trainer's constructor reset the env
    for t in range(2 * EP_LEN + 2):
        tr.env.step(torch.zeros(4, 9))
        assert eng.steps.tolist() == [t % EP_LEN + 1] * 4 and eng.reset_buf.tolist() == [t % EP_LEN + 1 == EP_LEN] * 4


# ---- the trainer on the oracle env ------------------------------------------------------------------------------------------------------------
def record_steps(tr, eng):
    seen, step = [], tr.env.step

    def wrapped(a):
        out = step(a)
        seen.append(dict(state=eng.state.clone(), reward=eng.reward.clone(), reset_buf=eng.reset_buf.clone(), steps=eng.steps.clone()))
        return out
    tr.env.step = wrapped
    return seen


def recompute(seen, n, ep_len):
    """the accumulator from per-step clones: the counters, SUM_LENGTH and SUM_RETURN from reward / reset_buf / steps alone (a loop per env), the error sums and
    predicates from the state clone of the ending step"""
    acc = [0] * ev.TRACK_ACC
    ret, armed = np.zeros(n, np.float32), np.zeros(n, bool)
    for rec in seen:
        r, rb, s = rec["reward"].numpy(), rec["reset_buf"].numpy(), rec["steps"].numpy()
        e_p, e_o, qfin = ev.step_errors(rec["state"])
        for i in range(n):
            ret[i], armed[i] = (r[i], True) if s[i] == 1 else (np.float32(ret[i] + r[i]), armed[i])
            if rb[i]:
                if armed[i] and np.isfinite(ret[i]) and bool(qfin[i]):
                    pos_ok, ori_ok = bool(e_p[i] <= 0.02), bool(e_o[i] <= np.float32(0.25))
                    for k, x in ((ev.T_EPISODES, 1), (ev.T_SUCCESS, pos_ok and ori_ok), (ev.T_POS_OK, pos_ok), (ev.T_ORI_OK, ori_ok), (ev.T_TIMEOUT, s[i] >= ep_len),
                                 (ev.T_SUM_LENGTH, int(s[i])), (ev.T_SUM_RETURN, round(float(ret[i]) * 2 ** 16)), (ev.T_SUM_POS_ERR, round(float(e_p[i]) * 2 ** 30)),
                                 (ev.T_SUM_ORI_ERR, round(float(e_o[i]) * 2 ** 28))):
                        acc[k] += int(x)
                elif armed[i]:
                    acc[ev.T_NONFINITE] += 1
                else:
                    acc[ev.T_UNARMED] += 1
                ret[i], armed[i] = 0.0, False
    return acc


def test_trainer_reports_what_the_buffers_hold(oracle):
    tr, env = trainer(oracle, track_episodes=True, games_to_track=10 ** 6)
    eng = env._engine
    assert tr.tracker is not None and tr.tracker.engine is eng and not tr.tracker.fused and tr.tracker.ep_len == EP_LEN
    assert (tr.tracker.pos_tol, tr.tracker.ori_tol, tr.tracker.rule) == (pytest.approx(0.02), pytest.approx(0.25), 1)
    seen = record_steps(tr, eng)
    st = tr.update(tr.rollout())
    assert set(st) == PARENT_KEYS | COUNT_KEYS and st["episodes"] == 0 and st["episodes_total"] == 0            # four steps: no episode has ended, no mean key
    stats = [st] + [tr.update(tr.rollout()) for _ in range(5)]                                                 # 24 steps: four ends per env
    want = recompute(seen, N, EP_LEN)
    assert want[ev.T_EPISODES] + want[ev.T_NONFINITE] == 4 * N and want[ev.T_UNARMED] == 0 and want[ev.T_TIMEOUT] == want[ev.T_EPISODES] > 0
    st = stats[-1]
    assert set(st) == PARENT_KEYS | COUNT_KEYS | MEAN_KEYS
    got = [sum(v[k] for v in tr.track_window) for k in range(ev.TRACK_ACC)]
    assert got == want                                                   # games_to_track is out of reach: the window is every epoch with an end
    n = want[ev.T_EPISODES]
    assert (st["episodes"], st["episodes_total"], st["episodes_nonfinite"], st["episodes_unarmed"]) == (n, n, want[ev.T_NONFINITE], 0)
    assert st["episode_return"] == want[ev.T_SUM_RETURN] / 2 ** 16 / n and st["episode_length"] == EP_LEN == want[ev.T_SUM_LENGTH] / n
    assert st["success_rate"] == want[ev.T_SUCCESS] / n and st["pos_ok_rate"] == want[ev.T_POS_OK] / n and st["ori_ok_rate"] == want[ev.T_ORI_OK] / n
    assert st["timeout_rate"] == 1.0 and st["final_pos_err"] == want[ev.T_SUM_POS_ERR] / 2 ** 30 / n and st["final_ori_err"] == want[ev.T_SUM_ORI_ERR] / 2 ** 28 / n
    # the return of an episode is the sum of its raw rewards: per step it is mean_reward's unit, over EP_LEN steps
    per_step = torch.stack([r["reward"] for r in seen]).double().mean()
    assert st["episode_return"] == pytest.approx(float(per_step) * EP_LEN, rel=1e-4)
    assert all("episode_return" in s for s in stats[1:]) and [s["episodes_total"] for s in stats] == [0, N, 2 * N, 2 * N, 3 * N, 4 * N]
    # evaluate() resets the envs underneath the tracker: the partial episodes are discarded
    tr.rollout()
    assert int(tr.tracker.env_trk[ev.TRK_ARMED].sum()) == N
    tr.evaluate(max_steps=2)
    assert int(tr.tracker.env_trk.abs().sum()) == 0
    assert tr.update(tr.rollout())["episodes_unarmed"] == 0              # every env re-armed at its first step after the reset


def test_the_default_window_is_the_last_epoch_with_ends(oracle):
    tr, _ = trainer(oracle, n=8, track_episodes=True, games_to_track=8)
    stats = tr.train(6)
    assert [s["episodes"] for s in stats] == [0, 8, 8, 8, 8, 8] and [s["episodes_total"] for s in stats] == [0, 8, 16, 16, 24, 32]
    assert len(tr.track_window) == 1 and stats[3]["episode_return"] == stats[2]["episode_return"]              # epoch 3 ends nothing: the window stays
    tr2, _ = trainer(oracle, n=8, track_episodes=True, games_to_track=9)
    assert [s["episodes"] for s in tr2.train(6)] == [0, 8, 16, 16, 16, 16]


def test_parameters_do_not_depend_on_the_key(oracle):
    on, _ = trainer(oracle, track_episodes=True)
    off, _ = trainer(oracle)
    assert off.tracker is None and off.track_window == [] and "track" not in off.state_dict()
    def run(tr):                                                         # the same exploration noise and minibatch order for both
        torch.manual_seed(11)
        return tr.train(3)
    s_on, s_off = run(on), run(off)
    assert all(torch.equal(a, b) for a, b in zip(on.net.parameters(), off.net.parameters()))
    for a, b in zip(s_on, s_off):
        assert set(b) == PARENT_KEYS | {"epoch", "frames"} and all(a[k] == b[k] for k in b)
    assert set(off.update(off.rollout())) == PARENT_KEYS
    ends, _ = trainer(oracle, track_episodes=True, episode_ends=True, value_bootstrap=True)
    ends_off, _ = trainer(oracle, episode_ends=True, value_bootstrap=True)
    a, b = run(ends), run(ends_off)
    assert all(torch.equal(p, q) for p, q in zip(ends.net.parameters(), ends_off.net.parameters()))
    assert a[-1]["episodes_total"] == 2 * N == sum(s["episodes_ended"] for s in a) and set(b[-1]) == PARENT_KEYS | {"epoch", "frames", "episodes_ended"}


def test_an_env_without_a_native_engine_is_refused():
    from minibatch_step_util import StubEnv
    with pytest.raises(ValueError, match="no native engine"):
        PPOTrainer(StubEnv(41, 113, "cpu"), 41, 113, 9, PPOConfig(track_episodes=True), device="cpu")
    PPOTrainer(StubEnv(41, 113, "cpu"), 41, 113, 9, PPOConfig(), device="cpu")        # ... and only with the key on


def test_score_to_win_stops_training(oracle, tmp_path):
    tr, _ = trainer(oracle, n=8, track_episodes=True, score_to_win=-1e9, name="won")
    stats = tr.train(10, checkpoint_dir=str(tmp_path))
    assert len(stats) == 2 and "won" not in stats[0] and stats[1]["won"] is True and stats[1]["episode_return"] > -1e9
    ck = torch.load(str(tmp_path / "won.pth"), weights_only=False)
    assert ck["epoch"] == 2 and ck["track"]["totals"] == [8, 0, 0]
    far, _ = trainer(oracle, n=8, track_episodes=True, score_to_win=1e9)
    assert len(far.train(3)) == 3
    off, _ = trainer(oracle, n=8, score_to_win=-1e9)                      # without tracking there is no episode return to compare
    assert len(off.train(3)) == 3


def test_best_checkpoint_follows_the_episode_return(oracle, tmp_path):
    tr, _ = trainer(oracle, n=8, track_episodes=True, save_best_after=0, name="b", save_frequency=10 ** 6)
    saves, save = [], tr.save

    def spy(path):
        saves.append((os.path.basename(path), tr.epoch, tr.best_reward))
        return save(path)
    tr.save = spy
    stats = tr.train(7, checkpoint_dir=str(tmp_path))
    best, want = -math.inf, []
    for s in stats:                                                       # a strict improvement of episode_return, and only of it
        if "episode_return" in s and s["episode_return"] > best:
            best = s["episode_return"]
            want.append(("b_best.pth", s["epoch"] + 1, best))
    assert want and [x for x in saves if x[0] == "b_best.pth"] == want and tr.best_reward == best
    assert "episode_return" not in stats[0] and all(x[1] >= 2 for x in want)              # no window, no best
    assert best != max(s["mean_reward"] for s in stats)


def test_save_and_restore(oracle, tmp_path):
    tr, _ = trainer(oracle, n=8, track_episodes=True, games_to_track=20, save_best_after=0)
    tr.train(5, checkpoint_dir=str(tmp_path))
    assert len(tr.track_window) == 3 and tr.track_totals == [24, 0, 0] and math.isfinite(tr.best_reward)
    path = tr.save(str(tmp_path / "ck.pth"))
    other, _ = trainer(oracle, n=8, track_episodes=True, games_to_track=20)
    other.rollout()
    assert int(other.tracker.env_trk[ev.TRK_ARMED].sum()) == 8 and int(other.tracker.acc.sum()) == 0
    other.tracker.acc[ev.T_UNARMED] = 5
    other.restore(path)
    assert other.track_window == tr.track_window and other.track_totals == tr.track_totals and other.best_reward == tr.best_reward
    assert int(other.tracker.env_trk.abs().sum()) == 0 and int(other.tracker.acc.abs().sum()) == 0
    st = other.update(other.rollout())
    # the envs are in the middle of episodes the zeroed tracker did not see begin: their end at step 6 is UNARMED; the window came with the checkpoint
    assert st["episodes_unarmed"] == 8 and st["episodes_total"] == 24 and st["episodes"] == 24 and "episode_return" in st
    # a checkpoint written without tracking: an empty window, and the best so far starts again (a reward per step is another unit)
    plain, _ = trainer(oracle, n=8, save_best_after=0)
    plain.train(1, checkpoint_dir=str(tmp_path / "plain"))
    assert math.isfinite(plain.best_reward)
    other.restore(plain.save(str(tmp_path / "plain.pth")))
    assert other.track_window == [] and other.track_totals == [0, 0, 0] and other.best_reward == -math.inf
    plain.restore(path)                                                   # and the other way round
    assert plain.best_reward == -math.inf and plain.tracker is None


# ---- the log ----------------------------------------------------------------------------------------------------------------------------------
def test_log_tags_and_line():
    from leibnizgym_amd.utils.rlg_train import episode_line, episode_scalars
    st = dict(frames=1000, epoch=3, episodes=0, mean_reward=0.1)
    assert episode_scalars(st, 2.0) == [] and episode_line(st) == ""
    st.update(episodes=12, episode_return=-3.5, episode_length=6.0, success_rate=0.25, timeout_rate=1.0, final_pos_err=0.05, final_ori_err=1.5)
    tags = episode_scalars(st, 2.0)
    assert [t[0] for t in tags] == ["rewards/frame", "rewards/iter", "rewards/time", "episode_lengths/frame", "episode_lengths/iter", "episode_lengths/time",
                                    "info/success_rate", "info/timeout_rate", "info/final_pos_err", "info/final_ori_err"]
    assert tags[0][1:] == (-3.5, 1000) and tags[1][1:] == (-3.5, 3) and tags[2][1:] == (-3.5, 2.0) and tags[4][1:] == (6.0, 3) and tags[6][1:] == (0.25, 1000)
    line = episode_line(st)
    assert "-3.500" in line and "6.0" in line and "0.250" in line and "12 episodes" in line


# ---- two ranks --------------------------------------------------------------------------------------------------------------------------------
def _rank(rank, world, port, out_dir):
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
    from oracle_util import load_oracle
    import test_track_episodes as me
    torch.set_num_threads(1)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    seen = []
    for name in ("all_reduce", "all_gather", "all_gather_into_tensor", "broadcast", "reduce", "reduce_scatter", "barrier", "all_to_all", "gather", "scatter"):
        def wrapped(*a, _f=getattr(dist, name), _n=name, **k):
            seen.append((_n, str(a[0].dtype) if a and torch.is_tensor(a[0]) else ""))
            return _f(*a, **k)
        setattr(dist, name, wrapped)
    tr, _ = me.trainer(load_oracle(), n=8, track_episodes=True, score_to_win=float(os.environ["TRACK_TEST_SCORE"]), games_to_track=16)
    local = []
    take = tr.tracker.merge

    def merge(group=None):
        local.append(tr.tracker.acc.clone())
        return take(group)
    tr.tracker.merge = merge
    del seen[:]                                                           # the constructor's broadcasts
    stats = tr.train(8)
    np.savez(os.path.join(out_dir, f"rank{rank}.npz"), window=np.array(tr.track_window), totals=np.array(tr.track_totals), epochs=len(stats),
             won=np.array([bool(s.get("won")) for s in stats]), ret=np.array([s.get("episode_return", np.nan) for s in stats]),
             n_track=tr.n_track_allreduce, n_int64=sum(1 for n, d in seen if n == "all_reduce" and d == "torch.int64"), n_coll=len(seen),
             n_other=tr.n_grad_allreduce + tr.n_kl_allreduce + tr.n_norm_allgather, local=torch.stack(local).numpy())
    dist.destroy_process_group()


def test_two_ranks_report_one_window_and_stop_together(oracle, tmp_path):
    # first without a reachable score: 8 epochs, the returns every rank reports
    def run(score, sub):
        os.makedirs(tmp_path / sub)
        os.environ["TRACK_TEST_SCORE"] = repr(score)
        with socket.socket() as s:
            s.bind(("127.0.0.1", 0))
            port = s.getsockname()[1]
        mp.spawn(_rank, args=(2, port, str(tmp_path / sub)), nprocs=2, join=True)
        return [np.load(os.path.join(tmp_path, sub, f"rank{r}.npz")) for r in range(2)]
    a, b = run(math.inf, "far")
    assert int(a["epochs"]) == int(b["epochs"]) == 8 and not a["won"].any()
    assert np.array_equal(a["window"], b["window"]) and np.array_equal(a["totals"], b["totals"]) and np.array_equal(a["ret"], b["ret"], equal_nan=True)
    assert a["totals"].tolist() == [5 * 16, 0, 0] and a["window"][:, ev.T_EPISODES].tolist() == [16]            # 32 steps: five ends, 16 envs in all
    for p in (a, b):                                                      # one all-reduce per epoch, an int64 one, and nothing else that is new
        assert int(p["n_track"]) == 8 == int(p["n_int64"]) and int(p["n_coll"]) == int(p["n_other"]) + 8
    assert not np.array_equal(a["local"], b["local"]) and a["local"][:, ev.T_EPISODES].sum() == b["local"][:, ev.T_EPISODES].sum() == 5 * 8
    # then a score between the returns of two epochs: both ranks stop in the epoch that first exceeds it
    rets = a["ret"][~np.isnan(a["ret"])]
    first = float(rets[0])
    above = [k for k, r in enumerate(a["ret"]) if not math.isnan(r) and r > first]
    score = first if above else first - 1.0                              # `first` itself is not above `first`: the run goes on to the first larger return
    stop = (above[0] if above else int(np.flatnonzero(~np.isnan(a["ret"]))[0])) + 1
    c, d = run(score, "near")
    assert int(c["epochs"]) == int(d["epochs"]) == stop and bool(c["won"][-1]) and bool(d["won"][-1]) and not c["won"][:-1].any()
    assert np.array_equal(c["window"], d["window"]) and int(c["n_track"]) == int(d["n_track"]) == stop
