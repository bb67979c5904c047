"""`track_episodes` on the GPU: the kernel of include/trifinger_ppo_track.h (csrc/tf_eval.hip: k_rollout_track) against the torch statement on the same
device buffers and against the launches it replaces, a burst and quiet steps, and the trainer on the HIP env in both modes.  The CPU side of the same
definitions is tests/test_track_episodes.py."""
import pytest
import torch

import track_episodes_util as tu
from leibnizgym_amd import _capi as capi
from leibnizgym_amd import evaluate as ev
from leibnizgym_amd import ppo_kernels as pk
from leibnizgym_amd.evaluate import EpisodeTracker
from leibnizgym_amd.ppo import PPOConfig, PPOTrainer

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SCALE = 0.01


def trackers(eng, **kw):
    a = EpisodeTracker(eng, tu.POS_TOL, tu.ORI_TOL, rule=tu.RULE, episode_length=tu.EP_LEN, **kw)
    b = EpisodeTracker(eng, tu.POS_TOL, tu.ORI_TOL, rule=tu.RULE, episode_length=tu.EP_LEN, **kw)
    tor = EpisodeTracker(eng, tu.POS_TOL, tu.ORI_TOL, rule=tu.RULE, episode_length=tu.EP_LEN, fused=False)
    assert a.fused and b.fused and not tor.fused
    return a, b, tor


@pytest.mark.parametrize("n", [1, 63, 64, 65, 257])
def test_kernel_against_the_torch_statement_and_the_launches_it_replaces(hip, n):
    """the scripted sequence of tests/track_episodes_util.py (40 steps: counted, unarmed and non-finite ends, episodes of length 1, terminations and
    time-outs): after EVERY step env_trk and acc of mode A, of mode B and of the torch statement are the same bits, mode A's outputs are those of
    tfp_rollout_reward and mode B's those of tfp_rollout_flags; at the end the accumulator is the naive loop's"""
    recs = tu.script(n)
    eng = tu.fake_engine(n, DEV)
    trk_a, trk_b, tor = trackers(eng)
    naive = tu.Naive(n)
    out = torch.empty(10, n, device=DEV)
    for t, rec in enumerate(recs):
        tu.load(eng, rec)
        done = rec["done"].to(DEV)
        out.fill_(-7.0)
        trk_a.step_fused(SCALE, out[0], done=done, done_t=out[1])
        trk_b.step_fused(SCALE, out[2], end_t=out[3], tout_t=out[4])
        pk.rollout_reward(eng.reward, done, SCALE, out[5], out[6])
        pk.rollout_flags(eng.reward, eng.reset_buf, eng.steps, SCALE, tu.EP_LEN, out[7], out[8], out[9])
        tor.update()
        naive.update(rec)
        bits = out.view(torch.int32)
        assert torch.equal(bits[0], bits[5]) and torch.equal(bits[1], bits[6]), t
        assert torch.equal(bits[2], bits[7]) and torch.equal(bits[3], bits[8]) and torch.equal(bits[4], bits[9]), t
        assert torch.equal(out[8], eng.reset_buf.float()) and torch.equal(out[6], done.float())
        for k in (trk_a, trk_b):
            assert torch.equal(k.env_trk, tor.env_trk) and torch.equal(k.acc, tor.acc), (t, k.acc.tolist(), tor.acc.tolist())
    assert trk_a.acc.tolist() == naive.acc and torch.equal(trk_a.env_trk.cpu(), naive.env_trk())
    if n >= 8:
        assert naive.acc[ev.T_EPISODES] > 0 and naive.acc[ev.T_UNARMED] > 0 and naive.acc[ev.T_NONFINITE] > 0
    v = trk_a.take()
    assert v.tolist() == naive.acc and int(trk_a.acc.abs().sum()) == 0


def random_state(n, seed):
    """cubes and goals at random poses a few centimetres and up to a full turn apart: general values for the device functions"""
    g = torch.Generator().manual_seed(seed)
    st = torch.zeros(capi.TF_STATE_ROWS, n)
    cp = (torch.rand(3, n, generator=g) - 0.5) * 0.3
    gp = cp + torch.randn(3, n, generator=g) * torch.rand(1, n, generator=g) * 0.04
    cq, gq = torch.randn(4, n, generator=g), torch.randn(4, n, generator=g)
    near = torch.arange(n) % 3 == 0                                        # a third of the goals within a small turn of the cube
    gq = torch.where(near.unsqueeze(0), cq + 0.05 * gq, gq)
    st[capi.S_CUBE_P:capi.S_CUBE_P + 3], st[capi.S_GOAL_P:capi.S_GOAL_P + 3] = cp, gp
    st[capi.S_CUBE_Q:capi.S_CUBE_Q + 4], st[capi.S_GOAL_Q:capi.S_GOAL_Q + 4] = cq / cq.norm(dim=0), gq / gq.norm(dim=0)
    return st


def test_a_burst_and_quiet_steps(hip):
    """1000 envs at general poses: quiet steps (no workgroup reports: the accumulator does not move), a burst in which EVERY env ends, a step in which one
    lane of one workgroup ends; the kernel's integers are the torch statement's, and a second run gives the same bits"""
    n = 1000
    eng = tu.fake_engine(n, DEV)
    g = torch.Generator().manual_seed(4)
    runs = []
    for _ in range(2):
        g.manual_seed(4)
        trk, _, tor = trackers(eng)
        s = torch.zeros(n, dtype=torch.int64)
        for t in range(12):
            s = s + 1
            ends = torch.ones(n, dtype=torch.bool) if t in (4, 9) else ((torch.arange(n) == 300) if t == 7 else torch.zeros(n, dtype=torch.bool))
            tu.load(eng, dict(state=random_state(n, 50 + t), reward=torch.randn(n, generator=g) * 30.0, reset_buf=ends, steps=s))
            before = trk.acc.clone()
            trk.update()
            tor.update()
            assert torch.equal(trk.acc, tor.acc) and torch.equal(trk.env_trk, tor.env_trk), (t, trk.acc.tolist(), tor.acc.tolist())
            if not bool(ends.any()):
                assert torch.equal(trk.acc, before)
            s = torch.where(ends, torch.zeros_like(s), s)
        runs.append(trk.acc.tolist())
    a = runs[0]
    assert runs[0] == runs[1] and a[ev.T_EPISODES] == 2 * n + 1 and a[ev.T_SUM_LENGTH] == 5 * n + 3 + 5 * (n - 1) + 2 and a[ev.T_UNARMED] == 0 == a[ev.T_NONFINITE]
    assert 0 < a[ev.T_SUCCESS] <= min(a[ev.T_POS_OK], a[ev.T_ORI_OK]) and max(a[ev.T_POS_OK], a[ev.T_ORI_OK]) < a[ev.T_EPISODES] and a[ev.T_TIMEOUT] == 0      # no episode reaches the limit of 10 steps


def test_entry_point_refuses_a_duck_typed_engine_it_would_misread(hip):
    good = vars(tu.fake_engine(4, DEV))
    assert EpisodeTracker(tu.fake_engine(4, DEV), 0.02, 0.2, rule=1).fused
    from types import SimpleNamespace
    for k, bad in (("reward", torch.zeros(4, dtype=torch.float64, device=DEV)), ("reset_buf", torch.zeros(4, dtype=torch.int64, device=DEV)),
                   ("steps", torch.zeros(4, dtype=torch.int32, device=DEV)), ("reward", torch.zeros(5, device=DEV)),
                   ("state", torch.zeros(capi.TF_STATE_ROWS, 4, dtype=torch.float64, device=DEV)), ("steps", torch.zeros(4, dtype=torch.int64))):
        with pytest.raises(ValueError, match=k):
            EpisodeTracker(SimpleNamespace(**dict(good, **{k: bad})), 0.02, 0.2, rule=1)


# ---- the trainer on the HIP env --------------------------------------------------------------------------------------------------------------
N, EP_LEN, T = 128, 6, 4


def hip_trainer(**kw):
    from leibnizgym_amd.config import gym_config
    from leibnizgym_amd.envs import TrifingerEnv
    from leibnizgym_amd.utils.rlg_train import RlGamesGpuEnvAdapter
    from leibnizgym_amd.wrappers import VecTaskPython
    cfg = gym_config("trifinger_difficulty_4")
    cfg.update(num_instances=N, seed=1, physics_engine="physx", asymmetric_obs=True, episode_length=EP_LEN)
    env = TrifingerEnv(config=cfg, device=DEV, verbose=False)
    ad = RlGamesGpuEnvAdapter("rlgpu", N, env=VecTaskPython(env, rl_device=DEV))
    # no gradient-norm truncation: the squared norm is a float sum over workgroups in the order they arrive, the one quantity of a minibatch step whose bits
    # may differ between two runs of the SAME trainer; with it out of the way (coefficient exactly 1) and one workgroup per minibatch of 128 samples in the
    # objective, two runs are comparable bit for bit
    c = PPOConfig(horizon=T, minibatches=4, mini_epochs=2, truncate_grads=False, value_truncate_grads=False, games_to_track=10 ** 6, **kw)
    return PPOTrainer(ad, 41, 113, 9, c, device=DEV), env


@pytest.mark.parametrize("ends", [False, True], ids=["mode-a", "mode-b-episode_ends"])
def test_trainer_on_the_hip_env(hip, monkeypatch, ends):
    """128 envs, episode_length 6, horizon 4: ONE tracking launch per env step where the reward / flags launch stood; the fused tracker's state and
    accumulator are those of a `fused=False` tracker fed the same buffers behind every step; rollout buffers and, after 4 epochs, parameters are the bits
    of a trainer with the key off"""
    calls = []
    for name in ("rollout_track", "rollout_reward", "rollout_flags"):
        monkeypatch.setattr(pk, name, lambda *a, _f=getattr(pk, name), _n=name, **k: (calls.append(_n), _f(*a, **k))[1])
    keys = dict(episode_ends=True, value_bootstrap=True) if ends else {}
    on, env = hip_trainer(track_episodes=True, **keys)
    off, _ = hip_trainer(**keys)
    eng = env._engine
    assert on.fused_loss and on.tracker.fused and on.tracker.engine is eng and off.tracker is None
    ref = EpisodeTracker(eng, fused=False)
    step = on.env.step

    def wrapped(a):
        out = step(a)
        ref.update()
        return out
    on.env.step = wrapped
    stats = []
    for k in range(4):
        torch.manual_seed(100 + k)
        buf = on.rollout()
        assert torch.equal(on.tracker.acc, ref.acc) and torch.equal(on.tracker.env_trk, ref.env_trk), (k, on.tracker.acc.tolist(), ref.acc.tolist())
        torch.manual_seed(100 + k)
        buf_off = off.rollout()
        for name in ("rew", "obs", "act", "val", "adv", "ret") + (("end", "tout", "w") if ends else ("done",)):
            assert torch.equal(buf[name], buf_off[name]), (k, name)
        want = ref.take().tolist()
        torch.manual_seed(200 + k)
        stats.append(on.update(buf))
        torch.manual_seed(200 + k)
        st_off = off.update(buf_off)
        assert all(stats[-1][q] == st_off[q] for q in st_off)
        got = on.track_window[-1] if want[ev.T_EPISODES] else [0] * ev.TRACK_ACC
        assert got == want
    assert calls.count("rollout_track") == 4 * T and calls.count("rollout_reward" if not ends else "rollout_flags") == 4 * T       # the latter: the key-off trainer's
    assert "rollout_flags" not in calls if not ends else "rollout_reward" not in calls
    assert all(torch.equal(a, b) for a, b in zip(on.net.parameters(), off.net.parameters()))
    assert [s["episodes_total"] + s["episodes_nonfinite"] for s in stats] == [0, N, 2 * N, 2 * N] and stats[-1]["episode_length"] == EP_LEN
    assert stats[-1]["timeout_rate"] == 1.0 and stats[-1]["episodes_unarmed"] == 0 and "episode_return" not in stats[0] and "episode_return" in stats[1]
