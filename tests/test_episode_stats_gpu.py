"""Episode statistics on the GPU: the kernel of csrc/tf_eval.hip (include/trifinger_ppo_eval.h) against the plain-torch path on the same device buffers and
the numpy reference (tests/episode_stats_ref.py), its predicates against the step's own pinned counts, PPOTrainer.evaluate / ActorCritic.mean_action on the
hand-written path, and scripts/evaluate_checkpoint.py.  The CPU side of the same definitions is tests/test_episode_stats.py."""
import json
import math
import os
import subprocess
import sys
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import parity_util as pu
from episode_stats_ref import RefStats, compare
from leibnizgym_amd import _capi as capi
from leibnizgym_amd import evaluate as ev
from leibnizgym_amd.evaluate import EpisodeStats

pytestmark = pytest.mark.gpu
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEV = "cuda:0"
POS_TOL, ORI_TOL = 0.02, 0.25


def mid_bin(gen, n, k_lo, k_hi):
    """n values 2^k (1 + j / 4 + 1 / 8) (1 +- 3 %), k in [k_lo, k_hi), j in 0..3: the middle of a histogram bin (four per octave), 9 % off its edges"""
    k = torch.randint(k_lo, k_hi, (n,), generator=gen).double()
    j = torch.randint(0, 4, (n,), generator=gen).double()
    return 2.0 ** k * (1.0 + j / 4 + 0.125) * (1.0 + 0.03 * (2 * torch.rand(n, generator=gen, dtype=torch.float64) - 1))


def synthetic_state(n, seed):
    """[TF_STATE_ROWS, n] float32: cubes at random poses, goals a mid-bin distance (2^-9 .. 0.4 m: values near 0.02 m are 7 % off it) and a mid-bin angle
    (2^-7 .. 2.9 rad: 0.25 rad is a bin edge) away - no sample within 1e-4 of a tolerance or an edge; float64 construction, rounded once"""
    g = torch.Generator().manual_seed(seed)
    st = torch.zeros(capi.TF_STATE_ROWS, n, dtype=torch.float64)
    cp = (torch.rand(3, n, generator=g, dtype=torch.float64) - 0.5) * 0.3
    cq = torch.randn(4, n, generator=g, dtype=torch.float64)
    cq = cq / cq.norm(dim=0)
    d = torch.randn(3, n, generator=g, dtype=torch.float64)
    gp = cp + d / d.norm(dim=0) * mid_bin(g, n, -9, -1)
    ax = torch.randn(3, n, generator=g, dtype=torch.float64)
    ax = ax / ax.norm(dim=0)
    th = mid_bin(g, n, -7, 2)                                         # up to 3.75 rad: what lies above 2.9 rad goes to the middle of the bin [2.5, 3.0)
    th = torch.where(th > 2.9, 2.75 * (1.0 + 0.03 * (2 * torch.rand(n, generator=g, dtype=torch.float64) - 1)), th)
    # The float32 quaternion product carries an ABSOLUTE error of a few 2^-24 whatever the angle, while the bound on the orientation-error sum
    # (episode_stats_ref.compare: episodes + 2^-20 sum|q|) is relative: it presumes a population whose sum is carried by angles of order one.  Every
    # fourth env therefore draws its angle from [1, 2) rad; with N = 1 that is the only env.
    th = torch.where(torch.arange(n) % 4 == 0, mid_bin(g, n, 0, 1), th)
    s, c = torch.sin(th / 2), torch.cos(th / 2)
    x1, y1, z1, w1 = cq
    x2, y2, z2, w2 = -ax[0] * s, -ax[1] * s, -ax[2] * s, c            # goal = cube (x) rot(axis, -theta): the angle between them is theta
    gq = torch.stack([w1 * x2 + x1 * w2 + y1 * z2 - z1 * y2, w1 * y2 - x1 * z2 + y1 * w2 + z1 * x2, w1 * z2 + x1 * y2 - y1 * x2 + z1 * w2,
                      w1 * w2 - x1 * x2 - y1 * y2 - z1 * z2])
    i = torch.arange(n)
    at, far = i % 16 == 1, i % 16 == 9                  # the end bins: a sixteenth of the envs exactly at the goal (bin 0 of both), a sixteenth 1.5 m off it
    gp = torch.where(at, cp, torch.where(far, cp + torch.tensor([[0.9], [-1.2], [0.0]], dtype=torch.float64), gp))
    gq = torch.where(at, cq, gq)
    st[18:21], st[21:25], st[31:34], st[34:38] = cp, cq, gp, gq
    return st.float()


def scattered(n):
    """ending pattern `scattered`: every 37th env, and in the second workgroup (envs 256 .. 511) exactly ONE lane"""
    m = torch.arange(n) % 37 == 3
    m[256:512] = False
    if n > 256:
        m[min(300, n - 1)] = True
    return m


PATTERNS = ("none", "none", "all", "scattered", "none", "all")
GOAL_EVENTS = (False, True, True, False, True, True)      # steps 0 and 3 carry no goal event: on step 0 EVERY workgroup, on step 3 every workgroup without an ending
                                                          # lane leaves at the early exit of k_eval_step; elsewhere 10 % of the lanes report one


def drive(n, seed, cap, nan_lane, repeat=1):
    """6 steps over synthetic buffers: the kernel, the torch path on the same device buffers and the numpy reference; returns their three vectors"""
    fake = SimpleNamespace(state=torch.zeros(capi.TF_STATE_ROWS, n, device=DEV), reward=torch.zeros(n, device=DEV),
                           reset_buf=torch.zeros(n, dtype=torch.bool, device=DEV), goal_reset_buf=torch.zeros(n, dtype=torch.bool, device=DEV),
                           steps=torch.zeros(n, dtype=torch.int64, device=DEV))
    kern = EpisodeStats(fake, POS_TOL, ORI_TOL, max_episodes_per_env=cap, rule=1)
    tor = EpisodeStats(fake, POS_TOL, ORI_TOL, max_episodes_per_env=cap, rule=1, fused=False)
    assert kern.fused and not tor.fused
    outs = []
    for _ in range(repeat):
        kern.reset(); tor.reset()
        ref = RefStats(n, POS_TOL, ORI_TOL, 1, cap=cap)
        g = torch.Generator().manual_seed(seed + 17)
        steps = torch.zeros(n, dtype=torch.int64)
        for t, pat in enumerate(PATTERNS):
            st = synthetic_state(n, seed * 100 + t)
            if nan_lane is not None and t == 2:
                st[18, nan_lane] = float("nan")
            ends = torch.zeros(n, dtype=torch.bool) if pat == "none" else (torch.ones(n, dtype=torch.bool) if pat == "all" else scattered(n))
            steps = steps + 1
            fake.state.copy_(st); fake.reward.copy_(torch.randn(n, generator=g) * 30.0); fake.reset_buf.copy_(ends)
            fake.goal_reset_buf.copy_((torch.rand(n, generator=g) < 0.1) & GOAL_EVENTS[t]); fake.steps.copy_(steps)
            kern.update(); tor.update()
            ref.update(st.numpy(), fake.reward.cpu().numpy(), ends.numpy(), fake.goal_reset_buf.cpu().numpy(), steps.numpy())
            steps = torch.where(ends, torch.zeros_like(steps), steps)
        outs.append((kern.result()["raw"], tor.result()["raw"], ref, kern.env_acc.clone(), tor.env_acc.clone()))
    return outs


@pytest.mark.parametrize("n", [1, 63, 64, 65, 257, 1000, 4097])
def test_kernel_against_the_torch_path_and_the_reference(hip, n):
    """G: synthetic buffers, 6 steps (nobody ends / everybody ends in one launch / scattered endings with a workgroup in which exactly one lane ends), with a
    NaN lane and repeated after reset(); then the same under a cap of one episode per env.  Equalities and tolerances as in test_episode_stats.py (A)."""
    runs = drive(n, seed=n, cap=0, nan_lane=n // 2, repeat=2)
    for k_raw, t_raw, ref, k_env, t_env in runs:
        frac = compare(k_raw, ref, f"kernel, N = {n}")
        compare(t_raw, ref, f"torch path on the device, N = {n}")
        assert frac == 0.0 and ref.near_tol == 0 and k_raw == t_raw     # the whole vector: the torch path forms the errors with step_errors, the kernel's bits
        assert k_raw[ev.NONFINITE] == 1 and k_raw[ev.EPISODES] == 2 * n - 1 + int(scattered(n).sum())
        assert torch.equal(k_env, t_env)                           # per-env state: returns (bits), at-goal steps, first hits, episode counts
    assert runs[0][0] == runs[1][0]                                # reset() and again: the same bits
    (k_raw, t_raw, ref, k_env, t_env), = drive(n, seed=n + 1, cap=1, nan_lane=None)
    compare(k_raw, ref, f"kernel under a cap, N = {n}")
    assert k_raw == t_raw and torch.equal(k_env, t_env)
    assert k_raw[ev.EPISODES] == n and k_raw[ev.ENVS_COMPLETE] == n and k_env[ev.ENV_EPISODES].tolist() == [1] * n


def test_entry_point_refuses_bad_arguments(hip):
    from leibnizgym_amd import ppo_kernels as pk
    lib, p = pk.load(), torch.zeros(capi.TF_STATE_ROWS * 4, device=DEV).data_ptr()
    ok = [p] * 7
    assert lib.tfp_eval_step(*ok, 0, 0.02, 0.2, 1, 0, None) == -1 and lib.tfp_eval_step(*ok, 2097153, 0.02, 0.2, 1, 0, None) == -1
    assert lib.tfp_eval_step(*ok, 4, 0.02, 0.2, 3, 0, None) == -1 and lib.tfp_eval_step(*ok, 4, 0.02, 0.2, -1, 0, None) == -1
    assert lib.tfp_eval_step(*ok, 4, 0.02, 0.2, 1, -1, None) == -1 and lib.tfp_eval_step(*ok, 4, float("nan"), 0.2, 1, 0, None) == -1
    for k in range(7):
        assert lib.tfp_eval_step(*[None if j == k else p for j in range(7)], 4, 0.02, 0.2, 1, 0, None) == -1
    assert lib.tfp_eval_test_predicates(None, 4, 0.02, 0.2, p, None) == -1 and lib.tfp_eval_test_predicates(p, 0, 0.02, 0.2, p, None) == -1
    good = dict(state=torch.zeros(capi.TF_STATE_ROWS, 4, device=DEV), reward=torch.zeros(4, device=DEV), reset_buf=torch.zeros(4, dtype=torch.uint8, device=DEV),
                goal_reset_buf=torch.zeros(4, dtype=torch.bool, device=DEV), steps=torch.zeros(4, dtype=torch.int64, device=DEV))
    assert EpisodeStats(SimpleNamespace(**good), 0.02, 0.2, rule=1).fused
    for k, bad in (("reward", torch.zeros(4, dtype=torch.float64, device=DEV)), ("reset_buf", torch.zeros(4, dtype=torch.int64, device=DEV)),
                   ("goal_reset_buf", torch.zeros(4, dtype=torch.int32, device=DEV)), ("steps", torch.zeros(4, dtype=torch.int32, device=DEV)),
                   ("reward", torch.zeros(5, device=DEV)), ("state", torch.zeros(capi.TF_STATE_ROWS, 4, dtype=torch.float64, device=DEV))):
        with pytest.raises(ValueError, match=k):             # a duck-typed engine whose buffers the kernel would misread
            EpisodeStats(SimpleNamespace(**dict(good, **{k: bad})), 0.02, 0.2, rule=1)
    with pytest.raises(ValueError):
        EpisodeStats(SimpleNamespace(state=torch.zeros(capi.TF_STATE_ROWS, 4), reward=torch.zeros(4), reset_buf=torch.zeros(4, dtype=torch.bool),
                                     goal_reset_buf=torch.zeros(4, dtype=torch.bool), steps=torch.zeros(4, dtype=torch.int64)), 0.02, 0.2, rule=1, fused=True)


def test_predicates_against_the_steps_own_counts(hip):
    """H: HIP env, 1000 envs, difficulty 4, no domain randomisation, 60 steps of random actions, goals planted near the cubes: at every step the number of
    envs with pos_ok / ori_ok from the evaluator's device code equals info[TF_INFO_POS_COUNT] / info[TF_INFO_ORI_COUNT] exactly - the bits the parity
    suite pins.  No sample is kept away from the tolerance here: the two sides must agree on every bit."""
    from leibnizgym_amd import ppo_kernels as pk
    from leibnizgym_amd.engine import TrifingerEngine, make_config
    n = 1000
    eng = TrifingerEngine(make_config(hip, n, seed=5, episode_length=25, **pu.CONFIGS["d4_torque_asym"]), device=DEV, lib=hip)
    pos_tol, ori_tol = float(eng.cfg.position_tolerance), float(eng.cfg.orientation_tolerance)
    eng.reset()
    g = torch.Generator().manual_seed(11)
    got, want, nonfinite = [], [], 0.0
    for t in range(60):
        if t % 5 == 0:                                   # goals a random 0 .. 4 cm and a yaw of 0 .. 0.5 rad off the cubes (tolerances: 2 cm, 0.25 rad)
            cube = eng.cube
            off = torch.randn(3, n, generator=g)
            off = off / off.norm(dim=0) * torch.rand(n, generator=g) * 0.04
            th = torch.rand(n, generator=g) * 0.5
            s, c = torch.sin(th / 2).to(DEV), torch.cos(th / 2).to(DEV)
            x, y, z, w = cube[3:7].clone()
            eng.goal[0:3] = cube[0:3] + off.to(DEV)
            eng.goal[3:7] = torch.stack([x * c + y * s, y * c - x * s, z * c + w * s, w * c - z * s])
        eng.step(pu.actions_for(t, n, eng.action_dim, 5).to(DEV))
        got.append(pk.eval_test_predicates(eng.state, pos_tol, ori_tol).tolist())
        info = eng.info.tolist()
        want.append([int(info[capi.INFO_POS_COUNT]), int(info[capi.INFO_ORI_COUNT])])
        nonfinite += info[capi.INFO_NUM_NONFINITE]
    assert nonfinite == 0
    assert got == want
    pos, ori = [a for a, _ in got], [b for _, b in got]
    assert 100 < max(pos) < n and 100 < max(ori) < n and len(set(pos)) > 5 and len(set(ori)) > 5          # the counts move: the comparison says something


def _trainer(n=256, **kw):
    from leibnizgym_amd.config import gym_config
    from leibnizgym_amd.envs import TrifingerEnv
    from leibnizgym_amd.ppo import PPOConfig, PPOTrainer
    from leibnizgym_amd.utils.rlg_train import RlGamesGpuEnvAdapter
    from leibnizgym_amd.wrappers import VecTaskPython
    cfg = gym_config("trifinger_difficulty_4")
    cfg.update(num_instances=n, seed=1, physics_engine="physx", asymmetric_obs=True, episode_length=20)
    env = TrifingerEnv(config=cfg, device=DEV, verbose=False)
    ad = RlGamesGpuEnvAdapter("rlgpu", n, env=VecTaskPython(env, rl_device=DEV))
    return PPOTrainer(ad, 41, 113, 9, PPOConfig(horizon=8, minibatches=4, mini_epochs=2, **kw), device=DEV), env


@pytest.mark.parametrize("normalize", [False, True], ids=["raw-input", "normalize-input"])
def test_trainer_end_to_end(hip, normalize):
    """I: 256 envs, episode_length 20.  The test drives mean_action -> env.step -> stats.update() for 45 steps and clones the env's buffers after every
    step: the numpy reference on the clones equals the kernel's vector under A's rules.  Then evaluate(episodes_per_env=2): 512 episodes on the walk,
    nothing of the trainer moved, mean_action == dist_and_value's mu bit for bit at M = 256 and M = 65, and training goes on."""
    tr, env = _trainer(normalize_input=normalize, normalize_input_value=normalize)
    assert tr.fused_loss
    if normalize:
        tr.train(1)                                                # records that are not the identity
    eng = ev.engine_of(tr.env)
    assert eng is env._engine
    stats = EpisodeStats(eng)
    assert stats.fused and stats.rule == 1
    ref = RefStats(256, stats.pos_tol, stats.ori_tol, stats.rule)
    clones = []
    with torch.no_grad():
        obs = tr.env.reset()["obs"]
        for t in range(45):
            out = tr.env.step(tr.net.mean_action(obs))[0]
            stats.update()
            obs = out["obs"]
            clones.append([x.clone() for x in (eng.state, eng.reward, eng.reset_buf, eng.goal_reset_buf, eng.steps)])
    for c in clones:
        ref.update(*[x.cpu().numpy() for x in c])
    r = stats.result()
    compare(r["raw"], ref, "end to end")
    assert r["episodes"] + r["nonfinite_episodes"] == 2 * 256 and r["nonfinite_episodes"] == 0
    before = {k: v.clone() for k, v in tr.net.state_dict().items()}
    recs = {k: {a: b.clone() for a, b in rec.state_dict().items()} for k, rec in tr._norm_records().items()}
    frames, epoch = tr.frames, tr.epoch
    r = tr.evaluate(episodes_per_env=2)
    assert r["episodes"] == 512 and r["envs_complete"] == 256 and r["steps"] == 40 and tr.fused_loss and tr.net.actor.mfma
    assert (tr.frames, tr.epoch) == (frames, epoch) and all(torch.equal(v, before[k]) for k, v in tr.net.state_dict().items())
    assert bool(recs) == normalize and all(torch.equal(b, recs[k][a]) for k, rec in tr._norm_records().items() for a, b in rec.state_dict().items())
    assert int(eng.steps.abs().sum()) == 0 and torch.equal(tr.last[0], eng.obs)
    obs, states = tr.last
    with torch.no_grad():
        for m in (256, 65):
            o, s = obs[:m].contiguous(), states[:m].contiguous()
            mu = tr.net.mean_action(o)
            assert mu.shape == (m, 9) and torch.equal(mu, tr.net.dist_and_value(o, s)[0])
            want = torch.nn.Sequential.forward(tr.net.actor, tr.net.obs_norm.normalize(o) if normalize else o)      # the layers as plain torch modules
            torch.testing.assert_close(mu, want, rtol=1e-3, atol=1e-4)
    st = tr.train(1)[-1]
    assert all(math.isfinite(st[k]) for k in ("loss", "kl", "mean_reward"))


def test_evaluate_checkpoint_script(hip, tmp_path):
    """J: scripts/evaluate_checkpoint.py on a checkpoint this test saved (64 envs, episode_length 20, K = 1), in a child process with a time limit: one
    parseable JSON line with episodes == 64"""
    tr, _ = _trainer(n=64)
    path = tr.save(str(tmp_path / "nn" / "trifinger.pth"))
    p = subprocess.run([sys.executable, "scripts/evaluate_checkpoint.py", "gym=trifinger_difficulty_4", f"checkpoint={path}", "num_envs=64",
                        "episodes_per_env=1", "gym.episode_length=20"], cwd=REPO, capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-2000:]
    lines = [ln for ln in p.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1
    r = json.loads(lines[0])
    assert r["episodes"] == 64 and r["num_envs"] == 64 and r["steps"] == 20 and len(r["raw"]) == ev.ACC and r["episode_length_mean"] == 20
