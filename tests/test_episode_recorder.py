"""The episode flight recorder (leibnizgym_amd/record.py, include/trifinger_ppo_record.h) on the CPU: the plain-torch statement over rollouts of the oracle
against a log the test keeps itself, synthetic buffers for arming, re-arming, non-finite ends and `watch`, the header / library / binding with every
refusal of the entry point, and PPOTrainer.evaluate(record=...) with the npz round trip.  Every comparison is exact.  The kernel's side of the same
definitions is tests/test_episode_recorder_gpu.py."""
import ctypes as C
import math
import os
import re
from types import SimpleNamespace

import pytest
import torch

import parity_util as pu
from leibnizgym_amd import _capi as capi
from leibnizgym_amd import evaluate as ev
from leibnizgym_amd import record as rc
from leibnizgym_amd.record import EpisodeRecorder

N, EP_LEN, STEPS = 5, 6, 20
INF = float("inf")


def engine(lib, n=N, episode_length=EP_LEN):
    from leibnizgym_amd.engine import TrifingerEngine, make_config
    return TrifingerEngine(make_config(lib, n, seed=3, episode_length=episode_length, **dict(pu.CONFIGS["d4_torque_asym"])), device="cpu", lib=lib)


def bits(x):
    return x.contiguous().view(torch.int32)


def run(eng, recs, t0, t1, log):
    """steps t0 .. t1 - 1 of the fixed random actions; after every step the test clones what a record is made of into `log`, then the recorders update"""
    for t in range(t0, t1):
        eng.step(pu.actions_for(t, eng.num_envs, eng.action_dim, 3))
        log.append({"rows": eng.state[0:59].clone(), "dr": eng.state[capi.S_DR:capi.S_DR + capi.TF_NUM_DR].clone(), "reward": eng.reward.clone(),
                    "steps": eng.steps.clone(), "reset_buf": eng.reset_buf.clone()})
        for r in recs:
            r.update()


def snapshot(r):
    return [x.clone() for x in (r.ring, r.hdr, r.env_rec)]


@pytest.mark.parametrize("every, length, want_steps", [(1, 8, [1, 2, 3, 4, 5, 6]), (1, 4, [3, 4, 5, 6]), (3, 8, [1, 4, 6])], ids=["no-wrap", "wrap", "every-3"])
def test_statement_against_an_independent_log(oracle, every, length, want_steps):
    """1: N = 5, episode_length 6, 20 steps.  pos_tol = -1 makes every episode a failure: every env freezes at its first time-out, and what take() returns
    equals the test's own log of the engine's buffers; frozen columns do not move under ten further steps; taken envs re-arm at their next s == 1."""
    eng = engine(oracle)
    rec = EpisodeRecorder(eng, select="failure", every=every, length=length, pos_tol=-1.0)
    assert (rec.fused, rec.rule, rec.ep_len, rec.watch) == (False, 1, EP_LEN, N)
    eng.reset()
    log = []
    run(eng, [rec], 0, 6, log)
    assert all(int(e["steps"][0]) == t + 1 for t, e in enumerate(log)) and log[5]["reset_buf"].all() and not log[4]["reset_buf"].any()
    assert rec.env_rec[rc.ENV_STATE].tolist() == [rc.FROZEN_STATE] * N
    assert rec.counts() == {"ended_armed": N, "frozen": N, "unarmed": 0, "records": N * (6 if every == 1 else 3)}
    frozen = snapshot(rec)
    run(eng, [rec], 6, 16, log)
    assert all(torch.equal(bits(a), bits(b)) for a, b in zip(frozen, snapshot(rec)))
    assert rec.counts()["records"] == N * (6 if every == 1 else 3) and rec.counts()["unarmed"] == 0            # a frozen env counts nothing
    eps = rec.take()
    assert [e["env"] for e in eps] == list(range(N))
    for i, e in enumerate(eps):
        assert e["steps"].tolist() == want_steps and e["length"] == 6 and e["count"] == (6 if every == 1 else 3)
        assert e["records"].shape == (len(want_steps), rc.REC_ROWS)
        for k, s in enumerate(want_steps):
            assert torch.equal(bits(e["records"][k, 0:59]), bits(log[s - 1]["rows"][:, i]))
            assert torch.equal(bits(e["records"][k, 59:60]), bits(log[s - 1]["reward"][i:i + 1]))
        ret = torch.zeros((), dtype=torch.float32)
        for s in range(6):                                                  # the float32 sum in step order
            ret = ret + log[s]["reward"][i]
        assert torch.equal(bits(torch.tensor([e["ret"]], dtype=torch.float32)), bits(ret.reshape(1)))
        assert torch.equal(bits(e["dr"]), bits(log[0]["dr"][:, i]))
        assert e["outcome"] == {"at_goal": False, "pos_ok": False, "ori_ok": e["outcome"]["ori_ok"], "timeout": True, "nonfinite": False}
        assert e["e_p"] > 0.0 and 0.0 <= e["e_o"] <= math.pi + 1e-6
    assert rec.take() == [] and rec.env_rec[rc.ENV_STATE].tolist() == [rc.IDLE] * N
    run(eng, [rec], 16, 20, log)                                            # s = 5, 6 (an end nobody saw from its start), 1 (re-arms), 2
    assert [int(log[t]["steps"][0]) for t in (16, 17, 18, 19)] == [5, 6, 1, 2]
    assert rec.env_rec[rc.ENV_STATE].tolist() == [rc.ARMED] * N and rec.env_rec[rc.ENV_COUNT].tolist() == [2 if every == 1 else 1] * N
    assert rec.counts()["unarmed"] == N and rec.counts()["ended_armed"] == N
    assert torch.equal(bits(rec.hdr), bits(log[18]["dr"]))
    rec.reset()
    assert not rec.ring.any() and not rec.env_rec.any() and not rec.acc.any() and not rec.hdr.any()


def test_selection_on_a_real_episode(oracle):
    """1, continued: with infinite tolerances every episode is a success - under select="failure" nothing freezes and ENDED_ARMED counts the three ends
    of every env, under select="success" every env freezes at its first end; with pos_tol = -1 the mirror image"""
    eng = engine(oracle)
    fail_inf = EpisodeRecorder(eng, select="failure", pos_tol=INF, ori_tol=INF)
    succ_inf = EpisodeRecorder(eng, select="success", pos_tol=INF, ori_tol=INF)
    succ_neg = EpisodeRecorder(eng, select="success", pos_tol=-1.0)
    assert fail_inf.length == EP_LEN + 1
    eng.reset()
    run(eng, [fail_inf, succ_inf, succ_neg], 0, STEPS, [])
    assert fail_inf.counts() == {"ended_armed": 3 * N, "frozen": 0, "unarmed": 0, "records": STEPS * N} and fail_inf.take() == []
    assert succ_neg.counts() == fail_inf.counts() and succ_neg.take() == []
    assert succ_inf.counts() == {"ended_armed": N, "frozen": N, "unarmed": 0, "records": 6 * N}
    eps = succ_inf.take(max_episodes=2)
    assert [e["env"] for e in eps] == [0, 1] and all(e["outcome"]["at_goal"] and e["outcome"]["timeout"] and e["length"] == 6 for e in eps)
    assert succ_inf.env_rec[rc.ENV_STATE].tolist() == [0, 0, 2, 2, 2] and [e["env"] for e in succ_inf.take()] == [2, 3, 4]


# ---- 2. synthetic buffers -----------------------------------------------------------------------------------------------------------------------------
SN = 7
POS_TOL, ORI_TOL = 0.02, 0.25


def fake_engine(n=SN, device="cpu"):
    return SimpleNamespace(state=torch.zeros(capi.TF_STATE_ROWS, n, device=device), reward=torch.zeros(n, device=device),
                           reset_buf=torch.zeros(n, dtype=torch.bool, device=device), goal_reset_buf=torch.zeros(n, dtype=torch.bool, device=device),
                           steps=torch.zeros(n, dtype=torch.int64, device=device))


def synthetic_state(n, seed):
    """random rows; unit quaternions; env i % 3 == 0 at its goal, == 1 5 cm and a half turn about z off it, == 2 at the goal's position only"""
    g = torch.Generator().manual_seed(seed)
    st = torch.randn(capi.TF_STATE_ROWS, n, generator=g)
    cq = st[capi.S_CUBE_Q:capi.S_CUBE_Q + 4]
    cq /= cq.norm(dim=0)
    i = torch.arange(n)
    x, y, z, w = cq.clone()
    turned = torch.stack([y, -x, w, -z])                                    # cube_q (x) (0, 0, 1, 0)
    st[capi.S_GOAL_P:capi.S_GOAL_P + 3] = st[capi.S_CUBE_P:capi.S_CUBE_P + 3] + torch.where(i % 3 == 1, 0.05, 0.0)
    st[capi.S_GOAL_Q:capi.S_GOAL_Q + 4] = torch.where(i % 3 == 0, cq, turned)
    return st


# steps and ends of four updates: env 1 is first seen in the middle of an episode, env 2 restarts without an end anybody saw
SCRIPT = [([1, 4, 1, 1, 1, 1, 1], [0, 0, 0, 0, 0, 0, 0]),
          ([2, 5, 2, 2, 2, 2, 2], [0, 0, 0, 0, 0, 0, 0]),
          ([3, 6, 1, 3, 3, 3, 3], [1, 1, 0, 1, 1, 1, 1]),
          ([1, 1, 2, 1, 1, 1, 1], [0, 0, 0, 0, 0, 0, 0])]


def drive(fake, observers, nan_at=None, script=SCRIPT):
    states = []
    for t, (s, rb) in enumerate(script):
        st = synthetic_state(fake.state.shape[1], 10 + t)
        if nan_at is not None and t == nan_at[0]:
            st[capi.S_CUBE_P, nan_at[1]] = float("nan")
        fake.state.copy_(st)
        fake.reward.copy_(torch.arange(len(s), dtype=torch.float32) + 0.25 * (t + 1))
        fake.steps.copy_(torch.tensor(s))
        fake.reset_buf.copy_(torch.tensor(rb, dtype=torch.bool))
        for o in observers:
            o.update()
        states.append(st)
    return states


def test_synthetic_buffers():
    """2: arming, re-arming, a non-finite end, `watch`, and the OUTCOME bits against EpisodeStats on the same buffers"""
    fake = fake_engine()
    kw = dict(pos_tol=POS_TOL, ori_tol=ORI_TOL, rule=1, episode_length=3, length=4)
    recs = {k: EpisodeRecorder(fake, select=k, **kw) for k in ("failure", "success", "nonfinite", "failure|success|nonfinite")}
    watch3 = EpisodeRecorder(fake, select="failure|success|nonfinite", watch=3, **kw)
    assert recs["failure|success|nonfinite"].select == 7 and watch3.ring.shape == (4, rc.REC_ROWS, 3)
    states = drive(fake, list(recs.values()) + [watch3], nan_at=(2, 0))
    for name, r in recs.items():
        st, cnt = r.env_rec[rc.ENV_STATE].tolist(), r.counts()
        assert cnt["unarmed"] == 1 and cnt["ended_armed"] == 5, name      # env 1: seen from s = 4, its end counts in UNARMED; env 2 did not end
        out = r.env_rec[rc.ENV_OUTCOME].tolist()
        assert out[0] & rc.OUT_NONFINITE and not any(o & rc.OUT_NONFINITE for o in out[1:]), name
        assert all(o & rc.OUT_TIMEOUT for k, o in enumerate(out) if k not in (1, 2)) and out[1] == 0 and out[2] == 0
        # envs 3 and 6 are at their goals, 4 is off it, 5 has the position only; 0 is non-finite; 1 was never armed; 2 re-armed at t = 2
        want = {"failure": [0, 1, 1, 0, 2, 2, 0], "success": [0, 1, 1, 2, 0, 0, 2], "nonfinite": [2, 1, 1, 0, 0, 0, 0],
                "failure|success|nonfinite": [2, 1, 1, 2, 2, 2, 2]}[name]
        want = [w if w == 2 or k in (1, 2) else 1 for k, w in enumerate(want)]          # what ended unfrozen re-armed at t = 3 (s == 1); so did env 1
        assert st == want, (name, st)
        assert cnt["frozen"] == st.count(2)
    every = recs["failure|success|nonfinite"]
    assert every.env_rec[rc.ENV_COUNT].tolist() == [3, 1, 2, 3, 3, 3, 3]
    # watch = 3: the buffers are three envs wide and equal the first three columns of the full recorder's
    assert torch.equal(bits(watch3.ring), bits(every.ring[:, :, :3])) and torch.equal(watch3.env_rec, every.env_rec[:, :3])
    assert torch.equal(bits(watch3.hdr), bits(every.hdr[:, :3])) and watch3.counts() == {"ended_armed": 1, "frozen": 1, "unarmed": 1, "records": 3 + 1 + 4}
    eps = {e["env"]: e for e in every.take()}
    assert sorted(eps) == [0, 3, 4, 5, 6]
    assert eps[0]["outcome"]["nonfinite"] and math.isnan(eps[0]["e_p"]) and math.isnan(float(eps[0]["records"][2, capi.S_CUBE_P]))
    assert eps[3]["outcome"] == {"at_goal": True, "pos_ok": True, "ori_ok": True, "timeout": True, "nonfinite": False}
    assert eps[4]["outcome"] == {"at_goal": False, "pos_ok": False, "ori_ok": False, "timeout": True, "nonfinite": False}
    assert eps[5]["outcome"] == {"at_goal": False, "pos_ok": True, "ori_ok": False, "timeout": True, "nonfinite": False}
    for i, e in eps.items():
        assert e["steps"].tolist() == [1, 2, 3] and e["ret"] == 3 * i + 1.5
        assert all(torch.equal(bits(e["records"][k, 0:59]), bits(states[k][0:59, i])) for k in range(3) if not (i == 0 and k == 2))
        assert torch.equal(bits(e["dr"]), bits(states[0][capi.S_DR:capi.S_DR + capi.TF_NUM_DR, i]))
    # env 2 re-armed at t = 2 without a seen end: its header is that step's, its ring starts over
    assert torch.equal(bits(every.hdr[:, 2]), bits(states[2][capi.S_DR:capi.S_DR + capi.TF_NUM_DR, 2]))
    assert torch.equal(bits(every.ring[0, 0:59, 2]), bits(states[2][0:59, 2])) and every.ring[:, rc.REC_STEP, 2].view(torch.int32).tolist()[:2] == [1, 2]


def test_outcome_bits_against_episode_stats():
    """2, last item: every env armed and every end frozen - the OUTCOME flags of the harvest, summed, are what EpisodeStats._update_torch counts on the same
    buffers (POS_OK, ORI_OK and SUCCESS over the finite episodes, NONFINITE)"""
    fake = fake_engine()
    script = [([1] * SN, [0] * SN), ([2] * SN, [0] * SN), ([3] * SN, [1] * SN)]
    rec = EpisodeRecorder(fake, select=7, pos_tol=POS_TOL, ori_tol=ORI_TOL, rule=1, episode_length=3)
    stats = ev.EpisodeStats(fake, POS_TOL, ORI_TOL, rule=1, fused=False)
    drive(fake, [rec, stats], nan_at=(2, 4), script=script)
    eps = rec.take()
    assert len(eps) == SN
    fin = [e for e in eps if not e["outcome"]["nonfinite"]]
    raw = stats.result()["raw"]
    assert raw[ev.EPISODES] == len(fin) == SN - 1 and raw[ev.NONFINITE] == 1
    assert raw[ev.POS_OK] == sum(e["outcome"]["pos_ok"] for e in fin) == 5            # envs 0, 2, 3, 5, 6 hold the position; 1 does not, 4 is the NaN lane
    assert raw[ev.ORI_OK] == sum(e["outcome"]["ori_ok"] for e in fin) == 3
    assert raw[ev.SUCCESS] == sum(e["outcome"]["at_goal"] for e in fin) == 3


# ---- 3. header, library, binding ------------------------------------------------------------------------------------------------------------------------
def test_header_library_and_binding():
    """3: the header's names are exported and bound, its constants are the module's, every refusal returns -1 before any launch (the pointers are never
    dereferenced), and a ring over max_bytes raises"""
    from leibnizgym_amd import ppo_kernels as pk
    src = open(os.path.join(os.path.dirname(pk.library_path()), "..", "..", "include", "trifinger_ppo_record.h")).read()
    code = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    names = sorted(set(re.findall(r"\b(tfp_[a-z0-9_]+)\s*\(", code)))
    assert names == ["tfp_record_step"]
    lib = pk.load()
    assert lib.tfp_record_step.restype is C.c_int and lib.tfp_record_step.argtypes
    fields = [f for chunk in re.findall(r"[^;{}]+;", re.search(r"typedef struct TfpRecordArgs \{(.*?)\} TfpRecordArgs;", code, re.S).group(1))
              for f in re.findall(r"(\w+)\s*[,;]", chunk)]
    assert fields == [f for f, _ in pk.TfpRecordArgs._fields_]
    assert C.sizeof(pk.TfpRecordArgs) == 8 * 8 + 8 + 2 * 4 + 6 * 4
    for k, v in (("TFP_REC_STATE_ROWS 59", rc.REC_STATE_ROWS), ("TFP_REC_ENV_ROWS = 8", rc.ENV_ROWS), ("TFP_REC_ACC = 4", rc.ACC)):
        assert k in code and int(k.split()[-1]) == v
    assert (rc.REC_ROWS, pk.REC_ROWS, pk.REC_ENV_ROWS, pk.REC_ACC) == (61, 61, 8, 4) and capi.S_TAU + 9 == rc.REC_STATE_ROWS == capi.S_PREV_OBJ_P

    def args(**kw):
        a = pk.TfpRecordArgs()
        for f in ("state", "reward", "reset_buf", "steps", "ring", "hdr", "env_rec", "acc"):
            setattr(a, f, 4096)                                             # never dereferenced: every call below is refused on the host
        a.episode_length, a.pos_tol, a.ori_tol, a.N, a.W, a.L, a.every, a.select, a.rule = 6, 0.02, 0.2, 4, 4, 3, 1, 1, 1
        for k, v in kw.items():
            setattr(a, k, v)
        return a
    assert lib.tfp_record_step(None, None) == -1
    for f in ("state", "reward", "reset_buf", "steps", "ring", "hdr", "env_rec", "acc"):
        assert lib.tfp_record_step(C.byref(args(**{f: None})), None) == -1, f
    bad = [dict(N=0), dict(N=2097153, W=1), dict(W=0), dict(W=5), dict(L=0), dict(every=0), dict(select=0), dict(select=8), dict(rule=-1), dict(rule=3),
           dict(episode_length=-1), dict(pos_tol=float("nan")), dict(ori_tol=float("nan"))]
    for kw in bad:
        assert lib.tfp_record_step(C.byref(args(**kw)), None) == -1, kw
    fake = fake_engine()
    with pytest.raises(ValueError, match="max_bytes.*watch.*length|watch.*length.*max_bytes"):
        EpisodeRecorder(fake, pos_tol=POS_TOL, ori_tol=ORI_TOL, rule=1, length=100, max_bytes=4 * 100 * 61 * SN - 1)
    assert EpisodeRecorder(fake, pos_tol=POS_TOL, ori_tol=ORI_TOL, rule=1, length=100, max_bytes=4 * 100 * 61 * SN).ring.numel() == 100 * 61 * SN
    for kw in (dict(select="crash"), dict(select=0), dict(every=0), dict(watch=0), dict(watch=SN + 1), dict(length=0), dict(rule=3), dict(fused=True)):
        with pytest.raises(ValueError):
            EpisodeRecorder(fake, **dict(dict(pos_tol=POS_TOL, ori_tol=ORI_TOL, rule=1, length=4), **kw))
    with pytest.raises(ValueError, match="length"):
        EpisodeRecorder(fake, pos_tol=POS_TOL, ori_tol=ORI_TOL, rule=1)    # no config, no episode length: the ring has no default
    assert rc.parse_select("failure|nonfinite") == 5 and rc.parse_select(" success ") == 2


# ---- 4. trainer integration -------------------------------------------------------------------------------------------------------------------------------
def _trainer(oracle, n=32, episode_length=10):
    from leibnizgym_amd.config import gym_config
    from leibnizgym_amd.envs import TrifingerEnv
    from leibnizgym_amd.ppo import PPOConfig, PPOTrainer
    from leibnizgym_amd.utils.rlg_train import RlGamesGpuEnvAdapter
    from leibnizgym_amd.wrappers import VecTaskPython
    cfg = gym_config("trifinger_difficulty_4")
    cfg.update(num_instances=n, seed=1, physics_engine="physx", asymmetric_obs=True, episode_length=episode_length)
    env = TrifingerEnv(config=cfg, device="cpu", verbose=False, lib=oracle)
    ad = RlGamesGpuEnvAdapter("rlgpu", n, env=VecTaskPython(env, rl_device="cpu"))
    return PPOTrainer(ad, 41, 113, 9, PPOConfig(horizon=8, minibatches=4, mini_epochs=2), device="cpu"), env


def test_trainer_evaluate_with_a_recorder(oracle, tmp_path, monkeypatch):
    """4: without `record` no recorder is constructed and the keys are the parent's; with it episodes_recorded == len(last_recording), and the harvest survives the npz round trip bit for bit"""
    tr, env = _trainer(oracle)
    made = []
    init = EpisodeRecorder.__init__
    monkeypatch.setattr(EpisodeRecorder, "__init__", lambda self, *a, **k: (made.append(1), init(self, *a, **k))[1])
    plain = tr.evaluate(episodes_per_env=1)
    assert made == [] and tr.last_recording is None
    assert set(plain) == set(ev.summarize([0] * ev.ACC)) | {"steps"}
    res = tr.evaluate(episodes_per_env=1, record={"select": "failure"})
    assert made == [1] and set(res) == set(plain) | {"episodes_recorded"}
    assert res["steps"] == plain["steps"] == 10 and res["episodes"] == plain["episodes"] == 32          # (another reset: other episodes than `plain` saw)
    eps = tr.last_recording
    assert res["episodes_recorded"] == len(eps) == res["episodes"] - res["raw"][ev.SUCCESS]
    assert len(eps) > 0 and all(e["length"] == 10 and e["steps"].tolist() == list(range(1, 11)) and not e["outcome"]["at_goal"] for e in eps)
    capped = tr.evaluate(episodes_per_env=1, record={"select": "failure|success", "every": 4, "watch": 8, "max_episodes": 3})
    assert capped["episodes_recorded"] == 3 and [e["env"] for e in tr.last_recording] == [0, 1, 2]
    assert all(e["steps"].tolist() == [1, 5, 9, 10] for e in tr.last_recording)
    with pytest.raises(ValueError, match="unknown"):
        tr.evaluate(record={"selct": "failure"})
    path = str(tmp_path / "rec" / "episodes.npz")
    rc.save_npz(path, eps)
    back = rc.load_npz(path)
    assert len(back) == len(eps)
    for a, b in zip(eps, back):
        assert {k: a[k] for k in ("env", "length", "count", "outcome", "outcome_bits")} == {k: b[k] for k in ("env", "length", "count", "outcome", "outcome_bits")}
        assert all(torch.equal(bits(torch.tensor([a[k]], dtype=torch.float32)), bits(torch.tensor([b[k]], dtype=torch.float32))) for k in ("ret", "e_p", "e_o"))
        assert torch.equal(bits(a["records"]), bits(b["records"])) and torch.equal(bits(a["dr"]), bits(b["dr"])) and torch.equal(a["steps"], b["steps"])
    rc.save_npz(str(tmp_path / "empty.npz"), [])
    assert rc.load_npz(str(tmp_path / "empty.npz")) == []
    state = rc.replay_state(eps[0])
    assert state.shape == (capi.TF_STATE_ROWS, 10) and torch.equal(bits(state[0:59]), bits(eps[0]["records"][:, 0:59].t()))
    assert torch.equal(state[capi.S_DR:capi.S_DR + capi.TF_NUM_DR], eps[0]["dr"].unsqueeze(1).expand(-1, 10)) and not state[59:capi.S_DR].any()
