"""The episode flight recorder on the GPU: the kernel of csrc/tf_eval.hip (include/trifinger_ppo_record.h: k_record_step) against the plain-torch statement
on the same device buffers, bit for bit after every update - synthetic buffers under a scripted pattern, then a real HIP engine beside EpisodeStats - and
the replay of a captured episode through the renderer against the live pictures.  Every comparison is exact.  The CPU side of the same definitions is
tests/test_episode_recorder.py."""
import pytest
import torch

import parity_util as pu
from leibnizgym_amd import _capi as capi
from leibnizgym_amd import evaluate as ev
from leibnizgym_amd import record as rc
from leibnizgym_amd.record import EpisodeRecorder
from test_episode_recorder import POS_TOL, ORI_TOL, bits, fake_engine, synthetic_state

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
UPDATES, BURST, NAN_AT, TAKES = 25, 12, 7, (10, 18)


def same(a, b, what):
    for k in ("ring", "hdr", "env_rec", "acc"):
        x, y = getattr(a, k), getattr(b, k)
        assert torch.equal(x if x.dtype == torch.int64 else bits(x), y if y.dtype == torch.int64 else bits(y)), (what, k)


def same_episodes(a, b, what):
    assert len(a) == len(b), what
    for x, y in zip(a, b):
        assert (x["env"], x["length"], x["count"], x["outcome_bits"]) == (y["env"], y["length"], y["count"], y["outcome_bits"]), what
        assert torch.equal(bits(x["records"]), bits(y["records"])) and torch.equal(bits(x["dr"]), bits(y["dr"])) and torch.equal(x["steps"], y["steps"]), what


@pytest.mark.parametrize("every", [1, 3])
@pytest.mark.parametrize("n", [1, 65, 257])
def test_kernel_against_the_statement(hip, n, every):
    """5: 25 updates of synthetic device buffers.  Env i runs episodes of 3 + i % 4 steps and enters i % 5 steps into one, so the lanes of a wavefront hold
    different slots and some are first seen in the middle of an episode; at update 12 every env ends in one launch (the burst); at update 7 env n // 2 ends
    with a NaN in a cube row.  For each `select` and W in {N, N - 1} a fused recorder and one on the torch statement see the same inputs: ring, hdr,
    env_rec and acc are equal bit for bit after EVERY update, and so is what take() hands out at updates 10 and 18 (which lets the frozen envs run on)."""
    fake = fake_engine(n, DEV)
    pairs = []
    for select in ("failure", "success", "nonfinite"):
        for w in sorted({n, max(1, n - 1)}):
            kw = dict(select=select, every=every, length=3, watch=w, pos_tol=POS_TOL, ori_tol=ORI_TOL, rule=1, episode_length=5)
            pairs.append((f"select={select} W={w}", EpisodeRecorder(fake, fused=True, **kw), EpisodeRecorder(fake, fused=False, **kw)))
    assert all(k.fused and not t.fused for _, k, t in pairs)
    i = torch.arange(n)
    period, s = 3 + i % 4, i % 5
    harvested = {what: 0 for what, _, _ in pairs}
    for t in range(UPDATES):
        s = s + 1
        rb = (s >= period) | (t == BURST)
        st = synthetic_state(n, 100 * n + t)
        if t == NAN_AT:
            st[capi.S_CUBE_P + 1, n // 2] = float("nan")
            rb[n // 2] = True
        fake.state.copy_(st); fake.reward.copy_(torch.randn(n, generator=torch.Generator().manual_seed(t)) * 30.0)
        fake.steps.copy_(s); fake.reset_buf.copy_(rb)
        for what, k, tor in pairs:
            k.update(); tor.update()
            same(k, tor, f"{what}, update {t}")
            if t in TAKES:
                a, b = k.take(), tor.take()
                same_episodes(a, b, f"{what}, take at update {t}")
                same(k, tor, f"{what}, after the take at update {t}")
                harvested[what] += len(a)
        s = torch.where(rb, torch.zeros_like(s), s)
    for what, k, _ in pairs:
        c = k.counts()
        assert c["records"] > 0 and c["ended_armed"] > 0 and (n == 1 or c["unarmed"] > 0), (what, c)
        assert c["frozen"] == harvested[what] + int((k.env_rec[rc.ENV_STATE] == rc.FROZEN_STATE).sum()), (what, c)
    by = {what: k for what, k, _ in pairs}
    assert by[f"select=nonfinite W={n}"].counts()["frozen"] >= 1                       # the NaN lane froze where non-finite ends are selected
    assert by[f"select=failure W={n}"].counts()["frozen"] + by[f"select=success W={n}"].counts()["frozen"] >= min(n, 3)
    if every == 1:
        assert int(by[f"select=nonfinite W={n}"].env_rec[rc.ENV_COUNT].max()) > 3 or n == 1      # a ring of 3 wrapped


def test_entry_point_on_the_device(hip):
    """the binding refuses what the kernel would misread, and a launch with select = 7 on device buffers returns 0"""
    fake = fake_engine(4, DEV)
    rec = EpisodeRecorder(fake, select=7, length=2, pos_tol=POS_TOL, ori_tol=ORI_TOL, rule=1, episode_length=3)
    assert rec.fused
    fake.steps.fill_(1)
    rec.update()
    assert rec.counts() == {"ended_armed": 0, "frozen": 0, "unarmed": 0, "records": 4} and rec.env_rec[rc.ENV_STATE].tolist() == [1] * 4
    for k, bad in (("reward", torch.zeros(4, dtype=torch.float64, device=DEV)), ("reset_buf", torch.zeros(4, dtype=torch.int64, device=DEV)),
                   ("steps", torch.zeros(4, dtype=torch.int32, device=DEV)), ("state", torch.zeros(capi.TF_STATE_ROWS, 4, dtype=torch.float64, device=DEV))):
        good = dict(vars(fake))
        good[k] = bad
        with pytest.raises(ValueError, match=k):
            EpisodeRecorder(type(fake)(**good), length=2, pos_tol=POS_TOL, ori_tol=ORI_TOL, rule=1)


def test_real_engine_beside_episode_stats(hip):
    """6: HIP engine, N = 65, episode_length 5, 16 steps of random actions; a fused recorder that selects everything, the torch statement beside it (equal
    bit for bit after every step) and EpisodeStats: the OUTCOME flags summed over the harvests are the evaluator's counters"""
    from leibnizgym_amd.engine import TrifingerEngine, make_config
    n = 65
    eng = TrifingerEngine(make_config(hip, n, seed=5, episode_length=5, **dict(pu.CONFIGS["d4_torque_asym"])), device=DEV, lib=hip)
    rec, tor, stats = EpisodeRecorder(eng, select=7), EpisodeRecorder(eng, select=7, fused=False), ev.EpisodeStats(eng)
    assert rec.fused and stats.fused and rec.length == 6 and (rec.pos_tol, rec.ori_tol, rec.rule) == (stats.pos_tol, stats.ori_tol, stats.rule)
    eng.reset()
    g = torch.Generator().manual_seed(11)
    eps = []
    for t in range(16):
        if t % 5 == 4:                                   # in front of the ending steps: goals 0 .. 4 cm off the cubes (tolerance 2 cm), orientation the cube's
            off = torch.randn(3, n, generator=g)
            off = off / off.norm(dim=0) * torch.rand(n, generator=g) * 0.04
            eng.goal[0:3] = eng.cube[0:3] + off.to(DEV)
            eng.goal[3:7] = eng.cube[3:7]
        eng.step(pu.actions_for(t, n, eng.action_dim, 5).to(DEV))
        rec.update(); tor.update(); stats.update()
        same(rec, tor, f"step {t}")
        if t % 5 == 4:
            a, b = rec.take(), tor.take()
            same_episodes(a, b, f"take at step {t}")
            eps += a
    eng.close()
    raw = stats.result()["raw"]
    assert len(eps) == 3 * n and all(e["length"] == 5 and e["steps"].tolist() == [1, 2, 3, 4, 5] and e["outcome"]["timeout"] for e in eps)
    fin = [e for e in eps if not e["outcome"]["nonfinite"]]
    assert raw[ev.EPISODES] == len(fin) and raw[ev.NONFINITE] == len(eps) - len(fin)
    assert raw[ev.POS_OK] == sum(e["outcome"]["pos_ok"] for e in fin) and raw[ev.ORI_OK] == sum(e["outcome"]["ori_ok"] for e in fin)
    assert raw[ev.SUCCESS] == sum(e["outcome"]["at_goal"] for e in fin)
    assert 0 < raw[ev.POS_OK] < len(fin)                 # the comparison says something
    assert rec.counts() == {"ended_armed": 3 * n, "frozen": 3 * n, "unarmed": 0, "records": 16 * n}


def test_replay_equals_live(hip, tmp_path):
    """7: 64 x 64 px, N = 4, episode_length 6, pos_tol = -1 (every episode is a failure).  Env 2 is rendered live after every step; the replay of its
    captured episode - time steps as the columns of a state matrix, in chunks of four views - gives the same colour, depth and segmentation, frame for
    frame, and with out_dir one PNG per step"""
    from leibnizgym_amd import render
    from leibnizgym_amd.engine import TrifingerEngine, make_config
    n = 4
    cfg = make_config(hip, n, seed=7, episode_length=6, **dict(pu.CONFIGS["d4_torque_asym"]))
    eng = TrifingerEngine(cfg, device=DEV, lib=hip)
    rec = EpisodeRecorder(eng, select="failure", pos_tol=-1.0)
    live_r = render.SceneRenderer(cfg.model, width=64, height=64, max_views=1, device=DEV)
    live_r.set_views([2], n)
    eng.reset()
    live = []
    for t in range(6):
        eng.step(pu.actions_for(t, n, eng.action_dim, 7).to(DEV))
        rec.update()
        live.append({k: v[0].clone() for k, v in live_r.render(eng.state).items()})
    live_r.close()
    eng.close()
    ep, = [e for e in rec.take() if e["env"] == 2]
    assert ep["steps"].tolist() == [1, 2, 3, 4, 5, 6]
    replay_r = render.SceneRenderer(cfg.model, width=64, height=64, max_views=4, device=DEV)
    color, depth, seg = rc.replay_frames(ep, replay_r, out_dir=str(tmp_path), aux=True)
    only_color = rc.replay_frames(ep, replay_r)
    replay_r.close()
    assert color.shape == (6, 64, 64, 4) and torch.equal(only_color, color)
    for t in range(6):
        assert torch.equal(color[t], live[t]["color"]), t
        assert torch.equal(bits(depth[t]), bits(live[t]["depth"])), t
        assert torch.equal(seg[t], live[t]["segmentation"]), t
    assert len({int(x) for x in seg.unique()}) > 3 and not torch.equal(color[0], color[5])          # a scene, and one that moves
    assert sorted(p.name for p in tmp_path.iterdir()) == [f"ep2_{s:04d}.png" for s in range(1, 7)]

