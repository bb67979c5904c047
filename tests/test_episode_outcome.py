"""One statement of the episode outcome: an EpisodeStats, an EpisodeTracker and an EpisodeRecorder that selects every end see the same synthetic buffers
and must agree on every count, and the recorder's frozen final errors are `evaluate.step_errors` bit for bit.  On the CPU the three run the torch statement
(evaluate.episode_outcome); on the GPU each runs its kernel of csrc/tf_eval.hip (episode_outcome there) next to its torch statement on the same device
buffers.  No sample is kept away from a tolerance: the rule is the same code for all three, so they agree on every bit or not at all."""
from types import SimpleNamespace

import pytest
import torch

from leibnizgym_amd import _capi as capi
from leibnizgym_amd import evaluate as ev
from leibnizgym_amd import record as rc
from test_episode_stats_gpu import scattered, synthetic_state

POS_TOL, ORI_TOL = 0.02, 0.25
SIZES = [1, 63, 64, 65, 257]
PATTERNS = ("none", "all", "scattered", "none", "scattered", "all")      # `scattered`: with 257 envs exactly ONE lane of the second workgroup ends
NAN_STEP = 1                                                             # an "all" step: the NaN lane ends there


def bits(x):
    return x.contiguous().view(torch.int32)


def observers(fake, fused):
    kw = dict(pos_tol=POS_TOL, ori_tol=ORI_TOL, rule=1, fused=fused)
    return (ev.EpisodeStats(fake, **kw), ev.EpisodeTracker(fake, episode_length=0, **kw),
            rc.EpisodeRecorder(fake, select="failure|success|nonfinite", length=2, episode_length=0, **kw))


def drive(n, dev, fused_sets):
    """6 steps; every env starts at steps == 1, so the tracker and the recorder are armed from the first launch on.  Returns per set of observers the five
    counts of each of the three - episodes, success, pos_ok, ori_ok, non-finite: the recorder's from the OUTCOME words of its harvest - and the raw
    accumulators; asserts the frozen e_p / e_o words against step_errors on the way"""
    fake = SimpleNamespace(state=torch.zeros(capi.TF_STATE_ROWS, n, device=dev), reward=torch.zeros(n, device=dev),
                           reset_buf=torch.zeros(n, dtype=torch.bool, device=dev), goal_reset_buf=torch.zeros(n, dtype=torch.bool, device=dev),
                           steps=torch.zeros(n, dtype=torch.int64, device=dev))
    sets = [observers(fake, f) for f in fused_sets]
    assert all(o.fused == f for s, f in zip(sets, fused_sets) for o in s)
    words = [[0] * 5 for _ in sets]                                      # the recorders' counts
    g = torch.Generator().manual_seed(n)
    steps = torch.zeros(n, dtype=torch.int64)
    for t, pat in enumerate(PATTERNS):
        st = synthetic_state(n, 1000 * n + t)
        if t == NAN_STEP:
            st[capi.S_CUBE_P, n // 2] = float("nan")
        ends = torch.zeros(n, dtype=torch.bool) if pat == "none" else (torch.ones(n, dtype=torch.bool) if pat == "all" else scattered(n))
        steps = steps + 1
        fake.state.copy_(st); fake.reward.copy_(torch.randn(n, generator=g) * 30.0); fake.reset_buf.copy_(ends); fake.steps.copy_(steps)
        e_p, e_o, _ = ev.step_errors(fake.state)
        for k, (stats, trk, rec) in enumerate(sets):
            stats.update(); trk.update(); rec.update()
            frozen = rec.env_rec[rc.ENV_STATE] == rc.FROZEN_STATE
            assert torch.equal(frozen.cpu(), ends), (t, "every end of an armed env freezes")
            assert torch.equal(rec.env_rec[rc.ENV_E_P][frozen], bits(e_p)[frozen]) and torch.equal(rec.env_rec[rc.ENV_E_O][frozen], bits(e_o)[frozen]), t
            for ep in rec.take():                                        # the harvest re-arms the env at its next first step
                o = ep["outcome"]
                fin = not o["nonfinite"]
                for j, hit in enumerate((fin, fin and o["at_goal"], fin and o["pos_ok"], fin and o["ori_ok"], o["nonfinite"])):
                    words[k][j] += int(hit)
        steps = torch.where(ends, torch.zeros_like(steps), steps)
    out = []
    for (stats, trk, rec), w in zip(sets, words):
        s, a = stats.acc.tolist(), trk.acc.tolist()
        counts = ([s[ev.EPISODES], s[ev.SUCCESS], s[ev.POS_OK], s[ev.ORI_OK], s[ev.NONFINITE]],
                  [a[ev.T_EPISODES], a[ev.T_SUCCESS], a[ev.T_POS_OK], a[ev.T_ORI_OK], a[ev.T_NONFINITE]], w)
        assert a[ev.T_UNARMED] == 0 and rec.counts()["unarmed"] == 0 and rec.counts()["ended_armed"] == sum(w[j] for j in (0, 4))
        out.append((counts, s, a, rec.acc.tolist()))
    return out


def check_counts(counts, n):
    stats, trk, rec = counts
    assert stats == trk == rec, (n, counts)
    ended = 2 * n + 2 * int(scattered(n).sum())
    assert stats[0] + stats[4] == ended and stats[4] == 1, (n, counts)   # every end is counted once, the NaN lane as non-finite
    assert n < 63 or 0 < stats[1] <= min(stats[2], stats[3]) < stats[0]  # rule 1: success needs both predicates, and both outcomes occur


@pytest.mark.parametrize("n", SIZES)
def test_the_three_observers_agree(n):
    (counts, _, _, _), = drive(n, "cpu", [False])
    check_counts(counts, n)


@pytest.mark.gpu
@pytest.mark.parametrize("n", SIZES)
def test_the_three_kernels_agree_with_each_other_and_with_the_statement(hip, n):
    (k_counts, *k_raw), (t_counts, *t_raw) = drive(n, "cuda:0", [True, False])
    check_counts(k_counts, n)
    check_counts(t_counts, n)
    assert k_raw == t_raw                                                # whole accumulators, error sums and histograms included: kernel == torch statement
