"""`diagnostics` of the in-repo PPO on the GPU (include/trifinger_ppo_diag.h): tfp_ppo_loss_diag at the smallest shapes where it can go wrong - a ragged
second block, five blocks and the ticket, A = 18, `old_v` given, weights, a KL row count - against the float64 statement of tests/ppo_diagnostics_util.py and,
for everything that is not the record, against the plain entry point on the same inputs; tfp_clip_adam_diag against tfp_clip_adam and against float64 norms;
the trainer's minibatch step and a trainer on the engine env with the key on."""
import math

import pytest
import torch

import minibatch_step_util as mu
import ppo_diagnostics_util as du
from leibnizgym_amd import ppo
from leibnizgym_amd import ppo_kernels as pk
from leibnizgym_amd.ppo import PPOConfig, PPOTrainer

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def launch(p, diag=None, plain=False):
    """one launch of the objective on the variant's inputs: (loss, d_mu, d_v, d_ls, stats [4]); `plain`: the entry point without KL row count and record"""
    i = {k: (t.to(DEV) if t is not None else None) for k, t in p.inputs.items()}
    stats = torch.zeros(4, device=DEV)
    kw = {}
    if i["old_v"] is not None:
        kw["old_v"] = i["old_v"]
    if i["w"] is not None:
        kw["adv_w"] = torch.stack([i["adv"], i["w"]], dim=1).contiguous()
    if not plain:
        kw.update(kl_rows=p.kl_rows, diag=diag)
    loss, d_mu, d_v, d_ls = pk.ppo_loss_and_grads(i["mu"], i["log_std"], i["v"], i["act"], i["old_nlp"], None if i["w"] is not None else i["adv"], i["ret"],
                                                  i["old_mu"], stats, p.e_clip, p.v_coef, p.ent_coef, p.bounds_coef, **kw)
    torch.cuda.synchronize()
    return loss.clone(), d_mu, d_v, d_ls.clone(), stats


@pytest.mark.parametrize("name", list(du.VARIANTS))
def test_objective_with_the_record(hip, name):
    p = du.planted(name)
    assert (p.B, p.A) == {"cell2": (1100, 9), "cell3": (333, 18)}.get(name, (333, 9))
    rec = pk.new_diag(DEV)
    assert rec.tolist() == ppo.new_diag_record("cpu").tolist()
    want = launch(p, plain=True)
    got = launch(p, diag=rec)
    du.check_record(p, rec, "tfp_ppo_loss_diag")                          # slots 0-5 exactly, 6-8 within the statistics tolerance
    assert rec[9:].tolist() == [0] * 7
    st = du.torch_statement(p).tolist()                                   # the torch statement: the same integers in slots 0-5
    assert rec.tolist()[:6] == st[:6]
    assert abs(int(rec[ppo.D_K3_SUM]) - st[ppo.D_K3_SUM]) <= du.RTOL * st[ppo.D_K3_SUM] + du.ATOL * 2 ** 28 * st[0]
    # what is not the record: d_mu and d_v bit for bit, the sums over the blocks within the tolerances of minibatch_step_util.check
    assert torch.equal(got[1], want[1]) and torch.equal(got[2], want[2])
    assert float((got[3] - want[3]).abs().max()) <= 3e-5 * float(want[3].abs().max()) + 1e-6 and torch.allclose(got[3], want[3], rtol=2e-4, atol=1e-7)
    assert torch.allclose(got[0], want[0], rtol=2e-5, atol=1e-6)
    cols = [0, 1, 2] if p.kl_rows is not None else [0, 1, 2, 3]           # the plain entry point's KL statistic is over every row
    assert torch.allclose(got[4][cols], want[4][cols], rtol=2e-5, atol=1e-6)
    if p.kl_rows is not None:                                             # ... tfp_ppo_loss_sym's is the one the record's launch owes
        i = {k: (t.to(DEV) if t is not None else None) for k, t in p.inputs.items()}
        stats = torch.zeros(4, device=DEV)
        pk.ppo_loss_and_grads(i["mu"], i["log_std"], i["v"], i["act"], i["old_nlp"], i["adv"], i["ret"], i["old_mu"], stats, p.e_clip, p.v_coef, p.ent_coef,
                              p.bounds_coef, kl_rows=p.kl_rows)
        assert torch.allclose(got[4], stats, rtol=2e-5, atol=1e-6)
    # a second launch doubles slots 0-6 and leaves the extremes
    first = rec.tolist()
    again = launch(p, diag=rec)
    assert rec.tolist()[:7] == [2 * x for x in first[:7]] and rec.tolist()[7:] == first[7:]
    du.check_record(p, rec, "two launches", launches=2)
    assert torch.equal(again[1], want[1]) and torch.equal(again[2], want[2])
    # the float accumulators were left clean: the plain entry point gives its usual answer
    after = launch(p, plain=True)
    assert torch.equal(after[1], want[1]) and torch.equal(after[2], want[2])
    assert torch.allclose(after[0], want[0], rtol=2e-5, atol=1e-6) and torch.allclose(after[3], want[3], rtol=2e-4, atol=1e-7)
    assert torch.allclose(after[4], want[4], rtol=2e-5, atol=1e-6)


def test_a_nonfinite_row_counts_in_nonfinite_alone(hip):
    p = du.planted("cell1")
    keep = p.inputs
    bad = dict(keep, old_nlp=keep["old_nlp"].clone())
    bad["old_nlp"][5], bad["old_nlp"][300] = float("nan"), 1000.0         # a NaN log-ratio in the first block; a ratio that overflows in the second
    p2 = du.Planted()
    p2.__dict__.update(p.__dict__)
    p2.inputs = bad
    rec = pk.new_diag(DEV)
    launch(p2, diag=rec)
    st = du.torch_statement(p2).tolist()
    got = rec.tolist()
    assert got[ppo.D_NONFINITE] == 2 == st[ppo.D_NONFINITE] and got[ppo.D_ROWS] == p.B - 2 and got[:6] == st[:6]
    for k in (ppo.D_RATIO_MAX, ppo.D_RATIO_MIN):                          # finite extremes: the two bad rows reached neither (the float32 ratios differ in rounding)
        assert du.bits_float(got[k]) == pytest.approx(du.bits_float(st[k]), rel=du.RTOL)
    assert abs(got[ppo.D_K3_SUM] - st[ppo.D_K3_SUM]) <= du.RTOL * st[ppo.D_K3_SUM] + du.ATOL * 2 ** 28 * st[0]


def adam_pair(n0, n1, grads, max_norms):
    """three steps of tfp_clip_adam and of tfp_clip_adam_diag from the same state; returns both optimisers and the record"""
    def make():
        torch.manual_seed(3)
        g0 = [torch.nn.Parameter(torch.randn(n0, device=DEV))]
        g1 = [torch.nn.Parameter(torch.randn(n1 - n0, device=DEV))] if n1 > n0 else []
        fo = pk.FlatClipAdam(g0, g1, 3e-4, 5e-4, max_norms[0], max_norms[1])
        assert (fo.n0, fo.n1) == (n0, n1)
        return fo
    a, b, rec = make(), make(), pk.new_diag(DEV)
    for g in grads:
        for fo, kw in ((a, {}), (b, {"diag": rec})):
            fo.flat_g.copy_(g)
            fo.step(gathered=True, **kw)
    torch.cuda.synchronize()
    return a, b, rec


def test_optimiser_with_the_record_one_block(hip):
    n = 1000
    gen = torch.Generator().manual_seed(5)
    grads = [torch.randn(n, generator=gen).to(DEV) * s for s in (0.01, 0.1, 1.0)]
    a, b, rec = adam_pair(n, n, grads, (1.0, 1.0))
    for what in ("flat_p", "m", "v", "step_count", "sq"):
        assert torch.equal(getattr(a, what), getattr(b, what)), what
    v = rec.tolist()
    norms = [float(g.double().norm()) for g in grads]
    assert v[ppo.D_STEPS] == 3 and v[ppo.D_TRUNC_A] == sum(x > 1.0 for x in norms) == 2 and v[:8] == [0] * 8 and v[8] == ppo.DIAG_RATIO_MIN_CLEAR
    assert v[ppo.D_TRUNC_V] == v[ppo.D_GN_V_SUM] == v[ppo.D_GN_V_MAX] == 0                       # one group
    assert v[ppo.D_GN_A_SUM] / 2 ** 24 == pytest.approx(sum(norms), rel=2e-5) and du.bits_float(v[ppo.D_GN_A_MAX]) == pytest.approx(max(norms), rel=2e-5)


def test_optimiser_with_the_record_two_groups(hip):
    """n1 = 5000 (five blocks), group norms planted at 0.5 x and 3 x their max_norm, alternating"""
    n0, n1, mx = 3000, 5000, (1.0, 2.0)
    gen = torch.Generator().manual_seed(6)
    plant = [(0.5, 3.0), (3.0, 0.5), (3.0, 3.0)]
    grads = []
    for fa, fv in plant:
        g = torch.randn(n1, generator=gen, dtype=torch.float64)
        g[:n0] *= fa * mx[0] / float(g[:n0].norm())
        g[n0:] *= fv * mx[1] / float(g[n0:].norm())
        grads.append(g.float().to(DEV))
    a, b, rec = adam_pair(n0, n1, grads, mx)
    assert torch.equal(a.step_count, b.step_count)
    for what in ("flat_p", "m", "v"):                                     # five blocks: the squared norms are float atomics in arrival order, in both optimisers
        assert torch.allclose(getattr(a, what), getattr(b, what), rtol=2e-5, atol=2e-7), what
    v = rec.tolist()
    na =[float(g[:n0].double().norm()) for g in grads]
    nv = [float(g[n0:].double().norm()) for g in grads]
    assert v[ppo.D_STEPS] == 3 and v[ppo.D_TRUNC_A] == 2 and v[ppo.D_TRUNC_V] == 2
    for q, norms in enumerate((na, nv)):
        assert v[ppo.D_GN_A_SUM + q] / 2 ** 24 == pytest.approx(sum(norms), rel=2e-5)
        assert du.bits_float(v[ppo.D_GN_A_MAX + q]) == pytest.approx(max(norms), rel=2e-5)
    # the torch statement of the same three steps gives the same counts
    st = ppo.new_diag_record("cpu")
    for x, y in zip(na, nv):
        ppo.diag_merge(st, ppo.diag_optimiser_statement([torch.tensor(x, dtype=torch.float32), torch.tensor(y, dtype=torch.float32)], list(mx)), objective=False)
    assert st.tolist()[9:12] == v[9:12]


@pytest.mark.parametrize("cell", [1, 6])
def test_the_minibatch_step_on_the_kernels_files_the_statement(hip, cell):
    p = du.planted(f"cell{cell}")
    tr = du.make_trainer(cell, DEV, fused=True, diagnostics=True)
    mu.install(p.case, tr)
    assert tr.fused_loss and tr.diag is not None and tr.diag.is_cuda
    d, idx = mu.minibatch(p.case, DEV)
    acc = tr._new_acc(DEV)
    tr._mb_backward(d, p.idx.to(DEV), acc)
    torch.cuda.synchronize()
    du.check_record(p, tr.diag, "trainer, kernels")
    fo = tr.flat_opt
    grads = {n: fo.grad_view(q) for n, q in tr.net.named_parameters()}
    mu.check(p.case, grads, acc["_fused"], "kernels, diagnostics on")
    norms = mu.group_norms(p.case, True)
    tr._mb_apply()
    torch.cuda.synchronize()
    v = tr.diag.tolist()
    assert v[ppo.D_STEPS] == 1 and [v[ppo.D_TRUNC_A], v[ppo.D_TRUNC_V]] == [int(x > 1.0) for x in norms]
    for q in range(2):
        assert v[ppo.D_GN_A_SUM + q] / 2 ** 24 == pytest.approx(norms[q], rel=2e-5) and du.bits_float(v[ppo.D_GN_A_MAX + q]) == pytest.approx(norms[q], rel=2e-5)


N, T, EP_LEN = 64, 4, 6


def hip_trainer(**kw):
    from leibnizgym_amd.config import gym_config
    from leibnizgym_amd.envs import TrifingerEnv
    from leibnizgym_amd.utils.rlg_train import RlGamesGpuEnvAdapter
    from leibnizgym_amd.wrappers import VecTaskPython
    cfg = gym_config("trifinger_difficulty_4")
    cfg.update(num_instances=N, seed=1, physics_engine="physx", asymmetric_obs=True, episode_length=EP_LEN)
    env = TrifingerEnv(config=cfg, device=DEV, verbose=False)
    ad = RlGamesGpuEnvAdapter("rlgpu", N, env=VecTaskPython(env, rl_device=DEV))
    return PPOTrainer(ad, 41, 113, 9, PPOConfig(horizon=T, minibatches=2, mini_epochs=2, **kw), device=DEV)


@pytest.mark.parametrize("keys", [{}, dict(episode_ends=True, clip_value_central=True)], ids=["plain", "episode_ends-clip_value"])
def test_trainer_on_the_engine_env(hip, keys):
    off = hip_trainer(**keys)
    tr = hip_trainer(diagnostics=True, **keys)
    assert tr.fused_loss and off.diag is None
    assert set(off.update(off.rollout())) == {"kl", "loss", "a_loss", "c_loss", "lr", "mean_reward"} | ({"episodes_ended"} if keys else set())
    want = {"clip_frac", "zero_grad_frac", "mu_out_frac", "approx_kl", "ratio_max", "ratio_min", "nonfinite_rows", "grad_norm", "grad_norm_max", "grad_trunc_frac",
            "grad_norm_value", "grad_norm_max_value", "grad_trunc_frac_value", "explained_variance", "entropy", "sigma_mean"} | ({"value_clip_frac"} if keys else set())
    for epoch in range(2):
        buf = tr.rollout()
        live = int(buf["w"].sum()) if tr.ends else T * N
        st = tr.update(buf)
        v = tr.last_diag
        assert want <= set(st) and all(math.isfinite(float(st[k])) for k in want)
        assert tr.diag.tolist() == ppo.new_diag_record("cpu").tolist()                           # taken and cleared
        assert v[ppo.D_STEPS] == 4 and v[ppo.D_NONFINITE] == 0 and v[ppo.D_ROWS] == 2 * live == 4 * (T * N // 2) - 2 * (T * N - live)
        assert all(0.0 <= st[k] <= 1.0 for k in ("clip_frac", "zero_grad_frac", "value_clip_frac", "mu_out_frac", "grad_trunc_frac", "grad_trunc_frac_value") if k in st)
        assert st["zero_grad_frac"] <= st["clip_frac"] and st["approx_kl"] >= -1e-7 and 0 < st["grad_norm"] <= st["grad_norm_max"]
        # the rollout kernel and the objective kernel round nlp differently: the first minibatch's ratios sit within rounding of 1
        assert st["ratio_min"] <= 1 + 1e-5 and st["ratio_max"] >= 1 - 1e-5
    if tr.ends:
        assert live < T * N
