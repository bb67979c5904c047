"""Planning on the GPU: the kernels of csrc/tf_plan.hip (include/trifinger_plan.h) against the torch statements of leibnizgym_amd/planning.py - the fork bit for
bit on every buffer, a forked HIP engine against its source over 20 steps, the sampled actions against the restatement from the oracle's primitives, the
update against the float64 statement, and one fused plan() against the statement plan() on the same engines."""
import ctypes as C

import numpy as np
import pytest
import torch

import guard_util as gu
import plan_util as pu
from leibnizgym_amd import planning as pl
from leibnizgym_amd.engine import TrifingerEngine, make_config

DEV = "cuda:0"
pytestmark = pytest.mark.gpu


def _stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def _short_source(hip, n, case="torque-asym", steps=6):
    a = pu.fork_engine(hip, DEV, n, 1, 0, case)
    a.reset()
    for t in range(steps):
        a.step(pu.random_actions(t, n, a.action_dim).to(DEV))
    return a


# ---- the fork ------------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_src,n_dst,kind", [(70, 130, "random"), (64, 64, "identity"), (32, 8192, "groups"), (70, 130, "bad")])
def test_fork_kernel_equals_the_statement(hip, n_src, n_dst, kind):
    src = _short_source(hip, n_src)
    idx = {"random": lambda: pu.fork_map(n_dst, n_src), "identity": lambda: torch.arange(n_dst, dtype=torch.int32),
           "groups": lambda: (torch.arange(n_dst) // 256).to(torch.int32), "bad": lambda: pu.fork_map(n_dst, n_src)}[kind]()
    if kind == "bad":
        idx[0], idx[64], idx[129] = -1, n_src, 2 ** 31 - 1
    idx = idx.to(DEV)
    got, want = (pu.fork_engine(hip, DEV, n_dst, 77, 1000, "torque-asym") for _ in range(2))
    for e in (got, want):
        e.reset()
    bad = torch.zeros(1, dtype=torch.int32, device=DEV)
    assert pl.fork_envs(got, src, idx, bad_count=bad) is None
    n_bad = pl.fork_envs(want, src, idx, fused=False)
    torch.cuda.synchronize()
    assert int(bad) == n_bad == (3 if kind == "bad" else 0)
    for k in pl.FORK_BUFFERS:
        gu.assert_same_bits(getattr(got, k).cpu(), getattr(want, k).cpu(), f"{kind} {n_src}->{n_dst}: `{k}`")
    if kind != "bad":
        pu.assert_fork_equal(got, src, idx, kind)


def test_fork_kernel_within_one_engine(hip):
    a = _short_source(hip, 130)
    want = {k: getattr(a, k).clone() for k in pl.FORK_BUFFERS}
    idx = (torch.arange(130) // 64 * 64).to(torch.int32).to(DEV)
    pl.fork_envs(a, a, idx)
    i = idx.to(torch.int64)
    for k in pl.FORK_BUFFERS:
        gu.assert_same_bits(getattr(a, k).cpu(), (want[k][:, i] if k == "state" else want[k][i]).cpu(), k)


@pytest.mark.parametrize("case,v_src,v_dst", [("torque-asym", None, None), ("position-asym", None, None), ("torque-sym", None, None),
                                              ("torque-asym", "narrow", "wide_helpers")])
def test_forked_hip_engine_reproduces_its_source(hip, case, v_src, v_dst):
    a = pu.lived_source(hip, DEV, case, variant=v_src)
    b = pu.fork_engine(hip, DEV, pu.FORK_DST, 77, 1000, case, variant=v_dst)
    idx = pu.fork_map(pu.FORK_DST, pu.FORK_SRC).to(DEV)
    pl.fork_envs(b, a, idx)
    pu.assert_fork_equal(b, a, idx, f"{case} fork")
    live = pu.fork_then_step(b, a, idx, 20, case)
    assert live >= 8, f"only {live} envs ever held a finger-cube impulse"


# ---- the sampled actions and the return ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("A", [9, 18])
def test_rollout_actions_equal_the_oracle_restatement(hip, oracle, A):
    E, S, H = 2, 64, 3
    lib = pu.plan_lib()
    c, d = pu.update_params(E, S, a=A, h=H)
    _, U = pu.update_case(E, S, a=A, h=H)
    U[0, 1, 0], U[1, 2, 3] = 0.99, -0.99                                      # the clamp bites
    n = E * S
    g = torch.Generator().manual_seed(3)
    rewards = [300.0 + 40.0 * torch.randn(n, generator=g) for _ in range(H)]
    rewards[2][7] = float("nan")
    resets = [torch.zeros(n, dtype=torch.uint8) for _ in range(H)]
    resets[1][5] = 1                                                          # env 5's episode ends in step 1: its return freezes there
    disc = torch.tensor([1.0, 0.95, 0.95 ** 2], dtype=torch.float32)
    Ud, discd = U.to(DEV), disc.to(DEV)
    G, alive, action = (gu.sentinel_filled(s, t, DEV) for s, t in (((n,), torch.float32), ((n,), torch.uint8), ((n, A), torch.float32)))
    Gs, alives, actions = torch.full((n,), 5.0), torch.zeros(n, dtype=torch.uint8), torch.zeros(n, A)
    i = torch.arange(n)
    for h in range(H + 1):
        r = (rewards[h - 1] if h else torch.zeros(n)).to(DEV)
        z = (resets[h - 1] if h else torch.zeros(n, dtype=torch.uint8)).to(DEV)
        assert lib.tfpl_rollout_actions(C.byref(c), h, Ud.data_ptr(), discd.data_ptr(), r.data_ptr(), z.data_ptr(), G.data_ptr(), alive.data_ptr(),
                                        action.data_ptr(), _stream()) == 0
        torch.cuda.synchronize()
        pl.rollout_actions_statement(d, h, U, disc, r.cpu(), z.cpu(), Gs, alives, actions)
        gu.assert_same_bits(G.cpu(), Gs, f"G in front of step {h}")
        assert torch.equal(alive.cpu(), alives), h
        if h < H:
            eps = pu.oracle_noise(oracle, i, h, A, d["seed"], d["plan_counter"], S)
            u = U[i // S, h].numpy()
            want = np.minimum(np.maximum(u + np.float32(d["sigma"]) * eps, np.float32(d["lo"])), np.float32(d["hi"])).astype(np.float32)
            gu.assert_same_bits(action.cpu(), torch.from_numpy(want), f"actions of step {h}")
            gu.assert_same_bits(actions, torch.from_numpy(want), f"the statement's actions of step {h}")
    assert not alives[5] and not alives[7] and not torch.isfinite(Gs[7]) and float(Gs[5]) == float(rewards[0][5] + disc[1] * rewards[1][5])
    assert bool((action.cpu().abs() == 1.0).any())


# ---- the update ----------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("normalize", [True, False], ids=["std", "plain"])
@pytest.mark.parametrize("E,S", pu.UPDATE_SHAPES)
def test_update_kernel_against_the_float64_statement(hip, E, S, normalize):
    """U and first within S * 2^-23 (the summation bound for weights summing to 1 and |a| <= 1); the weights within 4 * pu.W_DEVIATION = 4.12e-7, four times
    the float32-against-float64 deviation of the torch statement measured on the CPU on these inputs (1.03e-7)"""
    lib = pu.plan_lib()
    G, U = pu.update_case(E, S)
    for shift in (True, False):
        c, d = pu.update_params(E, S, normalize=normalize, lam=0.3 if normalize else 12.0, shift=shift)
        U64 = U.double()
        first64, w64, stats64, invalid64 = pl.update_statement(d, G, U64, torch.float64)
        Ud = U.to(DEV)
        first, w, stats = (gu.sentinel_filled(s, torch.float32, DEV) for s in ((E, 9), (E * S,), (E, pl.NUM_STATS)))
        invalid = gu.sentinel_filled((E,), torch.int32, DEV)
        assert lib.tfpl_update(C.byref(c), G.to(DEV).data_ptr(), Ud.data_ptr(), first.data_ptr(), w.data_ptr(), stats.data_ptr(), invalid.data_ptr(), _stream()) == 0
        torch.cuda.synchronize()
        tol = S * 2.0 ** -23
        eu, ef = float((Ud.cpu().double() - U64).abs().max()), float((first.cpu().double() - first64).abs().max())
        ew = float((w.cpu().double() - w64).abs().max())
        print(f"update E={E} S={S} normalize={normalize} shift={shift}: |dU| {eu:.3e} |dfirst| {ef:.3e} (bound {tol:.3e}) |dw| {ew:.3e} (bound {4 * pu.W_DEVIATION:.3e})")
        assert eu <= tol and ef <= tol, (eu, ef, tol)
        assert ew <= 4 * pu.W_DEVIATION, ew
        assert torch.equal(invalid.cpu(), invalid64)
        assert torch.allclose(stats.cpu().double(), stats64, rtol=1e-4, atol=1e-4)
        assert not bool(w.cpu()[~torch.isfinite(G)].any())


def test_update_kernel_leaves_a_group_without_valid_samples(hip):
    lib = pu.plan_lib()
    E, S = 3, 128
    G, U = pu.update_case(E, S)
    G[S:2 * S] = float("nan")
    c, d = pu.update_params(E, S)
    Ud = U.to(DEV)
    first, w, stats = (gu.sentinel_filled(s, torch.float32, DEV) for s in ((E, 9), (E * S,), (E, pl.NUM_STATS)))
    invalid = gu.sentinel_filled((E,), torch.int32, DEV)
    assert lib.tfpl_update(C.byref(c), G.to(DEV).data_ptr(), Ud.data_ptr(), first.data_ptr(), w.data_ptr(), stats.data_ptr(), invalid.data_ptr(), _stream()) == 0
    torch.cuda.synchronize()
    assert torch.equal(Ud[1].cpu(), U[1]) and torch.equal(first[1].cpu(), U[1, 0]) and int(invalid[1]) == S
    assert not w[S:2 * S].any() and not stats[1].any()
    assert not torch.equal(Ud[0].cpu(), U[0]) and abs(float(w[:S].sum()) - 1.0) <= S * 2.0 ** -23


# ---- one plan --------------------------------------------------------------------------------------------------------------------------------------------------
def test_fused_plan_equals_the_statement_plan(hip):
    E, S, H = 2, 64, 4
    planners = []
    for fused in (True, False):
        plant = TrifingerEngine(make_config(hip, E, seed=3, command_mode="torque", task_difficulty=1, episode_length=0), device=DEV, lib=hip)
        plant.reset()
        for t in range(5):
            plant.step(pu.random_actions(t, E, 9).to(DEV))
        planners.append(pl.MPPIPlanner(plant, samples=S, horizon=H, sigma=0.5, lam=0.3, gamma=0.95, seed=9, fused=fused))
    ours, theirs = planners
    for k in range(2):                                                       # the second plan starts from the shifted sequence of the first
        a, b = ours.plan().clone(), theirs.plan().clone()
        torch.cuda.synchronize()
        gu.assert_same_bits(ours.action.cpu(), theirs.action.cpu(), f"plan {k}: the last actions")
        gu.assert_same_bits(ours.G.cpu(), theirs.G.cpu(), f"plan {k}: the returns")
        for name in pu.COMPARED:
            gu.assert_same_bits(getattr(ours.rollout, name).cpu(), getattr(theirs.rollout, name).cpu(), f"plan {k}: rollout `{name}`")
        assert float((a - b).abs().max()) <= S * 2.0 ** -23
        assert float((ours.U - theirs.U).abs().max()) <= S * 2.0 ** -23
        assert bool(ours.G.cpu().std() > 0) and int(ours.bad_forks) == 0
        theirs.U.copy_(ours.U)                                               # both go on from the same sequence
        for p in planners:
            p.plant.step(a)
    for p in planners:
        p.close()
