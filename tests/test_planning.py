"""Planning on the CPU (include/trifinger_plan.h, leibnizgym_amd/planning.py): the header, the library and the binding agree; the fork on the oracle engine -
a forked env stepped with its source's action stays its source bit for bit, with live contacts; the noise statement against a restatement from the
oracle's own primitives; the properties of the update; and the closed loop: the planner beats zero and random actions.  The torch statements run here;
tests/test_planning_gpu.py holds the kernels to them.  No GPU needed."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest
import torch

import guard_util as gu
import plan_util as pu
from leibnizgym_amd import _capi as capi
from leibnizgym_amd import planning as pl
from leibnizgym_amd.engine import TrifingerEngine, make_config
from oracle_util import REPO

HEADER = os.path.join(REPO, "include", "trifinger_plan.h")


def _header():
    return re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)


def _declarations():
    return {name: (0 if params.strip() in ("", "void") else params.count(",") + 1)
            for name, params in re.findall(r"\b(tfpl_[a-z0-9_]+)\s*\(([^()]*)\)\s*;", _header())}


# ---- 1. header <-> library <-> binding -------------------------------------------------------------------------------------------------------------------
def test_header_library_and_binding_agree():
    lib = pu.plan_lib()                                      # loads without a GPU
    decls = _declarations()
    assert decls == {"tfpl_api_version": 0, "tfpl_last_error_string": 0, "tfpl_fork": 5, "tfpl_rollout_actions": 10, "tfpl_update": 8}, decls
    assert sorted(decls) == sorted(pl.SYMBOLS)
    raw = C.CDLL(pl.library_path())
    for name, count in sorted(decls.items()):
        assert hasattr(raw, name), f"{name} is declared but not exported"
        assert len(getattr(lib, name).argtypes) == count, name
    src = _header()
    for name in ("TFPL_API_VERSION", "TFPL_MAX_ACTION_DIM", "TFPL_MAX_HORIZON", "TFPL_MIN_SAMPLES", "TFPL_MAX_SAMPLES"):
        assert getattr(pl, name) == int(re.search(rf"#define {name} (\d+)", src).group(1)), name
    assert lib.tfpl_api_version() == pl.TFPL_API_VERSION
    assert pl.TFPL_STD_TINY == float(re.search(r"#define TFPL_STD_TINY ([0-9.e+-]+)f", src).group(1))
    assert pl.TF_MAX_ENVS == int(re.search(r"#define TF_MAX_ENVS (\d+)", open(os.path.join(REPO, "include", "trifinger.h")).read()).group(1))
    assert pl.FORK_BUFFERS == tuple(n for n, _ in capi.TfBuffers._fields_)[:11]


def test_struct_sizes_match_the_c_compiler(tmp_path):
    prog = r'''
#include <stdio.h>
#include <stddef.h>
#include "trifinger_plan.h"
int main(void) { printf("%zu %zu %zu %zu %zu %zu %d\n", sizeof(TfplSide), offsetof(TfplSide, num_envs), sizeof(TfplPlan), offsetof(TfplPlan, seed),
                        offsetof(TfplPlan, sigma), offsetof(TfplPlan, shift), TFPL_NUM_STATS); return 0; }'''
    src, exe = tmp_path / "s.c", tmp_path / "s"
    src.write_text(prog)
    subprocess.check_call(["gcc", "-I", os.path.join(REPO, "include"), "-o", str(exe), str(src)])
    sizes = [int(x) for x in subprocess.check_output([str(exe)]).decode().split()]
    assert sizes == [C.sizeof(pl.TfplSide), pl.TfplSide.num_envs.offset, C.sizeof(pl.TfplPlan), pl.TfplPlan.seed.offset, pl.TfplPlan.sigma.offset,
                     pl.TfplPlan.shift.offset, pl.NUM_STATS]


def test_no_symbol_of_another_library_is_declared():
    found = re.findall(r"\b(tf[prk]?_[a-z0-9_]+)\s*\(", _header())
    assert not found, found


def test_refusals_happen_on_the_host(oracle):
    """every refusal comes before a launch: they run here, with pointers nothing dereferences"""
    lib = pu.plan_lib()
    eng = TrifingerEngine(make_config(oracle, 8, asymmetric_obs=True), device="cpu", lib=oracle)
    wide = TrifingerEngine(make_config(oracle, 8, asymmetric_obs=True, command_mode="position_impedance"), device="cpu", lib=oracle)
    sym = TrifingerEngine(make_config(oracle, 8, asymmetric_obs=False), device="cpu", lib=oracle)
    a = pl.side_of(eng)
    for other in (wide, sym):
        b = pl.side_of(other)
        assert lib.tfpl_fork(C.byref(a), C.byref(b), 8, None, None) == pl.TFPL_ERR_INVALID_ARG
        assert lib.tfpl_last_error_string().startswith(b"tfpl_fork")
    assert lib.tfpl_fork(C.byref(a), C.byref(a), None, None, None) == pl.TFPL_ERR_INVALID_ARG
    assert lib.tfpl_fork(None, C.byref(a), 8, None, None) == pl.TFPL_ERR_INVALID_ARG
    b = pl.side_of(eng)
    b.buf.reward = None
    assert lib.tfpl_fork(C.byref(a), C.byref(b), 8, None, None) == pl.TFPL_ERR_INVALID_ARG
    b = pl.side_of(eng)
    b.num_envs = 0
    assert lib.tfpl_fork(C.byref(a), C.byref(b), 8, None, None) == pl.TFPL_ERR_INVALID_ARG
    ok, _ = pl.plan_params(2, 64, 3, 9, sigma=0.3, lam=0.3)
    for field, value in (("samples", 96), ("samples", 32), ("samples", 2048), ("groups", 0), ("horizon", 0), ("horizon", 257), ("action_dim", 25),
                         ("sigma", -1.0), ("lam", 0.0), ("lam", float("nan")), ("lo", 2.0)):
        bad, _ = pl.plan_params(2, 64, 3, 9, sigma=0.3, lam=0.3)
        setattr(bad, field, value)
        assert lib.tfpl_update(C.byref(bad), 8, 8, 8, 8, 8, 8, None) == pl.TFPL_ERR_INVALID_ARG, (field, value)
        assert lib.tfpl_rollout_actions(C.byref(bad), 0, 8, 8, 8, 8, 8, 8, 8, None) == pl.TFPL_ERR_INVALID_ARG, (field, value)
    for h in (-1, 4):
        assert lib.tfpl_rollout_actions(C.byref(ok), h, 8, 8, 8, 8, 8, 8, 8, None) == pl.TFPL_ERR_INVALID_ARG
    assert lib.tfpl_rollout_actions(C.byref(ok), 1, 8, None, 8, 8, 8, 8, 8, None) == pl.TFPL_ERR_INVALID_ARG
    assert lib.tfpl_rollout_actions(C.byref(ok), 0, None, 8, 8, 8, 8, 8, 8, None) == pl.TFPL_ERR_INVALID_ARG
    assert lib.tfpl_update(C.byref(ok), 8, 8, 8, 8, 8, None, None) == pl.TFPL_ERR_INVALID_ARG
    with pytest.raises(ValueError, match="differ in width"):
        pl.fork_envs(eng, sym, torch.zeros(8, dtype=torch.int32))
    with pytest.raises(ValueError, match="src_index"):
        pl.fork_envs(eng, eng, torch.zeros(8, dtype=torch.int64))
    with pytest.raises(RuntimeError, match="MI355X"):
        pl.fork_envs(eng, eng, torch.zeros(8, dtype=torch.int32), fused=True, validate=False)
    for kw in (dict(samples=100), dict(horizon=0), dict(sigma=-0.1), dict(lam=0.0), dict(iterations=0), dict(gamma=1.5), dict(rollout_overrides={"x": 1})):
        args = dict(samples=64, horizon=4, sigma=0.3, lam=0.3, lib=oracle)
        args.update(kw)
        with pytest.raises(ValueError):
            pl.MPPIPlanner(eng, **args)


# ---- 2. the fork ---------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", list(pu.FORK_CASES))
def test_fork_then_step_reproduces_the_source(oracle, case):
    """128 -> 200 envs, other seed, other id range, a map with repeats: every per-env buffer equals its source's column after the fork, and state, obs,
    states and reward still do after 40 steps with a[src] against a - with live finger-cube impulses, so free motion alone cannot pass"""
    a = pu.lived_source(oracle, "cpu", case)
    b = pu.fork_engine(oracle, "cpu", pu.FORK_DST, 77, 1000, case)
    idx = pu.fork_map(pu.FORK_DST, pu.FORK_SRC)
    assert len(set(idx.tolist())) < pu.FORK_DST and not bool((idx[1:] >= idx[:-1]).all())           # repeats, out of order
    assert (b.states_dim == 0) == (case == "torque-sym")
    assert pl.fork_envs(b, a, idx) == 0
    pu.assert_fork_equal(b, a, idx, f"{case} fork")
    live = pu.fork_then_step(b, a, idx, 40, case)
    assert live >= 8, f"only {live} envs ever held a finger-cube impulse"


def test_fork_skips_and_counts_indices_out_of_range(oracle):
    a = pu.lived_source(oracle, "cpu", "torque-asym", n=16)
    b = pu.fork_engine(oracle, "cpu", 24, 77, 1000, "torque-asym")
    b.reset()
    before = {k: getattr(b, k).clone() for k in pl.FORK_BUFFERS}
    idx = pu.fork_map(24, 16)
    idx[3], idx[20] = -1, 16
    assert pl.fork_envs(b, a, idx) == 2
    keep = torch.ones(24, dtype=torch.bool)
    keep[3] = keep[20] = False
    for k in pl.FORK_BUFFERS:
        d, s = getattr(b, k), getattr(a, k)
        i = idx.to(torch.int64)[keep]
        gu.assert_same_bits(d[:, keep] if k == "state" else d[keep], s[:, i] if k == "state" else s[i], k)
        gu.assert_same_bits(d[:, ~keep] if k == "state" else d[~keep], before[k][:, ~keep] if k == "state" else before[k][~keep], f"{k} of the skipped envs")


def test_fork_within_one_engine_needs_fixed_point_sources(oracle):
    a = pu.lived_source(oracle, "cpu", "torque-asym", n=16)
    with pytest.raises(ValueError, match="fixed point"):
        pl.fork_envs(a, a, torch.arange(16, dtype=torch.int32).roll(1))
    want = {k: getattr(a, k).clone() for k in pl.FORK_BUFFERS}
    idx = (torch.arange(16) // 4 * 4).to(torch.int32)               # envs 0, 4, 8, 12 are their own sources
    assert pl.fork_envs(a, a, idx) == 0
    i = idx.to(torch.int64)
    for k in pl.FORK_BUFFERS:
        gu.assert_same_bits(getattr(a, k), want[k][:, i] if k == "state" else want[k][i], k)


# ---- 3. the noise ------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("A", [9, 18])
def test_noise_equals_the_restatement_from_the_oracle_primitives(oracle, A):
    seed, counter, S = 0x1234567887654321, 7, 64
    i = torch.arange(2 * S)
    for h in (0, 1, 2):
        got = pl.noise_statement(i, h, A, seed, counter, S).numpy()
        want = pu.oracle_noise(oracle, i, h, A, seed, counter, S)
        assert np.array_equal(got.view(np.uint32), want.view(np.uint32)), (A, h)
        assert not got[0].any() and not got[S].any() and got[1].all()                               # sample 0 of each group rolls out the nominal sequence
    hh = torch.tensor([0, 1, 2]).repeat(2 * S)
    many = pl.noise_statement(i.repeat_interleave(3), hh, A, seed, counter, S).reshape(2 * S, 3, A)
    assert torch.equal(many[:, 1], pl.noise_statement(i, 1, A, seed, counter, S))
    flat = torch.cat([pl.noise_statement(i, h, A, seed, c, S)[1:S] for h in range(8) for c in (7, 8)]).reshape(-1)
    assert abs(float(flat.mean())) < 0.05 and abs(float(flat.std()) - 1.0) < 0.05                    # standard normal
    assert len(torch.unique(flat)) > 0.99 * flat.numel()                                             # no two counters collide


def test_one_hot_weights_return_that_samples_actions(oracle):
    E, S, A = 2, 64, 9
    _, d = pu.update_params(E, S, normalize=False, lam=1.0, shift=False)
    _, U = pu.update_case(E, S)
    G = torch.zeros(E * S)
    pick = [17, S + 40]
    G[pick] = 1.0e6
    acts = pl.applied_actions(d, U)
    assert bool((acts.abs() == 1.0).any()) and bool((acts.abs() < 1.0).any())                       # the clamp bites somewhere
    U1 = U.clone()
    first, w, stats, invalid = pl.update_statement(d, G, U1)
    assert torch.equal(w[pick], torch.ones(2)) and float(w.sum()) == 2.0
    assert torch.equal(U1, acts[pick]) and torch.equal(first, acts[pick][:, 0])
    assert torch.equal(stats[:, pl.STAT_ESS], torch.ones(2)) and not invalid.any()


# ---- 4. the update -----------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("normalize", [True, False])
def test_update_properties(normalize):
    E, S = 5, 192
    G, U = pu.update_case(E, S)
    G[2 * S:3 * S] = float("nan")                                                                    # group 2: no valid sample
    lam = 0.3 if normalize else 12.0
    for shift in (True, False):
        _, d = pu.update_params(E, S, normalize=normalize, lam=lam, shift=shift)
        U1 = U.clone()
        first, w, stats, invalid = pl.update_statement(d, G, U1)
        ws = w.reshape(E, S)
        sums = ws.sum(1)
        assert bool(((sums - 1.0).abs()[[0, 1, 3, 4]] <= S * 2.0 ** -23).all()) and float(sums[2]) == 0.0, sums
        assert not bool(ws[~torch.isfinite(G.reshape(E, S))].any()) and bool((ws[torch.isfinite(G.reshape(E, S))] > 0).any())
        assert invalid.tolist() == [int((~torch.isfinite(G[e * S:(e + 1) * S])).sum()) for e in range(E)] and invalid[2] == S
        assert torch.equal(U1[2], U[2]) and torch.equal(first[2], U[2, 0])                          # a group without a valid sample keeps its sequence
        acts = pl.applied_actions(d, U).reshape(E, S, pu.UPDATE_H, 9)
        new = (ws[:, :, None, None] * acts).sum(1)
        keep = [0, 1, 3, 4]
        want = torch.cat([new[:, 1:], new[:, -1:]], 1) if shift else new
        assert torch.allclose(U1[keep], want[keep], rtol=0, atol=S * 2.0 ** -23) and torch.allclose(first[keep], new[keep, 0], rtol=0, atol=S * 2.0 ** -23)
        assert bool((stats[keep, pl.STAT_ESS] >= 1.0).all()) and bool((stats[keep, pl.STAT_ESS] <= S).all())
        assert bool((stats[keep, pl.STAT_BEST] >= stats[keep, pl.STAT_MEAN]).all())
    # adding a constant to every return changes no weight: float64 sums, and exactly in float32 where the shifted returns are exact
    _, d = pu.update_params(E, S, normalize=normalize, lam=lam)
    _, w0, _, _ = pl.update_statement(d, G.double(), U.clone(), torch.float64)
    _, w1, _, _ = pl.update_statement(d, G.double() + 1000.0, U.clone(), torch.float64)
    assert torch.allclose(w0, w1, rtol=1e-9, atol=1e-15)
    if not normalize:
        Gi = torch.round(G)
        _, w0, _, _ = pl.update_statement(d, Gi, U.clone())
        _, w1, _, _ = pl.update_statement(d, Gi + 1024.0, U.clone())
        assert torch.equal(w0, w1)


def test_update_weight_deviation_is_the_recorded_one():
    """max |w32 - w64| of the statement over the cases of the GPU test: tests/test_planning_gpu.py holds the kernel's weights to four times pu.W_DEVIATION"""
    got = pu.weight_deviation()
    assert pu.W_DEVIATION / 2 <= got <= pu.W_DEVIATION, got


def test_rollout_actions_statement_freezes_the_return_of_an_ended_episode():
    E, S, H, A = 1, 64, 3, 9
    _, d = pu.update_params(E, S, a=A, h=H)
    _, U = pu.update_case(E, S, a=A, h=H)
    disc = torch.tensor([1.0, 0.5, 0.25])
    G, alive, action = torch.full((S,), 7.0), torch.zeros(S, dtype=torch.uint8), torch.zeros(S, A)
    reward, reset = torch.arange(S, dtype=torch.float32), torch.zeros(S, dtype=torch.bool)
    pl.rollout_actions_statement(d, 0, U, disc, reward, reset, G, alive, action)
    assert not G.any() and alive.all() and torch.equal(action, pl.applied_actions(d, U, 0))
    reset[5] = True
    reward[9] = float("inf")
    pl.rollout_actions_statement(d, 1, U, disc, reward, reset, G, alive, action)
    assert G[5] == 5.0 and not alive[5] and not alive[9] and not torch.isfinite(G[9]) and alive.sum() == S - 2
    reset[5] = False
    reward[9] = 9.0
    pl.rollout_actions_statement(d, 2, U, disc, reward, reset, G, alive, action)
    pl.rollout_actions_statement(d, 3, U, disc, reward, reset, G, alive, action)
    assert G[5] == 5.0 and G[6] == 6.0 * 1.75 and not torch.isfinite(G[9])                           # the ended episode kept its return, that step included
    assert torch.equal(action, pl.applied_actions(d, U, 2))                                           # h == H writes no action


# ---- 5. the closed loop ------------------------------------------------------------------------------------------------------------------------------------
LOOP = dict(E=4, S=64, H=8, steps=100, lam=0.3, sigma={"position": 0.3, "torque": 0.5})


def closed_loop_totals(lib, device, mode, fused=None):
    """the plant's return summed over its four envs after 100 control steps under zero actions, uniform random actions and the planner -> three floats"""
    out = []
    for who in ("zero", "random", "mppi"):
        plant = TrifingerEngine(make_config(lib, LOOP["E"], seed=3, command_mode=mode, task_difficulty=1, episode_length=0), device=device, lib=lib)
        plant.reset()
        planner = pl.MPPIPlanner(plant, samples=LOOP["S"], horizon=LOOP["H"], sigma=LOOP["sigma"][mode], lam=LOOP["lam"], fused=fused) if who == "mppi" else None
        g = torch.Generator().manual_seed(5)
        total = torch.zeros(LOOP["E"], device=device)
        for _ in range(LOOP["steps"]):
            if who == "zero":
                plant.step(torch.zeros(LOOP["E"], plant.action_dim, device=device))
            elif who == "random":
                plant.step((torch.rand(LOOP["E"], plant.action_dim, generator=g) * 2 - 1).to(device))
            else:
                planner.act()
            total += plant.reward
        out.append(float(total.sum()))
        plant.close()
        if planner is not None:
            planner.close()
    return out


@pytest.mark.parametrize("mode", ["position", "torque"])
def test_planner_beats_zero_and_random_actions(oracle, mode):
    """E = 4, S = 64, H = 8, 100 control steps, difficulty 1, default reward terms, lam 0.3, sigma 0.3 (position) / 0.5 (torque).  Measured on the oracle with
    the Philox statement: position 1588 (zero) / 1262 (random) / 14721 (planner: two envs reach the goal and collect the success bonus), torque 1949 / 1087 /
    6382 - 9.3 and 3.3 times the better baseline."""
    zero, rand, mppi = closed_loop_totals(oracle, "cpu", mode)
    print(f"closed loop {mode}: zero {zero:.1f} random {rand:.1f} planner {mppi:.1f}")
    assert mppi > zero and mppi > rand, (zero, rand, mppi)


def test_planner_statistics_and_reset_plan(oracle):
    plant = TrifingerEngine(make_config(oracle, 2, seed=3, command_mode="torque", task_difficulty=1, episode_length=0), device="cpu", lib=oracle)
    plant.reset()
    planner = pl.MPPIPlanner(plant, samples=64, horizon=4, sigma=0.5, lam=0.3, gamma=0.9, iterations=2,
                             rollout_overrides={"reward_terms": {"object_dist": {"activate": True, "weight": 2000}}, "success": {"activate": False}})
    r = planner.rollout
    assert r.num_envs == 128 and r.cfg.episode_length == 0 and r.cfg.dr_obs_noise == 0.0 and r.cfg.dr_action_repeat == 0.0
    assert r.cfg.env_id_offset != plant.cfg.env_id_offset and r.cfg.command_mode == plant.cfg.command_mode and not r.cfg.success_activate
    assert [int(t.activate) for t in r.cfg.reward] == [0, 0, 1, 0, 0, 0] and [int(t.activate) for t in plant.cfg.reward] == [1] * 6
    a, _ = planner.act()
    assert tuple(a.shape) == (2, 9) and planner.plan_counter == 2 and bool((a.abs() <= 1).all())
    st = planner.stats()
    assert tuple(st["weights"].shape) == (2, 64) and torch.allclose(st["weights"].sum(1), torch.ones(2), atol=64 * 2.0 ** -23)
    assert bool((st["best"] >= st["mean"]).all()) and bool((st["ess"] >= 1).all()) and not st["invalid"].any()
    assert torch.equal(st["returns"].max(1).values, st["best"])
    assert planner.U.any()
    planner.reset_plan(torch.tensor([True, False]))
    assert not planner.U[0].any() and planner.U[1].any()
    planner.close()
