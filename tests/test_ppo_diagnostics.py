"""`diagnostics` of the in-repo PPO on the CPU (include/trifinger_ppo_diag.h, leibnizgym_amd/ppo.py): the key and its default, the torch statement of the
record against a float64 statement on the planted minibatches (tests/ppo_diagnostics_util.py), the statement of the optimiser's slots, the trainer on the
oracle env - nothing new with the key off, the same parameters with it on, counts that add up -, the log tags and line, and two gloo ranks.  The kernels'
side of the same definitions is tests/test_ppo_diagnostics_gpu.py."""
import copy
import math
import os
import re
import socket
import sys

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

import minibatch_step_util as mu
import ppo_diagnostics_util as du
from leibnizgym_amd import ppo
from leibnizgym_amd.config import RLG_ASYMM
from leibnizgym_amd.ppo import PPOConfig, PPOTrainer

EP_LEN, N, T = 6, 32, 4
PARENT_KEYS = {"kl", "loss", "a_loss", "c_loss", "lr", "mean_reward"}
RECORD_KEYS = {"clip_frac", "zero_grad_frac", "mu_out_frac", "approx_kl", "ratio_max", "ratio_min", "nonfinite_rows", "grad_norm", "grad_norm_max",
               "grad_trunc_frac"}
VALUE_KEYS = {"grad_norm_value", "grad_norm_max_value", "grad_trunc_frac_value"}
TORCH_KEYS = {"explained_variance", "entropy", "sigma_mean"}
FRACTIONS = ("clip_frac", "zero_grad_frac", "value_clip_frac", "mu_out_frac", "grad_trunc_frac", "grad_trunc_frac_value")


# ---- the key --------------------------------------------------------------------------------------------------------------------------------------
def test_from_rlg_reads_the_key():
    assert "diagnostics" not in RLG_ASYMM["params"]["config"]                        # the default tree does not change
    assert PPOConfig().diagnostics is False and PPOConfig.from_rlg(RLG_ASYMM, num_envs=64).diagnostics is False
    tree = copy.deepcopy(RLG_ASYMM)
    tree["params"]["config"]["diagnostics"] = True
    assert PPOConfig.from_rlg(tree, num_envs=64).diagnostics is True


def test_the_header_and_the_statement_name_the_same_slots():
    from leibnizgym_amd import ppo_kernels as pk
    inc = os.path.join(os.path.dirname(pk.library_path()), "..", "..", "include", "trifinger_ppo_diag.h")
    src = re.sub(r"/\*.*?\*/", "", open(inc).read(), flags=re.S)
    slots = [(k, int(v)) for k, v in re.findall(r"TFP_DIAG_([A-Z0-9_]+) = (\d+)", src)]
    names = ["ROWS", "CLIPPED", "ZERO_GRAD", "VCLIPPED", "MU_OUT", "NONFINITE", "K3_SUM", "RATIO_MAX", "RATIO_MIN", "STEPS", "TRUNC_A", "TRUNC_V", "GN_A_SUM",
             "GN_V_SUM", "GN_A_MAX", "GN_V_MAX", "N"]
    assert slots == [(n, i) for i, n in enumerate(names)]
    assert [getattr(ppo, "D_" + n) for n in names[:-1]] == list(range(16)) and ppo.DIAG_N == pk.DIAG_N == 16
    assert "0x7F800000" in src and ppo.DIAG_RATIO_MIN_CLEAR == pk.DIAG_RATIO_MIN_CLEAR == 0x7F800000 and pk.DIAG_RATIO_MIN == ppo.D_RATIO_MIN
    assert sorted(set(re.findall(r"\b(tfp_[a-z0-9_]+)\s*\(", src))) == ["tfp_clip_adam_diag", "tfp_ppo_loss_diag"]
    lib = pk.load()
    assert lib.tfp_api_version() == 3 and len(lib.tfp_ppo_loss_diag.argtypes) == 24 and len(lib.tfp_clip_adam_diag.argtypes) == 16
    # refused on the host, before any launch: no record, a misaligned record (the pointers are never dereferenced)
    p = 4096
    loss = [p] * 9 + [0, 0, 4, 9, 0.2, 1.0, 0.0, 0.0] + [p] * 5 + [None]
    assert lib.tfp_ppo_loss_diag(*loss, None) == -1 and lib.tfp_ppo_loss_diag(*loss, p + 4) == -1
    adam = [p] * 4 + [4, 8] + [p] * 3 + [1.0, 1.0, 0.9, 0.999, 1e-8, None]
    assert lib.tfp_clip_adam_diag(*adam, None) == -1 and lib.tfp_clip_adam_diag(*adam, p + 4) == -1


# ---- the statement ----------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["cell1", "cell3", "cell6", "cell1_weighted", "cell1_kl_rows"])
def test_torch_statement_against_the_float64_statement(name):
    p = du.planted(name)
    assert p.B == {1: 333, 3: 333, 6: 333}[p.cell]                                   # no row of these cells sits at a MU_OUT edge
    rec = du.torch_statement(p)
    assert rec.dtype == torch.int64 and tuple(rec.shape) == (16,) and rec[9:].tolist() == [0] * 7
    du.check_record(p, rec, "torch fp32, CPU")
    want_rows = {"cell1_weighted": 333 - 48, "cell1_kl_rows": 111}.get(name, 333)    # ceil(333 / 7) = 48 rows with w = 0
    assert int(rec[ppo.D_ROWS]) == want_rows and (int(rec[ppo.D_VCLIPPED]) > 0) == (p.cell == 6)


def test_statement_counts_a_nonfinite_row_in_nonfinite_alone():
    p = du.planted("cell1")
    i = p.inputs
    nlp = ppo.neglogp(i["act"], i["mu"], i["log_std"].expand_as(i["mu"]))
    l = i["old_nlp"] - nlp
    base = ppo.diag_objective_statement(l, l.exp(), i["adv"], i["mu"], p.e_clip)
    l2 = l.clone()
    l2[5], l2[6] = float("nan"), 200.0                                               # a NaN log-ratio; a finite one whose ratio overflows
    rec = ppo.diag_objective_statement(l2, l2.exp(), i["adv"], i["mu"], p.e_clip)
    assert int(rec[ppo.D_NONFINITE]) == 2 and int(rec[ppo.D_ROWS]) == int(base[ppo.D_ROWS]) - 2
    keep = torch.ones(p.B, dtype=torch.bool)
    keep[5] = keep[6] = False
    rest = ppo.diag_objective_statement(l[keep], l[keep].exp(), i["adv"][keep], i["mu"][keep], p.e_clip)
    assert rec.tolist()[:5] == rest.tolist()[:5] and rec.tolist()[6:9] == rest.tolist()[6:9]
    # no live row: every slot in its cleared state
    none = ppo.diag_objective_statement(l, l.exp(), i["adv"], i["mu"], p.e_clip, w=torch.zeros(p.B))
    assert none.tolist() == ppo.new_diag_record("cpu").tolist()


def test_optimiser_statement_and_the_reported_keys():
    f = lambda x: torch.tensor(x, dtype=torch.float32)                               # noqa: E731
    rec = ppo.new_diag_record("cpu")
    for norms in ((0.5, 3.0), (2.0, 0.25), (0.75, 1e9)):
        ppo.diag_merge(rec, ppo.diag_optimiser_statement([f(norms[0]), f(norms[1])], [1.0, float("inf")]), objective=False)
    v = rec.tolist()
    assert v[ppo.D_STEPS] == 3 and v[ppo.D_TRUNC_A] == 1 and v[ppo.D_TRUNC_V] == 0 and v[:8] == [0] * 8 and v[8] == ppo.DIAG_RATIO_MIN_CLEAR
    assert v[ppo.D_GN_A_SUM] == int(3.25 * 2 ** 24) and v[ppo.D_GN_V_SUM] == int((3.25 + 65536.0) * 2 ** 24)       # the clamp at 2^16
    assert du.bits_float(v[ppo.D_GN_A_MAX]) == 2.0 and du.bits_float(v[ppo.D_GN_V_MAX]) == 65536.0
    st = ppo.diagnostic_stats(v, 9, False, True)
    assert set(st) == {"nonfinite_rows", "grad_norm", "grad_norm_max", "grad_trunc_frac"} | VALUE_KEYS                 # ROWS is 0: no fraction, no NaN
    assert st["grad_norm"] == 3.25 / 3 and st["grad_trunc_frac"] == 1 / 3 and st["grad_norm_max_value"] == 65536.0
    one = ppo.diag_optimiser_statement([f(1.5)], [1.0]).tolist()
    assert one[ppo.D_TRUNC_A] == 1 and one[ppo.D_TRUNC_V] == one[ppo.D_GN_V_SUM] == one[ppo.D_GN_V_MAX] == 0
    assert set(ppo.diagnostic_stats(one, 9, False, False)) == {"nonfinite_rows", "grad_norm", "grad_norm_max", "grad_trunc_frac"}
    v[ppo.D_ROWS], v[ppo.D_CLIPPED], v[ppo.D_MU_OUT], v[ppo.D_K3_SUM], v[ppo.D_VCLIPPED] = 100, 25, 90, 2 ** 28, 10
    v[ppo.D_RATIO_MAX], v[ppo.D_RATIO_MIN] = 0x3FC00000, 0x3F000000
    st = ppo.diagnostic_stats(v, 9, True, True)
    assert (st["clip_frac"], st["mu_out_frac"], st["approx_kl"], st["value_clip_frac"], st["ratio_max"], st["ratio_min"]) == (0.25, 0.1, 0.01, 0.1, 1.5, 0.5)
    assert "value_clip_frac" not in ppo.diagnostic_stats(v, 9, False, True)


@pytest.mark.parametrize("cell", [1, 6])
def test_the_torch_minibatch_step_files_the_statement(cell):
    """PPOTrainer._mb_backward and _mb_apply with the key on, plain torch: the record is the statement's, the gradients are the float64 statement's as before"""
    name = f"cell{cell}"
    p = du.planted(name)
    tr = du.make_trainer(cell, "cpu", fused=False, diagnostics=True)
    mu.install(p.case, tr)
    d, idx = mu.minibatch(p.case, "cpu")
    acc = tr._new_acc("cpu")
    tr._mb_backward(d, p.idx, acc)
    assert tr.diag.tolist() == du.torch_statement(p).tolist()
    du.check_record(p, tr.diag, "trainer, torch path")
    mu.check(p.case, {n: q.grad for n, q in tr.net.named_parameters()}, acc["_fused"], "torch fp32, diagnostics on")
    norms = mu.group_norms(p.case, True)
    tr._mb_apply()
    v = tr.diag.tolist()
    assert v[ppo.D_STEPS] == 1 and [v[ppo.D_TRUNC_A], v[ppo.D_TRUNC_V]] == [int(x > 1.0) for x in norms]
    for q in range(2):
        assert v[ppo.D_GN_A_SUM + q] / 2 ** 24 == pytest.approx(norms[q], rel=2e-5) and du.bits_float(v[ppo.D_GN_A_MAX + q]) == pytest.approx(norms[q], rel=2e-5)


# ---- the trainer on the oracle env ------------------------------------------------------------------------------------------------------------------
def trainer(oracle, n=N, **kw):
    from leibnizgym_amd.config import gym_config
    from leibnizgym_amd.envs import TrifingerEnv
    from leibnizgym_amd.utils.rlg_train import RlGamesGpuEnvAdapter
    from leibnizgym_amd.wrappers import VecTaskPython
    cfg = gym_config("trifinger_difficulty_4")
    cfg.update(num_instances=n, seed=1, physics_engine="physx", asymmetric_obs=True, episode_length=EP_LEN)
    env = TrifingerEnv(config=cfg, device="cpu", verbose=False, lib=oracle)
    ad = RlGamesGpuEnvAdapter("rlgpu", n, env=VecTaskPython(env, rl_device="cpu"))
    return PPOTrainer(ad, 41, 113, 9, PPOConfig(horizon=T, minibatches=2, mini_epochs=2, **kw), device="cpu")


def run(tr, epochs=2):
    torch.manual_seed(11)                                                            # the same exploration noise and minibatch order for every trainer
    return tr.train(epochs)


def test_key_off_reports_nothing_new_and_key_on_moves_no_parameter(oracle):
    off, on = trainer(oracle), trainer(oracle, diagnostics=True)
    assert off.diag is None and off.last_diag is None and on.diag.tolist() == ppo.new_diag_record("cpu").tolist()
    s_off, s_on = run(off), run(on)
    assert all(torch.equal(a, b) for a, b in zip(on.net.parameters(), off.net.parameters()))          # the record observes only
    for a, b in zip(s_on, s_off):
        assert set(b) == PARENT_KEYS | {"epoch", "frames"} and all(a[k] == b[k] for k in b)
        assert set(a) == set(b) | RECORD_KEYS | VALUE_KEYS | TORCH_KEYS
    assert off.n_diag_allreduce == on.n_diag_allreduce == 0


@pytest.mark.parametrize("keys", [{}, dict(episode_ends=True), dict(clip_value_central=True)], ids=["plain", "episode_ends", "clip_value"])
def test_counts_add_up(oracle, keys):
    tr = trainer(oracle, diagnostics=True, **keys)
    torch.manual_seed(11)
    for epoch in range(2):
        buf = tr.rollout()
        live = int(buf["w"].sum()) if tr.ends else T * N                             # a stale sample (w = 0) is no live row
        st = tr.update(buf)
        v = tr.last_diag
        assert tr.diag.tolist() == ppo.new_diag_record("cpu").tolist()               # taken and cleared
        assert v[ppo.D_STEPS] == 4 and v[ppo.D_ROWS] + v[ppo.D_NONFINITE] == 2 * live and v[ppo.D_NONFINITE] == 0 == st["nonfinite_rows"]
        assert v[ppo.D_ROWS] == 4 * (T * N // 2) - 2 * (T * N - live)
        assert ("value_clip_frac" in st) == bool(keys.get("clip_value_central"))
        assert all(0.0 <= st[k] <= 1.0 for k in FRACTIONS if k in st) and all(math.isfinite(float(x)) for x in st.values())
        assert st["clip_frac"] == v[ppo.D_CLIPPED] / v[ppo.D_ROWS] and st["approx_kl"] == v[ppo.D_K3_SUM] / 2 ** 28 / v[ppo.D_ROWS] >= 0.0
        assert st["mu_out_frac"] == v[ppo.D_MU_OUT] / (v[ppo.D_ROWS] * 9) and st["zero_grad_frac"] <= st["clip_frac"]
        assert 0 < st["grad_norm"] <= st["grad_norm_max"] and 0 < st["grad_norm_value"] <= st["grad_norm_max_value"]
        assert st["ratio_min"] <= st["ratio_max"] and st["sigma_mean"] > 0 and st["explained_variance"] <= 1.0
        if epoch == 0:                                                               # the first minibatch of an epoch trains on the rollout's own policy
            assert st["ratio_min"] <= 1.0 <= st["ratio_max"]
        ret, adv = buf["ret"].double(), buf["adv"].double()
        if not tr.ends:
            assert st["explained_variance"] == pytest.approx(1.0 - float(adv.var(unbiased=False) / ret.var(unbiased=False)), rel=1e-4, abs=1e-5)
            assert st["explained_variance"] == pytest.approx(1.0 - float((ret - buf["val"][:T].double()).var(unbiased=False) / ret.var(unbiased=False)),
                                                             rel=1e-3, abs=1e-4)
    if tr.ends:
        assert live < T * N                                                          # the second epoch holds the stale samples behind step 6


def test_no_truncation_still_reports_the_norm(oracle):
    tr = trainer(oracle, diagnostics=True, truncate_grads=False)
    st = run(tr, 1)[0]
    assert st["grad_trunc_frac"] == 0.0 and st["grad_norm"] > 0 and tr.last_diag[ppo.D_STEPS] == 4


# ---- the log ----------------------------------------------------------------------------------------------------------------------------------------
def test_log_tags_and_line():
    from leibnizgym_amd.utils.rlg_train import diagnostic_line, diagnostic_scalars
    st = dict(frames=1000, epoch=3, mean_reward=0.1, kl=0.01)
    assert diagnostic_scalars(st) == [] and diagnostic_line(st) == ""                # key off: nothing printed, nothing tagged
    st.update(clip_frac=0.25, approx_kl=0.0123, grad_norm=1.5, nonfinite_rows=0, entropy=12.0)
    tags = diagnostic_scalars(st)
    assert tags == [("diagnostics/clip_frac", 0.25, 1000), ("diagnostics/approx_kl", 0.0123, 1000), ("diagnostics/nonfinite_rows", 0, 1000),
                    ("diagnostics/grad_norm", 1.5, 1000), ("diagnostics/entropy", 12.0, 1000)]
    line = diagnostic_line(st)
    assert "clip 0.250" in line and "approx_kl 0.01230" in line and "grad norm 1.500" in line and "ev" not in line       # absent key, absent word
    st["explained_variance"] = -0.5
    assert "ev -0.500" in diagnostic_line(st) and ("diagnostics/explained_variance", -0.5, 1000) in diagnostic_scalars(st)


def test_native_runner_writes_the_tags(oracle, tmp_path, monkeypatch):
    from leibnizgym_amd.utils import rlg_train as rt
    tr = trainer(oracle, n=8, diagnostics=True, max_epochs=1)
    runner = rt.NativeRunner()
    runner.load({"params": {"config": {"print_stats": False}}})

    def build(args):
        runner.trainer, runner.writer = tr, rt.ScalarSink(os.path.join(args["logdir"], "summaries"))
        return tr.cfg
    monkeypatch.setattr(runner, "_build", build)
    seen = []
    add = rt.ScalarSink.add_scalar
    monkeypatch.setattr(rt.ScalarSink, "add_scalar", lambda self, tag, value, step: (seen.append((tag, step)), add(self, tag, value, step))[1])
    runner.run({"train": True, "logdir": str(tmp_path)})
    tags = [t for t, _ in seen if t.startswith("diagnostics/")]
    assert {"diagnostics/clip_frac", "diagnostics/approx_kl", "diagnostics/explained_variance", "diagnostics/grad_norm", "diagnostics/grad_norm_value"} <= set(tags)
    assert all(s == T * 8 for t, s in seen if t.startswith("diagnostics/"))          # over frames


# ---- two ranks ----------------------------------------------------------------------------------------------------------------------------------------
def _rank(rank, world, port, out_dir):
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
    from oracle_util import load_oracle
    import test_ppo_diagnostics as me
    torch.set_num_threads(1)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    seen = []
    for name in ("all_reduce", "all_gather", "all_gather_into_tensor", "broadcast", "reduce", "reduce_scatter", "barrier", "all_to_all", "gather", "scatter"):
        def wrapped(*a, _f=getattr(dist, name), _n=name, **k):
            seen.append((_n, str(a[0].dtype) if a and torch.is_tensor(a[0]) else ""))
            return _f(*a, **k)
        setattr(dist, name, wrapped)
    tr = me.trainer(load_oracle(), n=8, diagnostics=True)
    local, stats_of = [], tr._diag_stats

    def spy(ev_pair):
        local.append(tr.diag.clone())
        return stats_of(ev_pair)
    tr._diag_stats = spy
    del seen[:]                                                           # the constructor's broadcasts
    stats, reduced = [], []
    for _ in range(2):
        stats.append(tr.update(tr.rollout()))
        reduced.append(list(tr.last_diag))
    np.savez(os.path.join(out_dir, f"rank{rank}.npz"), local=torch.stack(local).numpy(), reduced=np.array(reduced), n_diag=tr.n_diag_allreduce,
             n_int64=sum(1 for n, d in seen if n == "all_reduce" and d == "torch.int64"), n_coll=len(seen),
             n_other=tr.n_grad_allreduce + tr.n_kl_allreduce + tr.n_norm_allgather, ratio_max=np.array([s["ratio_max"] for s in stats]),
             ratio_min=np.array([s["ratio_min"] for s in stats]), ev=np.array([s["explained_variance"] for s in stats]))
    dist.destroy_process_group()


def test_two_ranks_reduce_the_record_with_two_collectives(oracle, tmp_path):
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        port = s.getsockname()[1]
    mp.spawn(_rank, args=(2, port, str(tmp_path)), nprocs=2, join=True)
    a, b = (np.load(os.path.join(tmp_path, f"rank{r}.npz")) for r in range(2))
    assert np.array_equal(a["reduced"], b["reduced"]) and not np.array_equal(a["local"], b["local"])
    la, lb, red = a["local"], b["local"], a["reduced"]
    for e in range(2):
        assert la[e][ppo.D_ROWS] == lb[e][ppo.D_ROWS] == 2 * T * 8 and red[e][ppo.D_ROWS] == la[e][ppo.D_ROWS] + lb[e][ppo.D_ROWS]
        assert (red[e][:7] == la[e][:7] + lb[e][:7]).all()                                             # slots 0-6: the sum
        assert red[e][ppo.D_RATIO_MAX] == max(la[e][ppo.D_RATIO_MAX], lb[e][ppo.D_RATIO_MAX])          # the larger of the two
        assert red[e][ppo.D_RATIO_MIN] == min(la[e][ppo.D_RATIO_MIN], lb[e][ppo.D_RATIO_MIN])
        assert (red[e][9:] == la[e][9:]).all() and (la[e][9:] == lb[e][9:]).all()                      # the exchanged gradient's norms: the same, not reduced
        assert float(a["ratio_max"][e]) == du.bits_float(red[e][ppo.D_RATIO_MAX]) == float(b["ratio_max"][e])
    assert la[0][ppo.D_RATIO_MAX] != lb[0][ppo.D_RATIO_MAX]
    for p in (a, b):                                                      # two all-reduces per epoch, int64 ones, and nothing else that is new
        assert int(p["n_diag"]) == 4 == int(p["n_int64"]) and int(p["n_coll"]) == int(p["n_other"]) + 4
    assert not np.array_equal(a["ev"], b["ev"])                           # explained_variance is rank-local
