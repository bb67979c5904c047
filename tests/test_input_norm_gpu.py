"""The input-normalisation kernels (leibnizgym_amd/csrc/ppo_norm.hip and the statistics variant of the forward network walk) on the GPU, at the smallest
shapes at which each can still go wrong, and the trainer with both `normalize_input` keys on the HIP env.  References: torch, two passes in float64 for
the moments, the float32 expression torch.clamp((x - mean_f) * inv_std_f, -clip, clip) for everything that normalises (bit for bit)."""
import math
import os

import pytest
import torch

from leibnizgym_amd import ppo_kernels as pk
from leibnizgym_amd.ppo import InputNorm, PPOConfig, PPOTrainer

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
RTOL, ATOL = 1e-9, 1e-12
CLIP = 5.0


# ---- references -----------------------------------------------------------------------------------------------------------------------------
def two_pass(x):
    """[count, mean[D], M2[D]] of the rows of x, two passes in float64 on the same float32 values"""
    xd = x.reshape(-1, x.shape[-1]).double()
    mean = xd.mean(0)
    return torch.cat([torch.tensor([float(xd.shape[0])], dtype=torch.float64, device=x.device), mean, ((xd - mean) ** 2).sum(0)])


def chan(run, recs):
    """the merge formula in float64, written out: run, recs[j] = [count, mean[D], M2[D]]; recs in order"""
    D = (run.numel() - 1) // 2
    na, ma, Ma = float(run[0]), run[1:1 + D].clone(), run[1 + D:].clone()
    for r in recs:
        nb, mb, Mb = float(r[0]), r[1:1 + D], r[1 + D:]
        if na == 0:
            na, ma, Ma = nb, mb.clone(), Mb.clone()
            continue
        n = na + nb
        delta = mb - ma
        ma, Ma, na = ma + delta * nb / n, Ma + Mb + delta * delta * na * nb / n, n
    return torch.cat([torch.tensor([na], dtype=torch.float64, device=run.device), ma, Ma])


def published(rec):
    D = (rec.numel() - 1) // 2
    n = float(rec[0])
    var = rec[1 + D:] / n if n > 0 else torch.ones(D, dtype=torch.float64, device=rec.device)
    return rec[1:1 + D].float(), (1.0 / torch.sqrt(var + 1e-5)).float()


def assert_record_close(got, want):
    D = (want.numel() - 1) // 2
    assert float(got[0]) == float(want[0])
    assert torch.allclose(got[1:1 + D], want[1:1 + D], rtol=RTOL, atol=ATOL), (got[1:1 + D] - want[1:1 + D]).abs().max()
    assert torch.allclose(got[1 + D:] / got[0], want[1 + D:] / want[0], rtol=RTOL, atol=ATOL), (got[1 + D:] / got[0] - want[1 + D:] / want[0]).abs().max()


def assert_within_one_ulp(got, ref):
    """float32 `got` within one unit in the last place of float32 `ref` (two float64 values 1e-10 apart may round apart)"""
    up = torch.nextafter(ref, torch.full_like(ref, math.inf)) - ref
    dn = ref - torch.nextafter(ref, torch.full_like(ref, -math.inf))
    assert bool(((got - ref).abs() <= torch.maximum(up, dn)).all()), (got - ref).abs().max()


def planted(rows, D, seed):
    """standard normal [rows, D] with planted columns: constant; mean 1e4, standard deviation 1e-2; one outlier of 1e6.  With fewer than 4 columns
    the planted ones take turns with the row count."""
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(rows, D, generator=g)
    kinds = {}
    order = ["const", "hard", "outlier"]
    if D < 4:
        order = order[rows % 3:] + order[:rows % 3]
    for c, kind in zip(range(min(D, 3)), order):
        if kind == "const":
            x[:, c] = 0.37
        elif kind == "hard":
            x[:, c] = 1e4 + 1e-2 * torch.randn(rows, generator=g)
        else:
            x[rows // 2, c] = 1e6
        kinds[kind] = c
    return x.to(DEV).contiguous(), kinds


# ---- tfp_moments --------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("rows", [1, 63, 1025, 4099])
@pytest.mark.parametrize("D", [1, 41, 113])
def test_moments(hip, rows, D):
    D2 = {1: 41, 41: 113, 113: 1}[D]
    x0, k0 = planted(rows, D, 100 + rows + D)
    x1, _ = planted(rows, D2, 200 + rows + D)
    w0, w1 = two_pass(x0), two_pass(x1)
    both, a0, a1 = pk.moments([x0, x1]), pk.moments([x0]), pk.moments([x1])
    assert both is not None and both.dtype == torch.float64 and both.numel() == 2 + 2 * D + 2 * D2
    assert_record_close(a0, w0)
    assert_record_close(a1, w1)
    # two arrays in one call are the two calls, and a second call gives the same bits
    assert torch.equal(both, torch.cat([a0, a1]))
    assert torch.equal(pk.moments([x0, x1]), both) and torch.equal(pk.moments([x0]), a0)
    # the constant column: M2 exactly 0 and, published from count 0, exactly (float)(1 / sqrt(1e-5))
    if "const" in k0:
        c = k0["const"]
        assert float(a0[1 + D + c]) == 0.0 and float(a0[1 + c]) == float(torch.tensor(0.37, dtype=torch.float32).double())
        rec = InputNorm(D, DEV)
        pk.norm_merge([rec.state], [a0], 1, a0.numel(), [rec.mean_f], [rec.inv_std_f])
        want = torch.tensor(1.0 / math.sqrt(1e-5), dtype=torch.float64).float()
        assert float(rec.inv_std_f[c]) == float(want)
        assert torch.equal(rec.state, a0)                     # from count 0: the batch's own moments


def test_moments_declines_a_row_wider_than_a_workgroup(hip):
    assert pk.moments([torch.randn(4, 257, device=DEV)]) is None


# ---- tfp_norm_merge -------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k", [1, 2, 8])
def test_norm_merge(hip, k):
    g = torch.Generator().manual_seed(40 + k)
    Do, Ds = 41, 113
    sizes = [1, 300, 17, 64, 5, 1000, 2, 129][:k]
    bo = [(torch.randn(r, Do, generator=g) * 3 + 1).to(DEV) for r in sizes]
    bs = [(torch.randn(r, Ds, generator=g) * 0.01 + 1e3).to(DEV) for r in sizes]
    # the layout of a gathered vector: per "rank" [record of obs | record of states]
    L = 2 + 2 * Do + 2 * Ds
    vec = torch.cat([torch.cat([two_pass(a), two_pass(b)]) for a, b in zip(bo, bs)])
    ro, rs = InputNorm(Do, DEV), InputNorm(Ds, DEV)
    want_o, want_s = torch.zeros(1 + 2 * Do, dtype=torch.float64, device=DEV), torch.zeros(1 + 2 * Ds, dtype=torch.float64, device=DEV)
    for _ in range(2):                                        # from count 0, then into a running record
        pk.norm_merge([ro.state, rs.state], [vec, vec[1 + 2 * Do:]], k, L, [ro.mean_f, rs.mean_f], [ro.inv_std_f, rs.inv_std_f])
        want_o = chan(want_o, [vec[j * L:j * L + 1 + 2 * Do] for j in range(k)])
        want_s = chan(want_s, [vec[j * L + 1 + 2 * Do:(j + 1) * L] for j in range(k)])
        for rec, want in ((ro, want_o), (rs, want_s)):
            assert_record_close(rec.state, want)
            mf, isf = published(want)
            assert_within_one_ulp(rec.mean_f, mf)
            assert_within_one_ulp(rec.inv_std_f, isf)
    # ... which is the moments of everything, seen twice
    assert_record_close(ro.state, two_pass(torch.cat(bo + bo)))
    assert_record_close(rs.state, two_pass(torch.cat(bs + bs)))
    # one record alone in a call
    r1 = InputNorm(Do, DEV)
    pk.norm_merge([r1.state], [vec], k, L, [r1.mean_f], [r1.inv_std_f])
    assert_record_close(r1.state, chan(torch.zeros_like(r1.state), [vec[j * L:j * L + 1 + 2 * Do] for j in range(k)]))


# ---- tfp_gather_rows_norm -------------------------------------------------------------------------------------------------------------------------
def gather_case(rows, identity, device=DEV):
    """three arrays of widths 41, 9, 113 (the middle one without statistics), an index with repeats and out of order, inputs scaled so that the
    reference clamps a few per cent of the elements"""
    g = torch.Generator().manual_seed(11 + rows + (1000 if identity else 0))
    n_src = rows if identity else 300
    srcs = [(torch.randn(n_src, w, generator=g) * 2.8).to(device) for w in (41, 9, 113)]
    stats = [((torch.randn(w, generator=g) * 0.1).to(device), (0.8 + 0.4 * torch.rand(w, generator=g)).to(device), CLIP) if w != 9 else None for w in (41, 9, 113)]
    idx = None
    if not identity:
        idx = torch.randint(0, n_src, (rows,), generator=g)
        if rows > 1:
            idx[0], idx[-1] = n_src - 1, 0                    # out of order, both ends of the source
            idx[rows // 2] = idx[0]                           # a repeat
        idx = idx.to(device)
    return srcs, stats, idx


def gather_reference(srcs, stats, idx):
    out, clamped, total = [], 0, 0
    for s, st in zip(srcs, stats):
        x = s if idx is None else s[idx]
        if st is None:
            out.append(x.clone())
            continue
        raw = (x - st[0]) * st[1]
        out.append(torch.clamp(raw, -st[2], st[2]))
        clamped += int((raw.abs() > st[2]).sum())
        total += raw.numel()
    return out, clamped / total


@pytest.mark.parametrize("rows", [1, 5, 257])
@pytest.mark.parametrize("identity", [False, True])
def test_gather_with_statistics(hip, rows, identity):
    srcs, stats, idx = gather_case(rows, identity)
    want, share = gather_reference(srcs, stats, idx)
    assert 0.03 <= share <= 0.10, share                      # the reference itself clamps
    got = pk.gather_rows(srcs, idx, norm=stats)
    assert len(got) == 3
    for a, b in zip(got, want):
        assert a.shape == b.shape and torch.equal(a, b)
    assert torch.equal(got[1], srcs[1] if idx is None else srcs[1][idx])      # no statistics: copied bit for bit
    if idx is not None:                                       # no statistics at all: the plain gather
        for a, s in zip(pk.gather_rows(srcs, idx, norm=[None, None, None]), srcs):
            assert torch.equal(a, s[idx])
    else:
        assert torch.equal(pk.normalize_rows(srcs[0], *stats[0]), want[0])


# ---- the forward walk with statistics ---------------------------------------------------------------------------------------------------------------
def nets_and_stats(M, seed):
    g = torch.Generator().manual_seed(seed)

    def layers(din, dout):
        dims = [din, 400, 200, 100, dout]
        return [((torch.randn(dims[i + 1], dims[i], generator=g) / math.sqrt(dims[i])).to(DEV), (0.1 * torch.randn(dims[i + 1], generator=g)).to(DEV),
                 1 if i < 3 else 0, None) for i in range(4)]
    xa, xc = (torch.randn(M, 41, generator=g) * 2.5).to(DEV), (torch.randn(M, 113, generator=g) * 2.5).to(DEV)
    sa = ((torch.randn(41, generator=g) * 0.1).to(DEV), (0.8 + 0.4 * torch.rand(41, generator=g)).to(DEV), CLIP)
    sc = ((torch.randn(113, generator=g) * 0.1).to(DEV), (0.8 + 0.4 * torch.rand(113, generator=g)).to(DEV), CLIP)
    return xa, layers(41, 9), sa, xc, layers(113, 1), sc


def assert_same_outputs(got, want, store_hidden):
    assert got is not None and want is not None and len(got) == len(want)
    for ga, wa in zip(got, want):
        assert len(ga) == len(wa) == 4
        for l, (a, b) in enumerate(zip(ga, wa)):
            if l < 3 and not store_hidden:
                assert a is None and b is None
            else:
                assert torch.equal(a, b), l


@pytest.mark.parametrize("M", [1, 31, 33, 130])
@pytest.mark.parametrize("store_hidden", [True, False])
def test_walk_with_statistics(hip, M, store_hidden):
    xa, la, sa, xc, lc, sc = nets_and_stats(M, 50 + M)
    na, nc = pk.normalize_rows(xa, *sa), pk.normalize_rows(xc, *sc)
    assert torch.equal(na, torch.clamp((xa - sa[0]) * sa[1], -CLIP, CLIP)) and (M == 1 or bool((na.abs() == CLIP).any()))
    # the trainer's two networks, both with statistics: the plain walk on rows normalised by the gather
    want = pk.mlp_walk_forward([(na, la), (nc, lc)], store_hidden)
    got = pk.mlp_walk_forward([(xa, la), (xc, lc)], store_hidden, norms=[sa, sc])
    assert_same_outputs(got, want, store_hidden)
    # a network without statistics in the same call: the plain walk on its raw rows
    raw = pk.mlp_walk_forward([(xa, la), (xc, lc)], store_hidden)
    got = pk.mlp_walk_forward([(xa, la), (xc, lc)], store_hidden, norms=[sa, None])
    assert_same_outputs(got, [want[0], raw[1]], store_hidden)
    got = pk.mlp_walk_forward([(xa, la), (xc, lc)], store_hidden, norms=[None, sc])
    assert_same_outputs(got, [raw[0], want[1]], store_hidden)
    # the actor alone
    got = pk.mlp_walk_forward([(xa, la)], store_hidden, norms=[sa])
    assert_same_outputs(got, pk.mlp_walk_forward([(na, la)], store_hidden), store_hidden)
    # the pair entry point the trainer calls
    ya, yc = pk.mlp_forward_pair(xa, la, xc, lc, store_hidden=store_hidden, norms=(sa, sc))
    assert_same_outputs([ya, yc], want, store_hidden)


# ---- the trainer on the HIP env -----------------------------------------------------------------------------------------------------------------------
def hip_trainer(n, **kw):
    from leibnizgym_amd.config import gym_config
    from leibnizgym_amd.envs import TrifingerEnv
    from leibnizgym_amd.utils.rlg_train import RlGamesGpuEnvAdapter
    from leibnizgym_amd.wrappers import VecTaskPython
    cfg = gym_config("trifinger_difficulty_4")
    cfg.update(num_instances=n, seed=1, physics_engine="physx", asymmetric_obs=True, episode_length=20)
    env = TrifingerEnv(config=cfg, device=DEV, verbose=False)
    ad = RlGamesGpuEnvAdapter("rlgpu", n, env=VecTaskPython(env, rl_device=DEV))
    return PPOTrainer(ad, 41, 113, 9, PPOConfig(horizon=8, minibatches=4, mini_epochs=2, **kw), device=DEV)


def test_trainer_with_both_keys_on_the_hip_env(hip, tmp_path, monkeypatch):
    walks, per_layer = [], []
    walk, group = pk.mlp_walk_forward, pk.linear_fwd_group

    def spy_walk(nets, store_hidden=True, norms=None):
        out = walk(nets, store_hidden, norms)
        walks.append((norms is not None, out is not None, store_hidden))
        return out
    monkeypatch.setattr(pk, "mlp_walk_forward", spy_walk)
    monkeypatch.setattr(pk, "linear_fwd_group", lambda *a, **k: (per_layer.append(1), group(*a, **k))[1])
    T, n = 8, 512
    tr = hip_trainer(n, normalize_input=True, normalize_input_value=True)
    ro, rs = tr.net.obs_norm, tr.net.state_norm
    assert ro.fused and rs.fused
    buf1 = tr.rollout()
    assert torch.equal(ro.mean_f, torch.zeros(41, device=DEV))       # frozen during the rollout
    st = tr.update(buf1)
    assert all(math.isfinite(st[k]) for k in ("loss", "a_loss", "c_loss", "kl"))
    for rec, key in ((ro, "obs"), (rs, "states")):
        want = two_pass(buf1[key])
        assert float(rec.count) == T * n
        assert_record_close(rec.state, want)
        mf, isf = published(want)
        assert_within_one_ulp(rec.mean_f, mf)
        assert_within_one_ulp(rec.inv_std_f, isf)
    # the second epoch merges into a running record
    bufs = []
    upd = tr.update
    monkeypatch.setattr(tr, "update", lambda b: (bufs.append(b), upd(b))[1])
    stats = tr.train(1)
    assert all(math.isfinite(stats[0][k]) for k in ("loss", "a_loss", "c_loss", "kl"))
    for rec, key in ((ro, "obs"), (rs, "states")):
        want = two_pass(torch.cat([buf1[key], bufs[0][key]]))
        assert float(rec.count) == 2 * T * n
        assert_record_close(rec.state, want)
        mf, isf = published(want)
        assert_within_one_ulp(rec.mean_f, mf)
        assert_within_one_ulp(rec.inv_std_f, isf)
    # the fused path was taken: every rollout step walked raw rows with statistics, every minibatch walked the gather's normalised rows, nothing fell back
    assert len(walks) == 2 * (T + 2 * 4) and all(ok for _, ok, _ in walks) and per_layer == []
    assert sum(1 for nm, _, sh in walks if nm and not sh) == 2 * T and sum(1 for nm, _, sh in walks if not nm and sh) == 2 * 2 * 4
    # checkpoint round trip
    path = tr.save(os.path.join(tmp_path, "n.pth"))
    other = hip_trainer(n, normalize_input=True, normalize_input_value=True)
    other.restore(path)
    obs = torch.randn(64, 41, device=DEV) * 2
    assert torch.equal(tr.act(obs), other.act(obs))
    for a, b in ((ro, other.net.obs_norm), (rs, other.net.state_norm)):
        assert torch.equal(a.state, b.state) and torch.equal(a.mean_f, b.mean_f) and torch.equal(a.inv_std_f, b.inv_std_f)
    with pytest.raises(ValueError):
        hip_trainer(64).restore(path)


def test_off_is_off_on_the_gpu(hip, monkeypatch):
    calls = []
    for name in ("moments", "norm_merge", "normalize_rows", "_gather_rows_norm"):
        monkeypatch.setattr(pk, name, lambda *a, _n=name, **k: calls.append(_n))
    walk = pk.mlp_walk_forward
    monkeypatch.setattr(pk, "mlp_walk_forward", lambda nets, store_hidden=True, norms=None: (calls.append("walk norms") if norms is not None else None,
                                                                                            walk(nets, store_hidden))[1])
    tr = hip_trainer(64)
    tr.train(1)
    tr.act(torch.randn(3, 41, device=DEV))
    assert calls == [] and "input_norm" not in tr.state_dict() and tr.n_norm_allgather == 0
