"""The symmetry augmentation on the GPU (include/trifinger_ppo_symmetry.h: tfp_gather_rows_sym, tfp_ppo_loss_sym) and the trainer with
`symmetry_augmentation` on the HIP env.  References: leibnizgym_amd.symmetry.apply - the torch expression of the tables, run on the same GPU tensors - bit for
bit for the gather (behind statistics: the existing normalising gather on the transformed rows); the four existing entry points of the objective for
kl_rows = B, the float64 torch objective at the tolerances of tests/test_value_path_gpu.py (whose inputs these tests share) for kl_rows = B / 3; the
equivariance scenario and bounds of tests/symmetry_util.py, measured on the oracle, on the HIP engine."""
import math

import pytest
import torch

import leibnizgym_amd.ppo as ppo
import symmetry_util as su
import test_value_path_gpu as vp
from leibnizgym_amd import ppo_kernels as pk
from leibnizgym_amd import symmetry as sy
from leibnizgym_amd.ppo import PPOConfig, PPOTrainer, neglogp
from value_path_util import E_CLIP

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
CLIP = 5.0


def same_bits(a, b):
    """bit for bit, -0 against +0 included; a NaN equals a NaN (its payload is not part of the statement)"""
    nan = torch.isnan(a)
    z = torch.zeros((), device=a.device)
    return a.shape == b.shape and torch.equal(nan, torch.isnan(b)) and torch.equal(torch.where(nan, z, a).view(torch.int32), torch.where(nan, z, b).view(torch.int32))


# ---- tfp_gather_rows_sym ---------------------------------------------------------------------------------------------------------------------
# eight arrays in one launch: (width, which table or None, statistics) - both obs and both states widths, both action widths, a copied column and a copied
# array with statistics
ARRAYS = [(41, ("obs", 9), True), (50, ("obs", 18), False), (113, ("states", 9), True), (122, ("states", 18), False), (9, ("action", 9), False),
          (18, ("action", 18), True), (1, None, False), (9, None, True)]


@pytest.fixture(scope="module")
def gather_tables():
    t = {A: sy.tables_to(sy.trifinger_symmetry(A, True), DEV) for A in (9, 18)}
    return [(t[k[1]][k[0]], sy.pack(t[k[1]][k[0]])) if k is not None else (None, None) for _, k, _ in ARRAYS]


@pytest.mark.parametrize("identity", [False, True], ids=["idx", "identity"])
@pytest.mark.parametrize("rows", [1, 63, 64, 65, 257])
def test_gather_rows_sym_holds_the_bits_of_apply(hip, gather_tables, rows, identity):
    g = torch.Generator().manual_seed(17 + rows)
    n_src = rows if identity else 300
    srcs = [torch.randn(n_src, w, generator=g) * 2.8 for w, _, _ in ARRAYS]
    # -0, inf and NaN in permuted columns (joints 0 .. 17, an action) and in rotated ones (position 18 .. 20, quaternion 21 .. 24, a fingertip block)
    for s, (w, key, _) in zip(srcs, ARRAYS):
        if key is None or n_src < 3:
            continue
        cols = [0, 4, 8] if key[0] == "action" else [1, 10, 18, 19, 22, 23, 26, 29] + ([w - 72 + 1, w - 72 + 6 + 14, w - 72 + 6 + 13 + 4, w - 1] if key[0] == "states" else [])
        for j, c in enumerate(cols):
            s[j % n_src, c] = (-0.0, float("inf"), float("nan"), -float("inf"))[j % 4]
    srcs = [s.to(DEV) if w > 1 else s[:, 0].contiguous().to(DEV) for s, (w, _, _) in zip(srcs, ARRAYS)]      # the single column as a 1-D array, like old_nlp
    stats = [((torch.randn(w, generator=g) * 0.1).to(DEV), (0.8 + 0.4 * torch.rand(w, generator=g)).to(DEV), CLIP) if st else None for w, _, st in ARRAYS]
    idx = None
    if not identity:
        idx = torch.randint(0, n_src, (rows,), generator=g)
        if rows > 1:
            idx[0], idx[-1], idx[rows // 2] = n_src - 1, 0, n_src - 1     # out of order, both ends of the source, a repeat
        idx[rows // 3] = 1                                                  # the planted rows are among the gathered ones
        idx = idx.to(DEV)
    before = [s.clone() for s in srcs]
    got = pk.gather_rows_sym(srcs, idx, [p for _, p in gather_tables], norm=stats)
    assert len(got) == 8 and all(same_bits(a, b) for a, b in zip(srcs, before))      # the sources are only read
    planted = 0
    for a, s, (tab, _), st, (w, key, _) in zip(got, srcs, gather_tables, stats, ARRAYS):
        x = s if idx is None else s[idx]
        assert a.shape == (3 * rows,) + tuple(s.shape[1:])
        for k in range(3):
            y = x if (k == 0 or tab is None) else sy.apply(x, tab[k - 1])
            if st is not None:                                              # the torch expression, and the existing normalising gather on the transformed rows
                t = y.contiguous()
                y = torch.clamp((t - st[0]) * st[1], -CLIP, CLIP)
                assert same_bits(pk.gather_rows([t], None, norm=[st])[0], y)
            assert same_bits(a[k * rows:(k + 1) * rows], y), (w, key, k)
            planted += int((~torch.isfinite(y)).sum())
    assert planted > 0 or rows < 3
    # no table anywhere: three copies of the plain gather
    if idx is not None:
        for a, s in zip(pk.gather_rows_sym(srcs, idx, [None] * 8), srcs):
            assert same_bits(a, s[idx].repeat(3, *([1] * (s.dim() - 1))))


def test_gather_rows_sym_refuses_what_it_cannot_stage(hip):
    x = torch.zeros(4, 130, device=DEV)
    t = torch.zeros(2, 130, 4, dtype=torch.int32, device=DEV)
    with pytest.raises(ValueError, match="128"):
        pk.gather_rows_sym([x], None, [t])
    with pytest.raises(ValueError, match="another shape"):
        pk.gather_rows_sym([x[:, :9].contiguous()], None, [t])
    lib = pk.load()
    p = 4096                                                               # never dereferenced: refused on the host
    vp_ = lambda *a: (pk.C.c_void_p * len(a))(*a)                         # noqa: E731
    ip = lambda *a: (pk.C.c_int32 * len(a))(*a)                           # noqa: E731
    assert lib.tfp_gather_rows_sym(vp_(p), vp_(p), ip(130), None, None, None, vp_(p), 1, None, 4, None) == -4
    assert lib.tfp_gather_rows_sym(vp_(*[p] * 5), vp_(*[p] * 5), ip(*[120] * 5), None, None, None, vp_(*[p] * 5), 5, None, 4, None) == -4
    assert lib.tfp_gather_rows_sym(vp_(p), vp_(p), ip(9), None, None, None, vp_(p + 4), 1, None, 4, None) == -1
    assert lib.tfp_gather_rows_sym(vp_(p), vp_(p), ip(9), None, None, None, None, 1, None, 0, None) == -1
    assert lib.tfp_ppo_loss_sym(p, p, p, p, p, p, p, p, None, 0, 0, 8, 9, 0.2, 1.0, 0.0, 0.0, p, p, p, p, p, None) == -1       # kl_rows 0
    assert lib.tfp_ppo_loss_sym(p, p, p, p, p, p, p, p, None, 0, 9, 8, 9, 0.2, 1.0, 0.0, 0.0, p, p, p, p, p, None) == -1       # kl_rows > B
    assert lib.tfp_ppo_loss_sym(p, p, p, p, p + 4, p, p, p, None, 1, 4, 8, 9, 0.2, 1.0, 0.0, 0.0, p, p, p, p, p, None) == -1   # (adv, w) pairs: 8-byte aligned


# ---- tfp_ppo_loss_sym ------------------------------------------------------------------------------------------------------------------------
ARGS = dict(e_clip=E_CLIP, v_coef=2.0, ent_coef=0.003, bounds_coef=1e-4)


def reference64(mu, ls, v, act, old_nlp, adv, ret, old_mu, old_v, w, kl_rows, e_clip, v_coef, ent_coef, bounds_coef):
    """the objective of csrc/ppo_kernels.hip in the dtype of its inputs, every per-sample term times w_i, divisor B; the KL statistic over the first kl_rows
    rows alone, divisor kl_rows"""
    wm = lambda x: (w * x).mean()                                         # noqa: E731
    ratio = (old_nlp - neglogp(act, mu, ls.expand_as(mu))).exp()
    a_loss = wm(torch.max(-adv * ratio, -adv * ratio.clamp(1 - e_clip, 1 + e_clip)))
    c_loss = wm(ppo.clipped_value_loss(v, ret, old_v, e_clip) if old_v is not None else (v - ret).pow(2))
    b_loss = wm(((mu - 1.1).clamp(min=0).pow(2) + (-1.1 - mu).clamp(min=0).pow(2)).sum(-1))
    ent = (ls + 0.5 + 0.5 * math.log(2 * math.pi)).sum()
    kl = (w * (0.5 * ((mu - old_mu) / ls.exp()).pow(2)).sum(-1))[:kl_rows].mean()
    return a_loss + v_coef * c_loss - ent_coef * ent + bounds_coef * b_loss, a_loss, c_loss, kl


@pytest.mark.parametrize("A", [9, 18])
@pytest.mark.parametrize("B", [3, 192, 771])
@pytest.mark.parametrize("weighted", [False, True], ids=["plain", "w"])
@pytest.mark.parametrize("vclip", [False, True], ids=["plain", "vclip"])
def test_objective_with_a_kl_row_count(hip, B, A, vclip, weighted):
    """kl_rows = B: the entry point (old_v, weighted) selects - d_mu and d_v bit for bit at every size, the sums (one atomic per block of 256 samples)
    bit for bit up to two blocks and within the tolerances beyond, as tests/test_episode_ends_gpu.py::test_weighted_objective asks of w = 1.  kl_rows =
    B / 3 (257 of 771: past the first block) against the float64 objective, tolerances of tests/test_value_path_gpu.py quantity for quantity"""
    mu0, ls0, v0, act, old_nlp, adv, ret, old_mu, old_v = vp.objective_inputs(B, A)
    w = (torch.rand(B, generator=torch.Generator().manual_seed(B + A)) >= 0.25).float().to(DEV) if weighted else torch.ones(B, device=DEV)
    kw = {"old_v": old_v} if vclip else {}
    if weighted:
        kw["adv_w"] = torch.stack([adv, w], 1).contiguous()

    def run(**extra):
        s = torch.zeros(4, device=DEV)
        return pk.ppo_loss_and_grads(mu0, ls0, v0, act, old_nlp, None if weighted else adv, ret, old_mu, s, **kw, **extra, **ARGS) + (s,)
    loss0, d_mu0, d_v0, d_ls0, s0 = run()
    loss1, d_mu1, d_v1, d_ls1, s1 = run(kl_rows=B)
    assert torch.equal(d_mu0, d_mu1) and torch.equal(d_v0, d_v1)
    if (B + 255) // 256 <= 2:
        assert torch.equal(loss0, loss1) and torch.equal(d_ls0, d_ls1) and torch.equal(s0, s1)
    else:
        assert torch.allclose(loss0, loss1, rtol=2e-5, atol=1e-6) and torch.allclose(s0, s1, rtol=2e-5, atol=1e-6) and torch.allclose(d_ls0, d_ls1, rtol=2e-4, atol=1e-7)
    K = B // 3
    d = lambda t: t.double()                                              # noqa: E731
    mu, ls, v = (d(t).clone().requires_grad_(True) for t in (mu0, ls0, v0))
    loss, a_loss, c_loss, kl = reference64(mu, ls, v, d(act), d(old_nlp), d(adv), d(ret), d(old_mu), d(old_v) if vclip else None, d(w), K, **ARGS)
    loss.backward()
    want = torch.stack([loss.detach(), a_loss.detach(), c_loss.detach(), kl.detach()]).float()
    got_loss, d_mu, d_v, d_ls, stats = run(kl_rows=K)
    assert torch.equal(d_mu, d_mu0) and torch.equal(d_v, d_v0)             # the row count touches the statistic alone
    assert torch.allclose(loss.detach().float(), got_loss, rtol=2e-5, atol=1e-6)
    assert torch.allclose(want, stats, rtol=2e-5, atol=1e-6), (want.tolist(), stats.tolist())
    assert torch.allclose(mu.grad.float(), d_mu, rtol=1e-4, atol=1e-9) and torch.allclose(v.grad.float(), d_v, rtol=1e-5, atol=1e-10)
    assert torch.allclose(ls.grad.float(), d_ls, rtol=2e-4, atol=1e-7)
    if B >= 192:                                                           # the statistic of the first third is not that of the whole
        assert abs(float(stats[3]) - float(s0[3])) > 1e-4 * float(s0[3])
    with pytest.raises(ValueError, match="kl_rows"):
        run(kl_rows=B + 1)


# ---- equivariance on the HIP engine ------------------------------------------------------------------------------------------------------------
def test_the_step_is_equivariant_on_the_hip_engine(hip):
    tabs = sy.trifinger_symmetry(9, True)
    obs, states, rew, ok = su.scenario(hip, DEV)
    assert int(ok.sum()) >= su.HALF // 4, int(ok.sum())
    err = su.errors(obs, states, rew, ok, tabs)
    print("equivariance on the HIP engine:", int(ok.sum()), "pairs", err)
    for key, bound in su.BOUNDS.items():
        assert err[key] <= bound, (key, err[key], bound)
    obs, states, rew, ok = su.scenario(hip, DEV, sense=+1.0)
    assert int(ok.sum()) >= su.HALF // 4 and su.errors(obs, states, rew, ok, tabs)["obs"] > 0.05


# ---- the trainer on the HIP env --------------------------------------------------------------------------------------------------------------
N, T = 64, 4


def hip_trainer(**kw):
    from leibnizgym_amd.config import gym_config
    from leibnizgym_amd.envs import TrifingerEnv
    from leibnizgym_amd.utils.rlg_train import RlGamesGpuEnvAdapter
    from leibnizgym_amd.wrappers import VecTaskPython
    cfg = gym_config("trifinger_difficulty_4")
    cfg.update(num_instances=N, seed=1, physics_engine="physx", asymmetric_obs=True, episode_length=6)
    env = TrifingerEnv(config=cfg, device=DEV, verbose=False)
    ad = RlGamesGpuEnvAdapter("rlgpu", N, env=VecTaskPython(env, rl_device=DEV))
    return PPOTrainer(ad, 41, 113, 9, PPOConfig(horizon=T, minibatches=2, mini_epochs=2, **kw), device=DEV)


class CountingLib:
    """the loaded library with every call through it counted by entry point"""

    def __init__(self, lib):
        self._lib, self.calls = lib, []

    def __getattr__(self, name):
        fn = getattr(self._lib, name)
        if not name.startswith("tfp_"):
            return fn

        def counted(*a):
            self.calls.append(name)
            return fn(*a)
        return counted


def test_one_epoch_on_the_hip_env(hip, monkeypatch):
    keys = dict(normalize_input=True, normalize_input_value=True, clip_value_central=True)
    lib = CountingLib(pk.load())
    monkeypatch.setattr(pk, "_LIB", lib)
    steps = {}
    for on in (False, True):
        tr = hip_trainer(symmetry_augmentation=on, **keys)
        assert tr.fused_loss and (tr.sym is not None) == on
        buf = tr.rollout()
        flat = lambda x: x.reshape(T * N, *x.shape[2:])                   # noqa: E731
        a = flat(buf["adv"])
        d = dict(obs=flat(buf["obs"]), states=flat(buf["states"]), act=flat(buf["act"]), old_nlp=flat(buf["nlp"]), ret=flat(buf["ret"]),
                 adv=(a - a.mean()) / (a.std() + 1e-8), old_mu=flat(buf["mu"]), old_v=flat(buf["val"][:T]))
        idx = torch.randperm(T * N, device=DEV)[:T * N // 2]
        del lib.calls[:]
        tr._mb_backward(d, idx, tr._new_acc(DEV))
        tr._mb_apply()
        steps[on] = list(lib.calls)
        if on:                                                              # ... and the epoch: finite statistics, the gap among them
            st = tr.update(buf)
            assert all(math.isfinite(st[k]) for k in ("loss", "a_loss", "c_loss", "kl", "mean_reward", "symmetry_gap")) and st["symmetry_gap"] >= 0.0
            st = tr.train(1)[0]
            assert all(math.isfinite(st[k]) for k in ("loss", "a_loss", "c_loss", "kl", "symmetry_gap"))
            assert all(bool(torch.isfinite(p).all()) for p in tr.net.parameters())
    # the fused step keeps its launch count: the same calls, the augmenting gather and the objective with a KL row count in place of theirs
    rename = {"tfp_gather_rows_sym": "tfp_gather_rows_norm", "tfp_ppo_loss_sym": "tfp_ppo_loss_vclip"}
    assert [rename.get(c, c) for c in steps[True]] == steps[False], (steps[True], steps[False])
    assert steps[True].count("tfp_gather_rows_sym") == 1 and steps[True].count("tfp_ppo_loss_sym") == 1 and "tfp_gather_rows_sym" not in steps[False]


def test_the_key_off_is_reproducible_and_builds_nothing(hip, monkeypatch):
    """two trainers from the same seed, key off: the epoch's statistics are EQUAL, and nothing of the symmetry path runs.  Equality needs a trainer that is
    reproducible to begin with: the optimiser's squared gradient norms are float atomics over ~260 workgroups in arrival order (csrc/ppo_kernels.hip:
    k_grad_sqnorms), so wherever the truncation bites its coefficient moves in the last bit from run to run, with or without this feature (seen here: `loss`
    1.5630348920822144 against 1.563035011291504 with every other statistic equal).  With `truncate_grads: False` on both optimisers the coefficient is exactly
    1 whatever the sums are; every other launch of the epoch is order-free at this size (one block of the objective per minibatch, fixed-order chunk sums)"""
    def boom(*a, **k):
        raise AssertionError("a function of the symmetry path ran with the key off")
    for name in ("trifinger_symmetry", "apply", "pack"):
        monkeypatch.setattr(sy, name, boom)
    monkeypatch.setattr(pk, "gather_rows_sym", boom)
    out = []
    for _ in range(2):
        tr = hip_trainer(truncate_grads=False, value_truncate_grads=False)
        assert tr.sym is None
        out.append(tr.train(1)[0])
    assert "symmetry_gap" not in out[0] and out[0] == out[1] and math.isfinite(out[0]["loss"])


def test_kernels_and_torch_path_agree_with_the_key_on(hip):
    """one minibatch step of all T n samples, kernels against the torch path: the tolerance of tests/test_ppo_kernels.py::test_trainer_with_and_without_the_kernels"""
    keys = dict(symmetry_augmentation=True, normalize_input=True, normalize_input_value=True, episode_ends=True)
    tr, ref = hip_trainer(**keys), hip_trainer(fused_kernels=False, **keys)
    assert tr.fused_loss and not ref.fused_loss and all(torch.equal(a, b) for a, b in zip(tr.net.parameters(), ref.net.parameters()))
    buf = tr.rollout()
    flat = lambda x: x.reshape(T * N, *x.shape[2:])                       # noqa: E731
    wf = flat(buf["w"])
    a_n = ppo.masked_advantage_norm(flat(buf["adv"]), wf)
    d = dict(obs=flat(buf["obs"]), states=flat(buf["states"]), act=flat(buf["act"]), old_nlp=flat(buf["nlp"]), ret=flat(buf["ret"]), adv=a_n,
             old_mu=flat(buf["mu"]) + 0.01, w=wf, adv_w=torch.stack([a_n, wf], dim=1))
    idx = torch.randperm(T * N, device=DEV)
    before = [p.detach().clone() for p in tr.net.parameters()]
    accs = []
    for t in (tr, ref):
        accs.append(t._new_acc(DEV))
        t._mb_backward(d, idx, accs[-1])
        t._mb_apply()
    for a, b, c in zip(tr.net.parameters(), ref.net.parameters(), before):
        assert torch.allclose(a, b, atol=3e-5, rtol=1e-3) and not torch.equal(a, c)
    for k in ("loss", "a_loss", "c_loss", "kl"):
        x, y = float(accs[0][k]), float(accs[1][k])
        assert abs(x - y) < 1e-3 * max(1.0, abs(y)), (k, x, y)
    assert float(accs[1]["kl"]) > 0.0
    assert float(tr._symmetry_gap()) == pytest.approx(float(ref._symmetry_gap()), rel=1e-3, abs=1e-6)
