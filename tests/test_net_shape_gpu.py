"""The network-shape keys on the hand-written kernels: the extended network walk of csrc/ppo_mlp_walk.hip (include/trifinger_ppo_net.h: activation codes,
d2rl, statistics) against float64 torch, and the trainer on top of it.  The CPU side of the same keys is tests/test_net_shape.py."""
import pytest
import torch
import torch.nn.functional as F

from leibnizgym_amd import ppo_kernels as pk
from leibnizgym_amd.ppo import PPOConfig

SELU_L, SELU_A = 1.0507009873554805, 1.6732632423543772
# code -> (forward in float64, derivative from the OUTPUT y): the table of include/trifinger_ppo_net.h
ACTS = {"None": (0, lambda v: v, lambda y: torch.ones_like(y)),
        "elu": (1, F.elu, lambda y: torch.where(y > 0, torch.ones_like(y), y + 1)),
        "relu": (2, torch.relu, lambda y: (y > 0).to(y.dtype)),
        "tanh": (3, torch.tanh, lambda y: 1 - y * y),
        "sigmoid": (4, torch.sigmoid, lambda y: y * (1 - y)),
        "selu": (5, torch.selu, lambda y: torch.where(y > 0, torch.full_like(y, SELU_L), y + SELU_L * SELU_A)),
        "softplus": (6, F.softplus, lambda y: 1 - torch.exp(-y))}
SHAPES = [(77, [7, 33, 64, 5], [20, 416, 17, 3]), (130, [41, 400, 200, 100, 9], [113, 400, 200, 100, 1])]


def wide(dims, l, d2rl):
    """input width of layer l"""
    return dims[l] + (dims[0] if (d2rl and 1 <= l <= len(dims) - 3) else 0)


def make_net(dims, act, d2rl, gen, dev="cpu", grads=True):
    """(x, layers, gy): weights randn * fan_in^-0.5, biases 0.3 randn; the first eight output columns of the first layer carry ten times the weight, so
    their pre-activations reach |v| ~ 30 (tanh, sigmoid and softplus saturate there)"""
    n = len(dims) - 1
    layers = pk.LayerList()
    layers.d2rl = d2rl
    for i in range(n):
        k = wide(dims, i, d2rl)
        w = torch.randn(dims[i + 1], k, generator=gen) * k ** -0.5
        if i == 0 and n > 1:
            w[:8] *= 10.0
        b = torch.randn(dims[i + 1], generator=gen) * 0.3
        go = (torch.zeros(dims[i + 1], k, device=dev), torch.zeros(dims[i + 1], device=dev)) if grads else None
        layers.append((w.to(dev), b.to(dev), ACTS[act][0] if i < n - 1 else 0, go))
    return layers


def rows(M, d, gen, dev):
    return torch.randn(M, d, generator=gen).to(dev)


def reference_forward(x, layers, act):
    """float64: the list of what the walk stores per layer ([h | x] where the next layer of a d2rl network reads it) and the pre-activations"""
    f, x64, n, d2rl = ACTS[act][1], x.double(), len(layers), pk._d2rl(layers)
    inp, outs, pre = x64, [], []
    for l, (w, b, _, _) in enumerate(layers):
        v = inp @ w.double().t() + b.double()
        pre.append(v)
        h = f(v) if l < n - 1 else v
        inp = torch.cat([h, x64], dim=1) if (d2rl and l <= n - 3) else h
        outs.append(inp)
    return outs, pre


def reference_backward(x, layers, act, stored, gy):
    """float64 dZ chain with act' formed FROM THE OUTPUTS THE WALK STORED (as the kernel forms it: a pre-activation within rounding of a kink cannot flip
    a chain), over the hidden part of the wide weights; dW_l = dZ_l^T input_l (the wide rows), db_l = column sums"""
    der, n = ACTS[act][2], len(layers)
    dz = [None] * n
    dz[n - 1] = gy.double()
    for l in range(n - 1, 0, -1):
        N = layers[l - 1][0].shape[0]
        dz[l - 1] = (dz[l] @ layers[l][0].double()[:, :N]) * der(stored[l - 1].double()[:, :N])
    gw = [dz[l].t() @ (stored[l - 1].double() if l > 0 else x.double()) for l in range(n)]
    return dz, gw, [d.sum(0) for d in dz]


def close(got, want, what):
    torch.testing.assert_close(got.double(), want, rtol=2e-5, atol=2e-5, msg=lambda m: f"{what}: {m}")


def check_pair(M, dims_a, dims_c, act_a, act_c, d2rl_a, d2rl_c, seed):
    """forward, dZ chain and parameter gradients of two networks in one launch per direction against float64"""
    dev = "cuda:0"
    gen = torch.Generator().manual_seed(seed)
    nets = [(rows(M, d[0], gen, dev), make_net(d, a, k, gen, dev), rows(M, d[-1], gen, dev), a) for d, a, k in ((dims_a, act_a, d2rl_a), (dims_c, act_c, d2rl_c))]
    outs = pk.mlp_walk_forward([(x, layers) for x, layers, _, _ in nets])
    assert outs is not None
    for (x, layers, gy, act), ys in zip(nets, outs):
        want, _ = reference_forward(x, layers, act)
        for l, (y, y64) in enumerate(zip(ys, want)):
            assert y.shape == y64.shape and torch.isfinite(y).all(), f"{act}: output of layer {l}"
            close(y, y64, f"{act}: output of layer {l}")
    dzs = pk.mlp_walk_backward([(gy, ys, layers) for (x, layers, gy, _), ys in zip(nets, outs)])
    assert dzs is not None
    refs = [reference_backward(x, layers, act, ys, gy) for (x, layers, gy, act), ys in zip(nets, outs)]
    for (x, layers, gy, act), dz, (dz64, _, _) in zip(nets, dzs, refs):
        for l, (d, d64) in enumerate(zip(dz, dz64)):
            close(d, d64, f"{act}: dZ of layer {l}")
    (xa, la, gya, _), (xc, lc, gyc, _) = nets
    pk.mlp_backward_pair(xa, outs[0], gya, la, xc, outs[1], gyc, lc)
    pk.flush_partial_sums()
    for (x, layers, gy, act), (_, gw64, gb64) in zip(nets, refs):
        for l, (_, _, _, (gw, gb)) in enumerate(layers):
            assert float((gw.double() - gw64[l]).abs().max()) <= 3e-5 * (float(gw64[l].abs().max()) + 1e-12) + 1e-6, f"{act}: dW of layer {l}"
            assert float((gb.double() - gb64[l]).abs().max()) <= 3e-5 * (float(gb64[l].abs().max()) + 1e-12) + 1e-6, f"{act}: db of layer {l}"
    return nets, outs, dzs


def test_the_test_inputs_keep_away_from_the_kinks():
    """CPU: with this file's scaling at most 0.08 % of a layer's pre-activations lie within 1e-4 of zero (20 seeds), so the comparison of the OUTPUTS with
    float64 is insensitive to the kink of relu / selu (both continuous there anyway); the dZ reference forms act' from the stored outputs"""
    worst = 0.0
    for seed in range(20):
        gen = torch.Generator().manual_seed(seed)
        for M, da, dc in SHAPES:
            for d in (da, dc):
                x, layers = rows(M, d[0], gen, "cpu"), make_net(d, "relu", False, gen, grads=False)
                _, pre = reference_forward(x, layers, "relu")
                worst = max([worst] + [float((v.abs() < 1e-4).double().mean()) for v in pre[:-1]])
    assert worst <= 0.0008, worst


@pytest.mark.gpu
@pytest.mark.parametrize("M,dims_a,dims_c", SHAPES)
@pytest.mark.parametrize("act", ["relu", "tanh", "sigmoid", "selu", "softplus", "None", "elu"])
def test_walk_activations_match_float64(hip, act, M, dims_a, dims_c):
    """every activation code (elu: the control) at the ragged shapes and at the trainer's: all layer outputs, the dZ chain, dW and db"""
    nets, outs, _ = check_pair(M, dims_a, dims_c, act, act, False, False, seed=M + ACTS[act][0])
    if act in ("tanh", "sigmoid", "softplus"):
        _, pre = reference_forward(nets[0][0], nets[0][1], act)
        assert float(pre[0].abs().max()) > 20.0                                       # the saturated range was visited


@pytest.mark.gpu
@pytest.mark.parametrize("M,dims_a,dims_c", SHAPES + [(77, [7, 33, 5], [20, 17, 3])])
@pytest.mark.parametrize("act", ["elu", "tanh"])
def test_d2rl_walk_matches_the_cat_formula(hip, act, M, dims_a, dims_c):
    """d2rl on both networks against the float64 cat formula (outputs with the x columns in place, dZ, dW including its x columns, db); the rollout's form
    gives the same output bits; with statistics the result is the plain d2rl walk on normalize_rows(x), bit for bit"""
    nets, outs, _ = check_pair(M, dims_a, dims_c, act, act, True, True, seed=3 * M + ACTS[act][0])
    pairs = [(x, layers) for x, layers, _, _ in nets]
    for (x, layers), ys in zip(pairs, outs):
        for l in range(len(layers) - 2):
            assert ys[l].shape[1] == layers[l][0].shape[0] + x.shape[1] and torch.equal(ys[l][:, layers[l][0].shape[0]:], x)
    last = pk.mlp_walk_forward(pairs, store_hidden=False)
    for ys, yl in zip(outs, last):
        assert all(y is None for y in yl[:-1]) and torch.equal(yl[-1], ys[-1])
    gen = torch.Generator().manual_seed(M)
    stats = [((torch.randn(x.shape[1], generator=gen) * 0.5).cuda(), (torch.rand(x.shape[1], generator=gen) + 0.5).cuda(), 1.5) for x, _ in pairs]
    for norms in (stats, [stats[0], None]):
        got = pk.mlp_walk_forward(pairs, norms=norms)
        want = pk.mlp_walk_forward([(pk.normalize_rows(x, *nm) if nm is not None else x, layers) for (x, layers), nm in zip(pairs, norms)])
        for ys, yw in zip(got, want):
            assert all(torch.equal(a, b) for a, b in zip(ys, yw))
        only = pk.mlp_walk_forward(pairs, store_hidden=False, norms=norms)
        assert all(torch.equal(a[-1], b[-1]) for a, b in zip(only, want))


@pytest.mark.gpu
def test_what_does_not_fit_is_declined_by_the_query_and_by_the_walk(hip):
    """the forward walk of a d2rl network may take a whole CU's 160 KiB and no more; the query and the launch agree, in both directions"""
    dev = "cuda:0"
    gen = torch.Generator().manual_seed(0)
    big = make_net([416, 416, 416, 64, 4], "tanh", True, gen, dev, grads=False)              # rows of 832 floats: 2 x 107 KB
    fits = make_net([113, 416, 200, 100, 1], "tanh", True, gen, dev, grads=False)            # rows of 529 and 313 floats: 70 + 41 KB, beyond the plain walk's 80 KB
    plain_big = make_net([416, 416, 416, 416, 4], "tanh", False, gen, dev, grads=False)      # 2 x 54 KB: beyond 80 KB without the d2rl allowance
    too_wide = make_net([64, 432, 8], "tanh", False, gen, dev, grads=False)
    assert not pk.net_fits([big]) and pk.mlp_walk_forward([(rows(40, 416, gen, dev), big)]) is None
    assert pk.net_fits([big], backward=True)                                                  # the backward chain holds no wide rows
    assert pk.net_fits([fits]) and pk.net_fits([fits], backward=True)
    out = pk.mlp_walk_forward([(rows(40, 113, gen, dev), fits)])
    assert out is not None and torch.isfinite(out[0][-1]).all()
    assert not pk.net_fits([plain_big]) and pk.mlp_walk_forward([(rows(40, 416, gen, dev), plain_big)]) is None
    assert not pk.net_fits([too_wide]) and not pk.net_fits([too_wide], backward=True)
    x = rows(40, 64, gen, dev)
    assert pk.mlp_walk_forward([(x, too_wide)]) is None
    with pytest.raises(RuntimeError, match="declined"):                                       # never the ELU per-layer kernels for such a network
        pk.mlp_forward_pair(x, too_wide, x, too_wide)


@pytest.mark.gpu
def test_mixed_pair_equals_the_networks_alone(hip):
    """a tanh actor without d2rl beside an elu value network with d2rl, one launch per direction: the bits of each network walked alone"""
    M, (da, dc) = 130, SHAPES[1][1:]
    nets, outs, dzs = check_pair(M, da, dc, "tanh", "elu", False, True, seed=99)
    for (x, layers, gy, _), ys, dz in zip(nets, outs, dzs):
        alone = pk.mlp_walk_forward([(x, layers)])[0]
        assert all(torch.equal(a, b) for a, b in zip(alone, ys))
        dz_alone = pk.mlp_walk_backward([(gy, ys, layers)])[0]
        assert all(torch.equal(a, b) for a, b in zip(dz_alone, dz))


@pytest.mark.gpu
def test_elu_networks_get_the_old_bits_from_the_new_entry_points(hip):
    """act in {0, 1}: tfp_net_forward / tfp_net_backward return what tfp_mlp_forward / tfp_mlp_forward_norm / tfp_mlp_backward return"""
    M, (da, dc) = 130, SHAPES[1][1:]
    dev = "cuda:0"
    gen = torch.Generator().manual_seed(5)
    nets = [(rows(M, d[0], gen, dev), make_net(d, "elu", False, gen, dev, grads=False), rows(M, d[-1], gen, dev)) for d in (da, dc)]
    assert not any(pk.needs_net_walk(layers) for _, layers, _ in nets)
    pairs = [(x, layers) for x, layers, _ in nets]
    old, new = pk.mlp_walk_forward(pairs, ext=False), pk.mlp_walk_forward(pairs, ext=True)
    assert all(torch.equal(a, b) for ya, yb in zip(old, new) for a, b in zip(ya, yb))
    norms = [((torch.randn(41, generator=gen) * 0.5).cuda(), (torch.rand(41, generator=gen) + 0.5).cuda(), 5.0), None]
    old_n, new_n = pk.mlp_walk_forward(pairs, norms=norms, ext=False), pk.mlp_walk_forward(pairs, norms=norms, ext=True)
    assert all(torch.equal(a, b) for ya, yb in zip(old_n, new_n) for a, b in zip(ya, yb)) and not torch.equal(old_n[0][-1], old[0][-1])
    back = [(gy, ys, layers) for (_, layers, gy), ys in zip(nets, old)]
    dz_old, dz_new = pk.mlp_walk_backward(back, ext=False), pk.mlp_walk_backward(back, ext=True)
    assert all(torch.equal(a, b) for da_, db_ in zip(dz_old, dz_new) for a, b in zip(da_, db_))


def _trainer(fused, n=256, **kw):
    from leibnizgym_amd.config import gym_config
    from leibnizgym_amd.envs import TrifingerEnv
    from leibnizgym_amd.ppo import PPOTrainer
    from leibnizgym_amd.utils.rlg_train import RlGamesGpuEnvAdapter
    from leibnizgym_amd.wrappers import VecTaskPython
    cfg = gym_config("trifinger_difficulty_4")
    cfg.update(num_instances=n, seed=1, physics_engine="physx", asymmetric_obs=True, episode_length=20)
    env = TrifingerEnv(config=cfg, device="cuda:0", verbose=False)
    ad = RlGamesGpuEnvAdapter("rlgpu", n, env=VecTaskPython(env, rl_device="cuda:0"))
    return PPOTrainer(ad, 41, 113, 9, PPOConfig(horizon=8, minibatches=4, mini_epochs=2, fused_kernels=fused, **kw), device="cuda:0")


@pytest.mark.gpu
@pytest.mark.parametrize("keys", [dict(activation="tanh", d2rl=True, value_d2rl=True), dict(truncate_grads=False, lr_schedule="identity")],
                         ids=["tanh-d2rl", "no-truncation-identity"])
def test_trainer_on_the_kernels_and_on_torch(hip, keys):
    """the set-up of test_trainer_with_and_without_the_kernels (256 envs, horizon 8, 2 epochs = 16 Adam steps) with the new keys: the hand-written path
    takes the optimisation steps of plain torch, parameters within atol 3e-5 / rtol 1e-3, statistics within 1e-3 relative.  The margin is smallest for
    `tanh-d2rl`: Adam is scale-free, so rounding-level differences in elements of the wide weights whose gradient is small come back as full-size steps
    (DESIGN.md section 4 has the CPU sensitivity figures); the kernel's tanh is kept close to torch's for that reason."""
    def run(fused):
        tr = _trainer(fused, **keys)
        assert tr.fused_loss == fused and tr.torch_path_reason is None
        torch.manual_seed(11)
        stats = tr.train(2)
        return [p.detach().clone() for p in tr.net.parameters()], stats
    plain, s0 = run(False)
    fused, s1 = run(True)
    for a, b in zip(plain, fused):
        assert torch.allclose(a, b, atol=3e-5, rtol=1e-3)
    for k in ("loss", "a_loss", "c_loss", "kl"):
        assert abs(s0[-1][k] - s1[-1][k]) < 1e-3 * max(1.0, abs(s0[-1][k])), (k, s0[-1][k], s1[-1][k])
    if keys.get("lr_schedule") == "identity":
        assert s1[-1]["lr"] == 3e-4


@pytest.mark.gpu
def test_trainer_takes_the_torch_path_with_one_message(hip, capsys):
    """swish has no kernel; a d2rl network the walk declines has no per-layer fallback: both construct, say so once, and train on plain torch"""
    tr = _trainer(True, activation="swish")
    out = capsys.readouterr().out
    assert out.count("plain torch path") == 1 and "swish" in out
    assert not tr.fused_loss and tr.flat_opt is None and not tr.net.actor.mfma
    assert len(tr.train(1)) == 1
    # units [416, 416, 416] on the 113-wide input: the forward rows of 529 floats (2 x 70 KB) fit a CU, the two 416-wide dZ buffers of the backward walk
    # (2 x 54 KB) do not fit its 80 KB - and a d2rl network has no per-layer fallback
    tr = _trainer(True, n=64, units=[416, 416, 416], d2rl=True, value_d2rl=True)
    la, lc = tr.net.actor.layer_list(), tr.net.critic.layer_list()
    assert pk.net_fits([la, lc]) and not pk.net_fits([la, lc], backward=True)
    out = capsys.readouterr().out
    assert out.count("plain torch path") == 1 and "declines" in out and not tr.fused_loss
    stats = tr.train(1)
    assert len(stats) == 1 and all(torch.isfinite(p).all() for p in tr.net.parameters())
