"""`params.config.mixed_precision` on the hand-written kernels (include/trifinger_ppo_mixed.h): the network walk and the direct weight-gradient kernel with bf16
operands against float64 products of the ROUNDED operands (the statement: leibnizgym_amd/ppo.py `_MixedLinear`), and the trainer on top of them.  The CPU side is
tests/test_mixed_precision.py.

Every reference is chained layer by layer FROM THE KERNEL'S OWN STORED OUTPUTS AND dZ: a last-ulp difference upstream can flip a bf16 rounding downstream, which
is not an error of the layer under test.  Tolerances are the project's own for the fp32 kernels - rtol 2e-5 / atol 2e-5 for outputs and dZ, 3e-5 max |want| + 1e-6
for dW and db (tests/test_ppo_kernels.py) -: products of bf16 values are exact in fp32, so only the accumulation differs, and it can be no worse than that of a
product of fp32 operands.  Every test prints the worst error it saw before it asserts."""
import pytest
import torch
import torch.nn.functional as F

import minibatch_step_util as msu
from leibnizgym_amd import ppo_kernels as pk
from leibnizgym_amd.ppo import PPOConfig, PPOTrainer, bf16r

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SELU_L, SELU_A = 1.0507009873554805, 1.6732632423543772
# name -> (code, forward in float64, derivative from the OUTPUT y): the table of include/trifinger_ppo_net.h
ACTS = {"None": (0, lambda v: v, lambda y: torch.ones_like(y)),
        "elu": (1, F.elu, lambda y: torch.where(y > 0, torch.ones_like(y), y + 1)),
        "relu": (2, torch.relu, lambda y: (y > 0).to(y.dtype)),
        "tanh": (3, torch.tanh, lambda y: 1 - y * y),
        "sigmoid": (4, torch.sigmoid, lambda y: y * (1 - y)),
        "selu": (5, torch.selu, lambda y: torch.where(y > 0, torch.full_like(y, SELU_L), y + SELU_L * SELU_A)),
        "softplus": (6, F.softplus, lambda y: 1 - torch.exp(-y))}
# ragged first-layer K, K % 32 in {4, 8, 16, 0}, N % 16 != 0, M % 32 != 0, one network alone, one-layer networks, more blocks than one round
SHAPES = [(77, [7, 33, 64, 5], [20, 416, 17, 3]), (64, [16, 16], [3, 1]), (130, [41, 400, 200, 100, 9], None),
          (96, [41, 400, 200, 100, 18], [113, 400, 200, 100, 1]), (1000, [41, 400, 200, 100, 9], [113, 400, 200, 100, 1])]
FP32_WALK = ("tfp_mlp_forward", "tfp_mlp_forward_norm", "tfp_net_forward", "tfp_mlp_backward", "tfp_net_backward", "tfp_gemm_tn_partials_direct")
BF16 = ("tfp_net_forward_bf16", "tfp_net_backward_bf16", "tfp_gemm_tn_partials_direct_bf16")


def r64(t):
    return bf16r(t).double()


def make_net(dims, act, d2rl, gen):
    n = len(dims) - 1
    layers = pk.LayerList()
    layers.d2rl, layers.mixed = d2rl, True
    for i in range(n):
        k = dims[i] + (dims[0] if (d2rl and 1 <= i <= n - 2) else 0)
        w = (torch.randn(dims[i + 1], k, generator=gen) * k ** -0.5).to(DEV)
        b = (torch.randn(dims[i + 1], generator=gen) * 0.3).to(DEV)
        layers.append((w, b, ACTS[act][0] if i < n - 1 else 0, (torch.zeros(dims[i + 1], k, device=DEV), torch.zeros(dims[i + 1], device=DEV))))
    return layers


def close(got, want, what, worst):
    err = float((got.double() - want).abs().max())
    worst[0] = max(worst[0], err / (float(want.abs().max()) + 1e-30))
    torch.testing.assert_close(got.double(), want, rtol=2e-5, atol=2e-5, msg=lambda m: f"{what}: {m}")


def check_forward(x, layers, act, ys, worst):
    """every stored output against the float64 statement on the kernel's own stored input of that layer ([h | x] where a d2rl layer reads it)"""
    f, n = ACTS[act][1], len(layers)
    for l, (w, b, _, _) in enumerate(layers):
        inp = x if l == 0 else ys[l - 1]
        v = r64(inp) @ r64(w).t() + b.double()
        h = f(v) if l < n - 1 else v
        assert torch.isfinite(ys[l]).all()
        close(ys[l][:, :w.shape[0]], h, f"{act}: output of layer {l}", worst)
        if ys[l].shape[1] > w.shape[0]:
            assert torch.equal(ys[l][:, w.shape[0]:], x), "the x columns of a d2rl operand"


def check_backward(x, layers, act, ys, gy, dz, worst):
    """every dZ against the statement on the kernel's own dZ of the layer above, act' from the stored output; returns the float64 (dW, db) of every layer from
    the kernel's own dZ and stored inputs: dW = bf16r(dZ)^T bf16r(input), db = the column sums of the UN-ROUNDED dZ"""
    der, n = ACTS[act][2], len(layers)
    assert dz[n - 1] is gy or torch.equal(dz[n - 1], gy)
    for l in range(n - 1, 0, -1):
        N = layers[l - 1][0].shape[0]
        want = (r64(dz[l]) @ r64(layers[l][0])[:, :N]) * der(ys[l - 1].double()[:, :N])
        close(dz[l - 1], want, f"{act}: dZ of layer {l - 1}", worst)
    return [(r64(dz[l]).t() @ r64(ys[l - 1] if l > 0 else x), dz[l].double().sum(0)) for l in range(n)]


def check_grads(layers, want, what, worst):
    for l, ((_, _, _, (gw, gb)), (gw64, gb64)) in enumerate(zip(layers, want)):
        for got, w64, name in ((gw, gw64, "dW"), (gb, gb64, "db")):
            err, top = float((got.double() - w64).abs().max()), float(w64.abs().max())
            worst[0] = max(worst[0], err / (top + 1e-30))
            assert err <= 3e-5 * top + 1e-6, f"{what}: {name} of layer {l}: max |got - want| {err:.3e}, max |want| {top:.3e}"


def run_walk(M, dims_a, dims_c, act, d2rl, seed):
    gen = torch.Generator().manual_seed(seed)
    nets = [(torch.randn(M, d[0], generator=gen).to(DEV), make_net(d, act, d2rl, gen), torch.randn(M, d[-1], generator=gen).to(DEV))
            for d in (dims_a, dims_c) if d is not None]
    before = dict(pk.n_calls)
    outs = pk.forward_nets([(x, layers) for x, layers, _ in nets])
    w_out, w_dz, w_g = [0.0], [0.0], [0.0]
    for (x, layers, _), ys in zip(nets, outs):
        check_forward(x, layers, act, ys, w_out)
    dzs = pk.mlp_walk_backward([(gy, ys, layers) for (x, layers, gy), ys in zip(nets, outs)], mixed=True)
    assert dzs is not None
    want = [check_backward(x, layers, act, ys, gy, dz, w_dz) for (x, layers, gy), ys, dz in zip(nets, outs, dzs)]
    pk.backward_nets([(x, ys, gy, layers) for (x, layers, gy), ys in zip(nets, outs)])
    pk.flush_partial_sums()
    for (x, layers, _), w in zip(nets, want):
        check_grads(layers, w, act, w_g)
    print(f"M {M} {dims_a} {dims_c} {act} d2rl {d2rl}: worst error / max |want|: outputs {w_out[0]:.2e}, dZ {w_dz[0]:.2e}, dW and db {w_g[0]:.2e}")
    after = pk.n_calls
    assert after.get(BF16[0], 0) == before.get(BF16[0], 0) + 1 and after.get(BF16[1], 0) == before.get(BF16[1], 0) + 2
    assert after.get(BF16[2], 0) > before.get(BF16[2], 0) and after.get("n_mixed_dw_torch", 0) == before.get("n_mixed_dw_torch", 0)
    assert all(after.get(k, 0) == before.get(k, 0) for k in FP32_WALK)
    return nets, outs


@pytest.mark.parametrize("M,dims_a,dims_c", SHAPES)
def test_walk_and_weight_gradients_match_float64_of_the_rounded_operands(hip, M, dims_a, dims_c):
    """forward, dZ chain, dW and db at every shape (ELU); measured on MI355X: see the printed line and DESIGN.md section 4"""
    nets, outs = run_walk(M, dims_a, dims_c, "elu", False, seed=M)
    # the mode is on: the fp32 walk on the same network differs - on the first layer by at most (2^-7 + 2^-16) |x| |W|^T (ELU is 1-Lipschitz: the bound on the
    # pre-activations holds for the outputs) plus the fp32 kernels' own tolerance
    (x, layers, _), ys = nets[0], outs[0]
    y32 = pk.forward_nets([(x, pk.LayerList(layers))])[0]
    assert not torch.equal(y32[0], ys[0])
    bound = (2.0 ** -7 + 2.0 ** -16) * (x.double().abs() @ layers[0][0].double().abs().t()) + 2e-5
    assert bool(((y32[0].double() - ys[0].double()).abs() <= bound).all())


@pytest.mark.parametrize("act", ["relu", "tanh", "sigmoid", "selu", "softplus", "None"])
def test_every_activation_code_once(hip, act):
    run_walk(*SHAPES[0], act, False, seed=7 + ACTS[act][0])


def test_d2rl_is_not_declined(hip):
    """the bf16 walk takes d2rl networks (LDS stays fp32: the fp32 walk's budget): the [h | x] operand rounded elementwise"""
    M, da, dc = SHAPES[3]
    gen = torch.Generator().manual_seed(5)
    la, lc = make_net(da, "elu", True, gen), make_net(dc, "tanh", True, gen)
    assert pk.net_fits([la, lc], False, mixed=True) and pk.net_fits([la, lc], True, mixed=True)
    run_walk(M, da, dc, "tanh", True, seed=21)
    run_walk(77, [7, 33, 64, 5], [20, 416, 17, 3], "elu", True, seed=22)


def test_store_hidden_statistics_and_row_independence(hip):
    gen = torch.Generator().manual_seed(9)
    M, da, dc = SHAPES[0]
    pairs = [(torch.randn(M, d[0], generator=gen).to(DEV), make_net(d, "elu", False, gen)) for d in (da, dc)]
    outs = pk.forward_nets(pairs)
    last = pk.forward_nets(pairs, store_hidden=False)                                  # the rollout's form: the same output bits
    for ys, yl in zip(outs, last):
        assert all(y is None for y in yl[:-1]) and torch.equal(yl[-1], ys[-1])
    # statistics: formed in fp32 where the rows are staged, then rounded as the operand - the bits of the walk on normalize_rows(x), and the statement on it
    stats = [((torch.randn(x.shape[1], generator=gen) * 0.5).to(DEV), (torch.rand(x.shape[1], generator=gen) + 0.5).to(DEV), 1.5) for x, _ in pairs]
    for norms in (stats, [stats[0], None]):
        got = pk.forward_nets(pairs, norms=norms)
        xn = [pk.normalize_rows(x, *nm) if nm is not None else x for (x, _), nm in zip(pairs, norms)]
        want = pk.forward_nets([(x, layers) for x, (_, layers) in zip(xn, pairs)])
        worst = [0.0]
        for ys, yw, x, (_, layers) in zip(got, want, xn, pairs):
            assert all(torch.equal(a, b) for a, b in zip(ys, yw))
            check_forward(x, layers, "elu", ys, worst)
    # row independence: the forward of row-permuted input is the permuted forward, bit for bit (M = 1000: 32 blocks per network)
    M, da, dc = SHAPES[4]
    pairs = [(torch.randn(M, d[0], generator=gen).to(DEV), make_net(d, "elu", False, gen)) for d in (da, dc)]
    perm = torch.randperm(M, generator=gen).to(DEV)
    outs = pk.forward_nets(pairs)
    outs_p = pk.forward_nets([(x[perm].contiguous(), layers) for x, layers in pairs])
    for ys, yp in zip(outs, outs_p):
        assert all(torch.equal(y[perm], p) for y, p in zip(ys, yp))


# the eight weight-gradient products of the trainer's step: (N1, N2) of actor and central value network
DW = [(400, 41), (200, 400), (100, 200), (9, 100), (400, 113), (200, 400), (100, 200), (1, 100)]


@pytest.mark.parametrize("rows", [77, 1000, 2100])
def test_direct_weight_gradients(hip, rows):
    """[bf16r(dZ)^T bf16r(X) | column sums of the UN-ROUNDED dZ] at the eight trainer shapes: less than a slab, one slab short of full, three slabs with a
    ragged last one; the same call twice gives identical bits"""
    gen = torch.Generator().manual_seed(rows)
    a = [torch.randn(rows, n1, generator=gen).to(DEV) for n1, _ in DW]
    b = [torch.randn(rows, n2, generator=gen).to(DEV) for _, n2 in DW]
    runs = []
    for _ in range(2):
        outs = [(torch.full((n1, n2), 7.0, device=DEV), torch.full((n1,), 7.0, device=DEV)) for n1, n2 in DW]
        assert pk.gemm_tn_bias_direct(a, b, outs, mixed=True)
        pk.flush_partial_sums()
        runs.append(outs)
    worst = [0.0, 0.0]
    for k, (x, y, (gw, gb)) in enumerate(zip(a, b, runs[0])):
        want_w, want_b = r64(x).t() @ r64(y), x.double().sum(0)
        for i, (got, want, name) in enumerate(((gw, want_w, "dW"), (gb, want_b, "db"))):
            err, top = float((got.double() - want).abs().max()), float(want.abs().max())
            worst[i] = max(worst[i], err / top)
            assert err <= 3e-5 * top + 1e-6, f"rows {rows}, product {DW[k]}: {name}: max |got - want| {err:.3e}, max |want| {top:.3e}"
        assert float((r64(x).sum(0) - want_b).abs().max()) > 3e-5 * float(want_b.abs().max()) + 1e-6      # ... which the sums of the ROUNDED dZ would miss
    print(f"rows {rows}: worst error / max |want|: dW {worst[0]:.2e}, db {worst[1]:.2e}")
    assert all(torch.equal(p, q) and torch.equal(s, t) for (p, s), (q, t) in zip(*runs))


N, T = 128, 8


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


def test_trainer_runs_on_the_bf16_kernels(hip):
    tr = hip_trainer(mixed_precision=True)
    assert tr.torch_path_reason is None and tr.fused_loss and tr.net.mixed
    before = dict(pk.n_calls)
    buf = tr.rollout()
    la, lc = tr._layer_lists
    assert la.mixed and lc.mixed
    for t in (0, T - 1):                                                                # the update-form forward on the filed rows: the rollout's bits
        ya, yc = pk.mlp_forward_pair(buf["obs"][t].contiguous(), la, buf["states"][t].contiguous(), lc)
        assert torch.equal(ya[-1], buf["mu"][t]) and torch.equal(yc[-1].squeeze(-1), buf["val"][t])
    stats = [tr.update(buf), tr.update(tr.rollout())]
    assert all(torch.isfinite(torch.tensor([s["loss"], s["a_loss"], s["c_loss"], s["kl"]])).all() for s in stats)
    assert all(torch.isfinite(p).all() for p in tr.net.parameters())
    with torch.no_grad():                                                               # act() follows the mode: the walk again
        n0 = pk.n_calls[BF16[0]]
        assert torch.equal(tr.act(buf["obs"][0]), pk.mlp_walk_forward([(buf["obs"][0].contiguous(), la)], store_hidden=False, mixed=True)[0][-1])
        assert pk.n_calls[BF16[0]] == n0 + 2
    after = pk.n_calls
    assert all(after.get(k, 0) > before.get(k, 0) for k in BF16), (before, after)
    assert all(after.get(k, 0) == before.get(k, 0) for k in FP32_WALK + ("n_mixed_dw_torch",)), (before, after)


def test_one_minibatch_step_against_the_float64_statement(hip, monkeypatch):
    """the parameter gradients of PPOTrainer._mb_backward_fused with the key on, where the optimiser reads them, against the float64 statement chained from
    the step's own stored outputs and dZ (the planted minibatch of tests/minibatch_step_util.py, cell 1); the objective's launch is the fp32 one as ever"""
    case = msu.build(1)
    od, sd, A, units, _, _, _ = msu.CELLS[1]
    tr = PPOTrainer(msu.StubEnv(od, sd, DEV), od, sd, A, PPOConfig(units=list(units), mixed_precision=True), device=DEV)
    msu.install(case, tr)
    assert tr.fused_loss and tr.torch_path_reason is None
    seen = {}
    fwd, bwd = pk.mlp_forward_pair, pk.mlp_backward_pair

    def forward(xa, la, xc, lc, *a, **k):
        seen["fwd"] = (xa, xc) + fwd(xa, la, xc, lc, *a, **k)
        return seen["fwd"][2:]

    def backward(xa, ya, gya, la, xc, yc, gyc, lc):
        seen["g"] = (gya.clone(), gyc.clone())
        return bwd(xa, ya, gya, la, xc, yc, gyc, lc)
    monkeypatch.setattr(pk, "mlp_forward_pair", forward)
    monkeypatch.setattr(pk, "mlp_backward_pair", backward)
    d, idx = msu.minibatch(case, DEV)
    acc = tr._new_acc(DEV)
    tr.flat_opt.flat_g.fill_(7.0)
    tr._mb_backward(d, idx, acc)
    torch.cuda.synchronize()
    xa, xc, ya, yc = seen["fwd"]
    assert torch.equal(xa, d["obs"][idx]) and torch.equal(xc, d["states"][idx])
    la, lc = tr._layer_lists
    w_out, w_dz, w_g = [0.0], [0.0], [0.0]
    dzs = pk.mlp_walk_backward([(seen["g"][0], ya, la), (seen["g"][1], yc, lc)], mixed=True)
    for x, layers, ys, gy, dz in ((xa, la, ya, seen["g"][0], dzs[0]), (xc, lc, yc, seen["g"][1], dzs[1])):
        check_forward(x, layers, "elu", ys, w_out)
        check_grads(layers, check_backward(x, layers, "elu", ys, gy, dz, w_dz), "minibatch step", w_g)
    print(f"minibatch step: worst error / max |want|: outputs {w_out[0]:.2e}, dZ {w_dz[0]:.2e}, dW and db {w_g[0]:.2e}")
    # the statistics and the log-std gradient come from the objective's fp32 launch on the mixed forward
    assert torch.isfinite(acc["_fused"]).all() and torch.isfinite(tr.flat_opt.grad_view(tr.net.log_std)).all()
