"""The trainer's minibatch step on the GPU - plain torch (`fused_kernels=False`) and the hand-written kernels as PPOTrainer._mb_backward_fused wires them together -
against the float64 statement of tests/minibatch_step_util.py: every parameter's gradient where the optimiser will read it, the zero padding between the
slots of the flat gradient buffer, the four statistics; and one optimiser step on top (FlatClipAdam against a float64 restatement of clip_grad_norm_ per group
+ Adam step 1, applied to the flat gradient as read back from the device).  Unlike a comparison of parameters after some Adam steps, this sees a constant
factor on a group's gradient (a wrong v_coef, a missing 1 / B), a gradient in another parameter's slot and a store that spills into the padding."""
import math

import pytest
import torch

import minibatch_step_util as mu
from leibnizgym_amd import ppo_kernels as pk

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def slot(fo, p):
    """where the optimiser reads the gradient of `p`: element i of flat_g moves element i of flat_p, and `p` IS a piece of flat_p - the place follows from
    the parameter's own address, not from the bookkeeping (`grad_view`, `offsets`) the step was wired with"""
    o, rem = divmod(p.data_ptr() - fo.flat_p.data_ptr(), 4)
    assert rem == 0 and o % 4 == 0 and 0 <= o and o + p.numel() <= fo.flat_p.numel() and p.is_contiguous()
    return fo.flat_g[o:o + p.numel()].view_as(p)


def slot_mask(fo):
    mask = torch.zeros(fo.flat_g.numel(), dtype=torch.bool, device=fo.flat_g.device)
    for p in fo.params:
        o = (p.data_ptr() - fo.flat_p.data_ptr()) // 4
        assert not bool(mask[o:o + p.numel()].any())                      # no two parameters overlap
        mask[o:o + p.numel()] = True
    return mask


def fused_step(cell):
    """one `_mb_backward` of the cell's trainer on the kernels, every check of the gradient made; returns the trainer (gradients in flat_g, nothing applied)"""
    case = mu.build(cell)
    tr = mu.make_trainer(cell, DEV, fused=True)
    mu.install(case, tr)
    assert tr.fused_loss and tr.torch_path_reason is None and tr.clip_v == case.clip_v
    la, lc = tr.net.actor.layer_list(), tr.net.critic.layer_list()
    walk = pk.net_fits([la, lc], False) and pk.net_fits([la, lc], True)
    assert walk == (cell != 8)                                            # cell 8 is the per-layer fallback, every other cell the walk
    fo = tr.flat_opt
    mask = slot_mask(fo)
    assert int((~mask).sum()) > 0                                         # there is padding to spill into
    fo.flat_g.zero_()
    assert len(fo.params) == len(list(tr.net.parameters())) and all(any(q is p for q in fo.params) for p in tr.net.parameters())
    for p in fo.params:
        slot(fo, p).fill_(7.0)                                            # whatever the step does not write fails by itself
    assert bool((fo.flat_g[mask] == 7.0).all()) and bool((fo.flat_g[~mask] == 0.0).all())
    d, idx = mu.minibatch(case, DEV)
    acc = tr._new_acc(DEV)
    tr._mb_backward(d, idx, acc)
    torch.cuda.synchronize()
    assert all(p.grad is None for p in tr.net.parameters()) and tr.fused_loss
    pad = fo.flat_g[~mask]
    assert bool((pad == 0.0).all()), f"{int((pad != 0).sum())} padding elements of flat_g written, max |value| {float(pad.abs().max()):.3e}"
    mu.check(case, {n: slot(fo, p) for n, p in tr.net.named_parameters()}, acc["_fused"], "kernels")
    return tr


@pytest.mark.parametrize("cell", mu.CELL_IDS)
def test_torch_path_on_the_gpu_matches_the_float64_statement(hip, cell):
    case = mu.build(cell)
    tr = mu.make_trainer(cell, DEV, fused=False)
    mu.install(case, tr)
    assert not tr.fused_loss and tr.flat_opt is None
    d, idx = mu.minibatch(case, DEV)
    acc = tr._new_acc(DEV)
    tr._mb_backward(d, idx, acc)
    mu.check(case, {n: p.grad for n, p in tr.net.named_parameters()}, acc["_fused"], "torch fp32, GPU")


@pytest.mark.parametrize("cell", mu.CELL_IDS)
def test_kernels_match_the_float64_statement(hip, cell):
    fused_step(cell)


@pytest.mark.parametrize("cell", [1, 3])
def test_one_optimiser_step_on_the_flat_gradient(hip, cell):
    """tolerance: tests/test_ppo_kernels.py::test_flat_clip_adam_matches_torch (rtol 2e-5, atol 2e-7)"""
    case = mu.build(cell)
    tr = fused_step(cell)
    fo, c = tr.flat_opt, tr.cfg
    central = tr.net.central
    n = fo.flat_p.numel()
    if central:
        lrs, max_norms = (c.lr, c.lr_value), (c.grad_norm, c.value_grad_norm)
        norms = mu.group_norms(case, True)                                # one group is truncated, the other is not: on the reference
        assert norms[0] > 1.1 * max_norms[0] and norms[1] < 0.95 * max_norms[1], norms
        assert 0 < fo.n0 < fo.n1 == n
        for name, p in tr.net.named_parameters():                        # the actor's group (log_std in it) below n0, the critic's from n0 on
            assert ((p.data_ptr() - fo.flat_p.data_ptr()) // 4 >= fo.n0) == name.startswith("critic."), name
    else:
        lrs, max_norms = (c.lr, c.lr), (c.grad_norm, c.grad_norm)
        assert fo.n0 == fo.n1 == n
    mask = slot_mask(fo).cpu()
    g, p0 = fo.flat_g.double().cpu(), fo.flat_p.double().cpu()
    assert bool((fo.m == 0).all()) and bool((fo.v == 0).all()) and fo.step_count.tolist() == [0.0, 0.0]
    tr._mb_apply()
    torch.cuda.synchronize()
    b1, b2, eps = 0.9, 0.999, 1e-8
    want_p, want_m, want_v = p0.clone(), torch.zeros_like(g), torch.zeros_like(g)
    for (lo, hi), lr, mx in zip(((0, fo.n0), (fo.n0, fo.n1)), lrs, max_norms):
        gg = g[lo:hi]
        gg = gg * min(mx / (math.sqrt(float((gg * gg).sum())) + 1e-6), 1.0)                      # clip_grad_norm_ of the group
        want_m[lo:hi] = (1 - b1) * gg
        want_v[lo:hi] = (1 - b2) * gg * gg
        want_p[lo:hi] -= (lr / (1 - b1)) * want_m[lo:hi] / (want_v[lo:hi].sqrt() / math.sqrt(1 - b2) + eps)
    for what, got, want in (("flat_p", fo.flat_p, want_p), ("m", fo.m, want_m), ("v", fo.v, want_v)):
        got = got.double().cpu()
        print(f"cell {cell} {what}: max |got - want| {float((got - want).abs().max()):.3e}, max |want| {float(want.abs().max()):.3e}")
        assert torch.allclose(got, want, rtol=2e-5, atol=2e-7), what
        assert bool((got[~mask] == 0.0).all()), f"{what}: the padding moved"
    assert float((fo.flat_p.double().cpu() - p0).abs().max()) > 0.5 * min(lrs)                    # the step was taken
    assert fo.step_count.tolist() == [1.0, 1.0]
    if not central:
        par = 1                                                           # step 1 summed into the odd half of sq; its second slot is the empty group's
        sq = fo.sq.tolist()
        assert sq[2 * par + 1] == 0.0 and sq[2 * par] > 0.0, sq
