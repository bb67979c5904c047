"""The float64 statement of the minibatch step (tests/minibatch_step_util.py) against the trainer's plain torch path on the CPU: `p.grad` of every parameter
and the four statistics, per cell.  This holds the statement itself and the conditions on its inputs (asserted while a case is built); the kernels are held
to the same statement in tests/test_minibatch_step_gpu.py."""
import pytest
import torch

import minibatch_step_util as mu


@pytest.mark.parametrize("cell", mu.CELL_IDS)
def test_torch_path_matches_the_float64_statement(cell):
    case = mu.build(cell)
    tr = mu.make_trainer(cell, "cpu")
    mu.install(case, tr)
    assert not tr.fused_loss and tr.flat_opt is None and tr.clip_v == case.clip_v
    d, idx = mu.minibatch(case, "cpu")
    acc = tr._new_acc("cpu")
    tr._mb_backward(d, idx, acc)
    mu.check(case, {n: p.grad for n, p in tr.net.named_parameters()}, acc["_fused"], "torch fp32, CPU")


def test_the_cells_are_the_trainers_they_claim_to_be():
    """what each cell is there to reach, as far as it can be read without a GPU"""
    nets = {c: mu.make_trainer(c, "cpu").net for c in mu.CELL_IDS}
    assert all(nets[c].central for c in (1, 2, 4, 5, 6, 8)) and not nets[3].central and not nets[7].central
    assert nets[3].log_std.numel() == 18 and nets[3].critic[0].in_features == 41 and nets[7].critic_norm() is nets[7].obs_norm is not None
    assert nets[4].actor.d2rl and nets[4].critic.d2rl and nets[4].obs_norm is not None and nets[4].state_norm is not None
    assert not nets[5].actor.d2rl and nets[5].critic.d2rl and isinstance(nets[5].critic[1], torch.nn.Tanh) and isinstance(nets[5].actor[1], torch.nn.ELU)
    assert mu.build(6).clip_v and mu.build(7).clip_v and "old_v" in mu.build(6).d and "old_v" not in mu.build(1).d
    assert mu.build(2).idx.numel() == 1100 and 1024 < 1100 < 2048 and mu.build(1).idx.numel() == 333
    assert nets[8].actor[0].out_features == 448 and nets[8].actor[0].in_features % 4 != 0 and nets[8].critic[0].in_features % 4 == 0
    for c in mu.CELL_IDS:                                            # idx is a permuted subset: no row twice, not in order
        idx = mu.build(c).idx
        assert idx.unique().numel() == idx.numel() and not bool((idx[1:] > idx[:-1]).all())
