"""The four instantiations of k_gae (csrc/ppo_kernels.hip) through the one wrapper, ppo_kernels.gae_buffers, against the one specification, ppo.gae_spec with the
normalised-value step of ppo.gae_torch, run on the same GPU tensors: bit for bit.  Flags and records are those of tests/test_episode_ends_gpu.py."""
import pytest
import torch

from leibnizgym_amd import ppo_kernels as pk
from leibnizgym_amd.ppo import gae_torch
from test_episode_ends_gpu import flags, records

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
GAMMA, TAU = 0.99, 0.95


def same(got, want, keys, what):
    assert sorted(got) == sorted(keys), (what, sorted(got))
    for k in keys:
        assert got[k].shape == want[k].shape and torch.equal(got[k], want[k]), (what, k, float((got[k] - want[k]).abs().max()))


@pytest.mark.parametrize("T", [1, 3, 32])
@pytest.mark.parametrize("n", [1, 63, 64, 65, 257])
def test_every_instantiation_holds_the_bits_of_the_specification(hip, T, n):
    end, tout, last_end = (t.to(DEV) for t in flags(T, n))
    g = torch.Generator(device=DEV).manual_seed(100 * T + n)
    y = torch.randn(T + 1, n, device=DEV, generator=g) * 3
    y[0, 0], y[T, n - 1] = 7.5, -6.25                                     # beyond the clip on both sides, the bootstrap row included
    zero, zero_n = torch.zeros(T, n, device=DEV), torch.zeros(n, device=DEV)
    dones = {"none": zero, "all": torch.ones(T, n, device=DEV), "last step": zero.clone()}
    dones["last step"][T - 1] = 1.0
    for name, rec in (("raw", None),) + records():
        keys = ("adv", "ret") + (("ret_n", "v_old_n") if rec is not None else ())
        rew = torch.randn(T, n, device=DEV, generator=g) * (0.3 / float(rec.inv_std_f) if rec is not None else 0.3)   # rewards of the size of the values
        for dname, done in dones.items():                                  # <false, VNORM>
            same(pk.gae_buffers(rew, y, GAMMA, TAU, done=done, vnorm=rec), gae_torch(rew, y, GAMMA, TAU, done=done, vnorm=rec), keys, (name, "done", dname))
        plain = pk.gae_buffers(rew, y, GAMMA, TAU, done=zero, vnorm=rec)
        for boot in (False, True):                                         # <true, VNORM>
            mode = (end, tout, last_end, boot)
            got = pk.gae_buffers(rew, y, GAMMA, TAU, ends=mode, vnorm=rec)
            same(got, gae_torch(rew, y, GAMMA, TAU, ends=mode, vnorm=rec), keys + ("w",), (name, "ends", boot))
            assert bool((got["adv"][got["w"] == 0] == 0).all())            # a stale sample has no advantage
            quiet = pk.gae_buffers(rew, y, GAMMA, TAU, ends=(zero, tout, zero_n, boot), vnorm=rec)      # no end anywhere: the `done` instantiation
            same({k: quiet[k] for k in keys}, plain, keys, (name, "no end", boot))
            assert bool((quiet["w"] == 1).all())
    assert torch.equal(y[0, :1].cpu(), torch.tensor([7.5])) and float(end[T - 1, 0]) == 1.0      # the inputs are only read
