"""Shared by tests/test_value_path.py and tests/test_value_path_gpu.py: planted samples for the clipped value loss and its float64 restatement."""
import torch

E_CLIP = 0.2
MARGIN = 1e-3
# (v - v_old, ret - v_old) per regime; e = 0.2
REGIMES = (
    (0.10, 0.50),      # inside the range
    (0.50, 0.60),      # clipped, moved towards the return:   L_u = 0.01,   L_c = 0.16  -> L_c, no gradient
    (0.50, -0.30),     # clipped, moved away from the return: L_u = 0.64,   L_c = 0.25  -> L_u
    (0.00, 0.60),      # v = v_old exactly
    (-0.45, -0.70),    # the same on the other side:          L_u = 0.0625, L_c = 0.25  -> L_c
    (-0.45, 0.20),     #                                      L_u = 0.4225, L_c = 0.16  -> L_u
    (-0.10, -0.50),    # inside, below
)


def planted(B, device="cpu", seed=0):
    """(v, ret, v_old), float32 [B]: the regimes above cycled over the batch, v_old uniform in [-1, 1], every offset jittered by at most 0.03 (none on the
    v = v_old regime).  By construction every sample is at least MARGIN away from |v - v_old| = e, and every sample OUTSIDE the range at least MARGIN away
    from L_u = L_c (inside it the two terms agree to rounding by definition, and the selection does not look at them): asserted here, nothing is excluded."""
    g = torch.Generator().manual_seed(seed)
    k = torch.arange(B) % len(REGIMES)
    d = torch.tensor([r[0] for r in REGIMES], dtype=torch.float64)[k]
    r = torch.tensor([r[1] for r in REGIMES], dtype=torch.float64)[k]
    d = d + (torch.rand(B, generator=g, dtype=torch.float64) - 0.5) * 0.06 * (d != 0)
    r = r + (torch.rand(B, generator=g, dtype=torch.float64) - 0.5) * 0.06
    vo = torch.rand(B, generator=g, dtype=torch.float64) * 2 - 1
    v_old, v, ret = vo.float(), (vo + d).float(), (vo + r).float()
    v = torch.where(d == 0, v_old, v)
    # the margins, on the float32 values the code under test will see
    dd = v.double() - v_old.double()
    lu = (v.double() - ret.double()) ** 2
    lc = (v_old.double() + dd.clamp(-E_CLIP, E_CLIP) - ret.double()) ** 2
    outside = dd.abs() > E_CLIP
    assert bool(((dd.abs() - E_CLIP).abs() >= MARGIN).all())
    assert bool(((lu - lc).abs()[outside] >= MARGIN).all())
    if B >= len(REGIMES):                                     # all four kinds are present
        assert bool((outside & (lc > lu)).any()) and bool((outside & (lu > lc)).any()) and bool((~outside & (dd != 0)).any()) and bool((dd == 0).any())
    return v.to(device), ret.to(device), v_old.to(device)


def restated(v, ret, v_old, e=E_CLIP):
    """the definition in float64, written with max: c_i = max((v - ret)^2, (v_old + clamp(v - v_old, -e, e) - ret)^2), per sample"""
    v, ret, v_old = v.double(), ret.double(), v_old.double()
    return torch.maximum((v - ret) ** 2, (v_old + (v - v_old).clamp(-e, e) - ret) ** 2)


def restated_with_grad(v, ret, v_old, e=E_CLIP):
    """(c_i, d sum_i c_i / d v) of the restatement, the gradient from autograd in float64.  Away from the two boundaries (see `planted`) it is 2 (v - ret) or
    0; on the exact tie v = v_old, max splits the gradient between two terms that both have 2 (v - ret): the same number."""
    vd = v.double().clone().requires_grad_(True)
    c = restated(vd, ret, v_old, e)
    c.sum().backward()
    return c.detach(), vd.grad
