"""The headline units (0_0, 0_1, 0_2) are built WITHOUT domain randomisation; a config with `dr_enable` and no extended feature runs in units of its
own (d0_0, d0_1, d0_2: the same kernels with the run-time flag).  The units of the general box are split in the same way (2_* / d2_*: pinned to the
oracle with and without domain randomisation by tests/test_box_object.py; here: test_dispatch).  This file pins both to the oracle and to each other:

(a) a config without domain randomisation on the HIP library equals the oracle BIT FOR BIT on every per-env output, no env excluded, through the
    `narrow`, `wide` and `wide_helpers` instantiations, for N in {1, 63, 64, 65, 1000};
(b) the same config with `dr_enable = 1`, every range (1, 1), observation noise 0 and action repeat 0 - which the host sends to the d0_* units -
    equals run (a) bit for bit in every output buffer and every state row except the TF_S_DR rows.  Why that identity holds: every factor is drawn as
    fma(hi - lo, u, lo) = fma(0, u, 1) = 1.0f exactly, x * 1.0f is exact, and the draws are counter-based (seed, env, reset count, purpose), so drawing
    the factors moves no other stream.  It is first asserted between two ORACLE runs on the CPU (test_identity_of_neutral_ranges_on_the_oracle).

The rollouts (`envdefault_position`: position mode, every reward term, success termination on; 40-step episodes) have finger-cube and floor
contacts, time-out resets and goal resets; the reach is asserted on the oracle's snapshots, in the CPU half, with the same rollouts the GPU half uses.
"""
import numpy as np
import pytest

import parity_util as pu
from leibnizgym_amd import _capi as capi
from leibnizgym_amd.engine import TrifingerEngine, make_config

DEV = "cuda:0"
SIZES = [1, 63, 64, 65, 1000]
CFG = "envdefault_position"
STEPS = {1: 130, 63: 130, 64: 130, 65: 130, 1000: 130}
NEUTRAL_DR = {"activate": True, "cube_mass": (1.0, 1.0), "cube_size": (1.0, 1.0), "friction": (1.0, 1.0), "motor_torque": (1.0, 1.0),
              "link_mass": (1.0, 1.0), "restitution": (1.0, 1.0), "obs_noise": 0.0, "action_repeat_prob": 0.0}
DR_ROWS = slice(capi.S_DR, capi.S_DR + capi.TF_NUM_DR)


def _oracle_legs(oracle, n):
    """the oracle's rollouts (a) and (b) of size n, with the reach of (a) asserted"""
    a = pu.oracle_rollout(oracle, n, STEPS[n], CFG)
    b = pu.oracle_rollout(oracle, n, STEPS[n], CFG, extra=dict(domain_randomization=NEUTRAL_DR))
    counts = np.array([s["reset_count"] for s in a])
    steps = np.array([s["steps"] for s in a])
    # time-outs: every env's step counter falls back to zero at least twice in 130 steps of 40-step episodes
    assert ((steps[1:] < steps[:-1]).sum(axis=0) >= 2).all(), "no time-out resets"
    if n >= 63:
        # goal resets raise reset_count without a time-out (success termination is on); contacts: warm-start impulses of the finger-cube rows
        resets = (steps[1:] < steps[:-1]).sum(axis=0)
        assert ((counts[-1] - counts[0]) > resets + 1).any(), "no goal resets"
        assert any((s["state"][capi.S_LAM_FC:capi.S_LAM_FC + 12] != 0).any() for s in a), "no finger-cube contact"
    return a, b


# ---- CPU: the oracle legs, and identity (b) on the oracle -------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", SIZES)
def test_identity_of_neutral_ranges_on_the_oracle(oracle, n):
    a, b = _oracle_legs(oracle, n)
    for t, (x, y) in enumerate(zip(b, a)):
        pu.assert_bit_equal(x, y, f"oracle, neutral ranges vs no domain randomisation, N={n} step {t}", skip_rows=DR_ROWS)
    assert all((s["state"][capi.S_DR:capi.S_DR + 6] == 1.0).all() for s in b)


# ---- GPU ----------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("variant", pu.VARIANTS)
@pytest.mark.parametrize("n", SIZES)
def test_dr_off_units_equal_the_oracle(hip, oracle, n, variant):
    """(a): units 0_0 / 0_1 / 0_2"""
    want, _ = _oracle_legs(oracle, n)
    got = pu.rollout(hip, DEV, n, STEPS[n], CFG, variant=variant)
    for t, (x, y) in enumerate(zip(got, want)):
        pu.assert_bit_equal(x, y, f"DR off [{variant}] N={n} step {t}")


@pytest.mark.gpu
@pytest.mark.parametrize("variant", pu.VARIANTS)
@pytest.mark.parametrize("n", SIZES)
def test_neutral_ranges_in_the_dr_units_equal_dr_off(hip, oracle, n, variant):
    """(b): units d0_0 / d0_1 / d0_2 against (a) on the same library, and against the oracle's run of the same config (every row)"""
    _, want_b = _oracle_legs(oracle, n)
    a = pu.rollout(hip, DEV, n, STEPS[n], CFG, variant=variant)
    b = pu.rollout(hip, DEV, n, STEPS[n], CFG, variant=variant, extra=dict(domain_randomization=NEUTRAL_DR))
    for t, (x, y, w) in enumerate(zip(b, a, want_b)):
        pu.assert_bit_equal(x, y, f"neutral ranges vs DR off [{variant}] N={n} step {t}", skip_rows=DR_ROWS)
        pu.assert_bit_equal(x, w, f"neutral ranges vs oracle [{variant}] N={n} step {t}")


BOX = ([0.02, 0.08, 0.02], 500.0)      # the phase-3 cuboid


@pytest.mark.gpu
@pytest.mark.parametrize("variant", pu.VARIANTS)
@pytest.mark.parametrize("neutral_dr", [False, True])
def test_box_units_with_and_without_the_flag_equal_the_oracle(hip, oracle, variant, neutral_dr):
    """the general box through all three widths: units 2_* (built without domain randomisation) and, with the neutral ranges, d2_* (the run-time flag)"""
    extra = dict(domain_randomization=NEUTRAL_DR) if neutral_dr else {}
    want = pu.oracle_rollout(oracle, 321, 70, "d4_torque_asym", episode_length=25, extra=dict(extra, model=oracle.box_model(*BOX)))
    got = pu.rollout(hip, DEV, 321, 70, "d4_torque_asym", episode_length=25, extra=dict(extra, model=hip.box_model(*BOX)), variant=variant)
    for t, (x, y) in enumerate(zip(got, want)):
        pu.assert_bit_equal(x, y, f"box, neutral ranges {neutral_dr} [{variant}] step {t}")


FULL_DR = dict(pu.CONFIGS["d4_domain_randomization_extended"]["domain_randomization"])
BASE_DR = dict(pu.CONFIGS["d4_domain_randomization"]["domain_randomization"])


@pytest.mark.gpu
@pytest.mark.parametrize("variant", pu.VARIANTS)
@pytest.mark.parametrize("dr", ["off", "base", "full", "box-off", "box-base"])
def test_dispatch(hip, dr, variant):
    """tf_kernel_occupancy and the step go through the table of units for every (domain randomisation, width) pair, with the cube and with the general
    box (whose units are split in the same way: 2_* without, d2_* with the run-time flag): no null entry, no failed launch"""
    kw = dict(pu.CONFIGS["d4_torque_asym"])
    box = dr.startswith("box-")
    if box:
        kw["model"] = hip.box_model([0.02, 0.08, 0.02], 500.0)
        dr = dr[len("box-"):]
    if dr != "off":
        kw["domain_randomization"] = BASE_DR if dr == "base" else FULL_DR
    eng = TrifingerEngine(make_config(hip, 256, seed=3, episode_length=5, **kw), device=DEV, lib=hip)
    eng.kernel_variant = variant
    assert eng.kernel_variant == variant
    if box:
        assert eng.kernel_occupancy >= 1
    else:
        assert eng.kernel_occupancy == (4 if variant == "narrow" else 2 if variant == "wide" else 1)
    eng.reset()
    for t in range(8):
        eng.step(pu.actions_for(t, 256, eng.action_dim, 3).to(DEV))
    eng.step_random()
    snap = pu.snapshot(eng)
    assert np.isfinite(snap["obs"]).all() and np.isfinite(snap["reward"]).all()
    factors = snap["state"][capi.S_DR:capi.S_DR + 6]
    assert (factors == 1.0).all() if dr == "off" else (factors != 1.0).any()      # the factors were drawn where, and only where, they were asked for
    eng.close()
