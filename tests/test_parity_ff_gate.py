"""The link-speed gate of the middle-distal finger-finger rows (csrc/tf_contact.h: ff_link_speeds, ff_gate) against the oracle, BIT FOR BIT.

The kernels enter the block that builds a middle-distal row only where the gap can close within the substep at the fastest the two links can move
(gap < contact_slack + h (s_dist + s_mid), bounds the fingers publish with their free motion); the oracle has no such gate and enters at
gap < contact_margin.  A gate that is too tight drops a live row and nothing else shows it.  The older rollouts are thin on the case that matters -
live rows WELL ABOVE the slack, where only the speed term keeps the gate open - so this one is made of the steady state of the bench workload:

  1. ON THE ORACLE: bench.workload_kwargs(True) (episode length 750), 1026 envs (16 full wavefronts and a ragged one of 2 lanes), reset, the step
     counters spread over the episode (seeded), 200 steps of parity_util.actions_for (seeded 2 U - 1).
  2. That state goes to every engine through state_dict() / load_state_dict().
  3. 36 more steps on both sides with the same actions; every per-env output buffer and the whole state compared after the hand-over and after every
     step (parity_util.assert_bit_equal, no env and no row excluded), for the three widths (tf_set_kernel_variant) x four configurations: the headline
     config (units 0_*), its twin with the base domain randomisation as a run-time flag (d0_*), every domain-randomisation feature (1_*), the box (2_*).
  4. Reach, counted with the census build of the oracle (ff_census_util) on the headline configuration: at least MIN_M1 = 100 of the 1026 x 36
     env-steps hold a live middle-distal row (bit M1).  Measured on the oracle: 94 in the first 24 steps - under the floor, so the rollout is 36 steps
     long - and 137 in 36 (53 envs).  If the floor is missed: lengthen the rollout, never lower the floor.
  5. Reach above the slack.  At gap < contact_slack the gate is open whatever the speeds are: only a live row with gap > contact_slack can be lost to a
     speed bound that is too tight.  test_reach_above_the_slack counts them in THIS rollout on the instrumented oracle of tools/ff_gate_census.py (the
     counters of tools/experiments/ff_gate_census.patch) and asserts at least MIN_ABOVE_SLACK = 12.  The floor is not taken from this rollout: the census
     of 4096 envs (profiles/r18_ff_gate_census.txt) has 23 % of the live rows above the slack, 23 % of the MIN_M1 = 100 env-steps is 23 rows, and the
     floor is half of that (measured: 149 of 583 live rows).  The same run asserts that the C twin of the bound shuts no live row out.

Sensitivity (measured once on the GPU with a scratch build whose gate is gap < contact_slack alone, the speed term zero): 4 of the 12 cells of this file
fail - the four `narrow` ones: only the 128-register kernels carry the gate.
"""
import ctypes as C
import os
import sys
import tempfile

import numpy as np
import pytest
import torch

import bench
import ff_census_util as fc
import parity_util as pu
from leibnizgym_amd.engine import TrifingerEngine, make_config

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools"))
import ff_gate_census  # noqa: E402

DEV = "cuda:0"
N, SETTLE, STEPS, SEED = 1026, 200, 36, 18
MIN_M1 = 100
MIN_ABOVE_SLACK = 12     # live rows (per substep) with gap > contact_slack: see (5) of the module docstring
BOX = ([0.02, 0.08, 0.02], 500.0)
CASES = ("headline", "base_dr", "full_dr", "box")

_ORACLE = {}           # case -> (state_dict after the settle steps, snapshots of the 36 steps)


def _engine(lib, device, case, variant=None):
    kw = bench.workload_kwargs(True, 4, case == "full_dr")
    if case == "base_dr":
        kw["domain_randomization"] = pu.MATRIX_BASE_DR
    if case == "box":
        kw["model"] = lib.box_model(*BOX)
    eng = TrifingerEngine(make_config(lib, N, seed=SEED, **kw), device=device, lib=lib)
    if variant is not None:
        eng.kernel_variant = variant
        assert eng.kernel_variant == variant
    return eng


def _continue(eng, sd, before_step=None, after_step=None):
    """load the settled state and step STEPS times: snapshots after the hand-over and after every step"""
    eng.reset()
    eng.load_state_dict(sd)
    snaps = [pu.snapshot(eng)]
    for t in range(STEPS):
        if before_step is not None:
            before_step()
        eng.step(pu.actions_for(SETTLE + t, N, eng.action_dim, SEED).to(eng.state.device))
        snaps.append(pu.snapshot(eng))
        if after_step is not None:
            after_step()
    return snaps


def _oracle_rollout(oracle, case):
    if case not in _ORACLE:
        eng = _engine(oracle, "cpu", case)
        eng.reset()
        g = torch.Generator().manual_seed(SEED)
        eng.steps.copy_(torch.randint(0, int(eng.cfg.episode_length), (N,), generator=g, dtype=torch.int64))
        for t in range(SETTLE):
            eng.step(pu.actions_for(t, N, eng.action_dim, SEED))
        sd = eng.state_dict()
        snaps = _continue(eng, sd)
        eng.close()
        _ORACLE[case] = (sd, snaps)
    return _ORACLE[case]


def test_reach_on_the_oracle(oracle):
    """(4) of the module docstring, and that the census build steps the plain oracle's bits from the handed-over state"""
    sd, want = _oracle_rollout(oracle, "headline")
    eng = _engine(fc.census_library(), "cpu", "headline")
    mask = fc.bind_mask(eng)
    masks = []

    def clear():
        mask[:] = 0

    got = _continue(eng, sd, clear, lambda: masks.append(mask.copy()))
    eng.close()
    masks = np.stack(masks)
    for t, (x, y) in enumerate(zip(got, want)):
        pu.assert_bit_equal(x, y, f"census vs plain oracle, snapshot {t}")
    r = fc.reach(masks)
    print("\nheadline, %d envs x %d steps after %d settle steps: " % (N, STEPS, SETTLE) + "  ".join(f"{k} {v[0]}/{v[1]}" for k, v in r.items()))
    assert masks.shape == (STEPS, N)
    assert r["M1"][0] >= MIN_M1, r["M1"]


def test_reach_above_the_slack(oracle):
    """(5) of the module docstring"""
    sd, want = _oracle_rollout(oracle, "headline")
    with tempfile.TemporaryDirectory() as tmp:
        lib = ff_gate_census.build(tmp)
        eng = _engine(lib, "cpu", "headline")
        cnt = (C.c_int64 * 4)()
        first = [True]

        def clear_once():                                      # behind the hand-over: the rows of the reset's own launch do not count
            if first[0]:
                lib.dll.tf_ffg_counters(cnt, 1)
                first[0] = False

        got = _continue(eng, sd, clear_once)
        lib.dll.tf_ffg_counters(cnt, 0)
        eng.close()
    pu.assert_bit_equal(got[-1], want[-1], "instrumented vs plain oracle, last snapshot")
    live, above, above2, shut = (int(x) for x in cnt)
    print("\nheadline, %d envs x %d steps: %d live middle-distal rows, %d with gap > contact_slack, %d with gap > 2 contact_slack, %d shut out by the bound"
          % (N, STEPS, live, above, above2, shut))
    assert shut == 0
    assert above >= MIN_ABOVE_SLACK, (live, above)


@pytest.mark.gpu
@pytest.mark.parametrize("variant", pu.VARIANTS)
@pytest.mark.parametrize("case", CASES)
def test_cell_bit_exact(hip, oracle, case, variant):
    sd, want = _oracle_rollout(oracle, case)
    eng = _engine(hip, DEV, case, variant)
    got = _continue(eng, sd)
    eng.close()
    assert len(got) == len(want) == STEPS + 1
    for t, (x, y) in enumerate(zip(got, want)):
        pu.assert_bit_equal(x, y, f"{case} [{variant}] snapshot {t}")
