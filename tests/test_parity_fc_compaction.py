"""The per-lane order of the finger-cube blocks in the 128-register kernels (tf_roles.h, cube_role) against the oracle, bit for bit.

Per env the cube role still solves the blocks of the live fingers in ascending f with the same arithmetic; what changed is which lanes of a wavefront
work side by side in a pass, where the 1/D, bias and impulses of a slot live during the sweeps (registers selected per lane for passes 0 and 1, LDS for
pass 2), how the warm start walks the fingers and how the `last` hand-over finds the impulses.  None of that may move a bit: every per-env output of the
`narrow` instantiation - forced through tf_set_kernel_variant, since tf_create would pick a 256-register kernel at these sizes - equals the oracle's after
every step, no env excluded, on

    headline       the bench workload (bench.workload_kwargs: difficulty 4, torque mode, asymmetric obs), unit 0_0
    extended_dr    every domain-randomisation feature, extended ones included (unit 1_0)
    box            the general box object (unit 2_0)
    pinch          the headline config from a hand-built start: the cube at the stage centre, the three fingertips 0.4 .. 1.0 mm inside three of
                   its faces, so that all three finger-cube slots are live from step 1 (unit 0_0)

The change only shows where a lane has more than one live finger - with one live finger at most the passes are the old loop with dead blocks
skipped.  So the reach is counted, from the TF_S_FC_LINK rows after every step (low two bits != 0: fc_live of the last substep), and asserted: over
the four rollouts at least 1000 compared env-steps with two live slots and at least 100 with three (the oracle alone: see the figures
test_reach_on_the_oracle prints; 1000 envs x 130 steps from a reset with seed 7 each).  The CPU half asserts the same reach on the oracle's rollouts.
"""
import numpy as np
import pytest
import torch

import bench
import parity_util as pu
from leibnizgym_amd import _capi as capi
from leibnizgym_amd.engine import TrifingerEngine, make_config

DEV = "cuda:0"
N, STEPS, SEED, EPISODE = 1000, 130, 7, 60
CASES = ("headline", "extended_dr", "box", "pinch")
BOX = ([0.02, 0.08, 0.02], 500.0)
MIN_TWO, MIN_THREE = 1000, 100
PINCH_DEPTHS = (0.0004, 0.0006, 0.0008, 0.0010)      # fingertip spheres this far inside the cube's faces, env i takes depth i % 4

_ORACLE = {}


def _pinch_joint_angles():
    """[4, 9] joint angles: the three fingertips on three faces of a cube that rests at the stage centre (tests/test_contact_scenarios.py: the pose of
    the pinch-and-lift scenario), PINCH_DEPTHS inside"""
    import physics_ref as PR
    import test_contact_scenarios as CS
    rows = []
    for depth in PINCH_DEPTHS:
        d = PR.CUBE_HALF + CS.R_TIP - depth
        tips = [np.array([0.0, d, PR.CUBE_HALF]), np.array([d, -d * np.tan(np.pi / 6), PR.CUBE_HALF]), np.array([-d, -d * np.tan(np.pi / 6), PR.CUBE_HALF])]
        rows.append(np.concatenate([CS.ik(f, tips[f]) for f in range(3)]))
    return np.array(rows), PR.CUBE_HALF


def _place_pinch(eng, q4, half):
    n = eng.num_envs
    q = torch.tensor(q4[np.arange(n) % len(q4)].T, dtype=torch.float32)
    cube = torch.zeros((13, n), dtype=torch.float32)
    cube[2], cube[6] = half, 1.0                     # on the floor at the stage centre, identity quaternion (x, y, z, w), at rest
    eng.q[:] = q.to(eng.q.device)
    eng.qd[:] = 0.0
    eng.cube[:] = cube.to(eng.cube.device)


def _rollout(lib, device, case, variant=None):
    kw = {k: v for k, v in bench.workload_kwargs(True, 4, case == "extended_dr").items() if k != "episode_length"}
    if case == "extended_dr":
        kw["domain_randomization"] = pu.CONFIGS["d4_domain_randomization_extended"]["domain_randomization"]
    if case == "box":
        kw["model"] = lib.box_model(*BOX)
    eng = TrifingerEngine(make_config(lib, N, seed=SEED, episode_length=EPISODE, **kw), device=device, lib=lib)
    if variant is not None:
        eng.kernel_variant = variant
        assert eng.kernel_variant == variant
    eng.reset()
    if case == "pinch":
        _place_pinch(eng, *_pinch_joint_angles())
    snaps = [pu.snapshot(eng)]
    for t in range(STEPS):
        eng.step(pu.actions_for(t, N, eng.action_dim, SEED).to(device))
        snaps.append(pu.snapshot(eng))
    eng.close()
    return snaps


def _oracle_rollout(oracle, case):
    if case not in _ORACLE:
        _ORACLE[case] = _rollout(oracle, "cpu", case)
    return _ORACLE[case]


def live_counts(snaps):
    """(env-steps with two live finger-cube slots, with three) of the snapshots after every step"""
    two = three = 0
    for s in snaps[1:]:
        live = ((s["state"][capi.S_FC_LINK:capi.S_FC_LINK + 3].astype(np.int64) & 3) != 0).sum(axis=0)
        two += int((live == 2).sum())
        three += int((live == 3).sum())
    return two, three


# ---- CPU: the reach of the rollouts, on the oracle ----------------------------------------------------------------------------------------------
def test_reach_on_the_oracle(oracle):
    total = np.zeros(2, dtype=np.int64)
    for case in CASES:
        two, three = live_counts(_oracle_rollout(oracle, case))
        print("%-12s %d envs x %d steps: %6d env-steps with two live finger-cube slots, %6d with three" % (case, N, STEPS, two, three))
        total += (two, three)
    print("%-12s %28s %6d %35s %6d" % ("all", "", total[0], "", total[1]))
    assert total[0] >= MIN_TWO and total[1] >= MIN_THREE, total


def test_pinch_start_has_three_live_slots_from_step_one(oracle):
    s = _oracle_rollout(oracle, "pinch")[1]
    live = (s["state"][capi.S_FC_LINK:capi.S_FC_LINK + 3].astype(np.int64) & 3) != 0
    assert live.all(), "envs without three live finger-cube slots after step 1: %d" % int((~live.all(axis=0)).sum())


# ---- GPU ----------------------------------------------------------------------------------------------------------------------------------------
_COMPARED = {}


@pytest.mark.gpu
@pytest.mark.parametrize("case", CASES)
def test_narrow_kernels_equal_the_oracle(hip, oracle, case):
    want = _oracle_rollout(oracle, case)
    got = _rollout(hip, DEV, case, variant="narrow")
    assert len(got) == len(want) == STEPS + 1
    for t, (x, y) in enumerate(zip(got, want)):
        pu.assert_bit_equal(x, y, f"per-lane order of the finger-cube blocks [{case}, narrow] step {t}")
    _COMPARED[case] = live_counts(got)               # counted on what the GPU produced (bit-equal to the oracle's rows by now)
    print("%-12s compared: %d env-steps with two live finger-cube slots, %d with three" % ((case,) + _COMPARED[case]))


@pytest.mark.gpu
def test_compared_env_steps_reach_multi_finger_envs(hip, oracle):
    """the four comparisons above together (re-run here if this test is selected alone)"""
    for case in CASES:
        if case not in _COMPARED:
            test_narrow_kernels_equal_the_oracle(hip, oracle, case)
    two, three = (sum(c[k] for c in _COMPARED.values()) for k in (0, 1))
    print("compared env-steps with two live finger-cube slots: %d, with three: %d" % (two, three))
    assert two >= MIN_TWO and three >= MIN_THREE, (two, three)
