"""Every built instantiation of the fused step kernel against the oracle, BIT FOR BIT.

The step kernel is built as 19 translation units; unit_for() in csrc/trifinger_hip.hip picks one from units[dr][surf][ext][width], and each unit
instantiates the kernel for A in {9, 18} x ASYM in {false, true} x its launch modes.  This file walks that table: a cell is

    (family, width, A, ASYM, path)      family = (dr, surf, ext): the row of the table, selected by the config (parity_util.MATRIX_FAMILIES)
                                        width  = narrow / wide / wide_helpers, forced with TrifingerEngine.kernel_variant
                                        A      = 9 (torque) or 18 (position_impedance);  ASYM = asymmetric_obs
                                        path   = step  (tf_reset, then tf_step with parity_util.actions_for: TF_LM_RESET, TF_LM_STEP)
                                                 rand  (tf_step_random: TF_LM_STEP_RAND, action_buf compared)
                                                 split (tf_apply_resets / pre_step / simulate / post_step / finish_step)

21 table cells x 4 x 3 = 252 GPU rollouts of 130 envs (two full wavefronts and a ragged one of 2 lanes) x 36 steps in 12-step episodes, compared with
parity_util.assert_bit_equal after the reset and after every step, no env excluded.  `step` and `rand` are compared with the oracle's rollout of the
same path; `split` with the oracle's FUSED rollout under the row exceptions test_split_path_equals_fused documents (the oracle's own split path equals
its fused one under the same exceptions: test_oracle_split_path_equals_its_fused_step, no GPU needed).  The id of a failure names the cell:
`d2_1-A18-sym-split`; the s0_* units launched with domain randomisation on (family (1, 1, 0)) are `ds0_1`, `ds0_2`.

Reach.  A rollout that stopped touching anything would still be bit-equal, so every rollout also has to get somewhere: the counts of
parity_util.matrix_reach are asserted on the oracle's 64 rollouts (CPU tests) and again on what each GPU cell produced.  In the cube families the cubes
of envs 65.. are placed at the boundary after the reset (parity_util.place_cubes_at_the_boundary; on the low-ring model of the surface families that is
on the cone); the box families are not placed.  Measured on the oracle, the minimum over the `step` and `rand` rollouts of all cube families (24 + 24)
and of the box families (8 + 8), 130 x 36 = 4680 env-steps each, non-finite states 0 in every one:

                    live finger-cube   >= 2 live   boundary   cone (surface    time-outs   goal     torque repeats
                    slot                slots      contact    families only)               resets   (families with DR)
    cube families   971                 88          650        640              260         77       885
    box families    279                 11          (0: none)  -                260         26       885

Every floor is HALF of the measured minimum (the rollouts are seeded: that leaves room for a deliberate change of the spec, none for a rollout that
lost its contacts); time-outs are exactly 2 x 130 = 260.  With domain randomisation the six factor rows must leave 1.0 and (action_repeat_prob 0.2 in
every DR family) a non-zero applied torque must repeat bit for bit from one snapshot to the next at least half as often as measured.  If a floor is
missed: change the seed or the placement, never the floor.

What these rollouts do NOT reach: a census of the oracle (make -C oracle census) finds a live middle-distal finger-finger row in 3 .. 97 env-steps of
every `step` rollout but NO substep with two of them in any - nothing in which the placement of those rows, the order of their additions or a second
mailbox message could show.  That is pinned by tests/test_parity_ff_shared_finger.py: the same cells on rollouts of tangled finger poses.
"""
import os
import re
from collections import OrderedDict

import pytest

import parity_util as pu

DEV = "cuda:0"
WIDTHS = ("narrow", "wide", "wide_helpers")            # index = width of unit_for's table

# the non-null entries of units[2][2][3][3] as csrc/trifinger_hip.hip writes them: (dr, surf, ext, width) -> unit.  Kept as data on purpose: a unit
# added to (or taken from) the table without extending this matrix fails test_the_matrix_is_the_table_of_built_units.
TABLE_CELLS = [
    (0, 0, 0, 0, "0_0"), (0, 0, 0, 1, "0_1"), (0, 0, 0, 2, "0_2"),
    (0, 0, 2, 0, "2_0"), (0, 0, 2, 1, "2_1"), (0, 0, 2, 2, "2_2"),
    (0, 1, 0, 1, "s0_1"), (0, 1, 0, 2, "s0_2"),
    (1, 0, 0, 0, "d0_0"), (1, 0, 0, 1, "d0_1"), (1, 0, 0, 2, "d0_2"),
    (1, 0, 1, 0, "1_0"), (1, 0, 1, 1, "1_1"), (1, 0, 1, 2, "1_2"),
    (1, 0, 2, 0, "d2_0"), (1, 0, 2, 1, "d2_1"), (1, 0, 2, 2, "d2_2"),
    (1, 1, 0, 1, "s0_1"), (1, 1, 0, 2, "s0_2"),
    (1, 1, 1, 1, "s1_1"), (1, 1, 1, 2, "s1_2"),
]

# measured minima over the oracle's rollouts (module docstring); the asserted floor is half of each
MEASURED = {"cube": dict(live_fc=971, two_live=88, boundary=650, cone=640, goal_resets=77, tau_repeats=885),
            "box": dict(live_fc=279, two_live=11, goal_resets=26, tau_repeats=885)}      # (the boundary: 0 in two box rollouts, no floor)
TIMEOUTS = 2 * pu.MATRIX_N


def _label(dr, surf, ext, width, unit):
    return ("d" if dr and surf and not ext else "") + unit


def _tag(a, asym):
    return f"A{a}-{'asym' if asym else 'sym'}"


COMBOS = [(family, a, asym) for family in pu.MATRIX_FAMILIES for a in (9, 18) for asym in (False, True)]
COMBO_IDS = [f"{'d' if f == (1, 1, 0) else ''}{pu.MATRIX_FAMILIES[f]}-{_tag(a, asym)}" for f, a, asym in COMBOS]
# the widths of a (family, A, ASYM, path) follow each other, and `split` follows `step` (it is compared with the same oracle rollout): the cache of oracle
# rollouts below then holds what the next test needs
GPU_CELLS = [pytest.param((dr, surf, ext), WIDTHS[width], a, asym, path, id=f"{_label(dr, surf, ext, width, unit)}-{_tag(a, asym)}-{path}")
             for family, a, asym in COMBOS for path in ("step", "split", "rand")
             for dr, surf, ext, width, unit in TABLE_CELLS if (dr, surf, ext) == family]

_ORACLE = OrderedDict()           # (family, a, asym, path) -> (snapshots, reach); the last few only (a rollout is 6.5 MB, all of them 0.4 GB)


def _oracle_rollout(oracle, family, a, asym, path):
    key = (family, a, asym, path)
    if key not in _ORACLE:
        snaps = pu.matrix_rollout(oracle, "cpu", family, a, asym, path)
        _ORACLE[key] = (snaps, pu.matrix_reach(snaps, family, pu.matrix_model(oracle, family)))
        while len(_ORACLE) > 4:
            _ORACLE.popitem(last=False)
    return _ORACLE[key]


def _assert_reach(r, family, what):
    """the floors of the module docstring on the counts `r` of parity_util.matrix_reach"""
    dr, surf, ext = family
    print(f"\n{what}: {r}")
    assert r["nonfinite"] == 0.0, (what, r)
    assert r["timeouts"] == TIMEOUTS, (what, r)                 # every env timed out exactly twice
    for name, measured in MEASURED["box" if ext == 2 else "cube"].items():
        if name in r:                                           # `cone`: surface families, `tau_repeats`: families with domain randomisation
            assert 2 * r[name] >= measured > 0, (what, name, r[name], measured)
    assert ("cone" in r) == bool(surf) and ("tau_repeats" in r) == bool(dr), (what, r)
    if dr:
        assert r["factors_drawn"], (what, r)


# ---- CPU: the table, the oracle's reach, the oracle's split path ---------------------------------------------------------------------------------
def test_the_matrix_is_the_table_of_built_units():
    """TABLE_CELLS == the non-null entries of units[2][2][3][3] of unit_for() as the source writes them (the full build's table, not TF_DEV_MIN's),
    and every row of the table is a family of parity_util.MATRIX_FAMILIES with units of that family's name"""
    src = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "leibnizgym_amd", "csrc", "trifinger_hip.hip")).read()
    body = src[src.index("static const EnvUnit* unit_for("):]
    body = body[body.index("#else"):body.index("#endif")]
    table = body[body.index("units[2][2][3][3]"):]
    table = table[:table.index("};")]
    entries = re.findall(r"nullptr|&tf_unit_(\w+)", table.split("=", 1)[1])
    assert len(entries) == 2 * 2 * 3 * 3, entries              # re.findall gives "" for a nullptr
    in_source = [(i // 18, i // 9 % 2, i // 3 % 3, i % 3, unit) for i, unit in enumerate(entries) if unit]
    assert in_source == TABLE_CELLS
    assert len(TABLE_CELLS) == 21 and len(GPU_CELLS) == 21 * 4 * 3
    assert sorted({c[:3] for c in TABLE_CELLS}) == sorted(pu.MATRIX_FAMILIES)
    for dr, surf, ext, width, unit in TABLE_CELLS:
        assert unit == f"{pu.MATRIX_FAMILIES[(dr, surf, ext)]}_{width}", unit
        assert (width == 0) <= (not surf)                       # the surface families have no `narrow`
    ids = [p.id for p in GPU_CELLS]
    assert len(set(ids)) == len(ids)


@pytest.mark.parametrize("path", ("step", "rand"))
@pytest.mark.parametrize("family,a,asym", COMBOS, ids=COMBO_IDS)
def test_reach_of_the_matrix_rollouts_on_the_oracle(oracle, family, a, asym, path):
    _assert_reach(_oracle_rollout(oracle, family, a, asym, path)[1], family, f"oracle {family} {_tag(a, asym)} {path}")


@pytest.mark.parametrize("family,a,asym", COMBOS, ids=COMBO_IDS)
def test_oracle_split_path_equals_its_fused_step(oracle, family, a, asym):
    """what lets the GPU's split path be compared with the oracle's FUSED rollout: the oracle's five split entries give what its tf_step gives, under
    the row exceptions of test_split_path_equals_fused"""
    fused = _oracle_rollout(oracle, family, a, asym, "step")[0]
    split = pu.matrix_rollout(oracle, "cpu", family, a, asym, "split")
    for t, (x, y) in enumerate(zip(split, fused)):
        pu.assert_split_equals_fused(x, y, f"oracle split vs fused {family} {_tag(a, asym)} snapshot {t}")


# ---- GPU: the 252 cells --------------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("family,variant,a,asym,path", GPU_CELLS)
def test_cell_bit_exact(hip, oracle, family, variant, a, asym, path):
    want, _ = _oracle_rollout(oracle, family, a, asym, "step" if path == "split" else path)
    got = pu.matrix_rollout(hip, DEV, family, a, asym, path, variant=variant)          # (the engine must accept its variant: matrix_engine)
    what = f"{family} [{variant}] {_tag(a, asym)} {path}"
    for t, (x, y) in enumerate(zip(got, want)):
        if path == "split":
            pu.assert_split_equals_fused(x, y, f"{what} snapshot {t}")
        else:
            pu.assert_bit_equal(x, y, f"{what} snapshot {t}")
    _assert_reach(pu.matrix_reach(got, family, pu.matrix_model(oracle, family)), family, what)
