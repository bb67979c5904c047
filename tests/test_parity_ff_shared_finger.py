"""The finger-finger pre-pass of every built step-kernel unit against the oracle, BIT FOR BIT, where several live rows change one finger.

The pre-pass (three distal pairs in turn, then six middle-distal rows solved on the free velocities and ADDED in the order the pairs are listed:
oracle/tf_oracle.c above `if (m->ff_middle_pairs)`) is built in four placements - all six rows on the cube wavefront, the first group there and the
second on the finger wavefronts, all six on the finger wavefronts with mailboxes, or posted by the helper wavefronts (csrc/tf_roles.h between S1 and
S1b, tf_ff_distal.inc).  The order of the additions, the second mailbox message of a finger, its second own-row slot and the hand-over between the two
groups can be wrong only in a substep in which one finger is changed by two or more live rows - and the rollouts of tests/test_parity_unit_matrix.py
hold no substep with even two live middle-distal rows.  The rollouts of this file are made of such substeps.

Rollout.  parity_util.matrix_engine(family, A, ASYM) as in the unit matrix: reset, then ff_census_util.place_tangled_fingers overwrites q and dq/dt of
all 130 envs with poses harvested on the census build of the oracle (make -C oracle census; ff_census_util.harvest: 5 x 40000 robot resets spread with
dof_pos_stddev 2.5, each classed by the rows its next step had live together; filled pool index ascending with 40 MB2, 40 OWN2, 10 M3, 20 X, 10 DM,
10 D2 - 130 distinct poses, half of every class on either full wavefront, one MB2 and one OWN2 pose on lanes 128 and 129), then 12 steps - an episode
less its time-out reset.  Snapshots after the placement and after every step, compared with parity_util.assert_bit_equal / assert_split_equals_fused
against the PLAIN oracle, no env and no field excluded.  Cells: every entry of the unit matrix's TABLE_CELLS with its width forced, x (A9, asym),
(A18, sym) x step / split / rand = 126 GPU rollouts.

Reach.  Classes (ff_census_util, decided once per substep over the rows with lambda > 0): D1 a distal pair is live, D2 two or more; M1 a middle-distal
row, M2 two or more; MB2_f finger f is the distal side of two rows (second mailbox message), OWN2_f finger f owns two live rows (second own-row
slot), MB2 / OWN2 any f; X a finger is changed by a row of either group; DM by a distal pair and a middle-distal row; M3 by three or more
middle-distal rows.  Measured on the census oracle (which test_census_build_is_the_plain_oracle holds to the plain one bit for bit), the minimum over
the `step` and `rand` rollouts of (A9, asym) and (A18, sym) of the six cube families (24) and the two box families (8), 130 x 12 = 1560 env-steps
each, non-finite states 0 in every one; env-steps, and for MB2 / OWN2 / M3 also the envs that ever had one:

                     D1   D2   M1   M2  MB2  MB2_0 MB2_1 MB2_2  OWN2  OWN2_0 OWN2_1 OWN2_2    X   DM   M3   envs: MB2  OWN2   M3
    cube families   571   62  484  129   30      7    12    10    60      23     14     21  109  253   15          27    42   15
    box families    566   57  489  134   30      7    12    10    65      23     15     21  115  251   15          27    46   15

Every floor is HALF of the measured minimum, as in the unit matrix; conditions rather than measurements: every MB2_f and OWN2_f is non-zero in every
rollout, no pose is used twice, every env is compared.  If a floor is missed: change the seed or the selection, never the floor.

Sensitivity (measured once on the CPU with a scratch copy of the oracle that visits the two groups in the other order, o_ = 1 then 2; not kept):
against the plain oracle, families (0,0,0) and (0,0,2), `step`: this file's rollout differs in 54 of 130 envs after the first step with (A9, asym)
(75 within the 12 steps) and in 49 (56) with (A18, sym); the unit matrix's rollout in 0 of 130 envs over all its 36 steps, either combination.
And once on the GPU with a scratch build of the kernels in which finger 2 adds its own row of the first group before the row it received
(csrc/tf_roles.h behind S1b; the 256-register units only): 96 of the 126 cells of this file fail - all but the 30 of the 128-register units - while
the unit matrix's `step` cells of the same combinations all pass.
"""
import numpy as np
import pytest

import ff_census_util as fc
import parity_util as pu
from leibnizgym_amd import _capi as capi
from test_parity_unit_matrix import TABLE_CELLS, WIDTHS, _label, _tag

DEV = "cuda:0"

# measured minima over the census oracle's rollouts (module docstring); the asserted floor is half of each.  name -> env-steps; ENVS: envs that ever had one
MEASURED = {"cube": dict(D1=571, D2=62, M1=484, M2=129, MB2=30, MB2_0=7, MB2_1=12, MB2_2=10, OWN2=60, OWN2_0=23, OWN2_1=14, OWN2_2=21, X=109, DM=253,
                         M3=15),
            "box": dict(D1=566, D2=57, M1=489, M2=134, MB2=30, MB2_0=7, MB2_1=12, MB2_2=10, OWN2=65, OWN2_0=23, OWN2_1=15, OWN2_2=21, X=115, DM=251,
                        M3=15)}
MEASURED_ENVS = {"cube": dict(MB2=27, OWN2=42, M3=15), "box": dict(MB2=27, OWN2=46, M3=15)}

COMBOS = [(family, a, asym) for family in pu.MATRIX_FAMILIES for a, asym in ((9, True), (18, False))]
COMBO_IDS = [f"{'d' if f == (1, 1, 0) else ''}{pu.MATRIX_FAMILIES[f]}-{_tag(a, asym)}" for f, a, asym in COMBOS]
GPU_CELLS = [pytest.param((dr, surf, ext), WIDTHS[width], a, asym, path, id=f"{_label(dr, surf, ext, width, unit)}-{_tag(a, asym)}-{path}")
             for family, a, asym in COMBOS for path in ("step", "split", "rand")
             for dr, surf, ext, width, unit in TABLE_CELLS if (dr, surf, ext) == family]

_ORACLE = {}           # (family, a, asym, path) -> snapshots of the plain oracle (13 x 0.2 MB each, 32 of them)
_CENSUS = {}           # ... -> (snapshots, masks) of the census build


def _oracle_rollout(oracle, family, a, asym, path):
    key = (family, a, asym, path)
    if key not in _ORACLE:
        _ORACLE[key] = fc.rollout(oracle, "cpu", family, a, asym, path)
    return _ORACLE[key]


def _census_rollout(family, a, asym, path):
    key = (family, a, asym, path)
    if key not in _CENSUS:
        _CENSUS[key] = fc.rollout(fc.census_library(), "cpu", family, a, asym, path, census=True)
    return _CENSUS[key]


def _nonfinite(snaps):
    return float(sum(s["info"][capi.INFO_NUM_NONFINITE] for s in snaps[1:]))


# ---- CPU: the poses, the census build, the oracle's reach, the oracle's split path -----------------------------------------------------------------
def test_the_cells_are_the_table_of_built_units():
    assert len(GPU_CELLS) == len(TABLE_CELLS) * 2 * 3 == 126
    ids = [p.id for p in GPU_CELLS]
    assert len(set(ids)) == len(ids)


def test_poses_are_distinct_and_every_wavefront_holds_every_class():
    poses, classes = fc.harvest()
    assert poses.shape == (fc.POSE_ROWS, pu.MATRIX_N) and np.isfinite(poses).all()
    assert len({poses[:, i].tobytes() for i in range(pu.MATRIX_N)}) == pu.MATRIX_N                  # no pose twice
    for lanes in (slice(0, 64), slice(64, 128)):                                                    # the two full wavefronts
        for name in ("MB2_0", "MB2_1", "MB2_2", "OWN2_0", "OWN2_1", "OWN2_2", "M3", "X", "DM", "D2"):
            assert (classes[lanes] & fc.CLASSES[name]).any(), (lanes, name)
    assert classes[128] & fc.MB2 and classes[129] & fc.OWN2                                         # the ragged one: one of each


@pytest.mark.parametrize("path", ("step", "rand"))
@pytest.mark.parametrize("family,a,asym", COMBOS, ids=COMBO_IDS)
def test_census_build_is_the_plain_oracle(oracle, family, a, asym, path):
    """the census build gives the plain oracle's bits on this rollout: its masks say what the plain oracle's substeps held"""
    want = _oracle_rollout(oracle, family, a, asym, path)
    got, masks = _census_rollout(family, a, asym, path)
    assert len(got) == len(want) == fc.STEPS + 1 and masks.shape == (fc.STEPS, pu.MATRIX_N)
    for t, (x, y) in enumerate(zip(got, want)):
        pu.assert_bit_equal(x, y, f"census vs plain {family} {_tag(a, asym)} {path} snapshot {t}")


@pytest.mark.parametrize("path", ("step", "rand"))
@pytest.mark.parametrize("family,a,asym", COMBOS, ids=COMBO_IDS)
def test_reach_of_the_rollouts_on_the_oracle(family, a, asym, path):
    """the floors of the module docstring on the masks of the census oracle's rollout"""
    snaps, masks = _census_rollout(family, a, asym, path)
    what = f"census oracle {family} {_tag(a, asym)} {path}"
    r = fc.reach(masks)
    print(f"\n{what}: " + "  ".join(f"{k} {v[0]}/{v[1]}" for k, v in r.items()))
    assert _nonfinite(snaps) == 0.0, what
    kind = "box" if family[2] == 2 else "cube"
    for name, measured in MEASURED[kind].items():
        assert 2 * r[name][0] >= measured > 0, (what, name, r[name], measured)
    for name, measured in MEASURED_ENVS[kind].items():
        assert 2 * r[name][1] >= measured > 0, (what, name, r[name], measured)
    for f in range(3):                                          # conditions, not measurements
        assert r[f"MB2_{f}"][0] > 0 and r[f"OWN2_{f}"][0] > 0, (what, f, r)


@pytest.mark.parametrize("family,a,asym", COMBOS, ids=COMBO_IDS)
def test_oracle_split_path_equals_its_fused_step(oracle, family, a, asym):
    """what lets the GPU's split path be compared with the oracle's FUSED rollout, on these rollouts: the oracle's five split entries give what its
    tf_step gives, under the row exceptions of test_split_path_equals_fused"""
    fused = _oracle_rollout(oracle, family, a, asym, "step")
    split = fc.rollout(oracle, "cpu", family, a, asym, "split")
    for t, (x, y) in enumerate(zip(split, fused)):
        pu.assert_split_equals_fused(x, y, f"oracle split vs fused {family} {_tag(a, asym)} snapshot {t}")


# ---- GPU: the 126 cells ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("family,variant,a,asym,path", GPU_CELLS)
def test_cell_bit_exact(hip, oracle, family, variant, a, asym, path):
    want = _oracle_rollout(oracle, family, a, asym, "step" if path == "split" else path)
    got = fc.rollout(hip, DEV, family, a, asym, path, variant=variant)                 # (the engine must accept its variant: matrix_engine)
    what = f"{family} [{variant}] {_tag(a, asym)} {path}"
    assert len(got) == len(want) == fc.STEPS + 1
    for t, (x, y) in enumerate(zip(got, want)):
        if path == "split":
            pu.assert_split_equals_fused(x, y, f"{what} snapshot {t}")
        else:
            pu.assert_bit_equal(x, y, f"{what} snapshot {t}")
    assert _nonfinite(got) == 0.0, what
