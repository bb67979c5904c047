"""The finger-cube blocks of the 128-register sweep loop run in per-lane order (CPU suite; needs hipcc, no GPU).

The cube role of the 128-register kernels no longer enters the block of finger f whenever any lane of the wavefront has a live contact with finger f:
once per substep every lane orders its live fingers, and pass k of a sweep solves the block of the lane's k-th live finger through a per-lane record
base (tf_roles.h, cube_role; tools/fc_census.py: 1.90 passes per sweep instead of 2.97 blocks on the headline workload).  It is the form with permuted
register arrays: three unrolled passes, the 1/D, bias and impulses of passes 0 and 1 in registers (those of the rare third pass stay in LDS).  This file
holds the shape of that loop in the gfx950 code of the headline kernel (tools/isa_waits.py on unit 0_0) and the figures of this build, none looser than
those of tests/test_isa_dr_off.py.
"""
import os
import re
import sys

import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "tools"))
import isa_waits  # noqa: E402

# figure: (cap = this build, the build before the per-lane order = the caps of tests/test_isa_dr_off.py)
CAPS = {
    "instructions": (17343, 17353),
    "vgpr_spills": (28, 28),
    "sgpr_spills": (61, 61),
    "scratch_bytes": (108, 108),
    "scratch_loads": (42, 42),
    "scratch_stores": (25, 25),
    "global_loads": (110, 110),
    "single_load_waits": (14, 14),
    "single_load_waits_scratch": (12, 12),
    "store_covering_waits": (12, 12),
    "barriers": (20, 20),
}
CUBE_SWEEP_MAX = 849          # instructions of the cube role's sweep loop in this build (826 before: the hand-over of the last sweep, which sits in the loop, now goes through LDS)
BLOCK_MARK = "FC_REC(f, R_DL + d) = dl[d];"         # the statement of the block that hands the impulse increments to the finger role


@pytest.fixture(scope="module")
def headline():
    if isa_waits.find_hipcc() is None:
        pytest.skip("hipcc not found: the ISA of the step kernel cannot be produced")
    r = isa_waits.run(unit="0_0", kernel=isa_waits.HEADLINE, dev_min=True)
    print("\n".join("%-28s %s" % kv for kv in r["summary"].items()))
    return r


def _cube_sweep(r):
    sweeps = [lp for lp in r["loops"] if lp["innermost"] and lp["barriers"] >= 2]
    assert len(sweeps) == 2, [(lp["label"], lp["barriers"]) for lp in r["loops"]]
    return max(sweeps, key=lambda lp: lp["size"])                # the cube role's sweep carries the serial chain; the finger role's has 170 instructions


def _loop_code(r, lp):
    """the instructions of a loop of isa_waits.find_loops, in text order"""
    ins = r["ins"]
    leaders = {0}
    for i in ins:
        if i.labels:
            leaders.add(i.idx)
        if i.op.startswith(("s_cbranch", "s_branch")) or i.op == "s_endpgm":
            leaders.add(i.idx + 1)
    starts = sorted(x for x in leaders if x < len(ins))
    out = []
    for b in sorted(lp["blocks"]):
        out += ins[starts[b]:(starts[b + 1] if b + 1 < len(starts) else len(ins))]
    return out


@pytest.mark.parametrize("figure", sorted(CAPS))
def test_caps(headline, figure):
    cap, before = CAPS[figure]
    assert cap <= before
    got = headline["summary"][figure]
    print("%s: %s (cap %s, before %s)" % (figure, got, cap, before))
    assert got is not None and got <= cap, (figure, got, cap)


def test_caps_are_not_looser_than_those_of_the_dr_off_build():
    import test_isa_dr_off as older
    assert set(CAPS) == set(older.CAPS)
    for figure, (cap, _) in older.CAPS.items():
        assert CAPS[figure][0] <= cap, (figure, CAPS[figure][0], cap)
        assert CAPS[figure][1] == cap, (figure, CAPS[figure][1], cap)      # the second column here IS the older build


def test_cube_sweep_loop_holds_two_barriers_and_no_memory_traffic(headline):
    lp = _cube_sweep(headline)
    print("cube role's sweep loop: %d instructions, %d barriers, vector-memory %d, scratch %d" % (lp["size"], lp["barriers"], len(lp["vmem"]), len(lp["scratch"])))
    assert lp["barriers"] == 2, lp["barriers"]
    assert not lp["vmem"], [(x.text, x.loc) for x in lp["vmem"]]
    assert not lp["scratch"], [(x.text, x.loc) for x in lp["scratch"]]
    assert lp["size"] <= CUBE_SWEEP_MAX, lp["size"]


def test_finger_cube_block_appears_three_times_in_the_sweep_loop(headline):
    """Three unrolled passes: the three impulse increments a block hands to the finger role (R_DL) are stored three times in the sweep loop, nine
    dwords, through three address registers - the per-lane record bases of pass 0 and pass 1, which are not the wavefront's lane base that every
    other LDS access of the loop goes through, and the base of pass 2, which is (a third live finger can only be finger 2)."""
    src = open(os.path.join(isa_waits.CSRC, "tf_roles.h")).read().split("\n")
    lines = {"tf_roles.h:%d" % (k + 1) for k, l in enumerate(src) if BLOCK_MARK in l}
    assert len(lines) == 1, lines
    code = _loop_code(headline, _cube_sweep(headline))
    stores = [i for i in code if i.op.startswith("ds_write") and i.loc in lines]
    per_base = {}
    for i in stores:
        base = re.split(r"[ ,]+", i.text)[1]
        per_base[base] = per_base.get(base, 0) + (2 if "write2" in i.op else 1)
    print("LDS stores of the impulse increments in the sweep loop, dwords per address register: %s" % per_base)
    assert len(per_base) == 3, per_base                             # three copies of the block, one per pass
    use = {}
    for i in code:
        if i.op.startswith(("ds_read", "ds_write")):
            t = re.split(r"[ ,]+", i.text)
            base = t[2] if i.op.startswith("ds_read") else t[1]
            use[base] = use.get(base, 0) + 1
    lane_base = max(use, key=use.get)                               # the wavefront's lane base: the corner rows and pass 2 go through it
    assert lane_base in per_base, (per_base, lane_base)
    for base, dwords in per_base.items():
        if base != lane_base:
            assert dwords == 3, (base, dwords)                      # pass 0 and pass 1: the three increments, through the lane's own record base
        else:
            assert 3 <= dwords <= 6, (base, dwords)                 # pass 2: the compiler may pair an increment with one of the pass's running impulses
