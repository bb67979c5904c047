"""The headline unit 0_0 is built without domain randomisation (CPU suite; needs hipcc, no GPU).

`dr_enable` is fixed at tf_create, so the units 0_0 / 0_1 / 0_2 carry no domain-randomisation code at all (tf_env_kernels.hip: DR_RT) and the same
kernels with the run-time flag live in d0_0 / d0_1 / d0_2 (k_env_dr).  What that buys is register pressure in the 128-register kernel: this file holds
the figures of this build - tools/isa_waits.py on the kernel bench.py times - next to those of the same kernel with the run-time flag (which are the
caps of tests/test_isa_memory_waits.py; no cap here is looser), and checks that the d0_0 unit still is the kernel with the flag.
"""
import os
import sys

import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "tools"))
import isa_waits  # noqa: E402

# figure: (cap = this build, the same kernel with domain randomisation as a run-time flag = unit d0_0)
CAPS = {
    "instructions": (17353, 19211),
    "vgpr_spills": (28, 41),
    "sgpr_spills": (61, 62),
    "scratch_bytes": (108, 120),
    "scratch_loads": (42, 68),
    "scratch_stores": (25, 41),
    "global_loads": (110, 128),
    "single_load_waits": (14, 19),
    "single_load_waits_scratch": (12, 17),
    "store_covering_waits": (12, 12),
    "barriers": (20, 24),
}


@pytest.fixture(scope="module")
def headline():
    if isa_waits.find_hipcc() is None:
        pytest.skip("hipcc not found: the ISA of the step kernel cannot be produced")
    r = isa_waits.run(unit="0_0", kernel=isa_waits.HEADLINE, dev_min=True)
    print("\n".join("%-28s %s" % kv for kv in r["summary"].items()))
    return r


@pytest.fixture(scope="module")
def with_flag():
    if isa_waits.find_hipcc() is None:
        pytest.skip("hipcc not found: the ISA of the step kernel cannot be produced")
    r = isa_waits.run(unit="d0_0", kernel=isa_waits.HEADLINE, dev_min=True)
    print("\n".join("%-28s %s" % kv for kv in r["summary"].items()))
    return r


@pytest.mark.parametrize("figure", sorted(CAPS))
def test_caps(headline, figure):
    cap, flag = CAPS[figure]
    assert cap <= flag
    got = headline["summary"][figure]
    assert got is not None and got <= cap, (figure, got, cap)


def test_caps_are_not_looser_than_those_of_the_memory_wait_pass():
    import test_isa_memory_waits as older
    for figure, (cap, _) in older.CAPS.items():
        assert CAPS[figure][0] <= cap, (figure, CAPS[figure][0], cap)


def _state_row_loads(r, row):
    """global loads of the kernel whose source line is one that reads state row `row` (tf_roles.h; -gline-tables-only)"""
    src = open(os.path.join(isa_waits.CSRC, "tf_roles.h")).read().split("\n")
    lines = {"tf_roles.h:%d" % (k + 1) for k, l in enumerate(src) if "LDST(%s" % row in l}
    assert lines, row
    return [i for i in r["ins"] if i.kind == "gload" and i.loc in lines]


def test_cube_role_substep_loop_touches_no_memory(headline):
    """With the flag the cube role asks for its TF_S_DR rows again at the head of every substep and waits for them with everything older drained;
    without it the loop over the substeps of the cube role - the outer loop around the cube role's sweep loop - holds LDS and registers only."""
    loops = headline["loops"]
    sweeps = [lp for lp in loops if lp["innermost"] and lp["barriers"] >= 2]
    assert len(sweeps) == 2, [(lp["label"], lp["barriers"]) for lp in loops]
    cube_sweep = max(sweeps, key=lambda lp: lp["size"])          # the cube role's sweep carries the serial chain: 826 instructions against the finger role's 170
    outer = [lp for lp in loops if lp is not cube_sweep and cube_sweep["blocks"] < lp["blocks"]]
    assert len(outer) == 1, [(lp["label"], lp["size"]) for lp in outer]
    assert not outer[0]["vmem"], [(x.text, x.loc) for x in outer[0]["vmem"]]
    assert not outer[0]["scratch"], [(x.text, x.loc) for x in outer[0]["scratch"]]


def test_headline_kernel_reads_no_dr_row(headline):
    assert not _state_row_loads(headline, "TF_S_DR")
    assert _state_row_loads(headline, "TF_S_CUBE_P")              # (the line lookup does find rows that are read)


def test_flag_unit_is_the_kernel_with_the_flag(with_flag):
    """d0_0 compiles, its kernel is k_env_dr with the headline's template arguments, and it still reads the TF_S_DR rows"""
    s = with_flag["summary"]
    assert "k_env_dr" in with_flag["name"] and isa_waits.HEADLINE[len("k_env"):] in with_flag["name"], with_flag["name"]
    assert s["vgprs"] == 128 and s["occupancy"] == 4 and s["instructions"] > 10000, s
    assert len(_state_row_loads(with_flag, "TF_S_DR")) >= 6      # the six base factors, in the cube role's prologue at the least
    assert s["barriers"] >= 24, s                                 # the observation-noise barriers P4 / P5 of both roles are in the code object
