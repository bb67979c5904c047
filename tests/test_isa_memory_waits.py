"""Where the vector-memory traffic of the headline step kernel sits (CPU suite; needs hipcc, no GPU).

On gfx950 loads, stores and scratch traffic share one in-order counter, so a wait for one reloaded dword also waits for every older
store, and every wait inside the sweep loops would be paid 16 times a step.  DESIGN.md section 4 claims what this file guards:
no spill traffic and no vector-memory instruction inside the sweep loops, no dependent round trips on the warm-start rows, and a
bounded number of spills and of waits that hide nothing.  The figures come from tools/isa_waits.py (one compile of unit 0_0 with the
Makefile's flags, a linear model of the counter); the caps are the figures of this build, next to those of the build before it.
"""
import os
import sys

import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "tools"))
import isa_waits  # noqa: E402

# figure: (cap = this build, the build before the memory-wait pass).  A cap is never looser than the older figure.
CAPS = {
    "vgpr_spills": (41, 49),
    "sgpr_spills": (62, 100),
    "scratch_bytes": (120, 144),
    "single_load_waits": (19, 26),
    "store_covering_waits": (12, 12),
}


@pytest.fixture(scope="module")
def headline():
    if isa_waits.find_hipcc() is None:
        pytest.skip("hipcc not found: the ISA of the step kernel cannot be produced")
    r = isa_waits.run(unit="0_0", kernel=isa_waits.HEADLINE, dev_min=True)
    print("\n".join("%-28s %s" % kv for kv in r["summary"].items()))
    return r


def test_headline_kernel_shape(headline):
    s = headline["summary"]
    assert s["vgprs"] == 128 and s["occupancy"] == 4, s            # the 128-register kernel: four workgroups per CU
    assert s["barriers"] >= 20 and s["instructions"] > 10000, s    # the scan saw the whole kernel, not a stub


def test_sweep_loops_hold_no_memory_traffic(headline):
    """(i) the loops whose body holds the two sweep barriers (W1, W2): one per role, LDS and registers only"""
    sweeps = [lp for lp in headline["loops"] if lp["innermost"] and lp["barriers"] >= 2]
    assert len(sweeps) >= 2, [(lp["label"], lp["barriers"]) for lp in headline["loops"]]     # finger role and cube role
    for lp in sweeps:
        assert lp["barriers"] == 2, (lp["label"], lp["barriers"])
        assert not lp["scratch"], [(x.text, x.loc) for x in lp["scratch"]]
        assert not lp["vmem"], [(x.text, x.loc) for x in lp["vmem"]]


def test_no_serialised_state_row_loads(headline):
    """(ii) no chain of two or more single-load waits on state rows (load, wait, load, wait: a round trip each)"""
    bad = [[(w["load_text"], w["load_loc"]) for w in c] for c in headline["chains"] if isa_waits.max_run(c) >= 2]
    assert not bad, bad
    assert headline["summary"]["longest_state_row_chain"] == 0


@pytest.mark.parametrize("figure", sorted(CAPS))
def test_caps(headline, figure):
    """(iii) spills, scratch and the waits that hide nothing do not grow"""
    cap, before = CAPS[figure]
    assert cap <= before
    got = headline["summary"][figure]
    assert got is not None and got <= cap, (figure, got, cap)
