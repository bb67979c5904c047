"""The model's constants no longer sit in the spill slots of the 128-register step kernel (CPU suite; needs hipcc, no GPU).

The finger role of the headline kernel formed a dozen launch-invariant values on the vector ALU in front of its substep loop - the constant terms of the
mass matrix, 1 / cube_inertia, 1 - h damping, the base-frame images of the fingertip-floor row directions - found no register for them and reloaded them
from scratch in every substep, each reload a round trip to L2 behind every older store.  The host now forms them once, with the
same fp32 operations (tf_params.h: the fields behind ffm_inv_j; trifinger_hip.hip: fill_invariants), the kernels without domain randomisation fetch them
from the parameter block where they are used (fetch_here), and tid, lane and the env index are formed anew behind the substeps instead of living
through them in spill slots (tf_roles.h: ctx_again).  This file holds the figures of that build (tools/isa_waits.py on unit 0_0), each strictly below
the parent's, which stands beside it.

The count that matters is stated as one: scratch reloads, inside a loop that holds barriers, of a value that was stored in front of the loop and was
formed from scalar registers and literals only (isa_waits.loop_reloads: "uniform").  The parent had 9 of them among the 17 scratch instructions of the
finger role's substep loop; none is left.  The one scratch instruction that remains in that loop reloads a per-lane value, the float of the warm-start
code of the first substep, which no parameter block can hold.
"""
import os
import sys

import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "tools"))
import isa_waits  # noqa: E402

# figure: (cap = this build, the parent)
CAPS = {
    "barrier_loop_scratch_max": (1, 17),            # scratch instructions inside any one loop that holds barriers (the finger role's substep loop)
    "loop_reloads_of_preloop_stores": (1, 17),      # reloads in such loops of what was stored in front of the loop
    "loop_reloads_of_preloop_uniform": (0, 9),      # ... of values formed from scalar registers and literals only: the model's constants
    "vgpr_spills": (9, 22),
    "scratch_loads": (15, 33),
    "scratch_stores": (7, 21),
    "single_load_waits_scratch": (3, 9),
    "scratch_bytes": (40, 92),
}


@pytest.fixture(scope="module")
def headline():
    if isa_waits.find_hipcc() is None:
        pytest.skip("hipcc not found: the ISA of the step kernel cannot be produced")
    r = isa_waits.run(unit="0_0", kernel=isa_waits.HEADLINE, dev_min=True)
    print("\n".join("%-32s %s" % kv for kv in r["summary"].items()))
    return r


@pytest.mark.parametrize("figure", sorted(CAPS))
def test_caps(headline, figure):
    cap, parent = CAPS[figure]
    assert cap < parent                                            # every cap strictly below the parent's figure
    got = headline["summary"][figure]
    print("%s: %s (cap %s, parent %s)" % (figure, got, cap, parent))
    assert got is not None and got <= cap, (figure, got, cap)


def test_no_constant_of_the_launch_is_reloaded_in_a_barrier_loop(headline):
    for x in headline["reloads"]:
        print("slot %d (%d B) %s: stored %s, reloaded %s in %s" % (x["slot"], x["bytes"], "uniform" if x["uniform"] else "per lane",
                                                                  x["store"].loc, x["load"].loc, x["loop"]))
    uniform = [x for x in headline["reloads"] if x["uniform"]]
    assert len(uniform) == 0, [(x["slot"], x["store"].loc, x["load"].loc) for x in uniform]


def test_the_walk_tells_a_scalar_expression_from_a_lane_value():
    """isa_waits.wave_uniform on a hand-written block: a product of two SGPRs accumulated with a literal is uniform, a value that went through a lane's
    register or a load is not, and neither is one whose definition lies behind a change of EXEC."""
    lines = ["v_mul_f32_e64 v0, s36, s36", "v_fmac_f32_e64 v0, s94, s94", "v_mul_f32_e32 v1, s69, v0",       # m1 * (c1z c1z + c1x c1x)
             "v_lshlrev_b32_e32 v2, 2, v73", "v_or_b32_e32 v3, s20, v2",                                     # an LDS address of the lane
             "ds_read_b32 v4, v3", "v_add_f32_e32 v5, s1, v4",
             "scratch_store_dword off, v1, off offset:20", "scratch_store_dword off, v3, off offset:28", "scratch_store_dword off, v5, off offset:32",
             "v_mov_b32_e32 v6, 1.0", "s_or_b64 exec, exec, s[6:7]", "v_add_f32_e32 v7, s2, v6", "scratch_store_dword off, v7, off offset:36"]
    ins = [isa_waits.Ins(k, t.split()[0], t, isa_waits.classify(t.split()[0]), None, ()) for k, t in enumerate(lines)]
    assert isa_waits.wave_uniform(ins, 7, 1)
    assert not isa_waits.wave_uniform(ins, 8, 3)
    assert not isa_waits.wave_uniform(ins, 9, 5)
    assert not isa_waits.wave_uniform(ins, 13, 7)
    assert isa_waits.scratch_slot(ins[7]) == (20, 4)


def test_sweep_loops_and_older_caps_still_hold(headline):
    """the two figures of the older files that a different register allocation can move (tests/test_isa_fc_compaction.py holds them itself: restated here
    beside the figures of this build so that one run shows all of them)"""
    import test_isa_fc_compaction as older
    s = headline["summary"]
    assert s["instructions"] <= older.CAPS["instructions"][0], s["instructions"]
    sweeps = [lp for lp in headline["loops"] if lp["innermost"] and lp["barriers"] >= 2]
    assert len(sweeps) == 2 and max(lp["size"] for lp in sweeps) <= older.CUBE_SWEEP_MAX, [lp["size"] for lp in sweeps]
    assert not any(lp["scratch"] or lp["vmem"] for lp in sweeps)
