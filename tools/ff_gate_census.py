"""Developer tool (CPU only): how often the middle-distal finger-finger rows are near, pass the link-speed gate and are live - on the oracle.

    python tools/ff_gate_census.py [--envs 4096] [--settle 400] [--steps 60] [--out profiles/r18_ff_gate_census.txt]

The kernels build a middle-distal row only where the gap can close within the substep at the fastest the two links can move
(csrc/tf_contact.h: ff_link_speeds, ff_gate).  This script copies oracle/tf_oracle.c to a temporary directory, applies
tools/experiments/ff_gate_census.patch (instrumentation inside #ifdef TF_FF_CENSUS: the C twin of the kernels' bound; the committed oracle stays as it
is), builds it with the flags of `make -C oracle census` and steps the bench workload: bench.workload_kwargs(True), step counters spread over the
episode, seeded random actions 2 U - 1, `--settle` steps, then `--steps` census steps.  Per pair - first group (0;2) (1;0) (2;1), second group (0;1)
(1;2) (2;0) - and control step, both substeps ORed: the share of lanes and of wavefronts (64 consecutive envs) with gap < contact_margin (what the
kernels used to test), with the gate open, and with contact_live true (what the result needs).  VIOLATIONS - a row that is live where the gate is
shut - must be 0: the script exits 1 otherwise.  The bound in the patch is a hand-written C twin of csrc/tf_contact.h (ff_link_speeds) and of the
constants of tf_create: the census speaks for the kernels only while those stay the same lines.
"""
import argparse
import ctypes as C
import os
import shutil
import subprocess
import sys
import tempfile

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
import bench  # noqa: E402
from leibnizgym_amd._capi import TfLib  # noqa: E402
from leibnizgym_amd.engine import TrifingerEngine, make_config  # noqa: E402

PAIRS = ("(0;2)", "(1;0)", "(2;1)", "(0;1)", "(1;2)", "(2;0)")
SEED = 18


def oracle_cflags():
    """the CFLAGS line of oracle/Makefile: the census is built with the flags of the oracle it instruments"""
    for line in open(os.path.join(REPO, "oracle", "Makefile")):
        if line.startswith("CFLAGS"):
            return line.split("=", 1)[1].split()
    raise RuntimeError("oracle/Makefile: no CFLAGS line")


def build(tmp):
    os.makedirs(os.path.join(tmp, "oracle"))
    shutil.copy(os.path.join(REPO, "oracle", "tf_oracle.c"), os.path.join(tmp, "oracle"))
    for name in os.listdir(os.path.join(REPO, "oracle")):
        if name.endswith(".h"):
            shutil.copy(os.path.join(REPO, "oracle", name), os.path.join(tmp, "oracle"))
    subprocess.check_call(["patch", "-s", "-p1", "-i", os.path.join(REPO, "tools", "experiments", "ff_gate_census.patch")], cwd=tmp)
    so = os.path.join(tmp, "libtrifinger_oracle_ffg.so")
    subprocess.check_call([os.environ.get("CC", "cc")] + oracle_cflags() + ["-I", os.path.join(REPO, "oracle"), "-I", os.path.join(REPO, "include"), "-DTF_FF_CENSUS",
                           "-shared", "-o", so, os.path.join(tmp, "oracle", "tf_oracle.c"), "-lm"])
    lib = TfLib(so)
    lib.dll.tf_census_bind.argtypes = [C.c_void_p, C.c_void_p]
    lib.dll.tf_census_bind.restype = C.c_int
    lib.dll.tf_ffg_counters.argtypes = [C.POINTER(C.c_int64), C.c_int]
    lib.dll.tf_ffg_counters.restype = C.c_int
    return lib


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--envs", type=int, default=4096)
    ap.add_argument("--settle", type=int, default=400)
    ap.add_argument("--steps", type=int, default=60)
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "r18_ff_gate_census.txt"))
    args = ap.parse_args()
    n = args.envs
    assert n % 64 == 0, "whole wavefronts"
    with tempfile.TemporaryDirectory() as tmp:
        lib = build(tmp)
        eng = TrifingerEngine(make_config(lib, n, seed=SEED, **bench.workload_kwargs(True)), device="cpu", lib=lib)
        mask = np.zeros(n, dtype=np.int32)
        assert lib.dll.tf_census_bind(eng._handle, C.c_void_p(mask.ctypes.data)) == 0
        g = torch.Generator().manual_seed(SEED)
        eng.reset()
        eng.steps.copy_(torch.randint(0, int(eng.cfg.episode_length), (n,), generator=g, dtype=torch.int64))
        for _ in range(args.settle):
            eng.step((torch.rand(n, eng.action_dim, generator=g) * 2 - 1).contiguous())
        cnt = (C.c_int64 * 4)()
        lib.dll.tf_ffg_counters(cnt, 1)
        lanes = np.zeros((3, 6))
        waves = np.zeros((3, 6))
        for _ in range(args.steps):
            mask[:] = 0
            eng.step((torch.rand(n, eng.action_dim, generator=g) * 2 - 1).contiguous())
            u = mask.view(np.uint32)
            for c, first in enumerate((13, 19, 25)):
                for p in range(6):
                    bit = ((u >> np.uint32(first + p)) & np.uint32(1)).astype(bool)
                    lanes[c, p] += bit.mean()
                    waves[c, p] += bit.reshape(-1, 64).any(axis=1).mean()
        lib.dll.tf_ffg_counters(cnt, 0)
        eng.close()
    lanes *= 100.0 / args.steps
    waves *= 100.0 / args.steps
    live, above, above2, bad = (int(x) for x in cnt)
    rows = ["link-speed gate of the middle-distal rows: census on the oracle (tools/ff_gate_census.py)",
            f"workload: bench.workload_kwargs(True), {n} envs, counters spread over the episode, random actions, {args.settle} settle steps, {args.steps} census steps",
            "per pair and control step, both substeps ORed; wavefront = 64 consecutive envs; per cent of lanes / of wavefronts with at least one such lane", "",
            "%-34s" % "pair (fm;fd)" + "".join("%16s" % p for p in PAIRS)]
    for c, name in enumerate(("gap < contact_margin (old entry)", "gate open (new entry)", "contact_live (needed)")):
        rows.append("%-34s" % name + "".join("%7.2f /%6.1f " % (lanes[c, p], waves[c, p]) for p in range(6)))
    rows += ["", f"live rows (per substep): {live}; with gap > contact_slack: {above}; with gap > 2 contact_slack: {above2}",
             f"VIOLATIONS (live row, gate shut): {bad}"]
    text = "\n".join(rows) + "\n"
    print(text, end="")
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(text)
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
