#!/usr/bin/env python3
"""Developer tool (GPU box): what a fingertip action costs (include/trifinger_kin.h: tfk_tip_action) beside the torch statement of the same law
(leibnizgym_amd/kinematics.py: tip_action_statement, float32 on the same device - what a user had before the library) and beside the env step.

    python tools/fingertip_action_cost.py all [--out profiles/fingertip_action_cost.txt] [--sizes 8192,65536]
        every measurement below in a FRESH child process under a time limit of its own; a child that fails ends the run
    python tools/fingertip_action_cost.py wall N       device events around REPS back-to-back calls, after a warm-up of the same calls, three rounds with the
                                                       variants alternating: the fused launch in both modes, the torch statement in both modes, the env step
    python tools/fingertip_action_cost.py program N    the program of a counter-free `rocprofv3 --kernel-trace --stats` run: the fused launch in both modes and
                                                       the env step, alternating - the KERNEL times
The bar: the fused launch costs less than the statement."""
import argparse
import os
import re
import statistics
import subprocess
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
REPS = 200


def setup(n):
    import torch
    from leibnizgym_amd import _capi as capi
    from leibnizgym_amd import kinematics as kin
    from leibnizgym_amd.engine import TrifingerEngine, make_config
    dev = "cuda:0"
    hip = capi.load_hip_library()
    eng = TrifingerEngine(make_config(hip, n, seed=1, command_mode="torque"), device=dev, lib=hip)
    eng.reset()
    for _ in range(10):
        eng.step_random()
    fk = kin.FingerKinematics(eng.cfg.model, device=dev)
    g = torch.Generator(device=dev).manual_seed(3)
    cmd = torch.rand(n, 9, device=dev, generator=g) * 2 - 1
    action, target = torch.empty(n, 9, device=dev), torch.empty(n, 9, device=dev)
    variants = {}
    for mode in ("position", "torque"):
        p, d = kin.action_params("delta", mode, True)
        variants[f"fused {mode}"] = (lambda p=p: fk.tip_action(p, cmd, eng.q.T, eng.qd.T, action, target))
        variants[f"torch {mode}"] = (lambda d=d: kin.tip_action_statement(fk.constants, d, cmd, eng.q.T, eng.qd.T))
    variants["env step"] = eng.step_random
    return torch, variants


def cmd_wall(args):
    torch, variants = setup(args.n)
    times = {k: [] for k in variants}
    for fn in variants.values():                                   # warm-up of every shape the timed windows use
        for _ in range(20):
            fn()
    torch.cuda.synchronize()
    for _ in range(3):
        for name, fn in variants.items():
            reps = REPS if name.startswith("fused") or name == "env step" else 20
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            for _ in range(reps):
                fn()
            b.record()
            torch.cuda.synchronize()
            times[name].append(a.elapsed_time(b) * 1e3 / reps)
    for name, xs in times.items():
        print(f"wall n={args.n} {name:15s} {statistics.median(xs):10.2f} us per call  [{min(xs):.2f} .. {max(xs):.2f}]", flush=True)


def cmd_program(args):
    torch, variants = setup(args.n)
    for _ in range(50):
        for name in ("fused position", "fused torque", "env step"):
            variants[name]()
    torch.cuda.synchronize()
    print("program done", flush=True)


def child(argv, limit):
    p = subprocess.run(["timeout", "-k", "10", str(limit)] + argv, cwd=REPO, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    if p.returncode != 0:
        sys.stdout.write(p.stdout[-4000:])
        raise SystemExit(f"child {' '.join(argv)} ended with status {p.returncode}: stopping")
    return p.stdout


def cmd_all(args):
    me = [sys.executable, os.path.abspath(__file__)]
    out = []
    say = lambda s="": (out.append(s), print(s, flush=True))   # noqa: E731
    say("# tools/fingertip_action_cost.py all   (MI355X; every figure from a fresh process)")
    for n in [int(x) for x in args.sizes.split(",")]:
        say(f"\n## n = {n}: device events around back-to-back calls (us per call, median of three rounds [min .. max])")
        for l in child(me + ["wall", str(n)], 300).splitlines():
            if l.startswith("wall"):
                say(l)
        prof = os.path.join(args.scratch, f"prof_fingertip_{n}")
        child(["rocprofv3", "--kernel-trace", "--stats", "-d", prof, "-o", "r", "--"] + me + ["program", str(n)], 300)
        db = next((os.path.join(r, f) for r, _, fs in os.walk(prof) for f in fs if f.endswith(".db")), None)
        say(f"\n## n = {n}: kernel times, counter-free rocprofv3 --kernel-trace --stats, a run of its own")
        if db is None:
            say("not measured: the trace left no database")
            continue
        for l in child([sys.executable, os.path.join(REPO, "tools", "rocprof_summary.py"), "trace", db], 120).splitlines():
            if re.search(r"k_tip_action|k_env|calls", l):
                say(l[:200])
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(out) + "\n")


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    sub = ap.add_subparsers(dest="cmd", required=True)
    for name in ("wall", "program"):
        s = sub.add_parser(name)
        s.add_argument("n", type=int)
    a = sub.add_parser("all")
    a.add_argument("--out", default=os.path.join(REPO, "profiles", "fingertip_action_cost.txt"))
    a.add_argument("--sizes", default="8192,65536")
    a.add_argument("--scratch", default=os.environ.get("TMPDIR", "/tmp"))
    ns = ap.parse_args()
    {"wall": cmd_wall, "program": cmd_program, "all": cmd_all}[ns.cmd](ns)
