#!/usr/bin/env python3
"""Developer tool (GPU box): what planning costs (include/trifinger_plan.h) - the fork launch beside the torch statement of the same copy (eleven gathers
and scatters: what a user had before the library), the sampling and update launches beside the env step, and a whole plan() beside H env steps.

    python tools/mppi_cost.py all [--out profiles/r26_mppi_cost.txt] [--sizes 8192,65536]
        every measurement below in three FRESH child processes, each under a time limit of its own; a child that fails ends the run
    python tools/mppi_cost.py wall N       device events around REPS back-to-back calls, after a warm-up of the same calls: tfpl_fork and the statement at
                                           N destination envs (S = 256 copies per source), tfpl_rollout_actions, tfpl_update, the env step at N envs
    python tools/mppi_cost.py plan         wall time of MPPIPlanner.plan() at E = 32, S = 256, H = 16 against H x the engine's own step at 8192 envs
    python tools/mppi_cost.py program N    the program of a counter-free `rocprofv3 --kernel-trace --stats` run: the three launches and the env step
The bar: the fork launch costs less than the statement."""
import argparse
import os
import re
import statistics
import subprocess
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
REPS, S, H = 200, 256, 16


def setup(n):
    import ctypes as C
    import torch
    from leibnizgym_amd import _capi as capi
    from leibnizgym_amd import planning as pl
    from leibnizgym_amd.engine import TrifingerEngine, make_config
    dev = "cuda:0"
    hip = capi.load_hip_library()
    src = TrifingerEngine(make_config(hip, n // S, seed=1, command_mode="torque", episode_length=0), device=dev, lib=hip)
    dst = TrifingerEngine(make_config(hip, n, seed=2, command_mode="torque", episode_length=0, env_id_offset=1 << 24), device=dev, lib=hip)
    for e in (src, dst):
        e.reset()
        for _ in range(10):
            e.step_random()
    idx = (torch.arange(n, device=dev) // S).to(torch.int32)
    lib = pl.load()
    c, _ = pl.plan_params(n // S, S, H, 9, sigma=0.5, lam=0.3, seed=3)
    U = torch.zeros(n // S, H, 9, device=dev)
    disc = torch.ones(H, device=dev)
    G, alive, action = torch.zeros(n, device=dev), torch.zeros(n, dtype=torch.uint8, device=dev), torch.zeros(n, 9, device=dev)
    first, w, stats = torch.zeros(n // S, 9, device=dev), torch.zeros(n, device=dev), torch.zeros(n // S, pl.NUM_STATS, device=dev)
    invalid = torch.zeros(n // S, dtype=torch.int32, device=dev)
    st = lambda: C.c_void_p(torch.cuda.current_stream().cuda_stream)                      # noqa: E731
    variants = {
        "fused fork": lambda: pl.fork_envs(dst, src, idx, validate=False),
        "torch fork": lambda: pl.fork_envs(dst, src, idx, fused=False, validate=False),
        "rollout_actions": lambda: lib.tfpl_rollout_actions(C.byref(c), 1, U.data_ptr(), disc.data_ptr(), dst.reward.data_ptr(), dst.reset_buf.data_ptr(),
                                                            G.data_ptr(), alive.data_ptr(), action.data_ptr(), st()),
        "update": lambda: lib.tfpl_update(C.byref(c), G.data_ptr(), U.data_ptr(), first.data_ptr(), w.data_ptr(), stats.data_ptr(), invalid.data_ptr(), st()),
        "env step": dst.step_random,
    }
    return torch, variants


def timed(torch, fn, reps):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(reps):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) * 1e3 / reps


def cmd_wall(args):
    torch, variants = setup(args.n)
    for fn in variants.values():
        for _ in range(20):
            fn()
    torch.cuda.synchronize()
    times = {k: [] for k in variants}
    for _ in range(3):
        for name, fn in variants.items():
            times[name].append(timed(torch, fn, 20 if name == "torch fork" else REPS))
    for name, xs in times.items():
        print(f"wall n={args.n} {name:16s} {statistics.median(xs):10.2f} us per call  [{min(xs):.2f} .. {max(xs):.2f}]", flush=True)


def cmd_plan(args):
    import torch
    from leibnizgym_amd import _capi as capi
    from leibnizgym_amd import planning as pl
    from leibnizgym_amd.engine import TrifingerEngine, make_config
    hip = capi.load_hip_library()
    plant = TrifingerEngine(make_config(hip, 32, seed=1, command_mode="torque", episode_length=0), device="cuda:0", lib=hip)
    plant.reset()
    planner = pl.MPPIPlanner(plant, samples=S, horizon=H, sigma=0.5, lam=0.3)
    for _ in range(5):
        planner.plan()
    for _ in range(50):
        planner.rollout.step_random()
    torch.cuda.synchronize()
    plans = [timed(torch, planner.plan, 50) for _ in range(3)]
    steps = [timed(torch, planner.rollout.step_random, 400) for _ in range(3)]
    p, s = statistics.median(plans), statistics.median(steps)
    print(f"plan E=32 S={S} H={H}: plan() {p:.1f} us [{min(plans):.1f} .. {max(plans):.1f}]; env step at 8192 envs {s:.2f} us [{min(steps):.2f} .. {max(steps):.2f}]; "
          f"plan / (H x step) = {p / (H * s):.3f}", flush=True)


def cmd_program(args):
    torch, variants = setup(args.n)
    for _ in range(50):
        for name in ("fused fork", "rollout_actions", "update", "env step"):
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
    say("# tools/mppi_cost.py all   (MI355X; every figure from a fresh process, three processes per measurement)")
    for n in [int(x) for x in args.sizes.split(",")]:
        say(f"\n## n = {n} destination envs, S = {S}: device events around back-to-back calls (us per call, median of three rounds [min .. max]), three processes")
        for _ in range(3):
            for l in child(me + ["wall", str(n)], 300).splitlines():
                if l.startswith("wall"):
                    say(l)
            say()
        prof = os.path.join(args.scratch, f"prof_mppi_{n}")
        child(["rocprofv3", "--kernel-trace", "--stats", "-d", prof, "-o", "r", "--"] + me + ["program", str(n)], 300)
        db = next((os.path.join(r, f) for r, _, fs in os.walk(prof) for f in fs if f.endswith(".db")), None)
        say(f"## n = {n}: kernel times, counter-free rocprofv3 --kernel-trace --stats, a run of its own")
        if db is None:
            say("not measured: the trace left no database")
            continue
        for l in child([sys.executable, os.path.join(REPO, "tools", "rocprof_summary.py"), "trace", db], 120).splitlines():
            if re.search(r"k_fork|k_rollout_actions|k_update|k_env|calls", l):
                say(l[:200])
    say(f"\n## plan() at E = 32, S = {S}, H = {H} against H x the env step at 8192 envs, three processes")
    for _ in range(3):
        for l in child(me + ["plan"], 300).splitlines():
            if l.startswith("plan"):
                say(l)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(out) + "\n")


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    sub = ap.add_subparsers(dest="cmd", required=True)
    for name in ("wall", "program"):
        s = sub.add_parser(name)
        s.add_argument("n", type=int)
    sub.add_parser("plan")
    a = sub.add_parser("all")
    a.add_argument("--out", default=os.path.join(REPO, "profiles", "r26_mppi_cost.txt"))
    a.add_argument("--sizes", default="8192,65536")
    a.add_argument("--scratch", default=os.environ.get("TMPDIR", "/tmp"))
    ns = ap.parse_args()
    {"wall": cmd_wall, "plan": cmd_plan, "program": cmd_program, "all": cmd_all}[ns.cmd](ns)
