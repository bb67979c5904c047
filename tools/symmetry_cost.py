#!/usr/bin/env python3
"""Developer tool (GPU box): what `symmetry_augmentation` costs in the in-repo PPO (include/trifinger_ppo_symmetry.h: tfp_gather_rows_sym in place of
tfp_gather_rows_norm, tfp_ppo_loss_sym in place of the objective's entry point, three times the rows through the rest of the minibatch step).  Modelled on
tools/track_cost.py.

    python tools/symmetry_cost.py all [--out profiles/r19_symmetry.txt] [--parent-tree DIR] [--rounds 3] [--only gather,trainer]
        every measurement below, each in a FRESH child process under a time limit of its own, the configurations of a comparison alternating; the
        report holds medians and spreads.  --parent-tree: a built checkout of the parent commit, for the third trainer configuration.
    python tools/symmetry_cost.py gather             the program of a counter-free `rocprofv3 --kernel-trace --stats` run: the augmenting gather at B = 8192 with the
                                                     trainer's eight arrays, and the existing normalising gather on the 3 B tiled indices (the rows the augmenting
                                                     one writes, with a third of the reads), alternating, 200 launches each
    python tools/symmetry_cost.py trainer off|on [--tree DIR]
                                                     frames/s of the trainer at 8192 envs over the last 10 of 40 epochs and the time of a minibatch step, key off / on
A child that fails ends the run: nothing more is started on the GPU after it."""
import argparse
import os
import re
import statistics
import subprocess
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
T, M = 32, 8192
KEYS = ["rlg.params.config.symmetry_augmentation=True"]


def _tree(path):
    sys.path.insert(0, os.path.abspath(path) if path else REPO)


def med_spread(xs):
    return statistics.median(xs), min(xs), max(xs)


# ---- the program of the kernel trace ---------------------------------------------------------------------------------------------------------------
def cmd_gather(args):
    _tree(None)
    import torch
    from leibnizgym_amd import ppo_kernels as pk
    from leibnizgym_amd import symmetry as sy
    dev = "cuda:0"
    g = torch.Generator(device=dev).manual_seed(2)
    rows = T * M
    r = lambda *s: torch.randn(*s, device=dev, generator=g)               # noqa: E731
    # the trainer's eight arrays with every option on: obs, act, old_nlp, (adv, w), ret, old_mu, old_v, states
    srcs = [r(rows, 41), r(rows, 9), r(rows), r(rows, 2), r(rows), r(rows, 9), r(rows), r(rows, 113)]
    stat = lambda w: (r(w) * 0.1, 0.8 + 0.4 * torch.rand(w, device=dev, generator=g), 5.0)      # noqa: E731
    norm = [stat(41)] + [None] * 6 + [stat(113)]
    t = sy.tables_to(sy.trifinger_symmetry(9, True), dev)
    pa = sy.pack(t["action"])
    tables = [sy.pack(t["obs"]), pa, None, None, None, pa, None, sy.pack(t["states"])]
    idx = torch.randperm(rows, device=dev, generator=g)[:M].contiguous()
    idx3 = idx.repeat(3).contiguous()
    outs = [torch.empty((3 * M,) + tuple(s.shape[1:]), device=dev) for s in srcs]
    for _ in range(args.reps):
        pk.gather_rows_sym(srcs, idx, tables, outs=outs, norm=norm)
        pk.gather_rows(srcs, idx3, outs=outs, norm=norm)
    torch.cuda.synchronize()
    print("gather done", flush=True)


# ---- the trainer -------------------------------------------------------------------------------------------------------------------------------------
def cmd_trainer(args):
    _tree(args.tree)
    import torch
    from leibnizgym_amd.config import compose
    from leibnizgym_amd.envs import TrifingerEnv
    from leibnizgym_amd.ppo import PPOConfig, PPOTrainer
    from leibnizgym_amd.utils.rlg_train import RlGamesGpuEnvAdapter
    from leibnizgym_amd.wrappers import VecTaskPython
    cfg = compose(["gym=trifinger_difficulty_4", f"args.num_envs={M}"] + (KEYS if args.keys == "on" else []))
    dev = "cuda:0"
    n = cfg["gym"]["num_instances"]
    env = TrifingerEnv(config=cfg["gym"], device=dev, verbose=False)
    adapter = RlGamesGpuEnvAdapter("rlgpu", n, env=VecTaskPython(env, rl_device=dev))
    pc = PPOConfig.from_rlg(cfg["rlg"], num_envs=n)
    tr = PPOTrainer(adapter, env.get_obs_dim(), env.get_state_dim(), env.get_action_dim(), pc, device=dev)
    if args.keys == "on":
        assert tr.sym is not None and tr.fused_loss
    marks, upd = [], []
    update = tr.update

    def timed_update(buf):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        st = update(buf)
        torch.cuda.synchronize()
        upd.append(time.perf_counter() - t0)
        return st
    tr.update = timed_update

    def log(st):
        torch.cuda.synchronize()
        marks.append((time.perf_counter(), st["frames"]))
    stats = tr.train(args.epochs, log)
    (t0, f0), (t1, f1) = marks[-11], marks[-1]
    steps = pc.mini_epochs * pc.minibatches
    print(f"trainer_fps {args.keys} {(f1 - f0) / (t1 - t0):.4e} mb_step_us {1e6 * statistics.median(upd[-10:]) / steps:.1f} gap {stats[-1].get('symmetry_gap', float('nan')):.4f}",
          flush=True)


# ---- everything, in fresh processes ---------------------------------------------------------------------------------------------------------------------
def child(argv, limit, env=None):
    """one measurement in a fresh process under its own time limit; its stdout.  A failure ends the whole run (nothing is started behind a fault)."""
    p = subprocess.run(["timeout", "-k", "10", str(limit)] + argv, cwd=REPO, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, env=env)
    if p.returncode != 0:
        sys.stdout.write(p.stdout[-4000:])
        raise SystemExit(f"child {' '.join(argv)} ended with status {p.returncode}: stopping")
    return p.stdout


def trace(me, argv, scratch, tag):
    """{kernel name: (calls, avg us)} of a child under rocprofv3 --kernel-trace --stats, and the summary lines"""
    prof = os.path.join(scratch, f"prof_symmetry_{tag}")
    child(["rocprofv3", "--kernel-trace", "--stats", "-d", prof, "-o", "r", "--"] + me + argv, 420)
    db = None
    for root, _, files in os.walk(prof):
        for f in files:
            if f.endswith(".db"):
                db = os.path.join(root, f)
    lines = child([sys.executable, os.path.join(REPO, "tools", "rocprof_summary.py"), "trace", db], 120).splitlines()
    table = {}
    for l in lines[2:]:
        m = re.match(r"^(.*?)\s+(\d+)\s+([\d.]+)\s+([\d.]+)\s+([\d.]+)$", l)
        if not m:
            break
        table[m.group(1).strip()] = (int(m.group(2)), float(m.group(4)))
    return table, lines


def cmd_all(args):
    me = [sys.executable, os.path.abspath(__file__)]
    out = []
    say = lambda s="": (out.append(s), print(s, flush=True))   # noqa: E731
    only = set(args.only.split(","))
    say("# tools/symmetry_cost.py all   (MI355X; every figure from a fresh process, medians with [min .. max])")
    confs = ([("parent", ["off", "--tree", args.parent_tree])] if args.parent_tree else []) + [("key off", ["off"]), ("key on", ["on"])]
    pairs = None
    if "gather" in only:
        table, lines = trace(me, ["gather"], args.scratch, "gather")
        say(f"\n## the gather launch at B = {M}, the trainer's eight arrays (obs and states with statistics), sources of {T * M} rows: counter-free rocprofv3 "
            "--kernel-trace --stats, one run, the two launches alternating")
        for l in lines:
            if any(k in l for k in ("k_gather_rows_sym", "k_gather_rows_norm", "calls", "dispatch footprint")):
                say(l[:200])
        avg = lambda key: next((v[1] for k, v in table.items() if key in k), None)      # noqa: E731
        pairs = (avg("k_gather_rows_sym"), avg("k_gather_rows_norm"))
        if None not in pairs:
            say(f"augmenting gather {pairs[0]:.2f} us (8192 rows read, 3 x 8192 written) against the normalising gather on the 3 x 8192 tiled indices {pairs[1]:.2f} us: "
                f"ratio {pairs[0] / pairs[1]:.3f}")
    if "trainer" in only:
        fps, mbs, gap = {k: [] for k, _ in confs}, {k: [] for k, _ in confs}, []
        for _ in range(args.rounds):
            for name, argv in confs:
                line = [l for l in child(me + ["trainer", "--epochs", str(args.epochs)] + argv, 420).splitlines() if l.startswith("trainer_fps")][-1].split()
                fps[name].append(float(line[2])); mbs[name].append(float(line[4]))
                if name == "key on":
                    gap.append(float(line[6]))
        say(f"\n## trainer frames/s at {M} envs over the last 10 of {args.epochs} epochs, and the time of one minibatch step (update / (mini_epochs x minibatches), "
            f"median of those epochs); {args.rounds} fresh processes each, alternating")
        for name, _ in confs:
            m, lo, hi = med_spread(fps[name])
            say(f"{name:9s} {m:.4e}  [{lo:.4e} .. {hi:.4e}]  spread {100 * (hi - lo) / m:.2f} %   minibatch step {statistics.median(mbs[name]):.1f} us")
        off, on = statistics.median(fps["key off"]), statistics.median(fps["key on"])
        say(f"key on / key off = {on / off:.4f} (no bar: three times the rows through the walk is the expected price); symmetry_gap after {args.epochs} epochs "
            f"{statistics.median(gap):.4f}")
        if args.parent_tree:
            pm, plo, phi = med_spread(fps["parent"])
            inside = plo <= off <= phi
            say(f"key off / parent = {off / pm:.4f}; bar: key off inside the parent's own spread [{plo:.4e} .. {phi:.4e}]: {'MET' if inside else 'NOT MET' if off < plo else 'MET (above it)'}")
            if pairs is not None and None not in pairs:
                spread = (phi - plo) / pm
                say(f"bar: the augmenting gather no slower than the normalising gather on 3 B indices by more than the parent's spread ({100 * spread:.2f} %): "
                    f"{'MET' if pairs[0] <= pairs[1] * (1.0 + spread) else 'NOT MET'}")
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "a" if args.append else "w") as f:
        f.write("\n".join(out) + "\n")


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    sub = ap.add_subparsers(dest="cmd", required=True)
    k = sub.add_parser("gather"); k.add_argument("--reps", type=int, default=200)
    t = sub.add_parser("trainer"); t.add_argument("keys", choices=["off", "on"]); t.add_argument("--tree", default=None); t.add_argument("--epochs", type=int, default=40)
    a = sub.add_parser("all")
    a.add_argument("--out", default=os.path.join(REPO, "profiles", "r19_symmetry.txt"))
    a.add_argument("--only", default="gather,trainer", help="which parts to run (a run split over several sittings appends: --append)")
    a.add_argument("--append", action="store_true")
    a.add_argument("--epochs", type=int, default=40)
    a.add_argument("--parent-tree", default=None)
    a.add_argument("--rounds", type=int, default=3)
    a.add_argument("--scratch", default=os.environ.get("TMPDIR", "/tmp"))
    ns = ap.parse_args()
    {"gather": cmd_gather, "trainer": cmd_trainer, "all": cmd_all}[ns.cmd](ns)
