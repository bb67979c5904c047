#!/usr/bin/env python3
"""Developer tool (GPU box): what the network-shape keys of the agent tree (`network.mlp.activation`, `network.mlp.d2rl`; include/trifinger_ppo_net.h) cost in
the in-repo PPO, and whether the default (ELU, no d2rl) still costs what the parent commit's did.

    python tools/net_shape_cost.py all [--out profiles/r13_net_shape.txt] [--parent-tree DIR] [--rounds 3] [--confs elu,tanh,...] [--no-trainer]
        every measurement below, each in a FRESH child process under a time limit of its own, the configurations alternating; medians and spreads.
        --parent-tree: a built checkout of the parent commit (measured as `parent`, alternating with this tree's `elu`).
    python tools/net_shape_cost.py walk CONF [--tree DIR]       forward and backward network walk of both networks (M = 8192, 41 / 113 -> 400 -> 200 -> 100
                                                                 -> 9 / 1) between HIP events, us: median of 200 launches after 20
    python tools/net_shape_cost.py minibatch CONF [--tree DIR]  one minibatch step (gather ... Adam) of the trainer at 8192 envs between HIP events, us
    python tools/net_shape_cost.py trainer CONF [--tree DIR]    frames/s of the trainer at 8192 envs over the last 10 of --epochs epochs
CONF: elu (the default tree), relu, tanh, sigmoid, selu, softplus, None (that activation on both networks), d2rl (ELU, d2rl on both networks).
A child that fails ends the run: nothing more is started on the GPU after it."""
import argparse
import os
import statistics
import subprocess
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
M, DO, DS, UNITS, A = 8192, 41, 113, [400, 200, 100], 9
CONFS = ["elu", "relu", "tanh", "sigmoid", "selu", "softplus", "None", "d2rl"]
ACT_CODE = {"None": 0, "elu": 1, "relu": 2, "tanh": 3, "sigmoid": 4, "selu": 5, "softplus": 6}


def _tree(path):
    sys.path.insert(0, os.path.abspath(path) if path else REPO)


def conf_keys(conf):
    """the overrides of the launcher's tree for a configuration"""
    if conf == "elu":
        return []
    mlps = ("rlg.params.network.mlp", "rlg.params.config.central_value_config.network.mlp")
    return [f"{m}.d2rl=True" for m in mlps] if conf == "d2rl" else [f"{m}.activation={conf}" for m in mlps]


def cmd_walk(args):
    _tree(args.tree)
    import torch
    from leibnizgym_amd import ppo_kernels as pk
    dev, d2rl = "cuda:0", args.conf == "d2rl"
    code = ACT_CODE["elu" if d2rl else args.conf]
    g = torch.Generator(device=dev).manual_seed(1)
    r = lambda *s: torch.randn(*s, device=dev, generator=g)               # noqa: E731

    def net(dims):
        layers = pk.LayerList() if hasattr(pk, "LayerList") else []       # the parent tree has plain lists (and ELU only)
        if d2rl:
            layers.d2rl = True
        n = len(dims) - 1
        for i in range(n):
            k = dims[i] + (dims[0] if (d2rl and 1 <= i <= n - 2) else 0)
            layers.append((r(dims[i + 1], k) * k ** -0.5, r(dims[i + 1]) * 0.1, code if i < n - 1 else 0, None))
        return layers
    la, lc = net([DO] + UNITS + [A]), net([DS] + UNITS + [1])
    xa, xc, ga, gc = r(M, DO), r(M, DS), r(M, A), r(M, 1)
    outs = pk.mlp_walk_forward([(xa, la), (xc, lc)])
    assert outs is not None
    res = {}
    for name, fn in (("forward", lambda: pk.mlp_walk_forward([(xa, la), (xc, lc)])), ("backward", lambda: pk.mlp_walk_backward([(ga, outs[0], la), (gc, outs[1], lc)]))):
        for _ in range(20):
            fn()
        ev = []
        for _ in range(200):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(); fn(); e1.record()
            ev.append((e0, e1))
        torch.cuda.synchronize()
        res[name] = statistics.median(a.elapsed_time(b) * 1e3 for a, b in ev)
    print(f"walk_us {args.conf} {res['forward']:.1f} {res['backward']:.1f}", flush=True)


def make_trainer(args):
    _tree(args.tree)
    import torch
    from leibnizgym_amd.config import compose
    from leibnizgym_amd.envs import TrifingerEnv
    from leibnizgym_amd.ppo import PPOConfig, PPOTrainer
    from leibnizgym_amd.utils.rlg_train import RlGamesGpuEnvAdapter
    from leibnizgym_amd.wrappers import VecTaskPython
    cfg = compose(["gym=trifinger_difficulty_4", f"args.num_envs={M}"] + conf_keys(args.conf))
    dev = "cuda:0"
    n = cfg["gym"]["num_instances"]
    env = TrifingerEnv(config=cfg["gym"], device=dev, verbose=False)
    adapter = RlGamesGpuEnvAdapter("rlgpu", n, env=VecTaskPython(env, rl_device=dev))
    pc = PPOConfig.from_rlg(cfg["rlg"], num_envs=n)
    tr = PPOTrainer(adapter, env.get_obs_dim(), env.get_state_dim(), env.get_action_dim(), pc, device=dev)
    assert tr.fused_loss, "the configuration does not run on the hand-written kernels"
    return torch, tr


def cmd_trainer(args):
    torch, tr = make_trainer(args)
    marks = []

    def log(st):
        torch.cuda.synchronize()
        marks.append((time.perf_counter(), st["frames"]))
    tr.train(args.epochs, log)
    (t0, f0), (t1, f1) = marks[-11], marks[-1]
    print(f"trainer_fps {args.conf} {(f1 - f0) / (t1 - t0):.4e}", flush=True)


def cmd_minibatch(args):
    """the minibatch step as update() runs it, on the buffers of one rollout; the optimiser steps are real (the weights move), as in an epoch"""
    torch, tr = make_trainer(args)
    tr.train(2)
    buf = tr.rollout()
    inner_b, inner_a = tr._mb_backward, tr._mb_apply
    ev = []

    def backward(d, idx, acc):
        e0 = torch.cuda.Event(enable_timing=True); e0.record()
        ev.append([e0])
        return inner_b(d, idx, acc)

    def apply(gathered=False):
        out = inner_a(gathered)
        e1 = torch.cuda.Event(enable_timing=True); e1.record()
        ev[-1].append(e1)
        return out
    tr._mb_backward, tr._mb_apply = backward, apply
    tr.update(buf)
    torch.cuda.synchronize()
    steps = sorted(a.elapsed_time(b) * 1e3 for a, b in ev)
    print(f"minibatch_us {args.conf} {statistics.median(steps):.1f} {steps[0]:.1f} {steps[-1]:.1f} {len(steps)}", flush=True)


def child(argv, limit):
    """one measurement in a fresh process under its own time limit; its stdout.  A failure ends the whole run (nothing is started behind a fault)."""
    p = subprocess.run(["timeout", "-k", "10", str(limit)] + argv, cwd=REPO, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    if p.returncode != 0:
        sys.stdout.write(p.stdout[-4000:])
        raise SystemExit(f"child {' '.join(argv)} ended with status {p.returncode}: stopping")
    print(".", end="", flush=True, file=sys.stderr)            # a sign of life per child
    return p.stdout


def cmd_all(args):
    me = [sys.executable, os.path.abspath(__file__)]
    out = []
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)

    def say(s=""):
        out.append(s)
        print(s, flush=True)
        with open(args.out, "w") as f:                         # the report so far survives a run that is cut short
            f.write("\n".join(out) + "\n")
    confs = ([("parent", ["elu", "--tree", args.parent_tree])] if args.parent_tree else []) + [(c, [c]) for c in args.confs.split(",")]
    fmt = lambda xs: f"{statistics.median(xs):10.1f}  [{min(xs):.1f} .. {max(xs):.1f}]  spread {100 * (max(xs) - min(xs)) / statistics.median(xs):.2f} %"   # noqa: E731
    say(f"# tools/net_shape_cost.py all   (MI355X; every figure from a fresh process, {args.rounds} each, the configurations alternating; medians with [min .. max])")
    say("# parent = the parent commit's tree, default configuration; elu = this tree, default configuration; the others: that key on BOTH networks")
    fw, bw = {k: [] for k, _ in confs}, {k: [] for k, _ in confs}
    for _ in range(args.rounds):
        for name, argv in confs:
            line = [l for l in child(me + ["walk"] + argv, 180).splitlines() if l.startswith("walk_us")][-1].split()
            fw[name].append(float(line[2])); bw[name].append(float(line[3]))
    say(f"\n## network walk of both networks, M = {M}, {DO} / {DS} -> 400 -> 200 -> 100 -> {A} / 1: one launch, HIP events around the call, median of 200, us")
    for name, _ in confs:
        say(f"{name:9s} forward  {fmt(fw[name])}")
    for name, _ in confs:
        say(f"{name:9s} backward {fmt(bw[name])}")
    mbs = {k: [] for k, _ in confs}
    for _ in range(args.rounds):
        for name, argv in confs:
            line = [l for l in child(me + ["minibatch"] + argv, 300).splitlines() if l.startswith("minibatch_us")][-1].split()
            mbs[name].append(float(line[2]))
    say(f"\n## one minibatch step (gather .. Adam, HIP events around it, median of the 128 steps of an epoch) at {M} envs, us")
    for name, _ in confs:
        say(f"{name:9s} {fmt(mbs[name])}")
    if not args.no_trainer:
        fps = {k: [] for k, _ in confs}
        for _ in range(args.rounds):
            for name, argv in confs:
                line = [l for l in child(me + ["trainer"] + argv + ["--epochs", str(args.epochs)], 420).splitlines() if l.startswith("trainer_fps")][-1].split()
                fps[name].append(float(line[2]))
        say(f"\n## trainer frames/s at {M} envs over the last 10 of {args.epochs} epochs")
        for name, _ in confs:
            xs = fps[name]
            say(f"{name:9s} {statistics.median(xs):.4e}  [{min(xs):.4e} .. {max(xs):.4e}]  spread {100 * (max(xs) - min(xs)) / statistics.median(xs):.2f} %")


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    sub = ap.add_subparsers(dest="cmd", required=True)
    for name in ("walk", "trainer", "minibatch"):
        t = sub.add_parser(name); t.add_argument("conf", choices=CONFS); t.add_argument("--tree", default=None); t.add_argument("--epochs", type=int, default=40)
    a = sub.add_parser("all")
    a.add_argument("--out", default=os.path.join(REPO, "profiles", "r13_net_shape.txt"))
    a.add_argument("--parent-tree", default=None)
    a.add_argument("--rounds", type=int, default=3)
    a.add_argument("--epochs", type=int, default=40)
    a.add_argument("--confs", default=",".join(CONFS))
    a.add_argument("--no-trainer", action="store_true")
    ns = ap.parse_args()
    {"walk": cmd_walk, "trainer": cmd_trainer, "minibatch": cmd_minibatch, "all": cmd_all}[ns.cmd](ns)
