#!/usr/bin/env python3
"""Developer tool (GPU box): what `mixed_precision` costs or buys in the in-repo PPO (include/trifinger_ppo_mixed.h: the network walk and the direct
weight-gradient kernel with bf16 operands in place of their fp32 forms).  Modelled on tools/diagnostics_cost.py.

    python tools/mixed_precision_cost.py all --parent-tree DIR [--out profiles/r24_mixed_precision.txt] [--rounds 3] [--only launches,trainer]
        every measurement below, each in a FRESH child process under a time limit of its own, parent and tree alternating; the report holds medians and
        spreads.  A mixed launch counts as NOT SLOWER when it is within the run-to-run spread its fp32 form shows at the parent.  --parent-tree: a built
        checkout of the parent commit.
    python tools/mixed_precision_cost.py launches fp32|bf16 [--tree DIR]
        the three launches at the trainer's shapes (M = 8192, 41 / 113 -> 400 -> 200 -> 100 -> 9 / 1): the forward walk of both networks, the backward walk,
        the direct weight-gradient launch of the eight products.  Device events around 200 launches each, behind a long matrix product that lets the host
        run ahead (the window holds device time, not enqueue time); 20 launches of warm-up; the median of 5 windows.
    python tools/mixed_precision_cost.py trainer off|on [--tree DIR]
        frames/s of the trainer (the loop of scripts/train_ppo.py) at 8192 envs over the last 10 of 40 epochs, the time of a whole update() and of a minibatch
        step, key off / on
A child that fails ends the run: nothing more is started on the GPU after it."""
import argparse
import os
import statistics
import subprocess
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
M = 8192
KEYS = ["rlg.params.config.mixed_precision=True"]
DIMS = ([41, 400, 200, 100, 9], [113, 400, 200, 100, 1])
LAUNCHES = ("forward walk", "backward walk", "dW direct")


def _tree(path):
    sys.path.insert(0, os.path.abspath(path) if path else REPO)


def med_spread(xs):
    return statistics.median(xs), min(xs), max(xs)


# ---- the three launches under device events ------------------------------------------------------------------------------------------------------------
def cmd_launches(args):
    _tree(args.tree)
    import torch
    from leibnizgym_amd import ppo_kernels as pk
    dev = "cuda:0"
    g = torch.Generator(device=dev).manual_seed(2)
    r = lambda *s: torch.randn(*s, device=dev, generator=g)               # noqa: E731
    mixed = args.mode == "bf16"
    nets = []
    for d in DIMS:
        layers = pk.LayerList()
        if mixed:
            layers.mixed = True
        for i in range(len(d) - 1):
            layers.append((r(d[i + 1], d[i]) * d[i] ** -0.5, r(d[i + 1]) * 0.1, 1 if i < len(d) - 2 else 0, (r(d[i + 1], d[i]), r(d[i + 1]))))
        nets.append((r(M, d[0]), layers, r(M, d[-1])))
    kw = {"mixed": True} if mixed else {}
    outs = pk.forward_nets([(x, layers) for x, layers, _ in nets])
    dzs = pk.mlp_walk_backward([(gy, ys, layers) for (_, layers, gy), ys in zip(nets, outs)], **kw)
    gys, inps, gouts = [], [], []
    for (x, layers, _), ys, dz in zip(nets, outs, dzs):
        for k in range(len(layers) - 1, -1, -1):
            gys.append(dz[k]); inps.append(ys[k - 1] if k > 0 else x); gouts.append(layers[k][3])

    def dw():
        assert pk.gemm_tn_bias_direct(gys, inps, gouts, **kw)
        pk.discard_partial_sums()                                         # the launch alone: the chunk sums are the same launch in both modes
    work = {"forward walk": lambda: pk.forward_nets([(x, layers) for x, layers, _ in nets]),
            "backward walk": lambda: pk.mlp_walk_backward([(gy, ys, layers) for (_, layers, gy), ys in zip(nets, outs)], **kw), "dW direct": dw}
    big = r(8192, 8192)
    res = {}
    for name, fn in work.items():
        for _ in range(20):
            fn()
        torch.cuda.synchronize()
        wins = []
        for _ in range(5):
            for _ in range(3):
                torch.mm(big, big)                                        # ~30 ms of device work: the host enqueues the window while it runs
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(args.reps):
                fn()
            e1.record()
            torch.cuda.synchronize()
            wins.append(1e3 * e0.elapsed_time(e1) / args.reps)
        res[name] = statistics.median(wins)
    print("launch_us " + args.mode + " " + " ".join(f"{res[k]:.2f}" for k in LAUNCHES), flush=True)


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
        assert tr.net.mixed and tr.fused_loss and tr.torch_path_reason is None
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
    u = statistics.median(upd[-10:])
    print(f"trainer_fps {args.keys} {(f1 - f0) / (t1 - t0):.4e} update_ms {1e3 * u:.3f} mb_step_us {1e6 * u / steps:.1f} loss {stats[-1]['loss']:.5f} "
          f"kl {stats[-1]['kl']:.6f}", flush=True)


# ---- everything, in fresh processes ---------------------------------------------------------------------------------------------------------------------
def child(argv, limit):
    """one measurement in a fresh process under its own time limit; its stdout.  A failure ends the whole run (nothing is started behind a fault)."""
    p = subprocess.run(["timeout", "-k", "10", str(limit)] + argv, cwd=REPO, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    if p.returncode != 0:
        sys.stdout.write(p.stdout[-4000:])
        raise SystemExit(f"child {' '.join(argv)} ended with status {p.returncode}: stopping")
    return p.stdout


def cmd_all(args):
    me = [sys.executable, os.path.abspath(__file__)]
    out = []
    say = lambda s="": (out.append(s), print(s, flush=True))   # noqa: E731
    only = set(args.only.split(","))
    say("# tools/mixed_precision_cost.py all   (MI355X; every figure from a fresh process, medians with [min .. max]; parent and tree alternating)")
    if "launches" in only:
        confs = [("parent fp32", ["fp32", "--tree", args.parent_tree]), ("fp32", ["fp32"]), ("bf16", ["bf16"])]
        us = {name: {k: [] for k in LAUNCHES} for name, _ in confs}
        for _ in range(args.rounds):
            for name, argv in confs:
                line = [l for l in child(me + ["launches"] + argv, 300).splitlines() if l.startswith("launch_us")][-1].split()
                for k, v in zip(LAUNCHES, line[2:]):
                    us[name][k].append(float(v))
        say(f"\n## the three launches at M = {M}, 41 / 113 -> 400 -> 200 -> 100 -> 9 / 1: device events around 200 launches, median of 5 windows per process, "
            f"{args.rounds} processes each; us per launch")
        for name, _ in confs:
            say(f"{name:12s} " + "   ".join("{} {:.2f} [{:.2f} .. {:.2f}]".format(k, *med_spread(us[name][k])) for k in LAUNCHES))
        for k in LAUNCHES:
            pm, plo, phi = med_spread(us["parent fp32"][k])
            x = statistics.median(us["bf16"][k])
            verdict = "NOT SLOWER" if x <= pm + (phi - plo) else "SLOWER"
            say(f"{k}: bf16 {x:.2f} us against the parent's fp32 {pm:.2f} us (its spread {phi - plo:.2f} us): {pm / x:.2f} x, {verdict}")
    if "trainer" in only:
        confs = [("parent", ["off", "--tree", args.parent_tree]), ("key off", ["off"]), ("key on", ["on"])]
        fps, ups, mbs = ({k: [] for k, _ in confs} for _ in range(3))
        for _ in range(args.rounds):
            for name, argv in confs:
                line = [l for l in child(me + ["trainer", "--epochs", str(args.epochs)] + argv, 420).splitlines() if l.startswith("trainer_fps")][-1].split()
                fps[name].append(float(line[2])); ups[name].append(float(line[4])); mbs[name].append(float(line[6]))
        say(f"\n## trainer at {M} envs: frames/s over the last 10 of {args.epochs} epochs, a whole update() and one minibatch step (update / (mini_epochs x "
            f"minibatches)), medians of those epochs; {args.rounds} fresh processes each, alternating")
        for name, _ in confs:
            m, lo, hi = med_spread(fps[name])
            u, ulo, uhi = med_spread(ups[name])
            s, slo, shi = med_spread(mbs[name])
            say(f"{name:9s} {m:.4e} frames/s [{lo:.4e} .. {hi:.4e}]   update {u:.3f} ms [{ulo:.3f} .. {uhi:.3f}]   minibatch step {s:.1f} us [{slo:.1f} .. {shi:.1f}]")
        off, on = statistics.median(fps["key off"]), statistics.median(fps["key on"])
        _, plo, phi = med_spread(fps["parent"])
        say(f"key off frames/s inside the parent's own spread [{plo:.4e} .. {phi:.4e}]: {'yes' if plo <= off <= phi else 'above it' if off > phi else 'NO'}")
        say(f"key on / key off = {on / off:.4f} in frames/s; update {statistics.median(ups['key on']):.3f} ms against {statistics.median(ups['key off']):.3f} ms")
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "a" if args.append else "w") as f:
        f.write("\n".join(out) + "\n")


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    sub = ap.add_subparsers(dest="cmd", required=True)
    k = sub.add_parser("launches"); k.add_argument("mode", choices=["fp32", "bf16"]); k.add_argument("--tree", default=None); k.add_argument("--reps", type=int, default=200)
    t = sub.add_parser("trainer"); t.add_argument("keys", choices=["off", "on"]); t.add_argument("--tree", default=None); t.add_argument("--epochs", type=int, default=40)
    a = sub.add_parser("all")
    a.add_argument("--out", default=os.path.join(REPO, "profiles", "r24_mixed_precision.txt"))
    a.add_argument("--only", default="launches,trainer", help="which parts to run (a run split over several sittings appends: --append)")
    a.add_argument("--append", action="store_true")
    a.add_argument("--epochs", type=int, default=40)
    a.add_argument("--parent-tree", required=True)
    a.add_argument("--rounds", type=int, default=3)
    ns = ap.parse_args()
    {"launches": cmd_launches, "trainer": cmd_trainer, "all": cmd_all}[ns.cmd](ns)
