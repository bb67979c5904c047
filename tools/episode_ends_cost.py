#!/usr/bin/env python3
"""Developer tool (GPU box): what `episode_ends` / `value_bootstrap` cost in the in-repo PPO (include/trifinger_ppo_episode.h: tfp_rollout_flags, tfp_gae_ends,
tfp_ppo_loss_w; one more column in the gathered advantage array).  Modelled on tools/value_norm_cost.py.

    python tools/episode_ends_cost.py all [--out profiles/r15_episode_ends.txt] [--parent-tree DIR] [--rounds 3] [--only kernels,launches,minibatch,trainer]
        every measurement below, each in a FRESH child process under a time limit of its own, the configurations of a comparison alternating; the
        report holds medians and spreads.  --parent-tree: a built checkout of the parent commit, for the third trainer configuration.
    python tools/episode_ends_cost.py kernels        the program of a `rocprofv3 --kernel-trace --stats` run: the reward / flags launch (n = 8192), the advantage pass
                                                     (T = 32, n = 8192), the objective (B = 8192) and the minibatch gather, old and new variants side by side
    python tools/episode_ends_cost.py launches off|on [--tree DIR]
                                                     the program of a kernel trace of the TRAINER (8192 envs, 2 epochs): dispatches per kernel, for the launch counts
    python tools/episode_ends_cost.py minibatch off|on [--tree DIR]
                                                     one minibatch step (gather ... Adam) of the trainer at 8192 envs between HIP events, us
    python tools/episode_ends_cost.py trainer off|on [--tree DIR]
                                                     frames/s of the trainer at 8192 envs over the last 10 of 40 epochs, keys off / both keys on
A child that fails ends the run: nothing more is started on the GPU after it."""
import argparse
import os
import re
import statistics
import subprocess
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
T, M, DO, DS = 32, 8192, 41, 113
KEYS = ["rlg.params.config.episode_ends=True", "rlg.params.config.value_bootstrap=True"]
TRACE_EPOCHS = 2


def _tree(path):
    sys.path.insert(0, os.path.abspath(path) if path else REPO)


def med_spread(xs):
    return statistics.median(xs), min(xs), max(xs)


# ---- the program of the kernel trace ---------------------------------------------------------------------------------------------------------------
def cmd_kernels(args):
    _tree(None)
    import torch
    from leibnizgym_amd import ppo_kernels as pk
    from leibnizgym_amd.ppo import neglogp
    dev = "cuda:0"
    g = torch.Generator(device=dev).manual_seed(2)
    r = lambda *s: torch.randn(*s, device=dev, generator=g)               # noqa: E731
    rew, done, y = r(T, M) * 0.01, (r(T, M) > 2).float(), r(T + 1, M)
    end = (r(T, M) > 2).float()
    tout, last_end = end * (r(T, M) > 0).float(), (r(M) > 2).float()
    raw_r, reset, steps = r(M), (r(M) > 2), torch.randint(0, 1500, (M,), device=dev, generator=g)
    slot = torch.zeros(4, M, device=dev)
    mu, ls = r(M, 9) * 0.8, r(9) * 0.3 - 0.5
    act, old_mu, adv, v = mu + r(M, 9) * 0.6, mu + r(M, 9) * 0.05, r(M), r(M)
    ret = v + r(M) * 0.3
    old_nlp = neglogp(act, old_mu, ls.expand_as(old_mu)) + r(M) * 0.05
    adv_w = torch.stack([adv, (r(M) > -3).float()], 1).contiguous()
    stats = torch.zeros(4, device=dev)
    srcs = [r(T * M, w) for w in (DO, 9)] + [r(T * M) for _ in range(3)] + [r(T * M, 9), r(T * M, DS)]     # obs, act, old_nlp, adv, ret, old_mu, states
    wide = srcs[:3] + [r(T * M, 2)] + srcs[4:]                                                              # ... with (adv, w) in place of adv
    for rep in range(args.reps):
        idx = torch.randperm(T * M, device=dev)[:M]
        for _ in range(8):                                    # alternating: the parent's kernel, the episode-end variant
            pk.rollout_reward(raw_r, reset, 0.01, slot[0], slot[1])
            pk.rollout_flags(raw_r, reset, steps, 0.01, 750, slot[0], slot[2], slot[3])
            pk.gae(rew, done, y, 0.99, 0.95)
            pk.gae_ends(rew, end, tout, y, last_end, 0.99, 0.95, True)
            pk.ppo_loss_and_grads(mu, ls, v, act, old_nlp, adv, ret, old_mu, stats, 0.2, 1.0, 0.0, 1e-4)
            pk.ppo_loss_and_grads(mu, ls, v, act, old_nlp, None, ret, old_mu, stats, 0.2, 1.0, 0.0, 1e-4, adv_w=adv_w)
            pk.gather_rows(srcs, idx)
            pk.gather_rows(wide, idx)
    torch.cuda.synchronize()
    print("kernels done", flush=True)


# ---- the trainer -------------------------------------------------------------------------------------------------------------------------------------
def make_trainer(args):
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
        assert tr.ends and tr.cfg.value_bootstrap and tr.ends_ep_len > 0
    return torch, tr


def cmd_trainer(args):
    torch, tr = make_trainer(args)
    marks = []

    def log(st):
        torch.cuda.synchronize()
        marks.append((time.perf_counter(), st["frames"]))
    tr.train(args.epochs, log)
    (t0, f0), (t1, f1) = marks[-11], marks[-1]
    print(f"trainer_fps {args.keys} {(f1 - f0) / (t1 - t0):.4e}", flush=True)


def cmd_launches(args):
    torch, tr = make_trainer(args)
    tr.train(TRACE_EPOCHS)
    torch.cuda.synchronize()
    print("launches done", flush=True)


def cmd_minibatch(args):
    """the minibatch step as update() runs it, on the buffers of one rollout; the optimiser steps are real (the weights move), as in an epoch"""
    torch, tr = make_trainer(args)
    tr.train(2)                                               # code objects, allocator, a record that is not the initial one
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
    print(f"minibatch_us {args.keys} {statistics.median(steps):.1f} {steps[0]:.1f} {steps[-1]:.1f} {len(steps)}", flush=True)


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
    prof = os.path.join(scratch, f"prof_episode_ends_{tag}")
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
    say("# tools/episode_ends_cost.py all   (MI355X; every figure from a fresh process, medians with [min .. max])")
    confs = ([("parent", ["off", "--tree", args.parent_tree])] if args.parent_tree else []) + [("keys off", ["off"]), ("keys on", ["on"])]
    if "kernels" in only:
        # 1. the kernels side by side
        _, lines = trace(me, ["kernels"], args.scratch, "kernels")
        say(f"\n## reward / flags launch (n = {M}), advantage pass (T = {T}, n = {M}), objective (B = {M}) and minibatch gather (7 arrays out of {T} x {M} rows, adv [1] / (adv, w) [2])")
        say("## without and with episode ends: rocprofv3 --kernel-trace --stats, a run of its own, the variants alternating")
        for l in lines:
            if any(k in l for k in ("k_rollout_reward", "k_rollout_flags", "k_gae", "k_ppo_loss", "k_gather_rows", "calls", "dispatch footprint")):
                say(l[:200])
    if "launches" in only:
        cmd_all_launches(args, me, confs, say)
    if "minibatch" in only or "trainer" in only:
        cmd_all_rates(args, me, confs, say, only)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "a" if args.append else "w") as f:
        f.write("\n".join(out) + "\n")


def cmd_all_launches(args, me, confs, say):
    # 2. launch counts of the trainer
    tables = {name: trace(me, ["launches"] + argv, args.scratch, name.replace(" ", "_"))[0] for name, argv in confs}
    say(f"\n## dispatches of the trainer at {M} envs, {TRACE_EPOCHS} epochs (horizon {T}, 4 mini-epochs x 32 minibatches), per epoch; kernels whose count differs from `keys off`")
    for name, _ in confs:
        say(f"{name:9s} {sum(c for c, _ in tables[name].values()) / TRACE_EPOCHS:10.1f} dispatches per epoch")
    base = tables["keys off"]
    for name, _ in confs:
        if name == "keys off":
            continue
        for k in sorted(set(base) | set(tables[name])):
            a, b = base.get(k, (0, 0.0)), tables[name].get(k, (0, 0.0))
            if a[0] != b[0]:
                say(f"  {name:9s} {k[:120]:120s} {a[0] / TRACE_EPOCHS:8.1f} -> {b[0] / TRACE_EPOCHS:8.1f} per epoch   avg {a[1]:.2f} / {b[1]:.2f} us")


def cmd_all_rates(args, me, confs, say, only):
    # 3. one minibatch step, 4. frames/s: alternating fresh processes
    mbs, fps = {k: [] for k, _ in confs}, {k: [] for k, _ in confs}
    for _ in range(args.rounds if "minibatch" in only else 0):
        for name, argv in confs:
            line = [l for l in child(me + ["minibatch"] + argv, 420).splitlines() if l.startswith("minibatch_us")][-1].split()
            mbs[name].append(float(line[2]))
    for _ in range(args.rounds if "trainer" in only else 0):
        for name, argv in confs:
            line = [l for l in child(me + ["trainer", "--epochs", str(args.epochs)] + argv, 420).splitlines() if l.startswith("trainer_fps")][-1].split()
            fps[name].append(float(line[2]))
    if "minibatch" in only:
        cmd_all_report_mb(args, confs, say, mbs)
    if "trainer" in only:
        cmd_all_report_fps(args, confs, say, fps)


def cmd_all_report_mb(args, confs, say, mbs):
    say(f"\n## one minibatch step (gather .. Adam, HIP events around it, median of the 128 steps of an epoch) at {M} envs, us ({args.rounds} fresh processes each, alternating)")
    for name, _ in confs:
        m, lo, hi = med_spread(mbs[name])
        say(f"{name:9s} {m:8.1f}  [{lo:.1f} .. {hi:.1f}]  spread {100 * (hi - lo) / m:.2f} %")
    if args.parent_tree:
        pm, plo, phi = med_spread(mbs["parent"])
        say(f"bar: the parent's own spread [{plo:.1f} .. {phi:.1f}] for keys off; that plus 2 % of the step ({0.02 * pm:.1f} us: up to {phi + 0.02 * pm:.1f}) for keys on")


def cmd_all_report_fps(args, confs, say, fps):
    say(f"\n## trainer frames/s at {M} envs over the last 10 of {args.epochs} epochs ({args.rounds} fresh processes each, alternating)")
    for name, _ in confs:
        m, lo, hi = med_spread(fps[name])
        say(f"{name:9s} {m:.4e}  [{lo:.4e} .. {hi:.4e}]  spread {100 * (hi - lo) / m:.2f} %")
    off, on = statistics.median(fps["keys off"]), statistics.median(fps["keys on"])
    say(f"keys on / keys off = {on / off:.4f}" + (f";  keys off / parent = {off / statistics.median(fps['parent']):.4f}" if args.parent_tree else ""))


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    sub = ap.add_subparsers(dest="cmd", required=True)
    k = sub.add_parser("kernels"); k.add_argument("--reps", type=int, default=25)
    for name in ("trainer", "launches", "minibatch"):
        t = sub.add_parser(name); t.add_argument("keys", choices=["off", "on"]); t.add_argument("--tree", default=None); t.add_argument("--epochs", type=int, default=40)
    a = sub.add_parser("all")
    a.add_argument("--out", default=os.path.join(REPO, "profiles", "r15_episode_ends.txt"))
    a.add_argument("--only", default="kernels,launches,minibatch,trainer", help="which parts to run (a run split over several sittings appends: --append)")
    a.add_argument("--append", action="store_true")
    a.add_argument("--epochs", type=int, default=40)
    a.add_argument("--parent-tree", default=None)
    a.add_argument("--rounds", type=int, default=3)
    a.add_argument("--scratch", default=os.environ.get("TMPDIR", "/tmp"))
    ns = ap.parse_args()
    {"kernels": cmd_kernels, "trainer": cmd_trainer, "launches": cmd_launches, "minibatch": cmd_minibatch, "all": cmd_all}[ns.cmd](ns)
