#!/usr/bin/env python3
"""Developer tool (GPU box): what `track_episodes` costs in the in-repo PPO (include/trifinger_ppo_track.h: tfp_rollout_track, ONE launch where
tfp_rollout_reward / tfp_rollout_flags stand).  Modelled on tools/episode_ends_cost.py.

    python tools/track_cost.py all [--out profiles/r16_track_episodes.txt] [--parent-tree DIR] [--rounds 3] [--only kernels,launches,trainer]
        every measurement below, each in a FRESH child process under a time limit of its own, the configurations of a comparison alternating; the
        report holds medians and spreads.  --parent-tree: a built checkout of the parent commit, for the third trainer configuration.
    python tools/track_cost.py kernels               the program of a counter-free `rocprofv3 --kernel-trace --stats` run at n = 8192: the reward and flags launches,
                                                     the tracking launch in both modes on QUIET steps (nobody ends) and on a burst (everybody ends), and the
                                                     evaluator's k_eval_step on the same quiet step - the bar: tracking minus the launch it replaces must stay
                                                     below the evaluator's quiet step, or fusing bought nothing over calling the evaluator's kernel
    python tools/track_cost.py launches off|on [--tree DIR]
                                                     the program of a kernel trace of the TRAINER (8192 envs, 2 epochs): dispatches per kernel, for the launch counts
    python tools/track_cost.py trainer off|on [--tree DIR]
                                                     frames/s of the trainer at 8192 envs over the last 10 of 40 epochs, key off / on
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
KEYS = ["rlg.params.config.track_episodes=True"]
TRACE_EPOCHS = 2


def _tree(path):
    sys.path.insert(0, os.path.abspath(path) if path else REPO)


def med_spread(xs):
    return statistics.median(xs), min(xs), max(xs)


# ---- the program of the kernel trace ---------------------------------------------------------------------------------------------------------------
def cmd_kernels(args):
    _tree(None)
    import torch
    from types import SimpleNamespace
    from leibnizgym_amd import _capi as capi
    from leibnizgym_amd import ppo_kernels as pk
    from leibnizgym_amd.evaluate import EpisodeStats, EpisodeTracker
    dev = "cuda:0"
    g = torch.Generator(device=dev).manual_seed(2)
    state = torch.randn(capi.TF_STATE_ROWS, M, device=dev, generator=g) * 0.1
    eng = SimpleNamespace(state=state, reward=torch.randn(M, device=dev, generator=g), reset_buf=torch.zeros(M, dtype=torch.bool, device=dev),
                          goal_reset_buf=torch.zeros(M, dtype=torch.bool, device=dev), steps=torch.full((M,), 5, dtype=torch.int64, device=dev))
    done = torch.zeros(M, dtype=torch.bool, device=dev)
    slot = torch.zeros(4, M, device=dev)
    trk = EpisodeTracker(eng, 0.02, 0.25, rule=1, episode_length=750)
    evs = EpisodeStats(eng, 0.02, 0.25, rule=1)
    for rep in range(0 if args.burst else args.reps):
        for _ in range(8):                                    # alternating, all on a quiet step: nobody ends
            pk.rollout_reward(eng.reward, done, 0.01, slot[0], slot[1])
            pk.rollout_flags(eng.reward, eng.reset_buf, eng.steps, 0.01, 750, slot[0], slot[2], slot[3])
            trk.step_fused(0.01, slot[0], done=done, done_t=slot[1])
            trk.step_fused(0.01, slot[0], end_t=slot[2], tout_t=slot[3])
            evs.update()
    torch.cuda.synchronize()
    if args.burst:                                            # a trace of its own: every env ends, in both kernels
        eng.reset_buf.fill_(True)
        eng.steps.fill_(1)
        for rep in range(args.reps):
            trk.step_fused(0.01, slot[0], end_t=slot[2], tout_t=slot[3])
            evs.update()
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
        assert tr.tracker is not None and tr.tracker.fused
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
    prof = os.path.join(scratch, f"prof_track_{tag}")
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
    say("# tools/track_cost.py all   (MI355X; every figure from a fresh process, medians with [min .. max])")
    confs = ([("parent", ["off", "--tree", args.parent_tree])] if args.parent_tree else []) + [("key off", ["off"]), ("key on", ["on"])]
    diff = None
    if "kernels" in only:
        for tag, extra in (("quiet", []), ("burst", ["--burst"])):
            table, lines = trace(me, ["kernels"] + extra, args.scratch, "kernels_" + tag)
            say(f"\n## after-step launches at n = {M}: counter-free rocprofv3 --kernel-trace --stats, a run of its own, the variants alternating"
                + (" on QUIET steps (nobody ends)" if tag == "quiet" else ": a BURST (every env ends in every launch) of k_rollout_track and k_eval_step"))
            for l in lines:
                if any(k in l for k in ("k_rollout_reward", "k_rollout_flags", "k_rollout_track", "k_eval_step", "calls", "dispatch footprint")):
                    say(l[:200])
            if tag == "quiet":
                avg = lambda key: next((v[1] for k, v in table.items() if key in k), None)      # noqa: E731
                trk, rew, flg, evs = avg("k_rollout_track"), avg("k_rollout_reward"), avg("k_rollout_flags"), avg("k_eval_step")
                if None not in (trk, rew, flg, evs):
                    diff = trk - min(rew, flg)
                    say(f"bar: tracking launch {trk:.2f} us (both modes) - the cheaper launch it replaces {min(rew, flg):.2f} us = {diff:.2f} us; it must stay below "
                        f"k_eval_step's quiet step, {evs:.2f} us in this session: {'MET' if diff < evs else 'MISSED'}")
    if "launches" in only:
        tables = {name: trace(me, ["launches"] + argv, args.scratch, name.replace(" ", "_"))[0] for name, argv in confs}
        say(f"\n## dispatches of the trainer at {M} envs, {TRACE_EPOCHS} epochs (horizon {T}), per epoch; kernels whose count differs from `key off`")
        for name, _ in confs:
            say(f"{name:9s} {sum(c for c, _ in tables[name].values()) / TRACE_EPOCHS:10.1f} dispatches per epoch")
        base = tables["key off"]
        for name, _ in confs:
            for k in sorted(set(base) | set(tables[name])) if name != "key off" else []:
                a, b = base.get(k, (0, 0.0)), tables[name].get(k, (0, 0.0))
                if a[0] != b[0]:
                    say(f"  {name:9s} {k[:120]:120s} {a[0] / TRACE_EPOCHS:8.1f} -> {b[0] / TRACE_EPOCHS:8.1f} per epoch   avg {a[1]:.2f} / {b[1]:.2f} us")
    if "trainer" in only:
        fps = {k: [] for k, _ in confs}
        for _ in range(args.rounds):
            for name, argv in confs:
                line = [l for l in child(me + ["trainer", "--epochs", str(args.epochs)] + argv, 420).splitlines() if l.startswith("trainer_fps")][-1].split()
                fps[name].append(float(line[2]))
        say(f"\n## trainer frames/s at {M} envs over the last 10 of {args.epochs} epochs ({args.rounds} fresh processes each, alternating)")
        for name, _ in confs:
            m, lo, hi = med_spread(fps[name])
            say(f"{name:9s} {m:.4e}  [{lo:.4e} .. {hi:.4e}]  spread {100 * (hi - lo) / m:.2f} %")
        off, on = statistics.median(fps["key off"]), statistics.median(fps["key on"])
        say(f"key on / key off = {on / off:.4f}" + (f";  key off / parent = {off / statistics.median(fps['parent']):.4f}" if args.parent_tree else ""))
        if args.parent_tree:
            pm, plo, phi = med_spread(fps["parent"])
            say(f"bar: key off inside the parent's own spread [{plo:.4e} .. {phi:.4e}]"
                + (f"; key on no lower than its low end less {diff:.2f} us x {T} steps per epoch of {T * M} frames: "
                   f"{T * M / (T * M / plo + diff * 1e-6 * T):.4e}" if diff is not None and diff > 0 else "; key on inside it as well (the tracking launch is no dearer)"))
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "a" if args.append else "w") as f:
        f.write("\n".join(out) + "\n")


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    sub = ap.add_subparsers(dest="cmd", required=True)
    k = sub.add_parser("kernels"); k.add_argument("--reps", type=int, default=25); k.add_argument("--burst", action="store_true")
    for name in ("trainer", "launches"):
        t = sub.add_parser(name); t.add_argument("keys", choices=["off", "on"]); t.add_argument("--tree", default=None); t.add_argument("--epochs", type=int, default=40)
    a = sub.add_parser("all")
    a.add_argument("--out", default=os.path.join(REPO, "profiles", "r16_track_episodes.txt"))
    a.add_argument("--only", default="kernels,launches,trainer", help="which parts to run (a run split over several sittings appends: --append)")
    a.add_argument("--append", action="store_true")
    a.add_argument("--epochs", type=int, default=40)
    a.add_argument("--parent-tree", default=None)
    a.add_argument("--rounds", type=int, default=3)
    a.add_argument("--scratch", default=os.environ.get("TMPDIR", "/tmp"))
    ns = ap.parse_args()
    {"kernels": cmd_kernels, "trainer": cmd_trainer, "launches": cmd_launches, "all": cmd_all}[ns.cmd](ns)
