#!/usr/bin/env python3
"""Developer tool (GPU box): what checkpoint evaluation costs (leibnizgym_amd/evaluate.py, csrc/tf_eval.hip, PPOTrainer.evaluate).

    python tools/evaluate_cost.py all [--out profiles/r14_evaluate.txt] [--parent-tree DIR] [--rounds 3] [--envs 8192 65536]
        every measurement below, each in a FRESH child process under a time limit of its own, the two sides of a comparison alternating; the report
        holds medians and spreads.  --parent-tree: a built checkout of the parent commit whose play() loop is timed (without it: this tree's play(),
        which this feature leaves as it was).
    python tools/evaluate_cost.py loop evaluate|play N [--tree DIR]
        env-steps/s at N envs, episode_length 200, the default network: evaluate(episodes_per_env=2), deterministic, = 400 steps with the statistics,
        one walk launch per step and one host read per 32 steps; or play(400), the per-layer forward and one host read per step
    python tools/evaluate_cost.py steps quiet|burst N
        the program of a `rocprofv3 --kernel-trace --stats` run: 200 env steps with the statistics kernel behind each.  quiet: no episode ever ends
        (every workgroup leaves after the per-env update); burst: episode_length 1, EVERY env ends in EVERY launch (every workgroup reduces and
        issues its atomics).  The trace shows k_eval_step beside the step kernel.
A child that fails ends the run: nothing more is started on the GPU after it."""
import argparse
import os
import statistics
import subprocess
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EP_LEN, K = 200, 2


def _tree(path):
    sys.path.insert(0, os.path.abspath(path) if path else REPO)


def _trainer(n, episode_length):
    import torch  # noqa: F401
    from leibnizgym_amd.config import compose
    from leibnizgym_amd.envs import TrifingerEnv
    from leibnizgym_amd.ppo import PPOConfig, PPOTrainer
    from leibnizgym_amd.utils.rlg_train import RlGamesGpuEnvAdapter
    from leibnizgym_amd.wrappers import VecTaskPython
    cfg = compose(["gym=trifinger_difficulty_4", f"args.num_envs={n}", f"gym.episode_length={episode_length}"])
    dev = "cuda:0"
    env = TrifingerEnv(config=cfg["gym"], device=dev, verbose=False)
    adapter = RlGamesGpuEnvAdapter("rlgpu", n, env=VecTaskPython(env, rl_device=dev))
    return PPOTrainer(adapter, env.get_obs_dim(), env.get_state_dim(), env.get_action_dim(), PPOConfig.from_rlg(cfg["rlg"], num_envs=n), device=dev), env


def cmd_loop(args):
    _tree(args.tree)
    import torch
    tr, _ = _trainer(args.n, EP_LEN)
    steps = K * EP_LEN
    run = (lambda s: tr.evaluate(episodes_per_env=K, max_steps=s)["steps"]) if args.what == "evaluate" else (lambda s: (tr.play(s), s)[1])
    run(64)                                                   # warm-up: code objects, the allocator's blocks
    torch.cuda.synchronize()
    rates = []
    for _ in range(3):
        t0 = time.perf_counter()
        done = run(steps)
        torch.cuda.synchronize()
        rates.append(args.n * done / (time.perf_counter() - t0))
    print(f"loop_rate {args.what} {args.n} {statistics.median(rates):.4e} {min(rates):.4e} {max(rates):.4e}", flush=True)


def cmd_steps(args):
    _tree(None)
    import torch
    from leibnizgym_amd.evaluate import EpisodeStats, engine_of
    tr, env = _trainer(args.n, 1 if args.what == "burst" else 0)
    stats = EpisodeStats(engine_of(env))
    with torch.no_grad():
        obs = tr.env.reset()["obs"]
        for _ in range(200):
            obs = tr.env.step(tr.net.mean_action(obs))[0]["obs"]
            stats.update()
    r = stats.result()
    assert r["episodes"] + r["nonfinite_episodes"] == (200 * args.n if args.what == "burst" else 0), r["episodes"]
    print(f"steps done {args.what} {args.n} episodes {r['episodes']}", flush=True)


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
    say("# tools/evaluate_cost.py all   (MI355X; every figure from a fresh process, medians with [min .. max])")
    say(f"\n## env-steps/s of the loop: evaluate(episodes_per_env={K}), episode_length {EP_LEN}, deterministic, against play({K * EP_LEN}) "
        f"({'timed in a built checkout of the parent commit' if args.parent_tree else 'timed in this tree: play() is the code of the parent commit'}); "
        f"{args.rounds} fresh processes each, alternating")
    for n in args.envs:
        rate = {"evaluate": [], "play": []}
        for _ in range(args.rounds):
            for what in ("play", "evaluate"):
                argv = me + ["loop", what, str(n)] + (["--tree", args.parent_tree] if (what == "play" and args.parent_tree) else [])
                line = [l for l in child(argv, 420).splitlines() if l.startswith("loop_rate")][-1].split()
                rate[what].append(float(line[3]))
        for what in ("play", "evaluate"):
            m, lo, hi = statistics.median(rate[what]), min(rate[what]), max(rate[what])
            say(f"{n:6d} envs  {what:9s} {m:.4e}  [{lo:.4e} .. {hi:.4e}]  spread {100 * (hi - lo) / m:.2f} %")
        say(f"{n:6d} envs  evaluate / play = {statistics.median(rate['evaluate']) / statistics.median(rate['play']):.3f}")
    for n in args.envs:
        for what in ("quiet", "burst"):
            prof = os.path.join(args.scratch, f"prof_evaluate_{what}_{n}")
            child(["rocprofv3", "--kernel-trace", "--stats", "-d", prof, "-o", "r", "--"] + me + ["steps", what, str(n)], 420)
            db = None
            for root, _, files in os.walk(prof):
                for f in files:
                    if f.endswith(".db"):
                        db = os.path.join(root, f)
            say(f"\n## {n} envs, {what} steps (200 of them): rocprofv3 --kernel-trace --stats, a run of its own")
            for l in child([sys.executable, os.path.join(REPO, "tools", "rocprof_summary.py"), "trace", db], 120).splitlines():
                if any(k in l for k in ("k_eval_step", "k_env", "k_mlp_walk", "k_net_walk", "calls", "dispatch footprint")):
                    say(l[:200])
    say("\n(the register columns of the dispatch footprints are the profiler's - allocated granules per half of a 64-wide wavefront; the compiler's figures for k_eval_step: make -C leibnizgym_amd/csrc resource-usage-eval)")
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(out) + "\n")


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    sub = ap.add_subparsers(dest="cmd", required=True)
    lp = sub.add_parser("loop"); lp.add_argument("what", choices=["evaluate", "play"]); lp.add_argument("n", type=int); lp.add_argument("--tree", default=None)
    sp = sub.add_parser("steps"); sp.add_argument("what", choices=["quiet", "burst"]); sp.add_argument("n", type=int)
    a = sub.add_parser("all")
    a.add_argument("--out", default=os.path.join(REPO, "profiles", "r14_evaluate.txt"))
    a.add_argument("--parent-tree", default=None)
    a.add_argument("--rounds", type=int, default=3)
    a.add_argument("--envs", type=int, nargs="+", default=[8192, 65536])
    a.add_argument("--scratch", default=os.environ.get("TMPDIR", "/tmp"))
    ns = ap.parse_args()
    {"loop": cmd_loop, "steps": cmd_steps, "all": cmd_all}[ns.cmd](ns)
