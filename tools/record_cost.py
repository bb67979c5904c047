#!/usr/bin/env python3
"""Developer tool (GPU box): what the episode flight recorder costs (include/trifinger_ppo_record.h: tfp_record_step, ONE launch behind every env step of an
evaluation that records).  Modelled on tools/track_cost.py.

    python tools/record_cost.py all [--out profiles/r17_record.txt] [--parent-tree DIR] [--rounds 3] [--only kernels,evaluate]
        every measurement below, each in a FRESH child process under a time limit of its own, the configurations of a comparison alternating; the
        report holds medians and spreads.  --parent-tree: a built checkout of the parent commit, for the third evaluate configuration.
    python tools/record_cost.py kernels --n N        the program of a counter-free `rocprofv3 --kernel-trace --stats` run: on a QUIET step (nobody ends, nobody
                                                     frozen, every env armed, every = 1: every lane records) the record launch, the evaluator's k_eval_step
                                                     and a torch copy_ of state[0:59] into a [59, N] tensor - the traffic no form of this feature can avoid -
                                                     alternating, 200 launches each.  The bar: the record launch stays below k_eval_step + the copy.
    python tools/record_cost.py evaluate off|on [--tree DIR]
                                                     seconds of PPOTrainer.evaluate(episodes_per_env=1) at 8192 envs (the second of two evaluations of a
                                                     fresh trainer), without and with record={"select": "failure", "max_episodes": 16}: every env
                                                     watched, a ring of a whole episode, the first 16 frozen episodes harvested at the end
A child that fails ends the run: nothing more is started on the GPU after it."""
import argparse
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from track_cost import REPO, _tree, child, med_spread, trace  # noqa: E402

M = 8192
SIZES = (8192, 65536)
RING = 8
HARVEST = 16


def cmd_kernels(args):
    _tree(None)
    import torch
    from types import SimpleNamespace
    from leibnizgym_amd import _capi as capi
    from leibnizgym_amd import record as rc
    from leibnizgym_amd.evaluate import EpisodeStats
    dev, n = "cuda:0", args.n
    g = torch.Generator(device=dev).manual_seed(2)
    state = torch.randn(capi.TF_STATE_ROWS, n, device=dev, generator=g) * 0.1
    eng = SimpleNamespace(state=state, reward=torch.randn(n, device=dev, generator=g), reset_buf=torch.zeros(n, dtype=torch.bool, device=dev),
                          goal_reset_buf=torch.zeros(n, dtype=torch.bool, device=dev), steps=torch.full((n,), 5, dtype=torch.int64, device=dev))
    rec = rc.EpisodeRecorder(eng, select="failure", every=1, length=RING, pos_tol=0.02, ori_tol=0.25, rule=1, episode_length=750)
    rec.env_rec[rc.ENV_STATE] = rc.ARMED                      # every env in the middle of an episode it was seen the start of
    evs = EpisodeStats(eng, 0.02, 0.25, rule=1)
    dst = torch.empty(rc.REC_STATE_ROWS, n, device=dev)
    for _ in range(args.reps):                                # alternating, all on a quiet step: nobody ends
        rec.update()
        evs.update()
        dst.copy_(state[0:rc.REC_STATE_ROWS])
    torch.cuda.synchronize()
    c = rec.counts()
    assert c["records"] == args.reps * n and c["ended_armed"] == 0 and c["frozen"] == 0, c
    print("kernels done", flush=True)


def cmd_evaluate(args):
    _tree(args.tree)
    import torch
    from leibnizgym_amd.config import compose
    from leibnizgym_amd.envs import TrifingerEnv
    from leibnizgym_amd.ppo import PPOConfig, PPOTrainer
    from leibnizgym_amd.utils.rlg_train import RlGamesGpuEnvAdapter
    from leibnizgym_amd.wrappers import VecTaskPython
    cfg = compose(["gym=trifinger_difficulty_4", f"args.num_envs={M}"])
    dev = "cuda:0"
    n = cfg["gym"]["num_instances"]
    env = TrifingerEnv(config=cfg["gym"], device=dev, verbose=False)
    adapter = RlGamesGpuEnvAdapter("rlgpu", n, env=VecTaskPython(env, rl_device=dev))
    tr = PPOTrainer(adapter, env.get_obs_dim(), env.get_state_dim(), env.get_action_dim(), PPOConfig.from_rlg(cfg["rlg"], num_envs=n), device=dev)
    kw = {"record": {"select": "failure", "max_episodes": HARVEST}} if args.keys == "on" else {}
    for _ in range(2):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        res = tr.evaluate(episodes_per_env=1, **kw)
        torch.cuda.synchronize()
        dt = time.perf_counter() - t0
    print(f"evaluate_s {args.keys} {dt:.6f} steps {res['steps']} episodes {res['episodes']} recorded {res.get('episodes_recorded', '-')}", flush=True)


def cmd_all(args):
    me = [sys.executable, os.path.abspath(__file__)]
    out = []
    say = lambda s="": (out.append(s), print(s, flush=True))   # noqa: E731
    only = set(args.only.split(","))
    say("# tools/record_cost.py all   (MI355X; every figure from a fresh process, medians with [min .. max])")
    extra_us = None
    if "kernels" in only:
        for n in SIZES:
            table, lines = trace(me, ["kernels", "--n", str(n)], args.scratch, f"record_{n}")
            say(f"\n## after-step launches at n = {n}: counter-free rocprofv3 --kernel-trace --stats, a run of its own, alternating on QUIET steps "
                f"(every env armed, nobody ends, nobody frozen, every = 1, ring of {RING})")
            for l in lines:
                if any(k in l for k in ("k_record_step", "k_eval_step", "opy", "calls", "dispatch footprint")):
                    say(l[:200])
            avg = lambda key: next((v[1] for k, v in table.items() if key in k), None)      # noqa: E731
            r, e = avg("k_record_step"), avg("k_eval_step")
            c = next((v[1] for k, v in table.items() if "opy" in k and v[0] >= 200), None)
            if None not in (r, e, c):
                say(f"bar (a): record launch {r:.2f} us against k_eval_step's quiet step {e:.2f} us + the copy of state[0:59] {c:.2f} us = {e + c:.2f} us: "
                    f"{'MET' if r <= e + c else 'NOT MET'}")
                if n == M:
                    extra_us = r
    if "evaluate" in only:
        confs = ([("parent", ["off", "--tree", args.parent_tree])] if args.parent_tree else []) + [("record off", ["off"]), ("record on", ["on"])]
        secs, steps = {k: [] for k, _ in confs}, None
        for _ in range(args.rounds):
            for name, argv in confs:
                line = [l for l in child(me + ["evaluate"] + argv, 420).splitlines() if l.startswith("evaluate_s")][-1].split()
                secs[name].append(float(line[2]))
                steps = int(line[4])
                say(f"  {name:10s} {' '.join(line)}")
        say(f"\n## PPOTrainer.evaluate(episodes_per_env=1) at {M} envs, {steps} steps, seconds ({args.rounds} fresh processes each, alternating; record on: "
            f"select failure, every env watched, whole-episode ring, {HARVEST} episodes harvested)")
        for name, _ in confs:
            m, lo, hi = med_spread(secs[name])
            say(f"{name:10s} {m:.4f}  [{lo:.4f} .. {hi:.4f}]  spread {100 * (hi - lo) / m:.2f} %")
        if args.parent_tree:
            _, plo, phi = med_spread(secs["parent"])
            on, off = statistics.median(secs["record on"]), statistics.median(secs["record off"])
            say(f"bar: record off inside the parent's own spread [{plo:.4f} .. {phi:.4f}]: {'MET' if plo <= off <= phi else 'NOT MET'} ({off:.4f})")
            if extra_us is not None:
                hi = phi + extra_us * 1e-6 * steps
                say(f"bar (b): record on no higher than the parent's high end plus {extra_us:.2f} us x {steps} steps = {hi:.4f} s: "
                    f"{'MET' if on <= hi else 'NOT MET'} ({on:.4f})")
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "a" if args.append else "w") as f:
        f.write("\n".join(out) + "\n")


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    sub = ap.add_subparsers(dest="cmd", required=True)
    k = sub.add_parser("kernels"); k.add_argument("--reps", type=int, default=200); k.add_argument("--n", type=int, default=M)
    t = sub.add_parser("evaluate"); t.add_argument("keys", choices=["off", "on"]); t.add_argument("--tree", default=None)
    a = sub.add_parser("all")
    a.add_argument("--out", default=os.path.join(REPO, "profiles", "r17_record.txt"))
    a.add_argument("--only", default="kernels,evaluate", help="which parts to run (a run split over several sittings appends: --append)")
    a.add_argument("--append", action="store_true")
    a.add_argument("--parent-tree", default=None)
    a.add_argument("--rounds", type=int, default=3)
    a.add_argument("--scratch", default=os.environ.get("TMPDIR", "/tmp"))
    ns = ap.parse_args()
    {"kernels": cmd_kernels, "evaluate": cmd_evaluate, "all": cmd_all}[ns.cmd](ns)
