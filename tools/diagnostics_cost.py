#!/usr/bin/env python3
"""Developer tool (GPU box): what `diagnostics` costs in the in-repo PPO (include/trifinger_ppo_diag.h: tfp_ppo_loss_diag in place of the objective's entry
point, tfp_clip_adam_diag in place of tfp_clip_adam - the same launches, their DIAG instantiations).  Modelled on tools/symmetry_cost.py.

    python tools/diagnostics_cost.py all --parent-tree DIR [--out profiles/r23_diagnostics.txt] [--rounds 3] [--only launches,trainer]
        every measurement below, each in a FRESH child process under a time limit of its own, parent and tree alternating; the report holds medians and
        spreads and says MET / NOT MET by the letter.  --parent-tree: a built checkout of the parent commit.
    python tools/diagnostics_cost.py launches plain|diag [--tree DIR]
                                                     the program of a counter-free `rocprofv3 --kernel-trace --stats` run: the objective at B = 8192, A = 9 and
                                                     the optimiser's two launches over the trainer's flat buffer (118 k + 146 k floats), 300 steps, without / with
                                                     the record
    python tools/diagnostics_cost.py trainer off|on [--tree DIR]
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
M = 8192
KEYS = ["rlg.params.config.diagnostics=True"]
KERNELS = ("k_ppo_loss", "k_grad_sqnorms", "k_clip_adam")


def _tree(path):
    sys.path.insert(0, os.path.abspath(path) if path else REPO)


def med_spread(xs):
    return statistics.median(xs), min(xs), max(xs)


# ---- the program of the kernel trace ---------------------------------------------------------------------------------------------------------------
def cmd_launches(args):
    _tree(args.tree)
    import torch
    from leibnizgym_amd import ppo_kernels as pk
    dev = "cuda:0"
    g = torch.Generator(device=dev).manual_seed(2)
    r = lambda *s: torch.randn(*s, device=dev, generator=g)               # noqa: E731
    B, A = M, 9
    mu, act, old_mu = r(B, A), r(B, A), r(B, A)
    log_std, v, ret, adv = r(A) * 0.1, r(B), r(B), r(B)
    nlp = (0.5 * ((act - mu) / log_std.exp()) ** 2 + log_std + 0.9189385332046727).sum(-1)
    old_nlp = (nlp + 0.3 * r(B)).contiguous()                             # ratios on both sides of the clip range
    stats = torch.zeros(4, device=dev)
    fo = pk.FlatClipAdam([torch.nn.Parameter(r(118020))], [torch.nn.Parameter(r(146004))], 3e-4, 5e-4, 1.0, 1.0)
    kw = {"diag": pk.new_diag(dev)} if args.keys == "diag" else {}
    for _ in range(args.reps):
        pk.ppo_loss_and_grads(mu, log_std, v, act, old_nlp, adv, ret, old_mu, stats, 0.2, 1.0, 0.0, 1e-4, **kw)
        fo.flat_g.copy_(fo.flat_p)
        fo.step(gathered=True, **kw)
    torch.cuda.synchronize()
    print("launches done", kw["diag"].tolist() if kw else "", flush=True)


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
        assert tr.diag is not None and tr.fused_loss
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
    print(f"trainer_fps {args.keys} {(f1 - f0) / (t1 - t0):.4e} mb_step_us {1e6 * statistics.median(upd[-10:]) / steps:.1f} clip_frac "
          f"{stats[-1].get('clip_frac', float('nan')):.4f} approx_kl {stats[-1].get('approx_kl', float('nan')):.5f}", flush=True)


# ---- everything, in fresh processes ---------------------------------------------------------------------------------------------------------------------
def child(argv, limit, env=None):
    """one measurement in a fresh process under its own time limit; its stdout.  A failure ends the whole run (nothing is started behind a fault)."""
    p = subprocess.run(["timeout", "-k", "10", str(limit)] + argv, cwd=REPO, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, env=env)
    if p.returncode != 0:
        sys.stdout.write(p.stdout[-4000:])
        raise SystemExit(f"child {' '.join(argv)} ended with status {p.returncode}: stopping")
    return p.stdout


def trace(me, argv, scratch, tag):
    """{kernel of KERNELS: avg us} of a child under rocprofv3 --kernel-trace --stats"""
    prof = os.path.join(scratch, f"prof_diagnostics_{tag}")
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
        table[m.group(1).strip()] = float(m.group(4))
    return {k: next((v for name, v in table.items() if k in name), None) for k in KERNELS}


def cmd_all(args):
    me = [sys.executable, os.path.abspath(__file__)]
    out = []
    say = lambda s="": (out.append(s), print(s, flush=True))   # noqa: E731
    only = set(args.only.split(","))
    say("# tools/diagnostics_cost.py all   (MI355X; every figure from a fresh process, medians with [min .. max]; parent and tree alternating)")
    if "launches" in only:
        confs = [("parent", ["plain", "--tree", args.parent_tree]), ("key off", ["plain"]), ("key on", ["diag"])]
        us = {name: {k: [] for k in KERNELS} for name, _ in confs}
        for rnd in range(args.rounds):
            for name, argv in confs:
                got = trace(me, ["launches"] + argv, args.scratch, f"{name.replace(' ', '_')}_{rnd}")
                for k in KERNELS:
                    if got[k] is None:
                        raise SystemExit(f"{name}: no {k} in the trace: stopping")
                    us[name][k].append(got[k])
        say(f"\n## the objective at B = {M}, A = 9 and the optimiser's two launches over 118 k + 146 k floats: counter-free rocprofv3 --kernel-trace --stats, "
            f"300 steps per run, {args.rounds} runs each; average launch in us")
        for name, _ in confs:
            say(f"{name:9s} " + "   ".join("{} {:.2f} [{:.2f} .. {:.2f}]".format(k, *med_spread(us[name][k])) for k in KERNELS))
        pm, plo, phi = med_spread(us["parent"]["k_ppo_loss"])
        on = statistics.median(us["key on"]["k_ppo_loss"])
        bound = pm + (phi - plo) + 1.0
        say(f"bar: the objective with the record ({on:.2f} us) no more than the parent's launch ({pm:.2f} us) + the parent's spread ({phi - plo:.2f} us) + 1 us = "
            f"{bound:.2f} us: {'MET' if on <= bound else 'NOT MET'}")
        for k in KERNELS[1:]:
            _, lo, hi = med_spread(us["parent"][k])
            x = statistics.median(us["key on"][k])
            say(f"bar: {k} with the record ({x:.2f} us) inside the parent's spread [{lo:.2f} .. {hi:.2f}] us: {'MET' if lo <= x <= hi else 'MET (below it)' if x < lo else 'NOT MET'}")
    if "trainer" in only:
        confs = [("parent", ["off", "--tree", args.parent_tree]), ("key off", ["off"]), ("key on", ["on"])]
        fps, mbs = {k: [] for k, _ in confs}, {k: [] for k, _ in confs}
        for _ in range(args.rounds):
            for name, argv in confs:
                line = [l for l in child(me + ["trainer", "--epochs", str(args.epochs)] + argv, 420).splitlines() if l.startswith("trainer_fps")][-1].split()
                fps[name].append(float(line[2])); mbs[name].append(float(line[4]))
        say(f"\n## trainer frames/s at {M} envs over the last 10 of {args.epochs} epochs, and the time of one minibatch step (update / (mini_epochs x minibatches), "
            f"median of those epochs); {args.rounds} fresh processes each, alternating")
        for name, _ in confs:
            m, lo, hi = med_spread(fps[name])
            s, slo, shi = med_spread(mbs[name])
            say(f"{name:9s} {m:.4e}  [{lo:.4e} .. {hi:.4e}]  spread {100 * (hi - lo) / m:.2f} %   minibatch step {s:.1f} us [{slo:.1f} .. {shi:.1f}]")
        off, on = statistics.median(fps["key off"]), statistics.median(fps["key on"])
        _, plo, phi = med_spread(fps["parent"])
        _, slo, shi = med_spread(mbs["parent"])
        soff = statistics.median(mbs["key off"])
        say(f"bar: key off frames/s inside the parent's own spread [{plo:.4e} .. {phi:.4e}]: {'MET' if plo <= off <= phi else 'MET (above it)' if off > phi else 'NOT MET'}")
        say(f"bar: key off minibatch step inside the parent's own spread [{slo:.1f} .. {shi:.1f}] us: {'MET' if slo <= soff <= shi else 'MET (below it)' if soff < slo else 'NOT MET'}")
        say(f"key on / key off = {on / off:.4f} in frames/s, minibatch step {statistics.median(mbs['key on']):.1f} us against {soff:.1f} us (no bar)")
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "a" if args.append else "w") as f:
        f.write("\n".join(out) + "\n")


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    sub = ap.add_subparsers(dest="cmd", required=True)
    k = sub.add_parser("launches"); k.add_argument("keys", choices=["plain", "diag"]); k.add_argument("--tree", default=None); k.add_argument("--reps", type=int, default=300)
    t = sub.add_parser("trainer"); t.add_argument("keys", choices=["off", "on"]); t.add_argument("--tree", default=None); t.add_argument("--epochs", type=int, default=40)
    a = sub.add_parser("all")
    a.add_argument("--out", default=os.path.join(REPO, "profiles", "r23_diagnostics.txt"))
    a.add_argument("--only", default="launches,trainer", help="which parts to run (a run split over several sittings appends: --append)")
    a.add_argument("--append", action="store_true")
    a.add_argument("--epochs", type=int, default=40)
    a.add_argument("--parent-tree", required=True)
    a.add_argument("--rounds", type=int, default=3)
    a.add_argument("--scratch", default=os.environ.get("TMPDIR", "/tmp"))
    ns = ap.parse_args()
    {"launches": cmd_launches, "trainer": cmd_trainer, "all": cmd_all}[ns.cmd](ns)
