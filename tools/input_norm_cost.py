#!/usr/bin/env python3
"""Developer tool (GPU box): what `normalize_input` costs in the in-repo PPO (leibnizgym_amd/csrc/ppo_norm.hip, the statistics variant of the forward walk).

    python tools/input_norm_cost.py all [--out profiles/r11_input_norm.txt] [--parent-tree DIR] [--rounds 3]
        every measurement below, each in a FRESH child process under a time limit of its own, the configurations of a comparison alternating; the
        report holds medians and spreads.  --parent-tree: a built checkout of the parent commit, for the third trainer configuration.
    python tools/input_norm_cost.py moments          tfp_moments on the trainer's rollout buffer (262144 rows x (41 + 113) floats = 161 MB: 8192 envs,
                                                     horizon 32) against the expression it replaces, buf.double().mean(0) / .var(0) in torch; HIP events
    python tools/input_norm_cost.py kernels          the program of a `rocprofv3 --kernel-trace --stats` run: rollout-form walk and minibatch gather at
                                                     M = 8192, without and with statistics (the kernel names tell them apart)
    python tools/input_norm_cost.py trainer off|on [--tree DIR]
                                                     frames/s of the trainer at 8192 envs over the last 10 of 40 epochs, keys off / both keys on
A child that fails ends the run: nothing more is started on the GPU after it."""
import argparse
import os
import statistics
import subprocess
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ROWS, DO, DS, M = 262144, 41, 113, 8192
HBM_TBS = 8.0                       # the roofline DESIGN.md uses


def _tree(path):
    sys.path.insert(0, os.path.abspath(path) if path else REPO)


def med_spread(xs):
    return statistics.median(xs), min(xs), max(xs)


# ---- tfp_moments against torch ------------------------------------------------------------------------------------------------------------------
def cmd_moments(args):
    _tree(None)
    import torch
    from leibnizgym_amd import ppo_kernels as pk
    dev = "cuda:0"
    g = torch.Generator(device=dev).manual_seed(1)
    obs = torch.randn(ROWS, DO, device=dev, generator=g) * 3 + 1
    states = torch.randn(ROWS, DS, device=dev, generator=g) * 0.1 + 10

    def kernel():
        return pk.moments([obs, states])

    def torch_form():
        out = []
        for b in (obs, states):
            d = b.double()
            out += [d.mean(0), d.var(0, unbiased=False)]
        return out

    def timed(fn, reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(reps):
            fn()
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) * 1e3 / reps               # us per call
    for fn in (kernel, torch_form):                           # warm-up: code objects, the allocator's blocks
        for _ in range(5):
            fn()
    torch.cuda.synchronize()
    tk, tt = [], []
    for _ in range(7):                                        # alternating windows
        tk.append(timed(kernel, 50))
        tt.append(timed(torch_form, 10))
    # the same numbers from both
    rec = kernel()
    want = torch_form()
    ok = (torch.allclose(rec[1:1 + DO], want[0], rtol=1e-9, atol=1e-12) and torch.allclose(rec[1 + DO:1 + 2 * DO] / rec[0], want[1], rtol=1e-9, atol=1e-12)
          and torch.allclose(rec[2 + 2 * DO:2 + 2 * DO + DS], want[2], rtol=1e-9, atol=1e-12))
    nbytes = ROWS * (DO + DS) * 4
    mk, lk, hk = med_spread(tk)
    mt, lt, ht = med_spread(tt)
    print(f"moments_us kernel {mk:.1f} {lk:.1f} {hk:.1f} torch {mt:.1f} {lt:.1f} {ht:.1f} bytes {nbytes} agree {int(ok)}", flush=True)


# ---- the program of the kernel trace ---------------------------------------------------------------------------------------------------------------
def cmd_kernels(args):
    _tree(None)
    import math
    import torch
    from leibnizgym_amd import ppo_kernels as pk
    dev = "cuda:0"
    g = torch.Generator(device=dev).manual_seed(2)

    def layers(din, dout):
        dims = [din, 400, 200, 100, dout]
        return [(torch.randn(dims[i + 1], dims[i], device=dev, generator=g) / math.sqrt(dims[i]), torch.zeros(dims[i + 1], device=dev), 1 if i < 3 else 0, None)
                for i in range(4)]
    la, lc = layers(DO, 9), layers(DS, 1)
    xa, xc = torch.randn(M, DO, device=dev, generator=g) * 2, torch.randn(M, DS, device=dev, generator=g) * 2
    sa = (torch.zeros(DO, device=dev), torch.ones(DO, device=dev), 5.0)
    sc = (torch.zeros(DS, device=dev), torch.ones(DS, device=dev), 5.0)
    # the minibatch gather of the trainer: obs, act, old_nlp, adv, ret, old_mu, states out of a 32 x 8192 buffer
    T = 32
    srcs = [torch.randn(T * M, w, device=dev, generator=g) for w in (DO, 9)] + [torch.randn(T * M, device=dev, generator=g) for _ in range(3)] + \
           [torch.randn(T * M, w, device=dev, generator=g) for w in (9, DS)]
    nm = [sa] + [None] * 5 + [sc]
    for rep in range(args.reps):
        idx = torch.randperm(T * M, device=dev)[:M]
        for _ in range(8):                                    # alternating: plain, with statistics
            pk.mlp_forward_pair(xa, la, xc, lc, store_hidden=False)
            pk.mlp_forward_pair(xa, la, xc, lc, store_hidden=False, norms=(sa, sc))
            pk.gather_rows(srcs, idx)
            pk.gather_rows(srcs, idx, norm=nm)
    torch.cuda.synchronize()
    print("kernels done", flush=True)


# ---- the trainer -------------------------------------------------------------------------------------------------------------------------------------
def cmd_trainer(args):
    _tree(args.tree)
    import torch
    from leibnizgym_amd.config import compose
    from leibnizgym_amd.envs import TrifingerEnv
    from leibnizgym_amd.ppo import PPOConfig, PPOTrainer
    from leibnizgym_amd.utils.rlg_train import RlGamesGpuEnvAdapter
    from leibnizgym_amd.wrappers import VecTaskPython
    over = ["rlg.params.config.normalize_input=True", "rlg.params.config.central_value_config.normalize_input=True"] if args.keys == "on" else []
    cfg = compose(["gym=trifinger_difficulty_4", f"args.num_envs={M}"] + over)
    dev = "cuda:0"
    n = cfg["gym"]["num_instances"]
    env = TrifingerEnv(config=cfg["gym"], device=dev, verbose=False)
    adapter = RlGamesGpuEnvAdapter("rlgpu", n, env=VecTaskPython(env, rl_device=dev))
    pc = PPOConfig.from_rlg(cfg["rlg"], num_envs=n)
    tr = PPOTrainer(adapter, env.get_obs_dim(), env.get_state_dim(), env.get_action_dim(), pc, device=dev)
    if args.keys == "on":
        assert tr.net.obs_norm is not None and tr.net.state_norm is not None
    marks = []

    def log(st):
        torch.cuda.synchronize()
        marks.append((time.perf_counter(), st["frames"]))
    tr.train(args.epochs, log)
    (t0, f0), (t1, f1) = marks[-11], marks[-1]
    print(f"trainer_fps {args.keys} {(f1 - f0) / (t1 - t0):.4e}", flush=True)


# ---- everything, in fresh processes ---------------------------------------------------------------------------------------------------------------------
def child(argv, limit, env=None):
    """one measurement in a fresh process under its own time limit; its stdout.  A failure ends the whole run (nothing is started behind a fault)."""
    p = subprocess.run(["timeout", "-k", "10", str(limit)] + argv, cwd=REPO, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, env=env)
    if p.returncode != 0:
        sys.stdout.write(p.stdout[-4000:])
        raise SystemExit(f"child {' '.join(argv)} ended with status {p.returncode}: stopping")
    return p.stdout


def cmd_all(args):
    me = [sys.executable, os.path.abspath(__file__)]
    out = []
    say = lambda s="": (out.append(s), print(s, flush=True))   # noqa: E731
    say("# tools/input_norm_cost.py all   (MI355X; every figure from a fresh process, medians with [min .. max])")
    # 1. moments
    runs = []
    for _ in range(args.rounds):
        line = [l for l in child(me + ["moments"], 240).splitlines() if l.startswith("moments_us")][-1].split()
        runs.append([float(x) for x in line[2:5]] + [float(x) for x in line[6:9]] + [int(line[10]), int(line[12])])
    mk, mt = statistics.median(r[0] for r in runs), statistics.median(r[3] for r in runs)
    nbytes = runs[0][6]
    say(f"\n## tfp_moments on the trainer's rollout buffer: {ROWS} rows x ({DO} + {DS}) floats = {nbytes / 1e6:.0f} MB, two launches (slabs, merge); HIP events")
    say(f"kernel   {mk:9.1f} us  [{min(r[1] for r in runs):.1f} .. {max(r[2] for r in runs):.1f}]   {nbytes / mk / 1e6:7.2f} TB/s read = "
        f"{100 * nbytes / mk / 1e6 / HBM_TBS:.0f} % of the {HBM_TBS:.0f} TB/s HBM roofline")
    say(f"torch    {mt:9.1f} us  [{min(r[4] for r in runs):.1f} .. {max(r[5] for r in runs):.1f}]   buf.double().mean(0) / .var(0) per buffer;  kernel / torch = {mk / mt:.3f}")
    say(f"results agree at rtol 1e-9, atol 1e-12: {all(r[7] for r in runs)}")
    # 2. kernel trace
    prof = os.path.join(args.scratch, "prof_input_norm")
    child(["rocprofv3", "--kernel-trace", "--stats", "-d", prof, "-o", "r", "--"] + me + ["kernels"], 420)
    db = None
    for root, _, files in os.walk(prof):
        for f in files:
            if f.endswith(".db"):
                db = os.path.join(root, f)
    say(f"\n## rollout-form walk and minibatch gather at M = {M}, without and with statistics: rocprofv3 --kernel-trace --stats, a run of its own")
    summary = child([sys.executable, os.path.join(REPO, "tools", "rocprof_summary.py"), "trace", db], 120)
    for l in summary.splitlines():
        if any(k in l for k in ("k_mlp_walk", "k_gather_rows", "calls", "dispatch footprint")):
            say(l[:200])
    # 3. trainer
    confs = ([("parent", ["trainer", "off", "--tree", args.parent_tree])] if args.parent_tree else []) + [("keys off", ["trainer", "off"]), ("keys on", ["trainer", "on"])]
    fps = {k: [] for k, _ in confs}
    for _ in range(args.rounds):
        for name, argv in confs:                              # alternating order
            line = [l for l in child(me + argv, 420).splitlines() if l.startswith("trainer_fps")][-1].split()
            fps[name].append(float(line[2]))
    say(f"\n## trainer frames/s at {M} envs over the last 10 of 40 epochs ({args.rounds} fresh processes each, alternating)")
    for name, _ in confs:
        m, lo, hi = med_spread(fps[name])
        say(f"{name:9s} {m:.4e}  [{lo:.4e} .. {hi:.4e}]  spread {100 * (hi - lo) / m:.2f} %")
    base = statistics.median(fps["keys off"])
    on = statistics.median(fps["keys on"])
    say(f"keys on / keys off = {on / base:.4f}" + (f";  keys off / parent = {base / statistics.median(fps['parent']):.4f}" if args.parent_tree else ""))
    epoch_us = ROWS / on * 1e6
    say(f"an epoch with the keys on: {epoch_us:.0f} us; the moments pass ({mk:.1f} us) is {100 * mk / epoch_us:.2f} % of it")
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(out) + "\n")


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    sub = ap.add_subparsers(dest="cmd", required=True)
    sub.add_parser("moments")
    k = sub.add_parser("kernels"); k.add_argument("--reps", type=int, default=25)
    t = sub.add_parser("trainer"); t.add_argument("keys", choices=["off", "on"]); t.add_argument("--tree", default=None); t.add_argument("--epochs", type=int, default=40)
    a = sub.add_parser("all")
    a.add_argument("--out", default=os.path.join(REPO, "profiles", "r11_input_norm.txt"))
    a.add_argument("--parent-tree", default=None)
    a.add_argument("--rounds", type=int, default=3)
    a.add_argument("--scratch", default=os.environ.get("TMPDIR", "/tmp"))
    ns = ap.parse_args()
    {"moments": cmd_moments, "kernels": cmd_kernels, "trainer": cmd_trainer, "all": cmd_all}[ns.cmd](ns)
