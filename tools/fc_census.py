#!/usr/bin/env python3
"""Developer tool (CPU, through the oracle library): how many finger-cube slots are live per env and per wavefront in the bench workload.

The cube role of the 128-register step kernels solves the finger-cube block of a lane's k-th LIVE finger in pass k of a sweep (tf_roles.h, cube_role),
so a wavefront - 64 consecutive envs - runs as many passes as its busiest lane has live fingers.  The loop over the fingers f = 0..2 it replaced ran
finger f's block whenever ANY lane of the wavefront had a live contact with finger f.  This tool counts both on the oracle:

    python tools/fc_census.py [--envs 8192] [--global-envs 65536] [--steps 1000] [--from-step 750] [--every 10] [--dr] [--box]

Workload: bench.workload_kwargs(True) as bench.py sets it up (step counters spread over the episode, actions 2*U-1); a slot counts as live when
TF_S_FC_LINK + f holds a link (value & 3 != 0), which is fc_live of the last substep of the step.
"""
import argparse
import os
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (REPO, os.path.join(REPO, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

import numpy as np  # noqa: E402
import torch  # noqa: E402

import bench  # noqa: E402
from leibnizgym_amd import _capi as capi  # noqa: E402
from leibnizgym_amd.engine import TrifingerEngine, make_config  # noqa: E402
from oracle_util import load_oracle  # noqa: E402

WAVE = 64


def live_slots(state):
    """[3, N] bool: finger-cube slot f of the env is live (TF_S_FC_LINK + f carries the link in its low two bits, + 4 for a fingertip-wall contact)"""
    link = np.asarray(state[capi.S_FC_LINK:capi.S_FC_LINK + 3]).astype(np.int64)
    return (link & 3) != 0


def census(samples):
    """samples: list of [3, N] bool arrays (N a multiple of 64) -> dict of the shares the tool prints"""
    live = np.stack(samples)                                      # [S, 3, N]
    s, _, n = live.shape
    per_env = live.sum(axis=1)                                    # [S, N] live slots of an env
    waves = live.reshape(s, 3, n // WAVE, WAVE)
    blocks_before = waves.any(axis=3).sum(axis=1).ravel()         # fingers live in any lane: blocks of the loop over f
    passes_now = per_env.reshape(s, n // WAVE, WAVE).max(axis=2).ravel()      # live slots of the busiest lane: passes of the per-lane order
    share = lambda a, k: np.bincount(a, minlength=k)[:k] / a.size      # noqa: E731
    return {
        "wave_samples": int(blocks_before.size),
        "lanes_live_per_finger": live.mean(axis=(0, 2)),
        "envs_by_live_slots": share(per_env.ravel(), 4),
        "waves_by_blocks_before": share(blocks_before, 4),
        "waves_by_passes_now": share(passes_now, 4),
        "mean_blocks_before": float(blocks_before.mean()),
        "mean_passes_now": float(passes_now.mean()),
    }


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--envs", type=int, default=8192)
    ap.add_argument("--global-envs", type=int, default=65536, help="global_num_envs of the config (the reward schedule counts global env-steps)")
    ap.add_argument("--steps", type=int, default=1000)
    ap.add_argument("--from-step", type=int, default=750)
    ap.add_argument("--every", type=int, default=10)
    ap.add_argument("--dr", action="store_true", help="every domain-randomisation feature (bench.py --dr)")
    ap.add_argument("--box", action="store_true", help="the cuboid of bench.py --box")
    a = ap.parse_args()
    assert a.envs % WAVE == 0, "whole wavefronts only"
    lib = load_oracle()
    cfg = make_config(lib, a.envs, seed=7, global_num_envs=max(a.global_envs, a.envs),
                      model=lib.box_model((0.02, 0.08, 0.02), 500.0) if a.box else None, **bench.workload_kwargs(True, 4, a.dr))
    eng = TrifingerEngine(cfg, device="cpu", lib=lib)
    gen = torch.Generator().manual_seed(7)
    eng.reset()
    eng.steps.copy_(torch.randint(0, int(cfg.episode_length), (a.envs,), generator=gen, dtype=torch.int64))
    samples = []
    for k in range(a.steps):
        eng.step((torch.rand(a.envs, eng.action_dim, generator=gen) * 2 - 1).contiguous())
        if k >= a.from_step and (k - a.from_step) % a.every == 0:
            samples.append(live_slots(eng.state.numpy()))
    eng.close()
    c = census(samples)
    pc = lambda v: " / ".join("%.2f" % (100.0 * x) for x in v)      # noqa: E731
    print("finger-cube census: %d envs (global %d)%s%s, %d steps, sampled every %d from step %d: %d wavefront samples" %
          (a.envs, max(a.global_envs, a.envs), ", every DR feature" if a.dr else "", ", box object" if a.box else "", a.steps, a.every, a.from_step, c["wave_samples"]))
    print("  lanes live, per finger 0 / 1 / 2 [%%]:                                   %s" % pc(c["lanes_live_per_finger"]))
    print("  envs with 0 / 1 / 2 / 3 live finger-cube slots [%%]:                     %s" % pc(c["envs_by_live_slots"]))
    print("  wavefronts by blocks per sweep, loop over the fingers, 0 / 1 / 2 / 3 [%%]: %s   mean %.2f" % (pc(c["waves_by_blocks_before"]), c["mean_blocks_before"]))
    print("  wavefronts by passes per sweep, per-lane order, 0 / 1 / 2 / 3 [%%]:        %s   mean %.2f" % (pc(c["waves_by_passes_now"]), c["mean_passes_now"]))


if __name__ == "__main__":
    main()
