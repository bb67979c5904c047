#!/usr/bin/env python3
"""Planning demo: a few envs are driven by sampling-based MPC (leibnizgym_amd/planning.py: MPPIPlanner) on a population of forked envs - no training, no
checkpoint.  Every control step forks each env into `--samples` copies, rolls them `--horizon` steps forward on the GPU and applies the first action of
the return-weighted mean.

    python scripts/trifinger_mppi_demo.py [steps] [--num-envs 4] [--samples 256] [--horizon 16] [--mode torque|position] [--difficulty 1] [--frames DIR]

Every 50 steps (one simulated second) it prints the reward collected per env in that second, the mean distance of the cubes from their goals, the
planner's effective sample size and its control steps per wall second.  --frames renders the planned envs with the offscreen renderer of the collision
model (leibnizgym_amd/render.py) and writes DIR/frame_%06d.png every step."""
import argparse
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch  # noqa: E402

from leibnizgym_amd import _capi as capi  # noqa: E402
from leibnizgym_amd.engine import TrifingerEngine, make_config  # noqa: E402
from leibnizgym_amd.planning import MPPIPlanner  # noqa: E402

SIGMA = {"position": 0.3, "torque": 0.5}


def main(steps, num_envs, samples, horizon, mode, difficulty, frames=None, device="cuda:0", lib=None, seed=3):
    lib = lib if lib is not None else capi.load_hip_library()
    plant = TrifingerEngine(make_config(lib, num_envs, seed=seed, command_mode=mode, task_difficulty=difficulty, episode_length=0), device=device, lib=lib)
    plant.reset()
    planner = MPPIPlanner(plant, samples=samples, horizon=horizon, sigma=SIGMA[mode], lam=0.3)
    renderer = None
    if frames is not None:
        from leibnizgym_amd.render import SceneRenderer, mosaic, write_png
        renderer = SceneRenderer(plant.cfg.model, max_views=min(num_envs, 16), device=device)
        renderer.set_camera()
        renderer.set_views(list(range(min(num_envs, 16))), num_envs)
    second = torch.zeros(num_envs, device=plant.device)
    t0 = time.time()
    for k in range(1, steps + 1):
        planner.act()
        second += plant.reward
        planner.reset_plan()                                         # an env whose episode just ended starts from the zero sequence
        if renderer is not None:
            write_png(os.path.join(frames, f"frame_{k:06d}.png"), mosaic(renderer.render(plant.state)["color"]))
        if k % 50 == 0 or k == steps:
            dist = (plant.cube[0:3] - plant.goal[0:3]).norm(dim=0)                       # (the copies to the host synchronise)
            rate = k / (time.time() - t0)
            print(f"step {k:5d}: reward in the last second {[round(float(x), 1) for x in second]}, distance to goal {float(dist.mean()):.4f} m, "
                  f"ess {float(planner.stats()['ess'].mean()):.1f} of {samples}, {rate:.1f} control steps/s", flush=True)
            second.zero_()
    planner.close()
    plant.close()


if __name__ == "__main__":
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("steps", nargs="?", type=int, default=300)
    ap.add_argument("--num-envs", type=int, default=4)
    ap.add_argument("--samples", type=int, default=256)
    ap.add_argument("--horizon", type=int, default=16)
    ap.add_argument("--mode", choices=["torque", "position"], default="torque")
    ap.add_argument("--difficulty", type=int, default=1)
    ap.add_argument("--frames", metavar="DIR", default=None, help="render every step and write DIR/frame_%%06d.png")
    a = ap.parse_args()
    main(a.steps, a.num_envs, a.samples, a.horizon, a.mode, a.difficulty, a.frames)
