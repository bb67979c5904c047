#!/usr/bin/env python3
"""Fingertip-space control demo: the three fingertips trace circles above the resting cube, commanded in Cartesian space through
leibnizgym_amd/wrappers/fingertip_action.py (one launch of tfk_tip_action in front of every env step).

    python scripts/trifinger_fingertip_demo.py [steps] [--num-envs 64] [--mode torque|position] [--record frames/]

Every finger's target moves on a circle of radius 2 cm about (0.08, 0.05, 0.12) of its own frame (the frame of finger 0 turned by the finger's azimuth),
one turn in 200 steps.  The tracking error (mean and largest distance of a tip from its target, metres) is printed every 50 steps.  --record renders the
first four envs with the offscreen renderer of the collision model and writes frames/frame_%06d.png every step.  The default mode is torque (a Cartesian
PD law through the Jacobian transpose with gravity compensation); in position mode the env's own joint PD law is in the loop, which rings at the
default control step of 20 ms.
"""
import argparse
import math
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch  # noqa: E402

from leibnizgym_amd.envs import TrifingerEnv  # noqa: E402
from leibnizgym_amd.wrappers.fingertip_action import FingertipActionEnv  # noqa: E402

CENTRE, RADIUS, PERIOD = (0.08, 0.05, 0.12), 0.02, 200


def circle_command(params, k, n, device):
    """the absolute command [n, 9] whose targets are the point of step k on every finger's circle"""
    a = 2.0 * math.pi * k / PERIOD
    u = torch.tensor([CENTRE[0] + RADIUS * math.cos(a), CENTRE[1] + RADIUS * math.sin(a), CENTRE[2]], device=device)
    lo, hi = torch.tensor(params["box_lo"], device=device), torch.tensor(params["box_hi"], device=device)
    return ((u - lo) / (hi - lo) * 2.0 - 1.0).repeat(3).expand(n, 9).contiguous()


def main(steps, num_envs, mode, record=None):
    env_config = {"num_instances": num_envs, "command_mode": mode,
                  "reset_distribution": {"object_initial_state": {"type": "default"}}}          # the cube rests in the centre
    if record is not None:
        env_config["native"] = {"render": {"record_dir": record}}
    env = TrifingerEnv(config=env_config, device="cuda:0", verbose=False, visualize=record is not None)
    tips = FingertipActionEnv(env, frame="absolute")
    tips.reset()
    for k in range(1, steps + 1):
        tips.step(circle_command(tips.params, k, num_envs, env.device))
        if record is not None:
            env.render()
        if k % 50 == 0 or k == steps:
            err = (tips.last_target - tips.tip_positions()).reshape(num_envs, 3, 3).norm(dim=2)          # (the copy to the host synchronises)
            print(f"step {k:5d}: tracking error mean {float(err.mean()):.4f} m, max {float(err.max()):.4f} m", flush=True)
    env.close()


if __name__ == "__main__":
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("steps", nargs="?", type=int, default=600)
    ap.add_argument("--num-envs", type=int, default=64)
    ap.add_argument("--mode", choices=["torque", "position"], default="torque")
    ap.add_argument("--record", metavar="DIR", default=None, help="render every step and write DIR/frame_%%06d.png")
    a = ap.parse_args()
    main(a.steps, a.num_envs, a.mode, a.record)
