#!/usr/bin/env python3
"""Cost of the collision-model renderer (leibnizgym_amd/render.py) on the state of a 4096-env rollout.  Needs a GPU.

    python tools/render_bench.py [--out profiles/r8_render_cost.txt] [--quick]

Per configuration (1, 4 and 16 views at 256 x 256, 16 views at 512 x 512): HIP events around 200 back-to-back renders after 20 warm-up renders,
repeated 7 times (median, min - max); the recording rate of env.render() with `record_dir` (render + one device-to-host copy + mosaic + PNG);
registers, LDS, scratch and occupancy from the compiler (`make resource-usage-render`); the mean number of march samples per ray, derived from
the fp64 reference of tests/render_ref.py on its three seeded scenes.  --quick: one short pass (the program of a `rocprofv3 --kernel-trace` run).
"""
import argparse
import os
import statistics
import subprocess
import sys
import tempfile
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tests"))

import torch  # noqa: E402

from leibnizgym_amd import _capi as capi, render  # noqa: E402
from leibnizgym_amd.engine import TrifingerEngine, make_config  # noqa: E402
from leibnizgym_amd.envs import TrifingerEnv  # noqa: E402

DEV = "cuda:0"


def rollout_state(lib, n=4096, steps=50):
    import parity_util as pu
    cfg = make_config(lib, n, seed=11, episode_length=40, **dict(pu.CONFIGS["d4_torque_asym"]))
    eng = TrifingerEngine(cfg, device=DEV, lib=lib)
    eng.reset()
    for t in range(steps):
        eng.step(pu.actions_for(t, n, eng.action_dim, 11).to(DEV))
    st = eng.state.clone()
    eng.close()
    return cfg.model, st


def time_renders(r, st, renders, warmup):
    for _ in range(warmup):
        r.render(st)
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(renders):
        r.render(st)
    b.record()
    b.synchronize()
    return a.elapsed_time(b) * 1e3 / renders          # us per render


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--out", default=None)
    ap.add_argument("--quick", action="store_true")
    a = ap.parse_args()
    lib = capi.load_hip_library()
    model, st = rollout_state(lib)
    lines = [f"# tools/render_bench.py on {torch.cuda.get_device_name(0)}: state of a 4096-env rollout after 50 random steps, default camera, shading lit",
             "# HIP events around 200 back-to-back renders after 20 warm-up renders, 7 repeats: median (min - max)"]
    reps, renders, warm = (1, 20, 5) if a.quick else (7, 200, 20)
    for views, size in ((1, 256), (4, 256), (16, 256), (16, 512)):
        r = render.SceneRenderer(model, width=size, height=size, max_views=views, device=DEV)
        r.set_views(list(range(0, 4096, 4096 // views)), 4096)
        ts = [time_renders(r, st, renders, warm) for _ in range(reps)]
        r.close()
        med = statistics.median(ts)
        lines.append(f"{views:3d} views {size} x {size}: {med:9.1f} us per render ({min(ts):.1f} - {max(ts):.1f}); "
                     f"{med / views:8.1f} us per view; {views * size * size / med:8.1f} Mrays/s")
    if not a.quick:
        # what a user sees: env.render() with record_dir next to the step
        with tempfile.TemporaryDirectory() as d:
            env = TrifingerEnv(config={"num_instances": 4096, "command_mode": "torque",
                                       "native": {"render": {"envs": list(range(16)), "record_dir": d}}}, device=DEV, verbose=False, visualize=True)
            env.reset()
            act = torch.zeros(4096, 9, device=DEV)
            rates = []
            for _ in range(5):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                for _ in range(20):
                    env.step(act)
                    env.render()
                torch.cuda.synchronize()
                rates.append(20 / (time.perf_counter() - t0))
            env.close()
        lines.append(f"recording 16 views 256 x 256 (step + render + device-to-host copy + mosaic 1024 x 1024 + PNG on one host thread): "
                     f"{statistics.median(rates):.1f} frames/s ({min(rates):.1f} - {max(rates):.1f}, 5 x 20 frames); the host's PNG deflate, not the kernel, sets it")
        ru = subprocess.run(["make", "-s", "-C", os.path.join(REPO, "leibnizgym_amd", "csrc"), "resource-usage-render"], capture_output=True, text=True)
        lines.append("# compiler (-Rpass-analysis=kernel-resource-usage):")
        lines += ["  " + ln for ln in ru.stdout.strip().splitlines()]
        import numpy as np
        import render_ref as rr
        s = [rr.render(rr.Scene(model, rr.seeded_state(c)))["samples"] for c in range(3)]
        lines.append("# march samples per ray, fp64 reference on its three seeded scenes (256 x 256): mean "
                     + ", ".join(f"{x.mean():.1f}" for x in s) + "; maximum of an 8 x 8 wavefront tile, mean over tiles "
                     + ", ".join(f"{x.reshape(32, 8, 32, 8).max(axis=(1, 3)).mean():.1f}" for x in s) + f"; limit {rr.MARCH['max_steps']}")
        assert np.all([x.max() <= rr.MARCH["max_steps"] for x in s])
    text = "\n".join(lines) + "\n"
    print(text, end="")
    if a.out:
        with open(a.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
