"""Developer tool (GPU box): kernel time of the fused step (HIP events) on the bench workload with TfModel.cube_wall_surface off and on.
    python tools/surface_cost.py [N ...]            (default: 8192 16384 65536)
Off: the instantiation TF_KERNEL_AUTO picks for the default model; on: the one it picks with the switch (the 256-register kernels at every size - at
65536 envs that is a move from the 128-register kernel as well).  Best of three windows of 1000 steps, random actions drawn in the launch."""
import os
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
import torch

import bench
from leibnizgym_amd import _capi
from leibnizgym_amd.engine import TrifingerEngine, make_config


def kernel_us(lib, n, surface, asym=True, variant=None):
    m = lib.default_model()
    m.cube_wall_surface = 1 if surface else 0
    eng = TrifingerEngine(make_config(lib, n, seed=7, model=m, **bench.workload_kwargs(asym)), device="cuda:0", lib=lib)
    if variant is not None:
        eng.kernel_variant = variant
    picked = eng.kernel_variant
    eng.reset()
    for _ in range(50):
        eng.step_random()
    best = 1e9
    for _ in range(3):
        eng.enable_kernel_timing(1000)
        for _ in range(1000):
            eng.step_random()
        torch.cuda.synchronize()
        ms, cnt = eng.kernel_time_ms()
        best = min(best, ms / cnt * 1e3)
    eng.close()
    return best, picked


if __name__ == "__main__":
    sizes = [int(x) for x in sys.argv[1:]] or [8192, 16384, 65536]
    lib = _capi.load_hip_library()
    print(f"{'envs':>6}  {'off (AUTO)':>22}  {'on (AUTO)':>22}  {'on / off':>8}")
    for n in sizes:
        off, v_off = kernel_us(lib, n, False)
        on, v_on = kernel_us(lib, n, True)
        line = f"{n:6d}  {off:8.2f} us {v_off:>12s}  {on:8.2f} us {v_on:>12s}  {on / off:8.3f}"
        if v_on != v_off:      # the same instantiation without the switch: the cost of the rows alone
            same, _ = kernel_us(lib, n, False, variant=v_on)
            line += f"   (off, {v_on}: {same:.2f} us; on / that {on / same:.3f})"
        print(line, flush=True)
