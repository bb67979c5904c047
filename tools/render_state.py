#!/usr/bin/env python3
"""Render envs of a saved simulation state as PNGs: the collision model, exactly as the contact code sees it.  Needs a GPU.

    python tools/render_state.py checkpoint.pt 17 4021 [--out DIR] [--size 512] [--eye X Y Z] [--target X Y Z] [--fov 45] [--flat]
                                 [--object-size X Y Z [--object-density D]]

`checkpoint.pt` is `torch.save(env.state_dict(), ...)` (IsaacEnvBase.state_dict).  Writes DIR/env_<id>.png per env id and DIR/mosaic.png, and prints
the share of each body in every picture.  The model is the default one (or the default with the general box of --object-size): the state rows
carry poses and per-env randomisation, not the shapes."""
import argparse
import os
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

import torch  # noqa: E402

from leibnizgym_amd import _capi as capi, render  # noqa: E402


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("checkpoint")
    ap.add_argument("env_ids", nargs="+", type=int)
    ap.add_argument("--out", default="render_out")
    ap.add_argument("--size", type=int, default=512)
    ap.add_argument("--eye", nargs=3, type=float, default=list(render.DEFAULT_EYE))
    ap.add_argument("--target", nargs=3, type=float, default=list(render.DEFAULT_TARGET))
    ap.add_argument("--fov", type=float, default=render.DEFAULT_FOV_DEG)
    ap.add_argument("--flat", action="store_true", help="palette colours without shading")
    ap.add_argument("--object-size", nargs=3, type=float, default=None)
    ap.add_argument("--object-density", type=float, default=500.0)
    a = ap.parse_args()
    d = torch.load(a.checkpoint, map_location="cpu")
    state = d["state"].to(device="cuda:0", dtype=torch.float32).contiguous()
    if state.dim() != 2 or state.shape[0] != capi.TF_STATE_ROWS:
        raise SystemExit(f"{a.checkpoint}: `state` is {tuple(state.shape)}, expected [{capi.TF_STATE_ROWS}, N]")
    lib = capi.load_hip_library()
    model = lib.box_model(a.object_size, a.object_density) if a.object_size else lib.default_model()
    r = render.SceneRenderer(model, width=a.size, height=a.size, max_views=len(a.env_ids), device="cuda:0", shading="flat" if a.flat else "lit")
    r.set_views(a.env_ids, state.shape[1])           # ValueError for an id outside the checkpoint
    r.set_camera(a.eye, a.target, a.fov)
    out = r.render(state)
    color, seg = out["color"].cpu(), out["segmentation"].cpu()
    for v, env in enumerate(a.env_ids):
        path = os.path.join(a.out, f"env_{env}.png")
        render.write_png(path, color[v])
        counts = torch.bincount(seg[v].flatten().long(), minlength=render.NUM_IDS).tolist()
        print(f"{path}: " + " ".join(f"id{i}:{c}" for i, c in enumerate(counts) if c))
    render.write_png(os.path.join(a.out, "mosaic.png"), render.mosaic(color))
    r.close()


if __name__ == "__main__":
    main()
