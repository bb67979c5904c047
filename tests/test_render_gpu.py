"""The renderer of the collision model on the GPU against the fp64 reference of tests/render_ref.py: field parity (tfr_test_field), image
parity, shading, read-only behaviour and the public API.  The conditions the pixel comparisons rely on (how many pixels are edge pixels or
unresolved) are asserted on the reference alone in tests/test_render_host.py."""
import glob
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import parity_util as pu
import render_ref as rr
from leibnizgym_amd import _capi as capi
from leibnizgym_amd.engine import TrifingerEngine, make_config
from leibnizgym_amd.envs import TrifingerEnv
from leibnizgym_amd.wrappers import VecTaskPython

pytestmark = pytest.mark.gpu
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEV = "cuda:0"
CAP_ALL, CAP_FG = 0.15, 0.25            # excluded share of all pixels / of the robot and object pixels (tests/test_render_host.py)


def f32_exact(cols):
    """state columns as the device sees them: rounded to fp32 once, the reference continues from those numbers"""
    st = np.stack(cols, 1).astype(np.float32)
    return st, torch.from_numpy(st).to(DEV).contiguous()


def seeded_scenes():
    cols = [rr.seeded_state(c) for c in range(3)]
    return f32_exact(cols)


def compare_image(ref, color, depth, seg, what, shading_bound=None):
    """one view against the reference image `ref` on the pixels that are neither edge nor unresolved in the reference -> printed figures"""
    share_all, share_fg, ex = rr.excluded_shares(ref)
    assert share_all <= CAP_ALL and share_fg <= CAP_FG, (what, share_all, share_fg)
    cmp_ = ~ex
    same = seg == ref["seg"]
    n_cmp, n_bad = int(cmp_.sum()), int((cmp_ & ~same).sum())
    ok = cmp_ & same
    hit = ok & np.isfinite(ref["depth"])
    derr = float(np.abs(depth[hit] - ref["depth"][hit]).max())
    print(f"{what}: compared {n_cmp} px (excluded {share_all:.4f} / {share_fg:.4f}); id mismatches {n_bad}; depth err max {derr:.3e}")
    assert n_bad <= 0.0005 * n_cmp, (what, n_bad, n_cmp)
    assert np.all(np.isinf(depth[ok & ~np.isfinite(ref["depth"])])), what
    assert derr <= 2e-4, (what, derr)
    assert np.all(color[..., 3] == 255), what
    # the goal ghost: exact on the pixels where the reference blends it, away from the ghost's own silhouette and from where it meets the scene
    gedge = rr.edges(ref["ghost"]) | (np.abs(ref["ghost_t"] - np.where(np.isfinite(ref["depth"]), ref["depth"], 1e9)) < 1e-3)
    plain, blended = ok & ~ref["ghost"] & ~gedge, ok & ref["ghost"] & ~gedge
    if shading_bound is None:
        assert np.array_equal(color[plain][:, :3], rr.PALETTE[ref["seg"][plain]]), what
        want = (rr.PALETTE[ref["seg"][blended]].astype(np.uint32) + rr.GHOST[None] + 1) >> 1
        assert np.array_equal(color[blended][:, :3], want), what
    else:
        sel = plain | blended
        diff = int(np.abs(color[sel][:, :3].astype(int) - ref["color"][sel][:, :3].astype(int)).max())
        print(f"{what}: shaded colour, max per-channel difference {diff} (bound {shading_bound})")
        assert diff <= shading_bound, (what, diff)
    return int(blended.sum())


@pytest.fixture(scope="module")
def render_mod(hip):
    from leibnizgym_amd import render
    return render


# ---- 5. field parity ---------------------------------------------------------------------------------------------------
def test_field_parity(hip, render_mod):
    """20 000 seeded points per state: distance and boundary distance within 2e-6 of the fp64 reference; ids equal wherever the reference's best and
    second-best distances differ by more than 1e-5 m, with at most 1 % of the points so excluded"""
    cases = [("default", hip.default_model(), rr.seeded_state(1)),
             ("extended DR", hip.default_model(), rr.seeded_state(2, ext_dr=True)),
             ("phase-3 cuboid", hip.box_model((0.02, 0.08, 0.02), 500.0), rr.seeded_state(1, half_z=0.01))]
    rng = np.random.default_rng(7)
    for k, (name, model, col) in enumerate(cases):
        st_h, st_d = f32_exact([rr.neutral_state(), col, rr.neutral_state()])          # the env under test sits between two others
        pts = (rng.uniform([-0.3, -0.3, 0.0], [0.3, 0.3, 0.45], (20000, 3))).astype(np.float32)
        r = render_mod.SceneRenderer(model, width=64, height=64, max_views=1, device=DEV)
        r.set_views([1], 3)
        dist, ids, bd = [t.cpu().numpy() for t in r.field(st_d, 1, torch.from_numpy(pts).to(DEV))]
        r.close()
        sc = rr.Scene(model, st_h[:, 1].astype(np.float64))
        best, bid, second = rr.scene_field(sc, pts.astype(np.float64))
        want_bd = rr.boundary_field(sc, pts.astype(np.float64))
        e1, e2 = float(np.abs(dist - best).max()), float(np.abs(bd - want_bd).max())
        clear = (second - best) > 1e-5
        bad = int((ids[clear] != bid[clear]).sum())
        print(f"field parity, {name}: dist err {e1:.3e}, boundary err {e2:.3e}, ids compared {int(clear.sum())} of {len(pts)}, mismatches {bad}; "
              f"ids seen {len(np.unique(bid))}")
        assert e1 <= 2e-6 and e2 <= 2e-6, (name, e1, e2)
        assert (~clear).mean() <= 0.01 and bad == 0, (name, float((~clear).mean()), bad)
        assert len(np.unique(bid)) >= 10                                  # the points see most of the bodies


# ---- 6. / 7. image parity ----------------------------------------------------------------------------------------------
def rollout_state(hip, n=4096, steps=50):
    cfg = make_config(hip, n, seed=11, episode_length=40, **dict(pu.CONFIGS["d4_torque_asym"]))
    eng = TrifingerEngine(cfg, device=DEV, lib=hip)
    eng.reset()
    for t in range(steps):
        eng.step(pu.actions_for(t, n, eng.action_dim, 11).to(DEV))
    st = eng.state.clone()
    eng.close()
    return cfg.model, st


def test_image_parity_flat(hip, render_mod):
    """shading mode 0 at 256 x 256: ids equal except for at most 0.05 % of the compared pixels, colour == palette[id] exactly, depth within 2 eps;
    the three seeded scenes and 8 envs of a 4096-env rollout after 50 random steps"""
    model = hip.default_model()
    st_h, st_d = seeded_scenes()
    r = render_mod.SceneRenderer(model, width=256, height=256, max_views=8, device=DEV, shading="flat")
    r.set_views([0, 1, 2], 3)
    out = {k: v.cpu().numpy() for k, v in r.render(st_d).items()}
    ghost_px = 0
    for v in range(3):
        ref = rr.render(rr.Scene(model, st_h[:, v].astype(np.float64)))
        ghost_px += compare_image(ref, out["color"][v], out["depth"][v], out["segmentation"][v], f"scene {v}")
    assert ghost_px > 300                                                 # the ghost was really checked
    # rollout views: the caps are asserted on the reference first; a view that breaks them is replaced by the next env id
    model, st = rollout_state(hip)
    st_h = st.cpu().numpy()
    ids, refs = [], []
    for cand in range(0, 4096, 512):
        while True:
            ref = rr.render(rr.Scene(model, st_h[:, cand].astype(np.float64)))
            a, b, _ = rr.excluded_shares(ref)
            if a <= CAP_ALL and b <= CAP_FG:
                break
            print(f"rollout env {cand}: excluded shares {a:.3f} / {b:.3f} above the caps, next env id")
            cand += 1
            assert cand % 512 != 0
        ids.append(cand); refs.append(ref)
    r.set_views(ids, 4096)
    out = {k: v.cpu().numpy() for k, v in r.render(st).items()}
    for v, (env, ref) in enumerate(zip(ids, refs)):
        compare_image(ref, out["color"][v], out["depth"][v], out["segmentation"][v], f"rollout env {env}")
    r.close()


def test_image_parity_lit(hip, render_mod):
    """shading mode 1, same pixels: per-channel difference to the fp64 reference at most 2.  The bound is twice what an fp32 numpy restatement
    (render_ref with dt = float32) differs from the fp64 one on the three scenes: 1 (one rounding step of the uint8 colour; shade itself differs by at
    most 1.2e-3), with 0 id mismatches and 9.0e-5 m in depth - the kernel orders its FMAs differently from numpy."""
    model = hip.default_model()
    st_h, st_d = seeded_scenes()
    r = render_mod.SceneRenderer(model, width=256, height=256, max_views=3, device=DEV, shading="lit")
    r.set_views([0, 1, 2], 3)
    out = {k: v.cpu().numpy() for k, v in r.render(st_d).items()}
    r.close()
    for v in range(3):
        ref = rr.render(rr.Scene(model, st_h[:, v].astype(np.float64)), shading=1)
        compare_image(ref, out["color"][v], out["depth"][v], out["segmentation"][v], f"lit scene {v}", shading_bound=2)


# ---- 8. it only looks --------------------------------------------------------------------------------------------------
def test_render_only_reads_and_is_deterministic(hip, render_mod):
    model, st = rollout_state(hip, n=4096, steps=10)
    before = st.clone()
    r = render_mod.SceneRenderer(model, width=128, height=128, max_views=16, device=DEV)
    r.set_views(list(range(0, 4096, 256)), 4096)
    a = {k: v.clone() for k, v in r.render(st).items()}
    b = r.render(st)
    torch.cuda.synchronize()
    assert torch.equal(st.view(torch.int32), before.view(torch.int32))
    for k in a:
        assert torch.equal(a[k].view(torch.uint8) if a[k].dtype == torch.uint8 else a[k].view(torch.int32),
                           b[k].view(torch.uint8) if b[k].dtype == torch.uint8 else b[k].view(torch.int32)), k
    with pytest.raises(ValueError):
        r.set_views([4096], 4096)
    with pytest.raises(ValueError):
        r.set_views(list(range(17)), 4096)
    with pytest.raises(ValueError):
        r.render(st[:, :100].contiguous())                      # not the state the views were checked against
    r.close()


def _env(n, visualize, render_cfg=None, **cfg):
    c = {"num_instances": n, "command_mode": "torque", "seed": 3}
    c.update(cfg)
    if render_cfg is not None:
        c["native"] = {"render": render_cfg}
    return TrifingerEnv(config=c, device=DEV, verbose=False, visualize=visualize)


def test_rollout_with_render_every_step_is_bit_identical(hip):
    finals = []
    for visualize in (False, True):
        env = _env(4096, visualize, {"width": 64, "height": 64} if visualize else None)
        env.reset()
        for t in range(200):
            env.step(pu.actions_for(t, 4096, 9, 3).to(DEV))
            frame = env.render()
            assert (frame is not None) == visualize
        finals.append({k: getattr(env._engine, k).clone() for k in ("state", "obs", "reward")})
        env.close()
    for k in ("state", "obs", "reward"):
        a, b = finals[0][k], finals[1][k]
        assert torch.equal(a.view(torch.int32), b.view(torch.int32)), k


# ---- 9. through the public API -------------------------------------------------------------------------------------------
def test_env_render_api(hip, tmp_path, render_mod):
    rec = str(tmp_path / "frames")
    env = _env(16, True, {"width": 96, "height": 64, "envs": [0, 5, 9], "record_dir": rec, "shading": "flat"})
    env.reset()
    frame = env.render()
    assert frame.dtype == torch.uint8 and tuple(frame.shape) == (3, 64, 96, 4) and frame.device.type == "cuda"
    bg = torch.tensor(list(render_mod.PALETTE[0]) + [255], dtype=torch.uint8, device=frame.device)
    assert int((frame != bg).any(-1).sum()) > 0.2 * 3 * 64 * 96
    first = frame.clone()
    vec = VecTaskPython(env, rl_device=DEV, clip_obs=5, clip_actions=1)
    for _ in range(4):
        vec.step(torch.zeros(16, 9, device=DEV))
    files = sorted(glob.glob(os.path.join(rec, "frame_*.png")))
    assert [os.path.basename(f) for f in files] == ["frame_%06d.png" % i for i in range(5)]       # the explicit call and one per step
    img = rr.decode_png(files[0])
    assert img.shape == (2 * 64, 2 * 96, 4)                              # 3 views -> a 2 x 2 mosaic
    assert np.array_equal(img[:64, :96], first[0].cpu().numpy())
    env.set_camera_lookat((0.2, -0.6, 0.4), (0.0, 0.0, 0.05))
    moved = env.render()
    assert not torch.equal(moved, first)
    with pytest.raises(ValueError):
        env._renderer.set_views([16], 16)
    env.close()
    assert env._renderer is None
    with pytest.raises(ValueError, match="native.render"):
        _env(16, True, {"envs": [16]})


def _run(args, env=None, timeout=600):
    e = dict(os.environ)
    e.update(env or {})
    p = subprocess.run([sys.executable] + args, cwd=REPO, env=e, capture_output=True, text=True, timeout=timeout)
    assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-2000:]
    return p.stdout


def test_scripts_leave_frames_behind(hip, tmp_path):
    rec = str(tmp_path / "rec")
    _run(["scripts/trifinger_random_action.py", "6", "--record", rec], timeout=300)
    assert len(glob.glob(os.path.join(rec, "frame_*.png"))) == 6
    base = ["scripts/rlg_hydra.py", "gym=trifinger_difficulty_4", "args.num_envs=512", f"args.logdir={tmp_path}/logs"]
    _run(base + ["args.headless=True"], env={"TF_MAX_EPOCHS": "1"}, timeout=600)
    run0 = glob.glob(f"{tmp_path}/logs/*")
    assert len(run0) == 1 and not os.path.isdir(os.path.join(run0[0], "frames"))       # headless runs stay what they are
    _run(base + ["args.headless=False", "args.play=True", f"args.checkpoint={run0[0]}/nn/trifinger.pth"], env={"TF_PLAY_STEPS": "5"}, timeout=600)
    runs = [d for d in glob.glob(f"{tmp_path}/logs/*") if d != run0[0]]
    assert len(runs) == 1 and len(glob.glob(os.path.join(runs[0], "frames", "frame_*.png"))) >= 5
