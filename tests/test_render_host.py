"""Host side of the renderer of the collision model (include/trifinger_render.h, leibnizgym_amd/render.py) and the conditions the GPU tests
(tests/test_render_gpu.py) rely on, checked on the fp64 reference alone (tests/render_ref.py).  No GPU needed."""
import ctypes as C
import os
import re
import subprocess
import sys
import tempfile

import numpy as np
import pytest
import torch

import render_ref as rr
from leibnizgym_amd import _capi as capi
from leibnizgym_amd.engine import TrifingerEngine, make_config
from leibnizgym_amd.envs import TrifingerEnv
from oracle_util import REPO

HEADER = os.path.join(REPO, "include", "trifinger_render.h")


def render_lib():
    from leibnizgym_amd import render
    path = render.library_path()
    if not os.path.isfile(path):
        subprocess.check_call(["make", "-C", os.path.dirname(path), "-s", "libtrifinger_render.so"])
    return render, render.load()


# ---- 1. header <-> library <-> binding -------------------------------------------------------------------------------
def test_header_library_and_binding_agree():
    render, lib = render_lib()                               # loads without a GPU
    src = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    names = sorted(set(re.findall(r"\b(tfr_[a-z0-9_]+)\s*\(", src)))
    assert len(names) >= 8 and sorted(render.SYMBOLS) == names, set(names) ^ set(render.SYMBOLS)
    for n in names:
        assert hasattr(lib, n), n
    assert lib.tfr_api_version() == render.TFR_API_VERSION == int(re.search(r"#define TFR_API_VERSION (\d+)", src).group(1))
    assert render.TFR_MAX_VIEWS == int(re.search(r"#define TFR_MAX_VIEWS (\d+)", src).group(1))
    ids = re.search(r"enum \{ (TFR_ID_BACKGROUND[^}]*) \};", src).group(1)
    vals = {k.strip().split(" = ")[0]: int(k.strip().split(" = ")[1]) for k in ids.split(",")}
    assert vals == dict(TFR_ID_BACKGROUND=render.ID_BACKGROUND, TFR_ID_OBJECT=render.ID_OBJECT, TFR_ID_FLOOR=render.ID_FLOOR,
                        TFR_ID_BOUNDARY=render.ID_BOUNDARY, TFR_NUM_IDS=render.NUM_IDS)
    assert [tuple(int(v) for v in row) for row in rr.PALETTE] == render.PALETTE and tuple(int(v) for v in rr.GHOST) == render.GHOST


def test_struct_sizes_match_the_c_compiler():
    render, _ = render_lib()
    prog = r'''
#include <stdio.h>
#include <stddef.h>
#include "trifinger_render.h"
int main(void) { printf("%zu %zu %zu %zu\n", sizeof(TfrConfig), sizeof(TfModel), offsetof(TfrConfig, eps), offsetof(TfrConfig, t_max)); return 0; }'''
    with tempfile.TemporaryDirectory() as d:
        src, exe = os.path.join(d, "s.c"), os.path.join(d, "s")
        open(src, "w").write(prog)
        subprocess.check_call(["gcc", "-I", os.path.join(REPO, "include"), "-o", exe, src])
        sizes = [int(x) for x in subprocess.check_output([exe]).decode().split()]
    assert sizes == [C.sizeof(render.TfrConfig), C.sizeof(capi.TfModel), render.TfrConfig.eps.offset, render.TfrConfig.t_max.offset]


def test_host_entry_points_validate_without_a_gpu(oracle):
    """tfr_create / tfr_set_camera / tfr_set_views are host code: defaults, refusals and the id check run here"""
    render, lib = render_lib()
    cfg = render.TfrConfig()
    lib.tfr_default_config(C.byref(cfg))
    assert (cfg.width, cfg.height, cfg.max_views, cfg.max_steps, cfg.shading) == (256, 256, 16, 160, 1)
    assert (cfg.eps, cfg.relax, cfg.t_max) == (np.float32(1e-4), np.float32(0.9), 2.0)
    m, h = oracle.default_model(), C.c_void_p()
    for field, bad in (("width", 0), ("height", 5000), ("max_views", 65), ("max_steps", 0), ("shading", 2), ("relax", 1.5), ("eps", 0.0),
                       ("api_version", 7)):
        c2 = render.TfrConfig.from_buffer_copy(cfg)
        setattr(c2, field, bad)
        assert lib.tfr_create(C.byref(m), C.byref(c2), C.byref(h)) == capi.TF_ERR_INVALID_ARG, field
    assert lib.tfr_create(C.byref(m), C.byref(cfg), C.byref(h)) == 0
    ids = (C.c_int32 * 4)(0, 3, 7, 2)
    assert lib.tfr_render(h, C.c_void_p(8), C.c_void_p(8), None, None, None) == capi.TF_ERR_NOT_BOUND
    assert lib.tfr_set_views(h, ids, 4, 8) == 0
    assert lib.tfr_set_views(h, ids, 4, 7) == capi.TF_ERR_INVALID_ARG                 # id 7 >= num_envs 7
    assert b"env id" in lib.tfr_last_error_string()
    assert lib.tfr_set_views(h, (C.c_int32 * 1)(-1), 1, 8) == capi.TF_ERR_INVALID_ARG
    assert lib.tfr_set_views(h, (C.c_int32 * 17)(), 17, 8) == capi.TF_ERR_INVALID_ARG   # above max_views
    assert lib.tfr_set_views(h, ids, 0, 8) == capi.TF_ERR_INVALID_ARG
    f3 = lambda *v: (C.c_float * 3)(*v)      # noqa: E731
    assert lib.tfr_set_camera(h, f3(0.5, 0.3, 0.5), f3(0, 0, 0.1), 0.8) == 0
    assert lib.tfr_set_camera(h, f3(0, 0, 0.5), f3(0, 0, 0.1), 0.8) == capi.TF_ERR_INVALID_ARG      # straight down: no up vector
    assert lib.tfr_set_camera(h, f3(0.5, 0.3, 0.5), f3(0.5, 0.3, 0.5), 0.8) == capi.TF_ERR_INVALID_ARG
    assert lib.tfr_set_camera(h, f3(0.5, 0.3, 0.5), f3(0, 0, 0.1), 0.0) == capi.TF_ERR_INVALID_ARG
    assert lib.tfr_render(h, None, None, None, None, None) == capi.TF_ERR_INVALID_ARG
    assert lib.tfr_test_field(h, C.c_void_p(8), 8, C.c_void_p(8), None, None, None, 4, None) == capi.TF_ERR_INVALID_ARG   # env 8 of 8
    assert lib.tfr_destroy(h) == 0
    with pytest.raises(RuntimeError, match="no CPU path"):
        render.SceneRenderer(m, device="cpu")


# ---- 2. the reference's kinematics are the step's; known answers of the picture --------------------------------------
@pytest.mark.parametrize("cfg_name", ["d4_torque_asym", "d4_domain_randomization_extended"])
def test_reference_kinematics_are_the_steps(oracle, cfg_name):
    """tip_origin through the reference's link-3 frame == the TF_S_TIP_P rows the step wrote (world positions, base offset included)"""
    import parity_util as pu
    kw = dict(pu.CONFIGS[cfg_name])
    cfg = make_config(oracle, 16, seed=5, episode_length=40, **kw)
    eng = TrifingerEngine(cfg, device="cpu", lib=oracle)
    eng.reset()
    for t in range(6):
        eng.step(pu.actions_for(t, 16, eng.action_dim, 5))
    st = eng.state.numpy().astype(np.float64)
    ext = cfg_name.endswith("extended")
    off = st[capi.S_DR + capi.DR_BASE_POS:capi.S_DR + capi.DR_BASE_POS + 3]
    assert (np.abs(off).max() > 1e-3) == ext                      # the offsets are really there in the extended case
    for env in range(16):
        sc = rr.Scene(cfg.model, st[:, env])
        for f in range(3):
            np.testing.assert_allclose(sc.tip_world(f), st[capi.S_TIP_P + 3 * f:capi.S_TIP_P + 3 * f + 3, env], rtol=0, atol=2e-6)
    eng.close()


def _march_one(sc, eye, d, **kw):
    d = np.asarray(d, np.float64)
    t, hit, unres, _ = rr.march(sc, np.asarray(eye, np.float64), (d / np.linalg.norm(d))[None], **kw)
    return float(t[0]), int(hit[0]), bool(unres[0])


def test_known_answers_of_the_picture(oracle):
    m = oracle.default_model()
    sc = rr.Scene(m, rr.seeded_state(0))
    # straight down onto the resting cube: the top face, z = 2 x half extent
    t, hit, _ = _march_one(sc, (0.0, 0.0, 0.5), (0, 0, -1))
    assert hit == rr.ID_OBJECT and abs((0.5 - t) - 2 * m.cube_half) <= 1e-4 + 1e-9
    # along a fingertip's axis, from beyond the tip: cap_radius in front of the sphere centre
    for f in range(3):
        R3, p3 = sc.frames[f][2]
        a, b = p3 + R3 @ np.array(m.cap_a[:]), p3 + R3 @ sc.cap_b
        ax = (b - a) / np.linalg.norm(b - a)
        eye = b + 0.05 * ax
        t, hit, _ = _march_one(sc, eye, -ax)
        assert hit == 1 + 6 * f + 2, hit
        assert abs((0.05 - t) - m.cap_radius) <= 1e-4 + 1e-9
    # from outside through the near wall: the far inner wall or the floor, never the near side
    for az in np.linspace(0, 2 * np.pi, 12, endpoint=False):
        eye = np.array([0.6 * np.cos(az), 0.6 * np.sin(az), 0.12])
        for target_z in (0.02, 0.05, 0.10):
            d = np.array([0, 0, target_z]) - eye
            t, hit, _ = _march_one(sc, eye, d)
            assert hit != 0
            p = eye + t * d / np.linalg.norm(d)
            assert p @ eye < 0 or hit != rr.ID_BOUNDARY, (az, target_z, hit, p)      # a boundary hit lies beyond the stage axis
    # a ray that crosses z = 0 outside the disc is background
    t, hit, unres = _march_one(sc, (0.6, 0.0, 0.3), (0.2, 0, -1))
    assert hit == 0 and not unres
    # ids tie to the lower one and the box distance is exact and signed
    best, bid, second = rr.scene_field(sc, np.array([[0.0, 0.0, m.cube_half], [0.0, 0.0, 2 * m.cube_half + 0.01]]))
    # (the cube of the seeded state rests at 0.0325; cube_half is that number in fp32)
    assert bid.tolist() == [20, 20] and abs(best[0] + m.cube_half) < 1e-8 and abs(best[1] - 0.01) < 1e-8 and np.all(second > best)


# ---- 3. the conditions the GPU image test relies on ------------------------------------------------------------------
@pytest.mark.parametrize("case", [0, 1, 2])
def test_excluded_pixel_shares_of_the_reference(oracle, case):
    """edge or unresolved pixels at 256 x 256 from the default camera: at most 15 % of all pixels, at most 25 % of the robot and object pixels"""
    img = rr.render(rr.Scene(oracle.default_model(), rr.seeded_state(case)))
    share_all, share_fg, _ = rr.excluded_shares(img)
    fg = float(((img["seg"] >= 1) & (img["seg"] <= 20)).mean())
    print(f"case {case}: excluded {share_all:.4f} of all, {share_fg:.4f} of robot+object pixels; robot+object cover {fg:.3f}; "
          f"unresolved {int(img['unresolved'].sum())}; ghost pixels {int(img['ghost'].sum())}")
    assert share_all <= 0.15 and share_fg <= 0.25
    assert fg > 0.1 and img["unresolved"].mean() < 1e-3
    assert img["ghost"].sum() > 100 and (img["seg"] == rr.ID_BOUNDARY).sum() > 1000 and (img["seg"] == rr.ID_FLOOR).sum() > 1000


# ---- 4. env API on the injected library; PNG writer -------------------------------------------------------------------
def _env(oracle, visualize, native=None):
    cfg = {"num_instances": 4, "command_mode": "torque"}
    if native is not None:
        cfg["native"] = native
    return TrifingerEnv(config=cfg, device="cpu", verbose=False, visualize=visualize, lib=oracle)


def test_visualize_on_the_cpu_library_warns_and_returns_none(oracle, capsys):
    env = _env(oracle, True, {"render": {"width": 64, "height": 48, "envs": [1, 3]}})
    env.reset()
    assert env.render() is None
    assert "headless" in capsys.readouterr().out
    env.set_camera_lookat((1, 1, 1), (0, 0, 0))                    # accepted, nothing to move
    env.close()
    env = _env(oracle, False)
    assert env.render() is None and capsys.readouterr().out == ""
    env.close()


@pytest.mark.parametrize("bad", [{"width": 0}, {"height": "tall"}, {"envs": [4]}, {"envs": []}, {"envs": [-1]}, {"fov_deg": 0}, {"fov_deg": 180},
                                 {"shading": "phong"}, {"record_dir": 3}, {"colour": 1}, ["not a mapping"]])
def test_bad_render_config_raises(oracle, bad):
    with pytest.raises(ValueError, match="native.render"):
        _env(oracle, True, {"render": bad})
    _env(oracle, False, {"render": bad}).close()                  # not looked at without visualize


def test_render_config_defaults():
    from leibnizgym_amd import render
    rc = render.parse_render_config(None, 8192)
    assert rc == dict(width=256, height=256, envs=[0, 1, 2, 3], fov_deg=45.0, shading="lit", record_dir=None)
    assert render.parse_render_config({}, 2)["envs"] == [0, 1]
    assert (render.DEFAULT_EYE, render.DEFAULT_TARGET) == (rr.DEFAULT_CAMERA["eye"], rr.DEFAULT_CAMERA["target"])


def test_visualize_false_never_imports_the_render_module():
    code = ("import sys; sys.path.insert(0, %r); sys.path.insert(0, %r)\n"
            "from oracle_util import load_oracle\n"
            "from leibnizgym_amd.envs import TrifingerEnv\n"
            "import torch\n"
            "env = TrifingerEnv(config={'num_instances': 4}, device='cpu', verbose=False, visualize=False, lib=load_oracle())\n"
            "env.reset(); env.step(torch.zeros(4, 9)); env.render(); env.close()\n"
            "assert 'leibnizgym_amd.render' not in sys.modules\n"
            "env = TrifingerEnv(config={'num_instances': 4}, device='cpu', verbose=False, visualize=True, lib=load_oracle())\n"
            "assert 'leibnizgym_amd.render' in sys.modules\n") % (REPO, os.path.join(REPO, "tests"))
    subprocess.check_call([sys.executable, "-c", code], timeout=300)


def test_png_writer_round_trip_and_mosaic(oracle, tmp_path):
    from leibnizgym_amd import render
    rng = np.random.default_rng(0)
    views = rng.integers(0, 256, (5, 12, 20, 4), dtype=np.uint8)
    mos = render.mosaic(torch.from_numpy(views))
    assert tuple(mos.shape) == (2 * 12, 3 * 20, 4)                 # 5 views -> 3 columns x 2 rows
    assert torch.equal(mos[12:24, 20:40], torch.from_numpy(views[4])) and int(mos[12:24, 40:60].sum()) == 0
    assert np.array_equal(render.mosaic(views), mos.numpy())
    path = str(tmp_path / "sub" / "m.png")
    render.write_png(path, mos)
    assert np.array_equal(rr.decode_png(path), mos.numpy())
    render.write_png(path, views[0][:, :, :3].copy())
    assert np.array_equal(rr.decode_png(path), views[0][:, :, :3])
    with pytest.raises(ValueError):
        render.write_png(path, views.astype(np.float32)[0])
    # a reference-rendered frame goes through the same path
    img = rr.render(rr.Scene(oracle.default_model(), rr.seeded_state(1)), W=64, H=64, shading=1)
    render.write_png(path, img["color"])
    assert np.array_equal(rr.decode_png(path), img["color"])
