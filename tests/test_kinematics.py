"""Fingertip-space control on the CPU (include/trifinger_kin.h, leibnizgym_amd/kinematics.py, leibnizgym_amd/wrappers/fingertip_action.py): the header, the
library and the binding agree; the torch statements of the three laws against the independent fp64 URDF model of tests/test_physics_analytic.py; the
conditions the GPU tests (tests/test_kinematics_gpu.py) rely on, checked on the statements alone; the wrapper on the CPU oracle engine.  No GPU needed."""
import ctypes as C
import importlib.util
import os
import re

import numpy as np
import pytest
import torch

import kin_util as ku
import test_physics_analytic as pa
from leibnizgym_amd import _capi as capi
from leibnizgym_amd import kinematics as kin
from leibnizgym_amd.envs import TrifingerEnv
from leibnizgym_amd.wrappers import VecTaskPython
from leibnizgym_amd.wrappers.fingertip_action import FingertipActionEnv
from model_fixture import H_BASE, YAW
from oracle_util import REPO

HEADER = os.path.join(REPO, "include", "trifinger_kin.h")


def _header():
    return re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)


def _declarations():
    return {name: (0 if params.strip() in ("", "void") else params.count(",") + 1)
            for name, params in re.findall(r"\b(tfk_[a-z0-9_]+)\s*\(([^()]*)\)\s*;", _header())}


@pytest.fixture(scope="module")
def mc(oracle):
    return kin.model_constants(oracle.default_model())


# ---- 1. header <-> library <-> binding -------------------------------------------------------------------------------------------------------------------
def test_header_library_and_binding_agree():
    lib = ku.kin_lib()                                       # loads without a GPU
    decls = _declarations()
    assert len(decls) >= 7 and decls["tfk_api_version"] == 0 and decls["tfk_forward"] == 9 and decls["tfk_inverse"] == 9 and decls["tfk_tip_action"] == 10, decls
    assert sorted(decls) == sorted(kin.SYMBOLS), set(decls) ^ set(kin.SYMBOLS)
    raw = C.CDLL(kin.library_path())
    for name, count in sorted(decls.items()):
        assert hasattr(raw, name), f"{name} is declared but not exported"
        fn = getattr(lib, name)
        assert fn.argtypes is not None and len(fn.argtypes) == count, f"{name}: {len(fn.argtypes or [])} argument types bound, {count} parameters declared"
    src = _header()
    assert lib.tfk_api_version() == kin.TFK_API_VERSION == int(re.search(r"#define TFK_API_VERSION (\d+)", src).group(1))
    assert kin.TFK_MAX_IK_ITERS == int(re.search(r"#define TFK_MAX_IK_ITERS (\d+)", src).group(1))
    assert kin.TFK_MAX_ACTION_ITERS == int(re.search(r"#define TFK_MAX_ACTION_ITERS (\d+)", src).group(1))
    assert kin.TF_MAX_ENVS == int(re.search(r"#define TF_MAX_ENVS (\d+)", open(os.path.join(REPO, "include", "trifinger.h")).read()).group(1))


def test_struct_sizes_match_the_c_compiler(tmp_path):
    import subprocess
    prog = r'''
#include <stdio.h>
#include <stddef.h>
#include "trifinger_kin.h"
int main(void) { printf("%zu %zu %zu %zu %zu %zu\n", sizeof(TfkArray), sizeof(TfkIkParams), sizeof(TfkActionParams), offsetof(TfkActionParams, box_lo),
                        offsetof(TfkActionParams, kp), offsetof(TfkActionParams, gravity)); return 0; }'''
    src, exe = tmp_path / "s.c", tmp_path / "s"
    src.write_text(prog)
    subprocess.check_call(["gcc", "-I", os.path.join(REPO, "include"), "-o", str(exe), str(src)])
    sizes = [int(x) for x in subprocess.check_output([str(exe)]).decode().split()]
    assert sizes == [C.sizeof(kin.TfkArray), C.sizeof(kin.TfkIkParams), C.sizeof(kin.TfkActionParams), kin.TfkActionParams.box_lo.offset,
                     kin.TfkActionParams.kp.offset, kin.TfkActionParams.gravity.offset]


def test_no_symbol_of_another_library_is_declared():
    """the prefixes tf_, tfp_ and tfr_ belong to the step, the trainer and the renderer, and to the table of tests/test_guard_bands_gpu.py"""
    found = re.findall(r"\b(tf[pr]?_[a-z0-9_]+)\s*\(", _header())
    assert not found, found
    import test_guard_bands as tgb
    assert not [n for n in tgb.stream_entry_points() if n.startswith("tfk")]


def test_create_validates_on_the_host(oracle):
    lib = ku.kin_lib()
    h = C.c_void_p()
    assert lib.tfk_create(None, C.byref(h)) == kin.TFK_ERR_INVALID_ARG
    for edit in (lambda m: setattr(m, "base_height", float("nan")), lambda m: m.q_lo.__setitem__(1, 2.0), lambda m: setattr(m, "tau_max", 0.0),
                 lambda m: m.link_inertia[2].__setitem__(4, float("inf")), lambda m: m.tip_origin.__setitem__(0, float("nan"))):
        m = oracle.default_model()
        edit(m)
        assert lib.tfk_create(C.byref(m), C.byref(h)) == kin.TFK_ERR_INVALID_ARG
        assert lib.tfk_last_error_string().startswith(b"tfk_create")
    m = oracle.default_model()
    assert lib.tfk_create(C.byref(m), C.byref(h)) == 0
    # refusals happen before any launch: they run here, with pointers nothing dereferences
    arr = kin.TfkArray(8, 9, 1)
    ok = kin.TfkIkParams(4, 0.02, 0.5)
    for bad in (kin.TfkIkParams(0, 0.02, 0.5), kin.TfkIkParams(65, 0.02, 0.5), kin.TfkIkParams(4, 0.0, 0.5), kin.TfkIkParams(4, 0.02, -1.0),
                kin.TfkIkParams(4, float("nan"), 0.5)):
        assert lib.tfk_inverse(h, arr, arr, kin.NO_ARRAY, C.byref(bad), 8, 8, 4, None) == kin.TFK_ERR_INVALID_ARG
    assert lib.tfk_inverse(h, arr, arr, kin.NO_ARRAY, C.byref(ok), 8, 8, 0, None) == kin.TFK_ERR_INVALID_ARG
    assert lib.tfk_inverse(h, arr, arr, kin.NO_ARRAY, C.byref(ok), 8, 8, kin.TF_MAX_ENVS + 1, None) == kin.TFK_ERR_INVALID_ARG
    assert lib.tfk_inverse(h, kin.NO_ARRAY, arr, kin.NO_ARRAY, C.byref(ok), 8, 8, 4, None) == kin.TFK_ERR_INVALID_ARG
    assert lib.tfk_inverse(h, kin.TfkArray(8, -1, 1), arr, kin.NO_ARRAY, C.byref(ok), 8, 8, 4, None) == kin.TFK_ERR_INVALID_ARG
    assert lib.tfk_forward(h, arr, kin.NO_ARRAY, kin.NO_ARRAY, 8, 8, None, 4, None) == kin.TFK_ERR_INVALID_ARG      # tip_v without qd
    assert lib.tfk_forward(h, arr, kin.NO_ARRAY, kin.NO_ARRAY, None, None, None, 4, None) == kin.TFK_ERR_INVALID_ARG
    p, _ = kin.action_params("delta", "torque", True)
    assert lib.tfk_tip_action(h, C.byref(p), arr, arr, kin.NO_ARRAY, kin.NO_ARRAY, 8, None, 4, None) == kin.TFK_ERR_INVALID_ARG   # torque mode without qd
    p.mode = 2
    assert lib.tfk_tip_action(h, C.byref(p), arr, arr, arr, kin.NO_ARRAY, 8, None, 4, None) == kin.TFK_ERR_INVALID_ARG
    p, _ = kin.action_params("delta", "position", True)
    p.iters = 9
    assert lib.tfk_tip_action(h, C.byref(p), arr, arr, arr, kin.NO_ARRAY, 8, None, 4, None) == kin.TFK_ERR_INVALID_ARG
    assert lib.tfk_destroy(h) == 0


def test_binding_validates_by_name():
    for kw, word in ((dict(iters=0), "iters"), (dict(damping=0.0), "damping"), (dict(box_lo=(0.2, 0, 0)), "box_lo"), (dict(kp=(1, -1, 1)), "kp"),
                     (dict(stiffness=3), "stiffness")):
        with pytest.raises(ValueError, match=word):
            kin.action_params("delta", "position", True, **kw)
    with pytest.raises(ValueError, match="frame"):
        kin.action_params("relative", "position", True)
    dev = torch.device("cpu")
    good = torch.zeros(5, 9)
    assert kin.array_of(good.T.contiguous().T, "q", 9, 5, dev).env_stride == 1
    for t, word in ((good.double(), "float32"), (torch.zeros(5, 8), "shape"), (torch.zeros(9), "shape"), ([0.0] * 9, "torch tensor")):
        with pytest.raises(ValueError, match=word):
            kin.array_of(t, "q", 9, 5, dev)
    with pytest.raises(ValueError, match="lives on"):
        kin.array_of(good, "q", 9, 5, torch.device("cuda:0"))
    with pytest.raises(RuntimeError, match="cuda"):
        kin.FingerKinematics(device="cpu")


# ---- 2. the statements against the independent model ---------------------------------------------------------------------------------------------------
def _rz(a):
    c, s = np.cos(a), np.sin(a)
    return np.array([[c, -s, 0.0], [s, c, 0.0], [0.0, 0.0, 1.0]])


N_DRAWS = 500
# the statement reads the model's float32 constants, the independent model the fixture's doubles: they differ by 6e-8 relative on lengths below 0.17 m
# and on the yaw's sine and cosine, 3e-8 m on a position of the 0.34 m chain; central differences at 1e-6 add 1e-9 to a Jacobian entry
FP64_TOL = 1e-7


def test_forward_statement_matches_the_independent_model(mc):
    q = ku.uniform_joints(mc, N_DRAWS, 0)
    qd = torch.tensor(np.random.default_rng(1).uniform(-3, 3, (N_DRAWS, 9)))
    off = torch.tensor(np.random.default_rng(2).uniform(-0.01, 0.01, (N_DRAWS, 3)))
    tip_p, tip_v, jac = kin.forward_statement(mc, q, qd, off)
    assert tip_p.shape == (N_DRAWS, 9) and tip_v.shape == (N_DRAWS, 9) and jac.shape == (N_DRAWS, 3, 3, 3) and tip_p.dtype == torch.float64
    qn = q.numpy()
    for f in range(3):
        R = _rz(YAW[f])
        for i in range(N_DRAWS):
            qf = qn[i, 3 * f:3 * f + 3]
            want = R @ pa.tip_position(qf) + np.array([0.0, 0.0, H_BASE]) + off[i].numpy()
            np.testing.assert_allclose(tip_p[i, 3 * f:3 * f + 3].numpy(), want, atol=FP64_TOL, rtol=0)
            J = R @ np.stack([(pa.tip_position(qf + d) - pa.tip_position(qf - d)) / 2e-6 for d in np.eye(3) * 1e-6], axis=1)
            np.testing.assert_allclose(jac[i, f].numpy(), J, atol=FP64_TOL, rtol=0)
            np.testing.assert_allclose(tip_v[i, 3 * f:3 * f + 3].numpy(), J @ qd[i, 3 * f:3 * f + 3].numpy(), atol=10 * FP64_TOL, rtol=0)
    none = kin.forward_statement(mc, q)
    assert none[1] is None and torch.allclose(none[0].reshape(-1, 3, 3) + off[:, None, :], tip_p.reshape(-1, 3, 3), atol=1e-15, rtol=0)


def test_the_120_degree_turn_maps_a_finger_onto_the_next(mc):
    q3 = ku.uniform_joints(mc, N_DRAWS, 3)[:, :3]
    tip_p, tip_v, jac = kin.forward_statement(mc, q3.repeat(1, 3), q3.repeat(1, 3) * 0.7)
    lift = torch.tensor([0.0, 0.0, mc["H"]], dtype=torch.float64)
    for f in range(3):
        g = (f + 1) % 3
        R = torch.tensor(_rz(YAW[g] - YAW[f]))
        assert torch.allclose((tip_p[:, 3 * f:3 * f + 3] - lift) @ R.T, tip_p[:, 3 * g:3 * g + 3] - lift, atol=FP64_TOL, rtol=0)
        assert torch.allclose(tip_v[:, 3 * f:3 * f + 3] @ R.T, tip_v[:, 3 * g:3 * g + 3], atol=FP64_TOL, rtol=0)
        assert torch.allclose(torch.einsum("rs,nsc->nrc", R, jac[:, f]), jac[:, g], atol=FP64_TOL, rtol=0)


def test_gravity_term_matches_the_potential_of_the_independent_model(mc):
    """figures of tests/test_physics_analytic.py::_check_dynamics_leaf for the bias at rest: atol 3e-6, rtol 2e-4"""
    q = ku.uniform_joints(mc, 100, 4)[:, :3]
    g = torch.stack(kin.gravity_torque(mc, tuple(q[:, j] for j in range(3)), (0.0, 0.0, -pa.G)), dim=1).numpy()
    for i in range(100):
        qi = q[i].numpy()
        grad = np.array([(pa.potential(qi + d) - pa.potential(qi - d)) / 2e-6 for d in np.eye(3) * 1e-6])
        np.testing.assert_allclose(g[i], grad, atol=3e-6, rtol=2e-4)
    # ... and as the torque law adds it: zero gains, so the action is g alone, in every finger's base frame
    _, d = kin.action_params("delta", "torque", False, kp=(0, 0, 0), kd=(0, 0, 0), gravity=(0.0, 0.0, -pa.G))
    a, _ = kin.tip_action_statement(mc, d, torch.zeros(100, 9, dtype=torch.float64), q.repeat(1, 3), torch.zeros(100, 9, dtype=torch.float64))
    for f in range(3):
        np.testing.assert_allclose(a[:, 3 * f:3 * f + 3].numpy(), np.clip(g, -mc["tau_max"], mc["tau_max"]), atol=1e-12)


# ---- 3. the inverse statement: the condition the GPU test relies on -----------------------------------------------------------------------------------
@pytest.mark.parametrize("seed", (11,))
def test_inverse_statement_converges_inside_the_limits(mc, seed):
    n = 400
    target, q0 = ku.ik_case(mc, n, seed)
    q, res = kin.inverse_statement(mc, target, q0, None, **ku.IK)
    share = float((res > ku.IK_CONVERGED).double().mean())
    print(f"fingers left above {ku.IK_CONVERGED} m: {share:.4f}; largest residual {float(res.max()):.3e} m")
    assert share <= 0.05
    lo, hi = torch.tensor(mc["q_lo"] * 3, dtype=torch.float64), torch.tensor(mc["q_hi"] * 3, dtype=torch.float64)
    assert bool((q >= lo).all()) and bool((q <= hi).all())
    # a target outside the workspace: finite, on a limit
    far = torch.tensor([[0.5, 0.5, 0.5, 0.5, -0.5, 0.5, -0.5, -0.5, 0.5]], dtype=torch.float64)
    q, res = kin.inverse_statement(mc, far, q0[:1], None, **ku.IK)
    assert bool(torch.isfinite(q).all()) and bool((q >= lo).all()) and bool((q <= hi).all()) and bool((res > 0.3).all())
    assert all(bool(((q[0, 3 * f:3 * f + 3] == lo[:3]) | (q[0, 3 * f:3 * f + 3] == hi[:3])).any()) for f in range(3))
    # a damping far below what float32 resolves: the floor of the determinant (lambda^6, its exact lower bound) keeps the float32 statement finite
    q32, res32 = kin.inverse_statement(mc, far.float(), q0[:1].float(), None, iters=32, damping=1e-6, step_max=0.5)
    assert bool(torch.isfinite(q32).all()) and bool(torch.isfinite(res32).all())


def test_tip_action_statement_targets(mc):
    """the target law by hand: commands beyond +-1 are clamped, absolute commands span the box, every target lies in the finger's own box"""
    _, d = kin.action_params("absolute", "position", True)
    n = 64
    cmd = torch.tensor(np.random.default_rng(5).uniform(-1.5, 1.5, (n, 9)))
    q = ku.uniform_joints(mc, n, 6)
    a, t = kin.tip_action_statement(mc, d, cmd, q)
    a2, t2 = kin.tip_action_statement(mc, d, cmd.clamp(-1, 1), q)
    assert torch.equal(a, a2) and torch.equal(t, t2) and bool((a.abs() <= 1.0).all())
    lo, hi = np.array(d["box_lo"]), np.array(d["box_hi"])
    for f in range(3):
        u = t[:, 3 * f:3 * f + 3].numpy() @ _rz(YAW[f] - YAW[0])          # row vectors: u = R^T x
        want = lo + (np.clip(cmd[:, 3 * f:3 * f + 3].numpy(), -1, 1) + 1) / 2 * (hi - lo)
        np.testing.assert_allclose(u, want, atol=1e-7)
    _, d = kin.action_params("delta", "position", False, delta_scale=0.05)
    a, t = kin.tip_action_statement(mc, d, cmd, q)
    x, _, _ = kin.forward_statement(mc, q)
    for f in range(3):
        u = t[:, 3 * f:3 * f + 3].numpy() @ _rz(YAW[f] - YAW[0])
        assert (u >= lo - 1e-7).all() and (u <= hi + 1e-7).all()          # (the library's relative yaws are float32, this frame is exact)
        ux = (x[:, 3 * f:3 * f + 3] + 0.05 * cmd[:, 3 * f:3 * f + 3].clamp(-1, 1)).numpy() @ _rz(YAW[f] - YAW[0])
        np.testing.assert_allclose(u, np.clip(ux, lo, hi), atol=1e-7)
    qlo, qhi = torch.tensor(mc["q_lo"] * 3, dtype=torch.float64), torch.tensor(mc["q_hi"] * 3, dtype=torch.float64)
    assert bool((a >= qlo).all()) and bool((a <= qhi).all())                # not normalised: joint targets inside the limits


# ---- 4. the wrapper on the CPU oracle engine ------------------------------------------------------------------------------------------------------------
def _env(oracle, n=16, **cfg):
    base = dict(ku.LOOP_ENV, num_instances=n)
    base.update(cfg)
    return TrifingerEnv(config=base, device="cpu", verbose=False, lib=oracle)


@pytest.mark.parametrize("vec", (False, True), ids=("TrifingerEnv", "VecTaskPython"))
def test_wrapper_reaches_absolute_targets_on_the_oracle(oracle, vec):
    n = 16
    env = _env(oracle, n)
    w = FingertipActionEnv(VecTaskPython(env, rl_device="cpu") if vec else env, frame="absolute", fused=False)
    assert w.mode == "position" and w.fused is False
    assert (w.num_actions if vec else w.get_action_dim()) == 9                            # the inner env's interface, action width 9
    cmd = ku.loop_command(n, w.params)
    e0, e1 = ku.run_loop(w, cmd)
    z = w.last_target[:, 2::3]
    assert float(z.min()) >= 0.15 and float(e0.min()) > ku.LOOP_START
    ratio = e1 / e0
    print(f"initial tip error {float(e0.min()):.4f} .. {float(e0.max()):.4f} m, final {float(e1.max()):.4f} m, largest ratio {float(ratio.max()):.4f}")
    assert bool((ratio < ku.LOOP_BAR).all()), ratio
    out = w.step(cmd)
    assert len(out) == 4 and out[0].shape[0] == n                                        # the inner env's step, untouched


def test_wrapper_refusals(oracle):
    with pytest.raises(ValueError, match="no native engine"):
        FingertipActionEnv(object())
    with pytest.raises(ValueError, match="position_impedance"):
        FingertipActionEnv(_env(oracle, 2, command_mode="position_impedance"), fused=False)
    with pytest.raises(ValueError, match="normalize_action"):
        FingertipActionEnv(_env(oracle, 2), fused=False, normalize_action=False)
    with pytest.raises(ValueError, match="normalize_action"):
        FingertipActionEnv(_env(oracle, 2, normalize_action=False), fused=False, normalize_action=True)
    with pytest.raises(ValueError, match="command_mode"):
        FingertipActionEnv(_env(oracle, 2), fused=False, mode="torque")
    with pytest.raises(ValueError, match="fused=True"):
        FingertipActionEnv(_env(oracle, 2), fused=True)
    w = FingertipActionEnv(_env(oracle, 2, command_mode="torque"), frame="delta", normalize_action=True)
    assert w.mode == "torque" and w.fused is False and w.params["gravity"] == (0.0, 0.0, np.float32(-9.81))
    with pytest.raises(ValueError, match="Invalid shape"):
        w.step(torch.zeros(2, 18))
    for bad in (torch.zeros(2, 9, dtype=torch.float64), [[0.0] * 9] * 2):                 # read where it is: nothing is converted or copied
        with pytest.raises(ValueError, match="cmd"):
            w.step(bad)


def _train_script():
    spec = importlib.util.spec_from_file_location("train_ppo_script", os.path.join(REPO, "scripts", "train_ppo.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_train_script_refuses_fingertip_actions_with_symmetry():
    tp = _train_script()
    assert tp.parse_args(["gym=trifinger_difficulty_4", "epochs=3"]) == (3, None, None, ["gym=trifinger_difficulty_4"])        # off by default
    assert tp.parse_args(["--fingertip-actions", "delta", "epochs=2"])[2] == "delta" and tp.parse_args(["--fingertip-actions=absolute"])[2] == "absolute"
    for argv in (["--fingertip-actions", "delta", "--symmetry"], ["--symmetry", "--fingertip-actions=absolute"],
                 ["--fingertip-actions", "delta", "rlg.params.config.symmetry_augmentation=True"]):
        with pytest.raises(ValueError, match="--fingertip-actions with --symmetry"):
            tp.parse_args(argv)
    with pytest.raises(ValueError, match="delta, absolute"):
        tp.parse_args(["--fingertip-actions", "joint"])


# ---- 5. completeness of the guard-band table of the library ---------------------------------------------------------------------------------------------
def kin_stream_entry_points():
    """every tfk_* function of include/trifinger_kin.h that takes a `stream` argument, parsed as tests/test_guard_bands.py::stream_entry_points does"""
    return sorted(name for name, params in re.findall(r"\b(tfk_[a-z0-9_]+)\s*\(([^()]*)\)\s*;", _header()) if re.search(r"\bstream\b", params))


def test_every_launching_entry_point_of_the_library_is_a_row_or_exempt():
    import test_kin_guard_bands_gpu as table
    names = kin_stream_entry_points()
    assert names == ["tfk_forward", "tfk_inverse", "tfk_tip_action"], names
    covered = table.covered_entry_points()
    for name, reason in table.EXEMPT.items():
        assert isinstance(reason, str) and len(reason.split()) >= 3 and "\n" not in reason, (name, reason)
    assert not set(covered) & set(table.EXEMPT)
    missing = [n for n in names if n not in covered and n not in table.EXEMPT]
    assert not missing, f"entry points that launch on a stream without a guard-band row or an exemption: {missing}"
    stale = [n for n in list(covered) + list(table.EXEMPT) if n not in names]
    assert not stale, f"rows / exemptions for functions the header does not declare with a stream: {stale}"
