"""The critic's privileged states against fp64 physics: the fingertip block states[od+6 : od+45] and the fingertip wrench sensor
states[od+54 : od+72] (od = obs width; asymmetric_obs on, the shipped training configuration).

Every other test of these 57 slots compares HIP with the oracle, which restates the same formulas.  Here the references are the independent
fp64 URDF model (tests/physics_ref.py, tests/test_physics_analytic.py, tests/model_fixture.py) and conservation laws; nothing is taken
from the oracle.  The conventions these tests pin (sensors):

  * fingertip block, per finger: tip-link origin (3), orientation quaternion xyzw of Rz(yaw_f) Ry(q1) Rx(q2 + q3) (4), linear velocity of the
    origin (3), angular velocity (3), all in the world frame;
  * wrench, per finger: force (3) and torque (3) that the contacts exert ON the fingertip, as the mean over the substeps x control_decimation
    of the step, torque about the tip-link origin with the arm ending at the contact point on the FINGER's surface, both rotated into the
    tip-link frame at the POST-step pose; contacts of the distal link and fingertip with the cube, the floor and the boundary count, a
    contact held by the middle link and finger-finger contacts do not.

The scenarios run on the oracle in the CPU suite (fused step and split path) and under `-m gpu` on the HIP library with kernel_variant forced
to narrow / wide / wide_helpers and on the split path: the four ways the wrench is handed from the last substep to the observation phase.

TF_S_CF_FACE names the cube's lowest face after every substep (0 only after a reset), so "the cube is off the floor" is read from the normal
impulses of the four floor corners (no_floor_or_wall_impulse below).  Every check prints its largest residual before it asserts (pytest -s).
"""
import numpy as np
import pytest
import torch

import model_fixture as MF
import physics_ref as PR
import test_contact_scenarios as S
import test_physics_analytic as T
from leibnizgym_amd import _capi as capi
from oracle_util import golden

OD = 41                                    # obs width of the torque command mode: 32 + 9
TIP0, FT0 = OD + 6, OD + 54                # first slot of the fingertip block (3 x 13) and of the wrench block (3 x 6)
VARIANTS = ("narrow", "wide", "wide_helpers")
GRAVITY = np.array([0.0, 0.0, -9.81])
CLIP_OBS = 5.0                             # the clip of the shipped wrapper (leibnizgym_amd/wrappers/vec_task.py)


# ---- engines and steps on every path ---------------------------------------------------------------------------------------------------
def sensor_engine(lib, device, path, model_edit=None, n=1, **kw):
    """one torque-mode engine with the critic's states on; `path`: 'fused' (whatever instantiation the library picks), one of VARIANTS
    (forced), or 'split' (apply_resets / pre_step / simulate / post_step / finish_step)"""
    base = dict(command_mode="torque", normalize_action=False, apply_safety_damping=False, asymmetric_obs=True, normalize_obs=False)
    base.update(kw)
    eng = T.engine(lib, n=n, device=device, model_edit=model_edit, **base)
    if path in VARIANTS:
        eng.kernel_variant = path
        assert eng.kernel_variant == path
    return eng


def step_path(eng, act, path):
    if path == "split":
        eng.action_buf.copy_(act)
        eng.apply_resets()
        eng.pre_step()
        for _ in range(eng.cfg.control_decimation):
            eng.simulate()
        eng.post_step()
        eng.finish_step()
    else:
        eng.step(act)


def step_torque(eng, tau, path, *followers):
    act = torch.tensor(np.clip(tau, -0.36, 0.36), dtype=torch.float32, device=eng.device)[None, :]
    for e in (eng,) + followers:
        step_path(e, act, path)


def states_np(eng):
    return eng.states.cpu().numpy().astype(np.float64)


def scale_transform_ref(raw):
    """scale_transform (torch_utils.py:18-36) of raw states with the scale table of the golden `obs` fixture, clamped at the wrapper's clip; fp64"""
    g = golden("obs")
    lo, hi = g["torque_na0_states_lo"].astype(np.float64), g["torque_na0_states_hi"].astype(np.float64)
    return np.clip(2.0 * (raw - 0.5 * (lo + hi)) / (hi - lo), -CLIP_OBS, CLIP_OBS)


def wrench_world(sts, st_post):
    """the sensor's force and torque of the three fingers in the WORLD frame: rotated out of the tip-link frame with the fp64 rotation of the tip link
    at the post-step joint positions"""
    F, Tq = np.zeros((3, 3)), np.zeros((3, 3))
    for f in range(3):
        R = PR.link_rotation_world(f, st_post[3 * f:3 * f + 3], 3)
        F[f] = R @ sts[FT0 + 6 * f:FT0 + 6 * f + 3]
        Tq[f] = R @ sts[FT0 + 6 * f + 3:FT0 + 6 * f + 6]
    return F, Tq


# ---- 1. fingertip block ----------------------------------------------------------------------------------------------------------------
def fingertip_inputs():
    """130 envs (two full wavefronts and a ragged one): q uniform inside the joint limits, qd uniform in +-10; envs exactly on a lower / upper limit
    of each joint, at +-10 and at 0, some of them in the ragged tail.  fp32 values, [env, finger, joint]."""
    rng = np.random.default_rng(11)
    n = 130
    q = rng.uniform(PR.Q_LO, PR.Q_HI, (n, 3, 3))
    qd = rng.uniform(-PR.QD_MAX, PR.QD_MAX, (n, 3, 3))
    for j in range(3):
        q[2 * j, :, j] = PR.Q_LO[j]
        q[2 * j + 1, :, j] = PR.Q_HI[j]
        q[64 + j, j, :] = PR.Q_LO                              # one finger at a time, second wavefront
        qd[10 + j, :, j] = PR.QD_MAX
        qd[13 + j, :, j] = -PR.QD_MAX
    q[6], q[7], q[128], q[129] = PR.Q_LO, PR.Q_HI, PR.Q_HI, PR.Q_LO
    qd[8], qd[9], qd[16], qd[127], qd[129] = PR.QD_MAX, -PR.QD_MAX, 0.0, 0.0, PR.QD_MAX
    qd[17, 1], qd[128, 2] = 0.0, -PR.QD_MAX
    return q.astype(np.float32), qd.astype(np.float32)


def compare_fingertip_block(sts, q, qd, tag):
    """states [n, 113] against the fp64 tip-link state at the fp32 joint positions / velocities q, qd [n, 3, 3].  Tolerances: fp32 rounding,
    magnitude x 6e-8 x about ten operations - positions < 0.5 m: 1e-6 m; rotation entries (products of four sines / cosines of rounded half
    angles): 2e-6; velocities (levers <= 0.35 m, |qd| <= 10, three terms): 5e-6; quaternion norm 1e-6."""
    worst = dict(pos=0.0, rot=0.0, norm=0.0, lin=0.0, ang=0.0)
    for i in range(q.shape[0]):
        for f in range(3):
            got = sts[i, TIP0 + 13 * f:TIP0 + 13 * f + 13]
            p, R, v, w = PR.tip_state_ref(f, q[i, f], qd[i, f])
            worst["pos"] = max(worst["pos"], np.abs(got[0:3] - p).max())
            worst["rot"] = max(worst["rot"], np.abs(PR.quat_rot(got[3:7]) - R).max())
            worst["norm"] = max(worst["norm"], abs(np.linalg.norm(got[3:7]) - 1.0))
            worst["lin"] = max(worst["lin"], np.abs(got[7:10] - v).max())
            worst["ang"] = max(worst["ang"], np.abs(got[10:13] - w).max())
    print(f"[privileged state] fingertip block {tag}: " + ", ".join(f"{k} {v:.2e}" for k, v in worst.items()))
    assert worst["pos"] < 1e-6 and worst["rot"] < 2e-6 and worst["norm"] < 1e-6 and worst["lin"] < 5e-6 and worst["ang"] < 5e-6, (tag, worst)


def _check_fingertip_block(lib, device, paths):
    q, qd = fingertip_inputs()
    n = q.shape[0]
    assert ((q == PR.Q_LO.astype(np.float32)).any(0).all() and (q == PR.Q_HI.astype(np.float32)).any(0).all()
            and (np.abs(qd) == 10.0).any(0).all() and (qd == 0.0).any(0).all())      # every joint of every finger sees its edges
    for path in paths:
        eng = sensor_engine(lib, device, path if path != "post" else "fused", n=n)
        eng.cube[0:3] = torch.tensor([0.0, 0.0, 5.0], device=device)[:, None]        # the cube out of reach
        eng.q.copy_(torch.tensor(q.reshape(n, 9).T.copy(), device=device))
        eng.qd.copy_(torch.tensor(qd.reshape(n, 9).T.copy(), device=device))
        if path == "post":                                                             # the observation phase alone, on the written state
            eng.post_step()
            q1, qd1 = q, qd
            # ... and its normalised form: fingertip speeds of metres per second against the +-0.2 m/s of the scale table reach the wrapper's clip
            engn = sensor_engine(lib, device, "fused", n=n, normalize_obs=True)
            engn.set_clipping(CLIP_OBS, 0.0)
            engn.state.copy_(eng.state)
            engn.post_step()
            want, got = scale_transform_ref(states_np(eng))[:, TIP0:TIP0 + 39], states_np(engn)[:, TIP0:TIP0 + 39]
            engn.close()
            print(f"[privileged state] fingertip block, normalised and clamped: {np.abs(got - want).max():.2e}")
            assert (np.abs(want) == CLIP_OBS).sum() > 100 and (np.abs(want) < CLIP_OBS).sum() > 100
            assert np.abs(got - want).max() < 2e-6, np.abs(got - want).max()
        else:                                                                          # one fused step with zero torque: the block describes the state it ends in
            eng.step(torch.zeros(n, 9, device=device))
            st = eng.state.cpu().numpy()
            assert np.isfinite(st).all()
            q1, qd1 = st[0:9].T.reshape(n, 3, 3), st[9:18].T.reshape(n, 3, 3)
            assert np.abs(qd1).max() > 5.0 and not np.array_equal(q1, q)               # it moved, and still fast
        sts = states_np(eng)
        assert int(eng.info[capi.INFO_NUM_NONFINITE].item()) == 0
        eng.close()
        assert sts.shape == (n, OD + 72)
        compare_fingertip_block(sts, q1, qd1, path)


def test_fingertip_block_matches_fp64_kinematics(oracle):
    _check_fingertip_block(oracle, "cpu", ("post", "fused"))


@pytest.mark.gpu
def test_fingertip_block_matches_fp64_kinematics_gpu(hip):
    _check_fingertip_block(hip, "cuda:0", ("post",) + VARIANTS)


# ---- 2. + 5. wrench sensor: exact balances on the held cube, raw and normalised ---------------------------------------------------------------
N_SQUEEZE, N_LIFT, N_HOLD = 10, 55, 25      # control periods of 0.02 s: squeeze on the floor, lift by 55 mm, short hold


def pinch_run(lib, device, path, substeps, decimation, with_norm=False):
    """The pinch-and-lift grasp of tests/test_contact_scenarios.py, shortened, without cube damping (so that the cube's momentum changes by the contact
    forces and gravity alone).  Returns [(state before the step, state after it, states row of the step, normalised states row or None)]."""
    def edit(m):
        m.cube_linear_damping = 0.0
        m.cube_angular_damping = 0.0
    kw = dict(substeps=substeps, control_decimation=decimation)
    eng = sensor_engine(lib, device, path, edit, **kw)
    followers = ()
    if with_norm:                                              # the same env with normalize_obs on and the wrapper's clip, in lockstep
        engn = sensor_engine(lib, device, path, edit, normalize_obs=True, **kw)
        engn.set_clipping(CLIP_OBS, 0.0)
        followers = (engn,)
    d = PR.CUBE_HALF + S.R_TIP + 0.0005
    tips = [np.array([0.0, d, 0.0325]), np.array([d, -d * np.tan(np.pi / 6), 0.0325]), np.array([-d, -d * np.tan(np.pi / 6), 0.0325])]
    inward = [-t / np.linalg.norm(t[:2]) * np.array([1, 1, 0]) for t in tips]
    q0 = np.concatenate([S.ik(f, tips[f]) for f in range(3)])
    for e in (eng,) + followers:
        e.q[:, 0] = torch.tensor(q0, dtype=torch.float32, device=device)
    lift, rec = 0.0, []
    for i in range(0, N_SQUEEZE + N_LIFT + N_HOLD, decimation):
        if i >= N_SQUEEZE:
            lift = min(0.001 * N_LIFT, lift + 0.001 * decimation)
        # 1.5 N per finger: 200 N/m x 7.5 mm inside the face; a spring half as stiff where the torque is held for two control periods
        targets = [tips[f] + 0.0075 * decimation * inward[f] + np.array([0, 0, lift]) for f in range(3)]
        pre = S.state_np(eng)
        step_torque(eng, S.impedance_torques(pre, targets, kp=200.0 / decimation), path, *followers)
        rec.append((pre, S.state_np(eng), states_np(eng)[0], states_np(followers[0])[0] if with_norm else None))
    assert np.isfinite(rec[-1][1]).all() and rec[-1][1][capi.S_CUBE_P + 2] > 0.06          # the cube ended up in the air
    if with_norm:
        assert torch.equal(eng.state, followers[0].state)
    for e in (eng,) + followers:
        e.close()
    return rec


def no_floor_or_wall_impulse(st):
    """TF_S_CF_FACE names the lowest face of the cube after every substep (it is 0 only after a reset), so it cannot tell whether the floor pushes: the
    normal impulses of the four floor corners do (they are rewritten by every substep); TF_S_CW_FACE is 0 while no corner touches the boundary"""
    return not st[capi.S_LAM_CF:capi.S_LAM_CF + 12:3].any() and st[capi.S_CW_FACE] == 0


def cube_touches_only_distal_links(pre, post):
    """the cube is off the floor and the boundary when the step starts and when it ends, and no finger holds it with another link than the distal one"""
    return (no_floor_or_wall_impulse(pre) and no_floor_or_wall_impulse(post)
            and all((int(post[capi.S_FC_LINK + f]) & 3) in (0, 3) for f in range(3)))


def linear_balance(rec, decimation):
    """m dv/dt - (m g - sum_f R_f F_f) of every step in which the cube touches nothing but distal links: the sensor reports the force ON the
    fingertip, the cube gets its negative; dv over the whole step, so the sensor must be the MEAN over its substeps x decimation"""
    out = []
    for pre, post, sts, _ in rec:
        if not cube_touches_only_distal_links(pre, post):
            continue
        F, _ = wrench_world(sts, post)
        dv = post[capi.S_CUBE_V:capi.S_CUBE_V + 3] - pre[capi.S_CUBE_V:capi.S_CUBE_V + 3]
        out.append((np.abs(PR.CUBE_MASS * dv / (0.02 * decimation) - (PR.CUBE_MASS * GRAVITY - F.sum(0))).max(), np.linalg.norm(F, axis=1).max()))
    return np.array(out)


def finger_side_gap(f, st):
    """(gap, normal from the cube to the finger) of the distal shape of finger f nearest to the cube at the pose of state st, fp64"""
    c = st[capi.S_CUBE_P:capi.S_CUBE_P + 7]
    R = PR.quat_rot(c[3:7])
    gap, _, x, y, _ = min(PR.shape_candidates(f, st[3 * f:3 * f + 3], c[0:3], R, np.full(3, PR.CUBE_HALF), links=(3,)), key=lambda e: e[0])
    return gap, R @ ((x - y) / np.linalg.norm(x - y))


def angular_balance(rec):
    """I dw/dt - sum_f (y_f - c) x (-F_f), one substep per step.  The cube's rows act at y_f, the point on the CUBE's surface; the sensor's torque
    T_f = a_f x F_f has its arm a_f from the tip-link origin p_f to the point on the FINGER's surface, gap_f n_f further out (contacts are
    speculative: live at gaps of millimetres).  With y_f = p_f + a_f - gap_f n_f:
        sum_f (y_f - c) x (-F_f) = sum_f [(p_f - c) x (-F_f) - T_f + gap_f n_f x F_f],
    p_f, c, gap_f, n_f at the PRE-step pose (where the rows were built), F_f and T_f rotated to the world at the POST-step pose.
    Returns rows (residual, |I dw/dt|, |finger-side correction|)."""
    out = []
    for pre, post, sts, _ in rec:
        if not cube_touches_only_distal_links(pre, post):
            continue
        F, Tq = wrench_world(sts, post)
        c = pre[capi.S_CUBE_P:capi.S_CUBE_P + 3]
        rhs, corr = np.zeros(3), np.zeros(3)
        for f in range(3):
            p = PR.link_point_world(f, pre[3 * f:3 * f + 3], 3, MF.TIP)
            rhs += np.cross(p - c, -F[f]) - Tq[f]
            if np.any(F[f] != 0.0):
                gap, n = finger_side_gap(f, pre)
                corr += gap * np.cross(n, F[f])
        lhs = PR.CUBE_INERTIA * (post[capi.S_CUBE_W:capi.S_CUBE_W + 3] - pre[capi.S_CUBE_W:capi.S_CUBE_W + 3]) / 0.02
        out.append((np.abs(lhs - (rhs + corr)).max(), np.linalg.norm(lhs), np.linalg.norm(corr)))
    return np.array(out)


def normalised_form(rec):
    """the normalised states of the lockstep env against scale_transform of the raw ones, clamped"""
    worst, biggest = 0.0, 0.0
    for _, _, raw, nrm in rec:
        want = scale_transform_ref(raw)
        for sl in (slice(TIP0, TIP0 + 39), slice(FT0, FT0 + 18)):
            worst = max(worst, np.abs(nrm[sl] - want[sl]).max())
        biggest = max(biggest, np.abs(want[FT0:FT0 + 18]).max())
    return worst, biggest


def _check_wrench_on_held_cube(lib, device, path, cases=((1, 1), (2, 1), (2, 2))):
    """Bounds: fp32 rounding of forces of 1.5 N, arms of 0.05 m and of m dv/dt - 2e-6 N and 5e-7 N m."""
    for substeps, decimation in cases:
        rec = pinch_run(lib, device, path, substeps, decimation, with_norm=(substeps, decimation) == (2, 1))
        lin = linear_balance(rec, decimation)
        tag = f"{path} substeps {substeps} decimation {decimation}"
        print(f"[privileged state] held cube {tag}: {len(lin)} qualifying steps of {len(rec)}, linear residual {lin[:, 0].max():.2e} N, "
              f"largest force {lin[:, 1].max():.2f} N")
        assert len(lin) >= 30 and lin[:, 1].max() > 1.0, (tag, len(lin))
        assert lin[:, 0].max() < 2e-6, (tag, lin[:, 0].max())
        if (substeps, decimation) == (1, 1):
            ang = angular_balance(rec)
            n_dyn, n_corr = int((ang[:, 1] > 5e-3).sum()), int((ang[:, 2] > 1e-3).sum())
            print(f"[privileged state] held cube {tag}: angular residual {ang[:, 0].max():.2e} N m, {n_dyn} steps with |I dw/dt| > 5e-3, "
                  f"{n_corr} with a finger-side correction > 1e-3")
            assert len(ang) >= 30 and n_dyn >= 10 and n_corr >= 10, (tag, len(ang), n_dyn, n_corr)      # not vacuous: the grasp moves, the gaps are open
            assert ang[:, 0].max() < 5e-7, (tag, ang[:, 0].max())
        if (substeps, decimation) == (2, 1):
            worst, biggest = normalised_form(rec)
            print(f"[privileged state] held cube {tag}: normalised blocks {worst:.2e} off scale_transform, largest scaled wrench value {biggest:.2f}")
            assert biggest > 1.0                             # forces beyond the +-1 N of the scale table: the scaling is seen
            assert worst < 2e-6, (tag, worst)
    return rec                                               # of the last case


def test_wrench_balances_the_held_cube(oracle):
    _check_wrench_on_held_cube(oracle, "cpu", "fused")


@pytest.mark.gpu
@pytest.mark.parametrize("variant", VARIANTS)
def test_wrench_balances_the_held_cube_gpu(hip, variant):
    _check_wrench_on_held_cube(hip, "cuda:0", variant)


# ---- 6. the split path and its TF_S_FT rows -----------------------------------------------------------------------------------------------
def _check_split_path(lib, device):
    """The same balances with the five split entries, and the state rows they hand the wrench over in.  include/trifinger.h: TF_S_FT holds, per
    finger, world-frame force 3 + torque 3 about the tip-link origin, SUMMED over the substeps since tf_pre_step (tf_post_step divides by
    substeps x control_decimation and rotates).  With control_decimation = 2 the sum crosses two tf_simulate launches: the second reads the rows the
    first one wrote.  Checked without the sensor: the rows alone close the cube's linear momentum in the world frame, with the divisor 2 x 2."""
    substeps, decimation = 2, 2
    rec = _check_wrench_on_held_cube(lib, device, "split", cases=((1, 1), (2, 1), (substeps, decimation)))
    n_sub = substeps * decimation
    worst_rows, worst_sensor, n = 0.0, 0.0, 0
    for pre, post, sts, _ in rec:
        rows = post[capi.S_FT:capi.S_FT + 18].reshape(3, 6)
        F, Tq = wrench_world(sts, post)
        worst_sensor = max(worst_sensor, np.abs(rows[:, 0:3] / n_sub - F).max(), np.abs(rows[:, 3:6] / n_sub - Tq).max())
        if cube_touches_only_distal_links(pre, post):
            dv = post[capi.S_CUBE_V:capi.S_CUBE_V + 3] - pre[capi.S_CUBE_V:capi.S_CUBE_V + 3]
            worst_rows = max(worst_rows, np.abs(PR.CUBE_MASS * dv / (0.02 * decimation) - (PR.CUBE_MASS * GRAVITY - rows[:, 0:3].sum(0) / n_sub)).max())
            n += 1
    print(f"[privileged state] split path, TF_S_FT rows / {n_sub}: linear residual {worst_rows:.2e} N over {n} steps, {worst_sensor:.2e} off the sensor")
    assert n >= 30 and worst_rows < 2e-6, (n, worst_rows)
    assert worst_sensor < 1e-6, worst_sensor                 # the rotation of 1.5 N / 0.02 N m into the tip-link frame and back: a few ulp


def test_wrench_on_the_split_path(oracle):
    _check_split_path(oracle, "cpu")


@pytest.mark.gpu
def test_wrench_on_the_split_path_gpu(hip):
    _check_split_path(hip, "cuda:0")


# ---- 3. wrench sensor: a fingertip pressed against the arena, at rest --------------------------------------------------------------------
def press_run(lib, device, path, target, kp, kd, steps, q_start=None):
    """finger 0's tip is pulled towards `target` (outside the arena) by the impedance controller until it rests against the floor / the boundary"""
    eng = sensor_engine(lib, device, path)
    f32 = dict(dtype=torch.float32, device=device)
    eng.cube[0:3, 0] = torch.tensor([0.0, -0.10, 0.0325], **f32)                     # at rest on the floor, away from finger 0
    if q_start is not None:
        eng.q[0:3, 0] = torch.tensor(q_start, **f32)
    for _ in range(steps):
        tau = S.impedance_torques(S.state_np(eng), [target, None, None], kp=kp, kd=kd)
        step_torque(eng, tau, path)
    st, sts = S.state_np(eng), states_np(eng)[0]
    eng.close()
    return st, sts, np.clip(tau, -0.36, 0.36).astype(np.float32).astype(np.float64)


def check_press(st, sts, tau, normal_of, on_wall, tag):
    """at rest: the joint torques balance, J^T F + tau - g(q) = 0 with J the Jacobian of the contact point (what is left is the truncation of the 8
    sweeps: 5e-5 N m); the sensor's torque is arm x force with the arm from the tip-link origin to the cap centre minus cap_radius n (1e-7); the
    force on the fingertip points away from the surface"""
    q = st[0:3]
    assert np.abs(st[9:12]).max() < 1e-3, (tag, st[9:12])                             # at rest
    # this contact alone: bit 4 of the activity code says whether the boundary pushes (the TF_S_LAM_TW rows are defined only then), the floor rows
    # are rewritten by every substep
    wall_pushes, floor_lam = (int(st[capi.S_FC_LINK]) & 4) != 0, st[capi.S_LAM_TF]
    assert (wall_pushes and st[capi.S_LAM_TW] > 0 and floor_lam == 0) if on_wall else (not wall_pushes and floor_lam > 0), (tag, st[capi.S_FC_LINK], floor_lam)
    F, Tq = wrench_world(sts, st)
    B = PR.link_point_world(0, q, 3, S.TIP)
    n = normal_of(B)
    P = B - S.R_TIP * n
    statics = PR.point_jacobian(0, q, 3, P).T @ F[0] + tau[0:3] - S.gravity_torque(q)
    arm = np.cross(P - PR.link_point_world(0, q, 3, MF.TIP), F[0]) - Tq[0]
    print(f"[privileged state] {tag} press, F.n = {F[0] @ n:.3f} N: statics {np.abs(statics).max():.2e} N m, torque arm {np.abs(arm).max():.2e} N m")
    assert F[0] @ n > 0.2, (tag, F[0], n)
    assert np.abs(statics).max() < 5e-5, (tag, statics)
    assert np.abs(arm).max() < 1e-7, (tag, arm)
    assert np.abs(Tq[0]).max() > 1e-3                                                 # (the arm is not along the force)
    assert not sts[FT0 + 6:FT0 + 18].any()                                            # the other two fingers touch nothing
    return F[0]


def _check_press_on_the_arena(lib, device, path):
    # floor: the spring pulls the tip 20 mm below where it comes to rest: 100 N/m x 20 mm = 2 N
    rest = np.array([0.0, 0.12, S.R_TIP])
    st, sts, tau = press_run(lib, device, path, rest - np.array([0.0, 0.0, 0.02]), 100.0, 2.0, 60, q_start=S.ik(0, rest + np.array([0.0, 0.0, 0.003])))
    F = check_press(st, sts, tau, lambda B: np.array([0.0, 0.0, 1.0]), False, "floor")
    assert 1.8 < F[2] < 2.2, F
    # boundary: the set-up of test_fingertip_stays_inside_the_boundary

    def wall_normal(B):
        wc, wsn = PR.wall_tilt(B[2])
        rho = np.hypot(B[0], B[1])
        return np.array([-B[0] / rho * wc, -B[1] / rho * wc, wsn])
    st, sts, tau = press_run(lib, device, path, np.array([0.0, 0.205, 0.045]), 30.0, 1.5, 200)
    check_press(st, sts, tau, wall_normal, True, "boundary")


def test_wrench_of_a_fingertip_pressed_on_the_arena(oracle):
    _check_press_on_the_arena(oracle, "cpu", "fused")


@pytest.mark.gpu
@pytest.mark.parametrize("path", VARIANTS + ("split",))
def test_wrench_of_a_fingertip_pressed_on_the_arena_gpu(hip, path):
    _check_press_on_the_arena(hip, "cuda:0", path)


# ---- 4. what does not count ------------------------------------------------------------------------------------------------------------
def _check_not_counted(lib, device, path):
    # (a) the middle link holds the finger-cube contact (the scenario of test_middle_link_cannot_pass_through_the_cube, one substep per step so that
    # the activity code after a step names the link of its only substep): that finger's six values are exactly 0
    eng = sensor_engine(lib, device, path, gravity=(0.0, 0.0, 0.0), dt=0.01, substeps=1)
    q = np.array([-0.25, 0.35, -1.2])
    mid_local = np.array([0.028, 0.0, -0.08])
    mid = PR.link_point_world(0, q, 2, mid_local)
    side = PR.link_point_world(0, q + np.array([0.3, 0, 0]), 2, mid_local) - mid
    side /= np.linalg.norm(side)
    lo_, hi_ = 0.0, 0.2
    for _ in range(50):
        d_ = 0.5 * (lo_ + hi_)
        if S._capsule_gap(0, q, 2, np.concatenate([mid + side * d_, [0, 0, 0, 1]])) < 0.01:
            lo_ = d_
        else:
            hi_ = d_
    f32 = dict(dtype=torch.float32, device=device)
    eng.q[0:3, 0] = torch.tensor(q, **f32)
    eng.cube[0:3, 0] = torch.tensor(mid + side * hi_, **f32)
    tau = np.zeros(9)
    tau[0] = 0.2
    pushed = 0
    for _ in range(80):
        step_torque(eng, tau, path)
        st, sts = S.state_np(eng), states_np(eng)[0]
        if (int(st[capi.S_FC_LINK]) & 3) == 2:
            pushed += st[capi.S_LAM_FC] > 0
            assert not sts[FT0:FT0 + 6].any(), sts[FT0:FT0 + 6]
    assert pushed >= 3                                       # the middle link did push the cube
    eng.close()
    # (b) STATED DEVIATION: finger-finger contacts are solved in a pre-pass on the free velocities and are not in the sensor, although two distal links
    # pressed together do load the fingertips (an IsaacGym force sensor on the tip link would report them): all 18 values stay 0 while the two
    # fingertips of test_two_fingers_stop_at_two_radii push against each other
    eng = sensor_engine(lib, device, path)
    eng.cube[0:3, 0] = torch.tensor([0.0, -0.12, 0.0325], **f32)                     # at rest on the floor, out of every finger's reach
    meet = np.array([0.03, 0.02, 0.09])
    for i in range(80):
        step_torque(eng, S.impedance_torques(S.state_np(eng), [meet, meet, None], kp=120.0, kd=2.0), path)
        assert not states_np(eng)[0][FT0:FT0 + 18].any()
    st = S.state_np(eng)
    eng.close()
    segs = [(PR.link_point_world(f, st[3 * f:3 * f + 3], 3, PR.TIP_CAP[1]), PR.link_point_world(f, st[3 * f:3 * f + 3], 3, S.TIP)) for f in (0, 1)]
    Pa, Pb = PR.segment_segment(segs[0][0], segs[0][1], segs[1][0], segs[1][1])
    assert abs(np.linalg.norm(Pa - Pb) - 2 * S.R_TIP) < 1e-3                         # they do rest on each other, 2.4 cm short of their common target
    assert min(np.linalg.norm(segs[f][1] - meet) for f in (0, 1)) > 5e-3


def test_middle_link_and_finger_finger_contacts_are_not_in_the_wrench(oracle):
    _check_not_counted(oracle, "cpu", "fused")


@pytest.mark.gpu
@pytest.mark.parametrize("path", VARIANTS + ("split",))
def test_middle_link_and_finger_finger_contacts_are_not_in_the_wrench_gpu(hip, path):
    _check_not_counted(hip, "cuda:0", path)
