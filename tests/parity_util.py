"""Shared driver of the HIP-vs-oracle parity tests: run the same seeded rollout through both libraries."""
import numpy as np
import torch

from leibnizgym_amd.engine import TrifingerEngine, make_config

D4_REWARDS = {   # scripts/rlg_hydra.py:140-174
    "finger_move_penalty": {"activate": True, "weight": -0.1},
    "finger_reach_object_rate": {"activate": True, "norm_p": 2, "weight": -250,
                                 "thresh_sched_start": 0, "thresh_sched_end": 1e7},
    "object_dist": {"activate": True, "weight": 2000, "thresh_sched_start": 0, "thresh_sched_end": 10e10},
    "object_rot": {"activate": True, "weight": 2000, "epsilon": 0.01, "scale": 3.0,
                   "thresh_sched_start": 1e7, "thresh_sched_end": 1e10},
    "object_rot_delta": {"activate": False, "weight": -250},
    "object_move": {"activate": False, "weight": -750},
}
D1_REWARDS = {   # scripts/rlg_hydra.py:83-109
    "finger_move_penalty": {"activate": True, "weight": -0.1},
    "finger_reach_object_rate": {"activate": True, "norm_p": 2, "weight": -750},
    "object_dist": {"activate": True, "weight": 2000},
    "object_rot": {"activate": False, "weight": 300},
    "object_rot_delta": {"activate": False, "weight": -250},
    "object_move": {"activate": False, "weight": -750},
}

CONFIGS = {
    # BASELINE config 1/2 shape: difficulty 1, torque mode, symmetric obs (scripts/rlg_hydra.py:58-118)
    "d1_torque_sym": dict(command_mode="torque", task_difficulty=1, asymmetric_obs=False, reward_terms=D1_REWARDS,
                          success={"activate": False, "bonus": 5000.0, "position_tolerance": 0.01,
                                   "orientation_tolerance": 0.1}),
    # BASELINE config 3 shape: difficulty 4 reward schedule, asymmetric obs (shipped asymm.yaml)
    "d4_torque_asym": dict(command_mode="torque", task_difficulty=4, asymmetric_obs=True, reward_terms=D4_REWARDS,
                           success={"activate": False, "bonus": 5000.0, "position_tolerance": 0.02,
                                    "orientation_tolerance": 0.25}),
    # env default dict: position mode, every reward term on, success termination on -> goal resets + dones
    "envdefault_position": dict(command_mode="position", task_difficulty=1, asymmetric_obs=True,
                                success={"activate": True, "bonus": 5000.0, "position_tolerance": 0.05,
                                         "orientation_tolerance": 0.2}),
    # BASELINE config 4 shape: difficulty 4 + (build-defined) domain randomisation
    "d4_domain_randomization": dict(command_mode="torque", task_difficulty=4, asymmetric_obs=True,
                                    reward_terms=D4_REWARDS,
                                    domain_randomization={"activate": True, "cube_mass": (0.5, 1.5),
                                                          "cube_size": (0.85, 1.1), "friction": (0.5, 1.4),
                                                          "motor_torque": (0.8, 1.2), "link_mass": (0.8, 1.25),
                                                          "restitution": (0.25, 2.0), "obs_noise": 0.02,
                                                          "action_repeat_prob": 0.2},
                                    success={"activate": False, "bonus": 5000.0, "position_tolerance": 0.02,
                                             "orientation_tolerance": 0.25}),
    # the rest of the intent list: robot base / stage offsets, friction per body (the EXT kernels of the HIP library)
    "d4_domain_randomization_extended": dict(command_mode="torque", task_difficulty=4, asymmetric_obs=True,
                                             reward_terms=D4_REWARDS,
                                             domain_randomization={"activate": True, "cube_mass": (0.5, 1.5),
                                                                   "cube_size": (0.85, 1.1), "friction": (0.5, 1.4),
                                                                   "robot_base_position": (0.01, 0.02, 0.004),
                                                                   "stage_position": (0.02, 0.015),
                                                                   "friction_robot": (0.7, 1.3), "friction_object": (0.5, 1.5),
                                                                   "friction_stage": (0.6, 1.4), "obs_noise": 0.01},
                                             success={"activate": False, "bonus": 5000.0, "position_tolerance": 0.02,
                                                      "orientation_tolerance": 0.25}),
    # everything else: impedance actions (A=18), random robot reset, moving goal, difficulty 3, decimation 2, and the
    # wrapper clipping fused into the step with bounds tight enough to bite (tf_set_clipping)
    "impedance_random_moving": dict(_clipping=(0.8, 0.7), command_mode="position_impedance", task_difficulty=3, asymmetric_obs=True,
                                    robot_reset="random", goal_rotation=True, control_decimation=2,
                                    normalize_obs=False,
                                    success={"activate": True, "bonus": 100.0, "position_tolerance": 0.04,
                                             "orientation_tolerance": 3.2}),
    # robot resets that spread the joints widely: fingers meet at resets and under random torques, so the middle-distal finger-finger pairs
    # (TfModel.ff_middle_pairs, part of the default model since API 8) carry impulses (tests/test_ff_middle_pairs.py: the switch changes this very rollout)
    "ff_middle_pairs": dict(command_mode="torque", task_difficulty=1, asymmetric_obs=True,
                            robot_reset="random", dof_pos_stddev=1.2, dof_vel_stddev=0.5, reward_terms=D1_REWARDS,
                            success={"activate": False, "bonus": 5000.0, "position_tolerance": 0.01, "orientation_tolerance": 0.1}),
    # the opt-out: the distal pairs only (`native.ff_middle_pairs: false`, what every earlier API stepped), on the headline workload
    "fast_contact_set": dict(_model_edit=dict(ff_middle_pairs=0), command_mode="torque", task_difficulty=4, asymmetric_obs=True, reward_terms=D4_REWARDS,
                             robot_reset="random", dof_pos_stddev=1.2, dof_vel_stddev=0.5,
                             success={"activate": False, "bonus": 5000.0, "position_tolerance": 0.02, "orientation_tolerance": 0.25}),
}

PER_ENV_FIELDS = ("state", "action_buf", "obs", "states", "reward", "reset_buf", "goal_reset_buf", "successes",
                  "dones", "steps", "reset_count")


def snapshot(eng):
    d = {k: getattr(eng, k).detach().cpu().numpy().copy() for k in PER_ENV_FIELDS}
    d["info"] = eng.info.detach().cpu().numpy().copy()
    return d


def actions_for(step, n, a, seed):
    g = torch.Generator().manual_seed(seed * 100003 + step)
    return (torch.rand(n, a, generator=g) * 2 - 1).contiguous()


VARIANTS = ("narrow", "wide", "wide_helpers")     # the instantiations of the fused step (include/trifinger.h: tf_set_kernel_variant); at the sizes of these
                                                  # tests tf_create would always pick one of the 256-register ones, so the parity tests force each in turn

_ORACLE_ROLLOUTS = {}


def oracle_rollout(oracle, n, steps, cfg_name, **kw):
    """the oracle's rollout, computed once per argument set (several product variants are compared with it)"""
    key = (n, steps, cfg_name, repr(sorted(kw.items(), key=lambda kv: kv[0])))
    if key not in _ORACLE_ROLLOUTS:
        _ORACLE_ROLLOUTS[key] = rollout(oracle, "cpu", n, steps, cfg_name, **kw)
    return _ORACLE_ROLLOUTS[key]


LOW_RING_Z0 = -0.01      # wall_z[0] of the low-ring model: the vertical ring ends below the floor, the whole boundary is cone


def surface_model(lib, low_ring=False, base=None):
    """the default model (or `base`) with TfModel.cube_wall_surface on; `low_ring`: wall_z[0] = LOW_RING_Z0, the other knots as they are - a cube
    that slides to the boundary on the floor then touches the cone with its lower corners, so random rollouts run the surface rows all the time
    (on the shipped profile they almost never do)"""
    m = base if base is not None else lib.default_model()
    m.cube_wall_surface = 1
    if low_ring:
        m.wall_z[0] = LOW_RING_Z0
    return m


def cube_corner_positions(state, m):
    """The eight corners (+-h, +-h, +-h) of every env's cube in the pose of `state` (TF_STATE_ROWS x N), relative to the stage centre: h = cube_half
    of model `m` times the env's cube-size factor, rotated by the cube quaternion (x, y, z, w), the env's stage offset subtracted (0 without the
    extended domain randomisation).  -> (px, py, pz), each (8, N), and h (N,)"""
    from leibnizgym_amd import _capi as capi
    st = np.asarray(state, dtype=np.float64)
    dr = st[capi.S_DR:capi.S_DR + capi.TF_NUM_DR]
    hc = float(m.cube_half) * dr[1]                                               # cube size of the env (1 without randomisation)
    cp = st[capi.S_CUBE_P:capi.S_CUBE_P + 3].copy()
    cp[0:2] -= dr[capi.DR_STAGE_POS:capi.DR_STAGE_POS + 2]
    x, y, z, w = st[capi.S_CUBE_Q:capi.S_CUBE_Q + 4]
    px, py, pz = [], [], []
    for sx in (-1.0, 1.0):
        for sy in (-1.0, 1.0):
            for sz in (-1.0, 1.0):
                lx, ly, lz = sx * hc, sy * hc, sz * hc
                tx = 2 * (y * lz - z * ly); ty = 2 * (z * lx - x * lz); tz = 2 * (x * ly - y * lx)
                px.append(cp[0] + lx + w * tx + (y * tz - z * ty))
                py.append(cp[1] + ly + w * ty + (z * tx - x * tz))
                pz.append(cp[2] + lz + w * tz + (x * ty - y * tx))
    return np.array(px), np.array(py), np.array(pz), hc


def cone_census(state, m):
    """Per env (bool array): the pose of `state` has a boundary contact (cw_face != 0) and a cube corner - any of the eight - above wall_z[0] within
    contact_slack of the boundary profile of model `m`.  Geometric, from the pose alone: what says that the rows of the tilted surface
    (TfModel.cube_wall_surface) were live in the step that left this state."""
    from leibnizgym_amd import _capi as capi
    px, py, pz, _ = cube_corner_positions(state, m)
    wz, wr = np.array(m.wall_z[:], dtype=np.float64), np.array(m.wall_r[:], dtype=np.float64)
    r_at = np.where(pz < wz[-1], np.interp(pz, wz, wr), np.inf)                    # nothing above the last knot
    near = (pz > wz[0]) & (r_at - np.hypot(px, py) < float(m.contact_slack))
    return near.any(axis=0) & (np.asarray(state)[capi.S_CW_FACE] != 0)


def place_cubes_at_the_boundary(eng, m, first=0, speed=0.4):
    """Overwrite the cube state of envs first.. (after a reset, the same call on every engine of a comparison): the cube lies on the floor, one face
    towards the boundary, its lower outward corners 6 mm inside the profile of model `m` at floor height, sliding outward at `speed` - env i at the
    azimuth 2.4 i rad, so that the envs of a small population meet the boundary at different places within the first steps.  For the low-ring model
    (surface_model): the corners then arrive on the cone."""
    from leibnizgym_amd import _capi as capi
    n = eng.num_envs - first
    hc = float(m.cube_half)
    wz, wr = np.array(m.wall_z[:], dtype=np.float64), np.array(m.wall_r[:], dtype=np.float64)
    r_corner = float(np.interp(0.0, wz, wr)) - 0.006
    r_centre = np.sqrt(r_corner * r_corner - hc * hc) - hc                       # corners at (r_centre + hc, +-hc) in the frame of the azimuth
    phi = 2.4 * np.arange(n, dtype=np.float64)
    cube = np.zeros((13, n))
    cube[0], cube[1], cube[2] = r_centre * np.cos(phi), r_centre * np.sin(phi), hc
    cube[5], cube[6] = np.sin(phi / 2), np.cos(phi / 2)                          # yaw phi (quaternion x, y, z, w)
    cube[7], cube[8] = speed * np.cos(phi), speed * np.sin(phi)
    eng.cube[:, first:] = torch.tensor(cube, dtype=torch.float32).to(eng.cube.device)


def census_summary(flags):
    """flags: list of cone_census arrays of consecutive compared snapshots -> (env-steps counted, env-steps in all, envs that ever had one, envs in
    which the flag changes between two consecutive compared snapshots: a corner went from no boundary rows to live surface rows or back - on the
    low-ring model that is all a change can be, there is no ring a corner could cross over from)"""
    f = np.array(flags, dtype=bool)
    changes = (f[1:] != f[:-1]).any(axis=0) if len(f) > 1 else np.zeros(f.shape[1], dtype=bool)
    return int(f.sum()), int(f.size), int(f.any(axis=0).sum()), int(changes.sum())


def rollout(lib, device, n, steps, cfg_name, seed=3, episode_length=40, extra=None, variant=None, surface=None, place=False):
    """`surface`: None, "default" (TfModel.cube_wall_surface on) or "low_ring" (the same on the low-ring model: surface_model); `place`: the cubes
    are put at the boundary after the reset (place_cubes_at_the_boundary)"""
    kw = dict(CONFIGS[cfg_name])
    kw.update(extra or {})
    clipping = kw.pop("_clipping", None)
    model_edit = kw.pop("_model_edit", None)
    if model_edit:                                   # fields of the default TfModel to overwrite
        kw["model"] = lib.default_model()
        for name, value in model_edit.items():
            setattr(kw["model"], name, value)
    if surface is not None:
        assert surface in ("default", "low_ring"), surface
        kw["model"] = surface_model(lib, low_ring=surface == "low_ring", base=kw.get("model"))
    cfg = make_config(lib, n, seed=seed, episode_length=episode_length, **kw)
    eng = TrifingerEngine(cfg, device=device, lib=lib)
    if variant is not None:
        eng.kernel_variant = variant
        assert eng.kernel_variant == variant
    if clipping:
        eng.set_clipping(*clipping)
    eng.reset()
    if place:                                        # hand-placed cubes at the boundary (place_cubes_at_the_boundary), the same on every backend
        place_cubes_at_the_boundary(eng, cfg.model)
    snaps = [snapshot(eng)]
    for t in range(steps):
        act = actions_for(t, n, eng.action_dim, seed).to(device)
        eng.step(act)
        snaps.append(snapshot(eng))
    eng.close()
    return snaps


def assert_bit_equal(a, b, what, skip_rows=None):
    for k in PER_ENV_FIELDS:
        x, y = a[k], b[k]
        if k == "state" and skip_rows is not None:
            x, y = x.copy(), y.copy()
            for rows in (skip_rows if isinstance(skip_rows, (list, tuple)) else [skip_rows]):
                x[rows] = 0
                y[rows] = 0
        if x.dtype.kind == "f":
            same = (x.view(np.uint32) == y.view(np.uint32)) | (np.isnan(x) & np.isnan(y))
        else:
            same = x == y
        if not np.all(same):
            bad = np.argwhere(~same)
            i = tuple(bad[0])
            raise AssertionError(
                f"{what}: `{k}` differs at {len(bad)} element(s); first {i}: got={x[i]!r} want={y[i]!r}")
    np.testing.assert_allclose(a["info"], b["info"], rtol=2e-5, atol=2e-4, err_msg=f"{what}: info")


# ---- the matrix of built step-kernel units (tests/test_parity_unit_matrix.py) ---------------------------------------------------------------
# A family is the row (dr, surf, ext) of the host's table of units (unit_for in csrc/trifinger_hip.hip); the value is the prefix of its units' names.
# (1, 1, 0) launches the same s0_* units as (0, 1, 0) - they keep domain randomisation as a run-time flag - with the flag set.
MATRIX_FAMILIES = {(0, 0, 0): "0", (0, 0, 2): "2", (0, 1, 0): "s0", (1, 0, 0): "d0", (1, 0, 1): "1", (1, 0, 2): "d2", (1, 1, 0): "s0", (1, 1, 1): "s1"}
MATRIX_N, MATRIX_STEPS, MATRIX_EPISODE, MATRIX_SEED = 130, 36, 12, 3     # two full wavefronts and a ragged one of 2 lanes; three episodes of 12 steps
MATRIX_PLACE_FIRST = 65                                                  # the second and third wavefront start at the boundary
MATRIX_BOX = ([0.02, 0.08, 0.02], 500.0)
MATRIX_SUCCESS = {"activate": True, "bonus": 10.0, "position_tolerance": 0.08, "orientation_tolerance": 3.2}
MATRIX_BASE_DR = dict(CONFIGS["d4_domain_randomization"]["domain_randomization"])            # action_repeat_prob 0.2 among it
MATRIX_EXT_DR = dict(CONFIGS["d4_domain_randomization_extended"]["domain_randomization"], action_repeat_prob=0.2)
MATRIX_SPLIT_SKIP_ROWS = [slice(66, 84), slice(157, 172)]   # rows 66.. (wrench accumulators) are written by the split path only, rows 157.. (samples of
                                                            # the next reset) by the fused step only; info[9] (number of resets) is counted by the fused step only


def matrix_model(lib, family):
    """the collision model that selects `family`: the general box (ext 2), the low-ring model with the surface normal (surf), else the default"""
    _, surf, ext = family
    if ext == 2:
        return lib.box_model(*MATRIX_BOX)
    return surface_model(lib, low_ring=True) if surf else lib.default_model()


def matrix_engine(lib, device, family, a, asym, variant=None, n=MATRIX_N, episode_length=MATRIX_EPISODE):
    """one engine of the matrix cell (family, A = `a`, ASYM = `asym`), not yet reset; `variant` is forced and must be accepted; `n`, `episode_length`:
    the matrix's own unless given (tests/test_guard_bands*.py: smaller populations, shorter episodes)"""
    dr, _, ext = family
    kw = dict(command_mode={9: "torque", 18: "position_impedance"}[a], asymmetric_obs=bool(asym), task_difficulty=4, reward_terms=D4_REWARDS,
              robot_reset="random", dof_pos_stddev=0.6, dof_vel_stddev=0.3, success=MATRIX_SUCCESS, model=matrix_model(lib, family))
    if dr:
        kw["domain_randomization"] = MATRIX_EXT_DR if ext == 1 else MATRIX_BASE_DR
    eng = TrifingerEngine(make_config(lib, n, seed=MATRIX_SEED, episode_length=episode_length, **kw), device=device, lib=lib)
    assert eng.action_dim == a
    if variant is not None:
        eng.kernel_variant = variant
        assert eng.kernel_variant == variant
    return eng


def matrix_rollout(lib, device, family, a, asym, path, variant=None):
    """The rollout of one matrix cell: the snapshot after the reset (cube families: with the cubes of envs 65.. placed at the boundary) and after each
    of the 36 steps.  `path`: "step" (tf_step with actions_for), "rand" (tf_step_random) or "split" (the five entries of the split path, same actions
    as "step")."""
    assert path in ("step", "rand", "split"), path
    eng = matrix_engine(lib, device, family, a, asym, variant)
    eng.reset()
    if family[2] != 2:                               # the box families are not placed
        place_cubes_at_the_boundary(eng, eng.cfg.model, first=MATRIX_PLACE_FIRST)
    snaps = [snapshot(eng)]
    for t in range(MATRIX_STEPS):
        if path == "rand":
            eng.step_random()
        else:
            act = actions_for(t, MATRIX_N, a, MATRIX_SEED).to(device)
            if path == "step":
                eng.step(act)
            else:
                eng.action_buf.copy_(act)
                eng.apply_resets()
                eng.pre_step()
                eng.simulate()
                eng.post_step()
                eng.finish_step()
        snaps.append(snapshot(eng))                  # (the copies to the host synchronise)
    eng.close()
    return snaps


def assert_split_equals_fused(split, fused, what):
    """assert_bit_equal with the exceptions test_split_path_equals_fused documents (MATRIX_SPLIT_SKIP_ROWS, info[9]); neither snapshot is changed"""
    a, b = dict(split), dict(fused)
    a["info"], b["info"] = a["info"].copy(), b["info"].copy()
    a["info"][9] = b["info"][9] = 0.0
    assert_bit_equal(a, b, what, skip_rows=MATRIX_SPLIT_SKIP_ROWS)


def matrix_reach(snaps, family, m):
    """What the rollout `snaps` of a matrix cell touched, counted from its snapshots (the one after the reset is the reference of the first
    difference only): env-steps with a live finger-cube slot (TF_S_FC_LINK, low two bits), with at least two, with a boundary contact (TF_S_CW_FACE),
    with live cone rows (cone_census on model `m`; surface families), time-outs (the env's step counter falls), goal resets, non-finite states
    counted by the step; and for the families with domain randomisation whether the six factor rows ever leave 1.0 and the env-steps in which a
    non-zero applied torque repeats that of the previous snapshot bit for bit (action repeat)."""
    from leibnizgym_amd import _capi as capi
    dr, surf, _ = family
    st = np.stack([s["state"] for s in snaps])                                        # (1 + steps, rows, n)
    live = ((st[1:, capi.S_FC_LINK:capi.S_FC_LINK + 3].astype(np.int64) & 3) != 0).sum(axis=1)
    steps = np.stack([s["steps"] for s in snaps])
    r = dict(live_fc=int((live >= 1).sum()), two_live=int((live >= 2).sum()), boundary=int((st[1:, capi.S_CW_FACE] != 0).sum()),
             timeouts=int((steps[1:] < steps[:-1]).sum()), goal_resets=int(sum(s["goal_reset_buf"].sum() for s in snaps[1:])),
             nonfinite=float(sum(s["info"][capi.INFO_NUM_NONFINITE] for s in snaps[1:])))
    if surf:
        r["cone"] = int(sum(cone_census(s, m).sum() for s in st[1:]))
    if dr:
        tau = st[:, capi.S_TAU:capi.S_TAU + 9].view(np.uint32)
        r["factors_drawn"] = bool((st[1:, capi.S_DR:capi.S_DR + 6] != 1.0).any())
        r["tau_repeats"] = int(((tau[1:] == tau[:-1]).all(axis=1) & (st[1:, capi.S_TAU:capi.S_TAU + 9] != 0).any(axis=1)).sum())
    return r
