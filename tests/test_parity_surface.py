"""The four kernel units with the surface normal of the cube corners (TfModel.cube_wall_surface: s0_1, s0_2, s1_1, s1_2 - EXT 0 / 1, `wide` /
`wide_helpers`) must reproduce the oracle with the switch on BIT FOR BIT on every per-env output, no env excluded; info scalars to rtol 2e-5.

On the shipped boundary profile random rollouts almost never put a corner on the cone (11 of 576 000 env-steps), so most rollouts here run on the
LOW-RING model (parity_util.surface_model: wall_z[0] = -0.01, the vertical ring ends below the floor): a cube that slides to the boundary touches
the cone with its lower corners, and a tenth to a third of all env-steps run the surface rows.

Reach condition: every rollout asserts on the ORACLE's snapshots (never HIP's) that the cone block was exercised, by the geometric census of
parity_util.cone_census - a boundary contact (cw_face != 0) and a corner above wall_z[0] within contact_slack of the profile.  The oracle half of
every rollout runs on the CPU with the same bounds (test_reach_*: no GPU needed), so a change of the oracle, of the configs or of the placement that
loses the reach is seen without a GPU; the GPU tests apply the same helpers to the oracle leg they compare with.  Measured on the oracle (640 envs x
900 steps, 750-step episodes, seed 21, low ring: 63 compared steps = 40 320 env-steps):

    config                               env-steps on the cone     envs that ever had one
    d4_torque_asym                        5342 = 13.2 %            199
    d4_torque_asym, fused actions         5775 = 14.3 %            208
    d4_domain_randomization_extended      7562 = 18.8 %            251
    the same, fused actions               8122 = 20.1 %            255
    d4_domain_randomization              14943 = 37.1 %            460
    ff_middle_pairs                       5483 = 13.6 %            199

against the asserted 3 % and 100 envs.  The shipped profile: d4_torque_asym 11 env-steps of all 576 000 (3 envs), the extended DR 176 of 576 000
(14 envs) - these rollouts are compared after EVERY step, so that the rare events are among the compared ones.

What `changed` (envs whose census flag changes between compared snapshots) does and does not say: on the low-ring model every corner is above
wall_z[0] all the time, so a change is "no boundary rows <-> live cone rows" - by the hand placement in step 1, by a reset, by a cube that leaves the
wall - and never a corner that crosses wall_z[0] with live ring rows.  The hand-over of the warm-start rows between a corner's RING rows and its cone
rows is pinned by the rollouts on the shipped profile only (the two long ones and the eight short ones).
"""
import numpy as np
import pytest
import torch

import parity_util as pu
from leibnizgym_amd import _capi as capi
from leibnizgym_amd.engine import TrifingerEngine, make_config

DEV = "cuda:0"
SURF_VARIANTS = ("wide", "wide_helpers")


def _report(what, flags):
    hit, total, envs, changed = pu.census_summary(flags)
    print(f"\n{what}: {hit} of {total} compared env-steps with live cone rows (oracle census), {envs} envs, {changed} envs with a change")
    return hit, total, envs, changed


# ---- the rollouts and their reach conditions (shared by the CPU tests of the oracle legs and the GPU parity tests) ------------------------------
LONG_LEGS = [  # (config, low-ring model, actions drawn inside the launch: tf_step_random)
    ("d4_torque_asym", True, False), ("d4_torque_asym", True, True), ("d4_domain_randomization_extended", True, False),
    ("d4_domain_randomization_extended", True, True), ("d4_domain_randomization", True, False), ("ff_middle_pairs", True, False),
    ("d4_torque_asym", False, False), ("d4_domain_randomization_extended", False, False)]


def _assert_long_reach(low_ring, hit, total, envs):
    if low_ring:
        assert total == 63 * 640
        assert hit >= 0.03 * total and envs >= 100, (hit, total, envs)      # measured on the oracle: 13.2 % - 37.1 %, 199 - 460 envs (module docstring)
    else:
        assert total == 900 * 640 and hit >= 1, (hit, total)                 # measured on the oracle: 11 and 176 of 576 000


SETTINGS = [dict(substeps=1, solver_iterations=4), dict(substeps=3, solver_iterations=1), dict(dt=0.01, solver_iterations=12, control_decimation=3),
            dict(gravity=(0.3, -0.2, -3.7)), dict(normalize_action=False, apply_safety_damping=False), dict(solver_inner=2),
            dict(solver_iterations=3, solver_inner=3, substeps=1)]
RAGGED = [1, 4, 63, 64, 65]
SPLIT_CONFIGS = ["d4_domain_randomization", "d4_domain_randomization_extended"]

# arguments of pu.rollout per case.  "resets": the shipped profile, 40-step episodes, cone env-steps of the oracle's 131 000 measured per config, in
# the order of pu.CONFIGS: 17, 17, 161, 166, 13, 1558, 46, 56 (asserted: >= 1).  The others: cubes placed at the boundary of the low-ring model - they
# arrive on the cone in the first step (settings: 249 - 300 of the 300 envs have live cone rows from step 1 on; ragged: every env, up to the reset at
# step 40; split: 666 - 777 of 777; checkpoint: 223 of 256)
CASES = {f"resets-{c}": dict(n=1000, steps=130, cfg_name=c, surface="default") for c in pu.CONFIGS}
CASES.update({f"settings-{i}": dict(n=300, steps=50, cfg_name="envdefault_position", extra=e, surface="low_ring", place=True) for i, e in enumerate(SETTINGS)})
CASES.update({f"ragged-{n}": dict(n=n, steps=45, cfg_name="d4_torque_asym", surface="low_ring", place=True) for n in RAGGED})
CASES.update({f"split-{c}": dict(n=777, steps=70, cfg_name=c, seed=5, episode_length=30, surface="low_ring", place=True) for c in SPLIT_CONFIGS})
CASES["checkpoint"] = dict(n=256, steps=36, cfg_name="d4_domain_randomization_extended", surface="low_ring", place=True)
CHECKPOINT_STEP = 12


def _oracle_case(oracle, name):
    """the oracle's rollout of CASES[name], its census flags, and the reach condition of the case asserted on them"""
    kw = dict(CASES[name])
    n, steps, cfg_name = kw.pop("n"), kw.pop("steps"), kw.pop("cfg_name")
    want = pu.rollout(oracle, "cpu", n, steps, cfg_name, **kw)
    m = pu.surface_model(oracle, low_ring=kw["surface"] == "low_ring")
    flags = [pu.cone_census(s["state"], m) for s in want]
    hit, total, envs, changed = _report(name, flags)
    assert hit >= 1, (name, hit)                            # a live cone row ...
    if kw["surface"] == "low_ring":                         # ... and an env that goes from no boundary rows to live cone rows (module docstring)
        assert changed >= 1, (name, changed)
    if name == "checkpoint":                                # cone rows with impulses in TF_S_LAM_CW at the step the checkpoint is taken
        assert flags[CHECKPOINT_STEP].sum() >= n // 4 and (want[CHECKPOINT_STEP]["state"][capi.S_LAM_CW:capi.S_LAM_CW + 12] != 0).any()
    return want


def _case_engines(hip, name, variant, count):
    """`count` HIP engines of CASES[name] on `variant`, not yet reset"""
    c = CASES[name]
    kw = dict(pu.CONFIGS[c["cfg_name"]])
    engs = [TrifingerEngine(make_config(hip, c["n"], seed=c.get("seed", 3), episode_length=c.get("episode_length", 40),
                                        model=pu.surface_model(hip, c["surface"] == "low_ring"), **kw), device=DEV, lib=hip) for _ in range(count)]
    for e in engs:
        e.kernel_variant = variant
        assert e.kernel_variant == variant
    return engs


def _compare_case(hip, oracle, name):
    """CASES[name]: pu.rollout on every variant of the HIP library against the oracle's, compared after every step"""
    want = _oracle_case(oracle, name)
    kw = dict(CASES[name])
    n, steps, cfg_name = kw.pop("n"), kw.pop("steps"), kw.pop("cfg_name")
    for variant in SURF_VARIANTS:
        got = pu.rollout(hip, DEV, n, steps, cfg_name, variant=variant, **kw)
        for t, (a, b) in enumerate(zip(got, want)):
            pu.assert_bit_equal(a, b, f"{name} surface [{variant}] step {t}")


TAIL = dict(n=20000, tail=256, steps=45, seed=9, cfg_name="d4_domain_randomization")


def _oracle_tail(oracle):
    """the oracle shard of the last TAIL["tail"] envs of a population of TAIL["n"], cubes placed at the boundary of the low-ring model: its state and
    outputs after every step, reach asserted"""
    n, tail, seed = TAIL["n"], TAIL["tail"], TAIL["seed"]
    m = pu.surface_model(oracle, True)
    ref = TrifingerEngine(make_config(oracle, tail, seed=seed, episode_length=40, env_id_offset=n - tail, global_num_envs=n, model=m,
                                      **dict(pu.CONFIGS[TAIL["cfg_name"]])), device="cpu", lib=oracle)
    ref.reset()
    pu.place_cubes_at_the_boundary(ref, m)
    snaps = []
    for t in range(TAIL["steps"]):
        ref.step(pu.actions_for(t, tail, 9, seed))
        snaps.append(pu.snapshot(ref))
    ref.close()
    hit, _, _, changed = _report("tail shard of 20000 envs", [pu.cone_census(s["state"], m) for s in snaps])
    assert hit >= 1 and changed >= 1, (hit, changed)         # measured: 10208 of 11520 env-steps, all 256 envs
    return snaps


def _long_parity(hip, oracle, cfg_name, low_ring, fused_actions, n=640, steps=900, seed=21):
    """test_long_episodes_reach_the_boundary_and_stay_bit_exact with the switch on: the oracle and - with `hip` - both 256-register variants side by
    side, the low-ring model compared every 100 steps up to 300 and every 10 from there, the shipped profile after every step; the reach condition
    asserted on the oracle's snapshots.  hip = None: the oracle leg alone."""
    kw = dict(pu.CONFIGS[cfg_name])
    kw.pop("_clipping", None)
    ref = TrifingerEngine(make_config(oracle, n, seed=seed, episode_length=750, model=pu.surface_model(oracle, low_ring), **kw), device="cpu", lib=oracle)
    engs = {}
    for variant in SURF_VARIANTS if hip is not None else ():
        e = TrifingerEngine(make_config(hip, n, seed=seed, episode_length=750, model=pu.surface_model(hip, low_ring), **kw), device=DEV, lib=hip)
        e.kernel_variant = variant
        assert e.kernel_variant == variant
        engs[variant] = e
    m = pu.surface_model(oracle, low_ring)
    for e in (ref, *engs.values()):
        e.reset()
    flags = []
    for t in range(steps):
        if fused_actions:
            for e in (ref, *engs.values()):
                e.step_random()
        else:
            act = pu.actions_for(t, n, ref.action_dim, seed)
            ref.step(act)
            for e in engs.values():
                e.step(act.to(DEV))
        if not low_ring or t % 100 == 99 or (t >= 300 and t % 10 == 9):
            want = pu.snapshot(ref) if engs else None
            for variant, e in engs.items():
                pu.assert_bit_equal(pu.snapshot(e), want, f"{cfg_name} surface [{variant}] step {t}")
            flags.append(pu.cone_census(ref.state.numpy(), m))
    for e in (ref, *engs.values()):
        e.close()
    hit, total, envs, _ = _report(f"{cfg_name} {'low ring' if low_ring else 'shipped profile'}{' fused actions' if fused_actions else ''}", flags)
    _assert_long_reach(low_ring, hit, total, envs)


# ---- CPU: the oracle legs reach the cone -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cfg_name,low_ring,fused_actions", LONG_LEGS)
def test_reach_of_the_long_rollouts_on_the_oracle(oracle, cfg_name, low_ring, fused_actions):
    _long_parity(None, oracle, cfg_name, low_ring, fused_actions)


@pytest.mark.parametrize("name", list(CASES))
def test_reach_of_the_short_and_placed_rollouts_on_the_oracle(oracle, name):
    _oracle_case(oracle, name)


def test_reach_of_the_tail_shard_on_the_oracle(oracle):
    _oracle_tail(oracle)


# ---- GPU: long rollouts ------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("cfg_name,fused_actions", [(c, f) for c, low, f in LONG_LEGS if low])
def test_long_episodes_on_the_low_ring_model_stay_bit_exact(hip, oracle, cfg_name, fused_actions):
    """units s0_* (d4_torque_asym, d4_domain_randomization: restitution / friction / cube-size DR, ff_middle_pairs) and s1_* (extended DR: stage
    offset and per-body friction in the cone rows); `fused_actions`: through tf_step_random, both variants"""
    _long_parity(hip, oracle, cfg_name, True, fused_actions)


@pytest.mark.gpu
@pytest.mark.parametrize("cfg_name", [c for c, low, _ in LONG_LEGS if not low])
def test_long_episodes_on_the_shipped_profile_stay_bit_exact(hip, oracle, cfg_name):
    """the shipped geometry: rare events, with upper corners that cross from the ring to the cone"""
    _long_parity(hip, oracle, cfg_name, False, False)


# ---- GPU: short rollouts with resets -----------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("cfg_name", list(pu.CONFIGS))
def test_rollout_with_resets_bit_exact(hip, oracle, cfg_name):
    """test_rollout_bit_exact with the switch on, shipped profile: the reset launches and the launch modes that do not simulate go to the plain
    WIDE = 1 unit while the simulating ones go to the unit with the surface rows.  Every one of these rollouts has env-steps with live cone rows
    (CASES: 13 to 1558 of 131 000, asserted >= 1 on the oracle's snapshots).  No config of parity_util.CONFIGS is refused with the switch (none uses
    the general box); what is refused is asserted in test_what_the_surface_units_refuse."""
    _compare_case(hip, oracle, f"resets-{cfg_name}")


@pytest.mark.gpu
def test_what_the_surface_units_refuse(hip, oracle):
    """the 128-register kernels and the general box are not built with the switch - and both libraries say so in the same way for the box"""
    kw = dict(pu.CONFIGS["d4_torque_asym"])
    eng = TrifingerEngine(make_config(hip, 1000, model=pu.surface_model(hip), **kw), device=DEV, lib=hip)
    with pytest.raises(NotImplementedError):
        eng.kernel_variant = "narrow"
    eng.close()
    for lib, dev in ((hip, DEV), (oracle, "cpu")):
        with pytest.raises(NotImplementedError):
            TrifingerEngine(make_config(lib, 64, model=pu.surface_model(lib, base=lib.box_model([0.02, 0.08, 0.02], 500.0)), **kw), device=dev, lib=lib)
        bad = lib.default_model()
        bad.cube_wall_surface = 2
        with pytest.raises(ValueError):
            TrifingerEngine(make_config(lib, 64, model=bad, **kw), device=dev, lib=lib)


# ---- GPU: solver and stepping settings, ragged sizes --------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("i", range(len(SETTINGS)))
def test_solver_and_stepping_settings_on_the_low_ring_model(hip, oracle, i):
    """the settings of test_solver_and_stepping_settings (SETTINGS[i]) with the cubes placed at the boundary of the low-ring model: they arrive on
    the cone in the first step, the resets at step 40 take them away again"""
    _compare_case(hip, oracle, f"settings-{i}")


@pytest.mark.gpu
@pytest.mark.parametrize("n", RAGGED)
def test_ragged_sizes_on_the_low_ring_model(hip, oracle, n):
    """placed cubes: every env has live cone rows from step 1 to the reset at step 40 (oracle census)"""
    _compare_case(hip, oracle, f"ragged-{n}")


@pytest.mark.gpu
def test_auto_picks_wide_above_the_helper_limit_and_matches_the_oracle(hip, oracle):
    """a population above TF_HELPERS_MAX_ENVS with the switch: TF_KERNEL_AUTO runs `wide`; its last 256 envs (cubes placed at the boundary of the
    low-ring model) equal an oracle shard of exactly those envs, as in test_maximum_size_matches_the_oracle_at_the_far_end"""
    n, tail, seed = TAIL["n"], TAIL["tail"], TAIL["seed"]
    want = _oracle_tail(oracle)
    big = TrifingerEngine(make_config(hip, n, seed=seed, episode_length=40, model=pu.surface_model(hip, True), **dict(pu.CONFIGS[TAIL["cfg_name"]])),
                          device=DEV, lib=hip)
    assert big.kernel_variant == "wide"
    big.reset()
    pu.place_cubes_at_the_boundary(big, pu.surface_model(oracle, True), first=n - tail)
    for t in range(TAIL["steps"]):
        act = torch.zeros(n, 9, device=DEV)
        act[n - tail:] = pu.actions_for(t, tail, 9, seed).to(DEV)
        big.step(act)
        for name in ("obs", "states", "reward", "reset_buf", "steps", "reset_count"):
            assert np.array_equal(getattr(big, name)[n - tail:].cpu().numpy(), want[t][name]), (t, name)
        a = big.state[:, n - tail:].cpu().numpy()
        assert np.array_equal(a.view(np.uint32), want[t]["state"].view(np.uint32)), (t, "state")
    big.close()


# ---- GPU: split path, checkpoint ------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("variant", SURF_VARIANTS)
@pytest.mark.parametrize("cfg_name", SPLIT_CONFIGS)
def test_split_path_equals_fused_on_the_low_ring_model(hip, oracle, cfg_name, variant):
    """tf_apply_resets / pre_step / simulate / post_step / finish_step == tf_step with the switch on (EXT 0 and 1): tf_simulate alone goes through the
    unit with the surface rows.  The fused HIP step also equals the oracle's rollout, whose census says the cone rows were live."""
    name = f"split-{cfg_name}"
    want = _oracle_case(oracle, name)
    c = CASES[name]
    engs = _case_engines(hip, name, variant, 2)
    m = pu.surface_model(oracle, True)
    for e in engs:
        e.reset()
        pu.place_cubes_at_the_boundary(e, m)
    for t in range(c["steps"]):
        act = pu.actions_for(t, c["n"], 9, c["seed"]).to(DEV)
        engs[0].step(act)
        e = engs[1]
        e.action_buf.copy_(act)
        e.apply_resets()
        e.pre_step()
        e.simulate()
        e.post_step()
        e.finish_step()
        torch.cuda.synchronize()
        a, b = pu.snapshot(engs[0]), pu.snapshot(engs[1])
        pu.assert_bit_equal(a, want[t + 1], f"{cfg_name} surface fused [{variant}] step {t}")
        # rows 66.. (wrench accumulators) are written by the split path only, rows 157.. (samples of the next reset) by the fused step only;
        # info[9] (number of resets) is only counted by the fused kernel
        a["info"][9] = b["info"][9] = 0.0
        pu.assert_bit_equal(a, b, f"{cfg_name} surface split vs fused [{variant}] step {t}", skip_rows=[slice(66, 84), slice(157, 172)])
    for e in engs:
        e.close()


@pytest.mark.gpu
@pytest.mark.parametrize("variant", SURF_VARIANTS)
def test_checkpoint_in_the_middle_of_a_cone_contact(hip, oracle, variant):
    """state_dict at a step where the oracle's census has live cone rows (their impulses live in TF_S_LAM_CW: _oracle_case), load_state_dict into a
    fresh engine: the continuation equals the uninterrupted rollout and the oracle's, bit for bit"""
    want = _oracle_case(oracle, "checkpoint")
    c = CASES["checkpoint"]
    n, seed = c["n"], 3
    a, b = _case_engines(hip, "checkpoint", variant, 2)
    a.reset()
    pu.place_cubes_at_the_boundary(a, pu.surface_model(oracle, True))
    for t in range(CHECKPOINT_STEP):
        a.step(pu.actions_for(t, n, a.action_dim, seed).to(DEV))
    pu.assert_bit_equal(pu.snapshot(a), want[CHECKPOINT_STEP], f"checkpoint [{variant}] before saving")
    b.load_state_dict(a.state_dict())
    for t in range(CHECKPOINT_STEP, c["steps"]):
        act = pu.actions_for(t, n, a.action_dim, seed).to(DEV)
        a.step(act), b.step(act)
        pu.assert_bit_equal(pu.snapshot(b), want[t + 1], f"checkpoint [{variant}] restored, step {t}")
        pu.assert_bit_equal(pu.snapshot(a), want[t + 1], f"checkpoint [{variant}] uninterrupted, step {t}")
    a.close(), b.close()
