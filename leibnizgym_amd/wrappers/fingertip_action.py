"""Fingertip-space actions for a TriFinger env: the policy (or script) commands the three fingertips, the env still receives its native action.

`FingertipActionEnv` wraps a `TrifingerEnv` or a `VecTaskPython`.  Per control step it forms the env's native action [N, 9] from the fingertip command
with ONE launch of `tfk_tip_action` (include/trifinger_kin.h) on the engine's own state rows and hands it to the inner `step`: no host synchronisation, no
copy.  On an engine that is not on a GPU (the injected CPU library of the tests) - or with ``fused=False`` - the torch statement of the same law runs
instead (leibnizgym_amd/kinematics.py: tip_action_statement).  An extension: the reference has no Cartesian action space.
"""
import torch

from .. import _capi as capi
from .. import kinematics as kin
from ..evaluate import engine_of

_MODE_OF = {capi.COMMAND_MODES["position"]: "position", capi.COMMAND_MODES["torque"]: "torque"}


class FingertipActionEnv:
    """frame "delta": the command moves each tip by delta_scale x cmd metres from where it is; "absolute": cmd in [-1, 1]^3 spans the target box.  The
    box is stated for finger 0 and turned with each finger's azimuth.  mode None follows the env's command_mode ("position": the action is a joint target
    from a few damped-least-squares iterations; "torque": a Cartesian PD law through the Jacobian transpose with gravity compensation).  **params: the
    keys of kinematics.DEFAULT_ACTION.  `last_target` holds the world targets x_des [N, 9] of the last step.  Everything else is the inner env's.

    Position mode and the control step: the env's own joint PD law (kp 10, kd 0.001 on the distal joint) closes the loop behind the joint target, and at the
    default control step of 20 ms it does not settle even for a FIXED joint target - the distal joint rings at the velocity limit, whatever this wrapper
    commands.  The tips track in position mode at `sim.dt` 0.005 (what the tests use); at the default step use torque mode, which converges."""

    def __init__(self, env, frame="delta", mode=None, fused=None, normalize_action=None, **params):
        try:
            eng = engine_of(env)
        except ValueError as exc:
            raise ValueError(f"FingertipActionEnv: {type(env).__name__} has no native engine behind it; it wraps TrifingerEnv or VecTaskPython") from exc
        cm = int(eng.cfg.command_mode)
        if cm == capi.COMMAND_MODES["position_impedance"] or eng.action_dim != 9:
            raise ValueError("FingertipActionEnv: command_mode position_impedance (18 actions) is not served; use position or torque")
        env_mode = _MODE_OF[cm]
        if mode is not None and mode != env_mode:
            raise ValueError(f"FingertipActionEnv: mode {mode!r} but the env's command_mode is {env_mode!r}")
        env_norm = bool(eng.cfg.normalize_action)
        if normalize_action is not None and bool(normalize_action) != env_norm:
            raise ValueError(f"FingertipActionEnv: normalize_action={bool(normalize_action)} but the env's normalize_action is {env_norm}; the action "
                             "would be read in the wrong units")
        self.env, self.engine = env, eng
        self.frame, self.mode = frame, env_mode
        if "gravity" not in params:
            params["gravity"] = tuple(float(g) for g in eng.cfg.gravity)
        self._cparams, self.params = kin.action_params(frame, env_mode, env_norm, **params)
        on_gpu = eng.device.type == "cuda"
        self.fused = on_gpu if fused is None else bool(fused)
        if self.fused and not on_gpu:
            raise ValueError(f"FingertipActionEnv: fused=True needs an engine on a GPU, this one is on {eng.device}")
        n = eng.num_envs
        self._q, self._qd = eng.q.T, eng.qd.T                       # [N, 9] views of the state rows: the kernel reads them where they are
        self._off = kin.base_offset_rows(eng) if eng.cfg.dr_enable else None
        self._action = torch.zeros((n, 9), dtype=torch.float32, device=eng.device)
        self.last_target = torch.zeros((n, 9), dtype=torch.float32, device=eng.device)
        self.constants = kin.model_constants(eng.cfg.model)
        self._kin = kin.FingerKinematics(eng.cfg.model, device=eng.device) if self.fused else None

    def __getattr__(self, name):                                    # the rest of the env interface
        if name == "env":                                           # (before __init__ has set it: no recursion)
            raise AttributeError(name)
        return getattr(self.env, name)

    def native_action(self, cmd):
        """the env's native action [N, 9] for the fingertip command [N, 9] at the engine's present state (the wrapper's own buffer, overwritten by the
        next call); `last_target` receives x_des"""
        eng = self.engine
        if not isinstance(cmd, torch.Tensor) or cmd.dtype != torch.float32 or cmd.device != eng.device:
            raise ValueError(f"cmd: a float32 tensor on {eng.device} (the command is read where it is: nothing is converted or copied), got "
                             f"{getattr(cmd, 'dtype', type(cmd).__name__)} on {getattr(cmd, 'device', 'the host')}")
        if tuple(cmd.shape) != (eng.num_envs, 9):
            raise ValueError(f"Invalid shape for tensor `cmd`. Input: {tuple(cmd.shape)} != {(eng.num_envs, 9)}.")
        if self.fused:
            self._kin.tip_action(self._cparams, cmd, self._q, self._qd, self._action, self.last_target, base_offset=self._off)
        else:
            a, t = kin.tip_action_statement(self.constants, self.params, cmd, self._q, self._qd, self._off)
            self._action.copy_(a)
            self.last_target.copy_(t)
        return self._action

    def step(self, cmd):
        return self.env.step(self.native_action(cmd))

    def reset(self):
        return self.env.reset()

    def tip_positions(self):
        """[N, 9] view of the fingertip positions the step reports (TF_S_TIP_P)"""
        return self.engine.tip_pos.T
