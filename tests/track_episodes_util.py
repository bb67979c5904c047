"""Shared by tests/test_track_episodes.py and tests/test_track_episodes_gpu.py: a scripted sequence of engine buffers and the naive per-env statement of
include/trifinger_ppo_track.h in plain Python.

The scripted poses are chosen so that the final errors are EXACT in every arithmetic: the goal sits a Pythagorean offset (3 k, 4 k, 0) / 1024 m (axes
permuted) from the cube, so e_p = 5 k / 1024 with every intermediate exact, and the goal's orientation is the cube's or the cube's turned by pi about x, so
the relative quaternion has a vector part of norm exactly 0 or 1 and e_o is 0 or float32(pi).  The naive loop can therefore form them in float64 and still
owe every integer of the accumulator; general poses are the business of the trainer tests, which compare the two implementations of the device functions."""
import math
from types import SimpleNamespace

import numpy as np
import torch

from leibnizgym_amd import _capi as capi
from leibnizgym_amd import evaluate as ev

STEPS, EP_LEN = 40, 10
POS_TOL, ORI_TOL, RULE = 0.02, 0.25, 1
INF_AT, NAN_POSE_AT = (12, 4), (19, 5)          # (step, env % 8): an infinite reward; a NaN in the cube's quaternion at an ending step


def script(n, seed=0):
    """STEPS steps of buffers for n envs, lists of CPU tensors: state [TF_STATE_ROWS, n], reward [n], reset_buf [n] bool, steps [n] int64, done [n] bool.
    By env % 8: 0 starts in the middle of an episode (s = 4 at the first step: its first end is UNARMED), 1 starts fresh and only times out, 2 terminates
    in the first step of an episode now and then (episodes of length 1), 3 terminates at s = 3 (a termination that is no time-out), 4 receives an infinite
    reward once, 5 a NaN quaternion at an ending step, 6 and 7 start mid-episode at other phases.  Every env times out at s = EP_LEN."""
    g = torch.Generator().manual_seed(1000 + seed)
    i = torch.arange(n)
    kind = i % 8
    s = torch.tensor([3, 0, 0, 0, 0, 0, 6, 8])[kind].to(torch.int64)          # the count BEFORE the first step
    out = []
    for t in range(STEPS):
        s = s + 1
        term = ((kind == 2) & (s == 1) & ((t // 3 + i // 8) % 2 == 0)) | ((kind == 3) & (s == 3))
        reset = term | (s >= EP_LEN)
        reward = (torch.randn(n, generator=g) * 3.0).float()
        if t == INF_AT[0]:
            reward[kind == INF_AT[1]] = float("inf")
        k = (7 * t + 3 * i) % 9                                               # e_p = 5 k / 1024: k <= 4 is inside the tolerance of 0.02 m
        st = torch.zeros(capi.TF_STATE_ROWS, n)
        cp = (torch.randint(-64, 64, (3, n), generator=g).float()) / 1024.0
        off = torch.stack([3.0 * k, 4.0 * k, 0.0 * k]).float() / 1024.0
        off = torch.where((i % 2 == 0).unsqueeze(0), off, off.flip(0))
        cq = torch.zeros(4, n)
        cq[3] = 1.0
        gq = cq.clone()
        turned = (t + i) % 3 == 0                                             # the goal turned by pi about x: (1, 0, 0, 0)
        gq[0, turned], gq[3, turned] = 1.0, 0.0
        if t == NAN_POSE_AT[0]:
            cq[1, kind == NAN_POSE_AT[1]] = float("nan")
        st[capi.S_CUBE_P:capi.S_CUBE_P + 3], st[capi.S_GOAL_P:capi.S_GOAL_P + 3] = cp, cp + off
        st[capi.S_CUBE_Q:capi.S_CUBE_Q + 4], st[capi.S_GOAL_Q:capi.S_GOAL_Q + 4] = cq, gq
        out.append(dict(state=st, reward=reward, reset_buf=reset.clone(), steps=s.clone(), done=(torch.rand(n, generator=g) < 0.3)))
        s = torch.where(reset, torch.zeros_like(s), s)
    return out


def fake_engine(n, device):
    return SimpleNamespace(state=torch.zeros(capi.TF_STATE_ROWS, n, device=device), reward=torch.zeros(n, device=device),
                           reset_buf=torch.zeros(n, dtype=torch.bool, device=device), goal_reset_buf=torch.zeros(n, dtype=torch.bool, device=device),
                           steps=torch.zeros(n, dtype=torch.int64, device=device))


def load(engine, rec):
    for k in ("state", "reward", "reset_buf", "steps"):
        getattr(engine, k).copy_(rec[k])


def _fixed(x, lo, hi, scale):
    return int(round(min(max(float(x), lo), hi) * scale))                    # the product is exact in float64; round() rounds halves to even


class Naive:
    """the statement of include/trifinger_ppo_track.h, one env at a time; `events` lists what happened at every end"""

    def __init__(self, n, pos_tol=POS_TOL, ori_tol=ORI_TOL, rule=RULE, ep_len=EP_LEN):
        self.n, self.pos_tol, self.ori_tol, self.rule, self.ep_len = n, np.float32(pos_tol), np.float32(ori_tol), rule, ep_len
        self.ret, self.armed = np.zeros(n, np.float32), np.zeros(n, np.int32)
        self.acc = [0] * ev.TRACK_ACC
        self.events = []

    def errors(self, st, i):
        cp, cq = st[capi.S_CUBE_P:capi.S_CUBE_P + 3, i].astype(np.float64), st[capi.S_CUBE_Q:capi.S_CUBE_Q + 4, i].astype(np.float64)
        gp, gq = st[capi.S_GOAL_P:capi.S_GOAL_P + 3, i].astype(np.float64), st[capi.S_GOAL_Q:capi.S_GOAL_Q + 4, i].astype(np.float64)
        e_p = math.sqrt(float(((cp - gp) ** 2).sum()))
        x1, y1, z1, w1 = cq
        x2, y2, z2, w2 = -gq[0], -gq[1], -gq[2], gq[3]                      # cube (x) conj(goal)
        v = (w1 * x2 + x1 * w2 + y1 * z2 - z1 * y2, w1 * y2 - x1 * z2 + y1 * w2 + z1 * x2, w1 * z2 + x1 * y2 - y1 * x2 + z1 * w2)
        nrm = math.sqrt(v[0] ** 2 + v[1] ** 2 + v[2] ** 2)
        qfinite = bool(np.isfinite(cq).all() and np.isfinite(gq).all())
        e_o = 2.0 * math.asin(min(nrm, 1.0)) if qfinite else math.pi
        return np.float32(e_p), np.float32(e_o), qfinite

    def update(self, rec):
        st, r, rb, s = rec["state"].numpy(), rec["reward"].numpy(), rec["reset_buf"].numpy(), rec["steps"].numpy()
        a = self.acc
        with np.errstate(invalid="ignore", over="ignore"):
            for i in range(self.n):
                if s[i] == 1:
                    self.ret[i], self.armed[i] = r[i], 1
                else:
                    self.ret[i] = np.float32(self.ret[i] + r[i])
                if not rb[i]:
                    continue
                if self.armed[i]:
                    e_p, e_o, qfinite = self.errors(st, i)
                    pos_ok, ori_ok = bool(e_p <= self.pos_tol), bool(e_o <= self.ori_tol)
                    at_goal = pos_ok if self.rule == 0 else ((pos_ok and ori_ok) if self.rule == 1 else ori_ok)
                    tout = self.ep_len > 0 and s[i] >= self.ep_len
                    if np.isfinite(self.ret[i]) and np.isfinite(e_p) and np.isfinite(e_o) and qfinite:
                        a[ev.T_EPISODES] += 1
                        a[ev.T_SUCCESS] += at_goal
                        a[ev.T_POS_OK] += pos_ok
                        a[ev.T_ORI_OK] += ori_ok
                        a[ev.T_TIMEOUT] += bool(tout)
                        a[ev.T_SUM_LENGTH] += int(s[i])
                        a[ev.T_SUM_RETURN] += _fixed(self.ret[i], -ev.RETURN_MAX, ev.RETURN_MAX, ev.S_RETURN)
                        a[ev.T_SUM_POS_ERR] += _fixed(e_p, 0.0, ev.POS_ERR_MAX, ev.S_POS_ERR)
                        a[ev.T_SUM_ORI_ERR] += _fixed(e_o, 0.0, ev.ORI_ERR_MAX, ev.S_ORI_ERR)
                        self.events.append(("counted", int(s[i]), bool(tout)))
                    else:
                        a[ev.T_NONFINITE] += 1
                        self.events.append(("nonfinite", int(s[i]), bool(tout)))
                else:
                    a[ev.T_UNARMED] += 1
                    self.events.append(("unarmed", int(s[i]), False))
                self.ret[i], self.armed[i] = 0.0, 0

    def env_trk(self):
        return torch.stack([torch.from_numpy(self.ret.copy()).view(torch.int32), torch.from_numpy(self.armed.copy())])
