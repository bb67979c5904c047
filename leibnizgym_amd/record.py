"""A flight recorder for episodes: what answers "what happened in the episodes that failed?".

`EpisodeRecorder` binds to the buffers of a `TrifingerEngine` and is updated once per env step, behind the step, with no host synchronisation.  Per watched
env it keeps, on the device, a ring of the last `length` recorded steps of the current episode; when an episode ends in a selected way (failure, success,
non-finite) the env's ring is FROZEN IN PLACE - the recorder stops writing to that env until the host has harvested it with `take()`.  Nothing is copied,
nothing is handed from one workgroup to another and nothing depends on their order.  On the GPU an update is one launch of csrc/tf_eval.hip
(include/trifinger_ppo_record.h has the definitions and the layout of the buffers); `_update_torch` below is the plain-torch STATEMENT of the same
definitions - same buffers, same bits - and serves CPU tensors (the tests' oracle engines) and `fused=False`.  `replay_frames` renders a harvested episode
through the offscreen renderer, whose state matrix does not care whether its columns are envs or time steps.
"""
import os

import torch

from . import _capi as capi
from .evaluate import EngineObserver, episode_outcome

# include/trifinger_ppo_record.h
REC_STATE_ROWS = 59
REC_REWARD, REC_STEP, REC_ROWS = 59, 60, 61
ENV_STATE, ENV_COUNT, ENV_LENGTH, ENV_OUTCOME, ENV_RETURN, ENV_E_P, ENV_E_O, ENV_SPARE, ENV_ROWS = range(9)
IDLE, ARMED, FROZEN_STATE = 0, 1, 2
OUT_AT_GOAL, OUT_POS_OK, OUT_ORI_OK, OUT_TIMEOUT, OUT_NONFINITE = 1, 2, 4, 8, 16
SELECT = {"failure": 1, "success": 2, "nonfinite": 4}
ENDED_ARMED, FROZEN, UNARMED, RECORDS, ACC = range(5)

_OUT_NAMES = (("at_goal", OUT_AT_GOAL), ("pos_ok", OUT_POS_OK), ("ori_ok", OUT_ORI_OK), ("timeout", OUT_TIMEOUT), ("nonfinite", OUT_NONFINITE))
_NPZ_KEYS = ("env", "length", "count", "outcome_bits", "ret", "e_p", "e_o", "dr", "offsets", "records")


def parse_select(select):
    """the TFP_REC_SEL_* bits of a name, a `|`-joined set of names (failure, success, nonfinite) or an integer in 1..7"""
    if isinstance(select, int) and not isinstance(select, bool):
        bits = select
    else:
        names = [s.strip() for s in str(select).split("|")]
        unknown = [s for s in names if s not in SELECT]
        if unknown:
            raise ValueError(f"select: a `|`-joined set of {sorted(SELECT)}, got {select!r}")
        bits = 0
        for s in names:
            bits |= SELECT[s]
    if not 1 <= bits <= 7:
        raise ValueError(f"select: bits 1..7 ({SELECT}), got {select!r}")
    return bits


def decode_outcome(bits):
    return {k: bool(bits & b) for k, b in _OUT_NAMES}


class EpisodeRecorder(EngineObserver):
    """The last `length` recorded steps of the episodes of the first `watch` envs of `engine` (a TrifingerEngine, or anything with its buffer attributes)
    that end as `select` says: `update()` after every env step - no host synchronisation -, `take()` to harvest the frozen episodes, `counts()` for the
    integer counters, `reset()` to clear everything.  `every`: record the steps 1, 1 + every, ... of an episode and always its final step.  `length`
    defaults to ceil(episode_length / every) + 1: a whole episode; the tolerances, the at-goal rule and the episode length default to the engine's config
    as in `EpisodeStats`.  `fused`: None = the kernel where the buffers live on a GPU, the torch statement otherwise."""

    buffers = ("reward", "reset_buf", "steps")
    acc_size = ACC

    def __init__(self, engine, select="failure", every=1, length=None, watch=None, pos_tol=None, ori_tol=None, rule=None, fused=None, max_bytes=8 << 30,
                 episode_length=None):
        super().__init__(engine, pos_tol, ori_tol, rule, fused, episode_length)
        self.select = parse_select(select)
        self.every = int(every)
        if self.every < 1:
            raise ValueError(f"every {self.every} (>= 1)")
        n, dev = self.num_envs, self.acc.device
        self.watch = w = n if watch is None else int(watch)
        if not 1 <= w <= n:
            raise ValueError(f"watch = {watch}: the first `watch` of {n} envs, 1 .. {n}")
        if length is None:
            if self.ep_len <= 0:
                raise ValueError("an env without an episode length needs `length` (the ring defaults to a whole episode)")
            length = -(-self.ep_len // self.every) + 1
        self.length = L = int(length)
        if L < 1:
            raise ValueError(f"length = {length}: the ring holds at least one record")
        nbytes = 4 * L * REC_ROWS * w
        if nbytes > int(max_bytes):
            raise ValueError(f"the ring would take {nbytes} bytes ({nbytes / 2 ** 30:.2f} GiB = 4 x length {L} x {REC_ROWS} x watch {w}), more than "
                             f"max_bytes = {int(max_bytes)}: lower `watch` or `length`, raise `every`, or raise `max_bytes`")
        self.ring = torch.zeros((L, REC_ROWS, w), dtype=torch.float32, device=dev)
        self.hdr = torch.zeros((capi.TF_NUM_DR, w), dtype=torch.float32, device=dev)
        self.env_rec = torch.zeros((ENV_ROWS, w), dtype=torch.int32, device=dev)

    def reset(self):
        """forget everything: rings, headers, per-env state (frozen episodes included) and counters"""
        self.ring.zero_()
        self.hdr.zero_()
        self.env_rec.zero_()
        self.acc.zero_()

    def _launch(self):
        from . import ppo_kernels as pk
        e = self.engine
        pk.record_step(e.state, e.reward, e.reset_buf, e.steps, self.ring, self.hdr, self.env_rec, self.acc, self.every, self.select, self.ep_len,
                       self.pos_tol, self.ori_tol, self.rule)

    @torch.no_grad()
    def _update_torch(self):
        """the statement of include/trifinger_ppo_record.h in plain torch"""
        e, er, acc, w, L = self.engine, self.env_rec, self.acc, self.watch, self.length
        state = e.state[:, :w]
        r = e.reward[:w]
        s = e.steps[:w].to(torch.int64)
        s32 = s.clamp(0, 2 ** 31 - 1).to(torch.int32)
        rb = e.reset_buf[:w].to(torch.bool)
        st = er[ENV_STATE]
        live = st != FROZEN_STATE
        first = live & (s == 1)
        armed = live & (first | (st == ARMED))
        unarmed = live & ~armed & rb
        fzero = torch.zeros_like(r)
        ret = torch.where(first, fzero, er[ENV_RETURN].view(torch.float32)) + r
        cnt = torch.where(first, torch.zeros_like(st), er[ENV_COUNT])
        rec = armed & (rb | ((s32 - 1).to(torch.int64) % self.every == 0))
        ended = armed & rb
        e_p, e_o, pos_ok, ori_ok, at_goal, fin = episode_outcome(state, ret, self.pos_tol, self.ori_tol, self.rule)
        tout = (s >= self.ep_len) if self.ep_len > 0 else torch.zeros_like(rb)
        i32 = torch.int32
        outcome = (at_goal.to(i32) * OUT_AT_GOAL + pos_ok.to(i32) * OUT_POS_OK + ori_ok.to(i32) * OUT_ORI_OK + tout.to(i32) * OUT_TIMEOUT
                   + (~fin).to(i32) * OUT_NONFINITE)
        sel = torch.zeros_like(rb)
        if self.select & SELECT["failure"]:
            sel = sel | (fin & ~at_goal)
        if self.select & SELECT["success"]:
            sel = sel | (fin & at_goal)
        if self.select & SELECT["nonfinite"]:
            sel = sel | ~fin
        froze = ended & sel
        # the header of the episodes that start, the record into the slot (unsigned)COUNT % L of the lanes that record
        self.hdr.copy_(torch.where(first, state[capi.S_DR:capi.S_DR + capi.TF_NUM_DR], self.hdr))
        idx = rec.nonzero().flatten()
        if idx.numel():
            slot = (cnt[idx].to(torch.int64) & 0xFFFFFFFF) % L
            record = torch.cat([state[0:REC_STATE_ROWS, idx], r[idx].unsqueeze(0), s32[idx].view(torch.float32).unsqueeze(0)], 0)      # [REC_ROWS, k]
            self.ring[slot, :, idx] = record.t()
        er[ENV_COUNT] = torch.where(rec, cnt + 1, torch.where(first, torch.zeros_like(cnt), er[ENV_COUNT]))
        er[ENV_RETURN] = torch.where(armed, ret.view(i32), er[ENV_RETURN])
        nst = torch.where(ended, torch.where(froze, torch.full_like(st, FROZEN_STATE), torch.full_like(st, IDLE)), torch.full_like(st, ARMED))
        er[ENV_STATE] = torch.where(armed, nst, st)
        er[ENV_OUTCOME] = torch.where(ended, outcome, er[ENV_OUTCOME])
        er[ENV_LENGTH] = torch.where(froze, s32, er[ENV_LENGTH])
        er[ENV_E_P] = torch.where(froze, e_p.view(i32), er[ENV_E_P])
        er[ENV_E_O] = torch.where(froze, e_o.view(i32), er[ENV_E_O])
        acc[ENDED_ARMED] += ended.sum()
        acc[FROZEN] += froze.sum()
        acc[UNARMED] += unarmed.sum()
        acc[RECORDS] += rec.sum()

    def counts(self):
        """the counters as a dict of Python integers; the one synchronising read of `acc`"""
        raw = [int(x) for x in self.acc.cpu().tolist()]
        return {"ended_armed": raw[ENDED_ARMED], "frozen": raw[FROZEN], "unarmed": raw[UNARMED], "records": raw[RECORDS]}

    @torch.no_grad()
    def take(self, max_episodes=None):
        """Harvest the frozen episodes, in ascending env id, at most `max_episodes` of them (the others stay frozen): a list of dicts with `env`,
        `length` (the episode's steps), `count` (records written; the ring kept the last min(count, L)), `outcome` (decoded flags) and `outcome_bits`,
        `ret`, `e_p`, `e_o`, `dr` [TF_NUM_DR], `records` float32 [min(count, L), REC_ROWS] in chronological order and `steps` (the records' step
        numbers, int32) - CPU tensors and Python numbers.  The taken envs go back to idle and re-arm at their next first step.  Synchronises."""
        ids = (self.env_rec[ENV_STATE] == FROZEN_STATE).nonzero().flatten()
        if max_episodes is not None:
            ids = ids[:max(0, int(max_episodes))]
        if ids.numel() == 0:
            return []
        er = self.env_rec[:, ids].cpu()
        hdr = self.hdr[:, ids].cpu()
        ring = self.ring[:, :, ids].cpu()                                   # [L, REC_ROWS, k]
        L, out = self.length, []
        for j, env in enumerate(ids.cpu().tolist()):
            count = int(er[ENV_COUNT, j]) & 0xFFFFFFFF
            n = min(count, L)
            start = count % L if count > L else 0
            order = torch.tensor([(start + k) % L for k in range(n)], dtype=torch.int64)
            records = ring[order, :, j].contiguous()
            bits = int(er[ENV_OUTCOME, j])
            fl = er[:, j].contiguous().view(torch.float32)
            out.append({"env": env, "length": int(er[ENV_LENGTH, j]), "count": count, "outcome": decode_outcome(bits), "outcome_bits": bits,
                        "ret": float(fl[ENV_RETURN]), "e_p": float(fl[ENV_E_P]), "e_o": float(fl[ENV_E_O]), "dr": hdr[:, j].contiguous(),
                        "records": records, "steps": records[:, REC_STEP].contiguous().view(torch.int32).clone()})
        self.env_rec[ENV_STATE, ids] = IDLE
        return out


def save_npz(path, episodes):
    """the harvested episodes as one .npz of numbers: per-episode vectors, `dr` [K, TF_NUM_DR], all records stacked [sum, REC_ROWS] with `offsets` [K + 1]"""
    import numpy as np
    k = len(episodes)
    offsets = [0]
    for ep in episodes:
        offsets.append(offsets[-1] + int(ep["records"].shape[0]))
    records = torch.cat([ep["records"] for ep in episodes], 0) if k else torch.zeros((0, REC_ROWS))
    dr = torch.stack([ep["dr"] for ep in episodes], 0) if k else torch.zeros((0, capi.TF_NUM_DR))
    d = os.path.dirname(os.fspath(path))
    if d:
        os.makedirs(d, exist_ok=True)
    np.savez(path, env=np.array([ep["env"] for ep in episodes], dtype=np.int64), length=np.array([ep["length"] for ep in episodes], dtype=np.int64),
             count=np.array([ep["count"] for ep in episodes], dtype=np.int64), outcome_bits=np.array([ep["outcome_bits"] for ep in episodes], dtype=np.int64),
             ret=np.array([ep["ret"] for ep in episodes], dtype=np.float32), e_p=np.array([ep["e_p"] for ep in episodes], dtype=np.float32),
             e_o=np.array([ep["e_o"] for ep in episodes], dtype=np.float32), dr=dr.numpy().astype(np.float32), offsets=np.array(offsets, dtype=np.int64),
             records=records.numpy().astype(np.float32))


def load_npz(path):
    """the list `take()` returned, from a file `save_npz` wrote"""
    import numpy as np
    with np.load(path) as z:
        missing = [k for k in _NPZ_KEYS if k not in z.files]
        if missing:
            raise ValueError(f"{path}: not a recording (missing {missing})")
        a = {k: z[k] for k in _NPZ_KEYS}
    out = []
    for j in range(len(a["env"])):
        records = torch.from_numpy(a["records"][int(a["offsets"][j]):int(a["offsets"][j + 1])].copy())
        bits = int(a["outcome_bits"][j])
        out.append({"env": int(a["env"][j]), "length": int(a["length"][j]), "count": int(a["count"][j]), "outcome": decode_outcome(bits), "outcome_bits": bits,
                    "ret": float(a["ret"][j]), "e_p": float(a["e_p"][j]), "e_o": float(a["e_o"][j]), "dr": torch.from_numpy(a["dr"][j].copy()),
                    "records": records, "steps": records[:, REC_STEP].contiguous().view(torch.int32).clone()})
    return out


def replay_state(episode, device="cpu"):
    """the state matrix [TF_STATE_ROWS, T] of a harvested episode: time steps are the columns - rows 0 .. 58 from the records, the TF_S_DR rows from
    `dr` (every column the same), everything else zero"""
    records = episode["records"]
    t = int(records.shape[0])
    state = torch.zeros((capi.TF_STATE_ROWS, t), dtype=torch.float32)
    state[0:REC_STATE_ROWS] = records[:, 0:REC_STATE_ROWS].t()
    state[capi.S_DR:capi.S_DR + capi.TF_NUM_DR] = episode["dr"].to(torch.float32).unsqueeze(1)
    return state.to(device).contiguous()


@torch.no_grad()
def replay_frames(episode, renderer, out_dir=None, aux=False):
    """Render a harvested episode through a `render.SceneRenderer` (GPU only, like the renderer): the colour frames uint8 [T, H, W, 4], one per record,
    rendered in chunks of at most `renderer.max_views` views of the episode's state matrix (`replay_state`).  With `out_dir` the frames are also written
    as `ep<env>_<step:04d>.png`.  `aux=True` returns (color, depth, segmentation) instead.  The renderer's views are left on the last chunk."""
    from .render import write_png
    state = replay_state(episode, renderer.device)
    t = int(state.shape[1])
    color, depth, seg = [], [], []
    for c0 in range(0, t, renderer.max_views):
        renderer.set_views(range(c0, min(c0 + renderer.max_views, t)), t)
        o = renderer.render(state)
        color.append(o["color"].clone())
        if aux:
            depth.append(o["depth"].clone())
            seg.append(o["segmentation"].clone())
    if not color:
        raise ValueError("an episode without records has no frames")
    color = torch.cat(color, 0)
    if out_dir is not None:
        host = color.cpu()
        for k, s in enumerate(episode["steps"].tolist()):
            write_png(os.path.join(os.fspath(out_dir), f"ep{int(episode['env'])}_{int(s):04d}.png"), host[k])
    return (color, torch.cat(depth, 0), torch.cat(seg, 0)) if aux else color
