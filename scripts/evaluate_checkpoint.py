#!/usr/bin/env python3
"""Episode statistics of a checkpoint on the native TriFinger env, at env speed (leibnizgym_amd/evaluate.py; PPOTrainer.evaluate).

    python scripts/evaluate_checkpoint.py gym=trifinger_difficulty_4 checkpoint=run/nn/trifinger.pth num_envs=8192 episodes_per_env=2
                                          [pos_tol=0.02] [ori_tol=0.2] [stochastic=1] [max_steps=N] [further overrides of the config tree]
                                          [--record SELECT] [--record-max K] [--record-every E]
                                          [--record-dir DIR] [--record-frames]

The env is built the way scripts/train_ppo.py builds it, the checkpoint restored, every env run for `episodes_per_env` whole episodes under the
deterministic action (stochastic=1: mu + sigma * noise), and the result printed as ONE JSON line: success rate at the end of an episode, final position and
orientation error (mean, median and 90 % bins), episode return and length, time at the goal and time to reach it.  The network shape and the normalisation
switches are taken from the checkpoint where it records them; everything else from the agent tree.  Launched by torch.distributed.run, every rank
evaluates its shard and the statistics are summed over the ranks; rank 0 prints.

With --record SELECT (failure, success, nonfinite, or a `|`-joined set such as "failure|nonfinite") the episodes that end as selected are captured on the device (leibnizgym_amd/record.py: the last steps of every env's current episode, frozen
in place at a selected end) and every rank writes its first K of them (--record-max, ascending env id; default 16) to DIR/episodes.npz
(DIR/episodes_rank<r>.npz in a distributed run; --record-dir, default "recordings"): numbers only, read back with leibnizgym_amd.record.load_npz.
--record-every E keeps every E-th step and the final one.  With --record-frames the episodes are also rendered, one PNG per recorded step
(DIR/ep<env>_<step>.png)."""
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch  # noqa: E402

from leibnizgym_amd.config import compose  # noqa: E402
from leibnizgym_amd.envs import TrifingerEnv  # noqa: E402
from leibnizgym_amd.ppo import PPOConfig, PPOTrainer  # noqa: E402
from leibnizgym_amd.utils.rlg_train import RlGamesGpuEnvAdapter  # noqa: E402
from leibnizgym_amd.wrappers import VecTaskPython  # noqa: E402

# what of a checkpoint's recorded PPOConfig decides whether its tensors fit the trainer that restores them
SHAPE_KEYS = ("units", "activation", "value_activation", "d2rl", "value_d2rl", "normalize_input", "normalize_input_value", "normalize_value")


def main(argv):
    own = {"checkpoint": None, "num_envs": None, "episodes_per_env": "1", "pos_tol": None, "ori_tol": None, "stochastic": "0", "max_steps": None}
    rec = {"--record": None, "--record-max": "16", "--record-every": "1", "--record-dir": "recordings"}
    frames, rest, argv = False, [], list(argv)
    while argv:
        a = argv.pop(0)
        if a == "--record-frames":
            frames = True
            continue
        flag, eq, val = a.partition("=")
        if flag in rec:
            if not eq:
                if not argv:
                    raise SystemExit(f"evaluate_checkpoint.py: {flag} needs a value")
                val = argv.pop(0)
            rec[flag] = val
            continue
        key, _, val = a.partition("=")
        if key in own:
            own[key] = val
        else:
            rest.append(a)
    if not own["checkpoint"]:
        raise SystemExit("evaluate_checkpoint.py: checkpoint=<path> is required")
    if own["num_envs"] is not None:
        rest.append(f"args.num_envs={int(own['num_envs'])}")
    cfg = compose(rest)
    world = int(os.environ.get("WORLD_SIZE", "1"))
    rank = int(os.environ.get("RANK", "0"))
    local = int(os.environ.get("LOCAL_RANK", "0"))
    dev = f"cuda:{local}"
    torch.cuda.set_device(local)
    launched = "RANK" in os.environ and "MASTER_PORT" in os.environ
    if world > 1 or launched:
        import torch.distributed as dist
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        os.environ.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
        dist.init_process_group("nccl", device_id=torch.device(dev))
    n = cfg["gym"]["num_instances"]                 # envs per GPU
    env = TrifingerEnv(config=cfg["gym"], device=dev, verbose=False, env_id_offset=rank * n, global_num_instances=world * n)
    adapter = RlGamesGpuEnvAdapter("rlgpu", n, env=VecTaskPython(env, rl_device=dev))
    pc = PPOConfig.from_rlg(cfg["rlg"], num_envs=n)
    recorded = torch.load(own["checkpoint"], map_location="cpu", weights_only=False).get("config") or {}
    for k in SHAPE_KEYS:
        if k in recorded:
            setattr(pc, k, recorded[k])
    tr = PPOTrainer(adapter, env.get_obs_dim(), env.get_state_dim(), env.get_action_dim(), pc, device=dev)
    tr.restore(own["checkpoint"])
    res = tr.evaluate(episodes_per_env=int(own["episodes_per_env"]), deterministic=own["stochastic"] in ("0", "", "false", "False"),
                      max_steps=int(own["max_steps"]) if own["max_steps"] else None,
                      pos_tol=float(own["pos_tol"]) if own["pos_tol"] else None, ori_tol=float(own["ori_tol"]) if own["ori_tol"] else None,
                      record={"select": rec["--record"], "every": int(rec["--record-every"]), "max_episodes": int(rec["--record-max"])}
                      if rec["--record"] else None)
    if rec["--record"]:
        from leibnizgym_amd import record as rc
        path = os.path.join(rec["--record-dir"], "episodes.npz" if world == 1 else f"episodes_rank{rank}.npz")
        rc.save_npz(path, tr.last_recording)
        res["recording"] = path
        if frames and tr.last_recording:
            from leibnizgym_amd.render import SceneRenderer
            renderer = SceneRenderer(env._engine.cfg.model, device=dev)
            renderer.set_camera()
            for ep in tr.last_recording:
                rc.replay_frames(ep, renderer, out_dir=rec["--record-dir"])
            renderer.close()
    res.update(checkpoint=own["checkpoint"], num_envs=world * n, epoch=tr.epoch, frames=tr.frames)
    if rank == 0:
        print(json.dumps(res), flush=True)
    if world > 1 or launched:
        dist.destroy_process_group()


if __name__ == "__main__":
    main(sys.argv[1:])
