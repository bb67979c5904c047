"""bench.py's plain run and `--dump-outputs DIR`: the arrays the timed path hands its caller, float32 / float64, within 64 MB (a fixed,
seeded sample of env rows beyond that), identical for identical arguments.  The snapshot itself is checked on the CPU oracle; the
benchmark runs on the GPU box."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _engine(oracle, n):
    import bench
    from leibnizgym_amd.engine import TrifingerEngine, make_config
    eng = TrifingerEngine(make_config(oracle, n, seed=7, **bench.workload_kwargs(True)), device="cpu", lib=oracle)
    eng.reset()
    for _ in range(3):
        eng.step_random()
    return eng


def test_snapshot_holds_the_step_outputs(oracle):
    import bench
    eng = _engine(oracle, 64)
    got = bench.snapshot_outputs(eng)
    assert set(got) == set(bench.DUMP_BUFFERS)
    for k, a in got.items():
        want = getattr(eng, k).numpy()
        assert a.dtype == (np.float64 if k == "steps" else np.float32), (k, a.dtype)
        assert a.shape == want.shape and np.array_equal(a, want.astype(a.dtype)), k
    assert got["obs"].shape == (64, eng.obs_dim) and got["states"].shape == (64, eng.states_dim)
    eng.close()


def test_snapshot_samples_fixed_rows_beyond_the_cap(oracle, monkeypatch):
    import bench
    eng = _engine(oracle, 256)
    monkeypatch.setattr(bench, "DUMP_MAX_BYTES", 32 << 10)
    a, b = bench.snapshot_outputs(eng), bench.snapshot_outputs(eng)
    rows = a["sampled_env_ids"].astype(np.int64)
    assert 0 < len(rows) < 256 and np.all(np.diff(rows) > 0)
    assert sum(x.nbytes for x in a.values()) <= 32 << 10
    for k in bench.DUMP_BUFFERS:
        assert np.array_equal(a[k], getattr(eng, k).numpy()[rows].astype(a[k].dtype)), k
        assert np.array_equal(a[k], b[k]), k
    eng.close()


def _bench(tmp_path, name, *extra):
    d = tmp_path / name
    p = subprocess.run([sys.executable, "bench.py", "--steps", "12", "--warmup", "2", "--envs", "4096", "--settle", "20",
                        "--dump-outputs", str(d)] + list(extra), cwd=REPO, capture_output=True, text=True, timeout=600)
    assert p.returncode == 0, p.stdout[-1500:] + p.stderr[-1500:]
    lines = [ln for ln in p.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, lines
    return json.loads(lines[0]), {f[:-4]: np.load(d / f) for f in sorted(os.listdir(d))}


@pytest.mark.gpu
def test_plain_run_times_the_headline_and_dumps_what_it_computed(hip, tmp_path):
    """A plain run prints the headline keys only (no roofline, no side legs, no CPU baseline); `--full` adds them.  Both step the same env
    population, so the outputs of their last timed step are the same bits."""
    plain, out_p = _bench(tmp_path, "plain")
    full, out_f = _bench(tmp_path, "full", "--full", "--no-cpu-baseline")
    for k in ("metric", "value", "unit", "higher_is_better", "dtype", "ms_per_step"):
        assert k in plain, k
    assert plain["steps"] == 12 and abs(plain["value"] - 4096 / (plain["ms_per_step"] * 1e-3)) < 1e-6 * plain["value"]
    for k in ("roofline", "value_resident_actions", "value_fast_contact_set", "cpu_baseline"):
        assert k not in plain, k
    assert "roofline" in full and full["value_fast_contact_set"] > 0
    assert set(out_p) == set(out_f) == set(["obs", "states", "reward", "reset_buf", "goal_reset_buf", "successes", "dones", "action_buf", "steps"])
    for k in out_p:
        assert out_p[k].dtype in (np.float32, np.float64) and out_p[k].shape[0] == 4096, k
        assert np.array_equal(out_p[k], out_f[k]), k
    assert np.isfinite(out_p["obs"]).all() and np.abs(out_p["action_buf"]).max() <= 1.0
