"""The guard-band harness (tests/guard_util.py) must be able to fail, and the oracle runs through it: no GPU needed.

First the planted defects: numpy "kernels" of y[M, N] = 2 x[M, N] that each do one thing wrong, on banded arrays, in both placements; `check` has to name
the array, the side and the offset.  Then the CPU oracle's rollouts with every engine buffer re-bound to a banded view (guard_util.band_engine), bit-equal
to the plain engine's - the harness at work in the CPU suite, and a band check of the oracle beside tests/test_oracle_sanitizer.py.  Last the completeness
of the GPU table (tests/test_guard_bands_gpu.py): every exported function that takes a `stream` is a row of it or is exempt with a reason.
"""
import glob
import os
import re

import numpy as np
import pytest
import torch

import guard_util as gu
import parity_util as pu
from oracle_util import REPO

M, N = 5, 7


def _arrays(placement, rows=M, cols=N):
    x0 = torch.arange(rows * cols, dtype=torch.float32).reshape(rows, cols) + 1.0
    x, hx = gu.banded_like(x0, "in", placement, name="x")
    y, hy = gu.banded((rows, cols), torch.float32, "cpu", "out", placement, name="y")
    return x, hx, y, hy


def _flat(h):
    """the whole allocation behind a handle as a float32 numpy array sharing its memory, and the view's first element in it"""
    return h.raw.view(torch.float32).numpy(), h.lo


def _good(hx, hy):
    (fx, lx), (fy, ly) = _flat(hx), _flat(hy)
    fy[ly:ly + M * N] = 2.0 * fx[lx:lx + M * N]


@pytest.mark.parametrize("placement", gu.PLACEMENTS)
def test_a_correct_kernel_passes(placement):
    x, hx, y, hy = _arrays(placement)
    assert x.data_ptr() % 256 == (0 if placement == "aligned" else 4) and y.data_ptr() % 16 == (0 if placement == "aligned" else 4)
    assert len(hy.raw) == 2 * gu.BAND_MIN + M * N and hy.lo == gu.BAND_MIN
    assert bool((hy.raw == gu.OUT_NAN_F32).all()) and bool(torch.isnan(y).all())              # bands AND interior of an output: the sentinel
    assert bool((hx.raw[:hx.lo] == gu.IN_NAN_F32).all()) and bool((hx.raw[hx.lo + M * N:] == gu.IN_NAN_F32).all())
    _good(hx, hy)
    gu.check([hx, hy])
    assert torch.equal(y, 2.0 * x)


def test_band_is_two_rows_of_a_wide_array():
    _, h = gu.banded((2, 5000), torch.float32, "cpu", "out", "offset", name="wide")
    assert h.lo == 10000 and len(h.raw) == 3 * 10000


def _caught(handles, *words):
    with pytest.raises(AssertionError) as e:
        gu.check(handles)
    msg = str(e.value)
    for w in words:
        assert w in msg, (w, msg)
    return msg


@pytest.mark.parametrize("placement", gu.PLACEMENTS)
def test_a_store_past_the_last_row_is_caught(placement):
    x, hx, y, hy = _arrays(placement)
    _good(hx, hy)
    fy, ly = _flat(hy)
    fy[ly + M * N] = 1.0
    msg = _caught([hx, hy], "band of `y`", "after", f"offset +{M * N} ", f"row {M}, column 0")
    assert "`x`" not in msg


@pytest.mark.parametrize("placement", gu.PLACEMENTS)
def test_a_store_before_the_first_row_is_caught(placement):
    x, hx, y, hy = _arrays(placement)
    _good(hx, hy)
    fy, ly = _flat(hy)
    fy[ly - 1] = 1.0
    _caught([hx, hy], "band of `y`", "before", "offset -1 ", f"row -1, column {N - 1}")


@pytest.mark.parametrize("placement", gu.PLACEMENTS)
def test_a_store_into_an_input_is_caught(placement):
    x, hx, y, hy = _arrays(placement)
    _good(hx, hy)
    fx, lx = _flat(hx)
    fx[lx + 2 * N + 3] = -1.0
    msg = _caught([hx, hy], "input `x`", "interior", f"offset +{2 * N + 3} ", "row 2, column 3")
    assert "`y`" not in msg
    fx[lx + 2 * N + 3] = 2 * N + 3 + 1.0                              # put back: the bits count, not the history
    gu.check([hx, hy])
    fx[lx + M * N + 2] = 0.0                                          # ... and an input's band
    _caught([hx, hy], "input `x`", "after", f"offset +{M * N + 2} ")


@pytest.mark.parametrize("placement", gu.PLACEMENTS)
def test_an_unwritten_last_column_is_caught(placement):
    x, hx, y, hy = _arrays(placement)
    fx, lx = _flat(hx)
    fy, ly = _flat(hy)
    for r in range(M):
        fy[ly + r * N:ly + r * N + N - 1] = 2.0 * fx[lx + r * N:lx + r * N + N - 1]
    _caught([hx, hy], "output `y`", "still holds the sentinel", f"offset +{N - 1} ", f"row 0, column {N - 1}")
    hy.full = False                                                  # an output the call is documented to leave partly unwritten
    gu.check([hx, hy])


@pytest.mark.parametrize("placement", gu.PLACEMENTS)
def test_a_load_past_the_end_masked_by_multiplication_is_caught(placement):
    """the defect exact-sized buffers hide: the last row's sum takes one element past the end, 'masked' by a factor 0"""
    x, hx, y, hy = _arrays(placement)
    _good(hx, hy)
    fx, lx = _flat(hx)
    fy, ly = _flat(hy)
    with np.errstate(invalid="ignore"):
        fy[ly + M * N - 1] = 2.0 * fx[lx + M * N - 1] + fx[lx + M * N] * np.float32(0.0)
    _caught([hx, hy], "output `y`", "NaN", f"offset +{M * N - 1} ", f"row {M - 1}, column {N - 1}")
    fy[ly + M * N - 1] = 2.0 * fx[lx + M * N - 1]                      # the load selected away: fine
    gu.check([hx, hy])


def test_integer_and_byte_arrays():
    idx0 = torch.tensor([3, 0, 3, 4], dtype=torch.int64)
    idx, hi = gu.banded_like(idx0, "in", "offset", name="idx", in_fill=4)
    assert idx.data_ptr() % 16 == 8 and bool((hi.raw[:hi.lo] == 4).all())          # a VALID row index outside
    flags, hf = gu.banded((9,), torch.bool, "cpu", "out", "offset", name="flags")
    assert flags.dtype is torch.bool and flags.data_ptr() % 16 == 4 and hf.raw.dtype is torch.uint8 and bool((hf.raw == 0xA5).all())
    cnt, hc = gu.banded((9,), torch.int32, "cpu", "inout", "aligned", name="count", data=torch.zeros(9, dtype=torch.int32))
    flags[:] = True
    flags[4] = False
    cnt += 1
    gu.check([hi, hf, hc])
    hf.raw[hf.lo + 9] = 1
    hc.raw[hc.lo - 2] = 0
    msg = _caught([hi, hf, hc], "band of `flags`", "after", "offset +9 ", "band of `count`", "before", "offset -2 ")
    assert "`idx`" not in msg


# ---- the oracle through the banded engine ----------------------------------------------------------------------------------------------------------
def _box_engine(lib, device, n):
    return pu.matrix_engine(lib, device, (1, 0, 2), 18, True, n=n, episode_length=gu.ROLLOUT_EPISODE)


def _dr_ext_engine(lib, device, n):
    from leibnizgym_amd.engine import TrifingerEngine, make_config
    cfg = make_config(lib, n, seed=3, episode_length=gu.ROLLOUT_EPISODE, **pu.CONFIGS["d4_domain_randomization_extended"])
    return TrifingerEngine(cfg, device=device, lib=lib)


ORACLE_ENGINES = {"dr_extended": _dr_ext_engine, "box": _box_engine}
_PLAIN = {}


def _plain_oracle_rollout(oracle, name, n, path):
    key = (name, n, path)
    if key not in _PLAIN:
        _PLAIN[key] = gu.engine_rollout(ORACLE_ENGINES[name](oracle, "cpu", n), path, None, round_trip=path == "step")
    return _PLAIN[key]


@pytest.mark.parametrize("placement", gu.PLACEMENTS)
@pytest.mark.parametrize("path", ("step", "split"))
@pytest.mark.parametrize("n", (1, 65, 130))
@pytest.mark.parametrize("name", sorted(ORACLE_ENGINES))
def test_oracle_rollout_through_banded_buffers(oracle, name, n, path, placement):
    want = _plain_oracle_rollout(oracle, name, n, path)
    got = gu.engine_rollout(ORACLE_ENGINES[name](oracle, "cpu", n), path, placement, round_trip=path == "step")
    assert len(got) == len(want) == 1 + gu.ROLLOUT_STEPS + (4 if path == "step" else 0)
    for t, (a, b) in enumerate(zip(got, want)):
        pu.assert_bit_equal(a, b, f"oracle {name} n={n} {path} [{placement}] snapshot {t}")
    steps = np.stack([s["steps"] for s in got[:1 + gu.ROLLOUT_STEPS]])
    assert int((steps[1:] < steps[:-1]).sum()) >= 2 * n                 # the time-outs happened inside the run
    if path == "step":                                                  # the round trip: the two steps after load_state_dict repeat the two before it
        for k in (0, 1):
            pu.assert_bit_equal(got[-2 + k], got[-4 + k], f"oracle {name} n={n} [{placement}] step {k} after load_state_dict")


# ---- completeness of the GPU table -----------------------------------------------------------------------------------------------------------------
def stream_entry_points():
    """every function declared in include/*.h (comments removed, as tests/test_capi_symbols.py parses them) that takes a `stream` argument"""
    names = set()
    for h in sorted(glob.glob(os.path.join(REPO, "include", "*.h"))):
        src = re.sub(r"/\*.*?\*/", "", open(h).read(), flags=re.S)
        for name, params in re.findall(r"\b(tf[pr]?_[a-z0-9_]+)\s*\(([^()]*)\)\s*;", src):
            if re.search(r"\bstream\b", params):
                names.add(name)
    return sorted(names)


def test_every_launching_entry_point_is_a_row_or_exempt():
    import test_guard_bands_gpu as table
    names = stream_entry_points()
    assert len(names) >= 50 and "tf_step" in names and "tfp_ppo_loss_diag" in names and "tfr_render" in names and "tfp_reset_state" in names, names
    covered = table.covered_entry_points()
    for name, reason in table.EXEMPT.items():
        assert isinstance(reason, str) and len(reason.split()) >= 3 and "\n" not in reason, (name, reason)
    both = set(covered) & set(table.EXEMPT)
    assert not both, f"both a row and exempt: {sorted(both)}"
    missing = [n for n in names if n not in covered and n not in table.EXEMPT]
    assert not missing, f"entry points that launch on a stream without a guard-band row or an exemption: {missing}"
    stale = [n for n in list(covered) + list(table.EXEMPT) if n not in names]
    assert not stale, f"rows / exemptions for functions no header declares with a stream: {stale}"
