"""Guard bands of the planning library (include/trifinger_plan.h): the three launching entry points run on plain, `aligned` and `offset` banded arguments
(tests/guard_util.py; the small table classes and the runner are this file's own, in the form of tests/test_kin_guard_bands_gpu.py) - every pointer, those
inside the two TfplSide of tfpl_fork included.  Inputs are unchanged, bands are intact, no sentinel is left in a fully written output, and the outputs are
bit-equal to the plain run.  Shapes with ragged wavefronts on both sides, both action widths, with and without `states`, every kind of horizon step."""
import ctypes as C

import pytest
import torch

import guard_util as gu
import plan_util as pu
from leibnizgym_amd import _capi as capi
from leibnizgym_amd import planning as pl

DEV = "cuda:0"


class Arg:
    """one pointer argument.  role: gu.ROLES.  data: its contents (`in`, `inout`); shape / dtype: of an `out`.  in_fill: what the bands of an integer input hold"""

    def __init__(self, name, role, data=None, shape=None, dtype=torch.float32, in_fill=0):
        assert (data is None) == (role == "out"), name
        self.name, self.role, self.data, self.in_fill = name, role, data, in_fill
        self.shape = tuple(data.shape) if data is not None else tuple(shape)
        self.dtype = data.dtype if data is not None else dtype


class Case:
    """args: [Arg]; call(t) -> status, t the dict name -> tensor"""

    def __init__(self, args, call):
        self.args, self.call = args, call


def _stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def _materialise(case, placement):
    t, handles = {}, []
    for a in case.args:
        if placement is None:
            t[a.name] = gu.sentinel_filled(a.shape, a.dtype, DEV) if a.role == "out" else a.data.to(DEV).clone()
            continue
        view, h = gu.banded(a.shape, a.dtype, DEV, a.role, placement, name=a.name, data=None if a.role == "out" else a.data.to(DEV), in_fill=a.in_fill)
        t[a.name] = view
        handles.append(h)
    return t, handles


def _engine_buffers(n, A, SD, g):
    """the per-env buffers of an engine of n envs as plain tensors with random contents: name -> tensor"""
    f = lambda *s: torch.rand(*s, generator=g) * 2 - 1                                    # noqa: E731
    b = lambda: (torch.rand(n, generator=g) < 0.3).to(torch.uint8)                        # noqa: E731
    d = dict(state=f(capi.TF_STATE_ROWS, n), action_buf=f(n, A), obs=f(n, pl.TF_OBS_DIM_BASE + A), reward=f(n), reset_buf=b(), goal_reset_buf=b(), successes=b(),
             dones=b(), steps=torch.randint(0, 1 << 40, (n,), generator=g), reset_count=torch.randint(0, 1 << 20, (n,), generator=g).to(torch.int32))
    if SD:
        d["states"] = f(n, SD)
    return d


def _side(t, prefix, n, A, SD):
    s = pl.TfplSide()
    for k in pl.FORK_BUFFERS:
        x = t.get(prefix + k)
        setattr(s.buf, k, None if x is None else x.data_ptr())
    s.num_envs, s.action_dim, s.states_dim = n, A, SD
    return s


def cases_fork():
    for n_src, n_dst, A, SD, bad in ((70, 130, 9, 113, False), (1, 1, 9, 0, False), (65, 63, 18, 122, True), (3, 300, 9, 0, True)):
        def build(seed, n_src=n_src, n_dst=n_dst, A=A, SD=SD, bad=bad):
            lib = pu.plan_lib()
            g = torch.Generator().manual_seed(seed)
            idx = pu.fork_map(n_dst, n_src, seed)
            if bad:
                idx[0], idx[n_dst - 1] = n_src, -7
            args = [Arg("src." + k, "in", v) for k, v in _engine_buffers(n_src, A, SD, g).items()]
            args += [Arg("dst." + k, "inout", v) for k, v in _engine_buffers(n_dst, A, SD, g).items()]
            args += [Arg("src_index", "in", idx), Arg("bad_count", "inout", torch.zeros(1, dtype=torch.int32))]

            def call(t):
                a, b = _side(t, "dst.", n_dst, A, SD), _side(t, "src.", n_src, A, SD)
                return lib.tfpl_fork(C.byref(a), C.byref(b), t["src_index"].data_ptr(), t["bad_count"].data_ptr(), _stream())
            return Case(args, call)
        yield f"{n_src}to{n_dst}-A{A}-{'asym' if SD else 'sym'}" + ("-bad" if bad else ""), build


def cases_rollout_actions():
    for E, S, A, H, h in ((2, 64, 9, 3, 0), (2, 64, 9, 3, 1), (2, 64, 9, 3, 3), (1, 192, 18, 2, 0), (1, 192, 18, 2, 1), (3, 64, 18, 1, 1)):
        def build(seed, E=E, S=S, A=A, H=H, h=h):
            lib = pu.plan_lib()
            c, _ = pu.update_params(E, S, a=A, h=H)
            g = torch.Generator().manual_seed(seed)
            n = E * S
            _, U = pu.update_case(E, S, a=A, h=H, seed=seed)
            args = [Arg("U", "in", U), Arg("disc", "in", torch.tensor([0.9 ** k for k in range(H)], dtype=torch.float32)),
                    Arg("reward", "in", 300.0 + 40.0 * torch.randn(n, generator=g)), Arg("reset_buf", "in", (torch.rand(n, generator=g) < 0.2).to(torch.uint8))]
            if h == 0:
                args += [Arg("G", "out", shape=(n,)), Arg("alive", "out", shape=(n,), dtype=torch.uint8)]
            else:
                args += [Arg("G", "inout", 100.0 * torch.randn(n, generator=g)), Arg("alive", "inout", (torch.rand(n, generator=g) < 0.8).to(torch.uint8))]
            args += [Arg("action", "out", shape=(n, A))] if h < H else [Arg("action", "inout", torch.rand(n, A, generator=g))]
            call = lambda t: lib.tfpl_rollout_actions(C.byref(c), h, t["U"].data_ptr(), t["disc"].data_ptr(), t["reward"].data_ptr(),       # noqa: E731
                                                      t["reset_buf"].data_ptr(), t["G"].data_ptr(), t["alive"].data_ptr(), t["action"].data_ptr(), _stream())
            return Case(args, call)
        yield f"E{E}-S{S}-A{A}-H{H}-h{h}", build


def cases_update():
    for E, S, A, H, shift in ((1, 64, 9, 3, True), (5, 192, 9, 3, False), (2, 1024, 18, 2, True), (3, 64, 18, 1, True)):
        def build(seed, E=E, S=S, A=A, H=H, shift=shift):
            lib = pu.plan_lib()
            c, _ = pu.update_params(E, S, a=A, h=H, shift=shift)
            G, U = pu.update_case(E, S, a=A, h=H, seed=seed, invalid=False)
            args = [Arg("G", "in", G), Arg("U", "inout", U), Arg("first", "out", shape=(E, A)), Arg("w", "out", shape=(E * S,)),
                    Arg("stats", "out", shape=(E, pl.NUM_STATS)), Arg("invalid_count", "out", shape=(E,), dtype=torch.int32)]
            call = lambda t: lib.tfpl_update(C.byref(c), t["G"].data_ptr(), t["U"].data_ptr(), t["first"].data_ptr(), t["w"].data_ptr(),     # noqa: E731
                                             t["stats"].data_ptr(), t["invalid_count"].data_ptr(), _stream())
            return Case(args, call)
        yield f"E{E}-S{S}-A{A}-H{H}-{'shift' if shift else 'keep'}", build


# ---- THE TABLE: (entry points the row covers, case generator) -------------------------------------------------------------------------------------------
TABLE = [(("tfpl_fork",), cases_fork), (("tfpl_rollout_actions",), cases_rollout_actions), (("tfpl_update",), cases_update)]


def covered_entry_points():
    return sorted({name for names, _ in TABLE for name in names})


def _all_cases():
    out = []
    for names, gen in TABLE:
        for ident, build in gen():
            out.append(pytest.param(build, 1000 * len(out) + 29, id=f"{names[0]}-{ident}"))
    return out


def test_every_launching_entry_point_has_a_row():
    """every tfpl_* function of the header that takes a `stream`"""
    import re
    import test_planning as tp
    names = sorted(n for n, params in re.findall(r"\b(tfpl_[a-z0-9_]+)\s*\(([^()]*)\)\s*;", tp._header()) if re.search(r"\bstream\b", params))
    assert names == covered_entry_points() and len(names) == 3


@pytest.mark.gpu
@pytest.mark.parametrize("build,seed", _all_cases())
def test_plan_entry_point_on_banded_buffers(hip, build, seed):
    case = build(seed)
    plain, _ = _materialise(case, None)
    assert case.call(plain) == 0, "the plain run is refused"
    torch.cuda.synchronize()
    for a in case.args:
        if a.role == "out" and a.dtype.is_floating_point:
            assert bool(torch.isfinite(plain[a.name]).all()), f"plain `{a.name}` is not finite (an unwritten element holds the sentinel)"
    for placement in gu.PLACEMENTS:
        t, handles = _materialise(case, placement)
        rc = case.call(t)
        torch.cuda.synchronize()
        assert rc == 0, f"[{placement}] status {rc}"
        gu.check(handles)
        for a in case.args:
            if a.role != "in":
                gu.assert_same_bits(t[a.name], plain[a.name], f"`{a.name}` [{placement}]")
