"""Guard bands of the fingertip-space library (include/trifinger_kin.h): every tfk_* entry point that takes a `stream` runs on plain, `aligned` and `offset`
banded arguments (tests/guard_util.py; the small table classes and the runner below are this file's own, in the form of tests/test_guard_bands_gpu.py); the bands are checked and the outputs are bit-equal to the
plain run.  Shapes N in {1, 63, 65, 130}; every array input in both layouts - rows of a structure-of-arrays state ([9][N]) and row-major ([N][9]); every
optional output passed NULL in one case.  tests/test_kinematics.py checks that the table is complete."""
import ctypes as C

import pytest
import torch

import guard_util as gu
import kin_util as ku
from leibnizgym_amd import _capi as capi
from leibnizgym_amd import kinematics as kin

DEV = "cuda:0"


class Arg:
    """one pointer argument.  role: gu.ROLES.  data: its contents (`in`); shape / dtype: of an `out`"""

    def __init__(self, name, role, data=None, shape=None, dtype=torch.float32):
        assert (data is None) == (role == "out"), name
        self.name, self.role, self.data = name, role, data
        self.shape = tuple(data.shape) if data is not None else tuple(shape)
        self.dtype = data.dtype if data is not None else dtype


class Case:
    """args: [Arg]; call(t) -> status, t the dict name -> tensor"""

    def __init__(self, args, call):
        self.args, self.call = args, call


def _stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def _p(t):
    return None if t is None else t.data_ptr()


def _materialise(case, placement):
    """-> (name -> tensor on the GPU, handles).  placement None: plain exact-sized tensors, an output starting from the sentinel too"""
    t, handles = {}, []
    for a in case.args:
        if placement is None:
            t[a.name] = gu.sentinel_filled(a.shape, a.dtype, DEV) if a.role == "out" else a.data.to(DEV).clone()
            continue
        view, h = gu.banded(a.shape, a.dtype, DEV, a.role, placement, name=a.name, data=None if a.role == "out" else a.data.to(DEV))
        t[a.name] = view
        handles.append(h)
    return t, handles


LAYOUTS = ("rows", "rowmajor")

# functions with a `stream` argument that have no row, each with its reason
EXEMPT = {}


def _arr(t, layout, n, width):
    """the TfkArray of a banded tensor: [width, n] rows of a state, or [n, width] row-major"""
    if t is None:
        return kin.NO_ARRAY
    return kin.TfkArray(t.data_ptr(), 1, n) if layout == "rows" else kin.TfkArray(t.data_ptr(), width, 1)


def _in(name, x, layout):
    return Arg(name, "in", (x.T if layout == "rows" else x).contiguous().to(torch.float32))


class _Kin:
    """one handle for the default model, made at the first case"""
    handle = None

    @classmethod
    def get(cls):
        if cls.handle is None:
            lib, h = kin.load(), C.c_void_p()
            m = capi.load_hip_library().default_model()
            assert lib.tfk_create(C.byref(m), C.byref(h)) == 0
            cls.handle = (lib, h)
        return cls.handle


def _inputs(n, seed):
    mc = kin.model_constants(capi.load_hip_library().default_model())
    g = torch.Generator().manual_seed(seed)
    q = ku.uniform_joints(mc, n, seed)
    qd = torch.rand(n, 9, generator=g) * 6 - 3
    off = torch.rand(n, 3, generator=g) * 0.02 - 0.01
    cmd = torch.rand(n, 9, generator=g) * 3 - 1.5
    target, _ = ku.ik_case(mc, n, seed + 1)
    return q, qd, off, cmd, target


def cases_forward():
    for n in ku.SHAPES:
        for layout in LAYOUTS:
            for drop in ((None,) if (n, layout) != (65, "rows") else (None, "tip_v", "jac", "base_off")):
                def build(seed, n=n, layout=layout, drop=drop):
                    lib, h = _Kin.get()
                    q, qd, off, _, _ = _inputs(n, seed)
                    args = [_in("q", q, layout)]
                    args += [] if drop == "tip_v" else [_in("qd", qd, layout)]
                    args += [] if drop == "base_off" else [_in("base_off", off, layout)]
                    args += [Arg("tip_p", "out", shape=(n, 9))]
                    args += [] if drop == "tip_v" else [Arg("tip_v", "out", shape=(n, 9))]
                    args += [] if drop == "jac" else [Arg("jac", "out", shape=(n, 27))]
                    call = lambda t: lib.tfk_forward(h, _arr(t["q"], layout, n, 9), _arr(t.get("qd"), layout, n, 9), _arr(t.get("base_off"), layout, n, 3),   # noqa: E731
                                                     _p(t["tip_p"]), _p(t.get("tip_v")), _p(t.get("jac")), n, _stream())
                    return Case(args, call)
                yield f"n{n}-{layout}" + (f"-no_{drop}" if drop else ""), build


def cases_inverse():
    for n in ku.SHAPES:
        for layout in LAYOUTS:
            for drop in ((None,) if (n, layout) != (65, "rowmajor") else (None, "base_off")):
                def build(seed, n=n, layout=layout, drop=drop):
                    lib, h = _Kin.get()
                    q, _, off, _, target = _inputs(n, seed)
                    args = [_in("target", target, layout), _in("q0", q, layout)] + ([] if drop else [_in("base_off", off, layout)])
                    args += [Arg("q_out", "out", shape=(n, 9)), Arg("residual", "out", shape=(n, 3))]
                    p = kin.TfkIkParams(8, 0.02, 0.5)
                    call = lambda t: lib.tfk_inverse(h, _arr(t["target"], layout, n, 9), _arr(t["q0"], layout, n, 9), _arr(t.get("base_off"), layout, n, 3),   # noqa: E731
                                                     C.byref(p), _p(t["q_out"]), _p(t["residual"]), n, _stream())
                    return Case(args, call)
                yield f"n{n}-{layout}" + (f"-no_{drop}" if drop else ""), build


def cases_tip_action():
    for n in ku.SHAPES:
        for layout in LAYOUTS:
            for mode, frame in (("position", "delta"), ("torque", "absolute")):
                for drop in ((None,) if (n, layout) != (65, "rows") else (None, "target_out", "base_off")):
                    def build(seed, n=n, layout=layout, mode=mode, frame=frame, drop=drop):
                        lib, h = _Kin.get()
                        q, qd, off, cmd, _ = _inputs(n, seed)
                        args = [_in("cmd", cmd, layout), _in("q", q, layout)] + ([_in("qd", qd, layout)] if mode == "torque" else [])
                        args += [] if drop == "base_off" else [_in("base_off", off, layout)]
                        args += [Arg("action", "out", shape=(n, 9))] + ([] if drop == "target_out" else [Arg("target_out", "out", shape=(n, 9))])
                        p, _ = kin.action_params(frame, mode, True)
                        call = lambda t: lib.tfk_tip_action(h, C.byref(p), _arr(t["cmd"], layout, n, 9), _arr(t["q"], layout, n, 9),                   # noqa: E731
                                                            _arr(t.get("qd"), layout, n, 9), _arr(t.get("base_off"), layout, n, 3), _p(t["action"]),
                                                            _p(t.get("target_out")), n, _stream())
                        return Case(args, call)
                    yield f"n{n}-{layout}-{mode}-{frame}" + (f"-no_{drop}" if drop else ""), build


# ---- THE TABLE: (entry points the row covers, case generator) -------------------------------------------------------------------------------------------
TABLE = [(("tfk_forward",), cases_forward), (("tfk_inverse",), cases_inverse), (("tfk_tip_action",), cases_tip_action)]


def covered_entry_points():
    return sorted({name for names, _ in TABLE for name in names})


def _all_cases():
    out = []
    for names, gen in TABLE:
        for ident, build in gen():
            out.append(pytest.param(build, 1000 * len(out) + 23, id=f"{names[0]}-{ident}"))
    return out


@pytest.mark.gpu
@pytest.mark.parametrize("build,seed", _all_cases())
def test_kin_entry_point_on_banded_buffers(hip, build, seed):
    case = build(seed)
    plain, _ = _materialise(case, None)
    assert case.call(plain) == 0, "the plain run is refused"
    torch.cuda.synchronize()
    for a in case.args:
        if a.role == "out":
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
