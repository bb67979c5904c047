"""Offscreen renderer of the collision model: ctypes binding of include/trifinger_render.h (libtrifinger_render.so) and its torch front end.

The picture shows exactly what the contact code collides - the fitted link shapes, housing spheres, the object box, the floor disc and the
boundary profile - ray-marched by one HIP kernel from the resident ``state[172][N]`` rows.  GPU only: without the library or on a device that is
not ``cuda`` the constructor raises, like the engine.  `write_png` and `mosaic` are host helpers (stdlib only).
"""
import ctypes as C
import math
import os
import struct
import zlib

import torch

from . import _capi as capi

TFR_API_VERSION = 1
TFR_MAX_VIEWS = 64
TFR_MAX_SIZE = 4096
ID_BACKGROUND, ID_OBJECT, ID_FLOOR, ID_BOUNDARY, NUM_IDS = 0, 20, 21, 22, 23
SHADING = {"flat": 0, "lit": 1}

DEFAULT_EYE = (0.55, 0.35, 0.50)
DEFAULT_TARGET = (0.0, 0.0, 0.10)
DEFAULT_FOV_DEG = 45.0

# the colour table of include/trifinger_render.h: palette[id] = (R, G, B); GHOST is the goal's
_FINGER_SHADES = ((230, 60), (200, 40), (255, 100), (170, 30), (150, 20), (130, 10))
PALETTE = [(24, 24, 28)]
for _f in range(3):
    for _a, _b in _FINGER_SHADES:
        PALETTE.append(tuple(_a if _c == _f else _b for _c in range(3)))
PALETTE += [(0, 0, 0), (235, 200, 40), (120, 122, 126), (176, 150, 118)]
GHOST = (60, 220, 220)


class TfrConfig(C.Structure):
    _fields_ = [("api_version", C.c_int32), ("width", C.c_int32), ("height", C.c_int32), ("max_views", C.c_int32),
                ("max_steps", C.c_int32), ("shading", C.c_int32), ("eps", C.c_float), ("relax", C.c_float), ("t_max", C.c_float)]


_P = C.c_void_p
_F3 = C.POINTER(C.c_float)

# every symbol include/trifinger_render.h declares: name -> (restype, argtypes)
SYMBOLS = {
    "tfr_api_version": (C.c_int, []),
    "tfr_last_error_string": (C.c_char_p, []),
    "tfr_default_config": (None, [C.POINTER(TfrConfig)]),
    "tfr_create": (C.c_int, [C.POINTER(capi.TfModel), C.POINTER(TfrConfig), C.POINTER(_P)]),
    "tfr_destroy": (C.c_int, [_P]),
    "tfr_set_camera": (C.c_int, [_P, _F3, _F3, C.c_float]),
    "tfr_set_views": (C.c_int, [_P, C.POINTER(C.c_int32), C.c_int32, C.c_int32]),
    "tfr_render": (C.c_int, [_P, _P, _P, _P, _P, _P]),
    "tfr_test_field": (C.c_int, [_P, _P, C.c_int32, _P, _P, _P, _P, C.c_int32, _P]),
}

_LIB = None


def library_path():
    return os.path.join(os.path.dirname(os.path.abspath(__file__)), "csrc", "libtrifinger_render.so")


def load():
    """Load libtrifinger_render.so (cached); works without a GPU.  Fails loudly when it has not been built."""
    global _LIB
    if _LIB is None:
        path = library_path()
        if not os.path.isfile(path):
            raise capi.TfLibraryError(f"native library not found: {path}. Build it with `make -C leibnizgym_amd/csrc`. There is no fallback path.")
        lib = C.CDLL(path)
        for name, (res, args) in SYMBOLS.items():
            try:
                fn = getattr(lib, name)
            except AttributeError as exc:
                raise capi.TfLibraryError(f"{path} does not export `{name}` declared in include/trifinger_render.h") from exc
            fn.restype = res
            fn.argtypes = args
        if lib.tfr_api_version() != TFR_API_VERSION:
            raise capi.TfLibraryError(f"{path}: API version {lib.tfr_api_version()} != {TFR_API_VERSION}")
        _LIB = lib
    return _LIB


def _check(lib, rc, what):
    if rc == capi.TF_OK:
        return
    text = (lib.tfr_last_error_string() or b"").decode()
    exc = ValueError if rc == capi.TF_ERR_INVALID_ARG else RuntimeError
    raise exc(f"{what}: status {rc} ({text})")


class SceneRenderer:
    """Renders views of single envs from a state matrix.  The output tensors are owned by the renderer and valid until the next `render`."""

    def __init__(self, model=None, width=256, height=256, max_views=16, device="cuda:0", shading="lit", max_steps=160, eps=1e-4, relax=0.9,
                 t_max=2.0):
        self.device = torch.device(device)
        if self.device.type != "cuda":
            raise RuntimeError(f"the renderer runs only as a HIP kernel on an MI355X: device must be 'cuda:N' (got '{device}'); there is no CPU path")
        if shading not in SHADING:
            raise ValueError(f"shading: one of {sorted(SHADING)}, got {shading!r}")
        self.lib = load()
        self._dev_index = self.device.index if self.device.index is not None else torch.cuda.current_device()
        self.device = torch.device("cuda", self._dev_index)
        if model is None:
            model = capi.load_hip_library().default_model()
        cfg = TfrConfig()
        self.lib.tfr_default_config(C.byref(cfg))
        cfg.width, cfg.height, cfg.max_views = int(width), int(height), int(max_views)
        cfg.max_steps, cfg.shading = int(max_steps), SHADING[shading]
        cfg.eps, cfg.relax, cfg.t_max = float(eps), float(relax), float(t_max)
        self._handle = _P()
        _check(self.lib, self.lib.tfr_create(C.byref(model), C.byref(cfg), C.byref(self._handle)), "tfr_create")
        self.width, self.height, self.max_views = cfg.width, cfg.height, cfg.max_views
        self.num_envs = None
        self.env_ids = []
        self._out = None

    def close(self):
        if getattr(self, "_handle", None):
            self.lib.tfr_destroy(self._handle)
            self._handle = _P()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def set_camera(self, eye=DEFAULT_EYE, target=DEFAULT_TARGET, fov_deg=DEFAULT_FOV_DEG):
        e = (C.c_float * 3)(*[float(x) for x in eye])
        t = (C.c_float * 3)(*[float(x) for x in target])
        _check(self.lib, self.lib.tfr_set_camera(self._handle, e, t, math.radians(float(fov_deg))), "tfr_set_camera")

    def set_views(self, env_ids, num_envs):
        """which envs of a `num_envs`-wide state the views show; every id is checked on the host (ValueError) before the kernel sees it"""
        ids = [int(i) for i in env_ids]
        arr = (C.c_int32 * max(len(ids), 1))(*ids)
        _check(self.lib, self.lib.tfr_set_views(self._handle, arr, len(ids), int(num_envs)), "tfr_set_views")
        if ids != self.env_ids or self._out is None:
            v = len(ids)
            self._out = {"color": torch.empty((v, self.height, self.width, 4), dtype=torch.uint8, device=self.device),
                         "depth": torch.empty((v, self.height, self.width), dtype=torch.float32, device=self.device),
                         "segmentation": torch.empty((v, self.height, self.width), dtype=torch.uint8, device=self.device)}
        self.env_ids, self.num_envs = ids, int(num_envs)

    def _state_ptr(self, state):
        if self.num_envs is None:
            raise RuntimeError("SceneRenderer: set_views first")
        if (not isinstance(state, torch.Tensor) or state.dtype != torch.float32 or state.device != self.device or not state.is_contiguous()
                or tuple(state.shape) != (capi.TF_STATE_ROWS, self.num_envs)):
            raise ValueError(f"state: contiguous float32 [{capi.TF_STATE_ROWS}, {self.num_envs}] on {self.device}")
        return state.data_ptr()

    def _stream(self):
        return _P(torch.cuda.current_stream(self._dev_index).cuda_stream)

    def render(self, state):
        """-> {"color": uint8 [V, H, W, 4], "depth": float32 [V, H, W] (+inf: no hit), "segmentation": uint8 [V, H, W]}; one launch on torch's current
        stream of the renderer's device, no synchronisation"""
        ptr = self._state_ptr(state)
        o = self._out
        with torch.cuda.device(self._dev_index):
            rc = self.lib.tfr_render(self._handle, ptr, o["color"].data_ptr(), o["depth"].data_ptr(), o["segmentation"].data_ptr(), self._stream())
        _check(self.lib, rc, "tfr_render")
        return o

    def field(self, state, env, points):
        """(dist, id, boundary_dist) of the scene of env `env` at world `points` [n, 3] (float32, on the device): the leaf entry of the parity tests"""
        ptr = self._state_ptr(state)
        if points.dtype != torch.float32 or points.device != self.device or not points.is_contiguous() or points.dim() != 2 or points.shape[1] != 3:
            raise ValueError("points: contiguous float32 [n, 3] on the renderer's device")
        n = points.shape[0]
        dist = torch.empty(n, dtype=torch.float32, device=self.device)
        ids = torch.empty(n, dtype=torch.uint8, device=self.device)
        bd = torch.empty(n, dtype=torch.float32, device=self.device)
        with torch.cuda.device(self._dev_index):
            rc = self.lib.tfr_test_field(self._handle, ptr, int(env), points.data_ptr(), dist.data_ptr(), ids.data_ptr(), bd.data_ptr(), n, self._stream())
        _check(self.lib, rc, "tfr_test_field")
        return dist, ids, bd


# ---- host helpers --------------------------------------------------------------------------------------
def mosaic(color):
    """views [V, H, W, C] tiled row-major into one image [rows H, cols W, C] with cols = ceil(sqrt(V)); empty tiles are zero.  Tensor or array in,
    the same kind out."""
    v, h, w, c = color.shape
    cols = int(math.ceil(math.sqrt(v)))
    rows = (v + cols - 1) // cols
    out = color.new_zeros((rows * h, cols * w, c)) if isinstance(color, torch.Tensor) else __import__("numpy").zeros((rows * h, cols * w, c), color.dtype)
    for i in range(v):
        r, k = divmod(i, cols)
        out[r * h:(r + 1) * h, k * w:(k + 1) * w] = color[i]
    return out


def _chunk(tag, data):
    return struct.pack(">I", len(data)) + tag + data + struct.pack(">I", zlib.crc32(tag + data) & 0xffffffff)


def write_png(path, color):
    """Write one uint8 image [H, W, 3 or 4] (tensor on any device, or array) as an 8-bit RGB / RGBA PNG.  One device-to-host copy for a device tensor."""
    if isinstance(color, torch.Tensor):
        color = color.detach().cpu().numpy()
    if color.ndim != 3 or color.shape[2] not in (3, 4) or str(color.dtype) != "uint8":
        raise ValueError(f"write_png: uint8 [H, W, 3 or 4], got {color.dtype} {tuple(color.shape)}")
    h, w, c = color.shape
    rows = color.reshape(h, w * c)
    raw = b"".join(b"\x00" + rows[j].tobytes() for j in range(h))          # filter type 0 on every scanline
    png = (b"\x89PNG\r\n\x1a\n" + _chunk(b"IHDR", struct.pack(">IIBBBBB", w, h, 8, 6 if c == 4 else 2, 0, 0, 0))
           + _chunk(b"IDAT", zlib.compress(raw, 6)) + _chunk(b"IEND", b""))
    d = os.path.dirname(path)
    if d:
        os.makedirs(d, exist_ok=True)
    with open(path, "wb") as f:
        f.write(png)


# ---- the env's `native.render` section -------------------------------------------------------------------
RENDER_KEYS = ("width", "height", "envs", "fov_deg", "record_dir", "shading")


def parse_render_config(section, num_instances):
    """Validate `native.render` (ValueError) -> dict with every key filled: 256 x 256, the first min(num_instances, 4) envs, 45 degrees, lit, no
    recording.  Pure host code: the env calls it at construction whatever the device."""
    section = {} if section is None else section
    if not isinstance(section, dict):
        raise ValueError(f"native.render: a mapping, got {type(section).__name__}")
    unknown = sorted(set(section) - set(RENDER_KEYS))
    if unknown:
        raise ValueError(f"native.render: unknown key(s) {unknown}; known: {list(RENDER_KEYS)}")
    out = {}
    for k in ("width", "height"):
        v = section.get(k, 256)
        if isinstance(v, bool) or not isinstance(v, int) or not 1 <= v <= TFR_MAX_SIZE:
            raise ValueError(f"native.render.{k}: an integer in [1, {TFR_MAX_SIZE}], got {v!r}")
        out[k] = v
    envs = section.get("envs")
    envs = list(range(min(int(num_instances), 4))) if envs is None else list(envs)
    if not 1 <= len(envs) <= TFR_MAX_VIEWS:
        raise ValueError(f"native.render.envs: 1 to {TFR_MAX_VIEWS} env ids, got {len(envs)}")
    for i in envs:
        if isinstance(i, bool) or not isinstance(i, int) or not 0 <= i < int(num_instances):
            raise ValueError(f"native.render.envs: env id {i!r} outside [0, {int(num_instances)})")
    out["envs"] = envs
    fov = section.get("fov_deg", DEFAULT_FOV_DEG)
    if isinstance(fov, bool) or not isinstance(fov, (int, float)) or not 1.0 <= float(fov) <= 170.0:
        raise ValueError(f"native.render.fov_deg: a number in [1, 170], got {fov!r}")
    out["fov_deg"] = float(fov)
    shading = section.get("shading", "lit")
    if shading not in SHADING:
        raise ValueError(f"native.render.shading: one of {sorted(SHADING)}, got {shading!r}")
    out["shading"] = shading
    rec = section.get("record_dir")
    if rec is not None and not isinstance(rec, (str, os.PathLike)):
        raise ValueError(f"native.render.record_dir: a path or None, got {rec!r}")
    out["record_dir"] = None if rec is None else os.fspath(rec)
    return out
