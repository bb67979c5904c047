"""fp64 numpy restatement of the renderer's scene and march (include/trifinger_render.h), sharing no code with the kernel.

Everything takes a dtype `dt` so that the same text runs as an fp32 restatement: the bounds of the GPU tests come from comparing the two.
A scene is built from a TfModel (ctypes) and ONE column of the state matrix (172 floats).
"""
import struct
import zlib

import numpy as np

from leibnizgym_amd import _capi as capi

ID_OBJECT, ID_FLOOR, ID_BOUNDARY = 20, 21, 22
_SHADES = ((230, 60), (200, 40), (255, 100), (170, 30), (150, 20), (130, 10))
PALETTE = np.array([(24, 24, 28)] + [tuple(a if c == f else b for c in range(3)) for f in range(3) for a, b in _SHADES]
                   + [(0, 0, 0), (235, 200, 40), (120, 122, 126), (176, 150, 118)], dtype=np.uint8)
GHOST = np.array((60, 220, 220), dtype=np.uint32)
LIGHT = np.array((0.35, 0.25, 0.9)) / np.linalg.norm((0.35, 0.25, 0.9))
DEFAULT_CAMERA = dict(eye=(0.55, 0.35, 0.50), target=(0.0, 0.0, 0.10), fov=np.deg2rad(45.0))
MARCH = dict(eps=1e-4, relax=0.9, max_steps=160, t_max=2.0)


def _Ry(a):
    c, s = np.cos(a), np.sin(a)
    return np.array([[c, 0, s], [0, 1, 0], [-s, 0, c]])


def _Rx(a):
    c, s = np.cos(a), np.sin(a)
    return np.array([[1, 0, 0], [0, c, -s], [0, s, c]])


def quat_to_rot(q):
    x, y, z, w = [float(v) for v in q]
    return np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - w * z), 2 * (x * z + w * y)],
                     [2 * (x * y + w * z), 1 - 2 * (x * x + z * z), 2 * (y * z - w * x)],
                     [2 * (x * z - w * y), 2 * (y * z + w * x), 1 - 2 * (x * x + y * y)]])


def _shape(sh, dirs):
    g = lambda n: np.array(getattr(sh, n)[:], dtype=np.float64)      # noqa: E731
    return dict(a=g("a"), b=g("b"), w1=g("w1"), w2=g("w2"), rho=g("rho"), o1=g("o1"), o2=g("o2"), dirs=dirs)


class Scene:
    """the scene of one env: `prims` in id order as (id, kind, ...), the goal box, the stage centre and the boundary profile"""

    def __init__(self, model, col, dt=np.float64):
        m, st = model, np.asarray(col, dtype=np.float64)
        assert st.shape == (capi.TF_STATE_ROWS,)
        self.dt = dt
        dr = st[capi.S_DR:capi.S_DR + capi.TF_NUM_DR]
        boff = dr[capi.DR_BASE_POS:capi.DR_BASE_POS + 3]
        self.soff = dr[capi.DR_STAGE_POS:capi.DR_STAGE_POS + 2].astype(dt)
        j2, j3 = np.array(m.j2_origin[:], dtype=np.float64), np.array(m.j3_origin[:], dtype=np.float64)
        shapes = (_shape(m.shape1, (0, 2)), _shape(m.shape2, (0, 1)), _shape(m.shape3, (0, 1)))
        spheres = ((1, m.sph2[0]), (1, m.sph2[1]), (2, m.sph3[0]))           # (index of the link frame, sphere)
        self.prims, self.frames = [], []
        for f in range(3):
            q = st[capi.S_Q + 3 * f:capi.S_Q + 3 * f + 3]
            c, s = float(m.base_yaw_cos[f]), float(m.base_yaw_sin[f])
            W = np.array([[c, -s, 0], [s, c, 0], [0, 0, 1.0]])
            R1 = W @ _Ry(q[0]); p1 = np.array([0, 0, float(m.base_height)]) + boff
            R2 = R1 @ _Rx(q[1]); p2 = p1 + R1 @ j2
            R3 = R1 @ _Rx(q[1] + q[2]); p3 = p2 + R2 @ j3
            fr = [(R1, p1), (R2, p2), (R3, p3)]
            self.frames.append(fr)
            for l in range(3):
                self.prims.append((1 + 6 * f + l, "shape", fr[l][0].astype(dt), fr[l][1].astype(dt), shapes[l]))
            for k, (l, sp) in enumerate(spheres):
                cw = fr[l][1] + fr[l][0] @ np.array(sp.c[:], dtype=np.float64)
                self.prims.append((1 + 6 * f + 3 + k, "sphere", cw.astype(dt), dt(sp.radius)))
        half = np.array(m.box_half[:], dtype=np.float64) if m.box else np.full(3, float(m.cube_half))
        self.half = (half * dr[1]).astype(dt)
        self.obj_R, self.obj_p = quat_to_rot(st[capi.S_CUBE_Q:capi.S_CUBE_Q + 4]).astype(dt), st[capi.S_CUBE_P:capi.S_CUBE_P + 3].astype(dt)
        self.goal_R, self.goal_p = quat_to_rot(st[capi.S_GOAL_Q:capi.S_GOAL_Q + 4]).astype(dt), st[capi.S_GOAL_P:capi.S_GOAL_P + 3].astype(dt)
        self.prims.append((ID_OBJECT, "box", self.obj_R, self.obj_p, self.half))
        self.wr, self.wz = np.array(m.wall_r[:], dtype=np.float64), np.array(m.wall_z[:], dtype=np.float64)
        self.tip_origin = np.array(m.tip_origin[:], dtype=np.float64)
        self.cap_b, self.cap_radius = np.array(m.cap_b[:], dtype=np.float64), float(m.cap_radius)

    def tip_world(self, f):
        R3, p3 = self.frames[f][2]
        return p3 + R3 @ self.tip_origin


def shape_field(pl, sh, dt):
    a, d = sh["a"].astype(dt), (sh["b"] - sh["a"]).astype(dt)
    s = np.clip(((pl - a) @ d) / (d @ d), 0, 1).astype(dt)
    e = pl - (a + s[:, None] * d)
    D = np.sqrt((e * e).sum(1)).astype(dt)
    u = np.where((D >= 1e-12)[:, None], e / np.maximum(D, dt(1e-12))[:, None], dt(0))
    i1, i2 = sh["dirs"]
    lin = lambda v: dt(v[0]) + s * dt(v[1] - v[0])      # noqa: E731
    rho = lin(sh["rho"]); h1 = lin(sh["w1"]) - rho; h2 = lin(sh["w2"]) - rho
    ext = rho + h1 * np.abs(u[:, i1]) + h2 * np.abs(u[:, i2]) + lin(sh["o1"]) * u[:, i1] + lin(sh["o2"]) * u[:, i2]
    return (D - ext).astype(dt)


def scene_field(sc, p):
    """(minimum, its id - ties to the lower id -, second smallest value) over link shapes, spheres and object at world points p [n, 3]"""
    dt, n = sc.dt, p.shape[0]
    best, second, bid = np.full(n, np.inf, dt), np.full(n, np.inf, dt), np.zeros(n, np.int32)
    for pr in sc.prims:
        if pr[1] == "shape":
            d = shape_field(((p - pr[3]) @ pr[2]).astype(dt), pr[4], dt)
        elif pr[1] == "sphere":
            e = p - pr[2]; d = np.sqrt((e * e).sum(1)).astype(dt) - pr[3]
        else:
            q = np.abs(((p - pr[3]) @ pr[2]).astype(dt)) - pr[4]
            d = np.sqrt((np.maximum(q, 0) ** 2).sum(1)).astype(dt) + np.minimum(q.max(1), 0)
        t = d < best
        second = np.where(t, best, np.minimum(second, d)).astype(dt)
        best = np.where(t, d, best).astype(dt); bid = np.where(t, pr[0], bid)
    return best, bid, second


def boundary_field(sc, p, normal=False):
    dt = sc.dt
    x, y, z = p[:, 0] - sc.soff[0], p[:, 1] - sc.soff[1], p[:, 2]
    rho = np.sqrt(x * x + y * y).astype(dt)
    r = np.full(p.shape[0], sc.wr[0], dt); c = np.ones(p.shape[0], dt); sn = np.zeros(p.shape[0], dt)
    for k in range(3):
        sl = (sc.wr[k + 1] - sc.wr[k]) / (sc.wz[k + 1] - sc.wz[k]); ck = 1 / np.sqrt(1 + sl * sl)
        m = z > sc.wz[k]
        r = np.where(m, sc.wr[k] + (z - sc.wz[k]) * sl, r).astype(dt); c = np.where(m, ck, c).astype(dt); sn = np.where(m, sl * ck, sn).astype(dt)
    er, ez = rho - sc.wr[3], z - sc.wz[3]
    drim = np.sqrt(er * er + ez * ez).astype(dt)
    below = z < sc.wz[3]
    d = np.where(below, np.abs((r - rho) * c), drim).astype(dt)
    if not normal:
        return d
    nx, ny = x / np.maximum(rho, 1e-12), y / np.maximum(rho, 1e-12)
    k = er / np.maximum(drim, 1e-12)
    nrm = np.stack([np.where(below, -c * nx, k * nx), np.where(below, -c * ny, k * ny), np.where(below, sn, ez / np.maximum(drim, 1e-12))], 1)
    return d, nrm


def ray_box(R, c, h, eye, d, dt):
    """entry parameter of the rays eye + t d [n, 3] into the box (0 from inside), +inf for a miss"""
    o = ((eye - c) @ R).astype(dt); dl = (d @ R).astype(dt)
    tn, tf, miss = np.full(d.shape[0], -np.inf, dt), np.full(d.shape[0], np.inf, dt), np.zeros(d.shape[0], bool)
    for i in range(3):
        par = np.abs(dl[:, i]) < 1e-12
        inv = 1 / np.where(par, 1, dl[:, i])
        t1, t2 = (-h[i] - o[i]) * inv, (h[i] - o[i]) * inv
        miss |= par & (abs(o[i]) > h[i])
        tn = np.where(par, tn, np.maximum(tn, np.minimum(t1, t2))); tf = np.where(par, tf, np.minimum(tf, np.maximum(t1, t2)))
    hit = ~miss & (tn <= tf) & (tf > 0)
    return np.where(hit, np.maximum(tn, 0), np.inf).astype(dt)


def camera_rays(eye, target, fov, W, H, dt=np.float64):
    eye = np.asarray(eye, np.float64); fw = np.asarray(target, np.float64) - eye; fw /= np.linalg.norm(fw)
    rt = np.cross(fw, [0, 0, 1.0]); rt /= np.linalg.norm(rt); up = np.cross(rt, fw)
    th = np.tan(0.5 * fov)
    xs = ((np.arange(W) + 0.5) / W * 2 - 1) * th * W / H; ys = (1 - (np.arange(H) + 0.5) / H * 2) * th
    X, Y = np.meshgrid(xs, ys)
    d = fw[None, None] + X[..., None] * rt + Y[..., None] * up
    return eye.astype(dt), (d / np.linalg.norm(d, axis=-1, keepdims=True)).reshape(-1, 3).astype(dt)


def march(sc, e, d, eps=1e-4, relax=0.9, max_steps=160, t_max=2.0):
    """the march of include/trifinger_render.h for rays e + t d -> (t, id with 0 = background, unresolved: the ray
    still marched when max_steps ran out, samples taken)"""
    dt, n = sc.dt, d.shape[0]
    t = np.zeros(n, dt); hit = np.zeros(n, np.int32); alive = np.ones(n, bool); samples = np.zeros(n, np.int32)
    tfl = np.where(d[:, 2] < 0, -e[2] / np.minimum(d[:, 2], dt(-1e-9)), dt(np.inf)).astype(dt)
    exy = e[:2] - sc.soff
    tc = (-(exy * d[:, :2]).sum(1) / np.maximum((d[:, :2] ** 2).sum(1), dt(1e-12))).astype(dt)
    with np.errstate(invalid="ignore"):
        pf = exy[None] + tfl[:, None] * d[:, :2]
        on_disc = (pf ** 2).sum(1) <= dt(sc.wr[0]) ** 2
    for _ in range(max_steps):
        idx = np.nonzero(alive)[0]
        if idx.size == 0:
            break
        samples[idx] += 1
        p = e + t[idx, None] * d[idx]
        ds, ids, _ = scene_field(sc, p)
        after = t[idx] >= tc[idx]
        db = np.where(after, boundary_field(sc, p), np.inf)
        hs = ds < eps
        hb = (db < eps) & ~hs
        hit[idx[hs]] = ids[hs]; hit[idx[hb]] = ID_BOUNDARY
        tn = np.where(after, t[idx] + dt(relax) * np.minimum(ds, db), np.minimum(t[idx] + dt(relax) * ds, np.maximum(tc[idx], t[idx] + dt(eps))))
        t[idx] = np.where(hs | hb, t[idx], tn).astype(dt)
        alive[idx[hs | hb]] = False
        fl = alive[idx] & (t[idx] >= tfl[idx])
        hit[idx[fl]] = np.where(on_disc[idx[fl]], ID_FLOOR, 0); t[idx[fl]] = tfl[idx[fl]]; alive[idx[fl]] = False
        alive[idx[alive[idx] & (t[idx] > t_max)]] = False
    return t, hit, alive, samples


def render(sc, eye=DEFAULT_CAMERA["eye"], target=DEFAULT_CAMERA["target"], fov=DEFAULT_CAMERA["fov"], W=256, H=256, shading=0, **kw):
    """-> dict: color uint8 [H, W, 4], depth [H, W] (+inf: no hit), seg uint8 [H, W], unresolved bool [H, W] (max_steps ran out),
    ghost bool [H, W] (the goal was blended), ghost_t / raw_t [H, W], samples int [H, W]"""
    dt = sc.dt
    mk = dict(MARCH); mk.update(kw)
    e, d = camera_rays(eye, target, fov, W, H, dt)
    t, hit, unresolved, samples = march(sc, e, d, **mk)
    solid = hit > 0
    depth = np.where(solid, t, np.inf)
    shade = np.ones(d.shape[0], dt)
    if shading == 1:
        p = e + t[:, None] * d
        nrm = np.tile(np.array([0, 0, 1.0], dt), (d.shape[0], 1))
        sel = np.nonzero(solid & (hit <= ID_OBJECT))[0]
        if sel.size:
            g = np.zeros((sel.size, 3), dt)
            for j in range(3):
                off = np.zeros(3, dt); off[j] = 5e-4
                g[:, j] = scene_field(sc, p[sel] + off)[0] - scene_field(sc, p[sel] - off)[0]
            nrm[sel] = g / np.sqrt(np.maximum((g * g).sum(1), 1e-30))[:, None]
        sel = np.nonzero(hit == ID_BOUNDARY)[0]
        if sel.size:
            nrm[sel] = boundary_field(sc, p[sel], normal=True)[1]
        shade = np.where(solid, dt(0.35) + dt(0.65) * np.maximum((nrm @ LIGHT.astype(dt)), 0), 1).astype(dt)
    rgb = np.minimum(np.floor(PALETTE[hit].astype(dt) * shade[:, None] + dt(0.5)), 255).astype(np.uint32)
    tg = ray_box(sc.goal_R, sc.goal_p, sc.half, e, d, dt)
    ghost = tg < depth
    rgb = np.where(ghost[:, None], (rgb + GHOST[None] + 1) >> 1, rgb)
    color = np.concatenate([rgb.astype(np.uint8), np.full((d.shape[0], 1), 255, np.uint8)], 1)
    r = lambda a: a.reshape(H, W, *a.shape[1:])      # noqa: E731
    return dict(color=r(color), depth=r(depth), seg=r(hit.astype(np.uint8)), unresolved=r(unresolved), ghost=r(ghost), ghost_t=r(tg),
                samples=r(samples), shade=r(shade))


def edges(ids):
    """pixels with another id among their 3 x 3 neighbours; the image border counts"""
    e = np.zeros(ids.shape, bool)
    for dy in (-1, 0, 1):
        for dx in (-1, 0, 1):
            e |= np.roll(np.roll(ids, dy, 0), dx, 1) != ids
    e[0] = e[-1] = True; e[:, 0] = e[:, -1] = True
    return e


def excluded_shares(img):
    """(share of all pixels, share of the robot and object pixels) that are edge pixels or unresolved - the pixels an image comparison leaves out"""
    seg = img["seg"]
    ex = edges(seg) | img["unresolved"]
    fg = (seg >= 1) & (seg <= ID_OBJECT)
    return float(ex.mean()), float((ex & fg).sum() / max(int(fg.sum()), 1)), ex


# ---- the seeded scenes of the tests ----------------------------------------------------------------------
def neutral_state():
    st = np.zeros(capi.TF_STATE_ROWS, np.float64)
    st[capi.S_CUBE_Q + 3] = st[capi.S_GOAL_Q + 3] = st[capi.S_PREV_OBJ_Q + 3] = 1.0
    st[capi.S_DR:capi.S_DR + capi.TF_NUM_DR] = 1.0
    st[capi.S_DR + capi.DR_BASE_POS:capi.S_DR + capi.DR_FRICTION_ROBOT] = 0.0
    return st


def _quat(axis, ang):
    a = np.asarray(axis, np.float64) / np.linalg.norm(axis)
    return np.concatenate([a * np.sin(ang / 2), [np.cos(ang / 2)]])


def _qmul(a, b):
    ax, ay, az, aw = a; bx, by, bz, bw = b
    return np.array([aw * bx + ax * bw + ay * bz - az * by, aw * by - ax * bz + ay * bw + az * bx, aw * bz + ax * by - ay * bx + az * bw,
                     aw * bw - ax * bx - ay * by - az * bz])


def seeded_state(case, half_z=0.0325, ext_dr=False):
    """the three scenes of the picture tests: 0 the default pose with the cube at rest, 1 and 2 perturbed joints with a displaced (2: tilted) cube;
    the goal floats beside the object.  `ext_dr`: cube size, base and stage offsets as the extended domain randomisation would draw them"""
    rng = np.random.default_rng(100 + case)
    st = neutral_state()
    st[capi.S_Q:capi.S_Q + 9] = np.tile([0.0, 0.9, -1.7], 3) + (rng.uniform(-0.3, 0.3, 9) if case else 0)
    ang = rng.uniform(0, 2 * np.pi) if case else 0.0
    if ext_dr:
        st[capi.S_DR + 1] = 0.9
        st[capi.S_DR + capi.DR_BASE_POS:capi.S_DR + capi.DR_BASE_POS + 3] = (0.008, -0.012, 0.003)
        st[capi.S_DR + capi.DR_STAGE_POS:capi.S_DR + capi.DR_STAGE_POS + 2] = (0.015, -0.01)
    st[capi.S_CUBE_P:capi.S_CUBE_P + 3] = (0.03 * case, -0.02 * case, half_z * st[capi.S_DR + 1] + 0.02 * case)
    q = _quat((0, 0, 1), ang)
    if case == 2:
        q = _qmul(q, _quat((1, 0, 0), 0.4))
    st[capi.S_CUBE_Q:capi.S_CUBE_Q + 4] = q
    st[capi.S_GOAL_P:capi.S_GOAL_P + 3] = (-0.06 + 0.02 * case, 0.07, 0.09 + 0.01 * case)
    st[capi.S_GOAL_Q:capi.S_GOAL_Q + 4] = _qmul(_quat((0, 0, 1), 0.5 + case), _quat((0, 1, 0), 0.3 * case))
    return st


# ---- reading back what write_png wrote ---------------------------------------------------------------------
def decode_png(path):
    """the pixels [H, W, 3 or 4] of an 8-bit RGB / RGBA PNG with one IDAT chunk and filter type 0 on every scanline; checks the CRCs"""
    data = open(path, "rb").read()
    assert data[:8] == b"\x89PNG\r\n\x1a\n"
    pos, chunks = 8, []
    while pos < len(data):
        n, tag = struct.unpack(">I4s", data[pos:pos + 8])
        body = data[pos + 8:pos + 8 + n]
        assert struct.unpack(">I", data[pos + 8 + n:pos + 12 + n])[0] == zlib.crc32(tag + body) & 0xffffffff
        chunks.append((tag, body)); pos += 12 + n
    assert [t for t, _ in chunks] == [b"IHDR", b"IDAT", b"IEND"]
    w, h, depth, ctype, comp, flt, inter = struct.unpack(">IIBBBBB", chunks[0][1])
    assert (depth, comp, flt, inter) == (8, 0, 0, 0) and ctype in (2, 6)
    c = 4 if ctype == 6 else 3
    raw = np.frombuffer(zlib.decompress(chunks[1][1]), np.uint8).reshape(h, 1 + w * c)
    assert np.all(raw[:, 0] == 0)
    return raw[:, 1:].reshape(h, w, c)
