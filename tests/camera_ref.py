"""The checker of the camera tests: a numpy ray caster written from the scene definition of include/pbre_camera.h, not from the kernel.

Link frames come from model/contacts.py: link_frames (the float64 host FK), hull faces from model/objects.py: hull_pieces + scipy's
ConvexHull, the intersections are the analytic ones.  `dtype` selects the arithmetic of everything behind the FK (np.float64: the
reference proper; np.float32: the same program in the kernel's precision, used to measure what rounding alone changes).

Also here: the comparison rule every image test uses (silhouette pixels, `compare`)."""
import numpy as np

from pybullet_robot_envs.model.contacts import link_frames, _quat_R
from pybullet_robot_envs.model.objects import hull_pieces
from pybullet_robot_envs.model.table import HEADER, LINK_STRIDE, SPHERE_STRIDE

GREY = (0.7, 0.7, 0.7)          # the collision spheres when no visual list is set


class Cam(object):
    """the fields of pbre_camera with its defaults"""

    def __init__(self, view, proj, width, height, views=None):
        self.view, self.proj, self.width, self.height, self.views = np.asarray(view, float), np.asarray(proj, float), int(width), int(height), views
        self.ids = dict(robot=0, table=1, object=2, floor=3)
        l = np.array([0.3, -0.4, 0.85])
        self.light = l / np.linalg.norm(l)
        self.ambient = 0.4
        self.background, self.floor_rgb, self.table_rgb, self.object_rgb = (0.75, 0.85, 1.0), (0.6, 0.6, 0.6), (0.55, 0.4, 0.25), (0.9, 0.2, 0.2)


def collision_sphere_visuals(table):
    t = np.asarray(table, float)
    nl, ns = int(t[2]), int(t[5])
    base = HEADER + nl * LINK_STRIDE
    out = []
    for k in range(ns):
        s = t[base + k * SPHERE_STRIDE: base + (k + 1) * SPHERE_STRIDE]
        out.append([s[0], s[1], s[2], s[3], s[1], s[2], s[3], s[4], *GREY, 0.0])
    return np.asarray(out, np.float32).reshape(-1, 12)


# ---------------------------------------------------------------------------------------------- rays (o[3], D[P, 3]) against primitives
def _dot(a, b):
    return (a * b).sum(-1)


def ray_sphere(o, D, c, r):
    """entry root t[P] (inf: the line misses) of the sphere"""
    oc = o - c
    dd, b, cc = _dot(D, D), _dot(D, oc), _dot(oc, oc) - r * r
    h = b * b - dd * cc
    with np.errstate(invalid="ignore"):
        t = (-b - np.sqrt(h)) / dd
    return np.where(h >= 0, t, np.inf).astype(D.dtype)


def ray_capsule(o, D, a, b, r):
    """Entry root and outward normal of the capsule of radius r about the segment a-b: the smallest of the entry roots of the two end
    spheres and of the cylinder body (that one only between the end planes).  Every candidate is a point of the capsule, the true entry
    point is one of them, so their minimum is the entry root -- negative when the origin is inside or the capsule is behind."""
    dt = D.dtype
    ta, tb = ray_sphere(o, D, a, r), ray_sphere(o, D, b, r)
    ba, oa = b - a, o - a
    baba = _dot(ba, ba)
    tc = np.full(D.shape[0], np.inf, dt)
    y = np.zeros(D.shape[0], dt)
    if baba > 0:
        dd, bard, baoa, rdoa, oaoa = _dot(D, D), _dot(D, ba), _dot(ba, oa), _dot(D, oa), _dot(oa, oa)
        A, B, Cc = baba * dd - bard * bard, baba * rdoa - baoa * bard, baba * oaoa - baoa * baoa - r * r * baba
        h = B * B - A * Cc
        with np.errstate(invalid="ignore", divide="ignore"):
            t = (-B - np.sqrt(h)) / A
            y = baoa + t * bard
        ok = (A > 0) & (h >= 0) & (y >= 0) & (y <= baba)
        tc = np.where(ok, t, np.inf).astype(dt)
    t = np.minimum(np.minimum(ta, tb), tc)
    with np.errstate(invalid="ignore"):
        x = o + np.where(np.isfinite(t), t, 0)[:, None] * D
        n = np.where((t == ta)[:, None], (x - a) / r, np.where((t == tb)[:, None], (x - b) / r,
                     (x - a - (y / (baba if baba > 0 else 1))[:, None] * ba) / r))
    return t, n.astype(dt)


def ray_box(o, D, c, h):
    """entry root and entry-face normal of the box |x - c| <= h (slabs); a ray parallel to a slab is inside it when |o - c| <= h"""
    dt = D.dtype
    oc = o - c
    with np.errstate(divide="ignore", invalid="ignore"):
        t1, t2 = (-h - oc) / D, (h - oc) / D
    lo, hi = np.minimum(t1, t2), np.maximum(t1, t2)
    par = D == 0
    inside = np.abs(oc) <= h
    lo = np.where(par, np.where(inside, -np.inf, np.inf), lo)
    hi = np.where(par, np.where(inside, np.inf, -np.inf), hi)
    tin, tout = lo.max(1), hi.min(1)
    ax = lo.argmax(1)
    n = np.zeros(D.shape, dt)
    n[np.arange(D.shape[0]), ax] = -np.sign(D[np.arange(D.shape[0]), ax])
    return np.where(tin <= tout, tin, np.inf).astype(dt), n


def ray_cylinder(o, D, r, hz):
    """cylinder about z through the origin: x^2 + y^2 <= r^2, |z| <= hz"""
    dt = D.dtype
    A, B, Cc = D[:, 0] ** 2 + D[:, 1] ** 2, o[0] * D[:, 0] + o[1] * D[:, 1], o[0] ** 2 + o[1] ** 2 - r * r
    h = B * B - A * Cc
    with np.errstate(divide="ignore", invalid="ignore"):
        c0, c1 = (-B - np.sqrt(h)) / A, (-B + np.sqrt(h)) / A
        s1, s2 = (-hz - o[2]) / D[:, 2], (hz - o[2]) / D[:, 2]
    par = A == 0
    c0 = np.where(par, np.where(Cc <= 0, -np.inf, np.inf), np.where(h >= 0, c0, np.inf))
    c1 = np.where(par, np.where(Cc <= 0, np.inf, -np.inf), np.where(h >= 0, c1, -np.inf))
    zpar = D[:, 2] == 0
    zin = abs(o[2]) <= hz
    s0 = np.where(zpar, -np.inf if zin else np.inf, np.minimum(s1, s2))
    s3 = np.where(zpar, np.inf if zin else -np.inf, np.maximum(s1, s2))
    tin, tout = np.maximum(c0, s0), np.minimum(c1, s3)
    n = np.zeros(D.shape, dt)
    cap = s0 > c0
    n[:, 2] = np.where(cap, -np.sign(D[:, 2]), 0)
    with np.errstate(invalid="ignore"):
        tt = np.where(np.isfinite(tin), tin, 0)
        n[:, 0] = np.where(cap, 0, (o[0] + tt * D[:, 0]) / r)
        n[:, 1] = np.where(cap, 0, (o[1] + tt * D[:, 1]) / r)
    return np.where(tin <= tout, tin, np.inf).astype(dt), n


def ray_planes(o, D, normals, offsets):
    """convex body {x: normals . x + offsets <= 0}: entry = the largest t over the planes with n . d < 0, exit = the smallest over
    n . d > 0; a parallel plane with the origin outside: a miss"""
    dt = D.dtype
    den = D @ normals.T                         # [P, F]
    dist = (normals @ o + offsets)[None]        # > 0: outside
    with np.errstate(divide="ignore", invalid="ignore"):
        t = -dist / den
    tin_all = np.where(den < 0, t, -np.inf)
    tout_all = np.where(den > 0, t, np.inf)
    bad = ((den == 0) & (dist > 0)).any(1)
    tin, tout = tin_all.max(1), tout_all.min(1)
    n = normals[tin_all.argmax(1)]
    ok = (tin <= tout) & ~bad & np.isfinite(tin)
    return np.where(ok, tin, np.inf).astype(dt), n.astype(dt)


def ray_floor(o, D, z0):
    with np.errstate(divide="ignore", invalid="ignore"):
        t = (z0 - o[2]) / D[:, 2]
    return np.where(D[:, 2] < 0, t, np.inf).astype(D.dtype)


def shade(base, ndotl, ambient):
    v = 255 * base * (ambient + (1 - ambient) * np.maximum(0, ndotl))
    return np.clip(np.floor(v + 0.5), 0, 255)


def hull_planes(hull, dtype=np.float64):
    """[(normals [F, 3], offsets [F], bounding-sphere centre, radius)] per convex piece of the vertex list handed to set_object_hull"""
    from scipy.spatial import ConvexHull
    out = []
    for pc in hull_pieces(np.asarray(hull, float)):
        pc = pc.astype(np.float32).astype(float)              # the engine keeps the vertices as floats
        eq = ConvexHull(pc).equations
        eq = np.unique(np.round(eq, 9), axis=0)
        out.append((eq[:, :3].astype(dtype), eq[:, 3].astype(dtype)))
    return out


# ---------------------------------------------------------------------------------------------- camera
def camera_rays(view, proj, W, H, dtype):
    """eye [3], directions [H * W, 3] scaled so that t is the depth along the view axis, near, far"""
    V = np.asarray(view, dtype).reshape(4, 4).T
    P = np.asarray(proj, dtype)
    R, t = V[:3, :3], V[:3, 3]
    eye = -(R.T @ t)
    r, u, f = R[0], R[1], -R[2]
    i, j = np.meshgrid(np.arange(W, dtype=dtype), np.arange(H, dtype=dtype))
    x = 2 * (i + dtype(0.5)) / dtype(W) - 1
    y = 1 - 2 * (j + dtype(0.5)) / dtype(H)
    X, Y = ((x + P[8]) / P[0]).reshape(-1, 1), ((y + P[9]) / P[5]).reshape(-1, 1)
    D = f[None] + X * r[None] + Y * u[None]
    near, far = P[14] / (P[10] - 1), P[14] / (P[10] + 1)
    return eye.astype(dtype), D.astype(dtype), dtype(near), dtype(far)


def render(table, state, obj_off, phys, cam, visuals=None, no_object=False, hull=None, dtype=np.float64):
    """depth float [N, H, W], seg int32 [N, H, W], rgba uint8 [N, H, W, 4] of the batch state records state[N, F]"""
    dt = np.dtype(dtype).type
    table = np.asarray(table, float)
    st = np.asarray(state, float)
    n = st.shape[0]
    vis = collision_sphere_visuals(table) if visuals is None or len(visuals) == 0 else np.asarray(visuals, np.float32).reshape(-1, 12)
    R, p = link_frames(table, st[:, :int(table[3])])
    W, H = cam.width, cam.height
    tc, th, oh = (np.array(list(x), dt) for x in (phys.table_c, phys.table_h, phys.obj_h))
    shape = int(phys.obj_shape)
    planes = hull_planes(hull, dt) if (shape == 3 and not no_object) else None
    light = np.asarray(cam.light, np.float32).astype(dt)
    amb = dt(np.float32(cam.ambient))
    col = lambda c: np.asarray(c, np.float32).astype(dt)
    depth = np.empty((n, H * W), dt); seg = np.empty((n, H * W), np.int32); rgba = np.empty((n, H * W, 4), np.uint8)
    for e in range(n):
        view = cam.views[e] if cam.views is not None else cam.view
        o, D, near, far = camera_rays(np.asarray(view, np.float32), np.asarray(cam.proj, np.float32), W, H, dt)
        best = np.full(H * W, np.inf, dt); ids = np.full(H * W, -1, np.int32)
        nrm = np.zeros((H * W, 3), dt); base = np.tile(col(cam.background), (H * W, 1))

        def take(t, n_, id_, rgb):
            win = (t >= near) & (t <= far) & (t < best)
            best[win] = t[win]; ids[win] = id_; nrm[win] = n_[win] if np.ndim(n_) == 2 else n_; base[win] = rgb

        for v in vis:
            li = int(v[0])
            Rl, pl = R[e, li].astype(dt), p[e, li].astype(dt)
            a, b = pl + Rl @ v[1:4].astype(dt), pl + Rl @ v[4:7].astype(dt)
            t, n_ = ray_capsule(o, D, a, b, dt(v[7]))
            take(t, n_, cam.ids["robot"] + ((li + 1) << 24), (np.floor(255 * v[8:11].astype(float) + 0.5) / 255).astype(np.float32).astype(dt))
        if not no_object:
            Ro = _quat_R(st[e:e + 1, obj_off + 3:obj_off + 7].astype(np.float32).astype(dt))[0].astype(dt)
            po = st[e, obj_off:obj_off + 3].astype(dt)
            ol, Dl = Ro.T @ (o - po), D @ Ro
            if shape == 0:
                t, nl = ray_box(ol, Dl, np.zeros(3, dt), oh)
            elif shape == 1:
                t, nl = ray_capsule(ol, Dl, np.zeros(3, dt), np.zeros(3, dt), oh[0])
            elif shape == 2:
                t, nl = ray_cylinder(ol, Dl, oh[0], oh[2])
            else:
                t = np.full(H * W, np.inf, dt); nl = np.zeros((H * W, 3), dt)
                for nm, off in planes:
                    tp, npc = ray_planes(ol, Dl, nm, off)
                    w = (tp >= near) & (tp <= far) & (tp < t)
                    t[w] = tp[w]; nl[w] = npc[w]
            take(t, nl @ Ro.T, cam.ids["object"], col(cam.object_rgb))
        t, n_ = ray_box(o, D, tc, th)
        take(t, n_, cam.ids["table"], col(cam.table_rgb))
        take(ray_floor(o, D, dt(phys.ground_z)), np.array([0, 0, 1], dt), cam.ids["floor"], col(cam.floor_rgb))
        hit = ids != -1
        depth[e] = np.where(hit, best, far)
        seg[e] = ids
        ndl = np.where(hit, nrm @ light, 1)
        rgba[e, :, :3] = shade(base, ndl[:, None], amb).astype(np.uint8)
        rgba[e, :, 3] = 255
    return depth.reshape(n, H, W), seg.reshape(n, H, W), rgba.reshape(n, H, W, 4)


# ---------------------------------------------------------------------------------------------- the comparison rule
def silhouette(seg):
    """[H, W] bool: a pixel any of whose 8 neighbours has another id"""
    s = np.pad(seg, 1, mode="edge")
    H, W = seg.shape
    out = np.zeros(seg.shape, bool)
    for dy in (0, 1, 2):
        for dx in (0, 1, 2):
            out |= s[dy:dy + H, dx:dx + W] != seg
    return out


def seg_cap(H, W):
    """differing pixels allowed per image: 4 at 64 x 48, scaled by area, at least 2"""
    return max(2, int(round(4.0 * H * W / (64 * 48))))


def compare(ref, got):
    """ref, got: (depth, seg, rgba) of ONE image; ref is the float64 reference.  Returns (differing pixels, those of them that are not
    silhouette pixels, largest relative depth difference, largest colour-channel difference), the last two over the pixels that agree in
    segmentation and are not silhouette pixels."""
    sil = silhouette(ref[1])
    diff = ref[1] != got[1]
    m = ~diff & ~sil
    dd = (np.abs(got[0].astype(float) - ref[0].astype(float)) / ref[0].astype(float))[m].max() if m.any() else 0.0
    dc = np.abs(got[2][..., :3].astype(int) - ref[2][..., :3].astype(int))[m].max() if m.any() else 0
    return int(diff.sum()), int((diff & ~sil).sum()), float(dd), int(dc)
