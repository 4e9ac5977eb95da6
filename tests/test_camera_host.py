"""The camera without a GPU: the per-ray functions of csrc/pbre_camera.hpp compiled for the host against tests/camera_ref.py, the camera
helpers, the reference's own float32-vs-float64 figures (the GPU tests' tolerances), the default visual list, the emulation library."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import camera_ref as ref
import camera_scenes as scn
from pybullet_robot_envs import _capi, camera as pcam
from pybullet_robot_envs.model.visuals import default_visuals, MAX_PRIMS

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# Measured by test_reference_float32_against_float64 below (largest over its scenes: the Panda with the default visual list and with the
# collision spheres alone at 64 x 48 and 37 x 23, every object shape of camera_scenes.SHAPES tilted above the table at 64 x 48, the iCub
# and the iCub with hands at 48 x 32; the task camera with far = 10 perturbed by +-30 deg yaw and +-10 deg pitch).  Measured: depth
# 8.68e-6 (the single hull, env 1), colour 0, no differing segmentation pixel; the constants are those figures rounded up to one digit.
REF32_DEPTH_REL = 9e-6        # largest |depth32 - depth64| / depth64 on agreeing non-silhouette pixels
REF32_COLOUR = 0              # largest colour-channel difference there
# what the GPU tests allow (test_gpu_camera.py): the device does its FK in fp32 with another operation order
GPU_DEPTH_REL = 4 * REF32_DEPTH_REL
GPU_COLOUR = max(1, 2 * REF32_COLOUR)


@pytest.fixture(scope="module")
def host():
    d = os.path.join(ROOT, "tests", "camera_host")
    subprocess.check_call(["make", "-s", "-C", d])
    lib = C.CDLL(os.path.join(d, "build", "libpbre_camera_host.so"))
    for f in ("cam_capsule", "cam_box", "cam_cylinder", "cam_planes", "cam_floor", "cam_shade"):
        getattr(lib, f).restype = None
    return lib


def _p(a):
    return a.ctypes.data_as(C.c_void_p)


def _f32(*xs):
    return [np.ascontiguousarray(x, np.float32) for x in xs]


def _rays(rng, n, centre, radius):
    """rays from points around `centre` aimed near it, so that about half of them hit something of size `radius`"""
    o = centre + rng.normal(size=(n, 3)) * 8 * radius
    aim = centre + rng.normal(size=(n, 3)) * 0.4 * radius
    d = (aim - o) * rng.uniform(0.5, 2.0, (n, 1))           # not normalised, as in the kernel
    return _f32(o, d)


def _check(t_host, n_host, o, d, t_ref, n_ref, r, centre, what):
    """Hits agree except within rounding of a silhouette.  Entry roots: the float32
    discriminant b^2 - (d.d) c cancels from terms of size L^2 (L: origin to primitive) down to the root's r^2 cos^2, so the root carries
    an error of about eps L^2 / (r cos) along the ray (r: the surface's radius of curvature, or the primitive's size for flat faces);
    allowed: 16 times that, and that over r for the normal."""
    hit_h, hit_r = t_host > 0, np.isfinite(t_ref) & (t_ref > 0)
    both = hit_h & hit_r
    assert both.sum() > 0.1 * len(t_ref), "%s: only %d rays hit" % (what, both.sum())
    flips = hit_h != hit_r
    assert flips.sum() <= max(2, 0.002 * len(t_ref)), "%s: %d rays flip between hit and miss" % (what, flips.sum())
    dn = np.linalg.norm(d.astype(float), axis=1)
    err = np.abs(t_host[both] - t_ref[both]) * dn[both]
    graze = np.abs((n_ref[both] * d[both].astype(float)).sum(1)) / dn[both]      # |cos| of the incidence angle
    L2 = ((o[both].astype(float) - centre) ** 2).sum(1) + r * r
    ok = err <= 16 * np.finfo(np.float32).eps * L2 / (r * np.maximum(graze, 1e-3))
    assert ok.all(), "%s: entry root off by %g" % (what, err[~ok].max())
    if n_host is not None:
        ntol = 16 * np.finfo(np.float32).eps * L2 / (r * r * np.maximum(graze, 1e-3)) + 1e-5      # (the hit point's error over r)
        assert (np.abs(n_host[both] - n_ref[both]).max(1) <= ntol).all(), what


def _ref_capsule(o, d, a, b, r):
    t = np.empty(len(o)); n = np.empty((len(o), 3))
    for i in range(len(o)):
        ti, ni = ref.ray_capsule(o[i].astype(float), d[i:i + 1].astype(float), a.astype(float), b.astype(float), float(r))
        t[i], n[i] = ti[0], ni[0]
    return t, n


def _per_ray(fn, o, d, *args):
    t = np.empty(len(o)); n = np.zeros((len(o), 3))
    for i in range(len(o)):
        r = fn(o[i].astype(float), d[i:i + 1].astype(float), *args)
        if isinstance(r, tuple):
            t[i], n[i] = r[0][0], r[1][0]
        else:
            t[i] = r[0]
    return t, n


def test_host_capsule(host):
    rng = np.random.default_rng(1)
    for a, b, r in (([0.1, 0.2, 0.3], [0.4, 0.1, 0.5], 0.05), ([0, 0, 0], [0, 0, 0.3], 0.02), ([1, 1, 1], [1, 1, 1], 0.07)):
        a, b = _f32(a, b)
        o, d = _rays(rng, 3000, 0.5 * (a + b).astype(float), 0.5 * np.linalg.norm(b - a) + r)
        t = np.empty(len(o), np.float32); n = np.empty((len(o), 3), np.float32)
        host.cam_capsule(len(o), _p(o), _p(d), _p(a), _p(b), C.c_float(r), _p(t), _p(n))
        tr, nr = _ref_capsule(o, d, a, b, np.float32(r))
        _check(t, n, o, d, tr, nr, float(r), 0.5 * (a + b).astype(float), "capsule")


def test_host_capsule_degenerate(host):
    a, b = _f32([0, 0, 0], [0, 0, 0.3])
    r = np.float32(0.05)

    def cast(o, d, a=a, b=b):
        o, d = _f32([o], [d])
        t = np.empty(1, np.float32); n = np.empty((1, 3), np.float32)
        host.cam_capsule(1, _p(o), _p(d), _p(a), _p(b), C.c_float(r), _p(t), _p(n))
        return float(t[0]), n[0]
    # along the axis, from below: enters the cap sphere at z = -r
    t, n = cast([0, 0, -1], [0, 0, 2])
    assert abs(t - (1 - 0.05) / 2) < 1e-6 and np.allclose(n, [0, 0, -1], atol=1e-5)
    # parallel to the axis inside the radius, off centre
    t, n = cast([0.03, 0, -1], [0, 0, 1])
    assert abs(t - (1 - 0.04)) < 1e-5
    # parallel to the axis outside the radius: a miss
    assert cast([0.06, 0, -1], [0, 0, 1])[0] <= 0
    # origin inside the body / inside a cap: no hit is counted from inside
    assert cast([0.01, 0, 0.15], [1, 0, 0])[0] <= 0
    assert cast([0, 0, -0.02], [0, 1, 0])[0] <= 0
    # behind the origin
    assert cast([1, 0, 0.1], [1, 0, 0])[0] <= 0
    # perpendicular through the body
    t, n = cast([1, 0, 0.1], [-1, 0, 0])
    assert abs(t - 0.95) < 1e-6 and np.allclose(n, [1, 0, 0], atol=1e-5)
    # zero-length capsule: a sphere
    t, n = cast([0, -1, 0], [0, 1, 0], a, a)
    assert abs(t - 0.95) < 1e-6 and np.allclose(n, [0, -1, 0], atol=1e-5)
    tr, _ = ref.ray_capsule(np.array([0.03, 0, -1.0]), np.array([[0, 0, 1.0]]), a.astype(float), b.astype(float), 0.05)
    assert abs(tr[0] - 0.96) < 1e-12


def test_host_box(host):
    rng = np.random.default_rng(2)
    c, h = _f32([0.85, 0.0, 0.6], [0.75, 0.5, 0.025])
    o, d = _rays(rng, 3000, c.astype(float), 0.5)
    t = np.empty(len(o), np.float32); n = np.empty((len(o), 3), np.float32)
    host.cam_box(len(o), _p(o), _p(d), _p(c), _p(h), _p(t), _p(n))
    tr, nr = _per_ray(ref.ray_box, o, d, c.astype(float), h.astype(float))
    _check(t, n, o, d, tr, nr, 0.5, c.astype(float), "box")
    # a ray along a face lies inside that slab: it enters through the side it meets
    o1, d1 = _f32([[-1, 0, 0.625]], [[1, 0, 0]])
    host.cam_box(1, _p(o1), _p(d1), _p(c), _p(h), _p(t), _p(n))
    assert abs(t[0] - 1.1) < 1e-6 and np.allclose(n[0], [-1, 0, 0])
    assert abs(ref.ray_box(o1[0].astype(float), d1.astype(float), c.astype(float), h.astype(float))[0][0] - 1.1) < 1e-6
    # just above the face, parallel: a miss; from inside: no hit
    o1, d1 = _f32([[-1, 0, 0.626]], [[1, 0, 0]])
    host.cam_box(1, _p(o1), _p(d1), _p(c), _p(h), _p(t), _p(n))
    assert t[0] <= 0
    o1, d1 = _f32([[0.85, 0, 0.6]], [[0.3, 0.2, 1]])
    host.cam_box(1, _p(o1), _p(d1), _p(c), _p(h), _p(t), _p(n))
    assert t[0] <= 0


def test_host_cylinder(host):
    rng = np.random.default_rng(3)
    r, hz = np.float32(0.035), np.float32(0.05)
    o, d = _rays(rng, 3000, np.zeros(3), 0.05)
    t = np.empty(len(o), np.float32); n = np.empty((len(o), 3), np.float32)
    host.cam_cylinder(len(o), _p(o), _p(d), C.c_float(r), C.c_float(hz), _p(t), _p(n))
    tr, nr = _per_ray(ref.ray_cylinder, o, d, float(r), float(hz))
    _check(t, n, o, d, tr, nr, float(r), np.zeros(3), "cylinder")
    o1, d1 = _f32([[0.01, 0, 1]], [[0, 0, -1]])              # along the axis: enters the top cap
    host.cam_cylinder(1, _p(o1), _p(d1), C.c_float(r), C.c_float(hz), _p(t), _p(n))
    assert abs(t[0] - 0.95) < 1e-6 and np.allclose(n[0], [0, 0, 1])
    o1, d1 = _f32([[0.01, 0, 0.01]], [[1, 0, 0]])            # from inside
    host.cam_cylinder(1, _p(o1), _p(d1), C.c_float(r), C.c_float(hz), _p(t), _p(n))
    assert t[0] <= 0


def test_host_planes(host):
    from scipy.spatial import ConvexHull
    rng = np.random.default_rng(4)
    eq = ConvexHull(scn.HULL6).equations
    pl = np.concatenate([-(eq[:, :3] * eq[:, 3:4]), eq[:, :3]], axis=1).astype(np.float32)      # a point of each plane | its normal
    pl = np.ascontiguousarray(pl)
    o, d = _rays(rng, 3000, np.zeros(3), 0.05)
    t = np.empty(len(o), np.float32); n = np.empty((len(o), 3), np.float32)
    host.cam_planes(len(o), _p(o), _p(d), _p(pl), C.c_int(len(pl)), _p(t), _p(n))
    tr, nr = _per_ray(ref.ray_planes, o, d, eq[:, :3], eq[:, 3])
    _check(t, n, o, d, tr, nr, 0.05, np.zeros(3), "planes")
    o1, d1 = _f32([[0.0, 0.0, 0.0]], [[1, 0.2, 0.1]])        # from inside the hull
    host.cam_planes(1, _p(o1), _p(d1), _p(pl), C.c_int(len(pl)), _p(t), _p(n))
    assert t[0] <= 0


def test_host_floor_and_shade(host):
    o, d = _f32([[0, 0, 1], [0, 0, 1], [0, 0, -1]], [[1, 0, -0.5], [1, 0, 0.5], [0, 0, -1]])
    t = np.empty(3, np.float32)
    host.cam_floor(3, _p(o), _p(d), C.c_float(0.0), _p(t))
    assert abs(t[0] - 2.0) < 1e-6 and t[1] <= 0 and t[2] <= 0
    rng = np.random.default_rng(5)
    base, ndl = _f32(rng.uniform(0, 1, 4000), rng.uniform(-1, 1, 4000))
    out = np.empty(4000, np.int32)
    host.cam_shade(4000, _p(base), _p(ndl), C.c_float(0.4), _p(out))
    want = ref.shade(base.astype(float), ndl.astype(float), float(np.float32(0.4)))
    assert np.abs(out - want).max() <= 1 and (out != want).mean() < 0.01          # (a float32 product next to a rounding tie)
    assert out.min() >= 0 and out.max() <= 255


# ---------------------------------------------------------------------------------------------- camera helpers
def test_view_matrix_yaw0_pitch0_looks_along_y():
    V = pcam.view_matrix_from_yaw_pitch_roll([1.0, 2.0, 3.0], 2.0, 0, 0, 0, 2).reshape(4, 4).T
    assert np.allclose(-V[2, :3], [0, 1, 0]) and np.allclose(V[1, :3], [0, 0, 1]) and np.allclose(V[0, :3], [1, 0, 0])
    eye = -V[:3, :3].T @ V[:3, 3]
    assert np.allclose(eye, [1.0, 0.0, 3.0])
    V = pcam.view_matrix_from_yaw_pitch_roll([0, 0, 0], 1.3, 180, -40, 0, 2).reshape(4, 4).T      # the reference's: behind +y... looking down
    f = -V[2, :3]
    assert f[2] < 0 and f[1] < 0 and abs(f[0]) < 1e-12


def test_projection_gives_back_the_pixel_ray():
    W, H = 37, 23
    view, proj = scn.task_camera([0.0, 0.0, 0.625], W, H, 17.0, -6.0)
    o, D, near, far = ref.camera_rays(view, proj, W, H, np.float64)
    assert abs(near - 0.1) < 1e-12 and abs(far - scn.FAR) < 1e-9
    M = proj.reshape(4, 4).T @ view.reshape(4, 4).T
    for (j, i, depth) in ((0, 0, 0.5), (22, 36, 3.0), (11, 5, 1.7)):
        x = o + depth * D[j * W + i]
        c = M @ np.append(x, 1.0)
        ndc = c[:3] / c[3]
        assert abs(c[3] - depth) < 1e-9                    # clip w = depth along the view axis = the ray parameter
        assert abs((ndc[0] + 1) * 0.5 * W - (i + 0.5)) < 1e-9 and abs((1 - ndc[1]) * 0.5 * H - (j + 0.5)) < 1e-9


def test_depth_buffer_round_trip():
    d = np.array([0.1, 0.5, 2.0, 9.99, 10.0])
    b = pcam.depth_buffer(d, 0.1, 10.0)
    assert b[0] == 0.0 and abs(b[-1] - 1.0) < 1e-12 and np.all(np.diff(b) > 0)
    assert np.allclose(pcam.depth_from_buffer(b, 0.1, 10.0), d, rtol=1e-12)


# ---------------------------------------------------------------------------------------------- the reference against itself
def _scenes(panda):
    from pybullet_robot_envs.model.table import icub_table, icub_hands_table
    rng = np.random.default_rng(7)
    tbl = panda["table"]
    out = []
    st = scn.synthetic_state(tbl, 4, 48, 9, rng, scn.PANDA_HOME, 0.25)
    for k, (W, H) in enumerate(((64, 48), (37, 23))):
        for vis in (default_visuals(tbl), None):
            out.append(("panda", tbl, st, 9, scn.phys_like(), vis, None, W, H))
    for name, (shape, oh, hull) in scn.SHAPES.items():
        out.append((name, tbl, scn.synthetic_state(tbl, 3, 48, 9, rng, scn.PANDA_HOME, 0.25), 9,
                    scn.phys_like(shape, oh if oh is not None else (0.1, 0.1, 0.1)), default_visuals(tbl), hull, 64, 48))
    it = icub_table("l")[0]
    out.append(("icub", it, scn.synthetic_state(it, 3, 80, 20, rng, None, 0.2), 20, scn.phys_like(), default_visuals(it), None, 48, 32))
    ht = icub_hands_table("l")[0]
    out.append(("hands", ht, scn.synthetic_state(ht, 2, 272, 60, rng, None, 0.2), 60, scn.phys_like(), default_visuals(ht), None, 48, 32))
    return out


def test_reference_float32_against_float64(panda):
    rng = np.random.default_rng(11)
    worst_d, worst_c, total = 0.0, 0, 0
    for name, tbl, st, off, ph, vis, hull, W, H in _scenes(panda):
        view, proj = scn.task_camera(np.asarray(tbl[6:9]), W, H, rng.uniform(-30, 30), rng.uniform(-10, 10))
        cam = ref.Cam(view, proj, W, H)
        r64 = ref.render(tbl, st, off, ph, cam, vis, hull=hull, dtype=np.float64)
        r32 = ref.render(tbl, st, off, ph, cam, vis, hull=hull, dtype=np.float32)
        for e in range(st.shape[0]):
            assert len(np.unique(r64[1][e])) >= 3, "%s: the image shows fewer than three bodies" % name
            nd, off_sil, dd, dc = ref.compare([x[e] for x in r64], [x[e] for x in r32])
            print("%-9s env %d  %dx%d  seg diff %d (off silhouette %d)  depth rel %.3g  colour %d" % (name, e, W, H, nd, off_sil, dd, dc))
            assert nd <= ref.seg_cap(H, W) and off_sil == 0, name
            worst_d, worst_c, total = max(worst_d, dd), max(worst_c, dc), total + nd
    print("largest: depth rel %.3g, colour %d; %d differing pixels in all" % (worst_d, worst_c, total))
    assert worst_d <= REF32_DEPTH_REL and worst_c <= REF32_COLOUR


# ---------------------------------------------------------------------------------------------- visuals, emulation library
def test_default_visuals(panda):
    from pybullet_robot_envs.model.table import icub_table, icub_hands_table
    for tbl in (panda["table"], icub_table("l")[0], icub_hands_table("l")[0]):
        v = default_visuals(tbl)
        nl, ns = int(tbl[2]), int(tbl[5])
        assert v.shape[1] == 12 and ns < len(v) <= MAX_PRIMS
        assert np.all(v[:, 0] >= 0) and np.all(v[:, 0] < nl) and np.all(v[:, 0] == np.floor(v[:, 0]))
        sph, cap = v[:ns], v[ns:]
        assert np.all(sph[:, 1:4] == sph[:, 4:7])
        ln = np.linalg.norm(cap[:, 4:7] - cap[:, 1:4], axis=1)
        assert np.all(ln >= 1e-3) and np.all(cap[:, 7] >= 0.004 - 1e-9) and np.all(cap[:, 7] <= 0.04 + 1e-9)
        assert np.allclose(cap[:, 7], np.minimum(0.04, np.maximum(0.004, 0.25 * ln)), atol=1e-7)
        assert np.all(v[:, 8:11] >= 0) and np.all(v[:, 8:11] <= 1)
    assert len(default_visuals(panda["table"])) == 13 + 8     # 13 collision spheres, 8 link pairs further than 1 mm apart


def test_emulation_library_has_no_camera(panda, emu_lib):
    assert not hasattr(emu_lib, "pbre_camera_render")
    eng = _capi.Engine(panda["table"], task=_capi.TASK_PUSH, num_envs=2, lib=emu_lib)
    with pytest.raises(RuntimeError, match="no camera"):
        eng.render()
    eng.close()
