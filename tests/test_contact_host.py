"""The contact query without a GPU: the per-pair functions of csrc/pbre_contacts.hpp compiled for the host against tests/contact_ref.py,
the reference against model/contacts.py (its specification), the reference's own float32-vs-float64 figure (the GPU tests' tolerance), the
properties test_gpu_contact_query.py assumes of its state sets, a sanitizer run of the hull functions, the emulation library."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import camera_scenes as scn
import contact_ref as ref
import contact_scenes as cs
from pybullet_robot_envs import _capi
from pybullet_robot_envs.model import contacts
from pybullet_robot_envs.model.table import sphere_links

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# Measured by test_reference_float32_against_float64 below: the largest |float32 - float64| of contact_ref's `dist` over the GPU tests'
# state sets (the 131 Panda push states, every object shape against a hand sphere, on the table and over its edge, the iCub, the
# floating-base iCub, the iCub with hands and the robot-level Panda; forward kinematics included).  Measured: 2.53e-7 (robot-table, the box
# shape set); the constant is that figure rounded up to one digit.
REF32_DIST = 3e-7
# what the GPU tests allow (test_gpu_contact_query.py): the device does its FK in fp32 with another operation order
GPU_DIST = 4 * REF32_DIST
# the host build of the device's functions against the float64 reference on the same float32 inputs (no FK): every distance is a handful
# of rounded operations on coordinates below 2 m, 2^-23 relative each
HOST_DIST = 16 * 2.0 ** -23 * 2.0


@pytest.fixture(scope="module")
def host():
    d = os.path.join(ROOT, "tests", "contact_host")
    subprocess.check_call(["make", "-s", "-C", d])
    lib = C.CDLL(os.path.join(d, "build", "libpbre_contact_host.so"))
    lib.cq_hull_rb_max.restype = C.c_float
    for f in ("cq_sphere_object", "cq_sphere_table", "cq_object_table"):
        getattr(lib, f).restype = None
    return lib


def _p(a):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


def _hull_table(host, hull):
    out = np.zeros(host.cq_hull_floats(), np.float32)
    v = np.ascontiguousarray(hull, np.float64)
    assert host.cq_build_hull(_p(v), C.c_int(len(v)), _p(out)) == 0
    return out


SHAPES = dict(scn.SHAPES, compound3=(3, None, cs.SHAPE3))


@pytest.mark.parametrize("name", list(SHAPES))
def test_host_sphere_object(host, name):
    shape, oh, hull = SHAPES[name]
    oh = np.array(cs.hull_half(hull) if hull is not None else oh, np.float32)
    H = _hull_table(host, hull) if hull is not None else None
    rng = np.random.default_rng(3)
    n = 4000
    op = np.array([0.55, 0.1, 0.7], np.float32)
    quat = scn.quat_axis_angle([0.3, -0.5, 0.8], 0.9).astype(np.float32)
    Ro = contacts._quat_R(quat[None].astype(float))[0]
    # centres inside the object, around its surface and far outside the early-out radius
    scale = np.where(np.arange(n) % 4 == 0, 0.01, np.where(np.arange(n) % 4 == 3, 0.6, 0.08))[:, None]
    sc = (op + rng.uniform(-1, 1, (n, 3)) * scale).astype(np.float32)
    sr = rng.uniform(0.0, 0.03, n).astype(np.float32)
    margin = np.float32(1e-3)
    rb = host.cq_hull_rb_max(_p(H)) if H is not None else 0.0
    reach = np.float32(margin + rb)
    got = np.empty(n, np.float32)
    Rf = np.ascontiguousarray(contacts._quat_R(quat[None])[0], np.float32)
    host.cq_sphere_object(n, shape, _p(sc), _p(sr), _p(op), _p(Rf), _p(oh), _p(H), C.c_float(reach), _p(got))
    pieces = ref.hull_faces(hull) if hull is not None else None
    want = ref.sphere_object_dist(sc.astype(float), sr.astype(float), np.broadcast_to(op.astype(float), (n, 3)), np.broadcast_to(Rf.astype(float), (n, 3, 3)),
                                  shape, oh.astype(float), pieces)
    exact = want < reach if shape == 3 else np.ones(n, bool)
    assert (want < 0).sum() > 100 and exact.sum() > 1000 and (shape != 3 or (~exact).sum() > 100), (name, (want < 0).sum(), exact.sum())
    err = np.abs(got[exact] - want[exact])
    print("%s: largest |host - ref| %.3g over %d exact distances" % (name, err.max(), exact.sum()))
    assert err.max() <= HOST_DIST
    # beyond the reach: a lower bound that never drops below the margin
    assert (got[~exact] <= want[~exact] + HOST_DIST).all() and (got[~exact] >= margin).all()
    assert abs(Ro - Rf).max() < 1e-6


def test_host_sphere_table(host):
    rng = np.random.default_rng(4)
    n = 4000
    tc, th = np.array([0.85, 0.0, 0.6], np.float32), np.array([0.75, 0.5, 0.025], np.float32)
    sc = (tc + rng.uniform(-1.2, 1.2, (n, 3)) * th * np.where(np.arange(n) % 2 == 0, 1.0, 1.5)[:, None]).astype(np.float32)
    sr = rng.uniform(0.0, 0.05, n).astype(np.float32)
    got = np.empty(n, np.float32)
    host.cq_sphere_table(n, _p(sc), _p(sr), _p(tc), _p(th), _p(got))
    eye = np.broadcast_to(np.eye(3), (n, 3, 3))
    want = contacts._sphere_box_dist(sc.astype(float), sr.astype(float), np.broadcast_to(tc.astype(float), (n, 3)), eye, th.astype(float))
    assert (want < 0).sum() > 500 and (want > 0).sum() > 500
    assert np.abs(got - want).max() <= HOST_DIST


@pytest.mark.parametrize("name", list(SHAPES))
def test_host_object_table(host, name):
    shape, oh, hull = SHAPES[name]
    oh = tuple(cs.hull_half(hull) if hull is not None else oh)
    H = _hull_table(host, hull) if hull is not None else None
    rng = np.random.default_rng(5)
    n = 600
    ph = cs.phys_like(shape, oh)
    pose = np.zeros((n, 7), np.float32)
    pose[:, 0] = np.where(np.arange(n) % 3 == 0, 0.1 + rng.uniform(-0.08, 0.08, n), rng.uniform(0.3, 1.4, n))       # a third over the edge x = 0.1
    pose[:, 1] = rng.uniform(-0.6, 0.6, n)
    pose[:, 2] = 0.625 + rng.uniform(-0.08, 0.12, n)
    pose[:, 3:] = cs.random_quats(rng, n, 3.0)
    r = ref.query(np.asarray(_table1(), float), cs.compact(np.zeros((n, 1), np.float32), pose), 1, ph, hull=hull)
    got = np.empty(n, np.float32)
    tc, th, ohf = (np.array(x, np.float32) for x in (ph.table_c, ph.table_h, oh))
    host.cq_object_table(n, shape, _p(pose), _p(ohf), _p(H), _p(tc), _p(th), _p(got))
    want = r["dist"][:, 0]
    clear = r["edge"] > 1e-5                   # a candidate within rounding of the table's outline may count on one side only
    none = want > 1e38
    assert clear.sum() > 0.95 * n and none[clear].sum() > 10 and (~none[clear]).sum() > 200
    assert np.array_equal(got[clear] > 1e38, none[clear])
    ok = clear & ~none
    assert np.abs(got[ok] - want[ok]).max() <= HOST_DIST
    assert (r["d_ot"] > 1e38).any(axis=1)[ok].sum() > 20, "no pose with only a part of the candidates counting"


def _table1():
    """a RobotTable of one revolute link and one sphere (far from everything): the smallest robot contact_ref.query accepts"""
    from pybullet_robot_envs.model.table import build_table
    link = dict(name="l0", parent=-1, jtype=1, axis=[0, 0, 1], origin_xyz=[0, 0, 0], origin_R=np.eye(3), mass=1.0, com=[0, 0, 0], inertia=np.eye(3),
                lower=-1.0, upper=1.0, damping=0.0, lateral_friction=None)
    return build_table(dict(links=[link], base_position=[0.0, 0.0, 5.0], base_R=np.eye(3)), [("l0", [0, 0, 0], 0.01)], 0)


def test_sanitized_hull_functions(host):
    """the stand-alone program of tests/contact_host (AddressSanitizer + UBSan): tables of 1 and 4 pieces, 4 and 32 vertices per piece"""
    out = subprocess.run([os.path.join(ROOT, "tests", "contact_host", "build", "contact_san")], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0 and "contact_san OK" in out.stdout, out.stdout + out.stderr


# ---------------------------------------------------------------------------------------------- the reference against its specification
@pytest.fixture(scope="module")
def panda_set(panda):
    return cs.panda_states(panda)


def test_reference_is_contact_flags(panda, panda_set):
    tbl = panda["table"]
    R0, p0 = contacts.link_frames(tbl, panda_set[:, :9].astype(float))
    R1, p1 = ref.link_frames(tbl, panda_set[:, :9].astype(float))
    assert np.array_equal(R0, R1) and np.array_equal(p0, p1)
    r = ref.query(tbl, panda_set, 9, cs.phys_like())
    assert np.array_equal(r["flags"], contacts.contact_flags(tbl, panda_set, 9, cs.phys_like()))
    rng = np.random.default_rng(2)
    for name in SHAPES:
        q, pose, ph, hull = cs.shape_set(tbl, scn.PANDA_HOME, name, rng)
        st = cs.compact(q, pose)
        r = ref.query(tbl, st, 9, ph, hull=hull)
        assert np.array_equal(r["flags"], contacts.contact_flags(tbl, st, 9, ph, hull=hull)), name
    r = ref.query(tbl, panda_set, 9, cs.phys_like(), no_object=True)
    assert np.array_equal(r["flags"], contacts.contact_flags(tbl, panda_set, 9, cs.phys_like(), no_object=True))
    assert (r["dist"][:, :2] > 1e38).all() and (r["nearest"][:, 0] == -1).all() and not r["count"][:, 0].any() and not r["tips"].any()
    links, names = sphere_links(tbl, panda["model"])
    assert len(links) == 13 and names[int(r["nearest"][0, 1])] == panda["model"]["links"][links[int(r["nearest"][0, 1])]]["name"]


def _all_sets(panda, panda_set):
    """(name, table, compact records, obj_off, phys, hull) of every state set of test_gpu_contact_query.py"""
    tbl = panda["table"]
    out = [("panda", tbl, panda_set, 9, cs.phys_like(), None)]
    rng = np.random.default_rng(2)
    for name in SHAPES:
        q, pose, ph, hull = cs.shape_set(tbl, scn.PANDA_HOME, name, rng)
        out.append((name, tbl, cs.compact(q, pose), 9, ph, hull))
    for name, (t, nd, q0, spread) in cs.robot_sets().items():
        tips = cs.tip_spheres(t)
        q, pose, ph, hull = cs.shape_set(t, q0, "box", np.random.default_rng(6), n=8, spread=spread, tip_sphere=tips[1] if tips else None)
        out.append((name, t, cs.compact(q, pose), nd, ph, hull))
    return out


def test_state_sets_suit_the_gpu_tests(panda, panda_set):
    """what test_gpu_contact_query.py assumes, shown on the reference alone: at most 2 % of a batch within GPU_DIST of the margin, no
    candidate point within 0.1 mm of the table's outline, every flag value the sets are meant to show"""
    seen = set()
    for name, tbl, st, off, ph, hull in _all_sets(panda, panda_set):
        for mg in (None, 0.01, 0.0):
            r = ref.query(tbl, st, off, ph, margin=mg, hull=hull)
            assert ref.band(r, GPU_DIST).mean() <= 0.02, (name, mg)
            assert r["edge"].min() > 1e-4, (name, r["edge"].min())
            if mg is None:
                seen |= {(name, int(f)) for f in r["flags"]}
                if name in SHAPES:
                    # (a sphere beside the chosen one may touch the object too, so "outside the margin" is not asked of every shape)
                    assert (r["flags"][:-2] & 2).any() and r["flags"][-2] & 1 and r["flags"][-1] & 1, (name, r["flags"])
                    cnt = (r["d_ot"] < 1e38).sum(axis=1)
                    assert name == "sphere" or 0 < cnt[-1] < cnt[-2], (name, cnt)      # (the sphere has one candidate)
    assert {f for n, f in seen if n == "panda"} >= {0, 1, 2, 5}
    assert len({n for n, f in seen if n in SHAPES and f & 2 == 0}) >= 3 and len({n for n, f in seen if n in SHAPES and f & 2}) == len(SHAPES)
    assert any(ref.query(t, st, off, ph)["tips"].any() for name, t, st, off, ph, _ in _all_sets(panda, panda_set) if name in ("hands", "panda_arm"))


def test_reference_float32_against_float64(panda, panda_set):
    worst = 0.0
    for name, tbl, st, off, ph, hull in _all_sets(panda, panda_set):
        r64 = ref.query(tbl, st, off, ph, hull=hull, dtype=np.float64)
        r32 = ref.query(tbl, st, off, ph, hull=hull, dtype=np.float32)
        assert r32["dist"].dtype == np.float32
        far = r64["dist"] > 1e38
        assert np.array_equal(far, r32["dist"] > 1e38), name
        err = np.where(far, 0.0, np.abs(r64["dist"] - r32["dist"].astype(float))).max(axis=0)
        print("%-10s %3d envs  |dist32 - dist64| object-table %.3g  robot-object %.3g  robot-table %.3g" % (name, len(st), err[0], err[1], err[2]))
        worst = max(worst, err.max())
    print("largest: %.3g" % worst)
    assert worst <= REF32_DIST


# ---------------------------------------------------------------------------------------------- emulation library
def test_emulation_library_has_no_contact_query(panda, emu_lib):
    assert not hasattr(emu_lib, "pbre_contact_query")
    eng = _capi.Engine(panda["table"], task=_capi.TASK_PUSH, num_envs=2, lib=emu_lib)
    with pytest.raises(RuntimeError, match="no contact query"):
        eng.contact_query()
    eng.close()
