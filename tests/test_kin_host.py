"""The kinematics / dynamics query without a GPU: tests/kin_ref.py against the oracle in float64 (its specification: link frames, the
inverse of M by articulated-body impulse responses, forward dynamics, finite differences of the link frames), its own consistency
(vel = J qd, M symmetric positive definite, gravity torques = the gradient of the potential energy), the walks of csrc/pbre_kin.hpp compiled
for the host against it on the same float32 inputs, a sanitizer run of those walks, the reference's float32-vs-float64 figures (the GPU
tests' tolerances), the emulation library."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import kin_ref as ref
import kin_scenes as ks
import orc
from pybullet_robot_envs import _capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ["panda", "panda_arm", "icub", "icub_float", "hands"]

# Measured by test_reference_float32_against_float64 below: the largest |float32 - float64| of kin_ref's outputs over the GPU tests' state
# sets (kin_scenes.all_sets: the 131 Panda push records, 8 envs each of the iCub, the floating-base iCub, the iCub with hands and the
# robot-level Panda), forward kinematics included.  Each constant is the measured figure rounded up to one digit.
REF32_POS = 3e-7      # m; measured 2.31e-7 (panda)
REF32_QUAT = 2e-7     # measured 1.81e-7 (hands)
REF32_VEL = 2e-6      # m/s, rad/s; measured 1.08e-6 (hands)
REF32_JAC = 3e-7      # measured 2.52e-7 (icub)
REF32_MASS = 2e-6     # |dM_ij| / sqrt(M_ii M_jj); measured 1.15e-6 (icub_float)
REF32_TAU = 3e-6      # |dtau_j| / (1 + |tau_j|); measured 2.37e-6 (icub_float)
REF32 = dict(pos=REF32_POS, quat=REF32_QUAT, vel=REF32_VEL, jac=REF32_JAC, mass=REF32_MASS, tau=REF32_TAU)
# what the GPU tests allow (test_gpu_kin_query.py): the device runs other recursions in another operation order (the contact query's rule)
GPU_TOL = {k: 4 * v for k, v in REF32.items()}


@pytest.fixture(scope="module")
def tables(panda):
    return ks.tables(panda)


def _samples(tables, name, n=12, seed=5):
    t, q0, spread = tables[name]
    return (t,) + tuple(x.astype(float) for x in ks.robot_samples(t, q0, spread, n=n, seed=seed))


def _oracle(t):
    ora = orc.Oracle(t)
    ora.params.lin_damping = 0.0; ora.params.ang_damping = 0.0      # the query is rigid bodies only
    return ora


def _damping(t):
    K = ref.links_of(t)
    d = np.zeros(K["nd"])
    j = K["jtype"] != 0
    d[K["dof"][j]] = K["damping"][j]
    return d


# ---------------------------------------------------------------------------------------------- the reference against the oracle, float64
@pytest.mark.parametrize("name", NAMES)
def test_reference_against_oracle(tables, name):
    t, q, qd, qdd = _samples(tables, name)
    ora = _oracle(t)
    r = ref.query(t, q, qd, qdd, gravity_z=ora.params.gravity_z)
    nd, damp = int(t[3]), _damping(t)
    e_fk = e_m = e_fd = 0.0
    for e in range(len(q)):
        R, p = ora.fk(q[e])
        e_fk = max(e_fk, np.abs(R - r["R"][e]).max(), np.abs(p - r["p"][e]).max())
        e_m = max(e_m, np.abs(r["mass"][e] @ ora.minv(q[e]) - np.eye(nd)).max())
        e_fd = max(e_fd, np.abs(ora.forward_dynamics(q[e], qd[e], r["tau"][e] + damp * qd[e]) - qdd[e]).max())
    print("%s: frames %.2g  M Minv - I %.2g  forward dynamics %.2g" % (name, e_fk, e_m, e_fd))
    assert e_fk <= 1e-12 and e_m <= 1e-10 and e_fd <= 1e-9


@pytest.mark.parametrize("name", NAMES)
def test_reference_jacobian_against_finite_differences(tables, name):
    t, q, qd, _ = _samples(tables, name)
    ora = _oracle(t)
    nd, ee, h = int(t[3]), int(t[4]), 1e-6
    r = ref.query(t, q, qd)
    worst = 0.0
    for e in range(len(q)):
        for d in range(nd):
            dq = np.zeros(nd); dq[d] = h
            col = (ora.fk(q[e] + dq)[1][ee] - ora.fk(q[e] - dq)[1][ee]) / (2 * h)
            worst = max(worst, np.abs(col - r["jac"][e, :3, d]).max())
    print("%s: linear Jacobian of link %d against central differences of orc_fk: %.2g" % (name, ee, worst))
    assert worst <= 1e-8


@pytest.mark.parametrize("name", NAMES)
def test_reference_is_consistent(tables, name):
    t, q, qd, _ = _samples(tables, name, n=6)
    K = ref.links_of(t)
    # vel = J qd of the same point, at the origin and at the centre of mass (every link; every third one of the hands model, tips included)
    for at_com in (False, True):
        r = ref.query(t, q, qd, at_com=at_com)
        for li in sorted(set(range(0, K["nl"], 3 if K["nl"] > 40 else 1)) | {K["nl"] - 1}):
            J = ref.query(t, q, qd, links=[li], jac_link=li, jac_at_com=at_com)["jac"]
            assert np.abs(np.einsum("nij,nj->ni", J, qd) - r["vel"][:, li]).max() <= 1e-12, (name, li, at_com)
    M = r["mass"]
    assert np.abs(M - M.transpose(0, 2, 1)).max() <= 1e-14 * np.abs(M).max()
    assert np.linalg.eigvalsh(0.5 * (M + M.transpose(0, 2, 1))).min() > 0
    # gravity torques: qd = qdd = 0 gives the gradient of the potential energy (tau holds the robot against gravity)
    g = ref.query(t, q, np.zeros_like(q))["tau"]
    h = 1e-6
    worst = 0.0
    for d in range(K["nd"]):
        dq = np.zeros_like(q); dq[:, d] = h
        worst = max(worst, np.abs((ref.potential_energy(t, q + dq) - ref.potential_energy(t, q - dq)) / (2 * h) - g[:, d]).max())
    print("%s: gravity torque against dU/dq: %.2g" % (name, worst))
    assert worst <= 1e-7
    # a jac_point moves the linear rows by -[R pt]x times the angular rows
    pt = np.array([0.02, -0.03, 0.05], np.float32)
    a, b = ref.query(t, q, qd), ref.query(t, q, qd, jac_point=pt)
    off = np.einsum("nij,j->ni", a["R"][:, K["ee"]], pt.astype(float))
    assert np.abs(b["jac"][:, :3] - (a["jac"][:, :3] + np.cross(a["jac"][:, 3:].transpose(0, 2, 1), off[:, None, :]).transpose(0, 2, 1))).max() <= 1e-12


def test_quaternions_of_every_branch():
    rng = np.random.default_rng(8)
    qs = rng.normal(size=(400, 4))
    qs[:100, 3] *= 0.05                                  # rotations by nearly pi: the three diagonal branches
    qs /= np.linalg.norm(qs, axis=1, keepdims=True)
    x, y, z, w = qs.T
    R = np.stack([1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w), 2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w),
                  2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)], -1).reshape(-1, 3, 3)
    got = ref.quat_of(R)
    want = np.where(w[:, None] < 0, -qs, qs)
    assert np.abs(got - want).max() <= 1e-12 and (got[:, 3] >= 0).all()
    tr = np.trace(R, axis1=1, axis2=2)
    assert all(((np.argmax(np.concatenate([tr[:, None], np.einsum("nii->ni", R)], 1), axis=1)) == k).any() for k in range(4))


# ---------------------------------------------------------------------------------------------- the device's walks, compiled for the host
@pytest.fixture(scope="module")
def host():
    d = os.path.join(ROOT, "tests", "kin_host")
    subprocess.check_call(["make", "-s", "-C", d])
    lib = C.CDLL(os.path.join(d, "build", "libpbre_kin_host.so"))
    lib.kin_query.restype = None
    lib.kin_quat.restype = None
    return lib


def _p(a):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


def host_query(host, t, q, qd, qdd=None, g_up=9.8, links=None, at_com=False, jac_link=None, jac_point=(0, 0, 0), jac_at_com=False,
               want=("pose", "vel", "jac", "mass", "tau")):
    t = np.ascontiguousarray(t, np.float64)
    nl, nd = int(t[2]), int(t[3])
    n = len(q)
    W, _ = ks.lanes(nd)
    st = np.zeros((n, 2 * W + 16), np.float32)
    st[:, :nd] = q; st[:, W:W + nd] = qd
    links = np.arange(nl, dtype=np.int32) if links is None else np.ascontiguousarray(links, np.int32)
    shapes = dict(pose=(n, len(links), 7), vel=(n, len(links), 6), jac=(n, 6, nd), mass=(n, nd, nd), tau=(n, nd))
    out = {k: np.full(shapes[k], np.nan, np.float32) for k in want}
    pt = np.ascontiguousarray(jac_point, np.float32)
    qdd = None if qdd is None else np.ascontiguousarray(qdd, np.float32)
    host.kin_query(_p(t), n, _p(st), st.shape[1], W, C.c_float(g_up), len(links), _p(links), int(at_com), int(t[4]) if jac_link is None else int(jac_link),
                   _p(pt), int(jac_at_com), _p(qdd), *[_p(out.get(k)) for k in ("pose", "vel", "jac", "mass", "tau")])
    return out


@pytest.mark.parametrize("name", NAMES)
def test_host_walks_against_reference(host, tables, name):
    """every output of the host build within 4 x the reference's own float32 figure of the float64 reference on the same float32 inputs (the
    bound the GPU tests use: the walks are the device's)"""
    t, q0, spread = tables[name]
    q, qd, qdd = ks.robot_samples(t, q0, spread, n=12, seed=9)
    nl = int(t[2])
    cases = [dict(), dict(at_com=True, jac_link=nl - 1, jac_point=(0.02, -0.03, 0.05)), dict(jac_link=nl // 2, jac_at_com=True, links=[nl - 1, 0, 3, nl - 1])]
    for kw in cases:
        got = host_query(host, t, q, qd, qdd, **kw)
        want = ref.query(t, q, qd, qdd, **kw)
        err = ref.errors(want, got)
        print(name, kw, {k: "%.2g" % v for k, v in err.items()})
        for k, v in err.items():
            assert v <= GPU_TOL[k], (name, kw, k, v)
        assert np.array_equal(got["mass"], got["mass"].transpose(0, 2, 1)) and (got["pose"][..., 6] >= 0).all()
    zero = host_query(host, t, q, qd, np.zeros_like(qdd), want=("tau",))
    none = host_query(host, t, q, qd, None, want=("tau",))
    assert zero["tau"].tobytes() == none["tau"].tobytes()
    one = host_query(host, t, q, qd, qdd, want=("mass",))
    assert one["mass"].tobytes() == host_query(host, t, q, qd, qdd)["mass"].tobytes()


def test_host_quaternions(host):
    rng = np.random.default_rng(8)
    qs = rng.normal(size=(400, 4))
    qs[:100, 3] *= 0.05
    qs /= np.linalg.norm(qs, axis=1, keepdims=True)
    x, y, z, w = qs.T
    R = np.stack([1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w), 2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w),
                  2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)], -1).astype(np.float32)
    got = np.empty((400, 4), np.float32)
    host.kin_quat(400, _p(R), _p(got))
    want = ref.quat_of(R.reshape(-1, 3, 3).astype(float))
    flip = np.abs(want[:, 3]) < 1e-3
    d = np.abs(got - want).max(axis=1)
    d = np.where(flip, np.minimum(d, np.abs(got + want).max(axis=1)), d)
    assert d.max() <= GPU_TOL["quat"] and (got[:, 3] >= 0).all()


def test_sanitized_walks(host, tables, tmp_path):
    """the stand-alone program of tests/kin_host (AddressSanitizer + UBSan) on the largest table and on the one with prismatic joints"""
    paths = []
    for name in ("hands", "icub_float"):
        p = tmp_path / (name + ".f64")
        np.ascontiguousarray(tables[name][0], np.float64).tofile(p)
        paths.append(str(p))
    out = subprocess.run([os.path.join(ROOT, "tests", "kin_host", "build", "kin_san")] + paths, capture_output=True, text=True, timeout=120)
    assert out.returncode == 0 and "kin_san OK" in out.stdout, out.stdout + out.stderr
    assert "62 links, 60 DoF" in out.stdout and "26 DoF, 3 prismatic" in out.stdout, out.stdout


# ---------------------------------------------------------------------------------------------- the GPU tolerances, measured
def test_reference_float32_against_float64(panda):
    worst = {k: 0.0 for k in REF32}
    for name, t, q, qd, qdd in ks.all_sets(panda):
        r64 = ref.query(t, q, qd, qdd, dtype=np.float64)
        r32 = ref.query(t, q, qd, qdd, dtype=np.float32)
        assert all(r32[k].dtype == np.float32 for k in ("pose", "vel", "jac", "mass", "tau"))
        err = ref.errors(r64, r32)
        print("%-10s %3d envs  " % (name, len(q)) + "  ".join("%s %.3g" % kv for kv in err.items()))
        worst = {k: max(worst[k], err[k]) for k in worst}
    print("largest: " + "  ".join("%s %.3g" % kv for kv in worst.items()))
    for k in worst:
        assert worst[k] <= REF32[k], (k, worst[k])


# ---------------------------------------------------------------------------------------------- emulation library
def test_emulation_library_has_no_kin_query(panda, emu_lib):
    assert not hasattr(emu_lib, "pbre_kin_query")
    eng = _capi.Engine(panda["table"], task=_capi.TASK_PUSH, num_envs=2, lib=emu_lib)
    with pytest.raises(RuntimeError, match="no kinematics query"):
        eng.kin_query()
    eng.close()
