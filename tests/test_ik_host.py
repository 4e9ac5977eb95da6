"""The inverse-kinematics query without a GPU: tests/ik_ref.py against the oracle's orc_ik in float64 (its specification), the
position-only mode by its own properties, the solve of csrc/pbre_ik.hpp compiled for the host against the reference on the same float32
inputs, a sanitizer run of that solve, the reference's float32-vs-float64 figures (the GPU tests' tolerances) and the share of envs whose
stopping decision float32 arithmetic may legitimately take differently, the emulation library."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import contact_ref
import ik_ref as ref
import ik_scenes as sc
import kin_ref
import kin_scenes as ks
import orc
from pybullet_robot_envs import _capi
from pybullet_robot_envs.model.table import hand_pose_target

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# Measured by test_reference_float32_against_float64 below: the largest |float32 - float64| of ik_ref's outputs over the input sets of the
# GPU tolerance tests (ik_scenes.cases), envs whose stopping decision is ambiguous left out (they are skipped there too).  Each constant is
# the measured figure rounded up to one digit.
REF32_Q = 2e-6         # rad (m for a prismatic joint); measured 1.50e-6 (hands_tip_fingers_3d: up to 100 updates of the finger joints)
REF32_ERR_POS = 4e-7   # m; measured 3.61e-7 (panda_forced_3d)
REF32_ERR_ROT = 3e-7   # rad; measured 2.89e-7 (panda_point)
REF32 = dict(q=REF32_Q, err_pos=REF32_ERR_POS, err_rot=REF32_ERR_ROT)
# what the GPU tests allow (test_gpu_ik_query.py): the device runs the same iteration in another operation order (the kin query's rule)
GPU_TOL = {k: 4 * v for k, v in REF32.items()}
AMBIGUOUS_MAX = 0.02   # share of a batch whose stopping decision may be ambiguous (a condition of the tests, not a measurement)


def errors(want, got, keep=None):
    """the three figures the tolerances are stated in, of `got` against `want` (dicts with "q" and "err"), over the envs `keep`"""
    keep = np.ones(len(want["q"]), bool) if keep is None else keep
    f = lambda a: np.asarray(a, float)[keep]
    return dict(q=np.abs(f(got["q"]) - f(want["q"])).max(initial=0.0), err_pos=np.abs(f(got["err"])[:, 0] - f(want["err"])[:, 0]).max(initial=0.0),
                err_rot=np.abs(f(got["err"])[:, 1] - f(want["err"])[:, 1]).max(initial=0.0))


def ambiguous_of(r, kw):
    return ref.ambiguous(r, GPU_TOL["err_pos"], float(np.float32(kw.get("residual", 1e-3))), GPU_TOL["err_rot"], float(np.float32(kw.get("rot_residual", 0.0))))


# ---------------------------------------------------------------------------------------------- the reference against the oracle, float64
def _oracle(name):
    if name == "panda":
        o, t = orc.panda_oracle(task=1)
        o.set_ik_mode(True)
        return o, t
    if name == "panda_arm":
        return orc.panda_arm_oracle(use_ik=1)
    o, t, _ = orc.icub_arm_oracle("l", use_ik=1, control_orientation=1, floating_base=(name == "icub_float"))
    return o, t


@pytest.mark.parametrize("name", ["panda", "icub", "panda_arm", "icub_float"])
def test_reference_against_oracle(panda, name):
    """6-D mode through the hand_pose convention (Euler angles, ik_link_offset) against orc_ik at its defaults: the same iteration counts,
    q within 1e-9.  The floating-base iCub adds the ik_passive virtual joints, which neither may move."""
    o, t = _oracle(name)
    t = np.asarray(t, float)
    _, q0, spread = ks.tables(panda)[name]
    q, _, _ = ks.robot_samples(t, q0, spread, n=10, seed=41)
    q = q.astype(float)
    rng = np.random.default_rng(42)
    K, ee, moving, lower, upper = ref.chain_info(t)
    qt = q.copy()
    qt[:, moving] += rng.normal(0, 0.2, (len(q), moving.sum()))
    R, p = contact_ref.link_frames(t, qt)
    off = np.array([o.task.ik_link_offset[k] for k in range(3)])
    if name.startswith("icub"):
        assert np.abs(off).max() > 0.01
    eul = np.array([_capi_euler(R[e, ee]) for e in range(len(q))])
    pos = p[:, ee] - np.einsum("nij,j->ni", R[:, ee], off)                     # the hand pose whose link-frame target is p
    tp, tq = hand_pose_target(np.concatenate([pos, eul], axis=1), off)
    r = ref.solve(t, q, tp, tq, damping=o.task.ik_damping, residual=o.task.ik_residual, max_iters=o.task.ik_max_iters)
    worst = 0.0
    for e in range(len(q)):
        qo, it = o.ik(q[e], pos[e], eul[e])
        assert it == r["iters"][e], (name, e, it, r["iters"][e])
        worst = max(worst, np.abs(qo - r["q"][e]).max())
    print("%s: %d..%d iterations, q against orc_ik %.2g" % (name, r["iters"].min(), r["iters"].max(), worst))
    assert worst <= 1e-9 and r["iters"].min() >= 1 and r["iters"].max() < o.task.ik_max_iters
    assert np.array_equal(r["q"][:, ~moving], q[:, ~moving])
    if name == "icub_float":
        passive = np.asarray(t[24:24 + 40 * K["nl"]]).reshape(-1, 40)[:, 37] != 0
        assert passive.sum() == 6 and not moving[K["dof"][passive]].any()


def _capi_euler(R):
    """roll, pitch, yaw of a rotation matrix (pybullet.getEulerFromQuaternion's convention, away from the poles)"""
    return np.array([np.arctan2(R[2, 1], R[2, 2]), -np.arcsin(np.clip(R[2, 0], -1, 1)), np.arctan2(R[1, 0], R[0, 0])])


# ---------------------------------------------------------------------------------------------- position-only mode
def test_position_only(panda):
    c = sc.cases(panda)["panda_default_3d"]
    t, q = c["table"], c["q"].astype(float)
    tp = c["kw"]["target_pos"]
    r = ref.solve(t, q, tp)
    R, p = contact_ref.link_frames(t, r["q"])
    ee = int(t[4])
    d = np.linalg.norm(p[:, ee] - tp, axis=1)
    assert (r["iters"] < 100).all() and (d < 1e-3).all() and np.abs(d - r["err"][:, 0]).max() <= 1e-12 and not r["err"][:, 1].any()
    # one update with a small damping is the least-squares step (the minimum-norm solution of J dq = e): J^T (J J^T + l^2)^-1 e differs from
    # pinv(J) e by a relative l^2 / sigma_min^2; with l = 1e-5 and the Panda's sigma_min > 1e-2 on these states that is below 1e-6
    one = ref.solve(t, q, tp, damping=1e-5, residual=0.0, max_iters=1)
    K, _, moving, _, _ = ref.chain_info(t)
    R0, p0 = contact_ref.link_frames(t, q)
    J = kin_ref.point_jacobian(K, R0, p0, ee, p0[:, ee], np.float64)[:, :3]
    worst = 0.0
    for e in range(len(q)):
        assert np.linalg.svd(J[e][:, moving], compute_uv=False).min() > 1e-2
        dq = np.linalg.lstsq(J[e][:, moving], tp[e] - p0[e, ee], rcond=None)[0]
        worst = max(worst, np.abs(one["q"][e, moving] - q[e, moving] - dq).max() / np.abs(dq).max())
    print("position only: the small-damping update against numpy.linalg.lstsq, relative %.2g" % worst)
    assert worst <= 1e-6 and (one["iters"] == 1).all()


# ---------------------------------------------------------------------------------------------- the device's solve, compiled for the host
@pytest.fixture(scope="module")
def host():
    d = os.path.join(ROOT, "tests", "ik_host")
    subprocess.check_call(["make", "-s", "-C", d])
    lib = C.CDLL(os.path.join(d, "build", "libpbre_ik_host.so"))
    lib.ik_query.restype = C.c_int
    return lib


def _p(a):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


def host_query(host, table, q_start, target_pos, target_quat=None, link=None, point=(0, 0, 0), dof_mask=None, damping=0.1, residual=1e-3,
               rot_residual=0.0, max_iters=100, clamp_limits=False):
    t = np.ascontiguousarray(table, np.float64)
    q0 = np.ascontiguousarray(q_start, np.float32)
    n, nd = q0.shape
    out = dict(q=np.full((n, nd), np.nan, np.float32), err=np.full((n, 2), np.nan, np.float32), iters=np.full(n, -1, np.int32))
    tp = np.ascontiguousarray(target_pos, np.float32)
    tq = None if target_quat is None else np.ascontiguousarray(target_quat, np.float32)
    m = None if dof_mask is None else np.ascontiguousarray(dof_mask, np.uint8)
    rc = host.ik_query(_p(t), n, _p(q0), int(t[4]) if link is None else int(link), _p(np.ascontiguousarray(point, np.float32)), _p(tp), _p(tq), _p(m),
                       C.c_float(damping), C.c_float(residual), C.c_float(rot_residual), int(max_iters), int(clamp_limits), _p(out["q"]), _p(out["err"]), _p(out["iters"]))
    assert rc == 0
    return out


CASES = ["panda_forced_6d", "panda_forced_3d", "panda_default_6d", "panda_default_3d", "panda_rot_residual", "panda_unreachable", "panda_point",
         "panda_clamp", "icub_forced_6d", "icub_default_6d", "icub_float_forced_6d", "icub_float_default_6d", "panda_arm_forced_6d",
         "panda_arm_default_6d", "hands_tip_3d", "hands_tip_fingers_3d", "hands_tip_forced_3d"]


@pytest.mark.parametrize("name", CASES)
def test_host_solve_against_reference(host, panda, name):
    """the host build of the device's solve on every input set of the GPU tests: outside the ambiguous envs the iteration counts of the
    float64 reference and of ik_ref(dtype=float32), q and err within the GPU tests' bound of the float64 reference and within 5 x REF32 of
    the float32 one (each is within its own bound of the float64 reference)"""
    c = sc.cases(panda)[name]
    got = host_query(host, c["table"], c["q"], **c["kw"])
    r64, r32 = sc.reference(panda, name), sc.reference(panda, name, np.float32)
    ok = ~ambiguous_of(r64, c["kw"])
    assert np.isfinite(got["q"]).all() and np.isfinite(got["err"]).all()
    assert np.array_equal(got["iters"][ok], r64["iters"][ok]) and np.array_equal(got["iters"][ok], r32["iters"][ok])
    e64, e32 = errors(r64, got, ok), errors(r32, got, ok)
    print(name, {k: "%.2g" % v for k, v in e64.items()}, "against float32:", {k: "%.2g" % v for k, v in e32.items()})
    for k in e64:
        assert e64[k] <= GPU_TOL[k] and e32[k] <= 5 * REF32[k], (name, k, e64[k], e32[k])
    K, _, moving, _, _ = ref.chain_info(c["table"], c["kw"].get("link"), c["kw"].get("dof_mask"))
    assert got["q"][:, ~moving].tobytes() == np.ascontiguousarray(c["q"][:, ~moving]).tobytes()


def test_host_options(host, panda):
    c = sc.cases(panda)["panda_default_6d"]
    t, q, kw = c["table"], c["q"], c["kw"]
    zero = host_query(host, t, q, max_iters=0, **kw)
    r0 = ref.solve(t, q, max_iters=0, **kw)
    assert zero["q"].tobytes() == q.tobytes() and not zero["iters"].any() and errors(r0, zero)["err_pos"] <= GPU_TOL["err_pos"] and errors(r0, zero)["err_rot"] <= GPU_TOL["err_rot"]
    scaled = host_query(host, t, q, kw["target_pos"], kw["target_quat"] * np.float32(3.7))
    plain = host_query(host, t, q, **kw)
    assert errors(plain, scaled)["q"] <= GPU_TOL["q"] and np.array_equal(plain["iters"], scaled["iters"])
    cl = sc.cases(panda)["panda_clamp"]
    got = host_query(host, cl["table"], cl["q"], **cl["kw"])
    K, _, moving, lower, upper = ref.chain_info(cl["table"])
    lo, hi = lower.astype(np.float32), upper.astype(np.float32)
    qm = got["q"][:, moving]
    assert (qm >= lo[moving]).all() and (qm <= hi[moving]).all() and ((qm == lo[moving]) | (qm == hi[moving])).sum() > 20
    free = host_query(host, cl["table"], cl["q"], **dict(cl["kw"], clamp_limits=False))
    assert ((free["q"][:, moving] < lo[moving]) | (free["q"][:, moving] > hi[moving])).any(), "the limits never bite: the case tests nothing"


def _serial_table(n_links, jtype):
    """a RobotTable of n_links links in one chain, 0.05 m apart along x, every joint of type jtype about z"""
    nd = n_links if jtype else 0
    t = np.zeros(24 + 40 * n_links)
    t[0], t[2], t[3], t[4], t[18] = 1346523717.0, n_links, nd, n_links - 1, 1.0
    t[9], t[13], t[17] = 1.0, 1.0, 1.0
    for i in range(n_links):
        r = t[24 + 40 * i: 64 + 40 * i]
        r[0], r[1], r[4], r[5], r[33] = i - 1, jtype, 1.0, 0.05, (i if jtype else -1)
        r[8], r[12], r[16] = 1.0, 1.0, 1.0
        r[30], r[31] = -3.0, 3.0
    return t


def test_chain_limits(host):
    """what the on-chip layout holds (include/pbre_ik.h: PBRE_IK_MAX_CHAIN = 64 links, PBRE_IK_MAX_MOVING = 24 moving DoFs): a chain at a
    limit is solved, one past it is refused (the C ABI turns the code into PBRE_E_UNSUPPORTED) and nothing is written"""
    def run(t, mask=None):
        nd = int(t[3])
        q0 = np.zeros((3, max(nd, 1)), np.float32)[:, :nd]
        q0 = np.ascontiguousarray(q0 + np.float32(0.1))
        out = np.full((3, nd), -7.0, np.float32)
        tp = np.tile(np.array([[0.3, 0.2, 0.0]], np.float32), (3, 1))
        m = None if mask is None else np.ascontiguousarray(mask, np.uint8)
        rc = host.ik_query(_p(np.ascontiguousarray(t)), 3, _p(q0), int(t[4]), _p(np.zeros(3, np.float32)), _p(tp), None, _p(m), C.c_float(0.1), C.c_float(1e-3),
                           C.c_float(0.0), 10, 0, _p(out), None, None)
        return rc, out
    rc, out = run(_serial_table(24, 1))
    assert rc == 0 and np.isfinite(out).all() and (out != np.float32(0.1)).any()
    rc, out = run(_serial_table(25, 1))
    assert rc == 2 and (out == -7).all()
    rc, out = run(_serial_table(25, 1), mask=[1] * 24 + [0])          # a mask brings it back under the limit
    assert rc == 0 and (out[:, 24] == np.float32(0.1)).all() and np.isfinite(out).all()
    assert run(_serial_table(64, 0))[0] == 0 and run(_serial_table(65, 0))[0] == 1


def test_sanitized_solve(host, panda, tmp_path):
    """the stand-alone program of tests/ik_host (AddressSanitizer + UBSan) on the hands model (the longest chain: torso, arm, finger) and on
    the floating-base iCub (prismatic and passive virtual joints)"""
    T = ks.tables(panda)
    paths = []
    for name in ("hands", "icub_float"):
        p = tmp_path / (name + ".f64")
        np.ascontiguousarray(T[name][0], np.float64).tofile(p)
        paths.append(str(p))
    out = subprocess.run([os.path.join(ROOT, "tests", "ik_host", "build", "ik_san")] + paths, capture_output=True, text=True, timeout=120)
    assert out.returncode == 0 and "ik_san OK (10 queries)" in out.stdout, out.stdout + out.stderr
    assert "62 links, 60 DoF" in out.stdout and "26 DoF" in out.stdout, out.stdout


# ---------------------------------------------------------------------------------------------- the GPU tolerances, measured
def test_reference_float32_against_float64(panda):
    worst = {k: (0.0, "") for k in REF32}
    for name in CASES:
        c = sc.cases(panda)[name]
        r64, r32 = sc.reference(panda, name), sc.reference(panda, name, np.float32)
        assert r32["q"].dtype == np.float32 and r32["err"].dtype == np.float32
        amb = ambiguous_of(r64, c["kw"])
        # a condition of the tests, not a measurement: at most 2 % of a batch may have an ambiguous stopping decision
        assert amb.mean() <= AMBIGUOUS_MAX, (name, amb.sum(), len(amb))
        assert np.array_equal(r32["iters"][~amb], r64["iters"][~amb]), name
        err = errors(r64, r32, ~amb)
        print("%-22s %3d envs  %d ambiguous  iterations %d..%d  " % (name, len(amb), amb.sum(), r64["iters"].min(), r64["iters"].max()) + "  ".join("%s %.3g" % kv for kv in err.items()))
        worst = {k: max(worst[k], (err[k], name)) for k in worst}
    print("largest: " + "  ".join("%s %.3g (%s)" % ((k,) + v) for k, v in worst.items()))
    for k in worst:
        assert worst[k][0] <= REF32[k], (k, worst[k])


def test_unreachable_targets_at_the_default_damping_are_chaotic(panda):
    """Why the unreachable targets are compared with the reference at damping 1 and not at the default 0.1: with an error of 2 m the
    update at damping 0.1 is several radians per joint, the iteration is chaotic, and the reference's own float32 arithmetic ends more than
    0.1 m from its float64 result after 20 updates -- no float32 implementation can be held to the float64 figures there.  At damping 1
    (steps bounded by |e| / (2 damping) = 1 rad) float32 follows float64 to REF32 (test_reference_float32_against_float64)."""
    c = sc.cases(panda)["panda_unreachable"]
    kw = dict(c["kw"], damping=0.1)
    far = np.arange(len(c["q"])) < sc.UNREACHABLE
    a, b = ref.solve(c["table"], c["q"][far], **_rows(kw, far)), ref.solve(c["table"], c["q"][far], dtype=np.float32, **_rows(kw, far))
    assert (a["iters"] == 20).all() and np.abs(a["err"][:, 0] - b["err"][:, 0]).max() > 0.1


def _rows(kw, keep):
    return {k: (v[keep] if k in ("target_pos", "target_quat") else v) for k, v in kw.items()}


# ---------------------------------------------------------------------------------------------- emulation library
def test_emulation_library_has_no_ik_query(panda, emu_lib):
    assert not hasattr(emu_lib, "pbre_ik_query")
    eng = _capi.Engine(panda["table"], task=_capi.TASK_PUSH, num_envs=2, lib=emu_lib)
    with pytest.raises(RuntimeError, match="no inverse-kinematics query"):
        eng.ik_query(np.zeros((2, 3), np.float32))
    eng.close()
