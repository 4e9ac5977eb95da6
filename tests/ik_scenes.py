"""Inputs shared by the inverse-kinematics tests: test_ik_host.py measures ik_ref's float32-vs-float64 figures on them (the GPU
tolerances), test_gpu_ik_query.py hands the same start values and targets to engines.  Nothing here needs a GPU.

Recipe: q_target = clip(q + N(0, 0.2), limits) on the DoFs that move, the target pose = the float64 forward kinematics of q_target rounded to
float32 -- reachable by construction, 2 to 14 iterations away at the defaults.  A handful of targets 2 m away exercise the iteration cap."""
import functools

import numpy as np

import contact_scenes as cs
import ik_ref
import kin_ref
import kin_scenes as ks

_CASES = {}
N_OTHER = 64          # envs of every engine but the Panda push one (131 records): one full wave
UNREACHABLE = 5


def reach_targets(table, q, link=None, point=(0, 0, 0), dof_mask=None, sigma=0.2, seed=31):
    """target_pos [N, 3], target_quat [N, 4] float32 (the pose of `point` of `link` at q_target) and q_target"""
    import contact_ref
    K, link, moving, lower, upper = ik_ref.chain_info(table, link, dof_mask)
    rng = np.random.default_rng(seed)
    qt = np.asarray(q, float).copy()
    step = rng.normal(0, sigma, qt.shape)
    lim = moving & (lower < upper)
    qt[:, moving] += step[:, moving]
    qt[:, lim] = np.clip(qt[:, lim], lower[lim], upper[lim])
    R, p = contact_ref.link_frames(table, qt)
    x = p[:, link] + np.einsum("nij,j->ni", R[:, link], np.asarray(point, np.float32).astype(float))
    return x.astype(np.float32), kin_ref.quat_of(R[:, link]).astype(np.float32), qt


def finger_mask(table, tip):
    """[nd] uint8: the DoFs on the chain to `tip` that are not on the chain to the table's ee_link (the finger joints)"""
    _, _, to_tip, _, _ = ik_ref.chain_info(table, tip)
    _, _, to_hand, _, _ = ik_ref.chain_info(table, None)
    return (to_tip & ~to_hand).astype(np.uint8)


def tip_link(table):
    """a link that carries a fingertip collision sphere (the last one), else the last link"""
    tips = cs.tip_spheres(table)
    return int(table[24 + int(table[2]) * 40 + tips[-1] * 8]) if tips else int(table[2]) - 1


@functools.lru_cache(maxsize=None)
def _robot(name):
    t, nd, q0, spread = cs.robot_sets()[name]
    q, _, _ = ks.robot_samples(t, q0, spread, n=N_OTHER, seed=23)
    return t, q


def cases(panda):
    if not _CASES:
        _CASES.update(_build_cases(panda))
    return _CASES


def _build_cases(panda):
    """name -> dict(table_name, table, q [N, nd] float32 start values, kw: the arguments of ik_ref.solve / Engine.ik_query but q_start).
    These are exactly the input sets of the tolerance tests of test_gpu_ik_query.py."""
    out = {}
    pt = np.asarray(panda["table"], float)
    st, _ = ks.panda_records(panda)
    q = st[:, :9].copy()
    tp, tq, _ = reach_targets(pt, q)
    forced = dict(residual=0.0, max_iters=8)
    out["panda_forced_6d"] = dict(table_name="panda", table=pt, q=q, kw=dict(target_pos=tp, target_quat=tq, **forced))
    out["panda_forced_3d"] = dict(table_name="panda", table=pt, q=q, kw=dict(target_pos=tp, **forced))
    out["panda_default_6d"] = dict(table_name="panda", table=pt, q=q, kw=dict(target_pos=tp, target_quat=tq))
    out["panda_default_3d"] = dict(table_name="panda", table=pt, q=q, kw=dict(target_pos=tp))
    out["panda_rot_residual"] = dict(table_name="panda", table=pt, q=q, kw=dict(target_pos=tp, target_quat=tq, rot_residual=2e-3))
    far = tp.copy()
    far[:UNREACHABLE] += np.array([2.0, 0.0, 0.0], np.float32)
    # (damping 1: at the default 0.1 an error of 2 m makes the iteration chaotic, test_ik_host.py shows it on the reference itself)
    out["panda_unreachable"] = dict(table_name="panda", table=pt, q=q, kw=dict(target_pos=far, target_quat=tq, max_iters=20, damping=1.0))
    point = (0.02, -0.03, 0.05)
    tpp, tqp, _ = reach_targets(pt, q, link=7, point=point, seed=32)
    out["panda_point"] = dict(table_name="panda", table=pt, q=q, kw=dict(target_pos=tpp, target_quat=tqp, link=7, point=point))
    up = tp + np.array([0.0, 0.0, 2.0], np.float32)      # every env reaches for a point 2 m above: joints run into their limits
    out["panda_clamp"] = dict(table_name="panda", table=pt, q=q, kw=dict(target_pos=up, target_quat=tq, max_iters=20, damping=1.0, clamp_limits=True))
    for name in ("icub", "icub_float", "panda_arm"):
        t, qo = _robot(name)
        a, b, _ = reach_targets(t, qo, seed=33)
        out[name + "_forced_6d"] = dict(table_name=name, table=t, q=qo, kw=dict(target_pos=a, target_quat=b, **forced))
        out[name + "_default_6d"] = dict(table_name=name, table=t, q=qo, kw=dict(target_pos=a, target_quat=b))
    t, qo = _robot("hands")
    tip = tip_link(t)
    mask = finger_mask(t, tip)
    a, _, _ = reach_targets(t, qo, link=tip, seed=34)
    out["hands_tip_3d"] = dict(table_name="hands", table=t, q=qo, kw=dict(target_pos=a, link=tip))
    a, _, _ = reach_targets(t, qo, link=tip, dof_mask=mask, seed=35)
    out["hands_tip_fingers_3d"] = dict(table_name="hands", table=t, q=qo, kw=dict(target_pos=a, link=tip, dof_mask=mask))
    out["hands_tip_forced_3d"] = dict(table_name="hands", table=t, q=qo, kw=dict(target_pos=a, link=tip, **forced))
    return out


_REF = {}


def reference(panda, name, dtype=np.float64):
    """ik_ref.solve of a case, computed once per process and shared (do not modify the arrays)"""
    key = (name, np.dtype(dtype).name)
    if key not in _REF:
        c = cases(panda)[name]
        _REF[key] = ik_ref.solve(c["table"], c["q"], dtype=dtype, **c["kw"])
    return _REF[key]
