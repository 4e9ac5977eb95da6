"""State sets shared by the kinematics-query tests: test_kin_host.py measures kin_ref's float32-vs-float64 figures on them (the GPU
tolerances); test_gpu_kin_query.py places the same joint positions and velocities into engine records.  Nothing here needs a GPU."""
import numpy as np

import camera_scenes as scn
import contact_scenes as cs


def tables(panda):
    """name -> (RobotTable, q0, spread): the Panda task table and the four of contact_scenes.robot_sets()"""
    out = {"panda": (np.asarray(panda["table"], float), np.asarray(scn.PANDA_HOME, float), 0.2)}
    for name, (t, nd, q0, spread) in cs.robot_sets().items():
        out[name] = (t, q0, spread)
    return out


def lanes(nd):
    """lane width W and object offset of the engine's state record for a robot of nd DoF (include/pbre.h)"""
    return (16, 9) if nd <= 9 else ((32, 20) if nd <= 20 else ((64, 32) if nd <= 32 else (128, 60)))


def panda_records(panda):
    """the 131 records of contact_scenes.panda_states with the V lanes of the 9 joints ~ N(0, 1), and qdd ~ N(0, 3) [131, 9]"""
    st = cs.panda_states(panda).copy()
    rng = np.random.default_rng(21)
    st[:, 16:25] = rng.normal(0, 1, (len(st), 9)).astype(np.float32)
    return st, rng.normal(0, 3, (len(st), 9)).astype(np.float32)


def robot_samples(table, q0, spread, n=8, seed=22):
    """q, qd, qdd [n, nd] float32: configurations spread about q0, qd ~ N(0, 1), qdd ~ N(0, 3)"""
    nd = int(table[3])
    rng = np.random.default_rng(seed)
    q = np.asarray(q0, float)[None] + spread * rng.uniform(-1, 1, (n, nd))
    return q.astype(np.float32), rng.normal(0, 1, (n, nd)).astype(np.float32), rng.normal(0, 3, (n, nd)).astype(np.float32)


def all_sets(panda):
    """(name, table, q, qd, qdd) of every state set of test_gpu_kin_query.py"""
    T = tables(panda)
    st, qdd = panda_records(panda)
    out = [("panda", T["panda"][0], st[:, :9], st[:, 16:25], qdd)]
    for name in ("icub", "icub_float", "hands", "panda_arm"):
        t, q0, spread = T[name]
        out.append((name, t) + robot_samples(t, q0, spread))
    return out
