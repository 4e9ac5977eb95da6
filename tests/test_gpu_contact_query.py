"""The batched contact query on the GPU (csrc/pbre_contacts.hip) against the float64 reference of tests/contact_ref.py on the same float32
state, by the comparison rule of that module (contact_ref.compare): `dist` within GPU_DIST (test_contact_host.py: the reference's measured
float32-vs-float64 figure times 4); flags, counts and fingertip bits equal except in envs where some pair's reference distance is within
GPU_DIST of the margin (at most 2 % of a batch); `nearest` equal unless the two smallest reference distances are within 2 GPU_DIST."""
import ctypes as C

import numpy as np
import pytest

import camera_scenes as scn
import contact_ref as ref
import contact_scenes as cs
import parity
from pybullet_robot_envs import _capi
from pybullet_robot_envs.model.objects import hull_pieces
from test_contact_host import GPU_DIST, SHAPES

pytestmark = pytest.mark.gpu


def _rb_max(hull):
    """the largest bounding radius of the hull table's pieces (csrc/pbre_host.hpp: build_hull)"""
    pcs = hull_pieces(hull)
    if len(pcs) == 1:
        return float(np.float32(np.linalg.norm(pcs[0], axis=1).max()))
    return max(float(np.linalg.norm(p - 0.5 * (p.min(0) + p.max(0)), axis=1).max()) for p in pcs)


def _check(eng, what, margin=None, hull=None, no_object=False, got=None):
    st = eng.get_state()
    got = eng.contact_query(margin) if got is None else got
    ph = eng.get_physics()
    r = ref.query(eng._table, st, eng.obj_off, ph, margin=margin, no_object=no_object, hull=hull)
    n = eng.num_envs
    assert got["flags"].shape == (n,) and got["dist"].shape == (n, 3) and got["nearest"].shape == (n, 2) and got["count"].shape == (n, 2) and got["tips"].shape == (n,)
    assert got["dist"].dtype == np.float32 and all(got[k].dtype == np.int32 for k in ("flags", "nearest", "count", "tips"))
    reach = None if hull is None else float(r["margin"]) + _rb_max(hull)
    out = ref.compare(r, got, GPU_DIST, what, hull_reach=reach)
    assert out.mean() <= 0.02, "%s: %d of %d envs within GPU_DIST of the margin" % (what, out.sum(), n)
    assert r["edge"].min() > 1e-4, "%s: a candidate point within 0.1 mm of the table's outline" % what
    return r, got


@pytest.fixture(scope="module")
def panda_set(panda):
    return cs.panda_states(panda)        # 40 + 40 crafted contacts, 40 jittered arms, 11 lifted objects


@pytest.fixture(scope="module")
def pushed(hip_lib, panda, panda_set):
    """Panda push, 131 envs (two full waves and a partial one) holding panda_set"""
    eng = _capi.Engine(panda["table"], task=_capi.TASK_PUSH, num_envs=len(panda_set), lib=hip_lib)
    eng.reset()
    eng.set_state(panda_set)
    yield eng
    eng.close()


def test_panda_push_box(pushed, panda, panda_set, hip_lib):
    assert len(panda_set) == 131
    r, got = _check(pushed, "panda push")
    assert set(got["flags"]) >= {0, 1, 2, 5} and {0, 1, 2, 5} <= set(r["flags"])
    assert (got["dist"][:, 1] < 0).any() and (got["dist"][:, 2] < 0).any() and (got["count"] > 1).any()
    one = _capi.Engine(panda["table"], task=_capi.TASK_PUSH, num_envs=1, lib=hip_lib)
    try:
        one.reset()
        one.set_state(panda_set[45:46])
        r1, g1 = _check(one, "one env")
        assert g1["flags"][0] == got["flags"][45] and np.array_equal(g1["dist"][0], got["dist"][45])
    finally:
        one.close()


@pytest.mark.parametrize("name", list(SHAPES))
def test_object_shapes(hip_lib, panda, name):
    shape, oh, hull = SHAPES[name]
    phys = dict(obj_shape=shape, obj_h=list(oh)) if hull is None else {}
    eng = _capi.Engine(panda["table"], task=_capi.TASK_PUSH, num_envs=16, lib=hip_lib, phys=phys)
    try:
        if hull is not None:
            eng.set_object_hull(hull)
        eng.reset()
        q, pose, ph, _ = cs.shape_set(panda["table"], scn.PANDA_HOME, name, np.random.default_rng(2))
        eph = eng.get_physics()
        assert np.allclose(list(eph.obj_h), ph.obj_h, atol=1e-6) and np.allclose(list(eph.table_c), ph.table_c) and eph.obj_shape == shape
        eng.set_state(cs.embed(eng.get_state(), q, pose, eng.obj_off))
        r, got = _check(eng, name, hull=hull)
        assert (got["flags"][:14] & 2).any() and got["flags"][14] & 1 and got["flags"][15] & 1
        assert (got["dist"][:14:3, 1] < 0).all() and (got["dist"][1:14:3, 1] < 1e-3).all() and (got["dist"][2:14:3, 1] <= 0.005 + GPU_DIST).all()
        assert abs(got["dist"][14, 0] - 0.0004) < 1e-5 and abs(got["dist"][15, 0] - 0.0004) < 1e-5
    finally:
        eng.close()


def test_margins(pushed):
    base = pushed.contact_query()
    neg = pushed.contact_query(-1.0)
    for k in base:
        assert np.array_equal(base[k], neg[k]), k
    r1, wide = _check(pushed, "margin 1 cm", margin=0.01)
    r0, zero = _check(pushed, "margin 0", margin=0.0)
    assert np.array_equal(wide["dist"], base["dist"]) and np.array_equal(zero["dist"], base["dist"])
    assert (wide["count"] >= base["count"]).all() and (wide["count"] > base["count"]).any() and (zero["count"] <= base["count"]).all()
    assert (zero["count"] < base["count"]).any() and (zero["flags"] != base["flags"]).any()


def test_no_object(hip_lib, panda, panda_set):
    eng = _capi.Engine(panda["table"], task=_capi.TASK_REACH, num_envs=40, lib=hip_lib, flags=_capi.F_NO_OBJECT)
    try:
        eng.reset()
        st = eng.get_state()
        st[:, :9] = panda_set[:40, :9]                   # the crafted robot-table contacts
        eng.set_state(st)
        r, got = _check(eng, "no object", no_object=True)
        assert not (got["flags"] & 3).any() and (got["flags"] & 4).any()
        assert (got["dist"][:, :2] == np.float32(3.0e38)).all() and (got["nearest"][:, 0] == -1).all() and not got["count"][:, 0].any() and not got["tips"].any()
    finally:
        eng.close()


def test_buffers_regrow(hip_lib, panda, panda_set):
    """out="torch" on a fresh engine (no block of the host variant yet), then the host call, then out="torch" again: the same bytes"""
    import torch
    eng = _capi.Engine(panda["table"], task=_capi.TASK_PUSH, num_envs=len(panda_set), lib=hip_lib)
    try:
        eng.reset()
        eng.set_state(panda_set)
        t1 = eng.contact_query(out="torch")
        torch.cuda.synchronize()
        t1 = {k: v.cpu().numpy() for k, v in t1.items()}
        host = eng.contact_query()
        t2 = eng.contact_query(out="torch")
        torch.cuda.synchronize()
        assert set(t1) == set(host) == set(t2) == {"flags", "dist", "nearest", "count", "tips"} and set(host["flags"]) >= {0, 1, 2, 5}
        for k, v in host.items():
            assert v.shape == t1[k].shape and v.dtype == t1[k].dtype
            assert v.tobytes() == t1[k].tobytes() and v.tobytes() == t2[k].cpu().numpy().tobytes(), k
    finally:
        eng.close()


def _other_engine(name, hip_lib, n):
    if name == "icub":
        return parity.make_icub_pair(_capi.Engine, hip_lib, n, task=0, control_arm="l", use_ik=1)[0]
    if name == "icub_float":
        import orc
        _, tbl, info = orc.icub_oracle("l", task=1, use_ik=1, control_orientation=0, floating_base=True)
        return _capi.Engine(tbl, task=1, num_envs=n, lib=hip_lib, robot=_capi.ROBOT_ICUB, **parity.icub_overrides(info, "l", 1, 0, 1))
    if name == "hands":
        return parity.make_hands_pair(_capi.Engine, hip_lib, n, "r", 0)[0]
    return parity.make_panda_arm_pair(_capi.Engine, hip_lib, n)[0]


@pytest.mark.parametrize("name", ["icub", "icub_float", "hands", "panda_arm"])
def test_other_engines(hip_lib, name):
    """iCub reach (W = 32), the floating-base iCub (object behind the 32 DoF lanes), the iCub with hands (W = 128, five fingertip slots)
    and the robot-level Panda (fingertip slots 0 / 1): 8 envs each, the object against an arm or fingertip sphere"""
    tbl0, nd, q0, spread = cs.robot_sets()[name]
    eng = _other_engine(name, hip_lib, 8)
    try:
        assert np.array_equal(np.asarray(eng._table, float), tbl0) and eng.ndof == nd
        eng.reset()
        tips = cs.tip_spheres(tbl0)
        seen = 0
        for j, k in enumerate(tips if tips else [None]):
            q, pose, _, _ = cs.shape_set(tbl0, q0, "box", np.random.default_rng(6 + j), n=8, spread=spread, tip_sphere=k, phys=eng.get_physics())
            eng.set_state(cs.embed(eng.get_state(), q, pose, eng.obj_off))
            r, got = _check(eng, "%s sphere %s" % (name, k))
            assert (got["flags"] & 2).any()
            seen |= int(np.bitwise_or.reduce(got["tips"]))
        want = 0
        for k in tips:
            want |= 1 << (int(tbl0[24 + int(tbl0[2]) * 40 + k * 8 + 6]) - 1)
        assert seen == want and (not tips or want == {"hands": 31, "panda_arm": 3}[name]), (seen, want)
    finally:
        eng.close()


def test_oracle_anchor(pushed, panda, panda_set):
    """the smallest distance of the oracle's robot-object contact list (oracle.sim_step, as test_world_check_contact reads it) is dist[1]"""
    import orc
    ora = orc.Oracle(panda["table"], task=1)
    home = np.array(scn.PANDA_HOME)
    got = pushed.contact_query()
    n = 0
    for e in range(40, 80):                              # scenarios.object_contact_states
        _, info = ora.sim_step(panda_set[e].astype(np.float64), home, np.full(9, 0.2), np.ones(9))
        ro = [info.dist[c] for c in range(info.ncontacts) if info.type[c] == 1]
        assert ro, e
        # (the oracle computes in float64 from the same float32 record: its own rounding is below 1e-12)
        assert abs(min(ro) - float(got["dist"][e, 1])) <= GPU_DIST + 1e-12, (e, min(ro), got["dist"][e, 1])
        assert got["flags"][e] & 2
        n += 1
    assert n == 40


def test_query_is_read_only_and_ordered(pushed, panda, panda_set):
    import torch
    eng = pushed
    s0 = eng.get_state()
    a = eng.contact_query()
    assert np.array_equal(eng.get_state().view(np.uint32), s0.view(np.uint32))
    b = eng.contact_query()
    for k in a:
        assert a[k].tobytes() == b[k].tobytes()
    # one output alone is the full query's, and only the outputs asked for are returned
    d = eng.contact_query(flags=False, nearest=False, count=False, tips=False)
    assert set(d) == {"dist"} and d["dist"].tobytes() == a["dist"].tobytes()
    # skipped outputs: their part of a sentinel-filled device buffer stays as it was
    dev = torch.device("cuda", 0)
    n = eng.num_envs
    buf = torch.full((9 * n,), 0x7F7F7F7F, dtype=torch.int32, device=dev)
    o = _capi.ContactOut()
    o.flags = buf.data_ptr(); o.count = buf.data_ptr() + 4 * 6 * n
    eng._chk(eng.lib.pbre_contact_query_device(eng._ctx, C.byref(o), C.c_float(-1.0), C.c_void_p(_capi.torch_stream(dev))))
    torch.cuda.synchronize()
    h = buf.cpu().numpy()
    assert np.array_equal(h[:n], a["flags"]) and np.array_equal(h[6 * n:8 * n].reshape(n, 2), a["count"])
    assert (h[n:6 * n] == 0x7F7F7F7F).all() and (h[8 * n:] == 0x7F7F7F7F).all()
    # out="torch" behind a device step on the same stream describes the state that step produced
    rng = np.random.default_rng(3)
    act = torch.as_tensor(rng.uniform(-1, 1, (n, eng.act_dim)).astype(np.float32), device=dev)
    rows = torch.empty((n, eng.obs_dim + 2), device=dev, dtype=torch.float32)
    eng.step_device(act.data_ptr(), rows.data_ptr(), _capi.torch_stream(dev))
    t = eng.contact_query(out="torch")
    assert all(v.is_cuda for v in t.values()) and t["dist"].dtype == torch.float32 and t["flags"].dtype == torch.int32
    eng.sync()
    torch.cuda.synchronize()
    assert not np.array_equal(eng.get_state(), s0), "the step changed nothing"
    got = {k: v.cpu().numpy() for k, v in t.items()}
    _check(eng, "behind step_device", got=got)
    h2 = eng.contact_query()
    for k in got:
        assert got[k].tobytes() == h2[k].tobytes()
    eng.set_state(panda_set)


def test_python_layer(hip_lib, panda, panda_set):
    import torch
    from pybullet_robot_envs import _client
    from pybullet_robot_envs.envs.panda_envs.panda_push_gym_env import pandaPushGymEnv
    from pybullet_robot_envs.envs.panda_envs.panda_env import pandaEnv
    from pybullet_robot_envs.envs.icub_envs.icub_env_with_hands import iCubHandsEnv
    from pybullet_robot_envs.model.table import sphere_links
    n = 24
    st = np.concatenate([panda_set[:8], panda_set[40:56]])
    env = pandaPushGymEnv(num_envs=n, _lib=hip_lib)
    two = pandaPushGymEnv(num_envs=n, devices=[0, 0], _lib=hip_lib)
    try:
        env.reset(); two.reset()
        env._engine.set_state(st); two._engine.set_state(st)
        info = env.contact_info()
        assert info["flags"].shape == (n,) and info["flags"].dtype == np.int32 and info["dist"].shape == (n, 3) and info["dist"].dtype == np.float32
        assert info["nearest"].shape == (n, 2) and info["count"].shape == (n, 2) and info["tips"].shape == (n,)
        r = ref.query(env._engine._table, st, 9, env._engine.get_physics())
        keep = ~ref.band(r, GPU_DIST)
        assert keep.mean() >= 0.98
        rob = env._world.check_contact(env._robot.robot_id)
        tab = env._world.check_contact(env._world.table_id)
        assert np.array_equal(((info["flags"] & 2) != 0)[keep], rob[keep]) and np.array_equal(((info["flags"] & 1) != 0)[keep], tab[keep]) and rob.any() and not rob.all()
        links, names = sphere_links(env._robot.robot_table, env._robot._model)
        assert len(links) == 13 and len(names) == 13 and all(0 <= k < 13 for k in info["nearest"].ravel())
        assert names[int(info["nearest"][0, 1])] == env._robot._model["links"][links[int(info["nearest"][0, 1])]]["name"]
        t = env.contact_tensor(0.01)
        assert all(v.is_cuda for v in t.values()) and t["flags"].shape == (n,)
        torch.cuda.synchronize()
        wide = env.contact_info(0.01)
        for k in wide:
            assert np.array_equal(t[k].cpu().numpy(), wide[k]), k
        # MultiEngine: two engines on one device, the numpy results concatenated in env order
        assert isinstance(two._engine, _capi.MultiEngine)
        both = two.contact_info()
        for k in info:
            assert np.array_equal(both[k], info[k]), k
        with pytest.raises(NotImplementedError):
            two.contact_tensor()
    finally:
        env.close(); two.close()
    for cls in (pandaEnv, iCubHandsEnv):             # the robot-level classes used alone (iCubEnv: the base class of iCubHandsEnv)
        cid = _client.connect(2, lib=hip_lib)
        try:
            out = cls(cid).contact_info()
            assert out["flags"].shape == (2,) and out["dist"].shape == (2, 3) and (out["dist"][:, 2] < 1e38).all() and (out["nearest"][:, 1] >= 0).all()
        finally:
            _client.disconnect(cid)


def test_bad_arguments(pushed):
    eng = pushed
    lib = eng.lib
    o = _capi.ContactOut()
    buf = np.full(eng.num_envs, -7, np.int32)
    o.flags = buf.ctypes.data
    assert lib.pbre_contact_query(None, C.byref(o), C.c_float(-1.0)) == -1 and "null ctx" in lib.pbre_last_error(None).decode()
    assert lib.pbre_contact_query(eng._ctx, None, C.c_float(-1.0)) == -1 and "null" in lib.pbre_last_error(eng._ctx).decode()
    assert lib.pbre_contact_query(eng._ctx, C.byref(o), C.c_float(float("nan"))) == -1 and "NaN" in lib.pbre_last_error(eng._ctx).decode()
    assert lib.pbre_contact_query_device(eng._ctx, None, C.c_float(-1.0), None) == -1
    assert lib.pbre_contact_query_device(None, C.byref(o), C.c_float(-1.0), None) == -1
    assert (buf == -7).all()
    assert lib.pbre_contact_query(eng._ctx, C.byref(_capi.ContactOut()), C.c_float(-1.0)) == 0          # nothing asked for: a no-op
    with pytest.raises(RuntimeError, match="NaN"):
        eng.contact_query(float("nan"))
    with pytest.raises(ValueError):
        eng.contact_query(out="cupy")
    assert lib.pbre_contact_query(eng._ctx, C.byref(o), C.c_float(-1.0)) == 0 and (buf != -7).all()
