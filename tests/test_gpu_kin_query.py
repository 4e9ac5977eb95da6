"""The batched kinematics / dynamics query on the GPU (csrc/pbre_kin.hip) against the float64 reference of tests/kin_ref.py on the same
float32 state: every output within GPU_TOL (test_kin_host.py: the reference's own measured float32-vs-float64 figure times 4), in the six
measures of kin_ref.errors -- position (m), quaternion, velocity, Jacobian, |dM_ij| / sqrt(M_ii M_jj), |dtau_j| / (1 + |tau_j|)."""
import ctypes as C

import numpy as np
import pytest

import kin_ref as ref
import kin_scenes as ks
import parity
from pybullet_robot_envs import _capi
from test_kin_host import GPU_TOL

pytestmark = pytest.mark.gpu


def _qv(eng, st=None):
    st = eng.get_state() if st is None else st
    return st[:, :eng.ndof], st[:, eng.v_off:eng.v_off + eng.ndof]


def _check(eng, what, qdd=None, got=None, tol=GPU_TOL, **kw):
    q, qd = _qv(eng)
    got = eng.kin_query(qdd=qdd, **kw) if got is None else got
    r = ref.query(eng._table, q, qd, qdd, gravity_z=eng.get_physics().gravity_z, **{k: v for k, v in kw.items() if k in ("links", "at_com", "jac_link", "jac_point", "jac_at_com")})
    n, nd = eng.num_envs, eng.ndof
    nlq = r["pose"].shape[1]
    shapes = dict(pose=(n, nlq, 7), vel=(n, nlq, 6), jac=(n, 6, nd), mass=(n, nd, nd), tau=(n, nd))
    for k, v in got.items():
        assert v.shape == shapes[k] and v.dtype == np.float32 and np.isfinite(v).all(), (what, k, v.shape)
    err = ref.errors(r, got)
    print("%s: %d envs  " % (what, n) + "  ".join("%s %.3g (allowed %.3g)" % (k, v, tol[k]) for k, v in err.items()))
    for k, v in err.items():
        assert v <= tol[k], "%s: %s off by %g (allowed %g)" % (what, k, v, tol[k])
    if "pose" in got:
        assert (got["pose"][..., 6] >= 0).all()
    if "mass" in got:
        assert np.array_equal(got["mass"], got["mass"].transpose(0, 2, 1))
    return r, got


@pytest.fixture(scope="module")
def panda_set(panda):
    return ks.panda_records(panda)        # the 131 contact-query records with joint velocities ~ N(0, 1); qdd ~ N(0, 3)


@pytest.fixture(scope="module")
def pushed(hip_lib, panda, panda_set):
    """Panda push, 131 envs (two full waves and a partial one) holding panda_set"""
    eng = _capi.Engine(panda["table"], task=_capi.TASK_PUSH, num_envs=len(panda_set[0]), lib=hip_lib)
    eng.reset()
    eng.set_state(panda_set[0])
    yield eng
    eng.close()


def test_panda_push(pushed, panda, panda_set, hip_lib):
    st, qdd = panda_set
    assert len(st) == 131
    r, got = _check(pushed, "panda push", qdd=qdd)
    assert set(got) == {"pose", "vel", "jac", "mass", "tau"} and got["pose"].shape == (131, 12, 7)
    one = _capi.Engine(panda["table"], task=_capi.TASK_PUSH, num_envs=1, lib=hip_lib)
    try:
        one.reset()
        one.set_state(st[45:46])
        r1, g1 = _check(one, "one env", qdd=qdd[45:46])
        for k in got:
            assert g1[k][0].tobytes() == got[k][45].tobytes(), k
    finally:
        one.close()


def test_buffers_regrow(hip_lib, panda, panda_set):
    """The column buffer and the host variant's block grow from call to call on one engine (tau, then the Jacobian, then M, then
    everything); each result is, byte for byte, that of a second fresh engine whose first call asked for everything."""
    st, qdd = panda_set
    engs = [_capi.Engine(panda["table"], task=_capi.TASK_PUSH, num_envs=len(st), lib=hip_lib) for _ in range(2)]
    try:
        for e in engs:
            e.reset()
            e.set_state(st)
        grown, first = engs
        only = lambda k: {x: x == k for x in ("pose", "vel", "jac", "mass", "tau")}
        got = [grown.kin_query(qdd=qdd, **only(k)) for k in ("tau", "jac", "mass")] + [grown.kin_query(qdd=qdd)]
        want = first.kin_query(qdd=qdd)
        assert [set(g) for g in got] == [{"tau"}, {"jac"}, {"mass"}, {"pose", "vel", "jac", "mass", "tau"}] and set(want) == set(got[3])
        assert np.abs(want["tau"]).max() > 1.0 and np.abs(want["jac"]).max() > 0.1
        for g in got:
            for k, v in g.items():
                assert v.shape == want[k].shape and v.tobytes() == want[k].tobytes(), k
    finally:
        for e in engs:
            e.close()


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


def _tip_link(tbl):
    """a link that carries a fingertip collision sphere (the last one), else the last link"""
    import contact_scenes as cs
    tips = cs.tip_spheres(tbl)
    return int(tbl[24 + int(tbl[2]) * 40 + tips[-1] * 8]) if tips else int(tbl[2]) - 1


@pytest.mark.parametrize("name", ["icub", "icub_float", "hands", "panda_arm"])
def test_other_engines(hip_lib, panda, name):
    """iCub reach (W = 32), the floating-base iCub (26 DoF on 32 lanes, prismatic virtual joints), the iCub with hands (W = 128, 62 links)
    and the robot-level Panda: 8 envs each; the Jacobian of the hand, then of a fingertip (or the last link)"""
    tbl0, q0, spread = ks.tables(panda)[name]
    eng = _other_engine(name, hip_lib, 8)
    try:
        assert np.array_equal(np.asarray(eng._table, float), tbl0)
        if name == "icub_float":
            assert eng.ndof == 26 and eng.v_off == 64 and (tbl0[24 + 1:24 + 40 * 29:40] == 2).sum() == 3
        if name == "hands":
            assert eng.v_off == 128 and int(tbl0[2]) == 62 and eng.ndof == 60
        eng.reset()
        q, qd, qdd = ks.robot_samples(tbl0, q0, spread)
        st = eng.get_state()
        st[:, :eng.ndof] = q; st[:, eng.v_off:eng.v_off + eng.ndof] = qd
        eng.set_state(st)
        _check(eng, name, qdd=qdd)
        tip = _tip_link(tbl0)
        _check(eng, "%s, Jacobian of link %d" % (name, tip), qdd=qdd, jac_link=tip, jac_point=(0.004, -0.003, 0.01), links=[tip], mass=False, tau=False)
    finally:
        eng.close()


def test_oracle_anchor(pushed, panda, panda_set):
    """The device's results (not the reference) against the oracle, which shares no code with either.

    mass: the device's M = M_true + E with |E_ij| <= t_M d_i d_j, d_i = sqrt(M_ii), t_M = GPU_TOL["mass"], so
    |(M Minv - I)_ik| = |sum_j E_ij Minv_jk| <= t_M d_i sum_j d_j |Minv_jk|, evaluated with the oracle's Minv (cond(M) enters through it).
    tau: forward dynamics is affine in tau with matrix Minv, and |dtau_j| <= t_tau (1 + |tau_j|), so the acceleration it returns differs from
    the qdd passed in by at most t_tau sum_j |Minv_ij| (1 + |tau_j|) (tau_j of the float64 reference).  Both get 1e-9 for the oracle's and the
    reference's own float64 error (test_kin_host.py bounds those by 1e-10 and 1e-9)."""
    import orc
    st, qdd = panda_set
    ora = orc.Oracle(panda["table"], task=1)
    ora.params.lin_damping = 0.0; ora.params.ang_damping = 0.0
    assert ora.params.gravity_z == pushed.get_physics().gravity_z
    got = pushed.kin_query(qdd=qdd)
    q, qd = (x.astype(np.float64) for x in _qv(pushed))
    r = ref.query(panda["table"], q, qd, qdd)
    K = ref.links_of(panda["table"])
    damp = np.zeros(9); damp[K["dof"][K["jtype"] != 0]] = K["damping"][K["jtype"] != 0]
    worst = np.zeros(3)
    for e in range(0, 131, 2):
        Mi = ora.minv(q[e])
        M = got["mass"][e].astype(np.float64)
        d = np.sqrt(np.diag(r["mass"][e]))
        bound = GPU_TOL["mass"] * d[:, None] * (d[:, None] * np.abs(Mi)).sum(axis=0)[None, :] + 1e-9
        res = np.abs(M @ Mi - np.eye(9))
        assert (res <= bound).all(), (e, res.max(), bound.min())
        acc = ora.forward_dynamics(q[e], qd[e], got["tau"][e].astype(np.float64) + damp * qd[e])
        bq = GPU_TOL["tau"] * (np.abs(Mi) * (1 + np.abs(r["tau"][e]))[None, :]).sum(axis=1) + 1e-9
        assert (np.abs(acc - qdd[e]) <= bq).all(), (e, np.abs(acc - qdd[e]).max(), bq)
        p = ora.fk(q[e])[1]
        assert np.abs(p - got["pose"][e, :, :3]).max() <= GPU_TOL["pos"] + 1e-12
        worst = np.maximum(worst, [(res / bound).max(), (np.abs(acc - qdd[e]) / bq).max(), np.abs(p - got["pose"][e, :, :3]).max()])
    print("oracle anchor: M Minv - I at %.2f of its bound, forward dynamics at %.2f of its bound, positions within %.3g m" % tuple(worst))


def test_options(pushed, panda_set):
    st, qdd = panda_set
    full = pushed.kin_query(qdd=qdd)
    _check(pushed, "at_com", qdd=qdd, at_com=True, jac=False, mass=False, tau=False)
    _check(pushed, "jac_point", jac_link=7, jac_point=(0.03, -0.02, 0.11), pose=False, vel=False, mass=False, tau=False)
    _check(pushed, "jac_at_com", jac_link=5, jac_at_com=True, pose=False, vel=False, mass=False, tau=False)
    # a subset of links in arbitrary order with a repeat: the rows of the all-links query
    sub = [11, 2, 7, 2, 0]
    s = pushed.kin_query(links=sub, jac=False, mass=False, tau=False)
    assert s["pose"].shape == (131, 5, 7) and s["vel"].shape == (131, 5, 6)
    for j, li in enumerate(sub):
        assert s["pose"][:, j].tobytes() == full["pose"][:, li].tobytes() and s["vel"][:, j].tobytes() == full["vel"][:, li].tobytes(), li
    # qdd None is an explicit zero array
    a = pushed.kin_query(pose=False, vel=False, jac=False, mass=False)
    b = pushed.kin_query(qdd=np.zeros((131, 9), np.float32), pose=False, vel=False, jac=False, mass=False)
    assert set(a) == {"tau"} and a["tau"].tobytes() == b["tau"].tobytes() and a["tau"].tobytes() != full["tau"].tobytes()
    # jac_link None is the table's ee_link
    assert pushed.kin_query(jac_link=int(pushed._table[4]), pose=False, vel=False, mass=False, tau=False)["jac"].tobytes() == full["jac"].tobytes()


def test_query_is_read_only_and_ordered(pushed, panda_set):
    import torch
    eng = pushed
    st, qdd = panda_set
    s0 = eng.get_state()
    a = eng.kin_query(qdd=qdd)
    assert np.array_equal(eng.get_state().view(np.uint32), s0.view(np.uint32))
    b = eng.kin_query(qdd=qdd)
    for k in a:
        assert a[k].tobytes() == b[k].tobytes(), k
    # one output alone is the full query's, and only the outputs asked for are returned
    for k in a:
        d = eng.kin_query(qdd=qdd, **{o: o == k for o in a})
        assert set(d) == {k} and d[k].tobytes() == a[k].tobytes(), k
    # skipped outputs: their part of a sentinel-filled device buffer stays as it was
    dev = torch.device("cuda", 0)
    n, nd, nl = eng.num_envs, eng.ndof, 12
    sizes = dict(pose=n * nl * 7, vel=n * nl * 6, jac=n * 6 * nd, mass=n * nd * nd, tau=n * nd)
    off, total = {}, 0
    for k, v in sizes.items():
        off[k] = total; total += v
    buf = torch.full((total,), 0x7F7F7F7F, dtype=torch.int32, device=dev)
    dd = torch.as_tensor(qdd, device=dev)
    links = np.arange(nl, dtype=np.int32)
    o = _capi.KinQuery()
    o.links, o.n_links, o.jac_link, o.qdd = links.ctypes.data, nl, -1, dd.data_ptr()
    o.jac = buf.data_ptr() + 4 * off["jac"]; o.tau = buf.data_ptr() + 4 * off["tau"]
    eng._chk(eng.lib.pbre_kin_query_device(eng._ctx, C.byref(o), C.c_void_p(_capi.torch_stream(dev))))
    torch.cuda.synchronize()
    h = buf.cpu().numpy()
    for k in sizes:
        part = h[off[k]:off[k] + sizes[k]]
        if k in ("jac", "tau"):
            assert part.tobytes() == a[k].tobytes(), k
        else:
            assert (part == 0x7F7F7F7F).all(), k
    # out="torch" behind a device step on the same stream describes the state that step produced
    rng = np.random.default_rng(3)
    act = torch.as_tensor(rng.uniform(-1, 1, (n, eng.act_dim)).astype(np.float32), device=dev)
    rows = torch.empty((n, eng.obs_dim + 2), device=dev, dtype=torch.float32)
    eng.step_device(act.data_ptr(), rows.data_ptr(), _capi.torch_stream(dev))
    t = eng.kin_query(qdd=dd, out="torch")
    assert all(v.is_cuda and v.dtype == torch.float32 for v in t.values()) and set(t) == set(a)
    eng.sync()
    torch.cuda.synchronize()
    assert not np.array_equal(eng.get_state(), s0), "the step changed nothing"
    got = {k: v.cpu().numpy() for k, v in t.items()}
    # GPU_TOL was measured on sets with qd ~ N(0, 1).  A step from the crafted penetrating contacts leaves joint velocities of several
    # rad/s, and the velocity-product terms of vel and tau grow with them: this state gets the same rule -- 4 x the reference's own
    # float32-vs-float64 figure -- measured on itself, and never less than GPU_TOL.
    q1, qd1 = _qv(eng)
    own = ref.errors(ref.query(eng._table, q1, qd1, qdd), ref.query(eng._table, q1, qd1, qdd, dtype=np.float32))
    print("after the step: largest |qd| %.3g, the reference's float32 figures %s" % (np.abs(qd1).max(), {k: "%.3g" % v for k, v in own.items()}))
    _check(eng, "behind step_device", qdd=qdd, got=got, tol={k: max(GPU_TOL[k], 4 * own[k]) for k in GPU_TOL})
    h2 = eng.kin_query(qdd=qdd)
    for k in got:
        assert got[k].tobytes() == h2[k].tobytes(), k
    eng.set_state(st)


def test_python_layer(hip_lib, panda, panda_set):
    import torch
    from pybullet_robot_envs import _client
    from pybullet_robot_envs.envs.panda_envs.panda_push_gym_env import pandaPushGymEnv
    from pybullet_robot_envs.envs.panda_envs.panda_env import pandaEnv
    from pybullet_robot_envs.envs.icub_envs.icub_env_with_hands import iCubHandsEnv
    from pybullet_robot_envs.model.table import link_index, dof_names
    n = 24
    st = np.concatenate([panda_set[0][:8], panda_set[0][40:56]])
    qdd = panda_set[1][:n]
    env = pandaPushGymEnv(num_envs=n, _lib=hip_lib)
    two = pandaPushGymEnv(num_envs=n, devices=[0, 0], _lib=hip_lib)
    try:
        env.reset(); two.reset()
        env._engine.set_state(st); two._engine.set_state(st)
        model = env._robot._model
        names = ["panda_link5", "panda_grasptarget"]
        idx = [link_index(model, x) for x in names]
        assert idx == [[l["name"] for l in model["links"]].index(x) for x in names] and link_index(model, 3) == 3 and len(dof_names(model)) == 9
        with pytest.raises(KeyError):
            link_index(model, "no_such_link")
        info = env.kinematics_info(links=names, jac_link="panda_link5", qdd=qdd)
        assert info["pose"].shape == (n, 2, 7) and info["vel"].shape == (n, 2, 6) and info["jac"].shape == (n, 6, 9) and info["mass"].shape == (n, 9, 9) and info["tau"].shape == (n, 9)
        _check(env._engine, "kinematics_info", qdd=qdd, got=info, links=idx, jac_link=idx[0])
        assert not info["jac"][:, :, 5:].any() and info["jac"][:, :, :5].any(axis=(0, 1)).all()      # panda_link5 moves with joints 1..5 only
        t = env.kinematics_tensor(links=names, jac_link="panda_link5", qdd=torch.as_tensor(qdd, device="cuda:0"))
        assert all(v.is_cuda for v in t.values()) and t["pose"].shape == (n, 2, 7)
        torch.cuda.synchronize()
        for k in info:
            assert t[k].cpu().numpy().tobytes() == info[k].tobytes(), k
        # MultiEngine: two engines on one device, the numpy results concatenated in env order
        assert isinstance(two._engine, _capi.MultiEngine)
        both = two.kinematics_info(links=names, jac_link="panda_link5", qdd=qdd)
        for k in info:
            assert both[k].tobytes() == info[k].tobytes(), k
        with pytest.raises(NotImplementedError):
            two.kinematics_tensor()
    finally:
        env.close(); two.close()
    for cls, nl, nd in ((pandaEnv, 12, 9), (iCubHandsEnv, 62, 60)):      # the robot-level classes used alone (iCubEnv: the base class of iCubHandsEnv)
        cid = _client.connect(2, lib=hip_lib)
        try:
            rob = cls(cid)
            out = rob.kinematics_info()
            assert out["pose"].shape == (2, nl, 7) and out["jac"].shape == (2, 6, nd) and out["mass"].shape == (2, nd, nd) and out["tau"].shape == (2, nd)
            _check(rob._engine_or_build(), cls.__name__, got=out)
        finally:
            _client.disconnect(cid)


def test_bad_arguments(pushed):
    eng = pushed
    lib = eng.lib
    nd = eng.ndof
    buf = np.full((eng.num_envs, nd), -7.0, np.float32)
    links = np.array([0, 3], np.int32)

    def q(**kw):
        o = _capi.KinQuery()
        o.jac_link = -1
        o.tau = buf.ctypes.data
        for k, v in kw.items():
            if k == "jac_point":
                for i in range(3):
                    o.jac_point[i] = v[i]
            else:
                setattr(o, k, v)
        return o

    err = lambda: lib.pbre_last_error(eng._ctx).decode()
    assert lib.pbre_kin_query(None, C.byref(q())) == -1 and "null ctx" in lib.pbre_last_error(None).decode()
    assert lib.pbre_kin_query(eng._ctx, None) == -1 and "null" in err()
    assert lib.pbre_kin_query_device(eng._ctx, None, None) == -1 and lib.pbre_kin_query_device(None, C.byref(q()), None) == -1
    assert lib.pbre_kin_query(eng._ctx, C.byref(q(jac_point=(0.0, float("nan"), 0.0)))) == -1 and "NaN" in err()
    pose = np.full((eng.num_envs, 2, 7), -7.0, np.float32)
    bad = np.array([0, 12], np.int32)
    assert lib.pbre_kin_query(eng._ctx, C.byref(q(links=bad.ctypes.data, n_links=2, pose=pose.ctypes.data))) == -1 and "link index" in err()
    bad[1] = -1
    assert lib.pbre_kin_query(eng._ctx, C.byref(q(links=bad.ctypes.data, n_links=2, pose=pose.ctypes.data))) == -1
    many = np.zeros(13, np.int32)
    assert lib.pbre_kin_query(eng._ctx, C.byref(q(links=many.ctypes.data, n_links=13, pose=pose.ctypes.data))) == -1 and "link count" in err()
    assert lib.pbre_kin_query(eng._ctx, C.byref(q(links=None, n_links=2, pose=pose.ctypes.data))) == -1
    assert lib.pbre_kin_query(eng._ctx, C.byref(q(jac_link=12))) == -1 and lib.pbre_kin_query(eng._ctx, C.byref(q(jac_link=-2))) == -1
    assert (buf == -7).all() and (pose == -7).all()
    assert lib.pbre_kin_query(eng._ctx, C.byref(_capi.KinQuery())) == 0          # nothing asked for: a no-op
    with pytest.raises(RuntimeError, match="link index"):
        eng.kin_query(links=[99])
    with pytest.raises(ValueError):
        eng.kin_query(out="cupy")
    with pytest.raises(ValueError):
        eng.kin_query(qdd=np.zeros((3, nd), np.float32))
    assert lib.pbre_kin_query(eng._ctx, C.byref(q(links=links.ctypes.data, n_links=2, pose=pose.ctypes.data))) == 0 and (buf != -7).all() and (pose != -7).any()
