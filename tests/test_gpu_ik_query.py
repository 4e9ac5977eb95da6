"""The batched inverse-kinematics query on the GPU (csrc/pbre_ik.hip) against the float64 reference of tests/ik_ref.py on the same
float32 inputs (tests/ik_scenes.py): q and err within GPU_TOL (test_ik_host.py: the reference's own measured float32-vs-float64 figure
times 4), iteration counts exact wherever the reference's stopping decision is not ambiguous -- an env is ambiguous if, at some
iteration, the reference's position error lies within GPU_TOL["err_pos"] of the residual (with rot_residual > 0: or its rotation error
within GPU_TOL["err_rot"] of rot_residual); such envs are skipped, and at most 2 % of a batch may be."""
import ctypes as C

import numpy as np
import pytest

import contact_ref
import ik_ref as ref
import ik_scenes as sc
import parity
from pybullet_robot_envs import _capi
from pybullet_robot_envs.model.table import hand_pose_target
from test_ik_host import AMBIGUOUS_MAX, GPU_TOL, ambiguous_of, errors

pytestmark = pytest.mark.gpu


def _load(eng, q):
    """the joint positions q into the engine's records"""
    eng.reset()
    st = eng.get_state()
    st[:, :eng.ndof] = q
    eng.set_state(st)


def _check(eng, panda, name, from_state=False, got=None):
    """a case of ik_scenes on `eng` against its float64 reference; returns (reference, result, the envs compared)"""
    c = sc.cases(panda)[name]
    r = sc.reference(panda, name)
    if got is None:
        got = eng.ik_query(q_start=None if from_state else c["q"], **c["kw"])
    n, nd = eng.num_envs, eng.ndof
    assert got["q"].shape == (n, nd) and got["q"].dtype == np.float32 and got["err"].shape == (n, 2) and got["err"].dtype == np.float32
    assert got["iters"].shape == (n,) and got["iters"].dtype == np.int32 and np.isfinite(got["q"]).all() and np.isfinite(got["err"]).all()
    amb = ambiguous_of(r, c["kw"])
    assert amb.mean() <= AMBIGUOUS_MAX, "%s: %d of %d envs ambiguous" % (name, amb.sum(), n)
    ok = ~amb
    err = errors(r, got, ok)
    print("%s%s: %d envs, %d skipped, iterations %d..%d  " % (name, " (start values from the state)" if from_state else "", n, amb.sum(), r["iters"].min(), r["iters"].max())
          + "  ".join("%s %.3g (allowed %.3g)" % (k, v, GPU_TOL[k]) for k, v in err.items()))
    assert np.array_equal(got["iters"][ok], r["iters"][ok]), "%s: iteration counts differ in envs %s" % (name, np.nonzero(ok & (got["iters"] != r["iters"]))[0])
    for k, v in err.items():
        assert v <= GPU_TOL[k], "%s: %s off by %g (allowed %g)" % (name, k, v, GPU_TOL[k])
    _, _, moving, _, _ = ref.chain_info(c["table"], c["kw"].get("link"), c["kw"].get("dof_mask"))
    assert got["q"][:, ~moving].tobytes() == np.ascontiguousarray(c["q"][:, ~moving]).tobytes(), "%s: a DoF that does not move changed" % name
    return r, got, ok


@pytest.fixture(scope="module")
def pushed(hip_lib, panda):
    """Panda push, 131 envs (two full waves and a partial one) whose records hold the start values of the Panda cases"""
    q = sc.cases(panda)["panda_forced_6d"]["q"]
    assert len(q) == 131
    eng = _capi.Engine(panda["table"], task=_capi.TASK_PUSH, num_envs=len(q), lib=hip_lib)
    _load(eng, q)
    yield eng
    eng.close()


# ---------------------------------------------------------------------------------------------- forced iterations
@pytest.mark.parametrize("from_state", [False, True])
@pytest.mark.parametrize("name", ["panda_forced_6d", "panda_forced_3d"])
def test_forced_iterations(pushed, panda, name, from_state):
    """residual = 0, max_iters = 8: every env runs exactly 8 updates, no stopping decision is involved"""
    r, got, ok = _check(pushed, panda, name, from_state)
    assert ok.all() and (got["iters"] == 8).all()
    if name.endswith("3d"):
        assert not got["err"][:, 1].any()


# ---------------------------------------------------------------------------------------------- the stopping rule at the defaults
@pytest.mark.parametrize("name", ["panda_default_6d", "panda_default_3d", "panda_rot_residual"])
def test_stopping_rule(pushed, panda, name):
    r, got, ok = _check(pushed, panda, name)
    assert r["iters"].min() >= 2 and r["iters"].max() < 100 and len(set(r["iters"])) > 3, "the case decides nothing"
    assert (got["err"][ok, 0] < 1e-3).all()
    if name == "panda_rot_residual":
        assert (got["err"][ok, 1] < 2e-3).all() and (sc.reference(panda, name)["iters"] >= sc.reference(panda, "panda_default_6d")["iters"]).all()


def test_unreachable_targets(pushed, panda):
    """Targets 2 m away, max_iters = 20: iters == max_iters, q finite, err within tolerance of the reference's.  The comparison with the
    reference runs at damping 1: at the default 0.1 a 2 m error makes the update several radians per joint and the iteration chaotic --
    the reference's own float32 arithmetic then ends more than 0.1 m from its float64 result (test_ik_host.py:
    test_unreachable_targets_at_the_default_damping_are_chaotic), so there the checks are those that hold for any arithmetic: the cap,
    finite q, and err equal to the float64 forward kinematics' error at the q that was returned."""
    r, got, ok = _check(pushed, panda, "panda_unreachable")
    far = np.arange(131) < sc.UNREACHABLE
    assert ok.all() and (got["iters"][far] == 20).all() and (got["err"][far, 0] > 1.0).all() and (got["err"][~far, 0] < 0.1).all()
    c = sc.cases(panda)["panda_unreachable"]
    kw = dict(c["kw"], damping=None)
    d = pushed.ik_query(q_start=c["q"], **kw)
    assert (d["iters"][far] == 20).all() and np.isfinite(d["q"]).all() and np.isfinite(d["err"]).all()
    R, p = contact_ref.link_frames(c["table"], d["q"].astype(np.float64))
    ee = int(c["table"][4])
    perr = np.linalg.norm(kw["target_pos"] - p[:, ee], axis=1)
    _, ang = ref.rotvec(np.einsum("nij,nkj->nik", ref.quat_to_R(kw["target_quat"], np.float64), R[:, ee]), np.float64)
    print("default damping: err against the forward kinematics of the returned q: %.3g m, %.3g rad" % (np.abs(perr - d["err"][:, 0]).max(), np.abs(ang - d["err"][:, 1]).max()))
    assert np.abs(perr - d["err"][:, 0]).max() <= GPU_TOL["err_pos"] and np.abs(ang - d["err"][:, 1]).max() <= GPU_TOL["err_rot"]


# ---------------------------------------------------------------------------------------------- wave mates
def test_wave_mate_independence(pushed, panda, hip_lib):
    """a one-env engine holding record 45 returns rows byte-identical to row 45 of the 131-env batch (whose wave runs on while that env has
    converged, and stops while others have not)"""
    one = _capi.Engine(panda["table"], task=_capi.TASK_PUSH, num_envs=1, lib=hip_lib)
    try:
        for name in ("panda_default_6d", "panda_default_3d", "panda_forced_6d"):
            c = sc.cases(panda)[name]
            _load(one, c["q"][45:46])
            kw = {k: (v[45:46] if k in ("target_pos", "target_quat") else v) for k, v in c["kw"].items()}
            for qs in (None, c["q"]):
                big = pushed.ik_query(q_start=qs, **c["kw"])
                small = one.ik_query(q_start=None if qs is None else qs[45:46], **kw)
                for k in ("q", "err", "iters"):
                    assert small[k][0].tobytes() == big[k][45].tobytes(), (name, k)
            assert len(set(big["iters"][:64])) > 1 or name == "panda_forced_6d"
    finally:
        one.close()


# ---------------------------------------------------------------------------------------------- other engines
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
def test_other_engines(hip_lib, panda, name):
    """the pinned iCub (W = 32), the floating-base iCub (its passive virtual joints must not move, bit for bit), the iCub with hands (a
    fingertip link, position only: the chain runs through torso, arm and finger; then with dof_mask selecting the finger joints alone) and
    the robot-level Panda: 64 envs each"""
    mine = [k for k, c in sc.cases(panda).items() if c["table_name"] == name]
    assert len(mine) >= 2
    c0 = sc.cases(panda)[mine[0]]
    eng = _other_engine(name, hip_lib, len(c0["q"]))
    try:
        assert np.array_equal(np.asarray(eng._table, float), c0["table"]) and eng.num_envs == sc.N_OTHER
        _load(eng, c0["q"])
        for k in mine:
            r, got, ok = _check(eng, panda, k, from_state=k.endswith("forced_6d") or k == "hands_tip_3d")
            c = sc.cases(panda)[k]
            K, link, moving, _, _ = ref.chain_info(c["table"], c["kw"].get("link"), c["kw"].get("dof_mask"))
            if name == "icub":
                assert eng.v_off == 32
            if name == "icub_float":
                passive = np.asarray(c["table"][24:24 + 40 * K["nl"]]).reshape(-1, 40)[:, 37] != 0
                pd = K["dof"][passive]
                assert len(pd) == 6 and got["q"][:, pd].tobytes() == np.ascontiguousarray(c["q"][:, pd]).tobytes() and np.abs(c["q"][:, pd]).max() > 0
            if name == "hands":
                assert eng.v_off == 128 and link == sc.tip_link(c["table"]) and link != int(c["table"][4])
                if k == "hands_tip_3d":
                    # torso, arm and finger move (the tip's own joint turns about the driven point: its column is zero)
                    assert moving.sum() == 14 and (np.abs(got["q"] - c["q"])[:, moving].max(axis=0) > 0).sum() >= 13
                if k == "hands_tip_fingers_3d":
                    assert 2 <= moving.sum() <= 5 and (c["kw"]["dof_mask"] != 0).sum() == moving.sum()
    finally:
        eng.close()


# ---------------------------------------------------------------------------------------------- options
def test_options(pushed, panda):
    # clamp_limits: no returned q outside the limits, clamped DoFs exactly on them (and without the option some joints do leave them)
    r, got, ok = _check(pushed, panda, "panda_clamp")
    c = sc.cases(panda)["panda_clamp"]
    _, _, moving, lower, upper = ref.chain_info(c["table"])
    lo, hi = lower.astype(np.float32)[moving], upper.astype(np.float32)[moving]
    qm = got["q"][:, moving]
    on = (qm == lo) | (qm == hi)
    assert (qm >= lo).all() and (qm <= hi).all() and on.sum() > 20
    free = pushed.ik_query(q_start=c["q"], **dict(c["kw"], clamp_limits=False))
    assert ((free["q"][:, moving] < lo) | (free["q"][:, moving] > hi)).any()
    # a point of another link
    _check(pushed, panda, "panda_point")
    # an unnormalised target_quat is normalised by the kernel
    d = sc.cases(panda)["panda_default_6d"]
    scale = np.linspace(0.2, 5.0, 131).astype(np.float32)[:, None]
    got = pushed.ik_query(q_start=d["q"], **dict(d["kw"], target_quat=d["kw"]["target_quat"] * scale))
    _check(pushed, panda, "panda_default_6d", got=got)
    # max_iters = 0: the start values and their errors
    z = pushed.ik_query(max_iters=0, **d["kw"])
    r0 = ref.solve(d["table"], d["q"], max_iters=0, **d["kw"])
    e0 = errors(r0, z)
    assert z["q"].tobytes() == d["q"].tobytes() and not z["iters"].any() and e0["err_pos"] <= GPU_TOL["err_pos"] and e0["err_rot"] <= GPU_TOL["err_rot"]
    assert z["err"][:, 0].min() > 1e-3
    # link None is the table's ee_link; damping / residual / max_iters None are the engine's
    cfg = pushed.cfg
    same = pushed.ik_query(link=int(pushed._table[4]), damping=cfg.ik_damping, residual=cfg.ik_residual, max_iters=cfg.ik_max_iters, **d["kw"])
    base = pushed.ik_query(**d["kw"])
    assert all(same[k].tobytes() == base[k].tobytes() for k in base)


# ---------------------------------------------------------------------------------------------- consistency with the step
def test_consistency_with_the_step(hip_lib, panda):
    """An engine in IK mode steps; a query with the defaults, the hand pose that step commanded as the target and the joints before the
    step as start values gives the joint targets orc_ik gives on that state"""
    n = 64
    eng, ora = parity.make_pair(_capi.Engine, hip_lib, panda["table"], n, task=1, use_ik=1)
    try:
        assert eng.act_dim == 6
        eng.reset()
        rng = np.random.default_rng(12)
        for _ in range(3):
            eng.step(rng.uniform(-1, 1, (n, 6)).astype(np.float32))
        q0 = eng.get_state()[:, :9].copy()
        eng.step(rng.uniform(-1, 1, (n, 6)).astype(np.float32))
        xo = eng.x_off
        pose = eng.get_state()[:, xo + 6:xo + 12].astype(np.float64)
        tp, tq = hand_pose_target(pose, [eng.cfg.ik_link_offset[k] for k in range(3)])
        got = eng.ik_query(tp, target_quat=tq, q_start=q0)
        want = np.array([ora.ik(q0[e].astype(np.float64), pose[e, :3], pose[e, 3:])[0] for e in range(n)])
        its = np.array([ora.ik(q0[e].astype(np.float64), pose[e, :3], pose[e, 3:])[1] for e in range(n)])
        r = ref.solve(panda["table"], q0, tp.astype(np.float32), tq.astype(np.float32))
        ok = ~ambiguous_of(r, {})
        print("step consistency: orc_ik iterations %d..%d, q off by %.3g (allowed %.3g), %d skipped" % (its.min(), its.max(), np.abs(got["q"] - want)[ok].max(), GPU_TOL["q"], (~ok).sum()))
        assert (~ok).mean() <= AMBIGUOUS_MAX and np.array_equal(got["iters"][ok], its[ok]) and its.max() >= 1
        assert np.abs(got["q"] - want)[ok].max() <= GPU_TOL["q"]
    finally:
        eng.close()


# ---------------------------------------------------------------------------------------------- read-only, ordering, sentinels, buffers
def test_query_is_read_only_and_ordered(pushed, panda):
    import torch
    eng = pushed
    c = sc.cases(panda)["panda_default_6d"]
    kw = c["kw"]
    s0 = eng.get_state()
    a = eng.ik_query(**kw)
    assert np.array_equal(eng.get_state().view(np.uint32), s0.view(np.uint32))
    b = eng.ik_query(**kw)
    for k in a:
        assert a[k].tobytes() == b[k].tobytes(), k
    for k in a:                                                      # one output alone is the full query's
        d = eng.ik_query(**dict(kw, **{o: o == k for o in a}))
        assert set(d) == {k} and d[k].tobytes() == a[k].tobytes(), k
    # skipped outputs: their part of a sentinel-filled device buffer stays as it was
    dev = torch.device("cuda", 0)
    n, nd = eng.num_envs, eng.ndof
    sizes = dict(q=n * nd, err=n * 2, iters=n)
    off, total = {}, 0
    for k, v in sizes.items():
        off[k] = total; total += v
    buf = torch.full((total,), 0x7F7F7F7F, dtype=torch.int32, device=dev)
    tp, tq = torch.as_tensor(kw["target_pos"], device=dev), torch.as_tensor(kw["target_quat"], device=dev)
    o = _capi.IkQuery()
    o.link, o.damping, o.residual, o.max_iters = -1, -1.0, -1.0, -1
    o.target_pos, o.target_quat = tp.data_ptr(), tq.data_ptr()
    o.err = buf.data_ptr() + 4 * off["err"]
    eng._chk(eng.lib.pbre_ik_query_device(eng._ctx, C.byref(o), C.c_void_p(_capi.torch_stream(dev))))
    torch.cuda.synchronize()
    h = buf.cpu().numpy()
    assert h[off["err"]:off["err"] + sizes["err"]].tobytes() == a["err"].tobytes()
    assert (h[off["q"]:off["q"] + sizes["q"]] == 0x7F7F7F7F).all() and (h[off["iters"]:] == 0x7F7F7F7F).all()
    # out="torch" behind a device step on the same stream starts from the state that step produced
    rng = np.random.default_rng(3)
    act = torch.as_tensor(rng.uniform(-1, 1, (n, eng.act_dim)).astype(np.float32), device=dev)
    rows = torch.empty((n, eng.obs_dim + 2), device=dev, dtype=torch.float32)
    eng.step_device(act.data_ptr(), rows.data_ptr(), _capi.torch_stream(dev))
    t = eng.ik_query(tp, target_quat=tq, out="torch")
    assert all(v.is_cuda for v in t.values()) and t["q"].dtype == torch.float32 and t["iters"].dtype == torch.int32 and set(t) == set(a)
    eng.sync()
    torch.cuda.synchronize()
    s1 = eng.get_state()
    assert not np.array_equal(s1[:, :7], s0[:, :7]), "the step changed nothing"
    got = {k: v.cpu().numpy() for k, v in t.items()}
    h2 = eng.ik_query(**kw)
    for k in got:
        assert got[k].tobytes() == h2[k].tobytes(), k
    assert got["q"][:, 7:].tobytes() == np.ascontiguousarray(s1[:, 7:9]).tobytes() and got["q"].tobytes() != a["q"].tobytes()
    eng.set_state(s0)


def test_buffers_regrow(hip_lib, panda):
    """The host variant's block grows from call to call on one engine (iters alone, position only; then err; then everything with a start
    array and a quaternion); each result is, byte for byte, that of a fresh engine whose first call asked for it"""
    c = sc.cases(panda)["panda_default_6d"]
    engs = [_capi.Engine(panda["table"], task=_capi.TASK_PUSH, num_envs=131, lib=hip_lib) for _ in range(2)]
    try:
        for e in engs:
            _load(e, c["q"])
        grown, first = engs
        tp, tq = c["kw"]["target_pos"], c["kw"]["target_quat"]
        calls = [dict(target_pos=tp, q=False, err=False), dict(target_pos=tp, target_quat=tq, q=False, iters=False), dict(target_pos=tp, target_quat=tq, q_start=c["q"])]
        got = [grown.ik_query(**kw) for kw in calls]
        want = first.ik_query(**calls[2])
        assert [set(g) for g in got] == [{"iters"}, {"err"}, {"q", "err", "iters"}]
        assert got[1]["err"].tobytes() == want["err"].tobytes() and all(got[2][k].tobytes() == want[k].tobytes() for k in want)
        assert got[0]["iters"].tobytes() == first.ik_query(**calls[0])["iters"].tobytes() and want["iters"].max() > 1
    finally:
        for e in engs:
            e.close()


def test_bad_arguments(pushed, panda):
    """every refusal returns its code, says why, and launches nothing (the output buffer keeps its sentinel)"""
    eng = pushed
    lib = eng.lib
    n, nd = eng.num_envs, eng.ndof
    buf = np.full((n, nd), -7.0, np.float32)
    tp = np.ascontiguousarray(sc.cases(panda)["panda_default_6d"]["kw"]["target_pos"])

    def q(**kw):
        o = _capi.IkQuery()
        o.link, o.damping, o.residual, o.max_iters = -1, -1.0, -1.0, -1
        o.target_pos = tp.ctypes.data
        o.q = buf.ctypes.data
        for k, v in kw.items():
            if k == "point":
                for i in range(3):
                    o.point[i] = v[i]
            else:
                setattr(o, k, v)
        return o

    err = lambda: lib.pbre_last_error(eng._ctx).decode()
    assert lib.pbre_ik_query(None, C.byref(q())) == -1 and "null ctx" in lib.pbre_last_error(None).decode()
    assert lib.pbre_ik_query(eng._ctx, None) == -1 and "null" in err()
    assert lib.pbre_ik_query_device(eng._ctx, None, None) == -1 and lib.pbre_ik_query_device(None, C.byref(q()), None) == -1
    assert lib.pbre_ik_query(eng._ctx, C.byref(q(point=(0.0, float("nan"), 0.0)))) == -1 and "NaN" in err()
    assert lib.pbre_ik_query(eng._ctx, C.byref(q(target_pos=None))) == -1 and "target_pos" in err()
    assert lib.pbre_ik_query(eng._ctx, C.byref(q(max_iters=1001))) == -1 and "max_iters" in err()
    assert lib.pbre_ik_query(eng._ctx, C.byref(q(link=12))) == -1 and "link" in err()
    assert lib.pbre_ik_query(eng._ctx, C.byref(q(link=-2))) == -1 and lib.pbre_ik_query_device(eng._ctx, C.byref(q(link=12)), None) == -1
    assert (buf == -7).all()
    o = q()
    o.q = None
    assert lib.pbre_ik_query(eng._ctx, C.byref(o)) == 0 and (buf == -7).all()          # nothing asked for: a no-op
    with pytest.raises(RuntimeError, match="link is outside"):
        eng.ik_query(tp, link=99)
    with pytest.raises(ValueError):
        eng.ik_query(tp, out="cupy")
    with pytest.raises(ValueError):
        eng.ik_query(tp[:3])
    with pytest.raises(ValueError):
        eng.ik_query(tp, dof_mask=[1, 1])
    assert lib.pbre_ik_query(eng._ctx, C.byref(q(max_iters=1000))) == 0 and (buf != -7).all()


# ---------------------------------------------------------------------------------------------- the Python layer
def test_python_layer(hip_lib, panda):
    import torch
    from pybullet_robot_envs import _client
    from pybullet_robot_envs.envs.panda_envs.panda_push_gym_env import pandaPushGymEnv
    from pybullet_robot_envs.envs.panda_envs.panda_env import pandaEnv
    from pybullet_robot_envs.envs.icub_envs.icub_env import iCubEnv
    from pybullet_robot_envs.envs.icub_envs.icub_env_with_hands import iCubHandsEnv
    from pybullet_robot_envs.model.table import link_index
    n = 24
    c = sc.cases(panda)["panda_point"]
    keep = np.r_[0:8, 40:56]
    q0, tp, tq = c["q"][keep], c["kw"]["target_pos"][keep], c["kw"]["target_quat"][keep]
    r = ref.solve(c["table"], q0, tp, tq, link=7, point=c["kw"]["point"])
    ok = ~ambiguous_of(r, {})
    env = pandaPushGymEnv(num_envs=n, _lib=hip_lib)
    two = pandaPushGymEnv(num_envs=n, devices=[0, 0], _lib=hip_lib)
    try:
        env.reset(); two.reset()
        for e in (env, two):
            st = e._engine.get_state()
            st[:, :9] = q0
            e._engine.set_state(st)
        model = env._robot._model
        name7 = model["links"][7]["name"]
        assert isinstance(name7, str) and link_index(model, name7) == 7 and link_index(model, "panda_link5") != 7
        info = env.ik_info(tp, target_quat=tq, link=name7, point=c["kw"]["point"])
        assert set(info) == {"q", "err", "iters"} and np.array_equal(info["iters"][ok], r["iters"][ok]) and errors(r, info, ok)["q"] <= GPU_TOL["q"]
        with pytest.raises(KeyError):
            env.ik_info(tp, link="no_such_link")
        t = env.ik_tensor(torch.as_tensor(tp, device="cuda:0"), target_quat=torch.as_tensor(tq, device="cuda:0"), link=name7, point=c["kw"]["point"])
        assert all(v.is_cuda for v in t.values())
        torch.cuda.synchronize()
        for k in info:
            assert t[k].cpu().numpy().tobytes() == info[k].tobytes(), k
        # hand_pose=True: [N, 6] Euler and [N, 7] quaternion poses of the end-effector link (the Panda's ik_link_offset is zero)
        hp = sc.cases(panda)["panda_default_6d"]["kw"]
        direct = env.ik_info(hp["target_pos"][keep], target_quat=hp["target_quat"][keep])
        pose7 = np.concatenate([hp["target_pos"][keep], hp["target_quat"][keep]], axis=1)
        pose6 = np.concatenate([hp["target_pos"][keep], pandaEnv._euler_from_quat(hp["target_quat"][keep])], axis=1)
        by7, by6 = env.ik_info(pose7, hand_pose=True), env.ik_info(pose6, hand_pose=True)
        sure = ~ambiguous_of(sc.reference(panda, "panda_default_6d"), {})[keep]      # (a pose that went through Euler angles differs in the last bits)
        assert np.abs(by7["q"] - direct["q"])[sure].max() <= GPU_TOL["q"] and np.abs(by6["q"] - direct["q"])[sure].max() <= 2 * GPU_TOL["q"]
        assert np.array_equal(by7["iters"][sure], direct["iters"][sure]) and np.array_equal(by6["iters"][sure], direct["iters"][sure])
        with pytest.raises(ValueError):
            env.ik_info(pose7[:, :5], hand_pose=True)
        # MultiEngine: two engines on one device, the numpy results concatenated in env order
        assert isinstance(two._engine, _capi.MultiEngine)
        both = two.ik_info(tp, target_quat=tq, link=name7, point=c["kw"]["point"])
        for k in info:
            assert both[k].tobytes() == info[k].tobytes(), k
        with pytest.raises(NotImplementedError):
            two.ik_tensor(tp)
    finally:
        env.close(); two.close()
    # the robot-level classes used alone; the iCub classes apply ik_link_offset: exactly the target apply_action's IK is given
    for cls, nd in ((pandaEnv, 9), (iCubEnv, 20), (iCubHandsEnv, 60)):
        cid = _client.connect(2, lib=hip_lib)
        try:
            rob = cls(cid, use_IK=1)
            eng = rob._engine_or_build()
            off = np.array([eng.cfg.ik_link_offset[k] for k in range(3)])
            nd = eng.ndof
            assert (np.abs(off).max() > 0.01) == (cls is not pandaEnv)
            obs = eng.observe()[:, :6].astype(np.float64)
            pose = obs + np.array([0.01, -0.01, 0.005, 0.0, 0.0, 0.02])
            out = rob.ik_info(pose, hand_pose=True)
            a, b = hand_pose_target(pose, off)
            same = eng.ik_query(a, target_quat=b)
            assert out["q"].shape == (2, nd) and all(out[k].tobytes() == same[k].tobytes() for k in out)
            st = eng.get_state()
            want = ref.solve(eng._table, st[:, :nd], a.astype(np.float32), b.astype(np.float32), damping=eng.cfg.ik_damping, residual=eng.cfg.ik_residual, max_iters=eng.cfg.ik_max_iters)
            keep2 = ~ambiguous_of(want, {})
            print("%s: iterations %s, q off by %.3g" % (cls.__name__, want["iters"], np.abs(out["q"] - want["q"])[keep2].max(initial=0.0)))
            assert np.array_equal(out["iters"][keep2], want["iters"][keep2]) and errors(want, out, keep2)["q"] <= GPU_TOL["q"] and want["iters"].min() >= 1
        finally:
            _client.disconnect(cid)
