"""The batched ray-cast camera on the GPU (csrc/pbre_camera.hip) against the float64 reference of tests/camera_ref.py, by the comparison
rule of that module: per image at most seg_cap differing segmentation pixels, every one of them a silhouette pixel; depth and colour on
the agreeing non-silhouette pixels within GPU_DEPTH_REL / GPU_COLOUR (test_camera_host.py: measured float32-vs-float64 figures of the
reference, times 4 / times 2)."""
import ctypes as C

import numpy as np
import pytest

import camera_ref as ref
import camera_scenes as scn
import parity
from pybullet_robot_envs import _capi
from pybullet_robot_envs.model.contacts import link_frames
from pybullet_robot_envs.model.table import HEADER, LINK_STRIDE, SPHERE_STRIDE
from pybullet_robot_envs.model.visuals import default_visuals, MAX_PRIMS
from test_camera_host import GPU_DEPTH_REL, GPU_COLOUR

pytestmark = pytest.mark.gpu


def _cams(eng, W, H, dyaw=0.0, dpitch=0.0, views=None, **kw):
    """the same camera for the engine and for the reference (which reads the matrices as the floats the struct holds)"""
    view, proj = scn.task_camera(np.asarray(eng._table[6:9]), W, H, dyaw, dpitch, **kw)
    cam = eng.make_camera(W, H, view=view, proj=proj, views=views)
    return cam, ref.Cam(np.array(cam.view[:]), np.array(cam.proj[:]), W, H, views=None if views is None else np.asarray(views, np.float32))


def _check(eng, cam, rcam, visuals, what, hull=None, no_object=False, out=None):
    st = eng.get_state()
    out = eng.render(cam) if out is None else out
    want = ref.render(eng._table, st, eng.obj_off, eng.get_physics(), rcam, visuals, no_object=no_object, hull=hull)
    H, W = rcam.height, rcam.width
    assert out["depth"].shape == (eng.num_envs, H, W) and out["seg"].dtype == np.int32 and out["rgba"].shape == (eng.num_envs, H, W, 4)
    assert np.all(out["rgba"][..., 3] == 255)
    for e in range(eng.num_envs):
        nd, off_sil, dd, dc = ref.compare([x[e] for x in want], [out["depth"][e], out["seg"][e], out["rgba"][e]])
        print("%s env %d %dx%d: seg diff %d (off silhouette %d), depth rel %.3g, colour %d" % (what, e, W, H, nd, off_sil, dd, dc))
        assert nd <= ref.seg_cap(H, W), "%s env %d: %d segmentation pixels differ" % (what, e, nd)
        assert off_sil == 0, "%s env %d: %d differing pixels are not silhouette pixels" % (what, e, off_sil)
        assert dd <= GPU_DEPTH_REL, "%s env %d: depth off by %g (relative)" % (what, e, dd)
        assert dc <= GPU_COLOUR, "%s env %d: colour off by %d" % (what, e, dc)
    return out, want


@pytest.fixture(scope="module")
def pushed(hip_lib, panda):
    """Panda push, 5 envs, after reset and 30 random steps"""
    eng = _capi.Engine(panda["table"], task=_capi.TASK_PUSH, num_envs=5, lib=hip_lib, obj_pose_rnd_std=0.05, tg_pose_rnd_std=0.2)
    eng.reset()
    rng = np.random.default_rng(0)
    for _ in range(30):
        eng.step(rng.uniform(-1, 1, (5, eng.act_dim)).astype(np.float32))
    yield eng
    eng.close()


def test_panda_push_odd_image(pushed, panda):
    eng = pushed
    q = eng.get_state()[:, :7]
    assert np.abs(q - q[0]).max() > 0.05, "the envs' poses do not differ"
    cam, rcam = _cams(eng, 37, 23, 12.0, -4.0)          # 851 pixels: three full strips and one of 83
    vis = default_visuals(panda["table"])
    eng.set_visuals(vis)
    out, want = _check(eng, cam, rcam, vis, "default visuals")
    links = set(np.unique(want[1] >> 24)) - {0, -1}
    assert len(links) >= 5 and len(set(np.unique(want[1] & 0xFFFFFF))) >= 3, "the image shows too little of the scene"
    eng.set_visuals(None)                               # no list: the collision spheres alone
    out2, _ = _check(eng, cam, rcam, None, "collision spheres")
    assert (out2["seg"] != out["seg"]).any()
    eng.set_visuals(vis)


@pytest.mark.parametrize("name", list(scn.SHAPES))
def test_object_shapes(hip_lib, panda, name):
    shape, oh, hull = scn.SHAPES[name]
    phys = dict(obj_shape=shape, obj_h=list(oh)) if hull is None else {}
    eng = _capi.Engine(panda["table"], task=_capi.TASK_PUSH, num_envs=3, lib=hip_lib, phys=phys)
    try:
        if hull is not None:
            eng.set_object_hull(hull)
        eng.reset()
        st = eng.get_state()
        o = eng.obj_off
        cam, rcam = _cams(eng, 64, 48, -8.0, 3.0)
        st[:, o:o + 7] = scn.object_before_arm(panda["table"], st, rcam.view)
        eng.set_state(st)
        vis = default_visuals(panda["table"])
        out, want = _check(eng, cam, rcam, vis, name, hull=hull)
        seg = want[1]
        touching = 0
        for e in range(3):
            obj = seg[e] == 2
            assert obj.sum() >= 6, "%s env %d: the object covers %d pixels" % (name, e, obj.sum())
            robot = (seg[e] >> 24) > 0
            grown = np.zeros_like(obj)
            grown[1:] |= obj[:-1]; grown[:-1] |= obj[1:]; grown[:, 1:] |= obj[:, :-1]; grown[:, :-1] |= obj[:, 1:]
            touching += int((grown & robot).any())
        assert touching >= 1, "%s: the object is nowhere in front of the arm" % name
    finally:
        eng.close()


def test_no_object(hip_lib, panda):
    eng = _capi.Engine(panda["table"], task=_capi.TASK_REACH, num_envs=2, lib=hip_lib, flags=_capi.F_NO_OBJECT)
    try:
        eng.reset()
        cam, rcam = _cams(eng, 64, 48)
        out, _ = _check(eng, cam, rcam, default_visuals(panda["table"]), "no object", no_object=True)
        assert not (out["seg"] == 2).any()
    finally:
        eng.close()


def test_per_env_views(hip_lib, panda):
    eng = _capi.Engine(panda["table"], task=_capi.TASK_PUSH, num_envs=4, lib=hip_lib, obj_pose_rnd_std=0.05)
    try:
        eng.reset()
        base = np.asarray(panda["table"][6:9])
        views = np.stack([scn.task_camera(base, 64, 48, dy, dp, distance=ds)[0] for dy, dp, ds in ((-30, 5, 1.3), (25, -10, 1.1), (0, 10, 1.6), (50, 0, 1.2))])
        cam, rcam = _cams(eng, 64, 48, views=views)
        out, want = _check(eng, cam, rcam, default_visuals(panda["table"]), "per-env view")
        for a in range(4):                               # the four views differ enough for a mix-up to show
            for b in range(a + 1, 4):
                assert (want[1][a] != want[1][b]).mean() > 0.05
    finally:
        eng.close()


def test_icub_reach(hip_lib):
    eng, _, _ = parity.make_icub_pair(_capi.Engine, hip_lib, 3, task=0, control_arm="l", use_ik=1, obj_std=0.05, tg_std=0.2)
    try:
        eng.reset()
        rng = np.random.default_rng(1)
        for _ in range(10):
            eng.step(rng.uniform(-1, 1, (3, eng.act_dim)).astype(np.float32))
        cam, rcam = _cams(eng, 48, 32, 10.0, 0.0)
        out, want = _check(eng, cam, rcam, default_visuals(eng._table), "iCub reach")
        assert len(set(np.unique(want[1] >> 24)) - {0, -1}) >= 5, "the iCub is hardly in the image"
    finally:
        eng.close()


def test_icub_hands_fingertips(hip_lib):
    eng, _, _ = parity.make_hands_pair(_capi.Engine, hip_lib, 2, "r", 0)
    try:
        eng.reset()
        tbl = eng._table
        vis = default_visuals(tbl)
        assert int(tbl[5]) < len(vis) <= MAX_PRIMS, len(vis)    # the largest model: 34 spheres + one capsule per link pair
        cam, rcam = _cams(eng, 48, 32)
        _check(eng, cam, rcam, vis, "iCub with hands")
        # close-ups of the controlled hand from four sides: every fingertip link shows up
        nl, ns = int(tbl[2]), int(tbl[5])
        sph = tbl[HEADER + nl * LINK_STRIDE:].reshape(ns, SPHERE_STRIDE)
        tips = sorted({int(s[0]) for s in sph if s[6] > 0})
        assert len(tips) == 5
        st = eng.get_state()
        R, p = link_frames(tbl, st[:1, :60].astype(float))
        centre = p[0, tips].mean(0)
        seen_ref, seen = set(), set()
        for yaw in (0.0, 90.0, 180.0, 270.0):
            from pybullet_robot_envs import camera as pcam
            view = pcam.view_matrix_from_yaw_pitch_roll(centre, 0.3, yaw, -30.0, 0.0, 2)
            proj = pcam.projection_matrix_fov(40.0, 48.0 / 32.0, 0.05, scn.FAR)
            cam = eng.make_camera(48, 32, view=view, proj=proj)
            rc = ref.Cam(np.array(cam.view[:]), np.array(cam.proj[:]), 48, 32)
            out, want = _check(eng, cam, rc, vis, "hand close-up yaw %g" % yaw)
            seen_ref |= set(np.unique(want[1][0] >> 24) - 1)
            seen |= set(np.unique(out["seg"][0] >> 24) - 1)
        assert set(tips) <= seen_ref and set(tips) <= seen, (tips, sorted(seen))
    finally:
        eng.close()


def test_render_is_read_only_and_ordered(pushed, panda):
    import torch
    eng = pushed
    eng.set_visuals(default_visuals(panda["table"]))
    cam, _ = _cams(eng, 37, 23)
    s0 = eng.get_state()
    a = eng.render(cam)
    assert np.array_equal(eng.get_state().view(np.uint32), s0.view(np.uint32))
    b = eng.render(cam)
    for k in ("depth", "seg", "rgba"):
        assert a[k].tobytes() == b[k].tobytes()
    # depth alone (null seg and rgba) is the full render's depth, bit for bit
    d = eng.render(cam, seg=False, rgb=False)
    assert set(d) == {"depth"} and d["depth"].tobytes() == a["depth"].tobytes()
    # step - render - step from a snapshot gives the rows of step - step
    rng = np.random.default_rng(3)
    a1, a2 = (rng.uniform(-1, 1, (5, eng.act_dim)).astype(np.float32) for _ in range(2))
    eng.step(a1)
    r1 = [x.copy() for x in eng.step(a2)]
    s_end = eng.get_state()
    eng.set_state(s0)
    eng.step(a1)
    eng.render(cam)
    r2 = eng.step(a2)
    for x, y in zip(r1, r2):
        assert np.array_equal(x.view(np.uint32), y.view(np.uint32))
    assert np.array_equal(eng.get_state().view(np.uint32), s_end.view(np.uint32))
    # out="torch" behind a device step on the same stream shows the state that step produced
    eng.set_state(s0)
    dev = torch.device("cuda", 0)
    act = torch.as_tensor(a1, device=dev)
    rows = torch.empty((5, eng.obs_dim + 2), device=dev, dtype=torch.float32)
    eng.step_device(act.data_ptr(), rows.data_ptr(), _capi.torch_stream(dev))
    t = eng.render(cam, out="torch")
    assert t["depth"].is_cuda and t["seg"].dtype == torch.int32 and t["rgba"].dtype == torch.uint8
    eng.sync()
    torch.cuda.synchronize()
    h = eng.render(cam)
    assert not np.array_equal(h["depth"], a["depth"]), "the step changed nothing the camera sees"
    for k in ("depth", "seg", "rgba"):
        assert t[k].cpu().numpy().tobytes() == h[k].tobytes()


def test_buffers_regrow(hip_lib, panda):
    """One engine renders 8 x 6, then -- with a longer visual list -- 33 x 17 (561 pixels: two full strips and one of 49), then 8 x 6 again:
    the device table, the scene buffer and the host variant's block grow in between.  Each image is, byte for byte, that of a fresh engine
    whose first render it is.  131 envs of the contact query's crafted records."""
    import contact_scenes as cs
    st = cs.panda_states(panda)
    vis = default_visuals(panda["table"])
    assert len(st) == 131 and len(vis) > 4

    def fresh(visuals):
        e = _capi.Engine(panda["table"], task=_capi.TASK_PUSH, num_envs=len(st), lib=hip_lib)
        e.reset()
        e.set_state(st)
        e.set_visuals(visuals)
        return e

    eng = fresh(vis[:4])
    try:
        steps = [(8, 6, None), (33, 17, vis), (8, 6, None)]
        got = []
        for W, H, longer in steps:
            if longer is not None:
                eng.set_visuals(longer)
            got.append(eng.render(_cams(eng, W, H)[0]))
        assert got[1]["depth"].shape == (131, 17, 33) and len(np.unique(got[1]["seg"])) >= 4
        assert got[0]["seg"].tobytes() != got[2]["seg"].tobytes(), "the longer list changed nothing the camera sees"
        for (W, H, _), visuals, g in zip(steps, (vis[:4], vis, vis), got):
            one = fresh(visuals)
            try:
                want = one.render(_cams(one, W, H)[0])
            finally:
                one.close()
            for k in ("depth", "seg", "rgba"):
                assert g[k].shape == want[k].shape and g[k].tobytes() == want[k].tobytes(), (W, H, k)
    finally:
        eng.close()


def test_task_env_render(hip_lib):
    from pybullet_robot_envs.envs.panda_envs.panda_push_gym_env import pandaPushGymEnv
    env = pandaPushGymEnv(num_envs=2)
    try:
        env.reset()
        img = env.render(width=48, height=64)
        assert img.shape == (2, 64, 48, 3) and img.dtype == np.uint8
        assert len(np.unique(img.reshape(-1, 3), axis=0)) > 1
        assert env.render("human").size == 0
        t = env.render_tensor(width=24, height=16)
        assert t["rgba"].shape == (2, 16, 24, 4) and t["depth"].is_cuda
    finally:
        env.close()
    env = pandaPushGymEnv(num_envs=1)
    try:
        env.reset()
        assert env.render(width=48, height=64).shape == (64, 48, 3)
    finally:
        env.close()


def test_icub_task_env_render(hip_lib):
    from pybullet_robot_envs.envs.icub_envs.icub_reach_gym_env import iCubReachGymEnv
    env = iCubReachGymEnv(num_envs=2)
    try:
        env.reset()
        img = env.render(width=24, height=32)
        assert img.shape == (2, 32, 24, 3) and img.dtype == np.uint8 and len(np.unique(img.reshape(-1, 3), axis=0)) > 3
        assert env.render("human").size == 0
    finally:
        env.close()


def test_bad_arguments(pushed, panda):
    eng = pushed
    lib = eng.lib
    msg = lambda: lib.pbre_last_error(eng._ctx).decode()
    cam, _ = _cams(eng, 8, 8)
    cam.proj[11] = 0.0; cam.proj[15] = 1.0                                  # orthographic
    rc = lib.pbre_camera_render(eng._ctx, C.byref(cam), None, None, None)
    assert rc == -4 and "orthographic" in msg()
    cam, _ = _cams(eng, 8, 8)
    cam.width = 0
    rc = lib.pbre_camera_render(eng._ctx, C.byref(cam), None, None, None)
    assert rc == -1 and "width" in msg()
    rc = lib.pbre_camera_render(None, C.byref(cam), None, None, None)
    assert rc == -1 and "null ctx" in lib.pbre_last_error(None).decode()
    cam, _ = _cams(eng, 40000, 40000)                                       # 5 x 1.6e9 pixels
    rc = lib.pbre_camera_render(eng._ctx, C.byref(cam), None, None, None)
    assert rc == -1 and "INT32_MAX" in msg()
    too_many = np.tile(default_visuals(panda["table"])[:1], (MAX_PRIMS + 1, 1))
    with pytest.raises(RuntimeError, match="192"):
        eng.set_visuals(too_many)
    bad = default_visuals(panda["table"])[:2].copy()
    bad[1, 0] = 99                                                          # no such link
    with pytest.raises(RuntimeError, match="link"):
        eng.set_visuals(bad)
    assert eng.render(_cams(eng, 8, 8)[0])["seg"].shape == (5, 8, 8)        # the previous list is still in place
