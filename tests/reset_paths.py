"""Every branch of the one reset() the engines share (pbre_ctx::reset in csrc/pbre_capi.hip, the sequence of csrc/pbre_reset_seq.hpp), on
the smallest batches that reach it: run by tests/test_emu_reset_paths.py on the lane emulation and by tests/test_gpu_reset_paths.py on the
device.  Everything asserted is an equality -- numeric closeness of a reset to the oracle stays with parity.check_reset and the masked
reset checks of tests/parity.py."""
import numpy as np

import parity

# kind -> envs, the envs of the partial mask
#   panda: more than one 64-env wave and no multiple of 16; 5 selected envs are padded to 16 records, from both waves and both ends
#   icub: a half-filled wave (push: the initial distances; Cartesian control: the home pose's IK targets)
#   hands / panda_arm / icub_arm: the engines whose motor records persist
SHAPES = {"panda": (70, [0, 5, 63, 64, 69]), "icub": (5, [0, 3, 4]), "hands": (3, [2]), "panda_arm": (3, [1]), "icub_arm": (3, [0, 2])}


def make(Engine, lib, kind, table=None):
    n = SHAPES[kind][0]
    if kind == "panda":
        return Engine(table, task=1, num_envs=n, lib=lib, obj_pose_rnd_std=0.05, tg_pose_rnd_std=0.2), False
    if kind == "icub":
        return parity.make_icub_pair(Engine, lib, n, task=1, obj_std=0.05, tg_std=0.2)[0], False
    if kind == "hands":
        return parity.make_hands_pair(Engine, lib, n, obj_std=0.05)[0], True
    if kind == "panda_arm":
        return parity.make_panda_arm_pair(Engine, lib, n, obj_std=0.05)[0], True
    return parity.make_icub_arm_pair(Engine, lib, n, reset=False)[1], True


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def check(Engine, lib, kind, table=None):
    eng, mrec = make(Engine, lib, kind, table)
    n, sel = SHAPES[kind]
    mask = np.zeros(n, np.uint8)
    mask[sel] = 1
    on, off = mask == 1, mask == 0
    assert on.any() and off.any()
    ep = eng.x_off + 5                                   # the record's episode counter (include/pbre.h)
    rng = np.random.default_rng(3)

    obs = eng.reset()
    assert np.array_equal(bits(obs), bits(eng.observe()))
    assert np.array_equal(eng.get_state()[:, ep], np.zeros(n))
    fresh_motors = eng.get_motor_state() if mrec else None
    keep = [eng.x_off + 12, eng.x_off + 13, eng.x_off + 15, eng.v_off + 15] if kind == "panda" else []
    if keep:                                             # per-env object mass, friction, damping and link damping: a reset keeps them
        e = np.arange(n, dtype=np.float32)
        eng.set_physics_per_env(obj_mass=0.1 + 0.001 * e, obj_mu=0.9 + 0.001 * e, obj_lin_damping=0.04 + 0.0001 * e, robot_lin_damping=0.04 + 0.0002 * e)
    for _ in range(2):
        a = rng.uniform(-1, 1, (n, eng.act_dim)).astype(np.float32)
        eng.step(a)
    if mrec:                                             # a command of its own in every record: what the unselected envs must keep
        eng.set_motors([0, 1], [0.11, -0.07], 0.3, max_force=10.0, max_vel=1.0)
    before, motors = eng.get_state(), eng.get_motor_state() if mrec else None

    obs = eng.reset(mask)
    after = eng.get_state()
    assert np.array_equal(bits(after[off]), bits(before[off])), "a partial reset touched an unselected env's record"
    assert np.array_equal(after[on][:, ep], before[on][:, ep] + 1), "the selected envs' episode counters advance by exactly one"
    assert np.array_equal(bits(after[on][:, keep]), bits(before[on][:, keep]))
    assert not np.array_equal(bits(after[on]), bits(before[on]))
    if mrec:
        m = eng.get_motor_state()
        assert np.array_equal(bits(m[off]), bits(motors[off])), "a partial reset touched an unselected env's motor record"
        assert np.array_equal(bits(m[on]), bits(fresh_motors[on])), "the selected envs' motors hold the initial positions again"
        assert not np.array_equal(bits(m[on]), bits(motors[on]))
    assert np.array_equal(bits(obs), bits(eng.observe())), "reset(mask) returns the observation of the state it leaves"

    # a mask of all ones is a full reset: it records the settled snapshot again after a scene change had made it stale
    if not mrec:                                         # (the robot-level interfaces have no episodes: no pbre_reset_snapshot)
        eng.reset_snapshot(mask)
        eng.set_physics(erp=0.25)
        try:
            eng.reset_snapshot(mask)
            raise AssertionError("pbre_reset_snapshot used a stale snapshot")
        except RuntimeError as e:
            assert "stale" in str(e)
        eng.reset(mask)                                  # (a partial reset does not renew it)
        try:
            eng.reset_snapshot(mask)
            raise AssertionError("pbre_reset_snapshot used a stale snapshot")
        except RuntimeError as e:
            assert "stale" in str(e)
    before = eng.get_state()
    obs = eng.reset(np.ones(n, np.uint8))
    after = eng.get_state()
    assert np.array_equal(after[:, ep], before[:, ep] + 1)
    assert np.array_equal(bits(after[:, keep]), bits(before[:, keep]))
    assert np.array_equal(bits(obs), bits(eng.observe()))
    if mrec:
        assert np.array_equal(bits(eng.get_motor_state()), bits(fresh_motors))
    else:
        snap = eng.reset_snapshot(mask)
        assert np.array_equal(bits(snap), bits(eng.observe()))
        assert np.array_equal(eng.get_state()[:, ep], after[:, ep] + mask)
    eng.close()
