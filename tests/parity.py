"""Shared parity checks: run an engine (HIP library on the GPU, or the host lane emulation on
CPU) against the oracle on the same seeded inputs.  Tolerances are stated per quantity."""
import numpy as np

import orc
import scenarios

# Float tolerances.  Device arithmetic is fp32, the oracle fp64.  They are stated PER QUANTITY, as absolute errors in the quantity's
# own unit after one step from identical fp32 states (calibrated on the fp32 lane emulation and the GPU: about 4x the worst
# value seen over the scenarios of tests/test_emu_parity.py / test_gpu_parity.py; `tools/parity_report.py` prints the measured ones).
# Observation entries are compared in the raw (unscaled) layout of Appendix C of SURVEY.md.
TOL = {
    "q": 1.5e-6,          # joint angles [rad] (a step moves a joint by <= 0.025 rad; measured 1.8e-7)
    "qd": 1.5e-4,         # joint velocities [rad/s] (measured 1.4e-5)
    "obj_pos": 3e-7,      # object position [m]
    "obj_quat": 8e-7,     # object quaternion components (sign-aligned)
    "obj_v": 5e-5,        # object linear velocity [m/s]
    "obj_w": 5e-6,        # object angular velocity [rad/s]
    "obs_ee_pos": 1.5e-6, # end-effector position [m]
    "obs_ee_eul": 3e-6,   # end-effector Euler angles [rad] (compared modulo 2 pi)
    "obs_ee_vel": 2e-3,   # (v - offset) / [0.04, 0.07, 0.03]: the reference's normalised EE velocity (panda_env.py:174-178); measured 2.5e-4
    "obs_q": 1.5e-6,
    "obs_obj_pos": 3e-7, "obs_obj_eul": 1e-6,
    "obs_rel_pos": 2.5e-6, "obs_rel_eul": 5e-6,   # object pose in the hand frame (measured 3.25e-6, emulation and GPU alike: one of the 70
                          # sagging arms of check_panda_force_limited, whose hand-frame Euler angles amplify an EE Euler error of 1.25e-6)
    "obs_target": 1e-7,
    "reward": 2e-6,       # |dr| / (1 + |r|)
}
# Contact-rich crafted states (penetrating robot-table / robot-object contacts, stiff motor-vs-contact conflicts, 150 PGS sweeps
# amplify fp32 rounding; the oracle's own fp32 build is ~1.5e-4 away from its fp64 build in the lumped measure there)
TOL_CONTACT = {
    "q": 1e-5, "qd": 2.5e-3, "obj_pos": 5e-7, "obj_quat": 5e-6, "obj_v": 1e-4, "obj_w": 3e-3,
    "obs_ee_pos": 2e-6, "obs_ee_eul": 4e-6, "obs_ee_vel": 5e-3, "obs_q": 1e-5, "obs_obj_pos": 5e-7, "obs_obj_eul": 1e-5,
    "obs_rel_pos": 2.5e-6, "obs_rel_eul": 1e-5, "obs_target": 1e-7, "reward": 2e-6,
}
# reset(): 201 free-running settle steps from the same initial record in engine and oracle (the arm relaxes onto its hold targets, the
# cube drops 4.5 cm onto the table and comes to rest); measured on the lane emulation / the GPU: see CALIBRATION below
TOL_RESET = {       # measured (emulation / GPU): q 9.5e-8, obj_pos 1.6e-7, obj_quat 8e-8, obj_v 6.4e-6, EE pos 1.7e-7, rel pos 4e-7
    "q": 8e-7, "qd": 1e-5, "obj_pos": 8e-7, "obj_quat": 5e-7, "obj_v": 4e-5, "obj_w": 2e-6,
    "obs_ee_pos": 1e-6, "obs_ee_eul": 1.5e-6, "obs_ee_vel": 1e-4, "obs_q": 8e-7, "obs_obj_pos": 8e-7, "obs_obj_eul": 5e-7,
    "obs_rel_pos": 2.5e-6, "obs_rel_eul": 2e-6, "obs_target": 8e-7,
}
# ... with force-limited motors (max_motor_impulse 0.02: the arm sags onto the bound and creeps; measured q 2.2e-5, EE Euler 1.8e-5)
TOL_RESET_LIMITED = dict(TOL_RESET, q=1e-4, qd=6e-4, obs_q=1e-4, obs_ee_pos=2.5e-5, obs_ee_eul=8e-5, obs_ee_vel=6e-3, obs_rel_pos=2e-5, obs_rel_eul=5e-5)
# 40 - 60 free-running steps after the reset (no re-synchronisation; random actions, no env reaches a contact): the object's bounds are
# the reset's, the arm drifts (measured q 9e-7, qd 1.3e-5, normalised EE velocity 1.6e-4)
TOL_ROLLOUT60 = dict(TOL_RESET, q=1e-5, qd=1e-4, obs_q=1e-5, obs_ee_pos=5e-6, obs_ee_eul=1e-5, obs_ee_vel=1.5e-3, obs_rel_pos=7e-6, obs_rel_eul=1e-5,
                     reward=4e-6)       # GPU, 60 steps: q 2.1e-6, qd 1.4e-5, EE pos 9.6e-7, EE Euler 2.1e-6, EE velocity 2.3e-4, reward 7e-7
TOL_REWARD = 1e-4


def rel(a, b):
    return np.abs(np.asarray(a, np.float64) - b) / (1.0 + np.abs(b))


def angdiff(a, b):
    d = np.abs(np.asarray(a, np.float64) - b) % (2 * np.pi)
    return np.minimum(d, 2 * np.pi - d)


def panda_quantities(se, so, ob, out, rw=None, task=1):
    """max abs error per quantity, Panda layout (state record: include/pbre.h; observation: SURVEY App. C)"""
    q = {}
    if len(se) == 0:
        return q
    se = np.asarray(se, np.float64)
    q["q"] = np.abs(se[:, 0:9] - so[:, 0:9]).max()
    q["qd"] = np.abs(se[:, 16:25] - so[:, 16:25]).max()
    q["obj_pos"] = np.abs(se[:, 9:12] - so[:, 9:12]).max()
    sgn = np.sign((se[:, 12:16] * so[:, 12:16]).sum(1, keepdims=True))          # q and -q are the same rotation
    q["obj_quat"] = np.abs(se[:, 12:16] * sgn - so[:, 12:16]).max()
    q["obj_v"] = np.abs(se[:, 25:28] - so[:, 25:28]).max()
    q["obj_w"] = np.abs(se[:, 28:31] - so[:, 28:31]).max()
    ob = np.asarray(ob, np.float64)
    o = out[:, :-2]
    q["obs_ee_pos"] = np.abs(ob[:, 0:3] - o[:, 0:3]).max()
    q["obs_ee_eul"] = angdiff(ob[:, 3:6], o[:, 3:6]).max()
    q["obs_ee_vel"] = np.abs(ob[:, 6:9] - o[:, 6:9]).max()
    q["obs_q"] = np.abs(ob[:, 9:18] - o[:, 9:18]).max()
    q["obs_obj_pos"] = np.abs(ob[:, 18:21] - o[:, 18:21]).max()
    q["obs_obj_eul"] = angdiff(ob[:, 21:24], o[:, 21:24]).max()
    q["obs_rel_pos"] = np.abs(ob[:, 24:27] - o[:, 24:27]).max()
    q["obs_rel_eul"] = angdiff(ob[:, 27:30], o[:, 27:30]).max()
    if ob.shape[1] > 30:
        q["obs_target"] = np.abs(ob[:, 30:33] - o[:, 30:33]).max()
    if rw is not None:
        q["reward"] = rel(rw, out[:, -2]).max()
    return q


def group_quantities(eng, se, so, ob, out, tail=0):
    """max abs error per quantity for the lane-group engines (iCub: 20 DoF, iCub with hands: 60 DoF; state record Q[W] | V[W] | X[16],
    observation = EE position, EE Euler angles, EE linear velocity (raw, m/s), controlled joints, world / task entries, and for
    the hands `tail` = 7 fingertip force / count entries)"""
    nd, vo = eng.ndof, eng.v_off
    se = np.asarray(se, np.float64); ob = np.asarray(ob, np.float64)
    o = out[:, :-2]
    q = {"q": np.abs(se[:, :nd] - so[:, :nd]).max(), "qd": np.abs(se[:, vo:vo + nd] - so[:, vo:vo + nd]).max(),
         "obj_pos": np.abs(se[:, nd:nd + 3] - so[:, nd:nd + 3]).max()}
    sgn = np.sign((se[:, nd + 3:nd + 7] * so[:, nd + 3:nd + 7]).sum(1, keepdims=True))
    q["obj_quat"] = np.abs(se[:, nd + 3:nd + 7] * sgn - so[:, nd + 3:nd + 7]).max()
    q["obj_v"] = np.abs(se[:, vo + nd:vo + nd + 3] - so[:, vo + nd:vo + nd + 3]).max()
    q["obj_w"] = np.abs(se[:, vo + nd + 3:vo + nd + 6] - so[:, vo + nd + 3:vo + nd + 6]).max()
    q["obs_ee_pos"] = np.abs(ob[:, 0:3] - o[:, 0:3]).max()
    q["obs_ee_eul"] = angdiff(ob[:, 3:6], o[:, 3:6]).max()
    q["obs_ee_vel"] = np.abs(ob[:, 6:9] - o[:, 6:9]).max()
    end = ob.shape[1] - tail
    rest_e, rest_o = ob[:, 9:end], o[:, 9:end]
    q["obs_rest"] = np.minimum(np.abs(rest_e - rest_o), angdiff(rest_e, rest_o)).max()      # joints, positions, Euler angles (mod 2 pi)
    return q


# iCub (half-wave engine), one step from identical fp32 states, JOINT control; measured on the lane emulation: q 7e-8, qd 1.2e-5,
# EE velocity 3.4e-6 m/s, everything else <= 2.2e-7
TOL_ICUB = {"q": 1e-6, "qd": 1.5e-4, "obj_pos": 3e-7, "obj_quat": 5e-7, "obj_v": 5e-5, "obj_w": 5e-6,
            "obs_ee_pos": 1e-6, "obs_ee_eul": 2e-6, "obs_ee_vel": 5e-5, "obs_rest": 2e-6}
# IK control: the damped-least-squares iteration stops at a 1 mm residual, so fp32 and fp64 may stop one iteration apart; an env
# in which that happens gets joint targets ~3e-3 rad apart (1 mm at a 0.3 m lever) and moves kp = 0.2 of that in the step.  Such
# envs are held to TOL_ICUB_IK_FLIP, counted and reported; all others to TOL_ICUB.
TOL_ICUB_IK_FLIP = {"q": 1e-3, "qd": 0.25, "obs_ee_pos": 5e-4, "obs_ee_eul": 2e-3, "obs_ee_vel": 0.1, "obs_rest": 1e-3}


def merge_worst(worst, q):
    for k, v in q.items():
        worst[k] = max(worst.get(k, 0.0), float(v))
    return worst


MEASURE = __import__("os").environ.get("PBRE_PARITY_MEASURE") == "1"     # tools/parity_measured.py: also print the measured values


def assert_within(worst, tol=None, context=""):
    """PBRE_PARITY_MEASURE=1 (tools/parity_measured.py) additionally PRINTS the measured values; it never switches an assertion off."""
    tol = TOL if tol is None else tol
    if MEASURE:
        print("MEASURED %s: %s" % (context, dict((k, float("%.3g" % v)) for k, v in worst.items() if not isinstance(v, str))))
    bad = dict((k, (v, tol[k])) for k, v in worst.items() if k in tol and not v <= tol[k])
    assert not bad, "per-quantity tolerance exceeded (measured, bound): %r %s" % (bad, context)


def set_solver_iters(eng, k, *oracles):
    """The sweep count of an engine that was created and reset at the default one, and of the oracles it is compared with: without the
    second half the oracle silently stays at 150."""
    eng.set_physics(solver_iters=int(k))
    assert eng.get_physics().solver_iters == k
    for o in oracles:
        o.params.solver_iters = int(k)


def make_pair(Engine, lib, table, n, task=1, obj_std=0.05, tg_std=0.2, **kw):
    eng = Engine(table, task=task, num_envs=n, lib=lib, obj_pose_rnd_std=obj_std, tg_pose_rnd_std=tg_std, **kw)
    ora = orc.Oracle(table, task=task)
    if "solver_iters" in (kw.get("phys") or {}):      # (an engine created at another sweep count: without this the oracle silently stays at 150)
        ora.params.solver_iters = int(kw["phys"]["solver_iters"])
    ora.task.obj_pose_rnd_std = obj_std
    ora.task.tg_pose_rnd_std = tg_std
    if kw.get("use_ik"):
        ora.set_ik_mode(True)
    ora.task.action_repeat = kw.get("action_repeat", 1)
    ora.task.max_steps = kw.get("max_steps", ora.task.max_steps)
    return eng, ora


def check_reset(eng, ora, n, tol=None):
    obs = eng.reset()
    st_o, obs_o = ora.batch_reset(n)
    st_e = eng.get_state()
    task = ora.task.task if hasattr(ora.task, "task") else 1
    out_o = np.concatenate([obs_o, np.zeros((n, 2))], 1)
    assert_within(panda_quantities(st_e, st_o, obs, out_o, task=task), TOL_RESET if tol is None else tol, "(reset: 201 free-running settle steps)")
    return st_o


def ambiguous_envs(ora, s64, a, delta=3e-6):
    """Envs whose result depends on a contact candidate lying within `delta` of the contact margin: the
    contact set is a discontinuous function of the state there, so fp32 and fp64 may legitimately pick
    different sets.  Detected by re-running the oracle with the margin nudged either way."""
    m0 = ora.params.contact_margin
    base, _ = ora.batch_step(s64, a)
    bad = np.zeros(len(s64), bool)
    for m in (m0 + delta, m0 - delta):
        ora.params.contact_margin = m
        alt, _ = ora.batch_step(s64, a)
        bad |= np.abs(alt - base).max(axis=1) > 1e-9
    ora.params.contact_margin = m0
    return bad


def check_single_steps(eng, ora, states, rng, steps=1, tol=None, skip_ambiguous=False, max_skip=0.2, report=None, ora32=None, max_outliers=0.0):
    """From identical fp32 states, one step each; re-synchronised every step.  Every quantity is held to its own bound (`tol`:
    TOL by default, TOL_CONTACT for contact-rich states).  skip_ambiguous: envs whose contact set flips under a +-3 um nudge of the contact margin are excluded (a
    discontinuity, not an error); the excluded fraction is bounded by `max_skip` and reported, like the number of envs whose
    done flag differs (a success threshold crossed by an fp32 rounding).  ora32: the oracle's own fp32 build; with skip_ambiguous,
    envs in which that build already differs from the fp64 build by more than the bounds (a friction cone that saturates or not
    depending on the last bit of the input) are excluded and counted the same way.  max_outliers: fraction of the compared env-steps
    that may exceed the bounds (bistable friction states the probes miss: the response to a 1e-7 perturbation is itself random);
    outliers are counted, reported and still held to 30 x the bounds.  Returns the report dict (also filled into `report`)."""
    st = np.asarray(states, np.float64)
    n = st.shape[0]
    worst = {}
    rep = report if report is not None else {}
    rep.update({"envs": n, "steps": steps, "skipped_ambiguous": 0, "done_flips": 0, "compared": 0})
    task = ora.task.task if hasattr(ora.task, "task") else 1
    for _ in range(steps):
        a = rng.uniform(-1, 1, (n, eng.act_dim)).astype(np.float32)
        s32 = st.astype(np.float32)
        eng.set_state(s32)
        ob, rw, dn = eng.step(a)
        se = eng.get_state()
        so, out = ora.batch_step(s32.astype(np.float64), a)
        ok = np.ones(n, bool)
        if skip_ambiguous:
            ok = ~ambiguous_envs(ora, s32.astype(np.float64), a)
            if ora32 is not None:
                # conditioning probe: the fp64 oracle itself on inputs perturbed at the fp32 rounding level (and its own fp32 build);
                # an env whose result moves by more than the bounds under such a perturbation (a friction cone that saturates or
                # not, a box that starts to rock) cannot be compared at those bounds
                tt = TOL if tol is None else tol
                prng = np.random.default_rng(12345)
                trials = [ora32.batch_step(s32, a)]
                for _ in range(4):
                    sp = s32.astype(np.float64)
                    sp[:, :31] *= 1.0 + prng.uniform(-2e-7, 2e-7, (n, 31))
                    trials.append(ora.batch_step(sp, a))
                for s_f, o_f in trials:
                    for e in range(n):
                        qf = panda_quantities(np.asarray(s_f[e:e + 1], np.float64), so[e:e + 1], np.asarray(o_f[e:e + 1, :-2], np.float64), out[e:e + 1])
                        if any(v > 0.5 * tt[k] for k, v in qf.items() if k in tt):
                            ok[e] = False
            rep["skipped_ambiguous"] += int((~ok).sum())
            assert (~ok).mean() <= max_skip, "threshold-ambiguous states: %d of %d skipped (bound %.0f %%)" % ((~ok).sum(), n, 100 * max_skip)
        # reward/done: a success threshold can flip on an fp32 rounding; such envs are counted and their reward is not compared
        flip = (dn != out[:, -1]) & ok
        rep["done_flips"] += int(flip.sum())
        assert flip.sum() <= max(1, n // 100), "done flags differ in %d of %d envs" % (flip.sum(), n)
        rep["compared"] += int(ok.sum())
        if max_outliers > 0:
            tt = TOL if tol is None else tol
            for e in np.nonzero(ok)[0]:
                qe = panda_quantities(se[e:e + 1], so[e:e + 1], ob[e:e + 1], out[e:e + 1])
                if any(v > tt[k] for k, v in qe.items() if k in tt):
                    assert all(v <= 30 * tt[k] for k, v in qe.items() if k in tt), ("outlier beyond 30 x the bounds", qe)
                    rep["outliers"] = rep.get("outliers", 0) + 1
                    ok[e] = False
        merge_worst(worst, panda_quantities(se[ok], so[ok], ob[ok], out[ok]))
        k2 = ok & ~flip
        if k2.any():
            merge_worst(worst, {"reward": rel(rw[k2], out[k2, -2]).max()})
        st = so
    rep["worst"] = worst
    assert rep.get("outliers", 0) <= max_outliers * max(1, rep["compared"]), "outliers: %d of %d compared env-steps" % (rep.get("outliers", 0), rep["compared"])
    assert_within(worst, tol, "(%d envs x %d steps, %d skipped as ambiguous, %d done flips)" % (n, steps, rep["skipped_ambiguous"], rep["done_flips"]))
    return rep


def contact_states(ora, panda, base, rng, n_table=8, n_obj=8):
    return np.concatenate([
        scenarios.table_contact_states(ora, panda["model"], panda["spheres"], base, n_table, rng),
        scenarios.object_contact_states(ora, panda["model"], panda["spheres"], base, n_obj, rng)])


def check_auto_reset(Engine, lib, table, n=12, max_steps=4, flags=0, act_dim=7, **over):
    """PBRE_F_AUTO_RESET: when an env finishes, the same step re-initialises it (snapshot reset).  The state it lands in
    must equal -- up to the settle transients the snapshot skips -- what an explicit masked pbre_reset produces for the
    same episode number, and the step returns the terminal transition's reward/done with the fresh observation."""
    F_AUTO = 2
    kw = dict(task=1, num_envs=n, lib=lib, obj_pose_rnd_std=0.05, tg_pose_rnd_std=0.2, max_steps=max_steps)
    kw.update(over)
    auto = Engine(table, flags=F_AUTO | flags, **kw)
    ref = Engine(table, flags=flags, **kw)
    o_a, o_r = auto.reset(), ref.reset()
    assert np.array_equal(o_a, o_r)
    nd, vo, xo = auto.ndof, auto.v_off, auto.x_off
    rng = np.random.default_rng(9)
    finished = np.zeros(n, bool)
    for t in range(max_steps + 3):
        a = rng.uniform(-1, 1, (n, act_dim)).astype(np.float32)
        ob_a, rw_a, dn_a = auto.step(a)
        ob_r, rw_r, dn_r = ref.step(a)
        assert np.array_equal(dn_a, dn_r) and np.allclose(rw_a, rw_r, atol=1e-5)      # the transition itself is unchanged
        d = dn_r != 0
        assert np.allclose(ob_a[~d], ob_r[~d], atol=1e-5)
        if d.any():
            ref.reset(mask=d.astype(np.uint8))                                        # explicit reset of the same envs
            sa, sr = auto.get_state(), ref.get_state()
            assert np.array_equal(sa[d, xo + 5], sr[d, xo + 5]) and (sa[d, xo + 3] == 0).all() and (sa[d, xo + 4] == 0).all()
            assert np.abs(sa[d][:, :nd + 7] - sr[d][:, :nd + 7]).max() < 5e-5         # same sampled pose, settled height
            assert np.abs(sa[d][:, vo:vo + nd + 6]).max() < 1e-6 and np.abs(sr[d][:, vo:vo + nd + 6]).max() < 2e-3
            assert np.abs(sa[d][:, xo:xo + 3] - sr[d][:, xo:xo + 3]).max() < 5e-5    # same sampled target
            assert np.abs(sa[d][:, xo + 6:xo + 14] - sr[d][:, xo + 6:xo + 14]).max() < 2e-4    # hand pose, initial distances (iCub push)
            assert np.abs(ob_a[d] - ref.observe()[d]).max() < 2e-3                    # returned obs = first obs of the new episode
            ref.set_state(sa)                                                         # continue from identical states
            finished |= d
    assert finished.all()
    ep = auto.get_state()[:, xo + 5]
    assert (ep >= 1).all()


def check_ik_mode(Engine, lib, table, task, flags=0):
    """use_IK=1 against the oracle: reset (IK solve + extra step), single steps, hand-pose clipping."""
    n = 4
    eng, ora = make_pair(Engine, lib, table, n, task=task, use_ik=1, flags=flags)
    assert eng.act_dim == 6
    obs = eng.reset()
    st_o, obs_o = ora.batch_reset(n)
    st_e = eng.get_state()
    assert np.abs(st_e[:, 38:44] - [0.2, 0, 0.8, np.pi, 0, 0]).max() < 1e-6          # _home_hand_pose (panda_env.py:85-88)
    assert rel(st_e[:, :44], st_o[:, :44]).max() < 5e-4 and rel(obs, obs_o).max() < 5e-3
    assert np.abs(obs_o[:, :3] - [0.2, 0.0, 0.8]).max() < 2e-3                           # the arm reached the home hand pose
    # single steps from identical states (IK may stop one iteration apart in fp32/fp64 -> looser tolerance than joint mode)
    rng = np.random.default_rng(4)
    st = st_o
    for k in range(6):
        a = rng.uniform(-1, 1, (n, 6)).astype(np.float32)
        s32 = st.astype(np.float32)
        eng.set_state(s32)
        ob, rw, dn = eng.step(a)
        so, out = ora.batch_step(s32.astype(np.float64), a)
        se = eng.get_state()
        assert np.abs(se[:, 38:44] - so[:, 38:44]).max() < 1e-6                          # hand pose glue: exact up to fp32
        assert rel(se[:, :35], so[:, :35]).max() < 1e-3
        assert rel(ob, out[:, :-2]).max() < 2e-2
        st = so
    # workspace clipping of the hand pose: x starts at 0.2 < 0.3 and is clipped on the first step (panda_push_gym_env.py:214-218)
    assert abs(so[0, 38] - 0.3) < 0.03
    # masked reset keeps the unmasked envs and re-solves the home pose for the masked ones
    eng.set_state(so.astype(np.float32))
    mask = np.array([1, 0, 0, 1], np.uint8)
    eng.reset(mask)
    s2 = eng.get_state()
    assert np.abs(s2[1:3, :44] - so[1:3, :44].astype(np.float32)).max() == 0
    assert np.abs(s2[[0, 3], 38:44] - [0.2, 0, 0.8, np.pi, 0, 0]).max() < 1e-6 and (s2[[0, 3], 37] == 1).all()
    return eng


# ---------------------------------------------------------------------------------------------- iCub
def icub_overrides(info, control_arm="l", use_ik=1, control_orientation=0, reward_type=1):
    """pbre_config fields that differ from pbre_default_config(PBRE_ROBOT_ICUB) (left arm, IK, position only)."""
    ov = dict(use_ik=use_ik, control_orientation=control_orientation, reward_type=reward_type,
              act_dof=list(info["controlled"]) + [-1] * 6, home=list(info["home"]) + [0.0] * (40 - len(info["home"])),
              ik_pos_scale=0.01 if control_orientation else 0.005)
    if control_arm == "r":
        ov.update(home_hand_pose=[0.3, -0.26, 0.8, 0.0, 0.0, np.pi],
                  eu_lim=[-np.pi / 2, np.pi / 2, -np.pi / 2, np.pi / 2, np.pi / 2, 1.5 * np.pi],
                  ik_link_offset=[0.064668, -0.0056, -0.022681])
    return ov


def make_icub_pair(Engine, lib, n, task=0, control_arm="l", use_ik=1, control_orientation=0, reward_type=1, obj_std=0.0, tg_std=0.0, **kw):
    from pybullet_robot_envs import _capi
    ora, tbl, info = orc.icub_oracle(control_arm, task=task, use_ik=use_ik, control_orientation=control_orientation)
    ora.task.reward_type = reward_type
    ora.task.obj_pose_rnd_std = obj_std
    ora.task.tg_pose_rnd_std = tg_std
    ov = icub_overrides(info, control_arm, use_ik, control_orientation, reward_type)
    ov.update(kw)
    ora.task.action_repeat = kw.get("action_repeat", 1)
    ora.task.max_steps = kw.get("max_steps", ora.task.max_steps)
    eng = Engine(tbl, task=task, num_envs=n, lib=lib, robot=_capi.ROBOT_ICUB, obj_pose_rnd_std=obj_std, tg_pose_rnd_std=tg_std, **ov)
    return eng, ora, info


# Contact steps of the iCub engines (hand on the table / on the object: stiff motor-vs-contact conflicts, 150 sweeps amplify fp32
# rounding as on the Panda, TOL_CONTACT), per quantity; measured values: profiles/r03_parity_report_hip.json (GPU) and the lane
# emulation, bounds ~4x the worst of the two
# (worst measured, GPU: q 9.3e-7, qd 2.2e-4, obj_pos 5.1e-6 / obj_v 1.2e-3 -- the object squeezed between hand and table --, obj_quat
# 6.3e-7, obj_w 3.0e-4, EE position 2.3e-7, EE Euler angles 7.8e-7, EE velocity 3.3e-5 m/s)
TOL_ICUB_CONTACT = {"q": 4e-6, "qd": 1e-3, "obj_pos": 2e-5, "obj_quat": 3e-6, "obj_v": 5e-3, "obj_w": 1.5e-3,
                    "obs_ee_pos": 1e-6, "obs_ee_eul": 3e-6, "obs_ee_vel": 1.5e-4, "obs_rest": 2e-5}
# after reset(): 201-202 free-running settle steps in the engine and in the oracle (no re-synchronisation in between)
# (worst measured: q 2.2e-7, qd 1.1e-5, obj_pos 1.6e-7, EE position 2.0e-7, EE Euler angles 3.8e-7, EE velocity 3.0e-6)
TOL_ICUB_RESET = {"q": 1e-6, "qd": 5e-5, "obj_pos": 6e-7, "obj_quat": 4e-7, "obj_v": 3e-5, "obj_w": 1e-6,
                  "obs_ee_pos": 8e-7, "obs_ee_eul": 1.5e-6, "obs_ee_vel": 1.5e-5, "obs_rest": 1.5e-6}


def resolve_ik_flips(ora, step_fn, flip, se, so, out, nd, tol_q, delta=1e-4):
    """IK steps in which the fp32 engine and the fp64 oracle stop the damped-least-squares iteration one iteration apart: the position
    residual of an iteration lies within rounding of the stopping threshold (ik_residual, 1e-3 m; panda_env.py:269-272).  Such a step IS
    comparable at the strict bounds -- against the oracle run with the threshold nudged by +-delta (relative), which makes it stop on
    the other side of that iteration.  step_fn(): the oracle's step of the same inputs -> (states, rows).  For the envs in `flip` whose
    joint angles then agree within tol_q the rows of `so` / `out` are replaced by the matching variant's; returns the still-unresolved mask."""
    if not flip.any():
        return flip
    unresolved = flip.copy()
    r0 = ora.task.ik_residual
    try:
        for f in (1.0 + delta, 1.0 - delta):
            ora.task.ik_residual = r0 * f
            so2, out2 = step_fn()
            hit = unresolved & (np.abs(np.asarray(se, np.float64)[:, :nd] - so2[:, :nd]).max(1) <= tol_q)
            so[hit] = so2[hit]; out[hit] = out2[hit]
            unresolved &= ~hit
    finally:
        ora.task.ik_residual = r0
    return unresolved


def compare_groups(eng, se, so, ob, out, tol, use_ik, worst, context="", tail=0, sel=None):
    """per-quantity comparison of a lane-group engine's step with the oracle's, both from the same fp32 state.  With IK control an
    env whose damped-least-squares iteration stopped one iteration apart (TOL_ICUB_IK_FLIP) is held to that looser bound and
    counted; returns the number of such envs.  sel: boolean mask of the envs to compare."""
    n = se.shape[0]
    sel = np.ones(n, bool) if sel is None else np.asarray(sel, bool)
    nd = eng.ndof
    flip = (np.abs(np.asarray(se, np.float64)[:, :nd] - so[:, :nd]).max(1) > tol["q"]) & sel if use_ik else np.zeros(n, bool)
    ok = sel & ~flip
    if ok.any():
        merge_worst(worst, group_quantities(eng, se[ok], so[ok], ob[ok], out[ok], tail=tail))
    if flip.any():
        assert_within(group_quantities(eng, se[flip], so[flip], ob[flip], out[flip], tail=tail), TOL_ICUB_IK_FLIP, "(IK flip) " + context)
    return int(flip.sum())


def check_icub(Engine, lib, task, control_arm, use_ik, control_orientation, reward_type=1, n=2, steps=4, seed=3):
    """iCub lane-group kernel (one env per 64-lane wave) against the oracle: reset, then single steps from identical states."""
    eng, ora, info = make_icub_pair(Engine, lib, n, task, control_arm, use_ik, control_orientation, reward_type, obj_std=0.05, tg_std=0.2)
    assert eng.state_floats == ora.state_floats == 80 and eng.act_dim == ora.task.n_act and eng.obs_dim == ora.obs_dim
    xo = eng.x_off
    obs = eng.reset()
    st_o, obs_o = ora.batch_reset(n)
    st_e = eng.get_state()
    row_o = np.concatenate([obs_o, np.zeros((n, 2))], 1)
    assert_within(group_quantities(eng, st_e, st_o, obs, row_o), TOL_ICUB_RESET, "(iCub reset, task %d arm %s ik %d)" % (task, control_arm, use_ik))
    assert np.abs(st_e[:, xo:] - st_o[:, xo:]).max() < 2e-3
    rng = np.random.default_rng(seed)
    st = st_o
    worst, flips, unresolved = {}, 0, 0
    for k in range(steps):
        a = rng.uniform(-1, 1, (n, eng.act_dim)).astype(np.float32)
        s32 = st.astype(np.float32)
        eng.set_state(s32)
        ob, rw, dn = eng.step(a)
        so, out = ora.batch_step(s32.astype(np.float64), a)
        se = eng.get_state()
        assert np.abs(se[:, xo + 6:xo + 12] - so[:, xo + 6:xo + 12]).max() < 1e-6      # commanded hand pose
        nd = eng.ndof
        flip = np.abs(se[:, :nd] - so[:, :nd]).max(1) > TOL_ICUB["q"] if use_ik else np.zeros(n, bool)
        flips += int(flip.sum())
        so_next = so.copy()
        # an IK iteration whose residual lies within rounding of the stopping threshold: compared, at the STRICT bounds, with the oracle run
        # with the threshold nudged to the other side of that iteration; what is still unresolved is counted and capped below
        left = resolve_ik_flips(ora, lambda: ora.batch_step(s32.astype(np.float64), a), flip, se, so, out, nd, TOL_ICUB["q"])
        unresolved += int(left.sum())
        if (~left).any():
            merge_worst(worst, group_quantities(eng, se[~left], so[~left], ob[~left], out[~left]))
        if left.any():
            assert_within(group_quantities(eng, se[left], so[left], ob[left], out[left]), TOL_ICUB_IK_FLIP, "(IK stopped apart and not resolved by a threshold nudge, step %d)" % k)
        assert np.abs(rw - out[:, -2]).max() < 1e-3 * max(1.0, np.abs(out[:, -2]).max())
        assert (dn == out[:, -1]).all()
        st = so_next
    assert flips <= max(1, n * steps // 10), "IK iteration-count flips in %d of %d env-steps" % (flips, n * steps)
    assert unresolved <= max(0, n * steps // 100), "IK flips a +-1e-4 nudge of the stopping threshold does not explain: %d of %d env-steps" % (unresolved, n * steps)
    assert_within(worst, TOL_ICUB, "(iCub, %d envs x %d steps, %d IK flips, %d unresolved)" % (n, steps, flips, unresolved))
    return eng


def check_icub_force_limited(Engine, lib, n=1, steps=3, imp=0.004):
    """iCub with a motor impulse bound that binds (pbre_physics.max_motor_impulse; ~1 N m against gravity torques of a few N m):
    the clamp-free motor rows of the half-wave solver must hand over to the clamping rows (pbre_core.hpp FREE_ROWS)."""
    eng, ora, info = make_icub_pair(Engine, lib, n, task=1, control_arm="l", use_ik=0, phys={"max_motor_impulse": imp})
    ref, _, _ = make_icub_pair(Engine, lib, n, task=1, control_arm="l", use_ik=0)
    ora.params.max_motor_impulse = imp
    xo = eng.x_off
    eng.reset(); ref.reset()
    st, _ = ora.batch_reset(n)
    assert rel(eng.get_state()[:, :xo], st[:, :xo]).max() < 2e-3
    assert rel(ref.get_state()[:, :xo], eng.get_state()[:, :xo]).max() > 1e-3, "the bound does not bind: nothing tested"
    rng = np.random.default_rng(4)
    for k in range(steps):
        a = rng.uniform(-1, 1, (n, eng.act_dim)).astype(np.float32)
        s32 = st.astype(np.float32)
        eng.set_state(s32)
        ob, rw, dn = eng.step(a)
        st, out = ora.batch_step(s32.astype(np.float64), a)
        assert rel(eng.get_state()[:, :xo], st[:, :xo]).max() < 2e-3, (k, rel(eng.get_state()[:, :xo], st[:, :xo]).max())
        assert rel(ob, out[:, :-2]).max() < 2e-2
    return eng


def check_obj_split(Engine, lib, n=4, steps=3, exact=True):
    """Lane-group engines solve the object's rows per env in a kernel of their own (pbre_objstep.hpp) and use the result in every env
    whose robot does not touch the object.  Against the same engine with PBRE_OBJ_SPLIT=0 (all rows in one solve): the robot's state
    is bit-identical either way, the object agrees to rounding, an env WITH a robot-object contact is bit-identical as a whole even
    when it shares a wavefront with one without (env 1 of each pair has the object pushed into the hand), and all of it matches
    the oracle's coupled solve.
    exact=False: the two engines run different kernels (device, lane-per-env pipeline on: PBRE_OBJ_SPLIT=0 also selects the lane-group
    kernel for every step, the default engine the quad pipeline + the lane-group kernel for the envs with robot contacts), so the
    bitwise assertions become rounding-level ones; both still have to match the oracle."""
    import os
    os.environ["PBRE_OBJ_SPLIT"] = "0"
    try:
        one, ora, info = make_icub_pair(Engine, lib, n, task=1, control_arm="l", use_ik=1, obj_std=0.05, tg_std=0.2)
    finally:
        del os.environ["PBRE_OBJ_SPLIT"]
    two, _, _ = make_icub_pair(Engine, lib, n, task=1, control_arm="l", use_ik=1, obj_std=0.05, tg_std=0.2)
    xo, lc = one.x_off, 20
    one.reset(); two.reset()
    s1, s2 = one.get_state(), two.get_state()
    if exact:
        assert np.array_equal(s1[:, :lc], s2[:, :lc]) and np.array_equal(s1[:, 32:32 + lc], s2[:, 32:32 + lc])
        assert np.abs(s1 - s2).max() < 1e-5
    else:       # (the pipeline also runs the settle steps of a full reset)
        assert rel(s1[:, :xo], s2[:, :xo]).max() < 2e-4
    st, _ = ora.batch_reset(n)
    hand = two.observe()[:, :3]
    st = st.copy()
    st[1::2, lc:lc + 3] = hand[1::2] + np.array([0.0, 0.0, -0.045])      # object right under the hand of every second env
    rng = np.random.default_rng(8)
    touched = 0.0
    worst_c, worst_f, worst1, flips = {}, {}, {}, 0
    for k in range(steps):
        a = rng.uniform(-1, 1, (n, one.act_dim)).astype(np.float32)
        s32 = st.astype(np.float32)
        one.set_state(s32); two.set_state(s32)
        o1, r1, d1 = one.step(a)
        o2, r2, d2 = two.step(a)
        st, out = ora.batch_step(s32.astype(np.float64), a)
        e1, e2 = one.get_state(), two.get_state()
        if exact:
            assert np.array_equal(e1[:, :lc], e2[:, :lc]) and np.array_equal(e1[:, 32:32 + lc], e2[:, 32:32 + lc]), k
            assert np.array_equal(e1[1::2], e2[1::2]) and np.array_equal(o1[1::2], o2[1::2]), k
            assert np.abs(e1 - e2).max() < 1e-5 and np.abs(o1 - o2).max() < 1e-4
        else:
            assert rel(e1[:, :xo], e2[:, :xo]).max() < 2e-4 and rel(o1, o2).max() < 2e-3, (k, rel(e1[:, :xo], e2[:, :xo]).max(), rel(o1, o2).max())
            flips += compare_groups(one, e1, st, o1, out, TOL_ICUB_CONTACT, True, worst1, "obj_split, one solve, step %d" % k)
        # against the oracle, per quantity: the envs with the object under the hand (odd: coupled solve) to the contact bounds, the
        # others to the plain single-step bounds
        odd = (np.arange(n) % 2) == 1
        flips += compare_groups(two, e2, st, o2, out, TOL_ICUB_CONTACT, True, worst_c, "obj_split, coupled envs, step %d" % k, sel=odd)
        flips += compare_groups(two, e2, st, o2, out, TOL_ICUB, True, worst_f, "obj_split, contact-free envs, step %d" % k, sel=~odd)
        touched = max(touched, np.abs(st[1::2, 32 + lc:32 + lc + 2]).max())
    assert touched > 1e-3, "the hand never pushed the object: the coupled case was not exercised"
    assert flips <= max(2, n * steps // 5), "IK iteration-count flips in %d env-steps" % flips
    assert_within(worst_c, TOL_ICUB_CONTACT, "(iCub robot-object contact, coupled solve; %d IK flips)" % flips)
    assert_within(worst_f, TOL_ICUB, "(iCub, contact-free neighbours of the coupled envs)")
    if worst1:
        assert_within(worst1, TOL_ICUB_CONTACT, "(iCub, PBRE_OBJ_SPLIT=0 engine)")
    return two


def check_icub_table_contact(Engine, lib, n=2, steps=45):
    """iCub, Cartesian control, the hand driven down onto the table: robot-table contact rows (lane-per-env pipeline: rows of kw_quad /
    Lane::step).  Every step starts from the oracle's state (fp32), so the comparison is per step; the commanded hand pose ends up
    below the hand itself, which the table stopped."""
    eng, ora, info = make_icub_pair(Engine, lib, n, task=1, control_arm="l", use_ik=1, control_orientation=0, obj_std=0.05, tg_std=0.2)
    eng.reset()
    st, _ = ora.batch_reset(n)
    xo = eng.x_off
    rng = np.random.default_rng(11)
    worst, flips = {}, 0
    for k in range(steps):
        a = rng.uniform(-0.3, 0.3, (n, 3)).astype(np.float32)
        a[:, 2] = -1.0
        s32 = st.astype(np.float32)
        eng.set_state(s32)
        ob, rw, dn = eng.step(a)
        st, out = ora.batch_step(s32.astype(np.float64), a)
        se = eng.get_state()
        flips += compare_groups(eng, se, st, ob, out, TOL_ICUB_CONTACT, True, worst, "table contact, step %d" % k)
    hand_z, cmd_z = out[:, 2], st[:, xo + 8]
    assert (hand_z - cmd_z > 0.01).all(), (hand_z, cmd_z)         # the table holds the hand above the commanded pose
    assert flips <= max(2, n * steps // 10), "IK iteration-count flips in %d of %d env-steps" % (flips, n * steps)
    assert_within(worst, TOL_ICUB_CONTACT, "(iCub hand pressed on the table, %d envs x %d steps, %d IK flips)" % (n, steps, flips))
    worst["ik_flips"] = flips
    return worst


def check_icub_lane_ab(Engine, lib, monkeypatch, variant, n=64, steps=12, tol=2e-3):
    """iCub: a lane-per-env variant (PBRE_ICUB_LANE=variant) against the lane-group kernel (=0) on the same seeded free-running batch
    (joint and Cartesian control, auto-reset on and off).  The kernels round differently (M^-1 by Gauss-Jordan across a quad / by the
    sweep operator / one row per lane), so agreement is at rounding level over a short horizon; returns the worst relative difference."""
    worst = 0.0
    for task, arm, use_ik, ori in [(0, "l", 1, 0), (1, "r", 1, 1), (1, "l", 0, 0)]:
        for auto in (0, 2):
            res = []
            for lane in (0, variant):
                monkeypatch.setenv("PBRE_ICUB_LANE", str(lane))
                eng, ora, info = make_icub_pair(Engine, lib, n, task=task, control_arm=arm, use_ik=use_ik, control_orientation=ori,
                                                obj_std=0.05, tg_std=0.1, max_steps=5, flags=auto)
                eng.reset()
                rng = np.random.default_rng(3)
                rows = []
                for k in range(steps):
                    ob, rw, dn = eng.step(rng.uniform(-1, 1, (n, eng.act_dim)).astype(np.float32))
                    rows.append(np.concatenate([ob, rw[:, None], dn[:, None]], 1))
                res.append((np.array(rows), eng.get_state(), eng.kernel_info()))
            (a, sa, ia), (b, sb, ib) = res
            assert ia[2] == 0 and ib[2] == 1, (ia, ib)
            d = max(float(rel(a, b).max()), float(rel(sa, sb).max()))
            assert d < tol, (task, arm, use_ik, ori, auto, d)
            worst = max(worst, d)
    monkeypatch.delenv("PBRE_ICUB_LANE")
    return worst


def check_icub_push_policy(Engine, lib, monkeypatch, n=2048, steps=300):
    """iCub push under a scripted policy that drives the hand at the object (Cartesian control): a large share of the envs is in
    robot-object contact, i.e. in the pipeline's coupled solve (kw_quad_rc).  Contact dynamics amplify rounding differences, so the
    comparison with the lane-group kernel is at the level of the batch: finite states, unit quaternions, the same number of finished
    episodes and the same mean reward to a few per cent."""
    stats = []
    for lane in (1, 0):
        monkeypatch.setenv("PBRE_ICUB_LANE", str(lane))
        eng, ora, info = make_icub_pair(Engine, lib, n, task=1, control_arm="l", use_ik=1, control_orientation=0, obj_std=0.05, tg_std=0.2,
                                        max_steps=150, flags=2)
        obs = eng.reset()
        rng = np.random.default_rng(7)
        o0 = 9 + (eng.obs_dim - 9 - 15)
        dones = 0.0; rew = 0.0; cmax = 0
        for k in range(steps):
            d = obs[:, o0:o0 + 3] - obs[:, 0:3]; d[:, 2] += 0.02
            a = np.clip(d / (np.linalg.norm(d, axis=1, keepdims=True) + 1e-6) + 0.3 * rng.uniform(-1, 1, (n, 3)), -1, 1).astype(np.float32)
            obs, rw, dn = eng.step(a)
            dones += float(dn.sum()); rew += float(rw.mean())
            if k % 25 == 24: cmax = max(cmax, eng.kernel_info()[5])
        st = eng.get_state(); nd = eng.ndof
        assert np.isfinite(st).all() and np.isfinite(obs).all()
        assert np.abs(np.linalg.norm(st[:, nd + 3:nd + 7], axis=1) - 1).max() < 1e-5
        stats.append((dones, rew / steps, cmax))
    monkeypatch.delenv("PBRE_ICUB_LANE")
    (d1, r1, c1), (d0, r0, c0) = stats
    assert c1 > n // 20, "the policy did not bring the hands to the objects: %d envs in robot-object contact at most" % c1
    assert abs(d1 - d0) <= 0.03 * max(d0, 1.0) + 3 and abs(r1 - r0) <= 0.05 * abs(r0) + 1e-3, stats
    return stats


def check_icub_full_model(Engine, lib, n=2, steps=3):
    """The unpruned iCub (32 DoF with the legs: one env per 64-lane group, Shape64) against the engine's default 20-DoF model
    (Shape32): the legs cannot change any output (tests/test_golden_icub.py::test_pruned_legs_are_exact shows it for the oracle), so
    observations, rewards and terminations of the two engines agree to fp32 rounding through reset and closed-loop steps."""
    from pybullet_robot_envs import _capi
    from pybullet_robot_envs.model.table import icub_table
    tblf, _, infof = icub_table("l", full=True)
    ov = icub_overrides(infof, "l", 1, 0, 1)
    full = Engine(tblf, task=1, num_envs=n, lib=lib, robot=_capi.ROBOT_ICUB, obj_pose_rnd_std=0.05, tg_pose_rnd_std=0.2, **ov)
    small, ora, info = make_icub_pair(Engine, lib, n, task=1, control_arm="l", use_ik=1, obj_std=0.05, tg_std=0.2)
    assert full.state_floats == 144 and small.state_floats == 80 and full.obs_dim == small.obs_dim
    of, os_ = full.reset(), small.reset()
    assert rel(of, os_).max() < 2e-3, rel(of, os_).max()
    rng = np.random.default_rng(12)
    for k in range(steps):
        a = rng.uniform(-1, 1, (n, small.act_dim)).astype(np.float32)
        (of, rf, df), (os_, rs, ds) = full.step(a), small.step(a)
        assert rel(of, os_).max() < 5e-3, (k, rel(of, os_).max())
        assert np.abs(rf - rs).max() < 1e-3 * max(1.0, np.abs(rs).max()) and (df == ds).all()
    return full


def check_wave_neighbour_independence(Engine, lib, steps=3):
    """Two envs share a wavefront on the device (half-wave shape).  The solver's wave-level shortcuts -- clamp-free motor rows with a
    fall-back to clamping rows, object rows taken from the per-env object kernel, skipped limit rows -- must not leak between them:
    env 0 steps bit-identically whether env 1 is an ordinary state or one whose joint velocities (50 rad/s) push the wave onto the
    clamping fall-back, and also when env 1 has the object pushed into its hand (coupled solve for that group)."""
    eng, ora, info = make_icub_pair(Engine, lib, 2, task=1, control_arm="l", use_ik=0, obj_std=0.05, tg_std=0.2)
    xo, lc = eng.x_off, 20
    eng.reset()
    base = eng.get_state()
    hand = eng.observe()[:, :3]
    fast = base.copy(); fast[1, 32:32 + lc] = 50.0
    push = base.copy(); push[1, lc:lc + 3] = hand[1] + np.array([0.0, 0.0, -0.045])
    rng = np.random.default_rng(21)
    acts = rng.uniform(-1, 1, (steps, 2, eng.act_dim)).astype(np.float32)
    runs = []
    for st in (base, fast, push):
        eng.set_state(st)
        outs = []
        for k in range(steps):
            o, r, d = eng.step(acts[k])
            outs.append((o[0].copy(), float(r[0]), float(d[0]), eng.get_state()[0].copy()))
        runs.append(outs)
    for other in runs[1:]:
        for (o0, r0, d0, s0), (o1, r1, d1, s1) in zip(runs[0], other):
            assert np.array_equal(o0, o1) and r0 == r1 and d0 == d1 and np.array_equal(s0, s1)
    assert not np.array_equal(runs[0][0][3], base[0])
    return eng


def check_action_repeat(Engine, lib, table, use_ik=0, flags=0):
    """action_repeat = 3 (apply_action loop with the reference's compounding in-place action scaling, break on termination,
    counter per iteration) against the oracle: free-running, so that envs leave the loop in different iterations."""
    n = 6
    eng, ora = make_pair(Engine, lib, table, n, task=1, use_ik=use_ik, action_repeat=3, max_steps=7, flags=flags)
    eng.reset()
    st_o, _ = ora.batch_reset(n)
    st_o[:, 32:35] = [0.6, 0.3, 0.65]                    # far target: the step budget, not success, ends the episode
    st_o = st_o.astype(np.float32).astype(np.float64)
    eng.set_state(st_o.astype(np.float32))
    rng = np.random.default_rng(11)
    cnts = []
    for k in range(5):
        a = rng.uniform(-1, 1, (n, eng.act_dim)).astype(np.float32)
        ob, rw, dn = eng.step(a)
        st_o, out = ora.batch_step(st_o, a)
        se = eng.get_state()
        assert np.array_equal(se[:, 35], st_o[:, 35]) and (dn == out[:, -1]).all()       # counters: 3, 6, 8, 8, 8 (budget 7)
        assert rel(se[:, :35], st_o[:, :35]).max() < 2e-3 and rel(ob, out[:, :-2]).max() < 2e-2
        assert (se[:, 46] == 0).all()                                                     # the loop-exit flag never outlives a step
        cnts.append(int(se[0, 35]))
    assert cnts == [3, 6, 8, 8, 8], cnts


# ---------------------------------------------------------------------------------------------- iCub with hands
def hands_overrides(info, control_arm="l", use_ik=0):
    """pbre_config fields that differ from pbre_default_config(PBRE_ROBOT_ICUB_HANDS) (left arm, joint control)."""
    n = len(info["controlled"])
    ov = dict(use_ik=use_ik, act_dof=list(info["controlled"]) + [-1] * (64 - n), home=list(info["home"]),
              num_controlled_joints=n, num_joints_ctrl=n)
    if control_arm == "r":
        ov.update(home_hand_pose=[0.2, -0.3, 0.8, 0.0, 0.0, np.pi / 2],
                  eu_lim=[-np.pi / 2, np.pi / 2, -np.pi / 2, np.pi / 2, 0.0, np.pi],
                  ik_link_offset=[-0.011682, 0.051682, -0.000577])
    return ov


def make_hands_pair(Engine, lib, n, control_arm="r", use_ik=0, obj_std=0.0, **kw):
    from pybullet_robot_envs import _capi
    ora, tbl, info = orc.hands_oracle(control_arm, use_ik=use_ik)
    ora.task.obj_pose_rnd_std = obj_std
    ov = hands_overrides(info, control_arm, use_ik)
    ov.update(kw)
    eng = Engine(tbl, task=0, num_envs=n, lib=lib, robot=_capi.ROBOT_ICUB_HANDS, obj_pose_rnd_std=obj_std, **ov)
    ph = eng.get_physics()                     # scene of the demo (table at x = 1, brick-sized object): same numbers on both sides
    for f in ("table_c", "table_h", "obj_h", "obj_inertia"):
        for k in range(3):
            getattr(ora.params, f)[k] = getattr(ph, f)[k]
    ora.params.obj_mass = ph.obj_mass
    ora.params.implicit_joint_damping = ph.implicit_joint_damping
    return eng, ora, info


# iCub with hands (one env per wavefront), one step from identical fp32 states; measured on the lane emulation: joint control q 6e-8,
# qd 5e-6; IK control q 6e-7, qd 1.4e-4, EE velocity 9e-6 m/s
# hands, fingertip / palm contacts on the object and after reset (202 free-running settle steps of 60 joints): per quantity
# (worst measured, contacts: q 1.4e-7, qd 3.0e-5, obj_quat 1.0e-6, obj_v 1.5e-5, obj_w 4.9e-4, observation tail entries 2.0e-6; reset: q 1.0e-5
# and qd 1.0e-4 with IK control -- 202 settle steps towards an IK target that differs by the IK's own stopping tolerance --, else <= 4e-7)
TOL_HANDS_CONTACT = {"q": 6e-7, "qd": 1.5e-4, "obj_pos": 2e-7, "obj_quat": 4e-6, "obj_v": 6e-5, "obj_w": 2e-3,
                     "obs_ee_pos": 4e-7, "obs_ee_eul": 1.2e-6, "obs_ee_vel": 3e-5, "obs_rest": 8e-6}
TOL_HANDS_RESET = {"q": 4e-5, "qd": 4e-4, "obj_pos": 6e-7, "obj_quat": 4e-7, "obj_v": 3e-5, "obj_w": 1e-6,
                   "obs_ee_pos": 2e-7, "obs_ee_eul": 1.5e-6, "obs_ee_vel": 6e-6, "obs_rest": 4e-5}
TOL_HANDS = {"q": 5e-6, "qd": 1e-3, "obj_pos": 3e-7, "obj_quat": 8e-7, "obj_v": 5e-5, "obj_w": 5e-6,
             "obs_ee_pos": 1e-6, "obs_ee_eul": 3e-6, "obs_ee_vel": 1e-4, "obs_rest": 5e-6}


def check_hands(Engine, lib, control_arm="r", use_ik=0, n=1, steps=3, seed=7):
    """iCub with hands (60 DoF, one env per 128-virtual-lane group) against the oracle: reset, commands, single steps from identical
    states; finger commands through pbre_set_motors."""
    from pybullet_robot_envs.model.table import GRASP_POS
    eng, ora, info = make_hands_pair(Engine, lib, n, control_arm, use_ik)
    assert eng.state_floats == ora.state_floats == 272 and eng.act_dim == ora.task.n_act and eng.obs_dim == ora.obs_dim
    xo = eng.x_off
    obs = eng.reset()
    st_o, mrec, obs_o = ora.hands_reset(n)
    st_e = eng.get_state()
    row_o = np.concatenate([obs_o, np.zeros((n, 2))], 1)
    assert_within(group_quantities(eng, st_e, st_o, obs, row_o, tail=7), TOL_HANDS_RESET, "(hands reset, arm %s ik %d)" % (control_arm, use_ik))
    rng = np.random.default_rng(seed)
    home = np.asarray(info["home"])[info["controlled"]]
    st = st_o
    worst, flips = {}, 0
    for k in range(steps):
        if k == 1:      # pre_grasp / grasp of the controlled hand (icub_env_with_hands.py:181-234)
            pos = list(GRASP_POS)
            eng.set_motors(info["fingers"], pos, 0.1, 10.0)
            mrec = ora.hands_set_motors(mrec, info["fingers"], pos, 0.1, 10.0)
        if use_ik:
            a = np.tile(np.array([0.3, -0.1 if control_arm == "r" else 0.1, 0.8, 0.0, 0.0, 1.0], np.float32), (n, 1))
            a[:, :3] += rng.uniform(-0.02, 0.02, (n, 3)).astype(np.float32)
        else:
            a = (home[None, :] + rng.uniform(-0.2, 0.2, (n, len(home)))).astype(np.float32)
        s32 = st.astype(np.float32)
        eng.set_state(s32)
        ob, rw, dn = eng.step(a)
        so, mrec, out = ora.hands_step(s32.astype(np.float64), mrec, a)
        se = eng.get_state()
        nd = eng.ndof
        flip = np.abs(se[:, :nd] - so[:, :nd]).max(1) > TOL_HANDS["q"] if use_ik else np.zeros(n, bool)     # see TOL_ICUB_IK_FLIP
        flips += int(flip.sum())
        if (~flip).any():
            merge_worst(worst, group_quantities(eng, se[~flip], so[~flip], ob[~flip], out[~flip], tail=7))
        if flip.any():
            assert_within(group_quantities(eng, se[flip], so[flip], ob[flip], out[flip], tail=7), TOL_ICUB_IK_FLIP, "(IK flip, step %d)" % k)
        assert np.abs(ob[:, -7:] - out[:, -9:-2]).max() < 1e-6                       # no fingertip contact in this scenario: forces / counts are 0
        assert np.abs(rw - out[:, -2]).max() < 1e-3 * max(1.0, np.abs(out[:, -2]).max())
        assert (dn == out[:, -1]).all() and not dn.any()
        st = so
    assert flips <= max(1, n * steps // 10), "IK iteration-count flips in %d of %d env-steps" % (flips, n * steps)
    assert_within(worst, TOL_HANDS, "(hands, %d envs x %d steps, %d IK flips)" % (n, steps, flips))
    return eng, ora, info, st, mrec


def check_hands_force_limited_reset(Engine, lib, n=1, imp=0.004):
    """pbre_physics.max_motor_impulse small enough to bind on the hands model: the clamp-free motor rows are attempted (no motor
    has a reduced force), leave the bound and hand over to the clamping rows; reset (202 settle steps) against the oracle."""
    eng, ora, info = make_hands_pair(Engine, lib, n, "r", 0, phys={"max_motor_impulse": imp})
    ref, _, _ = make_hands_pair(Engine, lib, n, "r", 0)
    ora.params.max_motor_impulse = imp
    xo = eng.x_off
    eng.reset(); ref.reset()
    st_o, mrec, obs_o = ora.hands_reset(n)
    assert rel(eng.get_state()[:, :xo], st_o[:, :xo]).max() < 3e-3, rel(eng.get_state()[:, :xo], st_o[:, :xo]).max()
    assert rel(ref.get_state()[:, :xo], eng.get_state()[:, :xo]).max() > 1e-3, "the bound does not bind: nothing tested"
    return eng


def check_hands_contacts(Engine, lib, control_arm="r", steps=3):
    """Fingertip contacts: the object is placed under the index and middle fingertips of the closing hand (1.5 mm penetration);
    states, fingertip forces / counts (observation tail) against the oracle."""
    from pybullet_robot_envs.model.table import icub_hands_model, hand_joint_names
    eng, ora, info, st, mrec = check_hands(Engine, lib, control_arm, 0, n=1, steps=2)
    nd, xo = 60, eng.x_off
    m = icub_hands_model()
    by_joint = {l.get("joint_name"): i for i, l in enumerate(m["links"])}
    R, p = ora.fk(st[0, :nd])
    jn = hand_joint_names(control_arm)
    tips = [by_joint[jn[k]] for k in (3, 11)]                    # index, middle
    c = [p[i] + R[i] @ np.array([0.0168, 0.0, 0.0]) for i in tips]
    ph = eng.get_physics()
    s = st.copy()
    mid = 0.5 * (c[0] + c[1])
    s[0, nd:nd + 3] = [mid[0], mid[1], min(c[0][2], c[1][2]) - 0.0075 - ph.obj_h[2] + 0.0015]
    s[0, nd + 3:nd + 7] = [0, 0, 0, 1]
    s[0, eng.v_off + nd:eng.v_off + nd + 6] = 0
    a = np.asarray(info["home"], np.float32)[info["controlled"]][None, :]
    seen = 0.0
    worst = {}
    for k in range(steps):
        s32 = s.astype(np.float32)
        eng.set_state(s32)
        ob, rw, dn = eng.step(a)
        so, mrec, out = ora.hands_step(s32.astype(np.float64), mrec, a)
        se = eng.get_state()
        merge_worst(worst, group_quantities(eng, se, so, ob, out, tail=7))
        tail_e, tail_o = ob[0, -7:], out[0, -9:-2]
        assert np.array_equal(tail_e[5:], tail_o[5:]), (tail_e, tail_o)                 # tips in contact, contact points
        assert np.abs(tail_e[:5] - tail_o[:5]).max() < 2e-2 * (1.0 + np.abs(tail_o[:5]).max()), (tail_e, tail_o)
        seen = max(seen, tail_o[5])
        s = so
    assert seen >= 1, "no fingertip contact was exercised"
    assert_within(worst, TOL_HANDS_CONTACT, "(hands, index + middle fingertip on the object, arm %s)" % control_arm)
    return eng


def check_panda_force_limited(Engine, lib, table, n=6, imp=0.02):
    """Panda with a motor impulse bound that binds (pbre_physics.max_motor_impulse 0.02 ~ 5 N m against gravity torques of tens of
    N m): the lane-per-env kernel's clamp-free motor rows must detect it (sum |delta| over the solve exceeds the bound) and start
    over with the clamping rows; reset and single steps against the oracle with the same bound."""
    eng, ora = make_pair(Engine, lib, table, n, phys={"max_motor_impulse": imp})
    ref, _ = make_pair(Engine, lib, table, n)
    ora.params.max_motor_impulse = imp
    st = check_reset(eng, ora, n, TOL_RESET_LIMITED)
    ref.reset()
    assert rel(ref.get_state()[:, :9], eng.get_state()[:, :9]).max() > 1e-3, "the bound does not bind: nothing tested"
    check_single_steps(eng, ora, st, np.random.default_rng(13), steps=3)
    # and one step from the state the unlimited arm settles in (no contact, no joint at a limit: the simple-env kernel's own case)
    s0 = ref.get_state()
    a = np.random.default_rng(14).uniform(-1, 1, (n, eng.act_dim)).astype(np.float32)
    eng.set_state(s0)
    ob, rw, dn = eng.step(a)
    so, out = ora.batch_step(s0.astype(np.float64), a)
    assert_within(panda_quantities(eng.get_state(), so, ob, out, rw), TOL, "(force-limited motors, one step from the unlimited arm's settled state)")
    ref.set_state(s0)
    ref.step(a)
    assert rel(ref.get_state()[:, :9], eng.get_state()[:, :9]).max() > 1e-4      # the bound changed that step too
    return eng


def check_implicit_damping(Engine, lib, table, n=6):
    """pbre_physics.implicit_joint_damping on the Panda: the lane-per-env kernels do not implement it (the engine falls back to
    the lane-group kernel at creation, refuses to switch later); results against the oracle with the same option."""
    eng, ora = make_pair(Engine, lib, table, n, phys={"implicit_joint_damping": 1})
    ora.params.implicit_joint_damping = 1
    st = check_reset(eng, ora, n)
    check_single_steps(eng, ora, st, np.random.default_rng(11), steps=3)
    assert eng.kernel_info()[3] == 0, "the lane-per-env fast path must be off with implicit joint damping"
    e2, o2 = make_pair(Engine, lib, table, n)
    e2.reset()
    assert rel(e2.get_state(), eng.get_state()).max() > 1e-6          # the option does change the dynamics
    import pytest
    with pytest.raises(RuntimeError, match="explicit joint damping"):
        e2.set_physics(implicit_joint_damping=1)


# ---------------------------------------------------------------------------------------------- full-episode rollouts, glue-only
def check_panda_full_episode(Engine, lib, table, n=8, steps=1000, seed=3):
    """A whole 1000-step Panda-push episode, free running (no re-synchronisation) with i.i.d. U(-1,1) actions, against the
    oracle.  Stated drift bounds at EVERY checkpoint, per env:
      * envs whose robot never came within the contact margin of the table or the object: joint angles 2e-5 rad, joint velocities
        5e-4 rad/s (the position-controlled arm is contractive), object 1e-6 m / 2e-6 (quaternion);
      * envs that did have a robot contact (a finger pressed on the table, a joint driven into a contact): one contact step has a
        single-step error of up to TOL_CONTACT (150 sweeps of a stiff motor-vs-contact conflict in fp32: 2.5e-3 rad/s), which the
        position loop then contracts: joint angles 2e-3 rad, joint velocities 5e-2 rad/s; once the object was touched the closed loop
        is contact-chaotic (a 1e-7 difference decides whether a candidate is inside the margin): object within 2 cm.
    Which envs had a contact is read off the ORACLE's states with the engine's own detection rule (model/contacts.py); the counts are
    reported."""
    from pybullet_robot_envs.model import contacts
    eng, ora = make_pair(Engine, lib, table, n, max_steps=steps + 10)
    st = check_reset(eng, ora, n)
    st[:, 32:35] = [0.6, 0.3, 0.65]                      # far target: no success latch, the episode runs its full length
    st = st.astype(np.float32).astype(np.float64)
    eng.set_state(st.astype(np.float32))
    obj0 = st[:, 9:12].copy()
    rng = np.random.default_rng(seed)
    phys = eng.get_physics()
    worst = {"q": 0.0, "qd": 0.0, "q_contact": 0.0, "qd_contact": 0.0, "obj_untouched": 0.0, "obj_touched": 0.0}
    had_contact = np.zeros(n, bool)
    for k in range(steps):
        had_contact |= (contacts.contact_flags(table, st, 9, phys) & (contacts.ROBOT_TABLE | contacts.ROBOT_OBJECT)) != 0
        a = rng.uniform(-1, 1, (n, 7)).astype(np.float32)
        ob, rw, dn = eng.step(a)
        st, out = ora.batch_step(st, a)
        if k % 25 == 24 or k == steps - 1:
            se = eng.get_state().astype(np.float64)
            touched = np.abs(st[:, 9:12] - obj0).max(1) > 1e-5
            eq, eqd = np.abs(se[:, :9] - st[:, :9]).max(1), np.abs(se[:, 16:25] - st[:, 16:25]).max(1)
            free = ~had_contact
            if free.any():
                worst["q"] = max(worst["q"], eq[free].max()); worst["qd"] = max(worst["qd"], eqd[free].max())
            if had_contact.any():
                worst["q_contact"] = max(worst["q_contact"], eq[had_contact].max()); worst["qd_contact"] = max(worst["qd_contact"], eqd[had_contact].max())
            d = np.abs(se[:, 9:16] - st[:, 9:16]).max(1)
            if (~touched).any():
                worst["obj_untouched"] = max(worst["obj_untouched"], d[~touched].max())
            if touched.any():
                worst["obj_touched"] = max(worst["obj_touched"], d[touched].max())
            assert not dn.any() and not out[:, -1].any()
    worst["touched_envs"] = int(touched.sum())
    worst["robot_contact_envs"] = int(had_contact.sum())
    assert worst["q"] < 2e-5 and worst["qd"] < 5e-4 and worst["obj_untouched"] < 2e-6 and worst["obj_touched"] < 2e-2, worst
    assert worst["q_contact"] < 2e-3 and worst["qd_contact"] < 5e-2, worst
    assert (eng.get_state()[:, 35] == steps).all() and (st[:, 35] == steps).all()
    return worst


def check_icub_full_episode(Engine, lib, n=2, steps=2000, seed=5):
    """A whole 2000-step iCub-push episode in joint control (10 torso + arm joints, U(-1,1) actions), free running against the
    oracle; drift bounds at every 50th step: joint angles 2e-5 rad, joint velocities 5e-4 rad/s, object pose 2e-6.  (With IK
    control the restated closed loop is chaotic after ~250 steps -- tests/test_golden_icub.py: check_config1 -- so the
    full-length drift bound is stated for joint control.)"""
    eng, ora, info = make_icub_pair(Engine, lib, n, task=1, control_arm="l", use_ik=0, obj_std=0.05, tg_std=0.2, max_steps=steps + 10)
    eng.reset()
    st, _ = ora.batch_reset(n)
    xo, nd, vo = eng.x_off, eng.ndof, eng.v_off
    st[:, xo:xo + 3] = [0.9, 0.5, 0.65]
    st = st.astype(np.float32).astype(np.float64)
    eng.set_state(st.astype(np.float32))
    rng = np.random.default_rng(seed)
    worst = {"q": 0.0, "qd": 0.0, "obj": 0.0, "q_contact_envs": 0.0}
    obj0 = st[:, nd:nd + 3].copy()
    for k in range(steps):
        a = rng.uniform(-1, 1, (n, eng.act_dim)).astype(np.float32)
        ob, rw, dn = eng.step(a)
        st, out = ora.batch_step(st, a)
        if k % 50 == 49:
            se = eng.get_state().astype(np.float64)
            # an env whose arm has pushed the object (or the table) has been through contact-chaotic steps: loose bound, reported
            touched = np.abs(st[:, nd:nd + 3] - obj0).max(1) > 1e-5
            dq = np.abs(se[:, :nd] - st[:, :nd]).max(1)
            if (~touched).any():
                f = ~touched
                worst["q"] = max(worst["q"], dq[f].max())
                worst["qd"] = max(worst["qd"], np.abs(se[f, vo:vo + nd] - st[f, vo:vo + nd]).max())
                worst["obj"] = max(worst["obj"], np.abs(se[f, nd:nd + 7] - st[f, nd:nd + 7]).max())
            if touched.any():
                worst["q_contact_envs"] = max(worst["q_contact_envs"], dq[touched].max())
            assert not dn.any()
    worst["contact_envs"] = int(touched.sum())
    assert worst["q"] < 2e-5 and worst["qd"] < 5e-4 and worst["obj"] < 2e-6 and worst["q_contact_envs"] < 5e-2, worst
    assert touched.sum() <= n // 2, worst
    return worst


def check_device_glue(Engine, lib, table):
    """The observation glue ALONE on the device (<= 1e-6 relative in the fp32 path): pbre_set_state from the states of
    the reference-captured trajectories (tests/golden/panda_glue.npz, `*_pre_state[k+1]` = the state after step k), pbre_observe,
    against the raw observation the reference's own get_extended_observation produced for that state (`*_raw_obs[k]`).
    Bounds: |d| / (1 + |x|) <= 1e-6 on every entry except the three normalised end-effector velocity entries, which the
    reference divides by 0.04 / 0.07 / 0.03 (panda_env.py:174-178): those are held to 3e-6 m/s before the division (the fp32 rounding of
    the nine joint velocities of the input state alone is ~1e-6 m/s at the hand)."""
    import os
    G = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "panda_glue.npz"))
    worst = {"rel": 0.0, "ee_vel_mps": 0.0}
    for tag, task, ik in (("pushA", 1, 0), ("pushB", 1, 0), ("reachC", 0, 0), ("goalD", 2, 0), ("ikF", 1, 1)):
        pre, raw = G[tag + "_pre_state"], G[tag + "_raw_obs"]
        n = len(pre) - 1
        eng = Engine(table, task=task, num_envs=n, lib=lib, use_ik=ik)
        eng.set_state(pre[1:].astype(np.float32))
        ob = eng.observe().astype(np.float64)
        ref = raw[:-1]
        e = np.abs(ob - ref) / (1.0 + np.abs(ref))
        ang = [3, 4, 5, 21, 22, 23, 27, 28, 29]
        e[:, ang] = angdiff(ob[:, ang], ref[:, ang]) / (1.0 + np.abs(ref[:, ang]))
        vel = np.abs(ob[:, 6:9] - ref[:, 6:9]) * np.array([0.04, 0.07, 0.03])
        e[:, 6:9] = 0.0
        worst["rel"] = max(worst["rel"], e.max())
        worst["ee_vel_mps"] = max(worst["ee_vel_mps"], vel.max())
        eng.close()
    assert worst["rel"] <= 1e-6 and worst["ee_vel_mps"] <= 3e-6, worst
    return worst


# ---------------------------------------------------------------------------------------------- Panda, robot-level interface
def make_panda_arm_pair(Engine, lib, n, use_ik=0, control_orientation=1, obj_std=0.0, **kw):
    """pandaEnv used alone (pbre_config.robot_level = 1; reference panda_env.py:195-365): engine + oracle, same scene."""
    from pybullet_robot_envs import _capi
    ora, tbl = orc.panda_arm_oracle(use_ik, control_orientation)
    ora.task.obj_pose_rnd_std = obj_std
    eng = Engine(tbl, task=0, num_envs=n, lib=lib, robot=_capi.ROBOT_PANDA_ARM, use_ik=use_ik, control_orientation=control_orientation,
                 obj_pose_rnd_std=obj_std, **kw)
    ph = eng.get_physics()
    for f in ("table_c", "table_h", "obj_h", "obj_inertia"):
        for k in range(3):
            getattr(ora.params, f)[k] = getattr(ph, f)[k]
    ora.params.obj_mass = ph.obj_mass
    return eng, ora


TOL_PANDA_ARM = {"q": 2e-6, "qd": 3e-4, "obj_pos": 3e-7, "obj_quat": 8e-7, "obj_v": 5e-5, "obj_w": 5e-6,
                 "obs_ee_pos": 2e-6, "obs_ee_eul": 4e-6, "obs_ee_vel": 4e-3, "obs_rest": 3e-6}


def check_panda_arm(Engine, lib, use_ik=0, control_orientation=1, n=2, steps=4, seed=11, solver_iters=None):
    """The Panda's robot-level engine (half-wave lane groups with motor records) against the oracle: reset; fused command + step
    from identical states; finger commands with a force and a velocity bound (pandaEnv.apply_action_fingers: force 10,
    maxVelocity 1, panda_env.py:218-225); apply_action(max_vel) + stepSimulation loops (helloworld_panda.py:99-140)."""
    eng, ora = make_panda_arm_pair(Engine, lib, n, use_ik, control_orientation)
    assert eng.state_floats == ora.state_floats == 80 and eng.ndof == 9 and eng.act_dim == ora.task.n_act and eng.obs_dim == ora.obs_dim == 37
    xo = eng.x_off
    obs = eng.reset()
    st_o, mrec, obs_o = ora.hands_reset(n)
    st_e = eng.get_state()
    assert rel(st_e[:, :xo], st_o[:, :xo]).max() < 2e-4, rel(st_e[:, :xo], st_o[:, :xo]).max()
    assert rel(obs, obs_o).max() < 2e-3
    W = 32
    mot = eng.get_motor_state()
    assert mot.shape == (n, 4, W) and np.abs(mot[:, 0, :9] - mrec[:, :9]).max() < 1e-5 and (mot[:, 3] == 0).all()
    if solver_iters is not None:        # (everything after the reset at this sweep count, in engine and oracle)
        set_solver_iters(eng, solver_iters, ora)
    rng = np.random.default_rng(seed)
    home = np.array([0.0, -0.54, 0.0, -2.6, -0.30, 2.0, 1.0, 0.02, 0.02])
    worst, flips = {}, 0
    st = st_o
    for k in range(steps):
        if k == 1:      # grasp: fingers towards 0 with force 10 and maxVelocity 1
            eng.set_motors([7, 8], [0.0, 0.0], 0.1, 10.0, max_vel=1.0)
            mrec = ora.hands_set_motors(mrec, [7, 8], [0.0, 0.0], 0.1, 10.0, max_vel=1.0)
        if use_ik:
            a = np.tile(np.array([0.45, 0.0, 0.85, np.pi, 0.0, 0.0][:eng.act_dim], np.float32), (n, 1))
            a[:, :3] += rng.uniform(-0.03, 0.03, (n, 3)).astype(np.float32)
        else:
            a = (home[None, :] + rng.uniform(-0.2, 0.2, (n, 9)) * np.r_[np.ones(7), 0.05, 0.05]).astype(np.float32)
        s32 = st.astype(np.float32)
        eng.set_state(s32)
        m32 = np.zeros((n, 4, W), np.float32)
        for c in range(4):
            m32[:, c, :9] = mrec[:, c * orc.MAXD:c * orc.MAXD + 9]
        eng.set_motor_state(m32)
        ob, rw, dn = eng.step(a)
        so, mrec, out = ora.hands_step(s32.astype(np.float64), mrec, a)
        se = eng.get_state()
        flip = np.abs(se[:, :9] - so[:, :9]).max(1) > TOL_PANDA_ARM["q"] if use_ik else np.zeros(n, bool)
        flips += int(flip.sum())
        if (~flip).any():
            merge_worst(worst, group_quantities(eng, se[~flip], so[~flip], ob[~flip], out[~flip], tail=7))
        if flip.any():
            assert_within(group_quantities(eng, se[flip], so[flip], ob[flip], out[flip], tail=7), TOL_ICUB_IK_FLIP, "(IK flip, step %d)" % k)
        assert np.abs(ob[:, -7:] - out[:, -9:-2]).max() < 1e-5 and not dn.any()
        st = so
    assert flips <= max(1, n * steps // 10)
    assert_within(worst, TOL_PANDA_ARM, "(Panda robot level, %d IK flips)" % flips)
    # apply_action(max_vel) alone, then the simulation advances with the motors holding the command
    s32 = st.astype(np.float32)
    eng.set_state(s32)
    for c in range(4):
        m32[:, c, :9] = mrec[:, c * orc.MAXD:c * orc.MAXD + 9]
    eng.set_motor_state(m32)
    if use_ik:
        a = np.tile(np.array([0.5, 0.05, 0.8, np.pi, 0.0, 0.0][:eng.act_dim], np.float32), (n, 1))
    else:
        a = np.tile((home + np.r_[0.6 * np.ones(7), 0, 0]).astype(np.float32), (n, 1))
    eng.apply_action(a, max_vel=0.5)
    so, mrec = ora.hands_apply_action(s32.astype(np.float64), mrec, a, max_vel=0.5)
    mot = eng.get_motor_state()
    for c in range(4):
        assert np.abs(mot[:, c, :9] - mrec[:, c * orc.MAXD:c * orc.MAXD + 9]).max() < (2e-3 if use_ik else 1e-6), c
    if use_ik:
        assert (mot[:, 3, :7] == 0.5).all() and (mot[:, 1, :7] == np.float32(0.1)).all() and (mot[:, 3, 7:9] == m32[:, 3, 7:9]).all()
        for c in range(4):      # continue from identical commands (the IK may stop one iteration apart)
            m32[:, c, :9] = mrec[:, c * orc.MAXD:c * orc.MAXD + 9]
        eng.set_motor_state(m32)
    eng.settle(12)
    so = ora.hands_settle(so, mrec, 12)
    se = eng.get_state()
    assert np.abs(se[:, :9] - so[:, :9]).max() < 2e-5 and np.abs(se[:, 32:41] - so[:, 32:41]).max() < 2e-3
    if use_ik:
        assert np.abs(se[:, 32:39]).max() <= 0.5 + 1e-3        # the velocity bound binds: no arm joint moves faster than max_vel
    return eng


# ---------------------------------------------------------------------------------------------- iCub, robot-level interface
TOL_ICUB_ARM = dict(TOL_ICUB)      # measured on the lane emulation: q 8e-8, qd 1.2e-5, EE velocity 1e-5 m/s, everything else <= 3e-7


def make_icub_arm_pair(Engine, lib, n, control_arm="l", use_ik=0, control_orientation=1, reset=True, **kw):
    """iCubEnv used alone (pbre_config.robot_level = 1; reference icub_env.py:91-151, 259-360): engine (built by the drop-in class)
    + oracle, same scene.  reset=False: the engine as its constructor leaves it, for checks that set state and motor record themselves
    (tests/arm_rows.py).  The drop-in class builds its engine and resets it in one go (202 settle steps per env); the engine is still
    built by that code, with its arguments, and only the new INSTANCE answers that one reset() without doing anything."""
    from pybullet_robot_envs import _client
    from pybullet_robot_envs.envs.icub_envs import icub_env
    cid = _client.connect(n, lib=lib)
    robot = icub_env.iCubEnv(cid, use_IK=use_ik, control_arm=control_arm, control_orientation=control_orientation)
    if reset:
        eng = robot._robot_level()
    else:
        make = icub_env._capi.make_engine

        def make_unreset(*a, **k):
            e = make(*a, **k)
            e.reset = lambda mask=None: None
            return e
        icub_env._capi.make_engine = make_unreset
        try:
            eng = robot._robot_level()
        finally:
            icub_env._capi.make_engine = make
        del eng.reset                      # the class's reset() again
    ora, tbl, info = orc.icub_arm_oracle(control_arm, use_ik, control_orientation)
    ph = eng.get_physics()
    for f in ("table_c", "table_h", "obj_h", "obj_inertia"):
        for k in range(3):
            getattr(ora.params, f)[k] = getattr(ph, f)[k]
    ora.params.obj_mass = ph.obj_mass
    return robot, eng, ora, cid


def check_icub_arm(Engine, lib, control_arm="l", use_ik=0, control_orientation=1, n=2, steps=4, seed=5):
    """The iCub's robot-level engine (ShapeIA: half-wave lane groups with motor records) against the oracle: reset; fused command
    + step from identical states; apply_action(max_vel) + stepSimulation loops, through the drop-in iCubEnv."""
    from pybullet_robot_envs import _client
    robot, eng, ora, cid = make_icub_arm_pair(Engine, lib, n, control_arm, use_ik, control_orientation)
    nd = 20
    assert eng.state_floats == ora.state_floats == 80 and eng.ndof == nd and eng.act_dim == ora.task.n_act and eng.obs_dim == ora.obs_dim == 31
    xo = eng.x_off
    st_o, mrec, obs_o = ora.hands_reset(n)
    st_e = eng.get_state()
    obs = eng.observe()
    assert rel(st_e[:, :xo], st_o[:, :xo]).max() < 2e-3, rel(st_e[:, :xo], st_o[:, :xo]).max()
    assert rel(obs, obs_o).max() < 2e-2
    W = 32
    mot = eng.get_motor_state()
    assert mot.shape == (n, 4, W) and np.abs(mot[:, 0, :nd] - mrec[:, :nd]).max() < 2e-3 and (mot[:, 3] == 0).all()
    rng = np.random.default_rng(seed)
    dofs = robot.controlled_dofs()
    home = np.array(robot.sim_home())[dofs]
    hand = np.array(robot._home_hand_pose, np.float64)
    worst, flips = {}, 0
    st = st_o
    m32 = np.zeros((n, 4, W), np.float32)
    for k in range(steps):
        if use_ik:
            a = np.tile(hand[:eng.act_dim].astype(np.float32), (n, 1))
            a[:, :3] += rng.uniform(-0.03, 0.03, (n, 3)).astype(np.float32)
        else:
            a = (home[None, :] + rng.uniform(-0.2, 0.2, (n, len(dofs)))).astype(np.float32)
        s32 = st.astype(np.float32)
        eng.set_state(s32)
        for c in range(4):
            m32[:, c, :nd] = mrec[:, c * orc.MAXD:c * orc.MAXD + nd]
        eng.set_motor_state(m32)
        ob, rw, dn = eng.step(a)
        so, mrec, out = ora.hands_step(s32.astype(np.float64), mrec, a)
        se = eng.get_state()
        flip = np.abs(se[:, :nd] - so[:, :nd]).max(1) > TOL_ICUB_ARM["q"] if use_ik else np.zeros(n, bool)
        flips += int(flip.sum())
        if (~flip).any():
            merge_worst(worst, group_quantities(eng, se[~flip], so[~flip], ob[~flip], out[~flip]))
        if flip.any():
            assert_within(group_quantities(eng, se[flip], so[flip], ob[flip], out[flip]), TOL_ICUB_IK_FLIP, "(IK flip, step %d)" % k)
        assert not dn.any()
        st = so
    assert flips <= max(1, n * steps // 10)
    assert_within(worst, TOL_ICUB_ARM, "(iCub robot level, %d IK flips)" % flips)
    # apply_action(max_vel) through the drop-in class, then the simulation advances with the motors holding the command
    s32 = st.astype(np.float32)
    eng.set_state(s32)
    for c in range(4):
        m32[:, c, :nd] = mrec[:, c * orc.MAXD:c * orc.MAXD + nd]
    eng.set_motor_state(m32)
    if use_ik:
        cmd = hand[:6].copy(); cmd[:3] += [0.05, -0.04, 0.06]
        a = np.tile(cmd[:eng.act_dim].astype(np.float32), (n, 1))
        robot.apply_action(list(cmd[:6] if control_orientation else cmd[:3]), max_vel=0.5)
    else:
        a = np.tile((home + 0.5).astype(np.float32), (n, 1))
        robot.apply_action(list(home + 0.5), max_vel=0.5)
    so, mrec = ora.hands_apply_action(s32.astype(np.float64), mrec, a, max_vel=0.5)
    mot = eng.get_motor_state()
    for c in range(4):
        assert np.abs(mot[:, c, :nd] - mrec[:, c * orc.MAXD:c * orc.MAXD + nd]).max() < (5e-3 if use_ik else 1e-6), c
    if use_ik:
        assert (mot[:, 3, :nd] == 0.5).all() and (mot[:, 1, :nd] == np.float32(0.2)).all()
        for c in range(4):      # continue from identical commands (the IK may stop one iteration apart)
            m32[:, c, :nd] = mrec[:, c * orc.MAXD:c * orc.MAXD + nd]
        eng.set_motor_state(m32)
    else:
        lo, hi = np.array(robot.ll), np.array(robot.ul)
        ctl = [j for j, idx in enumerate(robot._joint_name_to_ids.values()) if idx in robot._joints_to_control]
        assert np.abs(mot[:, 0, dofs] - np.clip(home + 0.5, lo[ctl], hi[ctl])).max() < 1e-6       # clipped to the joint limits
        assert (mot[:, 3, dofs] == 0.5).all() and (mot[:, 1, dofs] == np.float32(0.5)).all()
    robot.step_simulation(12)
    so = ora.hands_settle(so, mrec, 12)
    se = eng.get_state()
    assert np.abs(se[:, :nd] - so[:, :nd]).max() < 5e-5 and np.abs(se[:, 32:32 + nd] - so[:, 32:32 + nd]).max() < 5e-3
    # (the bound is on each motor's target velocity; a joint still carrying momentum from the random steps before may be faster for a while)
    obs_r, lim = robot.get_observation()
    assert np.asarray(obs_r).shape[-1] == 9 + len(dofs) and len(lim) == 9 + len(dofs)
    _client.disconnect(cid)
    return worst


def run_panda_demo(robot, upto=4):
    """The scripted grasp of the reference's examples/helloworlds/helloworld_panda.py:89-140 on a stand-alone pandaEnv (IK control):
    pre-grasp, above the object, down to it, close the fingers, lift.  Returns the object poses [N, 7] after the phases run."""
    import math as m
    quat = [float(x) for x in robot._quat_from_euler(np.array([[m.pi, 0.0, 0.0]]))[0]]
    poses = []
    robot.pre_grasp(); robot.step_simulation(1)
    robot.apply_action([0.5, 0.0, 0.9] + quat); robot.step_simulation(100)                              # 1: above the object
    poses.append(robot.get_object_pose())
    if upto >= 2:
        robot.apply_action([0.5, 0.0, 0.67] + quat, max_vel=5); robot.pre_grasp(); robot.step_simulation(200)   # 2: down
        poses.append(robot.get_object_pose())
    if upto >= 3:
        robot.grasp(0); robot.step_simulation(120)                                                     # 3: close the fingers
        poses.append(robot.get_object_pose())
    if upto >= 4:
        robot.apply_action([0.5, 0.0, 0.9] + quat, max_vel=5); robot.grasp(0); robot.step_simulation(200)       # 4: up
        poses.append(robot.get_object_pose())
    return poses


# the Panda's robot-level engine with robot-object contacts, one step from identical states (check_panda_arm_grasp, tests/arm_rows.py)
TOL_PANDA_ARM_CONTACT = {"q": 2e-5, "qd": 5e-3, "obj_pos": 5e-6, "obj_quat": 5e-5}


def check_panda_arm_grasp(Engine, lib, n=1, steps=3):
    """Robot-object contacts of the Panda's robot-level engine against the oracle: the demo is run up to the closed grasp (both
    fingers squeezing the object: force-limited, velocity-limited finger motors, 2-4 robot-object contacts + object-table contacts),
    then single steps from identical states: state, fingertip forces / counts (observation tail)."""
    from pybullet_robot_envs import _client
    from pybullet_robot_envs.envs.panda_envs.panda_env import pandaEnv
    cid = _client.connect(n, lib=lib)
    robot = pandaEnv(cid, use_IK=1)
    run_panda_demo(robot, upto=3)
    eng = robot._client.engine
    _, ora = make_panda_arm_pair(Engine, lib, 1, 1, 1)
    n_tip, f_tip = robot.check_contact_fingertips(0)
    assert (np.atleast_1d(n_tip) == 2).all() and (np.atleast_2d(f_tip) > 1.0).all(), (n_tip, f_tip)
    st = eng.get_state().astype(np.float64)
    mot = eng.get_motor_state()
    mrec = np.zeros((n, 4 * orc.MAXD))
    for c in range(4):
        mrec[:, c * orc.MAXD:c * orc.MAXD + 9] = mot[:, c, :9]
    xo = eng.x_off
    a = st[:, xo + 6:xo + 12].astype(np.float32)                 # keep commanding the current hand pose
    seen = 0
    for k in range(steps):
        s32 = st.astype(np.float32)
        eng.set_state(s32)
        m32 = eng.get_motor_state()
        for c in range(4):
            m32[:, c, :9] = mrec[:, c * orc.MAXD:c * orc.MAXD + 9]
        eng.set_motor_state(m32)
        ob, rw, dn = eng.step(a)
        so, mrec2, out = ora.hands_step(s32.astype(np.float64), mrec, a)
        # the fused step re-commands all 9 motors from the IK (gain 0.2, default force): same on both sides
        se = eng.get_state()
        q = group_quantities(eng, se, so, ob, out, tail=7)
        tail_e, tail_o = ob[:, -7:], out[:, -9:-2]
        assert np.array_equal(tail_e[:, 5:], tail_o[:, 5:]), (tail_e, tail_o)                     # fingers in contact, contact points
        assert np.abs(tail_e[:, :5] - tail_o[:, :5]).max() < 2e-2 * (1.0 + np.abs(tail_o[:, :5]).max()), (tail_e, tail_o)
        assert all(q[k] < v for k, v in TOL_PANDA_ARM_CONTACT.items()), q
        seen = max(seen, int(tail_o[:, 6].max()))
        st, mrec = so, mrec2
    assert seen >= 2
    _client.disconnect(cid)


def check_per_env_physics(Engine, lib, table, n=8, flags=0):
    """Per-env domain randomisation (pbre_set_physics_per_env; reference change_physics_params, panda_push_gym_env.py:362-368): every
    env gets its own object mass / lateral friction / linear damping; sliding cubes and a pushed-into cube against the oracle with
    the same per-env values (they live in the state record), the values change the result, and they survive resets."""
    eng, ora = make_pair(Engine, lib, table, n, flags=flags)
    st = check_reset(eng, ora, n)
    rng = np.random.default_rng(17)
    mass = rng.uniform(0.05, 0.4, n).astype(np.float32)
    mu = rng.uniform(0.3, 1.2, n).astype(np.float32)
    damp = rng.uniform(0.0, 0.3, n).astype(np.float32)
    rdamp = rng.uniform(0.0, 0.5, n).astype(np.float32)     # the arm links' linear damping, per env (robot_damping, :365-367)
    eng.set_physics_per_env(obj_mass=mass, obj_mu=mu, obj_lin_damping=damp, robot_lin_damping=rdamp)
    se = eng.get_state()
    assert np.array_equal(se[:, 44], mass) and np.array_equal(se[:, 45], mu) and np.array_equal(se[:, 47], damp + 1) and np.array_equal(se[:, 31], rdamp + 1)
    st = se.astype(np.float64)
    st[:, 25:28] = [0.3, -0.2, 0.0]                        # sliding cubes: friction, mass and damping all matter
    # (a cube sliding on four saturated friction rows: its angular velocity carries the rounding of the contact impulses divided by
    # the 3.5 cm lever -- the bound of the contact-rich states applies to the object's rotation)
    tol = dict(TOL, obj_w=TOL_CONTACT["obj_w"], obj_quat=TOL_CONTACT["obj_quat"], obs_obj_eul=TOL_CONTACT["obs_obj_eul"], obs_rel_eul=TOL_CONTACT["obs_rel_eul"])
    rep = check_single_steps(eng, ora, st, rng, steps=3, tol=tol)
    # the same states with the batch defaults give a different object motion
    base = st.copy(); base[:, [44, 45, 47]] = 0
    eng.set_state(base.astype(np.float32))
    a = rng.uniform(-1, 1, (n, 7)).astype(np.float32)
    eng.step(a); s0 = eng.get_state()
    eng.set_state(st.astype(np.float32)); eng.step(a); s1 = eng.get_state()
    assert np.abs(s0[:, 25:27] - s1[:, 25:27]).max() > 1e-4
    assert np.array_equal(s0[:, :9], s1[:, :9])            # the robot does not touch the object: unaffected by the object's parameters
    # ... the robot's own damping: with the default (practically unbounded) motors a POSITION_CONTROL joint reaches its target velocity
    # whatever the damping, so the check runs with force-limited motors (max_motor_impulse 0.02, as check_panda_force_limited): there
    # the damping changes the arm's motion, the engine follows the oracle, and the untouched object is unaffected
    e2, o2 = make_pair(Engine, lib, table, n, flags=flags, phys={"max_motor_impulse": 0.02})
    o2.params.max_motor_impulse = 0.02
    e2.reset()
    e2.set_physics_per_env(robot_lin_damping=rdamp)
    sd = e2.get_state().astype(np.float64)
    assert np.array_equal(sd[:, 31], rdamp + 1)
    sd[:, 16:23] = 1.0                                     # moving arm: the damping acts on the links' velocities
    s32 = sd.astype(np.float32)
    base = s32.copy(); base[:, 31] = 0
    e2.set_state(base); e2.step(a); s2 = e2.get_state()
    e2.set_state(s32); e2.step(a); s3 = e2.get_state()
    big = rdamp > 0.2
    assert np.abs(s2[big, 16:25] - s3[big, 16:25]).max() > 1e-4 and np.array_equal(s2[:, 9:16], s3[:, 9:16])
    so3, _ = o2.batch_step(s32.astype(np.float64), a)
    assert np.abs(s3[:, :9] - so3[:, :9]).max() < TOL_CONTACT["q"] and np.abs(s3[:, 16:25] - so3[:, 16:25]).max() < TOL_CONTACT["qd"]
    e2.close()
    # resets (full, masked) keep the per-env values; a masked set changes only the selected envs
    eng.reset()
    assert np.array_equal(eng.get_state()[:, [44, 45, 47, 31]], np.stack([mass, mu, damp + 1, rdamp + 1], 1))
    m = np.zeros(n, np.uint8); m[[1, n - 1]] = 1
    eng.reset(mask=m)
    assert np.array_equal(eng.get_state()[:, [44, 45, 47, 31]], np.stack([mass, mu, damp + 1, rdamp + 1], 1))
    eng.set_physics_per_env(obj_mass=np.full(n, 0.2, np.float32), mask=m)
    want = mass.copy(); want[[1, n - 1]] = 0.2
    assert np.array_equal(eng.get_state()[:, 44], want)
    return rep


def check_other_objects(Engine, lib, table, names=("YcbGelatinBox", "domino/domino", "YcbCrackerBox"), n=6, flags=0):
    """obj_name other than the cube (reference world_env.py:18-25, 179-216): box stand-ins with their own size, mass, principal
    inertias and friction (model/objects.py).  The lane-per-env kernel steps such an object with ObjStep, complex envs go to the row
    kernel; against the oracle with the same box: reset (the object drops, tips and settles), sliding / spinning objects, a pushed
    object (robot-object contact)."""
    from pybullet_robot_envs.model.objects import object_physics
    out = {}
    for name in names:
        ph = object_physics(name)
        eng, ora = make_pair(Engine, lib, table, n, flags=flags, phys=ph)
        orc.set_object(ora, ph)
        ora32 = orc.Oracle(table, f32=True, task=1)
        ora32.task.obj_pose_rnd_std, ora32.task.tg_pose_rnd_std = ora.task.obj_pose_rnd_std, ora.task.tg_pose_rnd_std
        orc.set_object(ora32, ph)
        eng.reset()
        st, _ = ora.batch_reset(n)
        se = eng.get_state()
        assert np.isfinite(se).all()
        # (201 free-running settle steps; a tall box -- the cracker box is 21 cm high on a 6 cm base -- lands, rocks on its edges and
        # settles: measured 5.3e-4 in the lumped measure on the GPU's general row kernel, 1e-4 .. 4e-4 elsewhere)
        assert rel(se[:, :31], st[:, :31]).max() < 1.5e-3, (name, rel(se[:, :31], st[:, :31]).max())
        assert np.abs(se[:, 11] - (0.625 + ph["obj_h"][2])).max() < 5e-3, (name, se[:, 11])       # stands on the table on its z face (a tall box still rocks a little)
        rng = np.random.default_rng(5)
        s = st.copy()
        s[:, 25:28] = rng.uniform(-0.1, 0.1, (n, 3)) * [1, 1, 0]            # sliding
        s[:, 30] = rng.uniform(-1, 1, n)                                    # spinning about z
        # (a tall narrow box that slides starts to rock on an edge: vertices enter / leave the contact margin, where fp32 and fp64 may
        # pick different contact sets -- such states are excluded like the other threshold-ambiguous ones, and counted)
        tol = dict(TOL_CONTACT, obj_pos=2e-6, obs_obj_pos=2e-6, obj_v=5e-4)
        rep = check_single_steps(eng, ora, s, rng, steps=3, tol=tol, skip_ambiguous=True, max_skip=0.5, ora32=ora32, max_outliers=0.1)
        out[name] = dict(rep["worst"], skipped=rep["skipped_ambiguous"], outliers=rep.get("outliers", 0), compared=rep["compared"])
        # robot-object contact: the object placed against the fingers (complex env -> row kernel for a non-cube box)
        ee = eng.observe()[:, :3].astype(np.float64)
        s2 = st.copy()
        s2[:, 9:12] = ee + [0.0, 0.0, -(ph["obj_h"][2] + 0.012)]
        s2[:, 12:16] = [0, 0, 0, 1]
        check_single_steps(eng, ora, s2, rng, steps=1, tol=TOL_CONTACT, skip_ambiguous=True, max_skip=0.5, ora32=ora32, max_outliers=0.1)
        eng.close()
    return out


def contacts_flags_of(eng, table, states):
    from pybullet_robot_envs.model import contacts
    return contacts.contact_flags(table, np.asarray(states, np.float64), eng.ndof, eng.get_physics())


def check_round_objects(Engine, lib, table, names=("YcbTennisBall", "YcbTomatoSoupCan", "duck_vhacd"), n=6, flags=0):
    """The round members of the object list (reference world_env.py:18-25, 179-216; model/objects.py: ROUND_OBJECTS) as sphere / cylinder
    primitives, against the oracle with the same primitive:
      * reset: the object drops onto the table and settles (ball on its lowest point, can on its base);
      * a ROLLING object, free running for 120 steps from the same state in both: a ball given a push ends up rolling without
        slipping (|v - omega x r| -> 0: the property a box stand-in cannot have), a can lying on its side rolls along, an upright can
        slides on its base; single steps from identical states on the way, per quantity;
      * robot-object contact: the object placed against the fingers (sphere-vs-sphere / sphere-vs-cylinder rows)."""
    from pybullet_robot_envs.model.objects import object_physics
    out = {}
    for name in names:
        ph = object_physics(name)
        shape, r, hh = ph["obj_shape"], ph["obj_h"][0], ph["obj_h"][2]
        eng, ora = make_pair(Engine, lib, table, n, flags=flags, phys=ph)
        orc.set_object(ora, ph)
        assert eng.get_physics().obj_shape == shape and ora.params.obj_shape == shape and shape in (1, 2)
        ora32 = orc.Oracle(table, f32=True, task=1)
        ora32.task.obj_pose_rnd_std, ora32.task.tg_pose_rnd_std = ora.task.obj_pose_rnd_std, ora.task.tg_pose_rnd_std
        orc.set_object(ora32, ph)
        eng.reset()
        st, _ = ora.batch_reset(n)
        se = eng.get_state()
        assert np.isfinite(se).all()
        assert rel(se[:, :31], st[:, :31]).max() < 5e-4, (name, rel(se[:, :31], st[:, :31]).max())
        assert np.abs(se[:, 11] - (0.625 + hh)).max() < 2e-3, (name, se[:, 11])
        rng = np.random.default_rng(15)
        # ---- rolling / sliding, free running
        s = st.copy()
        s[:, 32:35] = [0.9, 0.9, 0.65]                                       # far target: no success on the way
        lying = shape == 2 and name != "duck_vhacd"
        if lying:                                                            # can on its side: axis along world x, resting on the table
            s[:, 12:16] = [0.0, np.sqrt(0.5), 0.0, np.sqrt(0.5)]
            s[:, 11] = 0.625 + r
        s[:, 25:28] = [0.0, 0.25, 0.0]                                       # pushed along +y (a lying can: across its axis)
        s32 = s.astype(np.float32)
        eng.set_state(s32)
        so = s32.astype(np.float64)
        zero = np.zeros((n, 7), np.float32)
        worst = {}
        for k in range(120):
            eng.step(zero)
            so, _ = ora.batch_step(so, zero)
        se = eng.get_state().astype(np.float64)
        v, w = so[:, 25:28], so[:, 28:31]
        rep = {"free_run_obj_pos_diff": float(np.abs(se[:, 9:12] - so[:, 9:12]).max()), "travel_cm": float(100 * (so[:, 10] - s[:, 10]).mean())}
        if shape == 1 or lying:
            slip = v[:, 1] + w[:, 0] * r                                    # contact-point velocity of a body rolling along +y: v_y - (omega x (0,0,-r))_y
            rep["slip_over_speed"] = float(np.abs(slip).max() / max(np.abs(v[:, 1]).max(), 1e-9))
            assert np.abs(v[:, 1]).min() > 0.05 and rep["slip_over_speed"] < 0.02, (name, rep, v[0], w[0])      # still moving, rolling without slipping
            assert np.abs(se[:, 28] * r + se[:, 26]).max() < 0.02 * np.abs(se[:, 26]).max() + 1e-4                # ... in the engine as well
        else:
            assert np.abs(v[:, :2]).max() < 1e-3 and np.abs(so[:, 12:14]).max() < 1e-3, (name, v[0], so[0, 12:16])     # friction stopped the upright can; it did not tip
        assert rep["free_run_obj_pos_diff"] < 2e-4, (name, rep)
        # ---- single steps from identical states while it moves
        # (from the rolling / resting states the free run ended in, nudged a little: a ball with an arbitrary spin sits on the edge of
        # its friction cone -- sticking in one tangent direction, sliding in the other -- where a rounding decides the regime; the
        # conditioning probe of check_single_steps would skip most of such states)
        s2 = so.copy()
        s2[:, 25:28] += rng.uniform(-0.01, 0.01, (n, 3)) * [1, 1, 0]
        tol = dict(TOL_CONTACT, obj_pos=2e-6, obs_obj_pos=2e-6, obj_v=5e-4)
        r1 = check_single_steps(eng, ora, s2, rng, steps=3, tol=tol, skip_ambiguous=True, max_skip=0.5, ora32=ora32, max_outliers=0.1)
        rep.update(dict(r1["worst"], skipped=r1["skipped_ambiguous"], outliers=r1.get("outliers", 0), compared=r1["compared"]))
        # ---- robot-object contact: the object under the fingers (complex env -> the row kernel's sphere-vs-round rows)
        from pybullet_robot_envs.model.table import panda_table, PANDA_SPHERES
        _, model = panda_table()
        s3 = st.copy()
        for e in range(n):                                                   # one hand / finger sphere ~2 mm inside the object, from above or from the side
            q = s3[e, :9]
            cs, rs = scenarios.sphere_centres(ora, model, PANDA_SPHERES, q)[-1 - (e % 4)]
            pen = 0.002
            if shape == 1:
                d = rng.normal(size=3); d[2] = -abs(d[2]) - 0.5; d /= np.linalg.norm(d)
                s3[e, 9:12] = cs + d * (rs + r - pen)
            elif e % 2 == 0:
                s3[e, 9:12] = cs + np.array([0.0, 0.0, -(rs + hh - pen)])     # the sphere on the can's top cap
            else:
                d = np.array([np.cos(0.7 * e), np.sin(0.7 * e), 0.0])
                s3[e, 9:12] = cs + d * (rs + r - pen)                          # ... on its lateral surface
            s3[e, 12:16] = [0, 0, 0, 1]
        f3 = contacts_flags_of(eng, table, s3)
        assert (f3 & 2).all(), ("the crafted states have no robot-object contact", f3)
        r2 = check_single_steps(eng, ora, s3, rng, steps=1, tol=TOL_CONTACT, skip_ambiguous=True, max_skip=0.5, ora32=ora32, max_outliers=0.1)
        rep["robot_contact_compared"] = r2["compared"]
        out[name] = rep
        eng.close()
    return out


def hull_test_objects():
    """name -> (vertices [nv, 3], mass, mu): synthetic convex hulls (no mesh of the reference's objects exists on any box): the cube as its 8
    vertices in the box primitive's vertex order, a tetrahedron, a 20-vertex rounded blob ("duck"), a 32-vertex one (the 16-lane kernels'
    two-pass candidate selection)"""
    h = 0.025
    out = {"box8": (np.array([[(1 if v & 1 else -1) * h, (1 if v & 2 else -1) * h, (1 if v & 4 else -1) * h] for v in range(8)], float), 0.1, 1.0)}
    out["tetra"] = (0.035 * np.array([[1, 1, 1], [1, -1, -1], [-1, 1, -1], [-1, -1, 1]], float), 0.05, 1.0)
    for name, nv, seed in (("blob20", 20, 7), ("blob32", 32, 8)):
        r = np.random.default_rng(seed)
        d = r.normal(size=(nv, 3)); d /= np.linalg.norm(d, axis=1)[:, None]
        out[name] = (d * [0.045, 0.035, 0.03], 0.1, 1.0)
    return out


def hull_surface_samples(verts, rng, n):
    """n (point on the hull's surface, outward unit normal there) pairs in the object frame: interior points of faces (even samples) and
    vertices with the mean normal of their faces (odd samples: inside the vertex's normal cone)"""
    from scipy.spatial import ConvexHull
    H = ConvexHull(verts)
    out = []
    for k in range(n):
        if k % 2 == 0:
            f = int(rng.integers(len(H.simplices)))
            w = rng.dirichlet([2.0, 2.0, 2.0])
            out.append((w @ verts[H.simplices[f]], H.equations[f, :3].copy()))
        else:
            v = int(H.vertices[rng.integers(len(H.vertices))])
            nn = H.equations[[i for i, t in enumerate(H.simplices) if v in t], :3].mean(0)
            out.append((verts[v].copy(), nn / np.linalg.norm(nn)))
    return out


def check_hull_objects(Engine, lib, table, names=("box8", "tetra", "blob20", "blob32"), n=6, flags=0):
    """Convex-hull objects (include/pbre.h: pbre_set_object_hull; engine: Core::step's hull candidates + sphere_hull) against the
    oracle's brute-force restatement (oracle/pbre_oracle.c: sphere_hull over ALL vertex triples -- not the engine's face table):
      * reset: the hull drops onto the table and settles on a face;
      * sliding / spinning hulls, single steps from identical states, per quantity;
      * robot-object contact: a finger / hand sphere 2 mm inside a face or at a vertex of the hull;
      * box8 (the cube as its 8 vertices): additionally against THIS engine with the box primitive (general kernel), the same states --
        the object-table rows bit for bit (same candidates, same order), the robot-object rows within the single-step bounds."""
    from pybullet_robot_envs.model.objects import hull_physics
    from pybullet_robot_envs.model.table import panda_table, PANDA_SPHERES
    from pybullet_robot_envs.model import contacts
    _, model = panda_table()
    out = {}
    for name in names:
        verts, mass, mu = hull_test_objects()[name]
        ph = hull_physics(verts, mass, mu)
        hv = np.asarray(ph["obj_hull"], float)
        eng, ora = make_pair(Engine, lib, table, n, flags=flags, phys=ph)
        orc.set_object(ora, ph)
        assert eng.get_physics().obj_shape == 3 and ora.params.obj_shape == 3 and ora.params.obj_hull_n == len(hv)
        ora32 = orc.Oracle(table, f32=True, task=1)
        ora32.task.obj_pose_rnd_std, ora32.task.tg_pose_rnd_std = ora.task.obj_pose_rnd_std, ora.task.tg_pose_rnd_std
        orc.set_object(ora32, ph)
        eng.reset()
        st, _ = ora.batch_reset(n)
        se = eng.get_state()
        assert np.isfinite(se).all()
        rep = {"reset_rel": float(rel(se[:, :31], st[:, :31]).max()), "rest_height": float(st[:, 11].mean() - 0.625)}
        # (201 free-running steps: a blob lands on a vertex, tips over an edge and settles on a face -- the lumped measure of the tall boxes)
        # A rounded blob dropped 7 cm lands on a vertex and tumbles over edges onto some face: which face is decided by roundings (fp32
        # against fp64), so for the blobs the two resets are only required to END alike -- at rest on the table, robot in the same pose --,
        # and everything below starts from the oracle's settled state in both.
        if name in ("box8", "tetra"):
            assert rep["reset_rel"] < 1.5e-3, (name, rep)
        else:
            # (measured: the blob still rocks at up to 5 rad/s when the reset's 101 steps with the world end -- in both; lumped difference 0.015)
            assert rep["reset_rel"] < 0.05 and rel(se[:, :9], st[:, :9]).max() < 1e-4, (name, rep)
            zero = np.zeros((n, 7), np.float32)
            for _ in range(600):                                             # let the oracle's blob come to rest: the base state of the checks below
                st, _o = ora.batch_step(st, zero)
            st[:, 35] = 0                                                    # (step counter)
            assert np.abs(st[:, 25:31]).max() < 0.02, (name, np.abs(st[:, 25:31]).max())
        assert (st[:, 11] > 0.625).all() and (st[:, 11] < 0.625 + ph["obj_h"][2] + 0.02).all(), (name, st[:, 11])
        rng = np.random.default_rng(25)
        s = st.copy()
        s[:, 32:35] = [0.9, 0.9, 0.65]
        s[:, 25:28] = rng.uniform(-0.1, 0.1, (n, 3)) * [1, 1, 0]
        s[:, 30] = rng.uniform(-1, 1, n)
        tol = dict(TOL_CONTACT, obj_pos=2e-6, obs_obj_pos=2e-6, obj_v=5e-4)
        r1 = check_single_steps(eng, ora, s, rng, steps=3, tol=tol, skip_ambiguous=True, max_skip=0.5, ora32=ora32, max_outliers=0.1)
        rep.update(dict(r1["worst"], skipped=r1["skipped_ambiguous"], outliers=r1.get("outliers", 0), compared=r1["compared"]))
        # ---- robot-object contact: a sphere of the hand 2 mm inside the hull at a face point / a vertex
        s3 = st.copy()
        s3[:, 32:35] = [0.9, 0.9, 0.65]
        samples = hull_surface_samples(hv, rng, n)
        for e in range(n):
            cs, rs = scenarios.sphere_centres(ora, model, PANDA_SPHERES, s3[e, :9])[-1 - (e % 4)]
            ps, nn = samples[e]
            # rotate the hull so that the sampled normal points from the object up at the sphere (a rotation about a horizontal axis + yaw)
            up = np.array([0.3 * np.cos(e), 0.3 * np.sin(e), 1.0]); up /= np.linalg.norm(up)
            ax = np.cross(nn, up); sn = np.linalg.norm(ax); cn = float(nn @ up)
            if sn < 1e-9:
                quat = np.array([0.0, 0.0, 0.0, 1.0]) if cn > 0 else np.array([1.0, 0.0, 0.0, 0.0])
            else:
                half = 0.5 * np.arctan2(sn, cn)
                quat = np.append(ax / sn * np.sin(half), np.cos(half))
            x, y, z, w = quat
            R = np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - w * z), 2 * (x * z + w * y)], [2 * (x * y + w * z), 1 - 2 * (x * x + z * z), 2 * (y * z - w * x)],
                          [2 * (x * z - w * y), 2 * (y * z + w * x), 1 - 2 * (x * x + y * y)]])
            s3[e, 12:16] = quat
            s3[e, 9:12] = cs - R @ (ps + nn * (rs - 0.002))          # sphere centre = surface point + normal x (radius - 2 mm)
        f3 = contacts.contact_flags(table, s3, eng.ndof, eng.get_physics(), hull=hv)
        assert (f3 & 2).all(), ("the crafted states have no robot-object contact", name, f3)
        r2 = check_single_steps(eng, ora, s3, rng, steps=1, tol=TOL_CONTACT, skip_ambiguous=True, max_skip=0.5, ora32=ora32, max_outliers=0.1)
        rep["robot_contact_compared"] = r2["compared"]
        if name == "box8":
            # the same states through the box PRIMITIVE on the general kernel
            prim = dict(ph); prim.pop("obj_hull"); prim["obj_shape"] = 0
            engb, _ = make_pair(Engine, lib, table, n, flags=flags | 4, phys=prim)          # PBRE_F_FORCE_GENERAL: the kernel the hull takes
            engb.reset()
            for states, exact in ((s, True), (s3, False)):
                s32 = states.astype(np.float32)
                eng.set_state(s32); engb.set_state(s32)
                a = rng.uniform(-1, 1, (n, 7)).astype(np.float32)
                oa, ob_ = eng.step(a), engb.step(a)
                ea, eb = eng.get_state().astype(np.float64), engb.get_state().astype(np.float64)
                if exact:
                    assert np.array_equal(ea, eb) and all(np.array_equal(x, y) for x, y in zip(oa, ob_)), "box-as-hull: object-table rows differ from the box primitive"
                else:
                    q = {"q": np.abs(ea[:, 0:9] - eb[:, 0:9]).max(), "qd": np.abs(ea[:, 16:25] - eb[:, 16:25]).max(), "obj_pos": np.abs(ea[:, 9:12] - eb[:, 9:12]).max(),
                         "obj_v": np.abs(ea[:, 25:28] - eb[:, 25:28]).max(), "obj_w": np.abs(ea[:, 28:31] - eb[:, 28:31]).max()}
                    assert_within(q, TOL_CONTACT, "(box as 8 hull vertices against the box primitive, robot-object contact)")
            engb.close()
        out[name] = rep
        eng.close()
    return out


def check_reset_snapshot(Engine, lib, table, n=8, **over):
    """pbre_reset_snapshot against an explicit masked pbre_reset of the same envs and episodes: the same sampled object pose and target
    (bit-identical: same Philox streams), the settled heights / robot pose within 5e-5, zero velocities, cleared counters; the other
    envs untouched; and an error before the first full reset."""
    import pytest
    kw = dict(task=1, num_envs=n, lib=lib, obj_pose_rnd_std=0.05, tg_pose_rnd_std=0.2)
    kw.update(over)
    a, b = Engine(table, **kw), Engine(table, **kw)
    m = np.zeros(n, np.uint8); m[[1, n - 2]] = 1
    with pytest.raises(RuntimeError, match="no settled snapshot"):
        a.reset_snapshot(m)
    a.reset(); b.reset()
    rng = np.random.default_rng(3)
    for _ in range(5):
        act = rng.uniform(-1, 1, (n, a.act_dim)).astype(np.float32)
        a.step(act); b.step(act)
    before = a.get_state()
    oa = a.reset_snapshot(m)
    ob = b.reset(mask=m)
    sa, sb = a.get_state(), b.get_state()
    nd, vo, xo = a.ndof, a.v_off, a.x_off
    keep = m == 0
    assert np.array_equal(sa[keep], before[keep]) and np.array_equal(sb[keep], before[keep])
    d = m == 1
    assert np.array_equal(sa[d, xo + 5], sb[d, xo + 5]) and (sa[d, xo + 5] == 1).all() and (sa[d, xo + 3] == 0).all()
    assert np.abs(sa[d][:, :nd + 7] - sb[d][:, :nd + 7]).max() < 5e-5
    assert np.abs(sa[d][:, vo:vo + nd + 6]).max() < 1e-6
    assert np.abs(sa[d][:, xo:xo + 3] - sb[d][:, xo:xo + 3]).max() < 5e-5
    assert np.abs(sa[d][:, xo + 6:xo + 14] - sb[d][:, xo + 6:xo + 14]).max() < 2e-4
    assert np.abs(oa[d] - ob[d]).max() < 2e-3 and np.array_equal(oa[keep], ob[keep])
    # and the batch keeps stepping identically-ish from there
    act = rng.uniform(-1, 1, (n, a.act_dim)).astype(np.float32)
    ra, rb = a.step(act), b.step(act)
    assert np.abs(ra[0] - rb[0]).max() < 5e-3 and np.array_equal(ra[2], rb[2])
    return a


# ---------------------------------------------------------------------------------------------- round 3: crafted contact states, closed-loop pushes
def icub_contact_states(ora, info, base, rng, n_obj=12, n_table=12, n_both=12, n_limit=12, control_arm="l"):
    """Crafted iCub states (joint control) for every contact category of the pipeline: a hand / forearm sphere pressed ~2 mm into the
    object (kw_quad_rc's coupled solve), one within [-4 mm, +0.8 mm] of the table top (kw_quad's robot-table rows), both, and a
    controlled joint beyond its limit.  Returns (states, kinds)."""
    from pybullet_robot_envs.model.table import icub_model, icub_spheres
    m = icub_model()
    names = [l["name"] for l in m["links"]]
    sph = [(names.index(ln), np.array(c), r) for ln, c, r in icub_spheres(m) if ln.startswith(control_arm + "_")]
    nd = ora.ndof
    ctrl = list(info["controlled"])
    lo = np.array([ora.model.lower[ora.model.link_of_dof[k]] for k in range(nd)])
    hi = np.array([ora.model.upper[ora.model.link_of_dof[k]] for k in range(nd)])
    home = np.asarray(base[:nd], float)
    ztop = ora.params.table_c[2] + ora.params.table_h[2]
    vo = (len(base) - 16) // 2
    oh = np.array([ora.params.obj_h[k] for k in range(3)])

    def centres(q):
        R, p = ora.fk(q)
        return [(p[i] + R[i] @ c, r) for i, c, r in sph]

    def arm_config(spread):
        q = home.copy()
        q[ctrl] += rng.normal(0, spread, len(ctrl))
        return np.clip(q, lo + 2e-3, hi - 2e-3)

    def on_table(q):
        ds = [c[2] - r - ztop for c, r in centres(q) if abs(c[0] - ora.params.table_c[0]) < ora.params.table_h[0] and abs(c[1] - ora.params.table_c[1]) < ora.params.table_h[1]]
        return bool(ds) and -0.004 < min(ds) < 0.0008

    def table_config():
        for _ in range(20000):
            q = arm_config(0.5)
            if on_table(q):
                return q
        raise RuntimeError("no table-contact configuration found")

    shape = int(ora.params.obj_shape)

    def clear_of_object(q, s):
        from pybullet_robot_envs.model import contacts as _ct
        cs = centres(q)
        C = np.array([c for c, _ in cs]); Rr = np.array([r for _, r in cs])
        oc = np.asarray(s[nd:nd + 3], float)
        qo = np.asarray(s[nd + 3:nd + 7], float)
        Ro = np.broadcast_to(_ct._quat_R(qo[None])[0], (len(cs), 3, 3))
        dist = (_ct._sphere_box_dist(C, Rr, oc[None], Ro, oh) if shape == 0 else _ct._sphere_round_dist(shape, C, Rr, oc[None], Ro, oh))
        return dist.min() > 0.005

    def put_object(s, q, pen=0.002):
        """the object against one arm sphere, ~pen deep; no other sphere deeper than that, the object not sunk into the table"""
        from pybullet_robot_envs.model import contacts as _ct
        cs = centres(q)
        C = np.array([c for c, _ in cs]); Rr = np.array([r for _, r in cs])
        I3 = np.broadcast_to(np.eye(3), (len(cs), 3, 3))
        for _ in range(4000):
            i = rng.integers(0, len(sph))
            c, r = cs[i]
            d = rng.normal(size=3); d[2] = -abs(d[2]); d /= np.linalg.norm(d)       # the object lies below / beside the hand
            k = int(np.argmax(np.abs(d)))                                           # face the sphere with the box's nearest face
            dd = np.zeros(3); dd[k] = np.sign(d[k])
            ext = oh[k]
            if shape == 1:                                                          # ball: any direction, radius oh[0]
                dd, ext = d, oh[0]
            elif shape == 2 and k < 2:                                              # upright cylinder touched on its side: radial direction
                dd = np.array([d[0], d[1], 0.0]) / np.hypot(d[0], d[1]); ext = oh[0]
            oc = c + dd * (r + ext - pen)
            if shape != 1 and k < 2 and oc[2] - oh[2] < ztop and abs(ztop + oh[2] + 2e-4 - c[2]) < oh[2] - 1e-3:
                oc[2] = ztop + oh[2] + 2e-4                                          # touched on its side: stand it on the table
            dist = (_ct._sphere_box_dist(C, Rr, oc[None], I3, oh) if shape == 0 else _ct._sphere_round_dist(shape, C, Rr, oc[None], I3, oh))
            bottom = oc[2] - (oh[0] if shape == 1 else oh[2])
            over_table = abs(oc[0] - ora.params.table_c[0]) < ora.params.table_h[0] and abs(oc[1] - ora.params.table_c[1]) < ora.params.table_h[1]
            if dist.min() >= -(pen + 5e-4) and (not over_table or bottom >= ztop - 1e-3):
                break
        else:
            raise RuntimeError("no object placement found")
        s[nd:nd + 3] = oc
        s[nd + 3:nd + 7] = [0, 0, 0, 1]
        s[vo + nd:vo + nd + 6] = rng.normal(0, 0.1, 6)

    out, kinds = [], []
    for kind, cnt in (("object", n_obj), ("table", n_table), ("both", n_both), ("limit", n_limit)):
        for _ in range(cnt):
            s = np.array(base, float)
            for _ in range(200):
                q = table_config() if kind in ("table", "both") else arm_config(0.3)
                if kind == "limit":
                    j = ctrl[rng.integers(0, len(ctrl))]
                    q[j] = (lo[j] - rng.uniform(0.005, 0.02)) if rng.random() < 0.5 else (hi[j] + rng.uniform(0.005, 0.02))
                if kind in ("object", "both") or clear_of_object(q, s):
                    break                                                           # (a big object at its reset pose: the arm must not be inside it)
            else:
                raise RuntimeError("no arm configuration clear of the object found")
            s[:nd] = q
            s[vo:vo + nd] = 0.0
            s[vo + np.array(ctrl)] = rng.normal(0, 0.3, len(ctrl))
            if kind in ("object", "both"):
                put_object(s, q)
            out.append(s); kinds.append(kind)
    return np.array(out), kinds


def check_icub_contact_states(Engine, lib, n_each=12, steps=1, seed=21, control_arm="l", obj_name=None):
    """>= 48 crafted contact states of the iCub push env (joint control), one step each against the oracle with per-quantity bounds
    (TOL_ICUB_CONTACT); states whose contact set flips under a +-3 um nudge of the margin are skipped and counted.
    obj_name: a member of the object list instead of the cube (model/objects.py; the round ones: sphere / cylinder primitives)."""
    kw = {}
    ph = None
    if obj_name is not None:
        from pybullet_robot_envs.model.objects import object_physics
        ph = object_physics(obj_name)
        kw["phys"] = ph
    eng0, ora, info = make_icub_pair(Engine, lib, 1, task=1, control_arm=control_arm, use_ik=0, obj_std=0.0, tg_std=0.2, **kw)
    if ph is not None:
        orc.set_object(ora, ph)
    base, _ = ora.batch_reset(1)
    rng = np.random.default_rng(seed)
    S, kinds = icub_contact_states(ora, info, base[0], rng, n_each, n_each, n_each, n_each, control_arm)
    n = len(S)
    eng, ora, info = make_icub_pair(Engine, lib, n, task=1, control_arm=control_arm, use_ik=0, obj_std=0.0, tg_std=0.2, max_steps=10 ** 6, **kw)
    if ph is not None:
        orc.set_object(ora, ph)
        assert eng.get_physics().obj_shape == ph["obj_shape"] == ora.params.obj_shape
    ora.task.max_steps = 10 ** 6
    eng.reset()
    kinds = np.array(kinds)
    rep = {"states": n, "skipped_ambiguous": 0}
    worst = {}
    st = S
    for k in range(steps):
        a = rng.uniform(-1, 1, (n, eng.act_dim)).astype(np.float32)
        s32 = st.astype(np.float32)
        eng.set_state(s32)
        ob, rw, dn = eng.step(a)
        se = eng.get_state()
        so, out = ora.batch_step(s32.astype(np.float64), a)
        ok = ~ambiguous_envs(ora, s32.astype(np.float64), a)
        rep["skipped_ambiguous"] += int((~ok).sum())
        for kind in ("object", "table", "both", "limit"):
            sel = ok & (kinds == kind)
            if sel.any():
                w = group_quantities(eng, se[sel], so[sel], ob[sel], out[sel])
                merge_worst(worst, w)
                rep[kind] = dict((kk, float("%.3g" % v)) for kk, v in w.items())
        st = so
    rep["complex_envs_stepped"] = eng.kernel_info()[5]
    assert rep["skipped_ambiguous"] <= n * steps // 5, rep
    assert_within(worst, TOL_ICUB_CONTACT, "(iCub crafted contact states: %d states, %d skipped as ambiguous)" % (n, rep["skipped_ambiguous"]))
    rep["worst"] = dict((kk, float("%.3g" % v)) for kk, v in worst.items())
    return rep


def five_fingertip_brick(ora, info, q, tips, obj_hz):
    """The brick's pose in the five-fingertip scene for the joints q (fingers straight, the thumb in the plane of the four tips): its
    5 x 7.5 cm face against the five tip spheres (links `tips`, centre 16.8 mm along x, radius 7.5 mm), on the side away from the palm, the
    shallowest tip 0.5 mm deep.  obj_hz: the brick's half height.  -> centre, quaternion, rotation matrix, (ex, ey, nrm): the face's
    in-plane axes and the normal that points from the tips into the brick"""
    R, p = ora.fk(q)
    c = np.array([p[i] + R[i] @ np.array([0.0168, 0.0, 0.0]) for i in tips])
    cen = c.mean(0)
    _, _, vt = np.linalg.svd(c - cen)
    ex, ey, nrm = vt[0], vt[1], vt[2]
    assert np.abs((c - cen) @ nrm).max() < 1e-3, "the five fingertips are not coplanar"
    palm = p[info["ee_link"]]
    if (palm - cen) @ nrm > 0:                            # the box goes on the side away from the palm
        nrm = -nrm
    ex = np.cross(ey, nrm)                                # right-handed frame (box x = ey: 5 cm, box y = ex: 7.5 cm, box z = nrm)
    u, v = (c - cen) @ ex, (c - cen) @ ey
    mid = cen + ex * 0.5 * (u.max() + u.min()) + ey * 0.5 * (v.max() + v.min())
    Rb = np.stack([ey, ex, -nrm] if np.linalg.det(np.stack([ey, ex, nrm], 1)) < 0 else [ey, ex, nrm], 1)
    if np.linalg.det(Rb) < 0:
        Rb[:, 0] = -Rb[:, 0]
    depth = (c - cen) @ nrm                               # > 0: further into the box side
    # face plane at cen + nrm * f: a tip sphere (radius 7.5 mm) penetrates by depth - f + 0.0075; the shallowest tip gets 0.5 mm
    f = depth.min() + 0.0075 - 0.0005
    centre = mid + nrm * (f + obj_hz) - nrm * ((mid - cen) @ nrm)
    tr = Rb[0, 0] + Rb[1, 1] + Rb[2, 2]
    qw = np.sqrt(max(1e-12, 1 + tr)) / 2
    quat = np.array([(Rb[2, 1] - Rb[1, 2]) / (4 * qw), (Rb[0, 2] - Rb[2, 0]) / (4 * qw), (Rb[1, 0] - Rb[0, 1]) / (4 * qw), qw])
    return centre, quat, Rb, (ex, ey, nrm)


def check_hands_five_fingertips(Engine, lib, control_arm="r", steps=3):
    """All five fingertips of the hand on the object: fingers straight, the thumb brought into the plane of the four fingertips
    (thumb joints 1.1775 / 1.37375 / 0.785 / 0: the five tip centres are coplanar within 0.1 mm), the brick-sized box held against
    them with its 5 x 7.5 cm face, every tip sphere 0.5 - 1.5 mm inside it (the thumb and the index touch it at its edges).  State,
    fingertip forces and contact counts against the oracle, per quantity (TOL_HANDS_CONTACT)."""
    from pybullet_robot_envs.model.table import icub_hands_model, hand_joint_names
    eng, ora, info = make_hands_pair(Engine, lib, 1, control_arm, 0)
    eng.reset()
    st_o, mrec, _ = ora.hands_reset(1)
    nd = 60
    m = icub_hands_model()
    by_joint = {l.get("joint_name"): i for i, l in enumerate(m["links"])}
    jn = hand_joint_names(control_arm)
    s = st_o.copy()
    fing = list(info["fingers"])
    pose = [0.0] * 16 + [1.1775, 1.37375, 0.785, 0.0]
    s[0, fing] = pose
    s[0, eng.v_off:eng.v_off + nd] = 0.0
    tips = [by_joint[jn[k]] for k in (3, 7, 11, 15, 19)]
    centre, quat, _, _ = five_fingertip_brick(ora, info, s[0, :nd], tips, eng.get_physics().obj_h[2])
    s[0, nd:nd + 3] = centre
    s[0, nd + 3:nd + 7] = quat
    s[0, eng.v_off + nd:eng.v_off + nd + 6] = 0
    a = np.asarray(info["home"], np.float32)[info["controlled"]][None, :].copy()
    ctrl = list(info["controlled"])
    for j, t in zip(fing, pose):
        a[0, ctrl.index(j)] = t
    eng.set_motors(fing, pose, 0.1, 10.0)
    mrec = ora.hands_set_motors(mrec, fing, pose, 0.1, 10.0)
    worst, seen = {}, 0
    for k in range(steps):
        s32 = s.astype(np.float32)
        eng.set_state(s32)
        ob, rw, dn = eng.step(a)
        so, mrec, out = ora.hands_step(s32.astype(np.float64), mrec, a)
        se = eng.get_state()
        merge_worst(worst, group_quantities(eng, se, so, ob, out, tail=7))
        tail_e, tail_o = ob[0, -7:], out[0, -9:-2]
        assert np.array_equal(tail_e[5:], tail_o[5:]), (tail_e, tail_o)                 # tips in contact, contact points
        assert np.abs(tail_e[:5] - tail_o[:5]).max() < 2e-2 * (1.0 + np.abs(tail_o[:5]).max()), (tail_e, tail_o)
        seen = max(seen, int(tail_o[5]))
        if k == 0:
            assert int(tail_o[5]) == 5, "only %d fingertips touch the object in the crafted state" % int(tail_o[5])
        s = so
    assert_within(worst, TOL_HANDS_CONTACT, "(hands, %d fingertips on the object, arm %s)" % (seen, control_arm))
    worst["fingertips_in_contact"] = seen
    return worst


def check_panda_push_closed_loop(Engine, lib, table, n=8, seed=5):
    """Long horizon WITH pushing: the scripted push of tests/scenarios.py (approach behind the cube, sweep +x through it), run closed
    loop -- every side tracks the joint targets from its OWN joint angles -- in the engine and in the oracle, free running for 280
    steps from the same reset.  The robot-object contact is contact-chaotic in detail (a 1e-7 difference decides which sphere touches
    first), but the push is a robust macroscopic event: per env, the cube's final displacement agrees within 1.5 cm (and 25 % of its
    length; measured on the GPU, 16 envs pushed 11 - 28 cm: 12 of them within 0.2 mm, the worst 2.8 cm on a 21 cm push), every cube moved
    more than 3 cm in both, and the arm -- position controlled, but pressing on a cube that sits a little differently -- ends within 1.5e-2 rad
    (measured 7e-3 in the env with the 2.8 cm difference, 2e-6 on the CPU emulation's 4 envs)."""
    eng, ora = make_pair(Engine, lib, table, n, obj_std=0.03, tg_std=0.0, max_steps=10 ** 6)
    ora.task.max_steps = 10 ** 6
    st = check_reset(eng, ora, n)
    st[:, 32:35] = [0.9, 0.9, 0.65]                       # far target: the episode does not end on the way
    st = st.astype(np.float32).astype(np.float64)
    eng.set_state(st.astype(np.float32))
    obj0 = st[:, 9:12].copy()
    plans = [scenarios.push_actions(ora, st[e]) for e in range(n)]
    n_app, n_push = plans[0][2], plans[0][3]
    se = eng.get_state().astype(np.float64)
    from pybullet_robot_envs.model import contacts as _ct
    ph = eng.get_physics()
    seq_same = np.ones(n, bool)         # the robot-object contact timeline of the env is the same on both sides, step for step
    for k in range(n_app + n_push):
        goal = [p[0] if k < n_app else p[1] for p in plans]
        a_e = np.array([np.append(scenarios.track(se[e], goal[e], 1.0 if k < n_app else 0.35), 0.0)[:7] for e in range(n)], np.float32)
        a_o = np.array([np.append(scenarios.track(st[e], goal[e], 1.0 if k < n_app else 0.35), 0.0)[:7] for e in range(n)], np.float32)
        eng.step(a_e)
        st, _ = ora.batch_step(st, a_o)
        se = eng.get_state().astype(np.float64)
        fe = _ct.contact_flags(table, se, 9, ph) & _ct.ROBOT_OBJECT
        fo = _ct.contact_flags(table, st, 9, ph) & _ct.ROBOT_OBJECT
        seq_same &= fe == fo
    de, do = se[:, 9:12] - obj0, st[:, 9:12] - obj0
    le, lo_ = np.linalg.norm(de[:, :2], axis=1), np.linalg.norm(do[:, :2], axis=1)
    rep = {"touched_envs": int((lo_ > 1e-3).sum()), "disp_engine_cm": np.round(100 * le, 2).tolist(), "disp_oracle_cm": np.round(100 * lo_, 2).tolist(),
           "worst_disp_diff_cm": float(100 * np.linalg.norm(de - do, axis=1).max()), "arm_q_diff": float(np.abs(se[:, :7] - st[:, :7]).max())}
    dd = np.linalg.norm(de - do, axis=1)
    rep["median_disp_diff_mm"] = float(1e3 * np.median(dd))
    rep["envs_within_1mm"] = int((dd < 1e-3).sum())
    if MEASURE:
        print("MEASURED (closed-loop push):", rep)
    assert rep["touched_envs"] == n and (le > 0.03).all() and (lo_ > 0.03).all(), rep
    # every env: the loose stick-slip bound (an env whose first touch falls one step apart in fp32 and fp64 integrates that difference) ...
    assert (dd <= 0.015 + 0.25 * lo_).all(), rep
    assert rep["arm_q_diff"] < 1.5e-2, rep
    # ... and (round-3 advice) the MAJORITY tightly: the median env ends within 1 mm of the oracle's cube, which a 10 % error in the
    # friction or contact rows -- 1 to 3 cm on these pushes -- could not pass
    assert rep["median_disp_diff_mm"] < 1.0 and rep["envs_within_1mm"] >= (n + 1) // 2, rep
    # ... and (round-4 verdict) TIGHTLY wherever the contact sequence did not diverge: an env in which the robot touches the cube in exactly
    # the same steps on both sides has no first-touch offset to integrate, and ends within 1 mm + 1 % of the push
    rep["envs_with_identical_contact_timeline"] = int(seq_same.sum())
    rep["worst_disp_diff_mm_identical_timeline"] = float(1e3 * dd[seq_same].max()) if seq_same.any() else None
    assert seq_same.sum() >= n // 4, rep
    assert (dd[seq_same] <= 1e-3 + 0.01 * lo_[seq_same]).all(), rep
    return rep


def check_icub_push_closed_loop(Engine, lib, n=8, steps=330, seed=6):
    """The iCub's counterpart: the hand is brought behind the cube and swept through it, closed loop on each side's OWN joint angles
    (joint control: with Cartesian control the restated IK closed loop is itself chaotic -- two branches of the damped-least-squares
    solution a rounding apart whip the arm differently, section 2 of DESIGN.md -- so a per-env comparison is only meaningful in joint
    space; the joint targets of the sweep come from the oracle's IK once, before the rollout).  Engine and oracle run free from the same
    reset; per env the cube's final displacement agrees within 3 mm (and 5 % of its length; measured: 0.5 mm on pushes of 2.5 - 8.6 cm),
    every cube was pushed > 2 cm in both."""
    eng, ora, info = make_icub_pair(Engine, lib, n, task=1, control_arm="l", use_ik=0, obj_std=0.03, tg_std=0.0, max_steps=10 ** 6)
    ora.task.max_steps = 10 ** 6
    eng.reset()
    st, _ = ora.batch_reset(n)
    xo, nd = eng.x_off, eng.ndof
    st[:, xo:xo + 3] = [0.9, 0.9, 0.65]
    s32 = st.astype(np.float32)
    eng.set_state(s32)
    st = s32.astype(np.float64)
    obj0 = st[:, nd:nd + 3].copy()
    ctrl = np.array(info["controlled"])
    ik_ora, _, _ = orc.icub_oracle("l", task=1, use_ik=1, control_orientation=0)
    hand_eul = np.array([ik_ora.task.home_hand_pose[k] for k in range(3, 6)])
    plans = []
    for e in range(n):
        q_up, _ = ik_ora.ik(st[e, :nd], obj0[e] + np.array([-0.085, 0.0, 0.13]), hand_eul)       # above and behind the cube first:
        q_pre, _ = ik_ora.ik(q_up, obj0[e] + np.array([-0.085, 0.0, 0.035]), hand_eul)           # the straight joint-space path would cut through it
        q_end, _ = ik_ora.ik(q_pre, obj0[e] + np.array([0.02, 0.0, 0.035]), hand_eul)
        plans.append((q_up, q_pre, q_end))
    scale = float(ora.task.act_scale)
    n_up, n_app = 90, 170

    def phase(k):
        return (0, 1.0) if k < n_up else ((1, 0.3) if k < n_app else (2, 0.06))

    def track(q, goal, amax):
        return np.clip((goal[ctrl] - q[ctrl]) / scale * 2.0, -amax, amax).astype(np.float32)

    se = eng.get_state().astype(np.float64)
    for k in range(steps):
        a_e = np.array([track(se[e], plans[e][phase(k)[0]], phase(k)[1]) for e in range(n)], np.float32)
        a_o = np.array([track(st[e], plans[e][phase(k)[0]], phase(k)[1]) for e in range(n)], np.float32)
        eng.step(a_e)
        st, _ = ora.batch_step(st, a_o)
        se = eng.get_state().astype(np.float64)
    de, do = se[:, nd:nd + 3] - obj0, st[:, nd:nd + 3] - obj0
    le, lo_ = np.linalg.norm(de[:, :2], axis=1), np.linalg.norm(do[:, :2], axis=1)
    rep = {"touched_envs": int((lo_ > 1e-3).sum()), "disp_engine_cm": np.round(100 * le, 2).tolist(), "disp_oracle_cm": np.round(100 * lo_, 2).tolist(),
           "worst_disp_diff_cm": float(100 * np.linalg.norm(de - do, axis=1).max()), "arm_q_diff": float(np.abs(se[:, :nd] - st[:, :nd]).max())}
    if MEASURE:
        print("MEASURED (iCub closed-loop push):", rep)
    assert rep["touched_envs"] == n and (le > 0.02).all() and (lo_ > 0.02).all(), rep
    assert (np.linalg.norm(de - do, axis=1) <= 0.003 + 0.05 * lo_).all(), rep
    return rep


def check_hands_demo_against_oracle(lib, n=1):
    """BASELINE config 5 closed loop: the reference's scripted grasp (examples/helloworlds/helloworld_icub.py:61-125) through the drop-in
    iCubHandsEnv on the engine AND, command by command, on the fp64 oracle (every pbre_apply_action / pbre_set_motors / pbre_settle the
    class issues is mirrored by orc_hands_apply_action / orc_hands_set_motors / orc_hands_settle): ~370 free-running steps with the
    fingers closing on the brick, lifting, carrying and releasing it.  Compared per phase: the brick's position.  Bounds (measured on the
    lane emulation / the GPU -> bound): fingers closed 0.3 mm -> 2 mm; lifted (19.5 cm up in both) 1.3 mm -> 5 mm; carried 5 mm -> 2 cm;
    after the release the brick tumbles onto the table: both at rest height of some face, landing spots within 8 cm."""
    import math as m
    from pybullet_robot_envs import _client
    from pybullet_robot_envs.envs.icub_envs.icub_env_with_hands import iCubHandsEnv
    cid = _client.connect(n, lib=lib)
    robot = iCubHandsEnv(cid, use_IK=1, control_arm='r')
    eng = robot._engine
    ora, tbl, info = orc.hands_oracle('r', use_ik=1)
    ph = eng.get_physics()
    for f in ("table_c", "table_h", "obj_h", "obj_inertia"):
        for k in range(3):
            getattr(ora.params, f)[k] = getattr(ph, f)[k]
    ora.params.obj_mass = ph.obj_mass
    ora.params.implicit_joint_damping = ph.implicit_joint_damping
    st_o, mrec, _ = ora.hands_reset(n)
    nd = eng.ndof
    se = eng.get_state()
    assert np.abs(se[:, :nd] - st_o[:, :nd]).max() < 5e-4 and np.abs(se[:, nd:nd + 7] - st_o[:, nd:nd + 7]).max() < 1e-6      # same scene, same settled pose
    S = {"st": st_o, "mr": mrec}
    e_apply, e_motors, e_settle = eng.apply_action, eng.set_motors, eng.settle

    def apply_action(a, max_vel=-1.0):
        e_apply(a, max_vel=max_vel)
        S["st"], S["mr"] = ora.hands_apply_action(S["st"], S["mr"], np.asarray(a, np.float64), max_vel)

    def set_motors(dofs, targets, kp, max_force=0.0, mask=None, max_vel=0.0):
        e_motors(dofs, targets, kp, max_force, mask)
        S["mr"] = ora.hands_set_motors(S["mr"], dofs, targets, kp, max_force)

    def settle(k, *a):
        e_settle(k)
        S["st"] = ora.hands_settle(S["st"], S["mr"], k)

    eng.apply_action, eng.set_motors, eng.settle = apply_action, set_motors, settle

    def quat(e):
        cr, sr, cp, sp, cy, sy = m.cos(e[0] / 2), m.sin(e[0] / 2), m.cos(e[1] / 2), m.sin(e[1] / 2), m.cos(e[2] / 2), m.sin(e[2] / 2)
        return [sr * cp * cy - cr * sp * sy, cr * sp * cy + sr * cp * sy, cr * cp * sy - sr * sp * cy, cr * cp * cy + sr * sp * sy]

    def brick():
        return eng.get_state()[:, nd:nd + 3].astype(np.float64), S["st"][:, nd:nd + 3].copy()

    rep = {}
    q2 = quat([m.pi / 2, m.pi / 3, -m.pi])
    pos_cl = [0, 0.6, 0.8, 1.0, 0, 0.6, 0.8, 1.0, 0, 0.6, 0.8, 1.0, 0, 0.6, 0.8, 1.0, 1.57, 0.8, 0.5, 0.8]
    robot.pre_grasp(); robot.step_simulation(10)
    robot.apply_action([0.49, 0.0, 0.8] + quat([0, 0, m.pi / 2]), max_vel=5); robot.pre_grasp(); robot.step_simulation(60)
    robot.apply_action([0.485, 0.0, 0.72] + q2, max_vel=5); robot.pre_grasp(); robot.step_simulation(60)
    be, bo = brick(); rest = bo[:, 2].copy()
    rep["untouched_diff_m"] = float(np.abs(be - bo).max())
    assert rep["untouched_diff_m"] < 1e-6
    robot.grasp(pos_cl); robot.step_simulation(60)
    be, bo = brick(); rep["closed_diff_m"] = float(np.abs(be - bo).max())
    assert rep["closed_diff_m"] < 2e-3, rep
    robot.apply_action([0.45, 0, 0.9] + q2, max_vel=5); robot.grasp(pos_cl); robot.step_simulation(60)
    be, bo = brick(); rep["lifted_diff_m"] = float(np.abs(be - bo).max())
    rep["lift_engine_m"], rep["lift_oracle_m"] = float((be[:, 2] - rest).min()), float((bo[:, 2] - rest).min())
    assert rep["lift_engine_m"] > 0.05 and rep["lift_oracle_m"] > 0.05 and rep["lifted_diff_m"] < 5e-3, rep
    robot.apply_action([0.3, -0.2, 0.9] + quat([0.0, 0.0, m.pi / 2]), max_vel=5); robot.grasp(pos_cl); robot.step_simulation(60)
    be, bo = brick(); rep["carried_diff_m"] = float(np.abs(be - bo).max())
    assert rep["carried_diff_m"] < 2e-2 and (be[:, 2] - rest).min() > 0.05 and (bo[:, 2] - rest).min() > 0.05, rep
    robot.pre_grasp(); robot.step_simulation(50)
    be, bo = brick(); rep["released_xy_diff_m"] = float(np.abs(be[:, :2] - bo[:, :2]).max())
    hmax = float(max(ph.obj_h[k] for k in range(3))) + 0.02
    assert (be[:, 2] < rest + hmax).all() and (bo[:, 2] < rest + hmax).all() and rep["released_xy_diff_m"] < 8e-2, rep
    eng.apply_action, eng.set_motors, eng.settle = e_apply, e_motors, e_settle
    _client.disconnect(cid)
    return rep


def check_panda_demo_against_oracle(lib, n=1):
    """The Panda counterpart: the reference's scripted grasp (examples/helloworlds/helloworld_panda.py:89-140) through the drop-in pandaEnv
    on the engine and, command by command, on the fp64 oracle (pbre_apply_action / pbre_set_motors / pbre_set_motor_state / pbre_settle
    mirrored): above the object, down to it, fingers closed on it, lifted.  ~620 free-running steps; the object's position per phase."""
    from pybullet_robot_envs import _client
    from pybullet_robot_envs.envs.panda_envs.panda_env import pandaEnv
    cid = _client.connect(n, lib=lib)
    robot = pandaEnv(cid, use_IK=1)
    eng = robot._robot_level()
    ora, tbl = orc.panda_arm_oracle(1, 1)
    ph = eng.get_physics()
    for f in ("table_c", "table_h", "obj_h", "obj_inertia"):
        for k in range(3):
            getattr(ora.params, f)[k] = getattr(ph, f)[k]
    ora.params.obj_mass = ph.obj_mass
    st_o, mrec, _ = ora.hands_reset(n)
    nd = eng.ndof
    se = eng.get_state()
    assert np.abs(se[:, :nd] - st_o[:, :nd]).max() < 5e-5 and np.abs(se[:, nd:nd + 7] - st_o[:, nd:nd + 7]).max() < 1e-6
    S = {"st": st_o, "mr": mrec}
    e_apply, e_motors, e_settle, e_setm = eng.apply_action, eng.set_motors, eng.settle, eng.set_motor_state

    def apply_action(a, max_vel=-1.0):
        e_apply(a, max_vel=max_vel)
        S["st"], S["mr"] = ora.hands_apply_action(S["st"], S["mr"], np.asarray(a, np.float64), max_vel)

    def set_motors(dofs, targets, kp, max_force=0.0, mask=None, max_vel=0.0):
        e_motors(dofs, targets, kp, max_force, mask, max_vel=max_vel)
        S["mr"] = ora.hands_set_motors(S["mr"], dofs, targets, kp, max_force, max_vel=max_vel)

    def set_motor_state(mot):
        e_setm(mot)
        for c in range(4):
            S["mr"][:, c * orc.MAXD:c * orc.MAXD + nd] = mot[:, c, :nd]

    def settle(k, *a):
        e_settle(k)
        S["st"] = ora.hands_settle(S["st"], S["mr"], k)

    eng.apply_action, eng.set_motors, eng.settle, eng.set_motor_state = apply_action, set_motors, settle, set_motor_state
    rep = {}
    poses = run_panda_demo(robot, upto=4)
    bo = S["st"][:, nd:nd + 3]
    be = np.atleast_2d(np.asarray(poses[3]))[:, :3]
    rest = np.atleast_2d(np.asarray(poses[0]))[:, 2]
    rep["lifted_diff_m"] = float(np.abs(be - bo).max())
    rep["lift_engine_m"], rep["lift_oracle_m"] = float((be[:, 2] - rest).min()), float((bo[:, 2] - rest).min())
    eng.apply_action, eng.set_motors, eng.settle, eng.set_motor_state = e_apply, e_motors, e_settle, e_setm
    _client.disconnect(cid)
    assert rep["lift_engine_m"] > 0.1 and rep["lift_oracle_m"] > 0.1 and rep["lifted_diff_m"] < 5e-3, rep
    return rep


def sliding_cube_reference(v0, mu, g, kl, dt, pyramid=1.0):
    """1-D restatement of a cube sliding along a friction-pyramid axis on the table under Coulomb friction and Bullet's velocity damping,
    with the step's own discretisation (semi-implicit Euler: the damped, friction-limited velocity first, then the position):
    v <- max(0, v - dt (pyramid mu g + kl (1 + |v|) v)), x <- x + dt v.  Returns the stopping distance."""
    v, x = float(v0), 0.0
    while v > 0.0:
        v = max(0.0, v - dt * (pyramid * mu * g + kl * (1.0 + abs(v)) * v))
        x += dt * v
    return x


def check_sliding_cube_kat(step_fn, st0, params, v0s=(0.3, 0.6)):
    """Analytic contact KAT (no PyBullet needed): the cube, given a horizontal velocity, must stop after the distance Coulomb friction
    mu = obj_mu * table_mu predicts (sliding_cube_reference), straight, without turning or lifting.  Along a world axis -- the axes of
    Bullet's friction pyramid on a horizontal plane (btPlaneSpace1 of n = +z) -- and along the diagonal, where the two clamped axis rows
    decelerate it sqrt(2) times harder (the pyramid approximation Bullet makes).  step_fn(state) -> next state under zero actions."""
    mu, g, kl, dt = params["mu"], params["g"], params["kl"], params["dt"]
    rep = {}
    for v0 in v0s:
        for name, d, pyr in (("axis", np.array([1.0, 0.0]), 1.0), ("diagonal", np.array([1.0, 1.0]) / np.sqrt(2.0), np.sqrt(2.0))):
            s = np.array(st0, np.float64).copy()
            s[:, 25:27] = v0 * d
            s[:, 27:31] = 0.0
            x0, q0 = s[0, 9:12].copy(), s[0, 12:16].copy()
            for k in range(600):
                s = np.asarray(step_fn(s), np.float64)
                if np.abs(s[0, 25:28]).max() < 1e-7 and k > 3:
                    break
            dist = float((s[0, 9:11] - x0[:2]) @ d)
            ref = sliding_cube_reference(v0, mu, g, kl, dt, pyr)
            rep["%s_v%.1f" % (name, v0)] = {"distance_m": dist, "reference_m": ref}
            assert abs(dist - ref) < 0.01 * ref + 2e-5, (name, v0, dist, ref)
            side = float((s[0, 9:11] - x0[:2]) @ np.array([-d[1], d[0]]))
            assert abs(side) < 1e-4 and abs(s[0, 11] - x0[2]) < 2e-4, (name, side, s[0, 11] - x0[2])          # straight, stays down
            assert np.abs(s[0, 12:16] - q0).max() < 2e-4, (name, s[0, 12:16], q0)                             # does not turn
    return rep


def check_rolling_onset_kat(make_step, v0=0.5):
    """Analytic contact KAT for the round primitives: a body set sliding without spin on a plane with Coulomb friction ends up rolling at
    v0 / (1 + I / (m r^2)) -- 5/7 v0 for a solid sphere, 2/3 v0 for a solid cylinder rolling on its side -- whatever the friction
    coefficient (angular momentum about the contact point is conserved).  Bullet's velocity damping (0.04 per second on both twists) takes
    ~1 % off during the 20-40 steps of the sliding phase: the bound is [-3.5 %, +0.5 %].  make_step(name) -> (st0, radius, step_fn)."""
    rep = {}
    for name, ratio, lying in (("YcbTennisBall", 5.0 / 7.0, False), ("YcbTomatoSoupCan", 2.0 / 3.0, True)):
        st0, r, step_fn = make_step(name)
        s = np.array(st0, np.float64).copy()
        s[:, 25:28] = [0.0, v0, 0.0]
        s[:, 28:31] = 0.0
        if lying:                                             # axis along world x, resting on the table
            s[:, 12:16] = [0.0, np.sqrt(0.5), 0.0, np.sqrt(0.5)]
            s[:, 11] = 0.625 + r
        onset = None
        for k in range(120):
            s = np.asarray(step_fn(s), np.float64)
            v, w = s[0, 26], s[0, 28]
            if abs(v + w * r) < 2e-4 * v0:                   # contact-point velocity of a body rolling along +y
                onset = (k, v / v0)
                break
        assert onset is not None, name
        rep[name] = {"steps_to_rolling": onset[0], "v_over_v0": float(onset[1]), "analytic": ratio}
        assert -0.035 * ratio < onset[1] - ratio < 0.005 * ratio, (name, onset, ratio)
    return rep


def check_free_fall_kat(step_fn, st0, params, lift=0.12, steps=30):
    """Analytic KAT: the cube released `lift` above its rest height falls under gravity and Bullet's velocity damping exactly as the step's
    discretisation says -- v <- v + dt (-g - kl (1 + |v|) v), z <- z + dt v -- until it comes within the contact margin of the table."""
    g, kl, dt = params["g"], params["kl"], params["dt"]
    s = np.array(st0, np.float64).copy()
    s[:, 11] += lift
    s[:, 25:31] = 0.0
    z, v, worst = float(s[0, 11]), 0.0, 0.0
    for k in range(steps):
        s = np.asarray(step_fn(s), np.float64)
        v = v + dt * (-g - kl * (1.0 + abs(v)) * v)
        z = z + dt * v
        worst = max(worst, abs(s[0, 11] - z), abs(s[0, 27] - v) * dt)
    assert z > st0[0, 11] + 0.02, "the reference run reached the table: shorten it"
    assert worst < 2e-6, worst
    assert np.abs(s[0, 9:11] - st0[0, 9:11]).max() < 1e-7 and np.abs(s[0, 12:16] - st0[0, 12:16]).max() < 1e-6      # straight down, no spin
    return {"steps": steps, "fall_m": float(st0[0, 11] + lift - s[0, 11]), "max_abs_error_m": worst}


def check_finger_force_kat(lib, n=1):
    """Analytic KAT for the robot-object contact rows and the force-limited motors: in the closed grasp of the reference's Panda demo
    (helloworld_panda.py: fingers commanded shut with force 10 N on a rigid object) each finger's motor sits at its force bound, so the
    normal forces of the finger's contact points must add up to exactly that bound -- static equilibrium of the prismatic finger joint,
    whose axis is horizontal with the hand pointing down.  (Two collision spheres per finger touch the object: 2 x 5.000 N.)"""
    from pybullet_robot_envs import _client
    from pybullet_robot_envs.envs.panda_envs.panda_env import pandaEnv
    cid = _client.connect(n, lib=lib)
    robot = pandaEnv(cid, use_IK=1)
    run_panda_demo(robot, upto=3)
    robot.step_simulation(40)
    eng = robot._robot_level()
    tail = eng.observe()[:, -7:].astype(np.float64)        # mean normal force finger 1 / 2, -, -, -, fingers in contact, contact points
    assert (tail[:, 5] == 2).all() and (tail[:, 6] % 2 == 0).all(), tail
    per_finger = tail[:, 6:7] / 2.0
    total = tail[:, :2] * per_finger
    _client.disconnect(cid)
    assert np.abs(total - 10.0).max() < 5e-3, total
    return {"contact_points": tail[0, 6], "normal_force_per_finger_N": total[0].tolist()}


def check_pair_split_is_bit_identical(Engine, lib, table, panda, setenv, n=256, steps=40, use_ik=0, phys=None, task=1):
    """The pair mapping of the simple class (csrc/pbre_capi.hip: k_fast_pair -- the robot's half of the step on one wave, the object's
    half on a second one, the object's new pose handed over in LDS; Fast::step_t<false, 1 / 2>) against the one-lane-per-env step
    (k_fast, ROLE 0): a full reset through each (201 settle launches in each mapping), contact-rich states among the envs so that the
    complex-env kernel runs beside it, `steps` steps with auto-reset and a short episode, per-env object parameters -- rows, states and
    classes bit for bit.  `setenv(name, value)` sets an environment variable for the engines created after it (the mapping is read at
    pbre_create: PBRE_PAIR=1 always, 0 never, default by batch size)."""
    kw = dict(task=task, num_envs=n, obj_pose_rnd_std=0.05, tg_pose_rnd_std=0.2, lib=lib, flags=2, max_steps=25, use_ik=use_ik)
    if phys:
        kw["phys"] = phys
    setenv("PBRE_PAIR", "1")
    a = Engine(table, **kw)
    setenv("PBRE_PAIR", "0")
    b = Engine(table, **kw)
    oa, ob = a.reset(), b.reset()
    assert np.array_equal(oa, ob) and np.array_equal(a.get_state(), b.get_state()), "reset through the pair mapping differs"
    st = a.get_state()
    if phys is None:
        ora = orc.Oracle(table, task=1)
        ora.task.obj_pose_rnd_std, ora.task.tg_pose_rnd_std = 0.05, 0.2
        base, _ = ora.batch_reset(1)
        S = contact_states(ora, panda, base[0], np.random.default_rng(1), 6, 6).astype(np.float32)
        st[:len(S), :S.shape[1]] = S
    rng = np.random.default_rng(21)
    st[:, 28:31] += rng.uniform(-0.5, 0.5, (n, 3)).astype(np.float32) * (rng.random((n, 1)) < 0.3)      # some objects spinning / sliding
    st[:, 25:27] += rng.uniform(-0.3, 0.3, (n, 2)).astype(np.float32) * (rng.random((n, 1)) < 0.3)
    a.set_state(st); b.set_state(st)
    if task >= 1 and phys is None:
        m = rng.uniform(0.05, 0.3, n).astype(np.float32); mu = rng.uniform(0.3, 1.2, n).astype(np.float32)
        for e in (a, b):
            e.set_physics_per_env(obj_mass=m, obj_mu=mu)
    for k in range(steps):
        act = rng.uniform(-1, 1, (n, a.act_dim)).astype(np.float32)
        ra, rb = a.step(act), b.step(act)
        for x, y in zip(ra, rb):
            assert np.array_equal(x, y), "step %d: rows differ between the pair mapping and the one-lane step" % k
    assert np.array_equal(a.get_state(), b.get_state())
    ia, ib = a.kernel_info(), b.kernel_info()
    assert ia[10] > 0 and ib[10] == 0, (ia, ib)
    return ia, ib


def check_nan_guard(Engine, lib, table, panda, n=64, flags_extra=0, use_ik=0):
    """NaN / Inf guard (pbre_kernel_info[12]): non-finite entries injected into the state of a few envs -- a joint
    angle, a joint velocity (Inf), the object's position, the object's angular velocity, and a joint velocity of an env with robot
    contacts (the complex-env kernel's path) -- are counted, returned as reward 0 / done 1, and with PBRE_F_AUTO_RESET the envs restart
    from the settled snapshot in the same step (finite state, next episode); every other env's row and state are bit for bit those of
    an engine that never saw the NaNs.  Without auto-reset the env keeps its non-finite state and is counted again."""
    kw = dict(task=1, num_envs=n, obj_pose_rnd_std=0.05, tg_pose_rnd_std=0.2, lib=lib, use_ik=use_ik)
    ora = orc.Oracle(table, task=1)
    ora.task.obj_pose_rnd_std, ora.task.tg_pose_rnd_std = 0.05, 0.2
    base, _ = ora.batch_reset(1)
    S = scenarios.table_contact_states(ora, panda["model"], panda["spheres"], base[0], 4, np.random.default_rng(1)).astype(np.float32)      # 4 envs with robot-table contacts
    rep = {}
    for auto in (True, False):
        a = Engine(table, flags=(2 if auto else 0) | flags_extra, **kw)
        b = Engine(table, flags=(2 if auto else 0) | flags_extra, **kw)
        a.reset(); b.reset()
        st = a.get_state()
        st[:len(S), :S.shape[1]] = S
        b.set_state(st)
        bad = [1, 9, 17, 23, 40]
        sa = st.copy()
        sa[9, 2] = np.nan             # a joint angle
        sa[17, 16 + 4] = np.inf       # a joint velocity
        sa[23, 10] = np.nan           # the object's position
        sa[40, 29] = -np.inf          # the object's angular velocity
        sa[1, 16 + 1] = np.nan        # a joint velocity of a complex env (robot-table contact: the row kernel's path)
        a.set_state(sa)
        c0 = a.kernel_info()[12]
        assert b.kernel_info()[12] == 0
        rng = np.random.default_rng(5)
        act = rng.uniform(-1, 1, (n, a.act_dim)).astype(np.float32)
        (oa, ra, da), (ob, rb, db) = a.step(act), b.step(act)
        ok = np.ones(n, bool); ok[bad] = False
        assert a.kernel_info()[12] - c0 == len(bad), (a.kernel_info()[12], c0)
        assert np.all(da[bad] == 1) and np.all(ra[bad] == 0)
        assert np.array_equal(oa[ok], ob[ok]) and np.array_equal(ra[ok], rb[ok]) and np.array_equal(da[ok], db[ok]), "a healthy env's row changed"
        s1, s1b = a.get_state(), b.get_state()
        assert np.array_equal(s1[ok], s1b[ok]), "a healthy env's state changed"
        if auto:
            assert np.isfinite(s1).all() and np.isfinite(oa).all(), "restarted envs must be finite"
            assert np.all(s1[bad, 37] == st[bad, 37] + 1), "restarted envs are in their next episode"
            assert np.all(s1[bad, 35] == 0)
            a.step(act)
            assert a.kernel_info()[12] - c0 == len(bad)         # no env is bad any more
        else:
            assert not np.isfinite(s1[bad]).all(axis=1).any(), "without auto-reset a non-finite env stays non-finite"
            a.step(act)
            assert a.kernel_info()[12] - c0 == 2 * len(bad)     # ... and is counted again
        rep["auto_reset" if auto else "count_only"] = int(a.kernel_info()[12] - c0)
        a.close(); b.close()
    return rep


def check_icub_nan_guard(Engine, lib, n=32, use_ik=0):
    """NaN / Inf guard on the iCub engines (the lane-group kernel's Core::observe, or the pipeline's kw_dyn -> kw_fin / Lane::finish,
    whichever PBRE_ICUB_LANE selects): non-finite joint angle / joint velocity / object position in three envs -- counted, reward 0,
    done 1, restarted under PBRE_F_AUTO_RESET; the other envs bit for bit those of an engine that never saw them."""
    mk = lambda: make_icub_pair(Engine, lib, n, 1, "l", use_ik, 0, obj_std=0.05, tg_std=0.2, flags=2)[0]
    a, b = mk(), mk()
    a.reset(); b.reset()
    st = a.get_state()
    nd, vo = a.ndof, a.v_off
    bad = [1, n // 2, n - 2]
    sa = st.copy()
    sa[bad[0], 5] = np.nan; sa[bad[1], vo + 2] = np.inf; sa[bad[2], nd + 1] = np.nan
    a.set_state(sa); b.set_state(st)
    c0 = a.kernel_info()[12]
    act = np.random.default_rng(5).uniform(-1, 1, (n, a.act_dim)).astype(np.float32)
    (oa, ra, da), (ob, rb, db) = a.step(act), b.step(act)
    ok = np.ones(n, bool); ok[bad] = False
    assert a.kernel_info()[12] - c0 == len(bad), (a.kernel_info(), c0)
    assert np.all(da[bad] == 1) and np.all(ra[bad] == 0)
    assert np.array_equal(oa[ok], ob[ok]) and np.array_equal(ra[ok], rb[ok]) and np.array_equal(da[ok], db[ok])
    s1 = a.get_state()
    assert np.array_equal(s1[ok], b.get_state()[ok])
    assert np.isfinite(s1).all() and np.isfinite(oa).all()
    xo = a.x_off
    assert np.all(s1[bad, xo + 5] == st[bad, xo + 5] + 1)
    a.step(act)
    assert a.kernel_info()[12] - c0 == len(bad)
    a.close(); b.close()


def check_four_robot_object_slots(Engine, lib, table, panda, flags=0, n=24, seed=31):
    """SURVEY a6 ("<= 4 cube-robot points"): the cube pinched between the fingers -- both spheres of both fingers on it, in a quarter of the
    states the palm sphere as a fifth candidate -- one step against the oracle with the same four slots, per quantity at TOL_CONTACT.
    Every state has >= 3 robot-object contacts in the oracle (the round-3 engine kept two)."""
    ora = orc.Oracle(table, task=1)
    ora.task.obj_pose_rnd_std, ora.task.tg_pose_rnd_std = 0.05, 0.2
    base, _ = ora.batch_reset(1)
    rng = np.random.default_rng(seed)
    S = scenarios.multi_sphere_object_states(ora, panda["model"], panda["spheres"], base[0], n, rng, want=3)
    assert len(S) == n
    counts = []
    for s in S:
        _, info = ora.sim_step(s, s[:9].copy(), np.full(9, 0.1), np.full(9, 1.0))
        counts.append(sum(1 for c in range(info.ncontacts) if info.type[c] == 1))
    assert min(counts) >= 3 and max(counts) == 4, counts
    eng, ora = make_pair(Engine, lib, table, len(S), flags=flags)
    ora32 = orc.Oracle(table, f32=True, task=1)
    ora32.task.obj_pose_rnd_std, ora32.task.tg_pose_rnd_std = 0.05, 0.2
    rep = check_single_steps(eng, ora, S, rng, steps=1, tol=TOL_CONTACT, skip_ambiguous=True, max_skip=0.3, ora32=ora32)
    rep["robot_object_contacts_per_state"] = counts
    return rep


# ---- pbre_physics.solver_residual_threshold (PyBullet's solverResidualThreshold; Bullet's exit test of the sweep loop) ----------------
# Engine and oracle run the same test on the same quantity -- the sweep's largest squared velocity-level row change against the threshold --
# in fp32 and fp64.  Where both leave the loop after the same sweep the results are held to the usual bounds (TOL / TOL_CONTACT).  Where
# the residual of a sweep lies within rounding of the threshold the two may leave one sweep apart; the results then differ by what that one
# sweep still changes, at most sqrt(threshold) = 3.2e-4 rad/s in the worst row of the env: those env-steps are counted, their fraction is
# bounded, and they are held to TOL_RT_FLIP (one sweep's worth, not a parity bound).
TOL_RT_FLIP = dict(TOL_CONTACT, q=5e-6, qd=1.2e-3, obj_v=4e-4, obj_w=4e-3, obs_q=5e-6, obs_ee_pos=5e-6, obs_ee_eul=1e-5, obs_ee_vel=2e-2, obs_rel_pos=8e-6,
                   obs_rel_eul=2e-5, obs_obj_pos=2e-6, obs_obj_eul=1e-5, obj_pos=2e-6, reward=8e-6)


def check_residual_threshold(Engine, lib, table, states=None, n=48, steps=3, thr=1e-7, flags=0, tol=None, seed=41, max_flip=0.05, report=None,
                             skip_ambiguous=False, max_skip=0.15, expect_early=True, solver_iters=None, **over):
    """One step each from identical fp32 states with the threshold on in engine and oracle.  Asserts: the engine's per-env sweep counts
    (pbre_get_sweeps) equal the oracle's except for a bounded fraction of one-sweep flips; equal-count env-steps within `tol`; flips within
    TOL_RT_FLIP; the test actually fires (some env leaves before solver_iters) and changes the result against a full solve.
    solver_iters: the sweep count the engine and the oracle are switched to AFTER the reset (which runs at the default count).
    expect_early=None: the firing assertions hold where the ORACLE's sweep counts say that an env left early (never the engine's)."""
    rng = np.random.default_rng(seed)
    if states is None:
        eng, ora = make_pair(Engine, lib, table, n, flags=flags, **over)
        if over.get("use_ik"):
            eng.reset(); st, _ = ora.batch_reset(n)         # (IK control: the reset's own bounds are check_ik_mode's)
        else:
            st = check_reset(eng, ora, n)                   # threshold 0: the usual reset, the usual bounds
    else:
        st = np.asarray(states, np.float64)
        n = st.shape[0]
        eng, ora = make_pair(Engine, lib, table, n, flags=flags, **over)
    if solver_iters is not None:
        set_solver_iters(eng, solver_iters, ora)
    with_thr = lambda e: e.set_physics(solver_residual_threshold=thr)
    try:
        eng.get_sweeps()
        raise AssertionError("pbre_get_sweeps must refuse while the threshold is 0")
    except RuntimeError:
        pass
    iters = int(ora.params.solver_iters)
    rep = report if report is not None else {}
    rep.update({"envs": n, "steps": steps, "flips": 0, "compared": 0, "early": 0, "skipped_ambiguous": 0})
    worst, worst_flip = {}, {}
    tt = TOL if tol is None else tol
    for k in range(steps):
        a = rng.uniform(-1, 1, (n, eng.act_dim)).astype(np.float32)
        s32 = st.astype(np.float32)
        # the full solve of the same step (threshold 0), for the "it changes something" assertion
        eng.set_physics(solver_residual_threshold=0.0)
        eng.set_state(s32); eng.step(a); s_full = eng.get_state()
        with_thr(eng); ora.params.solver_residual_threshold = thr
        try:
            eng.set_state(s32)
            ob, rw, dn = eng.step(a)
            se = eng.get_state()
            sw = eng.get_sweeps()
            so, out, used, to7 = ora.batch_step_sweeps(s32.astype(np.float64), a)
            ok = np.ones(n, bool)
            if skip_ambiguous:
                ok = ~ambiguous_envs(ora, s32.astype(np.float64), a)
        finally:
            ora.params.solver_residual_threshold = 0.0
        rep["skipped_ambiguous"] += int((~ok).sum())
        assert (~ok).mean() <= max_skip, "threshold-ambiguous contact sets: %d of %d skipped" % ((~ok).sum(), n)
        assert sw.min() >= 1 and sw.max() <= iters
        same = (sw == used) & ok
        flip = (sw != used) & ok
        rep["flips"] += int(flip.sum()); rep["compared"] += int(same.sum()); rep["early"] += int((used < iters).sum())
        rep.setdefault("max_sweep_gap", 0)
        if flip.any():
            rep["max_sweep_gap"] = max(rep["max_sweep_gap"], int(np.abs(sw[flip].astype(int) - used[flip]).max()))
        dflip = (dn != out[:, -1]) & ok
        assert dflip.sum() <= max(1, n // 50), "done flags differ in %d of %d envs" % (dflip.sum(), n)
        if same.any():
            merge_worst(worst, panda_quantities(se[same], so[same], ob[same], out[same]))
            k2 = same & ~dflip
            if k2.any():
                merge_worst(worst, {"reward": rel(rw[k2], out[k2, -2]).max()})
        if flip.any():
            merge_worst(worst_flip, panda_quantities(se[flip], so[flip], ob[flip], out[flip]))
        # an env that left the loop early is NOT where the full solve ends (else the option would be a no-op)
        early = used < iters - 20
        if early.any():
            rep["max_effect_qd"] = max(rep.get("max_effect_qd", 0.0), float(np.abs(se[early, 16:25] - s_full[early, 16:25]).max()))
        st = so
    eng.set_physics(solver_residual_threshold=0.0)
    rep["worst"], rep["worst_flip"] = worst, worst_flip
    total = max(1, rep["flips"] + rep["compared"])
    assert rep["flips"] <= max(1, int(max_flip * total)), "exit sweeps differ in %d of %d env-steps (bound %.0f %%)" % (rep["flips"], total, 100 * max_flip)
    assert rep["max_sweep_gap"] <= 2, "engine and oracle leave the loop %d sweeps apart" % rep["max_sweep_gap"]
    if expect_early:
        assert rep["early"] > 0, "the residual test never fired: nothing tested"
        assert rep.get("max_effect_qd", 0.0) > 1e-6, "leaving the loop early changed nothing"
    elif expect_early is None and "max_effect_qd" in rep:       # (the oracle left the loop more than 20 sweeps early in some env)
        assert rep["max_effect_qd"] > 1e-6, "leaving the loop early changed nothing"
    assert_within(worst, tt, "(residual threshold %g: %d env-steps with equal sweep counts, %d flips, %d ambiguous skipped)" % (thr, rep["compared"], rep["flips"], rep["skipped_ambiguous"]))
    assert_within(worst_flip, TOL_RT_FLIP, "(residual threshold %g: the %d env-steps that left the loop a sweep apart)" % (thr, rep["flips"]))
    return rep


def check_residual_threshold_moving_cubes(Engine, lib, table, n=32, seed=43):
    """Residual exit, round 6: a state whose cube MOVES (sliding / spinning on the table, no robot contact) is a complex-class state while the
    threshold is on (Fast::rt_class: the closed form of the exit sweep needs a cube at rest; one such lane sent its whole k_fast wave onto the
    explicit rows) -- stepped by the row kernel's explicit rows -- and a simple one with the threshold off.  Checks the class counts
    (pbre_kernel_info[3..5]) and, through check_residual_threshold, the step itself against the oracle."""
    rng = np.random.default_rng(seed)
    eng, ora = make_pair(Engine, lib, table, n)
    st = check_reset(eng, ora, n)
    X = 25                                    # object twist: st[25..30]
    moving = np.zeros(n, bool); moving[1::3] = True
    S = st.copy()
    k = int(moving.sum())
    ang, spd = rng.uniform(0, 2 * np.pi, k), rng.uniform(0.05, 0.08, k)   # sliding at 5..8 cm/s (friction takes 2 cm/s per step: none stops within the
    S[moving, X], S[moving, X + 1] = spd * np.cos(ang), spd * np.sin(ang)  # step the class counts are read after)
    S[moving, X + 5] = rng.uniform(-0.6, 0.6, k)                          # ... and spinning about the vertical
    a = np.zeros((n, eng.act_dim), np.float32)
    s32 = S.astype(np.float32)
    def one_step():
        """envs the simple-class kernel / the complex-class kernels stepped in one step (the HIP library reports the most recent step, the CPU
        emulation running sums)"""
        b = eng.kernel_info()
        eng.step(a)
        i = eng.kernel_info()
        if i[3] + i[4] + i[5] != n:
            i = [x - y for x, y in zip(i, b)]
        return i[3], i[4] + i[5]
    eng.set_state(s32)
    assert one_step() == (n, 0), "threshold off: a moving cube without contact is a simple-class state"
    eng.set_physics(solver_residual_threshold=1e-7)
    try:
        eng.set_state(s32)
        got = one_step()
        assert got == (n - k, k), "threshold on: the %d moving cubes are complex-class states (%r)" % (k, got)
        # a cube that has come to rest is a simple-class state again: 400 hold steps (friction stops an 8 cm/s slide within ~0.1 s)
        for _ in range(400):
            eng.step(a)
        got = one_step()
        assert got == (n, 0), "the cubes came to rest, every env is a simple-class one again (%r)" % (got,)
    finally:
        eng.set_physics(solver_residual_threshold=0.0)
    return check_residual_threshold(Engine, lib, table, states=S, steps=2, tol=TOL_CONTACT, expect_early=True, seed=seed)


TOL_RT_FLIP_GROUP = {"q": 5e-6, "qd": 1.2e-3, "obj_pos": 2e-6, "obj_quat": 3e-6, "obj_v": 5e-3, "obj_w": 4e-3,
                     "obs_ee_pos": 5e-6, "obs_ee_eul": 1e-5, "obs_ee_vel": 8e-4, "obs_rest": 2e-5}


def check_group_residual_threshold(eng, ora, st, rng, tol, steps=3, thr=1e-7, max_flip=0.1, report=None, tail=0, context=""):
    """The lane-group engines (iCub, iCub with hands, robot-level Panda: Core::step<RT>) with pbre_physics.solver_residual_threshold on,
    one step each from identical fp32 states against the oracle with the same threshold: equal per-env sweep counts except for a bounded
    fraction of one-sweep flips (TOL_RT_FLIP_GROUP), everything else within `tol`."""
    n = st.shape[0]
    iters = int(ora.params.solver_iters)
    rep = report if report is not None else {}
    rep.update({"flips": 0, "compared": 0, "early": 0, "max_sweep_gap": 0})
    worst, worst_flip = {}, {}
    eng.set_physics(solver_residual_threshold=thr); ora.params.solver_residual_threshold = thr
    try:
        for k in range(steps):
            a = rng.uniform(-1, 1, (n, eng.act_dim)).astype(np.float32)
            s32 = st.astype(np.float32)
            eng.set_state(s32)
            ob, rw, dn = eng.step(a)
            se = eng.get_state(); sw = eng.get_sweeps()
            so, out, used, to7 = ora.batch_step_sweeps(s32.astype(np.float64), a)
            same, flip = sw == used, sw != used
            rep["flips"] += int(flip.sum()); rep["compared"] += int(same.sum()); rep["early"] += int((used < iters).sum())
            if flip.any():
                rep["max_sweep_gap"] = max(rep["max_sweep_gap"], int(np.abs(sw[flip].astype(int) - used[flip]).max()))
                merge_worst(worst_flip, group_quantities(eng, se[flip], so[flip], ob[flip], out[flip], tail=tail))
            if same.any():
                merge_worst(worst, group_quantities(eng, se[same], so[same], ob[same], out[same], tail=tail))
            st = so
    finally:
        eng.set_physics(solver_residual_threshold=0.0); ora.params.solver_residual_threshold = 0.0
    rep["worst"], rep["worst_flip"] = worst, worst_flip
    total = max(1, rep["flips"] + rep["compared"])
    assert rep["early"] > 0, "the residual test never fired: nothing tested " + context
    assert rep["flips"] <= max(1, int(max_flip * total)), "exit sweeps differ in %d of %d env-steps %s" % (rep["flips"], total, context)
    assert rep["max_sweep_gap"] <= 2
    assert_within(worst, tol, "(residual threshold %g, %d env-steps with equal sweep counts, %d flips) %s" % (thr, rep["compared"], rep["flips"], context))
    assert_within(worst_flip, TOL_RT_FLIP_GROUP, "(residual threshold %g: one-sweep flips) %s" % (thr, context))
    return rep


def check_hands_residual_threshold(Engine, lib, n=1, steps=2, thr=1e-7, seed=9):
    """iCub with hands (Core::step<RT> on the 128-virtual-lane shape, rows in LDS): joint-control steps with the threshold on, against the
    oracle's hands_step with the same threshold -- equal sweep counts (one-sweep flips bounded), results within TOL_HANDS."""
    eng, ora, info = make_hands_pair(Engine, lib, n, "r", 0)
    eng.reset()
    st, mrec, _ = ora.hands_reset(n)
    rng = np.random.default_rng(seed)
    home = np.asarray(info["home"])[info["controlled"]]
    iters = int(ora.params.solver_iters)
    worst, flips, early, same_n = {}, 0, 0, 0
    eng.set_physics(solver_residual_threshold=thr); ora.params.solver_residual_threshold = thr
    try:
        for k in range(steps):
            a = (home[None, :] + rng.uniform(-0.2, 0.2, (n, len(home)))).astype(np.float32)
            s32 = st.astype(np.float32)
            eng.set_state(s32)
            ob, rw, dn = eng.step(a)
            so, mrec, out = ora.hands_step(s32.astype(np.float64), mrec, a)
            se, sw, used = eng.get_state(), eng.get_sweeps(), ora.last_sweeps
            same = sw == used
            flips += int((~same).sum()); same_n += int(same.sum()); early += int((used < iters).sum())
            assert np.abs(sw.astype(int) - used).max() <= 2
            if same.any():
                merge_worst(worst, group_quantities(eng, se[same], so[same], ob[same], out[same], tail=7))
            if (~same).any():
                assert_within(group_quantities(eng, se[~same], so[~same], ob[~same], out[~same], tail=7), TOL_RT_FLIP_GROUP, "(hands, one-sweep flip)")
            st = so
    finally:
        eng.set_physics(solver_residual_threshold=0.0); ora.params.solver_residual_threshold = 0.0
    assert early > 0, "the residual test never fired"
    assert flips <= max(1, (flips + same_n) // 4)
    assert_within(worst, TOL_HANDS, "(hands, residual threshold %g, %d env-steps, %d flips)" % (thr, same_n, flips))
    return eng


def object_block_states(base, rng, n):
    """States of the simple class that exercise every branch of the object block's closed form (Fast::obj_closed): cubes at rest, sliding
    (friction on / near the cone), spinning, dropped from a few mm, tilted onto an edge, tumbling, pressed into the table.  base: one settled
    state record."""
    st = np.tile(np.asarray(base, np.float32), (n, 1))
    kind = rng.integers(0, 7, n)
    for e in range(n):
        k = kind[e]
        if k == 1:
            v, a = 10 ** rng.uniform(-5, -0.3), rng.uniform(0, 2 * np.pi)
            st[e, 25], st[e, 26] = v * np.cos(a), v * np.sin(a)
        elif k == 2:
            st[e, 30] = 10 ** rng.uniform(-4, 1) * rng.choice([-1, 1])
        elif k == 3:
            st[e, 11] += 10 ** rng.uniform(-5, -1.5)
        elif k == 4:
            th, ax = 10 ** rng.uniform(-4, -0.3), rng.uniform(0, 2 * np.pi)
            st[e, 12:16] = [np.sin(th / 2) * np.cos(ax), np.sin(th / 2) * np.sin(ax), 0.0, np.cos(th / 2)]
            st[e, 11] += 0.04 * np.sin(th)
        elif k == 5:
            st[e, 28:30] = rng.normal(0, 1, 2) * 10 ** rng.uniform(-3, 0.5)
        elif k == 6:
            st[e, 27] = -10 ** rng.uniform(-4, 0)
    return st, kind


def check_closed_form_object_rows(Engine, lib, table, n=256, steps=12, seed=17, stats=None):
    """The simple class applies the tail of its sweeps over a resting cube's object-table rows in closed form where a per-env bound proves
    that no clamp binds (Fast::obj_closed); PBRE_F_SEQ_OBJECT runs Bullet's sequential rows throughout.  Same states, one step each:
    the robot (which these rows do not touch) bit for bit, the object's twist and pose within a quarter of the single-step bounds
    against the oracle -- for cubes at rest (closed form taken) and for sliding / tilted / tumbling ones (explicit rows: bit for bit, then
    closed form again once they have come to rest).  stats(): optional callable returning (failed, passed) lane counts (emulation)."""
    rng = np.random.default_rng(seed)
    kw = dict(task=1, num_envs=n, obj_pose_rnd_std=0.05, tg_pose_rnd_std=0.2, lib=lib)
    from pybullet_robot_envs import _capi
    c = Engine(table, **kw)
    s = Engine(table, flags=_capi.F_SEQ_OBJECT, **kw)
    c.reset()
    st, kind = object_block_states(c.get_state()[0], rng, n)
    c.set_state(st)
    if stats:
        stats(True)
    worst, exact = {}, 0
    for k in range(steps):
        a = (rng.uniform(-1, 1, (n, 7)) * 0.3).astype(np.float32)      # (small moves: the arm stays away from the cube, every env in the simple class)
        s.set_state(c.get_state())
        (obc, rwc, dnc), (obs_, rws, dns) = c.step(a), s.step(a)
        sc, ss = c.get_state(), s.get_state()
        assert c.kernel_info()[5] == 0, "an env left the simple class"
        assert np.array_equal(sc[:, :9], ss[:, :9]) and np.array_equal(sc[:, 16:25], ss[:, 16:25]) and np.array_equal(dnc, dns)
        exact += int((sc[:, 25:31] == ss[:, 25:31]).all(axis=1).sum())
        out_s = np.concatenate([obs_, rws[:, None], dns[:, None]], 1).astype(np.float64)
        merge_worst(worst, panda_quantities(sc, ss.astype(np.float64), obc, out_s, rwc))
    # (a quarter of the single-step bounds; half of them for the object's twist, which the violent members of the family -- cubes pressed
    # into the table at 1 m/s, dropped from 3 cm -- carry at three orders of magnitude above a resting cube's: measured on MI355X over
    # 4096 envs x 12 steps obj_w 1.3e-6 rad/s, on the emulation 1.1e-6)
    assert_within(worst, dict((kk, (0.5 if kk in ("obj_w", "obj_v") else 0.25) * v) for kk, v in TOL.items()), "(closed-form object rows against the sequential rows)")
    rep = {"worst": worst, "bitwise_equal_env_steps": exact, "env_steps": n * steps}
    if stats:
        failed, passed = stats(False)
        rep.update({"lanes_failed": failed, "lanes_passed": passed})
        assert passed > n * steps // 2 and failed > n // 8, rep       # both branches were taken
    return rep


# iCub with the soft-pinned FLOATING base (model/table.py: float_base -- six virtual joints held by the constraint's equivalent motors, legs
# lumped into the base body; 26 DoF on the 64-lane shape): one step from identical states; measured on the emulation q 1.5e-7, qd 1.3e-5
TOL_ICUB_FLOAT = dict(TOL_ICUB, q=1.5e-6, qd=2e-4, obs_ee_pos=1.5e-6, obs_ee_vel=2e-4)


def check_icub_base_force_bound(Engine, lib, n=2, steps=3, seed=10, base_force=200.0):
    """The base constraint's force bound (icub_env.py:95-101: createConstraint leaves maxForce at PyBullet's default, 500 N; VERDICT r5 "missing"
    item 4): the rows of the floating base's constraint are bounded by `base_force` N.  With 500 N the robot's weight (324 N) stays inside the
    bound -- check_icub_floating_base; HERE the bound is set BELOW the weight (a model parameter: table.float_base(base_force=...)), so the vertical
    row saturates and the robot sinks: single steps from identical states, engine against oracle within TOL_ICUB_FLOAT, and the base's
    vertical velocity after one step from rest is the free-fall deficit -(g - F / M) dt within 5 %."""
    from pybullet_robot_envs import _capi
    from pybullet_robot_envs.model.table import icub_table
    ora5, _, _ = orc.icub_oracle("l", task=1, use_ik=0, control_orientation=0, floating_base=True)
    ora, tbl, info = orc.icub_oracle("l", task=1, use_ik=0, control_orientation=0, floating_base=True, base_force=base_force)
    for o in (ora5, ora):
        o.task.obj_pose_rnd_std = 0.05; o.task.tg_pose_rnd_std = 0.2
    ov = icub_overrides(info, "l", 0, 0, 1)
    eng = Engine(tbl, task=1, num_envs=n, lib=lib, robot=_capi.ROBOT_ICUB, obj_pose_rnd_std=0.05, tg_pose_rnd_std=0.2, **ov)
    assert eng.ndof == 26

    def to_engine(a):            # (the engine keeps the object behind the 32 DoF lanes of its kernel shape, the oracle right behind the 26 joints)
        a = np.asarray(a, np.float32); b = np.zeros_like(a); vo = eng.v_off
        b[:, :26] = a[:, :26]; b[:, 32:39] = a[:, 26:33]
        b[:, vo:vo + 26] = a[:, vo:vo + 26]; b[:, vo + 32:vo + 38] = a[:, vo + 26:vo + 32]
        b[:, eng.x_off:] = a[:, eng.x_off:]
        return b

    def to_oracle(a):
        a = np.asarray(a); b = np.zeros_like(a); vo = eng.v_off
        b[:, :26] = a[:, :26]; b[:, 26:33] = a[:, 32:39]
        b[:, vo:vo + 26] = a[:, vo:vo + 26]; b[:, vo + 26:vo + 32] = a[:, vo + 32:vo + 38]
        b[:, eng.x_off:] = a[:, eng.x_off:]
        return b
    st, _ = ora5.batch_reset(n)            # the settled state of the 500 N model: the base at rest, held
    M = float(icub_table("l", floating_base=True)[1]["floating_base"]["lumped_mass"])
    mass_all = M + sum(l["mass"] for l in icub_table("l", floating_base=True)[1]["links"][7:])
    rng = np.random.default_rng(seed)
    worst = {}
    vo = eng.v_off
    for k in range(steps + 1):
        # (step 0 with zero actions -- gentle joint targets: the vertical row carries the weight alone; then random targets, whose reaction
        # forces are of the bound's size themselves)
        a = rng.uniform(-1, 1, (n, eng.act_dim)).astype(np.float32) if k else np.zeros((n, eng.act_dim), np.float32)
        s32 = st.astype(np.float32)
        eng.set_state(to_engine(s32))
        ob, rw, dn = eng.step(a)
        so, out = ora.batch_step(s32.astype(np.float64), a)
        se = to_oracle(eng.get_state())
        if k == 0:
            g = abs(float(ora.params.gravity_z)) if hasattr(ora.params, "gravity_z") else 9.8
            want = -(g - base_force / mass_all) * float(ora.params.dt)
            assert np.all(np.abs(so[:, vo + 2] / want - 1) < 0.05), ("oracle: the base does not sink at the free-fall deficit", so[:, vo + 2], want)
            assert np.all(np.abs(se[:, vo + 2] / want - 1) < 0.05), ("engine: the base does not sink at the free-fall deficit", se[:, vo + 2], want)
        merge_worst(worst, {"q": float(np.abs(se[:, :26] - so[:, :26]).max()), "qd": float(np.abs(se[:, vo:vo + 26] - so[:, vo:vo + 26]).max()),
                            "obs_ee_pos": float(np.abs(ob[:, :3] - out[:, :3]).max())})
        st = so
    assert_within(worst, TOL_ICUB_FLOAT, "(floating-base iCub, base constraint bounded at %g N, %d envs x %d steps)" % (base_force, n, steps))
    return {"worst": worst, "base_vz_after_one_step": float(se[0, vo + 2])}


def check_icub_floating_base(Engine, lib, n=2, steps=3, use_ik=1, seed=9):
    """The fidelity option for the reference's floating base (icub_env.py:95-101: createConstraint(JOINT_FIXED) on a floating multibody):
    (1) engine against oracle on the floating model -- reset and single steps within TOL_ICUB_FLOAT; (2) the option's effect, engine
    against engine: the same actions on the rigidly pinned default model; the base does move (sub-millimetre) and the hand's observation
    shifts by a measurable amount that stays small -- returned for the report."""
    from pybullet_robot_envs import _capi
    ora, tbl, info = orc.icub_oracle("l", task=1, use_ik=use_ik, control_orientation=0, floating_base=True)
    ora.task.obj_pose_rnd_std = 0.05; ora.task.tg_pose_rnd_std = 0.2
    ov = icub_overrides(info, "l", use_ik, 0, 1)
    raw = Engine(tbl, task=1, num_envs=n, lib=lib, robot=_capi.ROBOT_ICUB, obj_pose_rnd_std=0.05, tg_pose_rnd_std=0.2, **ov)
    assert raw.ndof == 26 and raw.obj_off == 32 and raw.state_floats == ora.state_floats and raw.obs_dim == ora.obs_dim and raw.act_dim == ora.task.n_act

    class _View(object):
        """the engine with its state records in the ORACLE's layout (object right behind the 26 joints; the engine keeps it behind the 32
        DoF lanes of its kernel shape, include/pbre.h)"""
        def __init__(self, e):
            self.e = e
        def __getattr__(self, k):
            return getattr(self.e, k)
        def _perm(self, a, to_engine):
            a = np.asarray(a); b = np.zeros_like(a); vo = self.e.v_off
            src, dst = (26, 32) if to_engine else (32, 26)
            b[:, :26] = a[:, :26]; b[:, dst:dst + 7] = a[:, src:src + 7]
            b[:, vo:vo + 26] = a[:, vo:vo + 26]; b[:, vo + dst:vo + dst + 6] = a[:, vo + src:vo + src + 6]
            b[:, self.e.x_off:] = a[:, self.e.x_off:]
            return b
        def get_state(self):
            return self._perm(self.e.get_state(), False)
        def set_state(self, s):
            self.e.set_state(self._perm(np.asarray(s, np.float32), True))
    eng = _View(raw)
    fixed, _, _ = make_icub_pair(Engine, lib, n, task=1, control_arm="l", use_ik=use_ik, obj_std=0.05, tg_std=0.2)
    obs = eng.reset(); obs_f = fixed.reset()
    st_o, obs_o = ora.batch_reset(n)
    st_e = eng.get_state()
    row_o = np.concatenate([obs_o, np.zeros((n, 2))], 1)
    assert_within(group_quantities(eng, st_e, st_o, obs, row_o), dict(TOL_ICUB_RESET, q=3e-6, obs_rest=3e-6), "(floating-base iCub, reset)")
    rep = {"base_sag_after_reset_m": float(np.abs(st_e[:, :3]).max()), "base_tilt_after_reset_rad": float(np.abs(st_e[:, 3:6]).max()),
           "reset_obs_shift_vs_pinned_base": float(np.abs(obs[:, :3] - obs_f[:, :3]).max())}
    rng = np.random.default_rng(seed)
    worst, flips, st = {}, 0, st_o
    for k in range(steps):
        a = rng.uniform(-1, 1, (n, eng.act_dim)).astype(np.float32)
        s32 = st.astype(np.float32)
        eng.set_state(s32)
        ob, rw, dn = eng.step(a)
        so, out = ora.batch_step(s32.astype(np.float64), a)
        se = eng.get_state()
        flip = np.abs(se[:, :26] - so[:, :26]).max(1) > TOL_ICUB_FLOAT["q"] if use_ik else np.zeros(n, bool)
        left = resolve_ik_flips(ora, lambda: ora.batch_step(s32.astype(np.float64), a), flip, se, so, out, 26, TOL_ICUB_FLOAT["q"])
        flips += int(left.sum())
        if (~left).any():
            merge_worst(worst, group_quantities(eng, se[~left], so[~left], ob[~left], out[~left]))
        st = so
    assert flips <= max(1, n * steps // 10)
    assert_within(worst, TOL_ICUB_FLOAT, "(floating-base iCub, %d envs x %d steps)" % (n, steps))
    # (2) the effect: free-running, the same actions on both models
    eng.reset(); fixed.reset()
    d_ee, d_base = 0.0, 0.0
    for k in range(40):
        a = rng.uniform(-1, 1, (n, eng.act_dim)).astype(np.float32)
        (o1, _, _), (o2, _, _) = eng.step(a), fixed.step(a)
        d_ee = max(d_ee, float(np.abs(o1[:, :3] - o2[:, :3]).max()))
        d_base = max(d_base, float(np.abs(eng.get_state()[:, :3]).max()))
    rep.update({"ee_pos_shift_vs_pinned_base_40_steps_m": d_ee, "base_excursion_40_steps_m": d_base, "worst": worst})
    # the base is dynamic (it moves) and the constraint holds it (it moves little).  (Until round 6 the constraint's rows were unbounded: excursion
    # < 5 mm, hand shift < 2 mm.  With the constraint's 500 N on every row the random joint targets' reaction forces DO saturate it: 7 mm / 12 mm.)
    assert 0 < d_base < 2e-2 and d_ee < 3e-2, rep
    return rep
