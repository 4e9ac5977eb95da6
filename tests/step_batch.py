"""One small Panda push batch that takes every path of the lane-per-env step code (csrc/pbre_fast.hpp), stepped the same way by every
caller: the host emulation built with either table layout (test_fast_tables.py), the GPU build against a recorded golden
(test_gpu_fast_tables.py) and the recorder of that golden (tools/make_golden_step_batch.py).

130 envs -- two full waves and a partial one -- start from a full reset; the first envs are overwritten with crafted states: robot-table
contacts, robot-object contacts, the cube pinched between the fingers (three or four spheres on it at once: more candidates than the
tie-break of the candidate list sees otherwise), joints at / beyond a limit.  Some cubes slide or spin, a few envs are three steps from the
end of their episode (snapshot reset at step 3), every env reaches max_steps within the 40 steps."""
import hashlib

import numpy as np

N = 130
STEPS = 40
MAX_STEPS = 25
KW = dict(task=1, obj_pose_rnd_std=0.05, tg_pose_rnd_std=0.2, max_steps=MAX_STEPS)
F_AUTO_RESET = 2
SHORT = [5, 17, 25, 40, 63, 64, 129]      # envs that start three steps from the end of their episode


def crafted_states(panda):
    """The crafted part of the start batch, float32 [k][48] (needs the oracle: CPU)."""
    import orc
    import scenarios
    ora = orc.Oracle(panda["table"], task=1)
    ora.task.obj_pose_rnd_std, ora.task.tg_pose_rnd_std = 0.05, 0.2
    base, _ = ora.batch_reset(1)
    base = base[0]
    rng = np.random.default_rng(8)
    m, sp = panda["model"], panda["spheres"]
    lim = np.repeat(base[None], 4, 0)
    lim[0, 3] = 0.02       # joint 4 above its upper limit 0.0
    lim[1, 5] = -0.12      # joint 6 below its lower limit -0.0873
    lim[2, 7] = 0.045      # finger beyond 0.04
    lim[3, 1] = -1.9       # joint 2 below -1.8326
    S = np.concatenate([scenarios.table_contact_states(ora, m, sp, base, 6, rng),
                        scenarios.object_contact_states(ora, m, sp, base, 6, rng),
                        scenarios.multi_sphere_object_states(ora, m, sp, base, 4, rng, want=3),
                        lim])
    assert len(S) == 20
    return S.astype(np.float32)


def start_state(eng, S):
    """reset() of the whole batch, then the crafted states and the per-env variations; returns the state the steps start from"""
    eng.reset()
    st = eng.get_state()
    st[:len(S), :S.shape[1]] = S
    rng = np.random.default_rng(21)
    n = len(st)
    st[:, 28:31] += rng.uniform(-0.5, 0.5, (n, 3)).astype(np.float32) * (rng.random((n, 1)) < 0.3)      # some cubes spinning / sliding
    st[:, 25:27] += rng.uniform(-0.3, 0.3, (n, 2)).astype(np.float32) * (rng.random((n, 1)) < 0.3)
    st[SHORT, 35] = MAX_STEPS - 2       # done -- and restarted from the snapshot -- by the third step (5, 17: crafted states)
    eng.set_state(st)
    return st


def run(eng, st0=None):
    """40 steps from the start state (set here when given).  Returns per step the [obs | reward | done] rows and the states."""
    if st0 is not None:
        eng.set_state(st0)
    rng = np.random.default_rng(22)
    rows, states = [], []
    for _ in range(STEPS):
        act = rng.uniform(-1, 1, (eng.num_envs, eng.act_dim)).astype(np.float32)
        ob, rw, dn = eng.step(act)
        rows.append(np.concatenate([ob, rw[:, None], dn[:, None]], 1).astype(np.float32))
        states.append(eng.get_state().copy())
    return np.array(rows), np.array(states)


def digest(a):
    return hashlib.sha256(np.ascontiguousarray(a, np.float32).tobytes()).hexdigest()
