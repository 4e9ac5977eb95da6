"""Time per call of the batched inverse-kinematics query (include/pbre_ik.h) beside a step of the same batch.

Panda-push envs (131072 by default) after `--preroll` untimed steps with random actions (auto-reset on: the stationary mix).  The targets
are the current hand pose of every env displaced by one unit action -- +-ik_pos_scale along each axis, +-ik_rot_scale about each Euler
angle, signs drawn per env -- which is what one step of an engine in IK mode asks of its own solver.  Timed: the query position-only and
with the full pose, at the engine's defaults, start values from the state, on torch's current stream into tensors allocated once; device
events around `--launches` enqueues (50), `--repeats` windows (7) after `--warmup` untimed calls: median, min, max of the per-call time.
Beside them, timed the same way in the same run, step_tensor of that engine (joint mode) and of an engine in IK mode, and the histogram
of `iters`.  Prints one JSON line and writes it to --out (default: profiles/r13_ik_query.json)."""
import argparse
import ctypes as C
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "pybullet-robot-envs_amd"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--envs", type=int, default=131072)
    ap.add_argument("--preroll", type=int, default=200)
    ap.add_argument("--launches", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r13_ik_query.json"))
    a = ap.parse_args()
    import torch
    from pybullet_robot_envs import _capi
    from pybullet_robot_envs.envs import pandaPushGymEnv
    from pybullet_robot_envs.envs.panda_envs.panda_env import pandaEnv
    from pybullet_robot_envs.model.table import hand_pose_target
    if not torch.cuda.is_available():
        raise SystemExit("bench_ik: no GPU (there is nothing to measure on a CPU)")
    dev = torch.device("cuda", 0)

    def windows(fn, launches):
        for _ in range(a.warmup):
            fn()
        torch.cuda.synchronize()
        ms = []
        for _ in range(a.repeats):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(launches):
                fn()
            e1.record()
            e1.synchronize()
            ms.append(e0.elapsed_time(e1) / launches)
        return {"median_ms": float(np.median(ms)), "min_ms": float(min(ms)), "max_ms": float(max(ms))}

    def stepped(use_ik):
        env = pandaPushGymEnv(num_envs=a.envs, use_IK=use_ik, obj_pose_rnd_std=0.05, tg_pose_rnd_std=0.2, auto_reset=True)
        env.reset()
        act = torch.empty((a.envs, env._engine.act_dim), device=dev)

        def step():
            act.uniform_(-1.0, 1.0)
            env.step_tensor(act)

        for _ in range(a.preroll):
            step()
        torch.cuda.synchronize()
        return env, step

    n = a.envs
    res = {"metric": "ik_query_ms_per_call", "unit": "ms", "envs": n, "launches_per_window": a.launches, "windows": a.repeats,
           "workload": "Panda push, %d envs after %d untimed steps with random actions (auto-reset); targets: the hand pose displaced by one unit action" % (n, a.preroll)}
    env, step = stepped(0)
    eng = env._engine
    cfg = eng.cfg
    hand = eng.kin_query(links=[int(eng._table[4])], vel=False, jac=False, mass=False, tau=False)["pose"][:, 0].astype(np.float64)
    rng = np.random.default_rng(13)
    sign = rng.choice([-1.0, 1.0], size=(n, 6))
    pose = np.concatenate([hand[:, :3] + cfg.ik_pos_scale * sign[:, :3], pandaEnv._euler_from_quat(hand[:, 3:]) + cfg.ik_rot_scale * sign[:, 3:]], axis=1)
    tp, tq = hand_pose_target(pose, [cfg.ik_link_offset[k] for k in range(3)])
    tp, tq = torch.as_tensor(tp, dtype=torch.float32, device=dev), torch.as_tensor(tq, dtype=torch.float32, device=dev)
    q = torch.empty((n, eng.ndof), dtype=torch.float32, device=dev)
    err = torch.empty((n, 2), dtype=torch.float32, device=dev)
    iters = torch.empty((n,), dtype=torch.int32, device=dev)
    stream = C.c_void_p(_capi.torch_stream(dev))
    res.update(ik_damping=cfg.ik_damping, ik_residual=cfg.ik_residual, ik_max_iters=cfg.ik_max_iters, ik_pos_scale=cfg.ik_pos_scale, ik_rot_scale=cfg.ik_rot_scale)
    for name, quat in (("position_only", None), ("full_pose", tq)):
        o = _capi.IkQuery()
        o.link, o.damping, o.residual, o.max_iters = -1, -1.0, -1.0, -1
        o.target_pos = tp.data_ptr()
        o.target_quat = None if quat is None else quat.data_ptr()
        o.q, o.err, o.iters = q.data_ptr(), err.data_ptr(), iters.data_ptr()
        w = windows(lambda: eng._chk(eng.lib.pbre_ik_query_device(eng._ctx, C.byref(o), stream)), a.launches)
        torch.cuda.synchronize()
        it = iters.cpu().numpy()
        hist = np.bincount(it, minlength=1)
        res[name] = dict(w, envs_per_s=n / (w["median_ms"] * 1e-3), iters_histogram={str(k): int(v) for k, v in enumerate(hist) if v},
                         iters_median=float(np.median(it)), iters_max=int(it.max()), err_pos_max=float(err[:, 0].max()), outputs_finite=bool(torch.isfinite(q).all()))
    res["value"] = res["full_pose"]["median_ms"]
    res["step_tensor_joint_mode"] = dict(windows(step, a.launches), note="includes the uniform_ that draws the actions", dominant_kernel_ms=float(eng.timing()[3]))
    env.close()
    env, step = stepped(1)
    res["step_tensor_ik_mode"] = dict(windows(step, a.launches), note="includes the uniform_ that draws the actions", dominant_kernel_ms=float(env._engine.timing()[3]))
    env.close()
    res["full_pose_over_ik_step"] = res["full_pose"]["median_ms"] / res["step_tensor_ik_mode"]["median_ms"]
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
