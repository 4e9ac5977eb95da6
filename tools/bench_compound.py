"""ms per step of a Panda push batch in its stationary mix with compound objects (include/pbre.h: pbre_set_object_hull) against the
cylinder primitive (lane path) and one 32-vertex hull (general row kernel), at 16384 and 131072 envs.  Protocol of bench.py's headline:
actions and output rows resident in HBM (pbre_step_device), auto-reset, episode clocks de-synchronised (step counters U{0..max_steps-1}),
an untimed pre-roll with a fresh U(-1, 1) draw per step, then the timed steps over a pool of 100 action batches.  Writes
profiles/r07_compound.json (or --out)."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "pybullet-robot-envs_amd"))


def blob(seed, c, r, n=32):
    g = np.random.default_rng(seed)
    d = g.normal(size=(n, 3)); d /= np.linalg.norm(d, axis=1)[:, None]
    return np.asarray(c) + d * r


def objects_to_time():
    from pybullet_robot_envs.model.objects import compound_physics, hull_physics, object_physics
    return {"cylinder": object_physics("YcbTomatoSoupCan", use_mesh=False),
            "hull32": hull_physics(blob(1, (0, 0, 0), [0.04, 0.03, 0.025]), 0.1, 1.0),
            "compound2": compound_physics([blob(k, (0.04 * k - 0.02, 0, 0), [0.02, 0.02, 0.02]) for k in range(2)], 0.1, 1.0),
            "compound4": compound_physics([blob(k, (0.03 * k - 0.045, 0, 0), [0.015, 0.02, 0.02]) for k in range(4)], 0.1, 1.0)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--envs", default="16384,131072")
    ap.add_argument("--steps", type=int, default=100)
    ap.add_argument("--preroll", type=int, default=1000)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r07_compound.json"))
    a = ap.parse_args()
    import torch
    from pybullet_robot_envs import _capi
    from pybullet_robot_envs.model.table import panda_table
    tbl, _ = panda_table()
    dev = torch.device("cuda", 0)
    max_steps = 1000
    res = {"protocol": "stationary mix: %d untimed steps (fresh actions each) after reset with de-synchronised episode clocks, then %d timed "
                       "steps; device-resident actions / outputs, auto-reset" % (a.preroll, a.steps), "ms_per_step": {}}
    for n in [int(x) for x in a.envs.split(",")]:
        for name, ph in objects_to_time().items():
            eng = _capi.Engine(tbl, task=_capi.TASK_PUSH, num_envs=n, obj_pose_rnd_std=0.05, tg_pose_rnd_std=0.2, flags=_capi.F_AUTO_RESET,
                               max_steps=max_steps, phys=ph)
            eng.reset()
            st = eng.get_state()
            st[:, eng.x_off + 3] = np.random.default_rng(4321).integers(0, max_steps, n).astype(np.float32)
            eng.set_state(st)
            op = torch.zeros((n, eng.obs_dim + 2), device=dev)
            sp = _capi.torch_stream(dev)
            fresh = torch.empty((n, 7), device=dev)
            for _ in range(a.preroll):
                fresh.uniform_(-1.0, 1.0)
                eng.step_device(fresh.data_ptr(), op.data_ptr(), sp)
            pool = [torch.rand((n, 7), device=dev) * 2 - 1 for _ in range(100)]
            torch.cuda.synchronize()
            k0 = eng.kernel_info()[7]
            t0 = time.perf_counter()
            for k in range(a.steps):
                eng.step_device(pool[k % len(pool)].data_ptr(), op.data_ptr(), sp)
            torch.cuda.synchronize()
            ms = 1e3 * (time.perf_counter() - t0) / a.steps
            info = eng.kernel_info()
            assert bool(torch.isfinite(op).all())
            res["ms_per_step"]["%s@%d" % (name, n)] = {"ms": round(ms, 4), "fast_envs_last_step": info[3], "general_envs_last_step": info[4],
                                                        "complex_envs_per_step": round((info[7] - k0) / a.steps, 1)}
            print(name, n, "%.4f ms/step" % ms, "fast", info[3], "general", info[4], flush=True)
            eng.close()
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
