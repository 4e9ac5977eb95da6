"""Time per call of the batched kinematics / dynamics query (include/pbre_kin.h) beside a step of the same batch:
  panda   Panda-push envs (131072 by default) after `--preroll` untimed steps with random actions (auto-reset on);
  hands   the iCub with hands used alone (8192 envs by default), joints spread about the home pose, joint velocities ~ N(0, 1).
For each: every output alone (pose + vel of every link count as one, "links") and all together, on torch's current stream into tensors
allocated once: device events around `--launches` enqueues (windows of milliseconds to tens of milliseconds), `--repeats` windows after
`--warmup` untimed calls (median, min, max of the per-call time); the bytes the outputs hold and the fraction of the HBM figure bench.py
uses (8 TB/s) that writing them in that time amounts to -- the column buffers' own traffic is not counted.  The Panda batch's
step_tensor is timed the same way, next to pbre_timing's figure for the step's dominant kernel.
Prints one JSON line and writes it to --out (default: profiles/r11_kin_query.json)."""
import argparse
import ctypes as C
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "pybullet-robot-envs_amd"))
HBM_PEAK_GBS = 8000.0      # bench.py's


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--envs", type=int, default=131072)
    ap.add_argument("--hands-envs", type=int, default=8192)
    ap.add_argument("--preroll", type=int, default=200)
    ap.add_argument("--launches", type=int, default=100)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r11_kin_query.json"))
    a = ap.parse_args()
    import torch
    from pybullet_robot_envs import _capi, _client
    from pybullet_robot_envs.envs import pandaPushGymEnv
    from pybullet_robot_envs.envs.icub_envs.icub_env_with_hands import iCubHandsEnv
    if not torch.cuda.is_available():
        raise SystemExit("bench_kin: no GPU (there is nothing to measure on a CPU)")
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

    def queries(eng):
        """per output set: the timing of pbre_kin_query_device into preallocated tensors"""
        n, nd, nl = eng.num_envs, eng.ndof, int(eng._table[2])
        shapes = dict(pose=(n, nl, 7), vel=(n, nl, 6), jac=(n, 6, nd), mass=(n, nd, nd), tau=(n, nd))
        bufs = {k: torch.empty(s, dtype=torch.float32, device=dev) for k, s in shapes.items()}
        links = np.arange(nl, dtype=np.int32)
        out = {}
        for name, keys in (("links", ("pose", "vel")), ("jac", ("jac",)), ("mass", ("mass",)), ("tau", ("tau",)), ("all", tuple(shapes))):
            o = _capi.KinQuery()
            o.links, o.n_links, o.jac_link = links.ctypes.data, nl, -1
            for k in keys:
                setattr(o, k, bufs[k].data_ptr())
            stream = C.c_void_p(_capi.torch_stream(dev))
            fn = lambda: eng._chk(eng.lib.pbre_kin_query_device(eng._ctx, C.byref(o), stream))
            w = windows(fn, a.launches)
            nbytes = int(sum(bufs[k].numel() * 4 for k in keys))
            gbs = nbytes / (w["median_ms"] * 1e-3) / 1e9
            out[name] = dict(w, output_bytes=nbytes, output_gb_per_s=gbs, frac_of_hbm_peak=gbs / HBM_PEAK_GBS, envs_per_s=n / (w["median_ms"] * 1e-3))
        ok = all(bool(torch.isfinite(b).all()) for b in bufs.values())
        return out, ok

    res = {"metric": "kin_query_ms_per_call", "unit": "ms", "launches_per_window": a.launches, "windows": a.repeats, "hbm_peak_gb_per_s": HBM_PEAK_GBS}
    # ---- Panda push
    n = a.envs
    env = pandaPushGymEnv(num_envs=n, obj_pose_rnd_std=0.05, tg_pose_rnd_std=0.2, auto_reset=True)
    env.reset()
    eng = env._engine
    act = torch.empty((n, eng.act_dim), device=dev)

    def step():
        act.uniform_(-1.0, 1.0)
        env.step_tensor(act)

    for _ in range(a.preroll):
        step()
    torch.cuda.synchronize()
    q, ok = queries(eng)
    s = windows(step, a.launches)
    res["panda"] = {"workload": "Panda push, %d envs after %d untimed steps with random actions (auto-reset)" % (n, a.preroll), "envs": n,
                    "links": int(eng._table[2]), "dof": eng.ndof, "query": q, "outputs_finite": ok,
                    "step_tensor": dict(s, note="includes the uniform_ that draws the actions"),
                    "step_dominant_kernel_ms": float(eng.timing()[3]), "all_over_step": q["all"]["median_ms"] / s["median_ms"]}
    res["value"] = q["all"]["median_ms"]
    env.close()
    # ---- the iCub with hands, used alone
    n = a.hands_envs
    cid = _client.connect(n)
    rob = iCubHandsEnv(cid)
    eng = rob._engine_or_build()
    rng = np.random.default_rng(7)
    st = eng.get_state()
    st[:, :eng.ndof] += 0.15 * rng.uniform(-1, 1, (n, eng.ndof)).astype(np.float32)
    st[:, eng.v_off:eng.v_off + eng.ndof] = rng.normal(0, 1, (n, eng.ndof)).astype(np.float32)
    eng.set_state(st)
    q, ok = queries(eng)
    res["hands"] = {"workload": "iCub with hands used alone, %d envs, joints spread 0.15 rad about the home pose, qd ~ N(0, 1)" % n, "envs": n,
                    "links": int(eng._table[2]), "dof": eng.ndof, "query": q, "outputs_finite": ok}
    _client.disconnect(cid)
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
