"""Images/s and rays/s of the batched camera (include/pbre_camera.h): 4096 Panda-push envs after a reset and a few random steps, the
task envs' camera, at 64 x 48 and at 84 x 84, for depth + segmentation and for all three outputs.  Device-resident outputs
(pbre_camera_render_device on torch's current stream), timed with device events around `--launches` renders after `--warmup` untimed
ones, `--repeats` windows per case (the spread is printed: median, min, max).  One render = k_cam_scene + k_cam_rays; a ray is one pixel
of one env.  Prints one JSON line per case; --out also writes them to a file."""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "pybullet-robot-envs_amd"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--envs", type=int, default=4096)
    ap.add_argument("--sizes", default="64x48,84x84")
    ap.add_argument("--launches", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if a.launches < 20:
        ap.error("--launches must be at least 20")
    import torch
    from pybullet_robot_envs import _capi, camera as pcam
    from pybullet_robot_envs.model.table import panda_table
    if not torch.cuda.is_available():
        raise SystemExit("bench_camera: no GPU (there is nothing to measure on a CPU)")
    tbl, _ = panda_table()
    eng = _capi.Engine(tbl, task=_capi.TASK_PUSH, num_envs=a.envs, obj_pose_rnd_std=0.05, tg_pose_rnd_std=0.2)
    eng.reset()
    rng = np.random.default_rng(0)
    for _ in range(20):
        eng.step(rng.uniform(-1, 1, (a.envs, eng.act_dim)).astype(np.float32))
    results = []
    for size in a.sizes.split(","):
        W, H = (int(x) for x in size.split("x"))
        view = pcam.view_matrix_from_yaw_pitch_roll(tbl[6:9], 1.3, 180, -40, 0, 2)
        proj = pcam.projection_matrix_fov(60, float(W) / H, 0.1, 100.0)
        cam = eng.make_camera(W, H, view=view, proj=proj)
        for name, kw in (("depth+seg", dict(depth=True, seg=True, rgb=False)), ("depth+seg+rgba", dict(depth=True, seg=True, rgb=True))):
            for _ in range(a.warmup):
                out = eng.render(cam, out="torch", **kw)
            torch.cuda.synchronize()
            ms = []
            for _ in range(a.repeats):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                for _ in range(a.launches):
                    out = eng.render(cam, out="torch", **kw)      # (fresh output tensors from torch's caching allocator: no device allocation)
                e1.record()
                e1.synchronize()
                ms.append(e0.elapsed_time(e1) / a.launches)
            seg = out["seg"]
            covered = float((seg >= 0).float().mean().item())
            med = float(np.median(ms))
            r = {"envs": a.envs, "width": W, "height": H, "outputs": name, "ms_per_render": med, "ms_min": min(ms), "ms_max": max(ms),
                 "images_per_s": a.envs / (med * 1e-3), "rays_per_s": a.envs * W * H / (med * 1e-3), "primitives": len(eng_visuals(eng)),
                 "pixels_hit": covered, "launches": a.launches, "repeats": a.repeats, "device": torch.cuda.get_device_name(0)}
            print(json.dumps(r))
            results.append(r)
    if a.out:
        with open(a.out, "w") as f:
            json.dump(results, f, indent=1)
    eng.close()


def eng_visuals(eng):
    from pybullet_robot_envs.model.visuals import default_visuals
    return default_visuals(eng._table)


if __name__ == "__main__":
    main()
