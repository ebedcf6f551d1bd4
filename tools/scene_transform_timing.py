"""Wall time of pt_scene_transform against pt_scene_update of the same animation in the same process.

  python tools/scene_transform_timing.py SCENE.pts | --standin buddha [--frames 20] [--only-transform]
  python tools/scene_transform_timing.py --all          # bunny, then the buddha stand-in, a process each

Every mesh of the scene turns about its own centroid, a few degrees more from frame to frame (spheres stay: group -1).  Handle
A takes the matrices (DeviceScene.transform: 84 bytes per mesh go to the device); handle B takes the desc the host twin makes
from the rest desc and the same matrices (transform_desc_host, then DeviceScene.update: every vertex goes to the device).  The
host's own transform time is listed apart and not counted against the update.  One JSON line per scene: median and max of both
calls over the frames after the first, the "transform_us0".."transform_us3" and "update_us0".."update_us3" split of the median
call, the first call of each (which pays for the snapshot and the refit plans), and whether the first and the last frame of
the two handles are equal bit for bit.  --only-transform runs handle A alone (a kernel trace of its own).
--all runs each scene in a process of its own under `timeout -k 10`, chained with &&: a step that fails or hangs ends the run.
-> profiles/scene_transform_timing.log"""
import argparse
import json
import os
import subprocess
import sys
import time

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)


def run_all(frames):
    me = os.path.abspath(__file__)
    bunny = os.path.join(REPO, "tests", "golden", "scenes", "bunny.pts")
    steps = [f"timeout -k 10 240 {sys.executable} {me} {bunny} --frames {frames}",
             f"timeout -k 10 420 {sys.executable} {me} --standin buddha --frames {frames}"]
    return subprocess.run(["bash", "-c", " && ".join(steps)]).returncode


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("scene", nargs="?", help="a .pts scene")
    ap.add_argument("--standin", choices=["buddha", "dragon"])
    ap.add_argument("--frames", type=int, default=20)
    ap.add_argument("--only-transform", action="store_true")
    ap.add_argument("--all", action="store_true")
    a = ap.parse_args()
    if a.all:
        sys.exit(run_all(a.frames))
    if bool(a.scene) == bool(a.standin):
        ap.error("give a .pts scene or --standin")
    from pathtracer_cuda_interactive_amd import PT_BVH_SORT_REFERENCE, HostScene, standins
    from pathtracer_cuda_interactive_amd import device as dev
    if a.standin:
        hs = standins.BUILDERS[a.standin + "_standin"](os.path.join(REPO, "tests", "golden", "scenes"))
    else:
        hs = HostScene.load(a.scene)
    d = hs.finalize(PT_BVH_SORT_REFERENCE)
    p = hs.render_params(160, 120, 2)
    ids, G = dev.groups_by_object(d)
    ids[ids >= d.num_meshes] = -1                       # spheres stay
    G = d.num_meshes
    centres = [standins.mesh_arrays(d, m)[0].astype(np.float64).mean(axis=0) for m in range(G)]

    def matrices(step):
        return np.stack([dev.rigid_matrix((0.1 * (m % 3), 1.0, 0.05 * (m % 2)), 3.0 * step * (1 + m % 4), centre=centres[m])
                         for m in range(G)])

    n = max(a.frames, 2)
    A = dev.DeviceScene(d)
    B = None if a.only_transform else dev.DeviceScene(d)
    try:
        A.set_groups(ids, G)
        t_split, u_split, host_ms, same = [], [], [], {}
        for step in range(1, n + 1):
            M = matrices(step)
            A.transform(M)
            t_split.append([A.info(f"transform_us{k}") for k in range(4)])
            if B is None:
                continue
            t0 = time.perf_counter()
            d1 = dev.transform_desc_host(d, ids, M)
            host_ms.append((time.perf_counter() - t0) * 1e3)
            B.update(d1)
            u_split.append([B.info(f"update_us{k}") for k in range(4)])
            if step in (1, n):
                same["first" if step == 1 else "last"] = bool(np.array_equal(A.render(p).view(np.uint32), B.render(p).view(np.uint32)))
        info = {k: A.info(k) for k in ("fast_tree", "fast_tree_is_callers", "residency", "transforms", "refit_shape0", "refit_shape1")}
    finally:
        A.close()
        if B is not None:
            B.close()

    def summary(split, names):
        later = sorted(split[1:], key=lambda u: u[0])
        med = later[len(later) // 2]
        return {"ms_median": med[0] / 1e3, "ms_max": later[-1][0] / 1e3, "first_ms": split[0][0] / 1e3,
                "first_once_ms": split[0][3] / 1e3, "split_median_ms": {k: med[1 + i] / 1e3 for i, k in enumerate(names)}}

    out = {"scene": a.standin + "_standin (stand-in geometry)" if a.standin else os.path.basename(a.scene), "shapes": d.num_shapes,
           "groups": G, "frames": n, "transform": summary(t_split, ("records", "refit", "snapshot_or_plan")), **info}
    if B is not None:
        out["update"] = summary(u_split, ("records_and_uploads", "refit", "plan"))
        out["host_transform_ms_median"] = float(np.median(host_ms))
        out["transform_over_update"] = out["transform"]["ms_median"] / out["update"]["ms_median"]
        out["first_frame_bit_equal"], out["last_frame_bit_equal"] = same["first"], same["last"]
    print(json.dumps(out))


if __name__ == "__main__":
    main()
