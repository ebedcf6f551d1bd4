"""Wall time of pt_scene_update against pt_scene_create of the same scene in the same process.

  python tools/scene_update_timing.py SCENE.pts | --standin buddha [--updates 20]

Every mesh of the scene gets a smooth per-vertex wobble whose phase advances from update to update (vertex normals are left as
they are: the tool times the update, it does not shade), and DeviceScene.update takes the new positions.  One JSON line: median
and max update time with the "update_us0".."update_us3" split of the median update (the first update, which also builds the
refit plans, is reported apart), "create_us0" of fresh creates of the same scene, and whether the first and the last updated
frame equal, bit for bit, the frame of a fresh create of the same geometry with the host's refitted pool.
-> profiles/scene_update_timing.log"""
import argparse
import json
import os
import sys

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)


def wobbled(d, meshes, step, dev):
    """desc with every mesh displaced by amp * sin(k . p + phase(step)), amp = 1 % of the mesh's extent."""
    edits = {}
    for m, (P, size) in enumerate(meshes):
        ph = 0.37 * step
        off = np.stack([np.sin(5.0 / size * P[:, 1] + ph), np.cos(4.0 / size * P[:, 2] + ph), np.sin(6.0 / size * P[:, 0] - ph)], axis=1)
        edits[m] = ((P + np.float32(0.01 * size) * off.astype(np.float32)).astype(np.float32), None)
    return dev.edited_desc(d, meshes=edits)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("scene", nargs="?", help="a .pts scene")
    ap.add_argument("--standin", choices=["buddha", "dragon"])
    ap.add_argument("--updates", type=int, default=20)
    a = ap.parse_args()
    if bool(a.scene) == bool(a.standin):
        ap.error("give a .pts scene or --standin")
    from pathtracer_cuda_interactive_amd import PT_BVH_SORT_REFERENCE, HostScene, host, standins
    from pathtracer_cuda_interactive_amd import device as dev
    if a.standin:
        hs = standins.BUILDERS[a.standin + "_standin"](os.path.join(REPO, "tests", "golden", "scenes"))
    else:
        hs = HostScene.load(a.scene)
    d = hs.finalize(PT_BVH_SORT_REFERENCE)
    p = hs.render_params(160, 120, 2)
    meshes = []
    for m in range(d.num_meshes):
        P = standins.mesh_arrays(d, m)[0]
        meshes.append((P, max(float((P.max(axis=0) - P.min(axis=0)).max()), 1e-6)))

    def fresh_frame(desc):
        f = dev.DeviceScene(host.refit_bvh(desc))
        try:
            return f.render(p), f.info("create_us0")
        finally:
            f.close()

    create_us = []
    for _ in range(5):                                  # the first creation also pays for HIP's start-up
        f = dev.DeviceScene(d)
        create_us.append(f.info("create_us0"))
        f.close()
    S = dev.DeviceScene(d)
    try:
        split, same = [], {}
        n = max(a.updates, 2)
        for step in range(1, n + 1):
            d1 = wobbled(d, meshes, step, dev)
            S.update(d1)
            split.append([S.info(f"update_us{k}") for k in range(4)])
            if step in (1, n):
                want, us = fresh_frame(d1)
                create_us.append(us)
                same["first" if step == 1 else "last"] = bool(np.array_equal(S.render(p).view(np.uint32), want.view(np.uint32)))
        info = {k: S.info(k) for k in ("fast_tree", "fast_tree_is_callers", "residency", "updates")}
    finally:
        S.close()
    later = sorted(split[1:], key=lambda u: u[0])
    med = later[len(later) // 2]
    create_med = float(np.median(create_us[1:]))
    print(json.dumps({
        "scene": a.standin + "_standin (stand-in geometry)" if a.standin else os.path.basename(a.scene), "shapes": d.num_shapes,
        "updates": n, "update_ms_median": med[0] / 1e3, "update_ms_max": later[-1][0] / 1e3,
        "update_ms_split_median": {"records_and_uploads": med[1] / 1e3, "refit": med[2] / 1e3, "plan": med[3] / 1e3},
        "first_update_ms": split[0][0] / 1e3, "first_update_plan_ms": split[0][3] / 1e3,
        "create_ms_median": create_med / 1e3, "creates": len(create_us) - 1, "update_over_create": med[0] / create_med,
        "first_frame_bit_equal": same["first"], "last_frame_bit_equal": same["last"], **info}))


if __name__ == "__main__":
    main()
