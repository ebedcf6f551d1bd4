"""Wall time of pt_scene_rebuild against pt_scene_create of the same scene in the same process, what a rebuild buys on a grid of
cubes that traded places, and what the tree-cost telemetry adds to a transform.

  python tools/scene_rebuild_timing.py SCENE.pts | --standin buddha [--rebuilds 20]
  python tools/scene_rebuild_timing.py --grid 8 [--rebuilds 20]

Scene mode: every mesh gets tools/scene_update_timing.py's wobble, DeviceScene.update takes the new positions and
DeviceScene.rebuild follows.  One JSON line: the median "rebuild_us0" with the "rebuild_us1".."rebuild_us3" split of the median
call, beside the median "create_us0" of fresh creates in the same process (of the rest scene and of the first and last wobbled
one on the host's refitted pool), whether the rebuild was below the create, and whether the first and the last rebuilt frame
equal the fresh create's bit for bit.
Grid mode: n^3 cubes (standins.grid_scene), every cube translated to another cell.  node_visits of one 160 x 120 frame at 2 spp
after the transform, after the rebuild and on a fresh create of the moved scene, and the median "transform_us0" of transforms
that alternate between two shuffles with option tree_cost 0 and 1 (a library without the option: the key "tree_cost" is null).
-> profiles/scene_rebuild_timing.log"""
import argparse
import json
import os
import sys

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tools"))


def median_row(rows):
    rows = sorted(rows, key=lambda u: u[0])
    return rows[len(rows) // 2]


def scene_mode(a):
    from scene_update_timing import wobbled

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
    create_us = []
    for _ in range(5):                                  # the first creation also pays for HIP's start-up
        f = dev.DeviceScene(d)
        create_us.append(f.info("create_us0"))
        f.close()
    S = dev.DeviceScene(d)
    try:
        split, adopted, same = [], [], {}
        n = max(a.rebuilds, 2)
        for step in range(1, n + 1):
            d1 = wobbled(d, meshes, step, dev)
            S.update(d1)
            adopted.append(int(S.rebuild()))
            split.append([S.info(f"rebuild_us{k}") for k in range(4)])
            if step in (1, n):
                f = dev.DeviceScene(host.refit_bvh(d1))
                create_us.append(f.info("create_us0"))
                same["first" if step == 1 else "last"] = bool(np.array_equal(S.render(p).view(np.uint32), f.render(p).view(np.uint32)))
                f.close()
        info = {k: S.info(k) for k in ("fast_tree", "fast_tree_is_callers", "residency", "sweep_on_device", "rebuilds", "rebuild_cost_permille")}
    finally:
        S.close()
    med = median_row(split)
    create_med = float(np.median(create_us[1:]))
    print(json.dumps({
        "scene": a.standin + "_standin (stand-in geometry)" if a.standin else os.path.basename(a.scene), "shapes": d.num_shapes,
        "rebuilds": n, "adopted": sum(adopted), "rebuild_ms_median": med[0] / 1e3, "rebuild_ms_max": max(u[0] for u in split) / 1e3,
        "rebuild_ms_split_median": {"leaf_boxes_and_build": med[1] / 1e3, "relayout_and_probe": med[2] / 1e3, "plan_and_sweep_tables": med[3] / 1e3},
        "create_ms_median": create_med / 1e3, "creates": len(create_us) - 1, "rebuild_over_create": med[0] / create_med,
        "rebuild_below_create": bool(med[0] < create_med), "first_frame_bit_equal": same["first"], "last_frame_bit_equal": same["last"], **info}))


def grid_mode(a):
    from pathtracer_cuda_interactive_amd import PtError, host, standins
    from pathtracer_cuda_interactive_amd import device as dev
    n = a.grid
    hs = standins.grid_scene(n)
    d0 = hs.finalize()
    ids, G = dev.groups_by_object(d0)
    M1, M2 = standins.grid_shuffle_matrices(n, 1), standins.grid_shuffle_matrices(n, 2)
    p = hs.render_params(160, 120, 2)

    def visits(S):
        S.set_option("stats", 1)
        S.render(p)
        v = S.counters().node_visits
        S.set_option("stats", 0)
        return v

    out = {"scene": f"grid of {n}^3 cubes, shuffled", "shapes": d0.num_shapes}
    S = dev.DeviceScene(d0)
    try:
        S.set_groups(ids, G)
        out["node_visits_at_rest"] = visits(S)
        S.transform(M1)
        out["node_visits_after_transform"] = visits(S)
        if hasattr(S, "rebuild"):
            out["rebuild_adopted"] = int(S.rebuild())
            out["node_visits_after_rebuild"] = visits(S)
            out["rebuild_ms"] = S.info("rebuild_us0") / 1e3
    finally:
        S.close()
    F = dev.DeviceScene(host.refit_bvh(dev.transform_desc_host(d0, ids, M1)))
    out["node_visits_fresh_create"] = visits(F)
    out["create_ms"] = F.info("create_us0") / 1e3
    F.close()
    for cost in (0, 1):
        S = dev.DeviceScene(d0)
        try:
            S.set_groups(ids, G)
            try:
                S.set_option("tree_cost", cost)
            except PtError:
                if cost:
                    out[f"transform_ms_median_tree_cost_{cost}"] = None
                    continue
            S.transform(M1)                              # pays the snapshot and the plans
            us = []
            for k in range(max(a.rebuilds, 2)):
                S.transform(M2 if k % 2 == 0 else M1)
                us.append(S.info("transform_us0"))
            out[f"transform_ms_median_tree_cost_{cost}"] = float(np.median(us)) / 1e3
            if cost:
                out["tree_cost1_permille"] = S.info("tree_cost1_permille")
        finally:
            S.close()
    print(json.dumps(out))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("scene", nargs="?", help="a .pts scene")
    ap.add_argument("--standin", choices=["buddha", "dragon"])
    ap.add_argument("--grid", type=int, default=0)
    ap.add_argument("--rebuilds", type=int, default=20)
    a = ap.parse_args()
    if sum([bool(a.scene), bool(a.standin), bool(a.grid)]) != 1:
        ap.error("give a .pts scene, --standin or --grid")
    grid_mode(a) if a.grid else scene_mode(a)


if __name__ == "__main__":
    main()
