"""N frames of a .pts scene under a moving camera and, optionally, wobbling meshes, cleaned in image space.

  python tools/animate.py SCENE.pts [--frames 8] [--size 640x480] [--spp 2] [--translate DX,DY,DZ | --orbit DEG] [--wobble]
                          [--denoise | --variance | --gradient | --gradient-sparse] [--relight K:R,G,B] [--reference-spp N] [--out PREFIX] [--time]
                          [--spin G:AXIS:DEG_PER_FRAME ... [--rebuild-at PERMILLE]] [--async-guides]

Per frame: pt_render at --spp, pt_render_guides against the previous frame's camera (and, with --wobble, the previous
geometry: every mesh gets device.wobbled_desc's per-vertex wobble through DeviceScene.update), pt_temporal_accumulate, and with
--denoise pt_denoise on the accumulated colour.  Writes PREFIX_NNN_noisy.ppm / _accumulated.ppm / _denoised.ppm, prints the
HIP-event time of every stage per frame and their medians, and with --reference-spp the RMSE of each stage's image against a
pt_render of that many samples on the same geometry.  --translate is in units of the median first-hit distance of frame 0 per
frame (default 0.02,0.008,-0.013); --orbit turns the camera about its look-at point by that many degrees per frame instead.
--variance: the temporal stage is pt_temporal_accumulate_moments and the spatial stage pt_denoise_variance on
its colour, moments and history length (stages "accumulate_moments" and "denoise_variance", image _variance.ppm).
--gradient (implies --variance): from the second frame on, pt_render of the previous frame's parameters on every
third row of the current scene (stage "rows"), pt_temporal_gradient of the previous noisy frame against it (stage "gradient"),
and pt_temporal_accumulate_adaptive with that map in place of pt_temporal_accumulate_moments (stage "accumulate_adaptive").
--gradient-sparse (implies --gradient): the re-trace is one pixel per tile instead of a row.  From the second
frame on, pt_gradient_pixels with the frame number as its seed (stage "pixels"), pt_render_pixels of the previous frame's
parameters at that list on the current scene (stage "list"), and pt_temporal_gradient_sparse (stage "gradient").
--spin G:AXIS:DEG_PER_FRAME (repeatable): object G — mesh G, or sphere G - num_meshes, device.groups_by_object's
numbering — turns about the x, y or z axis through its centroid by that many degrees per frame through DeviceScene.transform: the
matrices go to the device, no vertex is touched on the host, and the guides follow the previous transform's records.  Not with --wobble.
--rebuild-at PERMILLE (with --spin): option "rebuild_at_permille" on the animated handle — a transform after which
the internal tree's summed box area has reached PERMILLE / 1000 of what it was built with rebuilds the tree inside the same call.
Frames are rendered with "stats" 1; every frame's line carries its node visits, the cost ratio and "rebuilt" where that happened.
--async-guides: the guide stage is pt_render_guides_async on the frame's stream, so a frame is enqueued stage after
stage without a host sync in between; the images are the same, bit for bit.
--relight K:R,G,B: from frame K on every light's radiance is scaled by (R, G, B) through DeviceScene.update(shading=True).
--time: after the animation, each stage again on the last frame's inputs, warm, in windows of at least 0.5 s, with
pt_render_aov and one pt_denoise iteration as yardsticks and the bytes pt_temporal_accumulate must move."""
import argparse
import json
import os
import sys

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
from pathtracer_cuda_interactive_amd import PT_BVH_SORT_REFERENCE, HostScene, host  # noqa: E402
from pathtracer_cuda_interactive_amd import ctypes_defs as cd  # noqa: E402
from pathtracer_cuda_interactive_amd import device as dev  # noqa: E402

HBM_BYTES_PER_S = 6.29e12          # measured float4 copy rate of the MI355X
TEMPORAL = dict(max_history=0, sigma_z=0.0, normal_min=0.9)      # the library's defaults; normal_min has none


def timed(fn, window_s=0.5):
    """Mean device time of fn() in ms: warm, then batches between two events until the window is filled."""
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    total_ms, n, batch = 0.0, 0, 8
    while total_ms < window_s * 1e3:
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(batch):
            fn()
        e1.record()
        e1.synchronize()
        total_ms += e0.elapsed_time(e1)
        n += batch
        batch = min(batch * 2, 4096)
    return total_ms / n


def once(fn):
    """Device time of one fn() in ms between two events on the current stream."""
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1)


def orbited_params(hs, w, h, spp, degrees):
    """Render parameters of the scene's camera turned about its look-at point, around its up vector."""
    cam = hs.camera
    at, up = np.array(cam.lookat[:], np.float64), np.array(cam.up[:], np.float64)
    up /= np.linalg.norm(up)
    v = np.array(cam.lookfrom[:], np.float64) - at
    a = np.radians(degrees)
    v = v * np.cos(a) + np.cross(up, v) * np.sin(a) + up * (up @ v) * (1 - np.cos(a))
    p = hs.render_params(w, h, spp)
    cam.lookfrom[:] = [float(x) for x in at + v]
    rd = host.camera_ray_data(cam, w, h)
    for name, row in zip(("cam_origin", "cam_top_left", "cam_horizontal", "cam_vertical"), rd):
        getattr(p, name)[:] = [float(x) for x in row]
    return p


def rmse(a, b):
    return float(np.sqrt(np.mean((a.astype(np.float64) - b.astype(np.float64)) ** 2)))


def relit_desc(desc, factor):
    """A copy of `desc` with every light's radiance scaled per channel."""
    lights = [cd.PtLight(l.type, l.shape_id, cd.c_float3(*(float(np.float32(c) * np.float32(f)) for c, f in zip(l.radiance, factor))),
                         cd.c_float3(*l.position)) for l in (desc.lights[k] for k in range(desc.num_lights))]
    return dev.edited_desc(desc, lights=lights)


def spin_setup(d0, specs, scenes):
    """Parses --spin, gives the spun objects the groups 0, 1, ... on every handle of `scenes` (all other shapes: -1) and returns
    frame -> matrices [groups, 3, 4]."""
    from pathtracer_cuda_interactive_amd.standins import mesh_arrays
    ids, G = dev.groups_by_object(d0)
    sh = dev.shape_table(d0)
    spins = []
    for spec in specs:
        g, axis, deg = spec.split(":")
        g, axis = int(g), {"x": (1, 0, 0), "y": (0, 1, 0), "z": (0, 0, 1)}[axis.lower()]
        if not 0 <= g < G:
            raise SystemExit(f"--spin {spec}: the scene has objects 0..{G - 1}")
        centre = mesh_arrays(d0, g)[0].astype(np.float64).mean(axis=0) if g < d0.num_meshes else sh["center"][ids == g][0]
        spins.append((g, axis, float(deg), centre))
    group_of = np.full(d0.num_shapes, -1, np.int32)
    for k, (g, _, _, _) in enumerate(spins):
        group_of[ids == g] = k
    for s in scenes:
        s.set_groups(group_of, len(spins))
    return lambda frame: np.stack([dev.rigid_matrix(axis, deg * frame, centre=c) for _, axis, deg, c in spins])


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("scene")
    ap.add_argument("--frames", type=int, default=8)
    ap.add_argument("--size", default="640x480")
    ap.add_argument("--spp", type=int, default=2)
    ap.add_argument("--translate", default="0.02,0.008,-0.013")
    ap.add_argument("--orbit", type=float, default=0.0)
    ap.add_argument("--wobble", action="store_true")
    ap.add_argument("--denoise", action="store_true")
    ap.add_argument("--variance", action="store_true")
    ap.add_argument("--gradient", action="store_true")
    ap.add_argument("--gradient-sparse", action="store_true")
    ap.add_argument("--relight", default="")
    ap.add_argument("--spin", action="append", default=[])
    ap.add_argument("--reference-spp", type=int, default=0)
    ap.add_argument("--out", default="")
    ap.add_argument("--time", action="store_true")
    ap.add_argument("--async-guides", action="store_true")
    ap.add_argument("--rebuild-at", type=int, default=0, metavar="PERMILLE")
    a = ap.parse_args()
    if a.rebuild_at and not a.spin:
        ap.error("--rebuild-at needs --spin")
    a.gradient = a.gradient or a.gradient_sparse
    a.variance = a.variance or a.gradient
    relight_at, relight_factor = None, None
    if a.relight:
        relight_at, relight_factor = int(a.relight.split(":")[0]), [float(v) for v in a.relight.split(":")[1].split(",")]
    w, h = (int(v) for v in a.size.split("x"))
    hs = HostScene.load(a.scene)
    d0 = hs.finalize(PT_BVH_SORT_REFERENCE)
    ds = dev.DeviceScene(d0)
    ref = dev.DeviceScene(d0) if a.reference_spp else None
    spin_matrices = None
    if a.spin:
        if a.wobble:
            ap.error("--spin and --wobble both move the geometry: give one")
        spin_matrices = spin_setup(d0, a.spin, [s for s in (ds, ref) if s is not None])
        if a.rebuild_at:
            ds.set_option("rebuild_at_permille", a.rebuild_at)
            ds.set_option("stats", 1)
    stream = torch.cuda.current_stream().cuda_stream
    f3 = lambda: torch.empty((h, w, 3), device="cuda")           # noqa: E731
    f1 = lambda: torch.empty((h, w), device="cuda")              # noqa: E731
    color, albedo, denoised = f3(), f3(), f3()
    motion, prev_depth = torch.empty((h, w, 2), device="cuda"), f1()
    # what a frame leaves for the next one, ping-ponged: accumulated colour, normal, depth, history length
    sets = [dict(out=f3(), normal=f3(), depth=f1(), length=f1()) for _ in range(2)]
    if a.variance:
        for st in sets:
            st["moments"] = torch.empty((h, w, 2), device="cuda")
    if a.gradient:
        # the noisy frame is kept for the next frame's gradient; the re-traced rows and the map
        for st in sets:
            st["color"] = f3()
        _, th, tw = dev.gradient_grid(w, h)
        rows, lam = torch.empty((th, w, 3), device="cuda"), torch.zeros((th, tw), device="cuda")
        if a.gradient_sparse:
            # one pixel per tile: the list and its re-traced colours
            pixels, listed = torch.empty(th * tw, dtype=torch.int32, device="cuda"), torch.empty((th * tw, 3), device="cuda")
    p0 = hs.render_params(w, h, a.spp)
    ds.render_aov_into(p0, 0, 0, sets[0]["depth"].data_ptr(), 0)
    z = sets[0]["depth"]
    step = np.array([float(v) for v in a.translate.split(",")]) * float(z[z > 0].median()) if (z > 0).any() else np.zeros(3)
    stages = ["render", "guides", "accumulate"] + (["denoise"] if a.denoise else [])
    if a.variance:
        stages = ["render", "guides", "accumulate_moments", "denoise_variance"]
    if a.gradient:
        stages = ["render", "rows", "gradient", "guides", "accumulate_adaptive", "denoise_variance"]
    if a.gradient_sparse:
        stages = ["render", "pixels", "list", "gradient", "guides", "accumulate_adaptive", "denoise_variance"]
    times = {s: [] for s in stages}
    errors = {s: [] for s in ("noisy", "accumulated", "denoised", "variance")}
    p_prev = None
    for k in range(a.frames):
        p = orbited_params(hs, w, h, a.spp, a.orbit * k) if a.orbit else dev.translated_params(p0, step * k)
        p.seed = 1984 + k
        cur, old = sets[k & 1], sets[(k + 1) & 1]
        update_ms = 0.0
        relit = relight_at is not None and k >= relight_at
        moved = bool(a.wobble and k)
        desc_k = None
        if moved or (relit and (a.wobble or k == relight_at)):
            desc_k = dev.wobbled_desc(d0, k) if moved else d0
            if relit:
                desc_k = relit_desc(desc_k, relight_factor)
            ds.update(desc_k, geometry=moved, shading=relit)
            update_ms = ds.info("update_us0") / 1e3
        if spin_matrices is not None and k:
            rebuilds = ds.info("rebuilds_auto")
            ds.transform(spin_matrices(k))
            update_ms = ds.info("transform_us0") / 1e3
            rebuilt = ds.info("rebuilds_auto") > rebuilds
        if a.gradient:
            color = cur["color"]
        times["render"].append(once(lambda: ds.render_into(p, color.data_ptr(), stream)))
        if a.gradient_sparse:
            times["pixels"].append(once(lambda: ds.gradient_pixels_into(w, h, k, pixels.data_ptr(), stream)) if k else 0.0)
            times["list"].append(once(lambda: ds.render_pixels_into(p_prev, pixels.data_ptr(), th * tw, listed.data_ptr(), stream))
                                 if k else 0.0)
            times["gradient"].append(once(lambda: ds.temporal_gradient_sparse_into(w, h, old["color"].data_ptr(), pixels.data_ptr(),
                                                                                   listed.data_ptr(), lam.data_ptr(), stream))
                                     if k else 0.0)
        elif a.gradient:
            times["rows"].append(once(lambda: ds.render_into(dev.gradient_rows_params(p_prev), rows.data_ptr(), stream)) if k else 0.0)
            times["gradient"].append(once(lambda: ds.temporal_gradient_into(w, h, old["color"].data_ptr(), rows.data_ptr(),
                                                                            lam.data_ptr(), stream)) if k else 0.0)
        guide_ptrs = dict(albedo_ptr=albedo.data_ptr(), normal_ptr=cur["normal"].data_ptr(), depth_ptr=cur["depth"].data_ptr(),
                          motion_ptr=motion.data_ptr(), prev_depth_ptr=prev_depth.data_ptr())
        if a.async_guides:
            times["guides"].append(once(lambda: ds.render_guides_async_into(p, p_prev or p, previous_geometry=True, stream=stream, **guide_ptrs)))
        else:
            times["guides"].append(once(lambda: ds.render_guides_into(p, p_prev or p, previous_geometry=True, **guide_ptrs)))
        hist = [old[n].data_ptr() for n in ("out", "normal", "depth", "length")] if k else None
        if a.variance:
            hist5 = hist + [old["moments"].data_ptr()] if k else None
            if a.gradient:
                times["accumulate_adaptive"].append(once(lambda: ds.temporal_accumulate_adaptive_into(
                    w, h, color.data_ptr(), albedo.data_ptr(), cur["normal"].data_ptr(), motion.data_ptr(), prev_depth.data_ptr(), hist5,
                    cur["out"].data_ptr(), cur["length"].data_ptr(), cur["moments"].data_ptr(), lam.data_ptr(), stream=stream, **TEMPORAL)))
            else:
                times["accumulate_moments"].append(once(lambda: ds.temporal_accumulate_moments_into(
                    w, h, color.data_ptr(), albedo.data_ptr(), cur["normal"].data_ptr(), motion.data_ptr(), prev_depth.data_ptr(), hist5,
                    cur["out"].data_ptr(), cur["length"].data_ptr(), cur["moments"].data_ptr(), stream, **TEMPORAL)))
            times["denoise_variance"].append(once(lambda: ds.denoise_variance_into(
                w, h, cur["out"].data_ptr(), albedo.data_ptr(), cur["normal"].data_ptr(), cur["depth"].data_ptr(),
                cur["moments"].data_ptr(), cur["length"].data_ptr(), denoised.data_ptr(), 0, stream)))
        else:
            times["accumulate"].append(once(lambda: ds.temporal_accumulate_into(
                w, h, color.data_ptr(), cur["normal"].data_ptr(), motion.data_ptr(), prev_depth.data_ptr(), hist,
                cur["out"].data_ptr(), cur["length"].data_ptr(), stream, **TEMPORAL)))
        if a.denoise and not a.variance:
            times["denoise"].append(once(lambda: ds.denoise_into(w, h, cur["out"].data_ptr(), albedo.data_ptr(), cur["normal"].data_ptr(),
                                                                 cur["depth"].data_ptr(), denoised.data_ptr(), stream)))
        torch.cuda.synchronize()
        images = {"noisy": color, "accumulated": cur["out"]}
        if a.variance:
            images["variance"] = denoised
        elif a.denoise:
            images["denoised"] = denoised
        line = f"frame {k:3d}: " + "  ".join(f"{s} {times[s][-1]:7.3f} ms" for s in stages)
        if desc_k is not None:
            line += f"  (update {update_ms:.3f} ms)"
        elif spin_matrices is not None and k:
            line += f"  (transform {update_ms:.3f} ms)"
            if a.rebuild_at:
                line += f"  tree cost {ds.info('tree_cost1_permille')} permille" + ("  rebuilt" if rebuilt else "")
        if a.rebuild_at:
            line += f"  node visits {ds.counters().node_visits}"
        if a.gradient and k:
            line += f"  lambda: mean {float(lam.mean()):.3f}, {float((lam > 0).float().mean()):.3f} of the tiles positive"
        valid = prev_depth > 0
        line += f"  history: {float((cur['length'][valid] > 1).float().mean()) if valid.any() else 0.0:.3f} of the valid pixels, " \
                f"mean length {float(cur['length'].mean()):.2f}"
        if ref is not None:
            if desc_k is not None:
                ref.update(desc_k, geometry=moved, shading=relit)
            if spin_matrices is not None and k:
                ref.transform(spin_matrices(k))
            q = p.copy()
            q.spp, q.seed = a.reference_spp, 7
            truth = ref.render(q)
            for name, img in images.items():
                errors[name].append(rmse(img.cpu().numpy(), truth))
            line += "  RMSE " + "  ".join(f"{name} {errors[name][-1]:.5f}" for name in images)
        print(line, flush=True)
        if a.out:
            for name, img in images.items():
                host.write_image(f"{a.out}_{k:03d}_{name}.ppm", img.cpu().numpy())
        p_prev = p
    summary = {"scene": os.path.basename(a.scene), "size": a.size, "spp": a.spp, "frames": a.frames,
               "median_ms": {s: float(np.median(times[s][1:] or times[s])) for s in stages}}
    if ref is not None:
        summary["rmse_last_frame"] = {n: e[-1] for n, e in errors.items() if e}
    if a.time:
        cur, old = sets[(a.frames - 1) & 1], sets[a.frames & 1]
        hist = [old[n].data_ptr() for n in ("out", "normal", "depth", "length")]
        scratch = f3()
        t = {}
        t["pt_render"] = timed(lambda: ds.render_into(p, color.data_ptr(), stream))
        t["pt_render_aov (4 buffers)"] = timed(lambda: ds.render_aov_into(p, albedo.data_ptr(), scratch.data_ptr(), prev_depth.data_ptr(), 0))
        t["pt_render_guides (4 buffers + motion)"] = timed(lambda: ds.render_guides_into(
            p, p_prev, previous_geometry=True, albedo_ptr=albedo.data_ptr(), normal_ptr=scratch.data_ptr(), depth_ptr=cur["depth"].data_ptr(),
            motion_ptr=motion.data_ptr(), prev_depth_ptr=prev_depth.data_ptr()))
        t["pt_render_guides_async (4 buffers + motion)"] = timed(lambda: ds.render_guides_async_into(
            p, p_prev, previous_geometry=True, albedo_ptr=albedo.data_ptr(), normal_ptr=scratch.data_ptr(), depth_ptr=cur["depth"].data_ptr(),
            motion_ptr=motion.data_ptr(), prev_depth_ptr=prev_depth.data_ptr(), stream=stream))
        t["pt_temporal_accumulate"] = timed(lambda: ds.temporal_accumulate_into(
            w, h, color.data_ptr(), cur["normal"].data_ptr(), motion.data_ptr(), prev_depth.data_ptr(), hist, scratch.data_ptr(),
            cur["length"].data_ptr(), stream, **TEMPORAL))
        if a.variance:
            hist5 = hist + [old["moments"].data_ptr()]
            mom = torch.empty((h, w, 2), device="cuda")
            t["pt_temporal_accumulate_moments"] = timed(lambda: ds.temporal_accumulate_moments_into(
                w, h, color.data_ptr(), albedo.data_ptr(), cur["normal"].data_ptr(), motion.data_ptr(), prev_depth.data_ptr(), hist5,
                scratch.data_ptr(), cur["length"].data_ptr(), mom.data_ptr(), stream, **TEMPORAL))
            if a.gradient_sparse:
                t["pt_gradient_pixels"] = timed(lambda: ds.gradient_pixels_into(w, h, a.frames - 1, pixels.data_ptr(), stream))
                t["pt_render_pixels, one pixel per tile of the previous frame"] = timed(lambda: ds.render_pixels_into(
                    p_prev, pixels.data_ptr(), th * tw, listed.data_ptr(), stream))
                t["pt_temporal_gradient_sparse"] = timed(lambda: ds.temporal_gradient_sparse_into(
                    w, h, old["color"].data_ptr(), pixels.data_ptr(), listed.data_ptr(), lam.data_ptr(), stream))
            if a.gradient:
                t["pt_render, every 3rd row of the previous frame"] = timed(lambda: ds.render_into(dev.gradient_rows_params(p_prev),
                                                                                                   rows.data_ptr(), stream))
                t["pt_temporal_gradient"] = timed(lambda: ds.temporal_gradient_into(w, h, old["color"].data_ptr(), rows.data_ptr(),
                                                                                    lam.data_ptr(), stream))
                t["pt_temporal_accumulate_adaptive"] = timed(lambda: ds.temporal_accumulate_adaptive_into(
                    w, h, color.data_ptr(), albedo.data_ptr(), cur["normal"].data_ptr(), motion.data_ptr(), prev_depth.data_ptr(), hist5,
                    scratch.data_ptr(), cur["length"].data_ptr(), mom.data_ptr(), lam.data_ptr(), stream=stream, **TEMPORAL))
            t["pt_denoise, 5 iterations"] = timed(lambda: ds.denoise_into(w, h, cur["out"].data_ptr(), albedo.data_ptr(), cur["normal"].data_ptr(),
                                                                          cur["depth"].data_ptr(), scratch.data_ptr(), stream))
            t["pt_denoise_variance, 5 iterations"] = timed(lambda: ds.denoise_variance_into(
                w, h, cur["out"].data_ptr(), albedo.data_ptr(), cur["normal"].data_ptr(), cur["depth"].data_ptr(), cur["moments"].data_ptr(),
                cur["length"].data_ptr(), scratch.data_ptr(), 0, stream))
        t["pt_denoise, 1 iteration"] = timed(lambda: ds.denoise_into(w, h, color.data_ptr(), albedo.data_ptr(), cur["normal"].data_ptr(),
                                                                     cur["depth"].data_ptr(), scratch.data_ptr(), stream, iterations=1))
        # per pixel: colour, normal, motion, prev_depth in (36 B), one history pixel's colour, normal, depth, length in where
        # neighbouring lanes share their taps (32 B), colour and length out (16 B)
        moved = w * h * 84
        summary["timed_ms"] = t
        summary["accumulate_bytes"] = moved
        summary["accumulate_hbm_bound_us"] = moved / HBM_BYTES_PER_S * 1e6
    print(json.dumps(summary))
    ds.close()
    if ref is not None:
        ref.close()


if __name__ == "__main__":
    main()
