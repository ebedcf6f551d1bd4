#!/usr/bin/env python3
"""Offline render front-end (what the reference's main.cu does up to line 266, minus the window):
   python tools/render.py <scene.xml|scene.pts|buddha_standin|dragon_standin> [-o out.pfm|out.ppm] [--width W --height H --spp S]
                          [--traversal exact|pruned] [--seed 1984] [--bvh reference|lbvh|sah] [--nee]
                          [--adaptive MAX_ERROR [--batch-spp B] [--max-spp M] [--p-value P] [--min-luminance L] [--spp-map map.pfm]]
                          [--denoise [--denoise-iterations N --sigma-z Z --sigma-c C]] [--aov PREFIX]
Needs a GPU (no CPU fallback).  Multi-GPU: launch with torchrun; rows are interleaved over ranks, rank 0 writes."""
import argparse
import os
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("scene")
    ap.add_argument("-o", "--output", default="render.pfm")
    ap.add_argument("--width", type=int)
    ap.add_argument("--height", type=int)
    ap.add_argument("--spp", type=int)
    ap.add_argument("--seed", type=int, default=1984)
    ap.add_argument("--traversal", default="exact", choices=["exact", "pruned"])
    ap.add_argument("--bvh", default="reference", choices=["reference", "lbvh", "sah"],
                    help="reference: the host's reproduction of the reference tree (default); lbvh / sah: built on the GPU")
    ap.add_argument("--nee", action="store_true", help="next-event estimation (an extension: the reference samples no light)")
    ap.add_argument("--adaptive", type=float, metavar="MAX_ERROR",
                    help="adaptive sampling (an extension): sample each pixel until the relative half-width of its confidence "
                         "interval is at most MAX_ERROR; --spp is the first round")
    ap.add_argument("--batch-spp", type=int, default=0, help="adaptive: samples per later round (0 = --spp)")
    ap.add_argument("--max-spp", type=int, default=0, help="adaptive: most samples of one pixel (0 = 32 x --spp)")
    ap.add_argument("--p-value", type=float, default=0.05, help="adaptive: two-sided p-value of the interval")
    ap.add_argument("--min-luminance", type=float, default=0.01, help="adaptive: floor of the relative test's denominator")
    ap.add_argument("--spp-map", metavar="PATH", help="adaptive: write the per-pixel sample counts (PFM, the count in all channels)")
    ap.add_argument("--denoise", action="store_true",
                    help="filter the finished frame (an extension): edge-avoiding a-trous filter guided by first-hit albedo, normal and depth")
    ap.add_argument("--denoise-iterations", type=int, default=0, help="denoise: filter iterations, 1..8 (0 = 5)")
    ap.add_argument("--sigma-z", type=float, default=0.0, help="denoise: relative depth difference at half weight (0 = 0.05)")
    ap.add_argument("--sigma-c", type=float, default=0.0, help="denoise: luminance difference at half weight (0 = no colour term)")
    ap.add_argument("--aov", metavar="PREFIX", help="write the first-hit guide buffers: PREFIX_albedo.pfm, _normal.pfm, _depth.pfm")
    a = ap.parse_args()
    import numpy as np
    import torch
    import torch.distributed as dist

    from pathtracer_cuda_interactive_amd import (PT_BVH_SORT_REFERENCE, PT_RENDER_NEE, PT_TRAVERSAL_EXACT, PT_TRAVERSAL_PRUNED,
                                                 HostScene, standins, write_image)
    from pathtracer_cuda_interactive_amd import device as dev
    from pathtracer_cuda_interactive_amd import distributed as D
    world, rank, local = (int(os.environ.get(k, d)) for k, d in (("WORLD_SIZE", 1), ("RANK", 0), ("LOCAL_RANK", 0)))
    torch.cuda.set_device(local)
    if world > 1:
        dist.init_process_group("nccl", device_id=torch.device("cuda", local))
    t0 = time.perf_counter()
    hs = standins.BUILDERS[a.scene](os.path.join(REPO, "tests", "golden", "scenes")) if a.scene in standins.BUILDERS else HostScene.load(a.scene)
    desc = hs.finalize(PT_BVH_SORT_REFERENCE)
    depth = hs.bvh_depth
    if a.bvh != "reference":
        desc, info = dev.build_bvh_device(desc, dev.PT_BVH_DEVICE_SAH if a.bvh == "sah" else dev.PT_BVH_DEVICE_LBVH)
        depth = info["depth"]
    t1 = time.perf_counter()
    p = hs.render_params(a.width, a.height, a.spp, seed=a.seed)
    p.traversal = PT_TRAVERSAL_PRUNED if a.traversal == "pruned" else PT_TRAVERSAL_EXACT
    p.flags = PT_RENDER_NEE if a.nee else 0
    R = D.ShardedRenderer(desc)

    def finish(frame):
        """Rank 0, after the frame is assembled: guide buffers of the whole frame on this rank's GPU (one ray per pixel),
        the filter, the files.  Without --denoise / --aov the frame is returned as it is."""
        if not (a.denoise or a.aov):
            return frame, ""
        torch.cuda.synchronize()
        t_d = time.perf_counter()
        g = {k: torch.empty((p.height, p.width) + ((3,) if k != "depth" else ()), dtype=torch.float32, device=frame.device)
             for k in ("albedo", "normal", "depth")}
        R.scene.render_aov_into(p, g["albedo"].data_ptr(), g["normal"].data_ptr(), g["depth"].data_ptr(), 0)
        note = ""
        if a.denoise:
            frame = frame.contiguous()
            out = torch.empty_like(frame)
            R.scene.denoise_into(p.width, p.height, frame.data_ptr(), g["albedo"].data_ptr(), g["normal"].data_ptr(),
                                 g["depth"].data_ptr(), out.data_ptr(), torch.cuda.current_stream().cuda_stream,
                                 iterations=a.denoise_iterations, sigma_z=a.sigma_z, sigma_c=a.sigma_c)
            torch.cuda.synchronize()
            frame = out
            note = f"; guide buffers + denoise {(time.perf_counter() - t_d) * 1e3:.2f} ms"
        if a.aov:
            write_image(a.aov + "_albedo.pfm", g["albedo"].cpu().numpy())
            write_image(a.aov + "_normal.pfm", g["normal"].cpu().numpy())
            write_image(a.aov + "_depth.pfm", np.repeat(g["depth"].cpu().numpy()[..., None], 3, axis=2))
            note += f"; guide buffers -> {a.aov}_albedo.pfm, _normal.pfm, _depth.pfm"
        return frame, note
    if a.adaptive is not None:
        t_r = time.perf_counter()
        out = R.render_adaptive(p, a.adaptive, a.batch_spp, a.max_spp, a.p_value, a.min_luminance, rank, world)
        c = R.scene.counters()
        torch.cuda.synchronize()
        t2 = time.perf_counter()
        if rank == 0:
            frame, spp_map, _ = out
            frame, note = finish(frame)
            spp_map = spp_map.cpu().numpy()
            write_image(a.output, frame.cpu().numpy())
            if a.spp_map:
                write_image(a.spp_map, np.repeat(spp_map[..., None].astype(np.float32), 3, axis=2))
            print(f"{a.scene}: adaptive {p.width}x{p.height}, max_error {a.adaptive}, first round {p.spp} spp: "
                  f"mean {spp_map.mean():.2f} spp (min {spp_map.min()}, max {spp_map.max()}), "
                  f"{R.scene.info('adaptive_rounds')} rounds and kernel {c.kernel_ms:.2f} ms on rank 0, {t2 - t_r:.3f} s -> {a.output}"
                  + (f", {a.spp_map}" if a.spp_map else "") + note)
        R.close()
        if world > 1:
            dist.destroy_process_group()
        return
    frame = R.render(p, rank, world)
    c = R.scene.counters()
    torch.cuda.synchronize()
    t2 = time.perf_counter()
    if rank == 0:
        frame, note = finish(frame)
        write_image(a.output, frame.cpu().numpy())
        print(f"{a.scene}: {desc.num_shapes} primitives, {a.bvh} BVH of depth {depth}; parse+build {t1 - t0:.2f} s; "
              f"{p.width}x{p.height} spp={p.spp}: kernel {c.kernel_ms:.2f} ms on rank 0 ({c.segments / c.kernel_ms / 1e3:.0f} Msamples/s), "
              f"upload+render+gather {t2 - t1:.3f} s -> {a.output}" + note)
    R.close()
    if world > 1:
        dist.destroy_process_group()


if __name__ == "__main__":
    main()
