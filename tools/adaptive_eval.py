#!/usr/bin/env python3
"""What adaptive sampling (pt_render_adaptive) buys, on scene1, cbox and bunny at 640x480:
  reference  a 4096-spp pt_render with another seed
  adaptive   spp 16, batch 16, max 512, max_error 0.05
  uniform    pt_render with the adaptive frame's total sample count (rounded to whole spp)
For each frame: RMSE against the reference (linear and sqrt display), total samples, rounds, wall time, summed kernel_ms.
Then the per-round cost of the adaptive frame (rounds of a few pixels pay a launch, a drain and a host read each).
Needs a GPU.   python tools/adaptive_eval.py [--scenes scene1,cbox,bunny] [--ref-spp 4096] [--reps 3]"""
import argparse
import os
import sys
import time

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)


def rmse(a, b):
    return float(np.sqrt(np.mean((a.astype(np.float64) - b) ** 2)))


def rmse_display(a, b):
    return rmse(np.sqrt(np.clip(a, 0, None)), np.sqrt(np.clip(b, 0, None)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--scenes", default="scene1,cbox,bunny")
    ap.add_argument("--width", type=int, default=640)
    ap.add_argument("--height", type=int, default=480)
    ap.add_argument("--ref-spp", type=int, default=4096)
    ap.add_argument("--spp", type=int, default=16)
    ap.add_argument("--batch", type=int, default=16)
    ap.add_argument("--max-spp", type=int, default=512)
    ap.add_argument("--max-error", type=float, default=0.05)
    ap.add_argument("--reps", type=int, default=3, help="timed repetitions of each frame (the fastest is reported)")
    a = ap.parse_args()
    from pathtracer_cuda_interactive_amd import PT_BVH_SORT_REFERENCE, HostScene
    from pathtracer_cuda_interactive_amd import device as dev
    print(f"{a.width}x{a.height}; reference {a.ref_spp} spp seed 7; adaptive spp {a.spp} batch {a.batch} max {a.max_spp} "
          f"max_error {a.max_error} (p 0.05, min_luminance 0.01); uniform = same total samples; times: best of {a.reps}")
    print(f"{'scene':8s} {'frame':9s} {'samples':>11s} {'spp':>7s} {'rounds':>6s} {'wall ms':>9s} {'kernel ms':>9s} "
          f"{'RMSE lin':>10s} {'RMSE sqrt':>10s}")
    for name in a.scenes.split(","):
        hs = HostScene.load(os.path.join(REPO, "tests", "golden", "scenes", name + ".pts"))
        desc = hs.finalize(PT_BVH_SORT_REFERENCE)
        ds = dev.DeviceScene(desc)
        try:
            ds.set_option("timing_frames", 1)
            ref = ds.render(hs.render_params(a.width, a.height, a.ref_spp, seed=7)).astype(np.float64)
            p = hs.render_params(a.width, a.height, a.spp)
            best = None
            for _ in range(a.reps):
                t0 = time.perf_counter()
                img, spp_map, _ = ds.render_adaptive(p, a.max_error, batch_spp=a.batch, max_spp=a.max_spp)
                wall = (time.perf_counter() - t0) * 1e3
                c = ds.counters()
                if best is None or wall < best[0]:
                    best = (wall, c.kernel_ms, c.resolve_ms)
            rounds = ds.info("adaptive_rounds")
            total = int(spp_map.sum())
            assert total == c.paths
            print(f"{name:8s} {'adaptive':9s} {total:11d} {total / spp_map.size:7.2f} {rounds:6d} {best[0]:9.2f} {best[1]:9.2f} "
                  f"{rmse(img, ref):10.5f} {rmse_display(img, ref):10.5f}")
            u_spp = max(1, int(round(total / spp_map.size)))
            pu = hs.render_params(a.width, a.height, u_spp)
            ubest = None
            for _ in range(a.reps):
                t0 = time.perf_counter()
                uimg = ds.render(pu)
                wall = (time.perf_counter() - t0) * 1e3
                c = ds.counters()
                if ubest is None or wall < ubest[0]:
                    ubest = (wall, c.kernel_ms)
            print(f"{name:8s} {'uniform':9s} {u_spp * spp_map.size:11d} {u_spp:7d} {1:6d} {ubest[0]:9.2f} {ubest[1]:9.2f} "
                  f"{rmse(uimg, ref):10.5f} {rmse_display(uimg, ref):10.5f}")
            # equal wall time: the uniform spp whose frame takes as long as the adaptive one
            e_spp = max(1, int(u_spp * best[0] / ubest[0]))
            pe = hs.render_params(a.width, a.height, e_spp)
            ebest = None
            for _ in range(a.reps + 1):                          # the first call grows the sample buffer: not timed
                t0 = time.perf_counter()
                eimg = ds.render(pe)
                wall = (time.perf_counter() - t0) * 1e3
                if _ and (ebest is None or wall < ebest[0]):
                    ebest = (wall, ds.counters().kernel_ms)
            print(f"{name:8s} {'uni=wall':9s} {e_spp * spp_map.size:11d} {e_spp:7d} {1:6d} {ebest[0]:9.2f} {ebest[1]:9.2f} "
                  f"{rmse(eimg, ref):10.5f} {rmse_display(eimg, ref):10.5f}")
            hist = {int(n): int((spp_map == n).sum()) for n in np.unique(spp_map)}
            stopped_first = hist.get(a.spp, 0) / spp_map.size
            at_max = hist.get(a.max_spp, 0) / spp_map.size
            per_round = (best[0] - best[1] - best[2]) / max(rounds, 1)
            print(f"{name:8s} pixels stopping at {a.spp}: {100 * stopped_first:.1f} %, at {a.max_spp}: {100 * at_max:.1f} %; "
                  f"wall - kernel - resolve = {best[0] - best[1] - best[2]:.2f} ms over {rounds} rounds "
                  f"({per_round:.3f} ms per round: launches, drains, read-backs)")
        finally:
            ds.close()


if __name__ == "__main__":
    main()
