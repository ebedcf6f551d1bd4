"""pt_temporal_accumulate_moments and pt_denoise_variance against pt_temporal_accumulate and pt_denoise on the
same handle and the same 2-spp frame: HIP-event times, warm, every figure over a window of at least 0.5 s, and the bytes each
call must move by its record layout.  Runs on the GPU box.
Usage: python tools/gpu_variance_time.py [cbox bunny ...]      PT_TIME_WINDOW=0.02 shortens the windows and
PT_TIME_SIZES=640x480 picks the frame sizes

The history is two frames of a still camera, so every tap is kept.  pt_denoise_variance is timed twice: with that history's
length (2 < min_history: every filterable pixel gathers the 7 x 7 spatial estimate, the worst case) and with the length set to
8 (no pixel does)."""
import os
import sys

import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
from gpu_denoise_time import HBM_BYTES_PER_S, ITERATIONS, SC, SIZES, timed  # noqa: E402

from pathtracer_cuda_interactive_amd import PT_BVH_SORT_REFERENCE, HostScene  # noqa: E402
from pathtracer_cuda_interactive_amd import device as dev  # noqa: E402

TEMPORAL = dict(max_history=0, sigma_z=0.0, normal_min=0.9)


def main():
    stream = torch.cuda.current_stream().cuda_stream
    for name in sys.argv[1:] or ["cbox", "bunny"]:
        hs = HostScene.load(os.path.join(SC, name + ".pts"))
        ds = dev.DeviceScene(hs.finalize(PT_BVH_SORT_REFERENCE))
        for w, h in SIZES:
            p = hs.render_params(w, h, 2)
            f3 = lambda: torch.empty((h, w, 3), device="cuda")       # noqa: E731
            f1 = lambda: torch.empty((h, w), device="cuda")          # noqa: E731
            f2 = lambda: torch.empty((h, w, 2), device="cuda")       # noqa: E731
            color, albedo, normal, out = f3(), f3(), f3(), f3()
            depth, prev_depth, motion = f1(), f1(), f2()
            hist = dict(color=f3(), length=f1(), moments=f2())
            cur = dict(color=f3(), length=f1(), moments=f2())
            ds.render_into(p, color.data_ptr(), stream)
            ds.render_guides_into(p, p, albedo_ptr=albedo.data_ptr(), normal_ptr=normal.data_ptr(), depth_ptr=depth.data_ptr(),
                                  motion_ptr=motion.data_ptr(), prev_depth_ptr=prev_depth.data_ptr())
            ptrs = (color.data_ptr(), albedo.data_ptr(), normal.data_ptr(), motion.data_ptr(), prev_depth.data_ptr())
            ds.temporal_accumulate_moments_into(w, h, *ptrs, None, hist["color"].data_ptr(), hist["length"].data_ptr(),
                                                hist["moments"].data_ptr(), stream, **TEMPORAL)
            hist5 = [hist["color"].data_ptr(), normal.data_ptr(), depth.data_ptr(), hist["length"].data_ptr(), hist["moments"].data_ptr()]
            t_acc, n_acc = timed(lambda: ds.temporal_accumulate_into(w, h, ptrs[0], ptrs[2], ptrs[3], ptrs[4], hist5[:4],
                                                                     cur["color"].data_ptr(), cur["length"].data_ptr(), stream, **TEMPORAL))
            t_mom, n_mom = timed(lambda: ds.temporal_accumulate_moments_into(w, h, *ptrs, hist5, cur["color"].data_ptr(),
                                                                             cur["length"].data_ptr(), cur["moments"].data_ptr(),
                                                                             stream, **TEMPORAL))
            guides = (albedo.data_ptr(), normal.data_ptr(), depth.data_ptr())
            t_dn, n_dn = timed(lambda: ds.denoise_into(w, h, cur["color"].data_ptr(), *guides, out.data_ptr(), stream,
                                                       iterations=ITERATIONS))
            assert float(cur["length"].max()) == 2.0
            t_vs, n_vs = timed(lambda: ds.denoise_variance_into(w, h, cur["color"].data_ptr(), *guides, cur["moments"].data_ptr(),
                                                                cur["length"].data_ptr(), out.data_ptr(), 0, stream,
                                                                iterations=ITERATIONS))
            long_len = torch.full((h, w), 8.0, device="cuda")
            t_vl, n_vl = timed(lambda: ds.denoise_variance_into(w, h, cur["color"].data_ptr(), *guides, cur["moments"].data_ptr(),
                                                                long_len.data_ptr(), out.data_ptr(), 0, stream, iterations=ITERATIONS))
            npix = w * h
            # pt_temporal_accumulate: 36 B of this frame in, 32 B of one history pixel (neighbouring lanes share their taps),
            # 16 B out; the moments call adds the albedo (12 B), the history's moments (8 B) and the moments out (8 B)
            acc_b, mom_b = npix * 84, npix * 112
            # pt_denoise: see gpu_denoise_time.py; pt_denoise_variance's prep reads moments and length as well (52 B in, 32 B out)
            dn_b = npix * (72 + 48 * (ITERATIONS - 1) + 56)
            vd_b = npix * (84 + 48 * (ITERATIONS - 1) + 56)
            us = lambda b: b / HBM_BYTES_PER_S * 1e6                 # noqa: E731
            print(f"{name:6s} {w}x{h}: pt_temporal_accumulate {t_acc * 1e3:7.1f} us ({n_acc} calls; {acc_b / 1e6:.1f} MB = {us(acc_b):.1f} us "
                  f"at the HBM copy rate, {100 * us(acc_b) / (t_acc * 1e3):.1f} %) | pt_temporal_accumulate_moments {t_mom * 1e3:7.1f} us "
                  f"({n_mom}; {mom_b / 1e6:.1f} MB = {us(mom_b):.1f} us, {100 * us(mom_b) / (t_mom * 1e3):.1f} %) = {t_mom / t_acc:.2f} x | "
                  f"pt_denoise {ITERATIONS} iterations {t_dn * 1e3:7.1f} us ({n_dn}; {dn_b / 1e6:.1f} MB = {us(dn_b):.1f} us, "
                  f"{100 * us(dn_b) / (t_dn * 1e3):.1f} %) | pt_denoise_variance {ITERATIONS} iterations, history 2 (spatial estimate "
                  f"everywhere) {t_vs * 1e3:7.1f} us ({n_vs}) = {t_vs / t_dn:.2f} x, history 8 {t_vl * 1e3:7.1f} us ({n_vl}; "
                  f"{vd_b / 1e6:.1f} MB = {us(vd_b):.1f} us, {100 * us(vd_b) / (t_vl * 1e3):.1f} %) = {t_vl / t_dn:.2f} x", flush=True)
        ds.close()


if __name__ == "__main__":
    main()
