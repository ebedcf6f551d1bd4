"""The temporal-gradient stages beside what they accompany, on one handle and the same 2-spp frame: the row
render at stride 3 beside the full frame, pt_temporal_gradient, and pt_temporal_accumulate_adaptive beside
pt_temporal_accumulate_moments; and the sparse variant's stages beside the rows ones: pt_gradient_pixels, the
pixel-list render of one pixel per tile, pt_temporal_gradient_sparse, and the sum of either chain.  HIP-event times, warm, every figure over a window of at least 0.5 s.  Runs on the GPU box.
Usage: python tools/gpu_gradient_time.py [cbox bunny ...]      PT_TIME_WINDOW=0.02 shortens the windows and
PT_TIME_SIZES=640x480,1280x960 picks the frame sizes (default 640x480)

The history is two frames of a still camera, so every tap is kept and every pixel reads its tile's lambda; the map is timed
twice: all 0 (an unchanged scene: the plain blend) and the one the gradient of a relit scene (lights x (0.2, 0.5, 1)) gives."""
import os
import sys

import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
os.environ.setdefault("PT_TIME_SIZES", "640x480")
from animate import relit_desc  # noqa: E402
from gpu_denoise_time import HBM_BYTES_PER_S, SC, SIZES, timed  # noqa: E402

from pathtracer_cuda_interactive_amd import PT_BVH_SORT_REFERENCE, HostScene  # noqa: E402
from pathtracer_cuda_interactive_amd import device as dev  # noqa: E402

TEMPORAL = dict(max_history=0, sigma_z=0.0, normal_min=0.9)


def main():
    stream = torch.cuda.current_stream().cuda_stream
    for name in sys.argv[1:] or ["cbox", "bunny"]:
        hs = HostScene.load(os.path.join(SC, name + ".pts"))
        d0 = hs.finalize(PT_BVH_SORT_REFERENCE)
        ds = dev.DeviceScene(d0)
        for w, h in SIZES:
            p = hs.render_params(w, h, 2)
            rows_p = dev.gradient_rows_params(p)
            _, th, tw = dev.gradient_grid(w, h)
            f3 = lambda n=h: torch.empty((n, w, 3), device="cuda")   # noqa: E731
            f1 = lambda: torch.empty((h, w), device="cuda")          # noqa: E731
            f2 = lambda: torch.empty((h, w, 2), device="cuda")       # noqa: E731
            color, albedo, normal, rows = f3(), f3(), f3(), f3(th)
            depth, prev_depth, motion = f1(), f1(), f2()
            lam, zero = torch.empty((th, tw), device="cuda"), torch.zeros((th, tw), device="cuda")
            pixels, listed = torch.empty(th * tw, dtype=torch.int32, device="cuda"), torch.empty((th * tw, 3), device="cuda")
            lam_s = torch.empty((th, tw), device="cuda")
            hist = dict(color=f3(), length=f1(), moments=f2())
            cur = dict(color=f3(), length=f1(), moments=f2())
            t_full, n_full = timed(lambda: ds.render_into(p, color.data_ptr(), stream))
            t_rows, n_rows = timed(lambda: ds.render_into(rows_p, rows.data_ptr(), stream))
            torch.cuda.synchronize()
            assert torch.equal(rows, color[1::3]), "the row render must repeat the full frame's rows"
            t_pix, n_pix = timed(lambda: ds.gradient_pixels_into(w, h, 1, pixels.data_ptr(), stream))
            t_list, n_list = timed(lambda: ds.render_pixels_into(p, pixels.data_ptr(), th * tw, listed.data_ptr(), stream))
            torch.cuda.synchronize()
            assert torch.equal(listed, color.reshape(-1, 3)[pixels.long()]), "the list render must repeat the full frame's pixels"
            ds.render_guides_into(p, p, albedo_ptr=albedo.data_ptr(), normal_ptr=normal.data_ptr(), depth_ptr=depth.data_ptr(),
                                  motion_ptr=motion.data_ptr(), prev_depth_ptr=prev_depth.data_ptr())
            ptrs = (color.data_ptr(), albedo.data_ptr(), normal.data_ptr(), motion.data_ptr(), prev_depth.data_ptr())
            ds.temporal_accumulate_moments_into(w, h, *ptrs, None, hist["color"].data_ptr(), hist["length"].data_ptr(),
                                                hist["moments"].data_ptr(), stream, **TEMPORAL)
            hist5 = [hist["color"].data_ptr(), normal.data_ptr(), depth.data_ptr(), hist["length"].data_ptr(), hist["moments"].data_ptr()]
            outs = (cur["color"].data_ptr(), cur["length"].data_ptr(), cur["moments"].data_ptr())
            ds.temporal_gradient_into(w, h, color.data_ptr(), rows.data_ptr(), lam.data_ptr(), stream)
            torch.cuda.synchronize()
            assert float(lam.abs().max()) == 0.0, "an unchanged scene must give lambda 0"
            ds.temporal_gradient_sparse_into(w, h, color.data_ptr(), pixels.data_ptr(), listed.data_ptr(), lam_s.data_ptr(), stream)
            torch.cuda.synchronize()
            assert float(lam_s.abs().max()) == 0.0, "an unchanged scene must give lambda 0 (sparse)"
            ds.update(relit_desc(d0, (0.2, 0.5, 1.0)), geometry=False, shading=True)
            ds.render_into(rows_p, rows.data_ptr(), stream)
            t_grad, n_grad = timed(lambda: ds.temporal_gradient_into(w, h, color.data_ptr(), rows.data_ptr(), lam.data_ptr(), stream))
            ds.render_pixels_into(p, pixels.data_ptr(), th * tw, listed.data_ptr(), stream)
            t_sgrad, n_sgrad = timed(lambda: ds.temporal_gradient_sparse_into(w, h, color.data_ptr(), pixels.data_ptr(), listed.data_ptr(),
                                                                              lam_s.data_ptr(), stream))
            ds.update(d0, geometry=False, shading=True)
            t_mom, n_mom = timed(lambda: ds.temporal_accumulate_moments_into(w, h, *ptrs, hist5, *outs, stream, **TEMPORAL))
            t_ad0, n_ad0 = timed(lambda: ds.temporal_accumulate_adaptive_into(w, h, *ptrs, hist5, *outs, zero.data_ptr(), stream=stream,
                                                                              **TEMPORAL))
            t_ad1, n_ad1 = timed(lambda: ds.temporal_accumulate_adaptive_into(w, h, *ptrs, hist5, *outs, lam.data_ptr(), stream=stream,
                                                                              **TEMPORAL))
            torch.cuda.synchronize()
            # pt_temporal_gradient: one row in three of the previous frame and the re-traced rows in (24 B per sampled pixel), per
            # tile 32 B out of the reduce, 32 B in and out per iteration but the last, 32 B in and 4 B out of the last
            grad_b = th * w * 24 + th * tw * (32 + 64 * 2 + 36)
            us = lambda b: b / HBM_BYTES_PER_S * 1e6                 # noqa: E731
            print(f"{name:6s} {w}x{h}: pt_render 2 spp {t_full * 1e3:7.1f} us ({n_full} calls) | every 3rd row of it ({th} rows) "
                  f"{t_rows * 1e3:7.1f} us ({n_rows}) = {t_rows / t_full:.2f} x | pt_temporal_gradient, {tw}x{th} tiles, 3 iterations "
                  f"{t_grad * 1e3:7.1f} us ({n_grad}; {grad_b / 1e6:.2f} MB = {us(grad_b):.2f} us at the HBM copy rate), lambda mean "
                  f"{float(lam.mean()):.3f} | pt_temporal_accumulate_moments {t_mom * 1e3:7.1f} us ({n_mom}) | "
                  f"pt_temporal_accumulate_adaptive, lambda 0 {t_ad0 * 1e3:7.1f} us ({n_ad0}) = {t_ad0 / t_mom:.2f} x, relit lambda "
                  f"{t_ad1 * 1e3:7.1f} us ({n_ad1}) = {t_ad1 / t_mom:.2f} x", flush=True)
            # pt_temporal_gradient_sparse: per tile 4 B of the list, 12 B of the previous frame (a 32-B sector each where the
            # stride spreads them) and 12 B re-traced in, then the same records
            sgrad_b = th * tw * (4 + 32 + 12) + th * tw * (32 + 64 * 2 + 36)
            rows_chain, sparse_chain = t_rows + t_grad, t_pix + t_list + t_sgrad
            print(f"{name:6s} {w}x{h} sparse: pt_gradient_pixels {t_pix * 1e3:7.1f} us ({n_pix}) | pt_render_pixels, one pixel per tile "
                  f"({th * tw} pixels) {t_list * 1e3:7.1f} us ({n_list}) = {t_list / t_full:.2f} x the frame, {t_list / t_rows:.2f} x the "
                  f"rows | pt_temporal_gradient_sparse {t_sgrad * 1e3:7.1f} us ({n_sgrad}; {sgrad_b / 1e6:.2f} MB = {us(sgrad_b):.2f} us at "
                  f"the HBM copy rate), lambda mean {float(lam_s.mean()):.3f} | chain: rows + gradient {rows_chain * 1e3:7.1f} us, "
                  f"pixels + list + sparse gradient {sparse_chain * 1e3:7.1f} us = {sparse_chain / rows_chain:.2f} x", flush=True)
        ds.close()


if __name__ == "__main__":
    main()
