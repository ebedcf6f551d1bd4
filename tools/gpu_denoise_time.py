"""pt_render_aov and pt_denoise against the 4-spp frame they clean: HIP-event times, warm, every figure over a
window of at least 0.5 s, and the bytes an iteration must move by the record layout.  Runs on the GPU box.
Usage: python tools/gpu_denoise_time.py [cbox bunny ...]      PT_TIME_WINDOW=0.02 shortens the windows and
PT_TIME_SIZES=640x480 picks the frame sizes (kernel-trace runs: one scene and one size per run gives the per-kernel split)"""
import os
import sys

import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
from pathtracer_cuda_interactive_amd import PT_BVH_SORT_REFERENCE, PT_TRAVERSAL_PRUNED, HostScene  # noqa: E402
from pathtracer_cuda_interactive_amd import device as dev  # noqa: E402

SC = os.path.join(REPO, "tests", "golden", "scenes")
SIZES = tuple(tuple(int(v) for v in s.split("x")) for s in os.environ.get("PT_TIME_SIZES", "640x480,1280x960").split(","))
ITERATIONS = 5
HBM_BYTES_PER_S = 6.29e12          # measured float4 copy rate of the MI355X


WINDOW_S = float(os.environ.get("PT_TIME_WINDOW", "0.5"))


def timed(fn, window_s=WINDOW_S):
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
    return total_ms / n, n


def main():
    stream = torch.cuda.current_stream().cuda_stream
    for name in sys.argv[1:] or ["cbox", "bunny"]:
        hs = HostScene.load(os.path.join(SC, name + ".pts"))
        d = hs.finalize(PT_BVH_SORT_REFERENCE)
        ds = dev.DeviceScene(d)
        for w, h in SIZES:
            p = hs.render_params(w, h, 4)
            fb = torch.empty((h, w, 3), device="cuda")
            alb, nor, out = torch.empty_like(fb), torch.empty_like(fb), torch.empty_like(fb)
            dep = torch.empty((h, w), device="cuda")
            t_frame, n_frame = timed(lambda: ds.render_into(p, fb.data_ptr(), stream))
            t_aov, n_aov = timed(lambda: ds.render_aov_into(p, alb.data_ptr(), nor.data_ptr(), dep.data_ptr(), 0))
            t_aov_p, _ = timed(lambda: ds.render_aov_into(p, alb.data_ptr(), nor.data_ptr(), dep.data_ptr(), 0,
                                                          traversal=PT_TRAVERSAL_PRUNED))
            t_dn, n_dn = timed(lambda: ds.denoise_into(w, h, fb.data_ptr(), alb.data_ptr(), nor.data_ptr(), dep.data_ptr(),
                                                       out.data_ptr(), stream, iterations=ITERATIONS))
            npix = w * h
            # prep: colour, albedo, normal, depth in (40 B), two records out (32 B); an iteration: two records in, one out (48 B);
            # the last one: two records and the albedo in (44 B), the frame out (12 B)
            moved = npix * (72 + 48 * (ITERATIONS - 1) + 56)
            floor_ms = moved / HBM_BYTES_PER_S * 1e3
            print(f"{name:6s} {w}x{h}: pt_render 4 spp {t_frame:7.3f} ms ({n_frame} calls) | pt_render_aov {t_aov:7.3f} ms ({n_aov}, "
                  f"blocking: includes its host sync; pruned traversal {t_aov_p:7.3f} ms) | pt_denoise {ITERATIONS} iterations {t_dn:7.3f} ms ({n_dn}) = "
                  f"{t_dn / (ITERATIONS + 1) * 1e3:6.1f} us per launch; {48 * npix / 1e6:.1f} MB per iteration, {moved / 1e6:.1f} MB per call "
                  f"= {floor_ms * 1e3:.1f} us at the HBM copy rate ({100 * floor_ms / t_dn:.1f} % of the time taken) | "
                  f"aov + denoise = {(t_aov + t_dn) / t_frame:.2f} x the frame", flush=True)
        ds.close()


if __name__ == "__main__":
    main()
