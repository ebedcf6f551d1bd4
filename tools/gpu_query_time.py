"""The lane-refilling query kernel against the one-shot kernels it stands beside: HIP-event times, warm, every
figure over a window of at least 0.5 s.  Runs on the GPU box.
  pt_render_guides (blocking: its time includes the host sync of every call) against pt_render_guides_async (enqueued back to
  back on one stream) on cbox and bunny at 640x480 and 1280x960, six buffers;
  pt_debug_intersect against pt_trace_rays, closest and any, on bunny for 32,768 and 1,048,576 random rays: host pointers
  (wall time per call: staging and copies included on both sides) and, pt_trace_rays alone, device pointers (events).
The asynchronous calls are also timed at explicit grids (option "query_blocks") and refill thresholds ("query_refill"), which
is what the automatic choices rest on.
Usage: python tools/gpu_query_time.py [cbox bunny ...]      PT_TIME_WINDOW=0.02 shortens the windows, PT_TIME_SIZES=640x480
picks the frame sizes, PT_TIME_RAYS=32768 the ray counts"""
import os
import sys
import time

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
from pathtracer_cuda_interactive_amd import PT_BVH_SORT_REFERENCE, PT_QUERY_ANY, PT_QUERY_CLOSEST, HostScene  # noqa: E402
from pathtracer_cuda_interactive_amd import device as dev  # noqa: E402

SC = os.path.join(REPO, "tests", "golden", "scenes")
SIZES = tuple(tuple(int(v) for v in s.split("x")) for s in os.environ.get("PT_TIME_SIZES", "640x480,1280x960").split(","))
RAYS = tuple(int(v) for v in os.environ.get("PT_TIME_RAYS", "32768,1048576").split(","))
WINDOW_S = float(os.environ.get("PT_TIME_WINDOW", "0.5"))
GRIDS = (256, 512, 1024, 2048)
REFILLS = (1, 16, 32, 64)


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
    return total_ms / n


def walled(fn, window_s=WINDOW_S):
    """Mean wall time of a blocking fn() in ms: warm, then calls until the window is filled."""
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    n, t0 = 0, time.perf_counter()
    while time.perf_counter() - t0 < window_s:
        fn()
        n += 1
    return (time.perf_counter() - t0) / n * 1e3


def random_rays(n):
    rng = np.random.default_rng(5)
    o = (rng.standard_normal((n, 3)) * 2).astype(np.float32)
    t = (rng.standard_normal((n, 3)) * 0.7).astype(np.float32)
    dirs = t - o
    dirs /= np.linalg.norm(dirs, axis=1, keepdims=True)
    return np.concatenate([o, dirs.astype(np.float32), np.full((n, 1), 1e-4, np.float32), np.full((n, 1), 3.0e38, np.float32)],
                          axis=1).astype(np.float32)


def grids(ds, fn):
    """fn() timed on the automatic launch, then at every grid of GRIDS and every refill threshold of REFILLS with the other
    knob automatic."""
    parts = [f"{timed(fn):7.3f} ms ({ds.info('query_grid')} blocks)", "\n         by query_blocks:"]
    for g in GRIDS:
        ds.set_option("query_blocks", g)
        parts.append(f"{g} {timed(fn):6.3f}")
    ds.set_option("query_blocks", 0)
    parts.append("\n         by query_refill:")
    for r in REFILLS:
        ds.set_option("query_refill", r)
        parts.append(f"{r} {timed(fn):6.3f}")
    ds.set_option("query_refill", 0)
    return " ".join(parts)


def main():
    stream = torch.cuda.current_stream().cuda_stream
    for name in sys.argv[1:] or ["cbox", "bunny"]:
        hs = HostScene.load(os.path.join(SC, name + ".pts"))
        d = hs.finalize(PT_BVH_SORT_REFERENCE)
        ds = dev.DeviceScene(d)
        print(f"{name}: query_chunk {ds.info('query_chunk')}, {ds.info('num_cus')} CUs, stack_entries {ds.info('stack_entries')}", flush=True)
        for w, h in SIZES:
            p = hs.render_params(w, h, 1)
            prev = dev.translated_params(p, np.array([0.01, 0.005, -0.01]))
            bufs = {"albedo": torch.empty((h, w, 3), device="cuda"), "normal": torch.empty((h, w, 3), device="cuda"),
                    "depth": torch.empty((h, w), device="cuda"), "prim": torch.empty((h, w), device="cuda", dtype=torch.int32),
                    "motion": torch.empty((h, w, 2), device="cuda"), "prev_depth": torch.empty((h, w), device="cuda")}
            ptrs = {k + "_ptr": b.data_ptr() for k, b in bufs.items()}
            t_block = timed(lambda: ds.render_guides_into(p, prev, **ptrs))
            one = p.copy()                                            # one row: what a blocking call costs beside its kernel
            one.row_begin, one.row_end = 0, 1
            t_row = timed(lambda: ds.render_guides_into(one, prev, **ptrs))
            ds.set_option("query_guides", 2)
            t_shot = timed(lambda: ds.render_guides_async_into(p, prev, stream=stream, **ptrs))
            ds.set_option("query_guides", 1)
            print(f"{name:6s} {w}x{h}: pt_render_guides {t_block:7.3f} ms (blocking; a one-row call {t_row:7.3f} ms) | "
                  f"pt_render_guides_async, one-shot kernel: {t_shot:7.3f} ms | refilling kernel: "
                  + grids(ds, lambda: ds.render_guides_async_into(p, prev, stream=stream, **ptrs)), flush=True)
            ds.set_option("query_guides", 0)
        if name == "bunny":
            for n in RAYS:
                rays = random_rays(n)
                d_rays = torch.from_numpy(rays).cuda()
                t_out = torch.empty((n, 3), device="cuda")
                p_out = torch.empty((n,), device="cuda", dtype=torch.int32)
                w_dbg = walled(lambda: ds.intersect(rays))
                w_closest = walled(lambda: ds.trace_rays(rays))
                w_any = walled(lambda: ds.trace_rays(rays, mode=PT_QUERY_ANY))
                print(f"{name:6s} {n} rays, host pointers, wall per call: pt_debug_intersect {w_dbg:8.3f} ms | pt_trace_rays closest "
                      f"{w_closest:8.3f} ms | any {w_any:8.3f} ms", flush=True)
                for mode, label in ((PT_QUERY_CLOSEST, "closest"), (PT_QUERY_ANY, "any")):
                    print(f"{name:6s} {n} rays, device pointers, pt_trace_rays {label}: "
                          + grids(ds, lambda: ds.trace_rays_into(d_rays.data_ptr(), n, t_out.data_ptr(), p_out.data_ptr(), mode=mode,
                                                                 stream=stream)), flush=True)
        ds.close()


if __name__ == "__main__":
    main()
