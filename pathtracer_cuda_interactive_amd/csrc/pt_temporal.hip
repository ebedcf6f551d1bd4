// pt_temporal.hip — kernels of pt_temporal_accumulate and pt_temporal_accumulate_moments and the host twins' loops (the rules
// themselves: pt_temporal.h).
//
// One thread per pixel, 64 x 4 pixel tiles as in pt_denoise.hip: a wave covers 64 consecutive pixels of a row, so its own
// records are consecutive bytes and, where neighbouring pixels move alike, so are the two tap rows it gathers.  No LDS, no
// scratch: at most four taps, each used once.
#include <hip/hip_runtime.h>

#include "pt_temporal.h"

namespace ptt {

namespace {

constexpr int kTileW = 64, kTileH = 4;

__global__ __launch_bounds__(kTileW * kTileH) void accumulate_kernel(Resolved r, const float* __restrict__ normal,
                                                                      const float* __restrict__ motion,
                                                                      const float* __restrict__ prev_depth,
                                                                      const float* __restrict__ hist_color,
                                                                      const float* __restrict__ hist_normal,
                                                                      const float* __restrict__ hist_depth,
                                                                      const float* __restrict__ hist_len, const float* color,
                                                                      float* out_color, float* __restrict__ out_len) {
    const int px = blockIdx.x * kTileW + (threadIdx.x & (kTileW - 1));
    const int py = blockIdx.y * kTileH + (threadIdx.x / kTileW);
    if (px >= r.width || py >= r.height) return;
    accumulate_pixel(r, px, py, normal, motion, prev_depth, hist_color, hist_normal, hist_depth, hist_len, color, out_color, out_len);
}

// pt_temporal_accumulate_moments: the same shape; the pointers travel by value in the kernel's arguments
__global__ __launch_bounds__(kTileW * kTileH) void accumulate_moments_kernel(Resolved r, float albedo_floor, pt_temporal_io io) {
    const int px = blockIdx.x * kTileW + (threadIdx.x & (kTileW - 1));
    const int py = blockIdx.y * kTileH + (threadIdx.x / kTileW);
    if (px >= r.width || py >= r.height) return;
    accumulate_moments_pixel(r, albedo_floor, px, py, io);
}

}  // namespace

int run_device_moments(const Resolved& r, float albedo_floor, const pt_temporal_io& io, void* hip_stream) {
    const dim3 grid((unsigned)((r.width + kTileW - 1) / kTileW), (unsigned)((r.height + kTileH - 1) / kTileH));
    hipLaunchKernelGGL(accumulate_moments_kernel, grid, dim3(kTileW * kTileH), 0, reinterpret_cast<hipStream_t>(hip_stream), r,
                       albedo_floor, io);
    return (int)hipGetLastError();
}

void run_host_moments(const Resolved& r, float albedo_floor, const pt_temporal_io& io) {
    for (int py = 0; py < r.height; py++)
        for (int px = 0; px < r.width; px++) accumulate_moments_pixel(r, albedo_floor, px, py, io);
}

int run_device(const Resolved& r, const float* color, const float* normal, const float* motion, const float* prev_depth,
               const float* hist_color, const float* hist_normal, const float* hist_depth, const float* hist_len,
               float* out_color, float* out_len, void* hip_stream) {
    const dim3 grid((unsigned)((r.width + kTileW - 1) / kTileW), (unsigned)((r.height + kTileH - 1) / kTileH));
    hipLaunchKernelGGL(accumulate_kernel, grid, dim3(kTileW * kTileH), 0, reinterpret_cast<hipStream_t>(hip_stream), r, normal,
                       motion, prev_depth, hist_color, hist_normal, hist_depth, hist_len, color, out_color, out_len);
    return (int)hipGetLastError();
}

void run_host(const Resolved& r, const float* color, const float* normal, const float* motion, const float* prev_depth,
              const float* hist_color, const float* hist_normal, const float* hist_depth, const float* hist_len,
              float* out_color, float* out_len) {
    for (int py = 0; py < r.height; py++)
        for (int px = 0; px < r.width; px++)
            accumulate_pixel(r, px, py, normal, motion, prev_depth, hist_color, hist_normal, hist_depth, hist_len, color, out_color,
                             out_len);
}

}  // namespace ptt
