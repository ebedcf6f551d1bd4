// pt_gradient.hip — the kernels of pt_temporal_gradient, pt_gradient_pixels and pt_temporal_gradient_sparse and their device
// drivers (the rules and the host twins' drivers: pt_gradient.h).
//
// One thread per tile of the gradient grid, the 64 x 4 launch tiles of pt_tile.h: a wave covers 64 consecutive tiles of a tile
// row, so the records it writes are 2 KiB of consecutive bytes and the two record halves of a tap are consecutive per wave at
// every spacing.  No LDS, no scratch.  The grid is 1 / stride^2 of the frame (214 x 160 tiles for 640 x 480 at stride 3): the
// records stay in L2 between the passes.
#include <hip/hip_runtime.h>

#include "pt_gradient.h"
#include "pt_tile.h"

namespace ptg {

namespace {

__global__ __launch_bounds__(pttile::kTileThreads) void reduce_kernel(Resolved r, const float* __restrict__ prev_color,
                                                                       const float* __restrict__ resampled, Tile* __restrict__ x0) {
    int tx, ty;
    if (!pttile::pixel(r.tw, r.th, tx, ty)) return;
    x0[(size_t)ty * (size_t)r.tw + (size_t)tx] = reduce(r, prev_color, resampled, tx, ty);
}

// The sparse variant: the pixel of every tile, 4 consecutive bytes per lane, and x_0 from that one pixel.  The
// gather of prev_color is 12 bytes per lane at a stride of about 12 * stride bytes along a wave.
__global__ __launch_bounds__(pttile::kTileThreads) void pixels_kernel(Resolved r, uint32_t seed, int32_t* __restrict__ pixels_out) {
    int tx, ty;
    if (!pttile::pixel(r.tw, r.th, tx, ty)) return;
    pixels_out[(size_t)ty * (size_t)r.tw + (size_t)tx] = tile_pixel(r, seed, tx, ty);
}

__global__ __launch_bounds__(pttile::kTileThreads) void reduce_sparse_kernel(Resolved r, const float* __restrict__ prev_color,
                                                                              const int32_t* __restrict__ pixels,
                                                                              const float* __restrict__ resampled, Tile* __restrict__ x0) {
    int tx, ty;
    if (!pttile::pixel(r.tw, r.th, tx, ty)) return;
    x0[(size_t)ty * (size_t)r.tw + (size_t)tx] = reduce_sparse(r, prev_color, pixels, resampled, tx, ty);
}

// One iteration.  LAST: the iteration that writes lambda instead of the next record.
template <bool LAST>
__global__ __launch_bounds__(pttile::kTileThreads) void filter_kernel(const Tile* __restrict__ x, int tw, int th, int spacing, float gain,
                                                                       float norm_floor, Tile* __restrict__ x_next,
                                                                       float* __restrict__ lambda_out) {
    int tx, ty;
    if (!pttile::pixel(tw, th, tx, ty)) return;
    const Tile t = filter(x, tx, ty, tw, th, spacing);
    const size_t p = (size_t)ty * (size_t)tw + (size_t)tx;
    if (LAST) lambda_out[p] = lambda_of(t, gain, norm_floor);
    else x_next[p] = t;
}

// the iterations on x_0 = xs[0], behind either reduce
int filter_device(const Resolved& r, Tile* const (&xs)[2], float* lambda_out, hipStream_t stream) {
    const dim3 grid = pttile::grid(r.tw, r.th), block(pttile::kTileThreads);
    for (int k = 0; k < r.iterations; k++) {
        const bool last = k == r.iterations - 1;
        hipLaunchKernelGGL(last ? filter_kernel<true> : filter_kernel<false>, grid, block, 0, stream, (const Tile*)xs[k & 1], r.tw, r.th,
                           1 << k, r.gain, r.norm_floor, xs[(k + 1) & 1], lambda_out);
    }
    return (int)hipGetLastError();
}

}  // namespace

int run_device(const Resolved& r, const float* prev_color, const float* resampled, float* lambda_out, void* xa, void* xb, void* hip_stream) {
    hipStream_t stream = reinterpret_cast<hipStream_t>(hip_stream);
    Tile* const xs[2] = {reinterpret_cast<Tile*>(xa), reinterpret_cast<Tile*>(xb)};
    hipLaunchKernelGGL(reduce_kernel, pttile::grid(r.tw, r.th), dim3(pttile::kTileThreads), 0, stream, r, prev_color, resampled, xs[0]);
    return filter_device(r, xs, lambda_out, stream);
}

int run_device_sparse(const Resolved& r, const float* prev_color, const int32_t* pixels, const float* resampled, float* lambda_out, void* xa,
                      void* xb, void* hip_stream) {
    hipStream_t stream = reinterpret_cast<hipStream_t>(hip_stream);
    Tile* const xs[2] = {reinterpret_cast<Tile*>(xa), reinterpret_cast<Tile*>(xb)};
    hipLaunchKernelGGL(reduce_sparse_kernel, pttile::grid(r.tw, r.th), dim3(pttile::kTileThreads), 0, stream, r, prev_color, pixels, resampled,
                       xs[0]);
    return filter_device(r, xs, lambda_out, stream);
}

int pixels_device(const Resolved& r, uint32_t seed, int32_t* pixels_out, void* hip_stream) {
    hipLaunchKernelGGL(pixels_kernel, pttile::grid(r.tw, r.th), dim3(pttile::kTileThreads), 0, reinterpret_cast<hipStream_t>(hip_stream), r, seed,
                       pixels_out);
    return (int)hipGetLastError();
}

}  // namespace ptg
