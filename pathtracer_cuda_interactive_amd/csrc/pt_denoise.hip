// pt_denoise.hip — kernels of pt_denoise and pt_denoise_variance and their device driver (the rules themselves and the host
// twins' driver: pt_denoise.h).
//
// One thread per pixel, the 64 x 4 pixel tiles of pt_tile.h: a wave covers 64 consecutive pixels of a row, so the two record
// loads of a tap are 1 KiB of consecutive bytes per wave at every spacing (the spacing moves the whole row segment, not the
// lanes apart), and the five taps of a tap row overlap in all but 2 * spacing records.  A frame's records (32 B per pixel
// read, 16 B written per iteration) stay in L2 / Infinity Cache between the passes.
#include <hip/hip_runtime.h>

#include "pt_denoise.h"
#include "pt_tile.h"

namespace ptdn {

namespace {

__global__ __launch_bounds__(pttile::kTileThreads) void prep_kernel(const float* __restrict__ color, const float* __restrict__ albedo,
                                                                const float* __restrict__ normal, const float* __restrict__ depth,
                                                                uint32_t npix, float scale, float albedo_floor,
                                                                float4* __restrict__ guide, float4* __restrict__ x0) {
    const uint32_t p = blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= npix) return;
    const float c[3] = {color[3 * (size_t)p], color[3 * (size_t)p + 1], color[3 * (size_t)p + 2]};
    const float a[3] = {albedo[3 * (size_t)p], albedo[3 * (size_t)p + 1], albedo[3 * (size_t)p + 2]};
    const float n[3] = {normal[3 * (size_t)p], normal[3 * (size_t)p + 1], normal[3 * (size_t)p + 2]};
    Rec g, x;
    dn_prep(c, a, n, depth[p], scale, albedo_floor, g, x);
    guide[p] = make_float4(g.x, g.y, g.z, g.w);
    x0[p] = make_float4(x.x, x.y, x.z, x.w);
}

// pt_denoise_variance: guide record, x_0 and the initial variance in one pass; the same tile shape as the filter, because a
// pixel with a short history gathers a 7 x 7 window of its neighbours' inputs
__global__ __launch_bounds__(pttile::kTileThreads) void vprep_kernel(Resolved r, const float* __restrict__ color,
                                                                      const float* __restrict__ albedo,
                                                                      const float* __restrict__ normal,
                                                                      const float* __restrict__ depth,
                                                                      const float* __restrict__ moments,
                                                                      const float* __restrict__ hist_len, float4* __restrict__ guide,
                                                                      float4* __restrict__ x0) {
    int px, py;
    if (!pttile::pixel(r.width, r.height, px, py)) return;
    Rec g, x;
    vdn_prep(r, color, albedo, normal, depth, moments, hist_len, px, py, g, x);
    const size_t p = (size_t)py * (size_t)r.width + (size_t)px;
    guide[p] = make_float4(g.x, g.y, g.z, g.w);
    x0[p] = make_float4(x.x, x.y, x.z, x.w);
}

// One iteration in mode M.  LAST: the iteration that writes the caller's frame (x * a') and, in the variance mode, the
// variance instead of the next colour record.  out_variance: Variance only, may be null.
template <Mode M, bool LAST>
__global__ __launch_bounds__(pttile::kTileThreads) void filter_kernel(const float4* __restrict__ guide, const float4* __restrict__ x,
                                                                       int width, int height, int spacing, int normal_power_log2,
                                                                       float kz, float kl, float var_floor,
                                                                       float4* __restrict__ x_next, const float* __restrict__ albedo,
                                                                       float albedo_floor, float* __restrict__ out,
                                                                       float* __restrict__ out_variance) {
    int px, py;
    if (!pttile::pixel(width, height, px, py)) return;
    const Rec r = filter<M>(guide, x, px, py, width, height, spacing, normal_power_log2, kz, kl, var_floor);
    const size_t p = (size_t)py * (size_t)width + (size_t)px;
    if (LAST) {
        const float a[3] = {albedo[3 * p], albedo[3 * p + 1], albedo[3 * p + 2]};
        float o[3];
        if constexpr (M == Mode::Variance) vdn_store(r, a, albedo_floor, o, out_variance ? out_variance + p : nullptr);
        else dn_store(r, a, albedo_floor, o);
        out[3 * p] = o[0]; out[3 * p + 1] = o[1]; out[3 * p + 2] = o[2];
    } else {
        x_next[p] = make_float4(r.x, r.y, r.z, r.w);
    }
}

template <Mode M>
constexpr auto filter_fn(bool last) { return last ? filter_kernel<M, true> : filter_kernel<M, false>; }

}  // namespace

int run_device(const Resolved& r, const Frames& f, void* guide_v, void* xa_v, void* xb_v, void* hip_stream) {
    hipStream_t stream = reinterpret_cast<hipStream_t>(hip_stream);
    float4* guide = reinterpret_cast<float4*>(guide_v);
    float4* xs[2] = {reinterpret_cast<float4*>(xa_v), reinterpret_cast<float4*>(xb_v)};
    const dim3 grid = pttile::grid(r.width, r.height), block(pttile::kTileThreads);
    if (r.mode == Mode::Variance) {
        hipLaunchKernelGGL(vprep_kernel, grid, block, 0, stream, r, f.color, f.albedo, f.normal, f.depth, f.moments, f.hist_len, guide,
                           xs[0]);
    } else {
        const uint32_t npix = (uint32_t)r.width * (uint32_t)r.height;
        hipLaunchKernelGGL(prep_kernel, dim3((npix + block.x - 1) / block.x), block, 0, stream, f.color, f.albedo, f.normal, f.depth,
                           npix, r.scale, r.albedo_floor, guide, xs[0]);
    }
    for (int k = 0; k < r.iterations; k++) {
        const bool last = k == r.iterations - 1;
        const float4* src = xs[k & 1];
        float4* dst = xs[(k + 1) & 1];
        auto fn = r.mode == Mode::Variance ? filter_fn<Mode::Variance>(last)
                  : r.mode == Mode::Color  ? filter_fn<Mode::Color>(last)
                                           : filter_fn<Mode::Plain>(last);
        hipLaunchKernelGGL(fn, grid, block, 0, stream, (const float4*)guide, src, r.width, r.height, 1 << k, r.normal_power_log2, r.kz,
                           r.kl[k], r.var_floor, dst, f.albedo, r.albedo_floor, f.out, f.out_variance);
    }
    return (int)hipGetLastError();
}

}  // namespace ptdn
