// pt_denoise.hip — kernels of pt_denoise and pt_denoise_variance and the host twins' driver loops (the rules themselves:
// pt_denoise.h).
//
// One thread per pixel, 64 x 4 pixel tiles: a wave covers 64 consecutive pixels of a row, so the two record loads of a tap
// are 1 KiB of consecutive bytes per wave at every spacing (the spacing moves the whole row segment, not the lanes apart),
// and the five taps of a tap row overlap in all but 2 * spacing records.  A frame's records (32 B per pixel read, 16 B written
// per iteration) stay in L2 / Infinity Cache between the passes.
#include <hip/hip_runtime.h>

#include <vector>

#include "pt_denoise.h"

namespace ptdn {

namespace {

constexpr int kTileW = 64, kTileH = 4;

__global__ __launch_bounds__(kTileW * kTileH) void prep_kernel(const float* __restrict__ color, const float* __restrict__ albedo,
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

// LAST: the iteration that writes the caller's frame (x * a') instead of the next colour record
template <bool COLOR, bool LAST>
__global__ __launch_bounds__(kTileW * kTileH) void filter_kernel(const float4* __restrict__ guide, const float4* __restrict__ x,
                                                                  int width, int height, int spacing, int normal_power_log2,
                                                                  float kz, float kc, float4* __restrict__ x_next,
                                                                  const float* __restrict__ albedo, float albedo_floor,
                                                                  float* __restrict__ out) {
    const int px = blockIdx.x * kTileW + (threadIdx.x & (kTileW - 1));
    const int py = blockIdx.y * kTileH + (threadIdx.x / kTileW);
    if (px >= width || py >= height) return;
    const Rec r = dn_filter<COLOR>(guide, x, px, py, width, height, spacing, normal_power_log2, kz, kc);
    const size_t p = (size_t)py * (size_t)width + (size_t)px;
    if (LAST) {
        const float a[3] = {albedo[3 * p], albedo[3 * p + 1], albedo[3 * p + 2]};
        float o[3];
        dn_store(r, a, albedo_floor, o);
        out[3 * p] = o[0]; out[3 * p + 1] = o[1]; out[3 * p + 2] = o[2];
    } else {
        x_next[p] = make_float4(r.x, r.y, r.z, r.w);
    }
}

// pt_denoise_variance: guide record, x_0 and the initial variance in one pass; the same tile shape as the filter, because a
// pixel with a short history gathers a 7 x 7 window of its neighbours' inputs
__global__ __launch_bounds__(kTileW * kTileH) void vprep_kernel(VResolved r, const float* __restrict__ color,
                                                                 const float* __restrict__ albedo, const float* __restrict__ normal,
                                                                 const float* __restrict__ depth, const float* __restrict__ moments,
                                                                 const float* __restrict__ hist_len, float4* __restrict__ guide,
                                                                 float4* __restrict__ x0) {
    const int px = blockIdx.x * kTileW + (threadIdx.x & (kTileW - 1));
    const int py = blockIdx.y * kTileH + (threadIdx.x / kTileW);
    if (px >= r.width || py >= r.height) return;
    Rec g, x;
    vdn_prep(r, color, albedo, normal, depth, moments, hist_len, px, py, g, x);
    const size_t p = (size_t)py * (size_t)r.width + (size_t)px;
    guide[p] = make_float4(g.x, g.y, g.z, g.w);
    x0[p] = make_float4(x.x, x.y, x.z, x.w);
}

// LAST: the iteration that writes the caller's frame (x * a') and variance instead of the next colour record
template <bool LAST>
__global__ __launch_bounds__(kTileW * kTileH) void vfilter_kernel(const float4* __restrict__ guide, const float4* __restrict__ x,
                                                                   int width, int height, int spacing, int normal_power_log2,
                                                                   float kz, float sl2, float var_floor, float4* __restrict__ x_next,
                                                                   const float* __restrict__ albedo, float albedo_floor,
                                                                   float* __restrict__ out, float* __restrict__ out_variance) {
    const int px = blockIdx.x * kTileW + (threadIdx.x & (kTileW - 1));
    const int py = blockIdx.y * kTileH + (threadIdx.x / kTileW);
    if (px >= width || py >= height) return;
    const Rec r = vdn_filter(guide, x, px, py, width, height, spacing, normal_power_log2, kz, sl2, var_floor);
    const size_t p = (size_t)py * (size_t)width + (size_t)px;
    if (LAST) {
        const float a[3] = {albedo[3 * p], albedo[3 * p + 1], albedo[3 * p + 2]};
        float o[3];
        vdn_store(r, a, albedo_floor, o, out_variance ? out_variance + p : nullptr);
        out[3 * p] = o[0]; out[3 * p + 1] = o[1]; out[3 * p + 2] = o[2];
    } else {
        x_next[p] = make_float4(r.x, r.y, r.z, r.w);
    }
}

}  // namespace

int run_device_variance(const VResolved& r, const float* color, const float* albedo, const float* normal, const float* depth,
                        const float* moments, const float* hist_len, float* out, float* out_variance, void* guide_v, void* xa_v,
                        void* xb_v, void* hip_stream) {
    hipStream_t stream = reinterpret_cast<hipStream_t>(hip_stream);
    float4* guide = reinterpret_cast<float4*>(guide_v);
    float4* xs[2] = {reinterpret_cast<float4*>(xa_v), reinterpret_cast<float4*>(xb_v)};
    const int threads = kTileW * kTileH;
    const dim3 grid((unsigned)((r.width + kTileW - 1) / kTileW), (unsigned)((r.height + kTileH - 1) / kTileH));
    hipLaunchKernelGGL(vprep_kernel, grid, dim3(threads), 0, stream, r, color, albedo, normal, depth, moments, hist_len, guide, xs[0]);
    for (int k = 0; k < r.iterations; k++) {
        const bool last = k == r.iterations - 1;
        const float4* src = xs[k & 1];
        float4* dst = xs[(k + 1) & 1];
        hipLaunchKernelGGL(last ? vfilter_kernel<true> : vfilter_kernel<false>, grid, dim3(threads), 0, stream, (const float4*)guide,
                           src, r.width, r.height, 1 << k, r.normal_power_log2, r.kz, r.sl2, r.var_floor, dst, albedo, r.albedo_floor,
                           out, out_variance);
    }
    return (int)hipGetLastError();
}

void run_host_variance(const VResolved& r, const float* color, const float* albedo, const float* normal, const float* depth,
                       const float* moments, const float* hist_len, float* out, float* out_variance) {
    const size_t npix = (size_t)r.width * (size_t)r.height;
    std::vector<Rec> guide(npix), xa(npix), xb(npix);
    for (int py = 0; py < r.height; py++)
        for (int px = 0; px < r.width; px++) {
            const size_t p = (size_t)py * r.width + px;
            vdn_prep(r, color, albedo, normal, depth, moments, hist_len, px, py, guide[p], xa[p]);
        }
    Rec* xs[2] = {xa.data(), xb.data()};
    for (int k = 0; k < r.iterations; k++) {
        const Rec* src = xs[k & 1];
        Rec* dst = xs[(k + 1) & 1];
        for (int py = 0; py < r.height; py++)
            for (int px = 0; px < r.width; px++)
                dst[(size_t)py * r.width + px] = vdn_filter(guide.data(), src, px, py, r.width, r.height, 1 << k, r.normal_power_log2,
                                                            r.kz, r.sl2, r.var_floor);
    }
    const Rec* last = xs[r.iterations & 1];
    for (size_t p = 0; p < npix; p++)
        vdn_store(last[p], albedo + 3 * p, r.albedo_floor, out + 3 * p, out_variance ? out_variance + p : nullptr);
}

int run_device(const Resolved& r, const float* color, const float* albedo, const float* normal, const float* depth, float* out,
               void* guide_v, void* xa_v, void* xb_v, void* hip_stream) {
    hipStream_t stream = reinterpret_cast<hipStream_t>(hip_stream);
    float4* guide = reinterpret_cast<float4*>(guide_v);
    float4* xs[2] = {reinterpret_cast<float4*>(xa_v), reinterpret_cast<float4*>(xb_v)};
    const uint32_t npix = (uint32_t)r.width * (uint32_t)r.height;
    const int threads = kTileW * kTileH;
    hipLaunchKernelGGL(prep_kernel, dim3((npix + threads - 1) / threads), dim3(threads), 0, stream, color, albedo, normal, depth,
                       npix, r.scale, r.albedo_floor, guide, xs[0]);
    const dim3 grid((unsigned)((r.width + kTileW - 1) / kTileW), (unsigned)((r.height + kTileH - 1) / kTileH));
    for (int k = 0; k < r.iterations; k++) {
        const bool last = k == r.iterations - 1;
        const float4* src = xs[k & 1];
        float4* dst = xs[(k + 1) & 1];
        auto fn = r.color_term ? (last ? filter_kernel<true, true> : filter_kernel<true, false>)
                               : (last ? filter_kernel<false, true> : filter_kernel<false, false>);
        hipLaunchKernelGGL(fn, grid, dim3(threads), 0, stream, (const float4*)guide, src, r.width, r.height, 1 << k,
                           r.normal_power_log2, r.kz, r.kc[k], dst, albedo, r.albedo_floor, out);
    }
    return (int)hipGetLastError();
}

void run_host(const Resolved& r, const float* color, const float* albedo, const float* normal, const float* depth, float* out) {
    const size_t npix = (size_t)r.width * (size_t)r.height;
    std::vector<Rec> guide(npix), xa(npix), xb(npix);
    for (size_t p = 0; p < npix; p++)
        dn_prep(color + 3 * p, albedo + 3 * p, normal + 3 * p, depth[p], r.scale, r.albedo_floor, guide[p], xa[p]);
    Rec* xs[2] = {xa.data(), xb.data()};
    for (int k = 0; k < r.iterations; k++) {
        const Rec* src = xs[k & 1];
        Rec* dst = xs[(k + 1) & 1];
        for (int py = 0; py < r.height; py++)
            for (int px = 0; px < r.width; px++)
                dst[(size_t)py * r.width + px] =
                    r.color_term ? dn_filter<true>(guide.data(), src, px, py, r.width, r.height, 1 << k, r.normal_power_log2, r.kz, r.kc[k])
                                 : dn_filter<false>(guide.data(), src, px, py, r.width, r.height, 1 << k, r.normal_power_log2, r.kz, r.kc[k]);
    }
    const Rec* last = xs[r.iterations & 1];
    for (size_t p = 0; p < npix; p++) dn_store(last[p], albedo + 3 * p, r.albedo_floor, out + 3 * p);
}

}  // namespace ptdn
