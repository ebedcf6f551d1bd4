// pt_gradient.h — the per-tile rules of pt_temporal_gradient (include/pt_api.h), written once for the device
// kernels of pt_gradient.hip and for the host twin pt_temporal_gradient_host: the previous frame's noisy colour against a
// re-trace of every stride-th of its rows on the current scene, reduced to one difference and one normaliser per tile of
// stride x stride pixels, smoothed by an unguided à-trous filter on the tile grid and turned into lambda in [0, 1], the share
// of its history that pt_temporal_accumulate_adaptive makes a pixel drop.  The host twin's driver, run_host, is here too.
//
// Every operation is an IEEE fp32 + - * / in the order written (no contraction: the build forbids it), so the device, the
// host twin and a numpy restatement give the same bits.
//
// Layout: one 32-B record per tile, (d.r, d.g, d.b, -, m.r, m.g, m.b, -), ping-ponged between the iterations.
//
// The sparse variant (pt_gradient_pixels, pt_temporal_gradient_sparse) re-traces one pixel per tile in place of a
// row: tile_pixel chooses it, in wrapping uint32 arithmetic, reduce_sparse makes x_0 from it, and filter / lambda_of are shared.
#pragma once

#include <stdint.h>

#include <vector>

#include "../../include/pt_api.h"
#include "pt_math.h"

namespace ptg {

struct alignas(16) Tile { float dr, dg, db, u0, mr, mg, mb, u1; };   // two float4 on the device, the same bytes on the host
static_assert(sizeof(Tile) == 32, "Tile must be 32 bytes");

// pt_gradient_params with the defaults resolved, and the tile grid
struct Resolved {
    int32_t width, height, stride, iterations;
    int32_t r0, tw, th;                      // first sampled row, tiles per tile row, tile rows
    float gain, norm_floor;
};

// The tile grid of a frame at a stride (given, 1..16).  False where the frame has no sampled row.
inline bool tile_grid(int32_t width, int32_t height, int32_t stride, int32_t* r0, int32_t* tw, int32_t* th) {
    *r0 = stride / 2;
    *tw = (width + stride - 1) / stride;
    *th = height > *r0 ? (height - *r0 + stride - 1) / stride : 0;
    return height > *r0;
}

// nullptr, or the name of the first field that is out of range
inline const char* resolve(const pt_gradient_params* g, Resolved* r) {
    auto pos_finite = [](float v) { return v > 0.0f && v <= 3.402823466e+38f; };
    if (g->width <= 0 || g->height <= 0) return "width / height";
    if ((int64_t)g->width * (int64_t)g->height > (1ll << 30)) return "width * height (more than 2^30 pixels)";
    if (g->stride < 0 || g->stride > 16) return "stride";
    if (g->iterations < 0 || g->iterations > 8) return "iterations";
    if (g->gain != 0.0f && !pos_finite(g->gain)) return "gain";
    if (g->norm_floor != 0.0f && !pos_finite(g->norm_floor)) return "norm_floor";
    r->width = g->width; r->height = g->height;
    r->stride = g->stride ? g->stride : 3;
    r->iterations = g->iterations ? g->iterations : 3;
    r->gain = g->gain != 0.0f ? g->gain : 2.0f;
    r->norm_floor = g->norm_floor != 0.0f ? g->norm_floor : 1e-6f;
    if (!tile_grid(r->width, r->height, r->stride, &r->r0, &r->tw, &r->th)) return "height (no sampled row: height <= stride / 2)";
    return nullptr;
}

// x_0 of tile (tx, ty): the sums of the tile's sampled row in both frames, their difference and the larger of the two
PT_HD Tile reduce(const Resolved& r, const float* __restrict__ prev_color, const float* __restrict__ resampled, int tx, int ty) {
    const int y = r.r0 + r.stride * ty;
    const int x_begin = r.stride * tx;
    const int x_end = x_begin + r.stride < r.width ? x_begin + r.stride : r.width;
    const float* a = prev_color + 3 * ((size_t)y * (size_t)r.width);
    const float* b = resampled + 3 * ((size_t)ty * (size_t)r.width);
    float ar = 0.0f, ag = 0.0f, ab = 0.0f, br = 0.0f, bg = 0.0f, bb = 0.0f;
    for (int x = x_begin; x < x_end; x++) {
        ar = ar + a[3 * (size_t)x]; ag = ag + a[3 * (size_t)x + 1]; ab = ab + a[3 * (size_t)x + 2];
        br = br + b[3 * (size_t)x]; bg = bg + b[3 * (size_t)x + 1]; bb = bb + b[3 * (size_t)x + 2];
    }
    return Tile{br - ar, bg - ag, bb - ab, 0.0f, ar < br ? br : ar, ag < bg ? bg : ag, ab < bb ? bb : ab, 0.0f};
}

// The pixel of tile t = ty * tw + tx at `seed`: one PCG output step of the tile number on the seed's stream gives an offset in
// the tile, clamped to the frame.  All of it wrapping uint32 arithmetic; the pixel index fits (width * height <= 2^30).
PT_HD uint32_t tile_hash(uint32_t t, uint32_t seed) {
    const uint32_t v = t * 747796405u + (seed * 2891336453u + 1u);
    const uint32_t w = ((v >> ((v >> 28) + 4u)) ^ v) * 277803737u;
    return (w >> 22) ^ w;
}
PT_HD int32_t tile_pixel(const Resolved& r, uint32_t seed, int tx, int ty) {
    const uint32_t h = tile_hash((uint32_t)ty * (uint32_t)r.tw + (uint32_t)tx, seed);
    const int ox = (int)((h & 0xffffu) % (uint32_t)r.stride), oy = (int)((h >> 16) % (uint32_t)r.stride);
    const int x = r.stride * tx + ox < r.width - 1 ? r.stride * tx + ox : r.width - 1;
    const int y = r.stride * ty + oy < r.height - 1 ? r.stride * ty + oy : r.height - 1;
    return y * r.width + x;
}

// x_0 of tile (tx, ty) from its one listed pixel: prev_color at the entry against the tile's re-traced value.  An entry outside
// the frame forms no address; the tile then compares the re-traced value with itself.
PT_HD Tile reduce_sparse(const Resolved& r, const float* __restrict__ prev_color, const int32_t* __restrict__ pixels,
                         const float* __restrict__ resampled, int tx, int ty) {
    const size_t t = (size_t)ty * (size_t)r.tw + (size_t)tx;
    const int32_t e = pixels[t];
    const float* b = resampled + 3 * t;
    const float* a = e >= 0 && e < r.width * r.height ? prev_color + 3 * (size_t)e : b;
    const float ar = a[0], ag = a[1], ab = a[2], br = b[0], bg = b[1], bb = b[2];
    return Tile{br - ar, bg - ag, bb - ab, 0.0f, ar < br ? br : ar, ag < bg ? bg : ag, ab < bb ? bb : ab, 0.0f};
}

// One iteration at tile (tx, ty): 25 taps at `spacing` on the tile grid, a tap outside the grid skipped before its address is formed
PT_HD Tile filter(const Tile* __restrict__ x, int tx, int ty, int tw, int th, int spacing) {
    const float h[5] = {1.0f / 16.0f, 1.0f / 4.0f, 3.0f / 8.0f, 1.0f / 4.0f, 1.0f / 16.0f};
    float dr = 0.0f, dg = 0.0f, db = 0.0f, mr = 0.0f, mg = 0.0f, mb = 0.0f, wsum = 0.0f;
#pragma unroll
    for (int dy = -2; dy <= 2; dy++) {
        const int qy = ty + spacing * dy;
        if (qy < 0 || qy >= th) continue;
#pragma unroll
        for (int dx = -2; dx <= 2; dx++) {
            const int qx = tx + spacing * dx;
            if (qx < 0 || qx >= tw) continue;
            const Tile q = x[(size_t)qy * (size_t)tw + (size_t)qx];
            const float w = h[dy + 2] * h[dx + 2];
            dr = dr + q.dr * w; dg = dg + q.dg * w; db = db + q.db * w;
            mr = mr + q.mr * w; mg = mg + q.mg * w; mb = mb + q.mb * w;
            wsum = wsum + w;
        }
    }
    const float inv = 1.0f / wsum;
    return Tile{dr * inv, dg * inv, db * inv, 0.0f, mr * inv, mg * inv, mb * inv, 0.0f};
}

// lambda of a tile from its last record
PT_HD float lambda_of(const Tile& t, float gain, float norm_floor) {
    const float rr = __builtin_fabsf(t.dr) / ptm::fmax2(t.mr, norm_floor);
    const float rg = __builtin_fabsf(t.dg) / ptm::fmax2(t.mg, norm_floor);
    const float rb = __builtin_fabsf(t.db) / ptm::fmax2(t.mb, norm_floor);
    return ptm::fmin2(gain * ptm::fmax2(ptm::fmax2(rr, rg), rb), 1.0f);
}

// Device side (pt_gradient.hip).  xa / xb: tw * th records each, device memory owned by the caller (the scene handle); the
// three frames: device pointers.  Enqueues 1 + iterations kernels on `stream`, no host sync.  Returns a hipError_t.
int run_device(const Resolved& r, const float* prev_color, const float* resampled, float* lambda_out, void* xa, void* xb, void* hip_stream);
// The sparse variant: pixels [th * tw] and resampled [th * tw, 3] in place of the rows.  The same number of kernels.
int run_device_sparse(const Resolved& r, const float* prev_color, const int32_t* pixels, const float* resampled, float* lambda_out, void* xa,
                      void* xb, void* hip_stream);
// pixels_out [th * tw] = tile_pixel of every tile: one kernel on `stream`, no host sync.  Returns a hipError_t.
int pixels_device(const Resolved& r, uint32_t seed, int32_t* pixels_out, void* hip_stream);

// Host twins: the same functions over the tile grid, pass by pass.  filter_host: the iterations and the final step on x_0 = xa.
inline void filter_host(const Resolved& r, std::vector<Tile>& xa, float* lambda_out) {
    const size_t ntiles = (size_t)r.tw * (size_t)r.th;
    std::vector<Tile> xb(ntiles);
    Tile* xs[2] = {xa.data(), xb.data()};
    for (int k = 0; k < r.iterations; k++) {
        const Tile* src = xs[k & 1];
        Tile* dst = xs[(k + 1) & 1];
        for (int ty = 0; ty < r.th; ty++)
            for (int tx = 0; tx < r.tw; tx++) dst[(size_t)ty * r.tw + tx] = filter(src, tx, ty, r.tw, r.th, 1 << k);
    }
    const Tile* last = xs[r.iterations & 1];
    for (size_t t = 0; t < ntiles; t++) lambda_out[t] = lambda_of(last[t], r.gain, r.norm_floor);
}
inline void run_host(const Resolved& r, const float* prev_color, const float* resampled, float* lambda_out) {
    std::vector<Tile> xa((size_t)r.tw * (size_t)r.th);
    for (int ty = 0; ty < r.th; ty++)
        for (int tx = 0; tx < r.tw; tx++) xa[(size_t)ty * r.tw + tx] = reduce(r, prev_color, resampled, tx, ty);
    filter_host(r, xa, lambda_out);
}
inline void run_host_sparse(const Resolved& r, const float* prev_color, const int32_t* pixels, const float* resampled, float* lambda_out) {
    std::vector<Tile> xa((size_t)r.tw * (size_t)r.th);
    for (int ty = 0; ty < r.th; ty++)
        for (int tx = 0; tx < r.tw; tx++) xa[(size_t)ty * r.tw + tx] = reduce_sparse(r, prev_color, pixels, resampled, tx, ty);
    filter_host(r, xa, lambda_out);
}
inline void pixels_host(const Resolved& r, uint32_t seed, int32_t* pixels_out) {
    for (int ty = 0; ty < r.th; ty++)
        for (int tx = 0; tx < r.tw; tx++) pixels_out[(size_t)ty * r.tw + tx] = tile_pixel(r, seed, tx, ty);
}

}  // namespace ptg
