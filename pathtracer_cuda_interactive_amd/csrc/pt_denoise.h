// pt_denoise.h — the per-pixel rule of pt_denoise (include/pt_api.h), written once for the device kernels
// of pt_denoise.hip and for the host twin pt_denoise_host: an edge-avoiding à-trous filter on albedo-divided colour, guided
// by first-hit normal and depth.
//
// Every operation is an IEEE fp32 + - * / in the order written (no contraction: the build forbids it), so the device, the
// host twin and a numpy restatement give the same bits.  Weights are rational (1 / (1 + x^2 k)) instead of exp for that reason.
//
// Layout: two 16-B records per pixel.
//   guide  (n.x, n.y, n.z, z)      constant over the iterations
//   colour (x.r, x.g, x.b, f)      f = 1 filterable (max albedo channel > 0), 0 not; ping-ponged between the iterations
// One pass packs them (dn_prep), one pass per iteration gathers 25 taps of both (dn_filter); the last iteration multiplies the
// albedo back and writes the caller's frame (dn_store).
#pragma once

#include <stdint.h>

#include "../../include/pt_api.h"
#include "pt_math.h"

namespace ptdn {

struct Rec { float x, y, z, w; };            // 16 B; float4 on the device, the same bytes on the host
static_assert(sizeof(Rec) == 16, "Rec must be 16 bytes");

// pt_denoise_params with the defaults resolved and the per-iteration constants worked out (host side, fp32)
struct Resolved {
    int32_t width, height, iterations, normal_power_log2;
    float scale, albedo_floor;
    float kz;                                // 1 / sigma_z^2
    int32_t color_term;                      // sigma_c != 0
    float kc[8];                             // 1 / (sigma_c 2^-k)^2 per iteration
};

// nullptr, or the name of the first field that is out of range
inline const char* resolve(const pt_denoise_params* d, Resolved* r) {
    auto pos_finite = [](float v) { return v > 0.0f && v <= 3.402823466e+38f; };
    if (d->width <= 0 || d->height <= 0) return "width / height";
    if ((int64_t)d->width * (int64_t)d->height > (1ll << 30)) return "width * height (more than 2^30 pixels)";
    if (d->iterations < 0 || d->iterations > 8) return "iterations";
    if (d->normal_power_log2 < 0 || d->normal_power_log2 > 10) return "normal_power_log2";
    if (d->sigma_z != 0.0f && !pos_finite(d->sigma_z)) return "sigma_z";
    if (d->sigma_c != 0.0f && !pos_finite(d->sigma_c)) return "sigma_c";
    if (d->scale != 0.0f && !pos_finite(d->scale)) return "scale";
    if (d->albedo_floor != 0.0f && !pos_finite(d->albedo_floor)) return "albedo_floor";
    r->width = d->width; r->height = d->height;
    r->iterations = d->iterations ? d->iterations : 5;
    r->normal_power_log2 = d->normal_power_log2;
    r->scale = d->scale != 0.0f ? d->scale : 1.0f;
    r->albedo_floor = d->albedo_floor != 0.0f ? d->albedo_floor : 0.01f;
    const float sz = d->sigma_z != 0.0f ? d->sigma_z : 0.05f;
    r->kz = 1.0f / (sz * sz);
    r->color_term = d->sigma_c != 0.0f;
    for (int k = 0; k < 8; k++) {
        const float sc = d->sigma_c * (1.0f / (float)(1 << k));     // exact: a power of two
        r->kc[k] = r->color_term ? 1.0f / (sc * sc) : 0.0f;
    }
    return nullptr;
}

PT_HD float lum(float r, float g, float b) { return 0.2126f * r + 0.7152f * g + 0.0722f * b; }

PT_HD bool filterable(const float* albedo) { return ptm::fmax2(ptm::fmax2(albedo[0], albedo[1]), albedo[2]) > 0.0f; }

// x_0 and the guide record of one pixel
PT_HD void dn_prep(const float* color, const float* albedo, const float* normal, float depth, float scale, float albedo_floor,
                   Rec& guide, Rec& x0) {
    guide = Rec{normal[0], normal[1], normal[2], depth};
    const float r = color[0] * scale, g = color[1] * scale, b = color[2] * scale;
    if (filterable(albedo))
        x0 = Rec{r / ptm::fmax2(albedo[0], albedo_floor), g / ptm::fmax2(albedo[1], albedo_floor),
                 b / ptm::fmax2(albedo[2], albedo_floor), 1.0f};
    else
        x0 = Rec{r, g, b, 0.0f};
}

// x_{k+1} of pixel (px, py) from the records of iteration k; spacing = 1 << k.  Taps in the order dy = -2..2 (outer),
// dx = -2..2 (inner): the sums are not associative.  Every tap is clipped to the frame before its address is formed.
template <bool COLOR, class R>
PT_HD Rec dn_filter(const R* __restrict__ guide, const R* __restrict__ x, int px, int py, int width, int height, int spacing,
                    int normal_power_log2, float kz, float kc) {
    const size_t p = (size_t)py * (size_t)width + (size_t)px;
    const R xp = x[p];
    if (xp.w == 0.0f) return Rec{xp.x, xp.y, xp.z, 0.0f};
    const R gp = guide[p];
    const float inv_zp = 1.0f / ptm::fmax2(gp.w, 1e-20f);
    const float lp = COLOR ? lum(xp.x, xp.y, xp.z) : 0.0f;
    const float h[5] = {1.0f / 16.0f, 1.0f / 4.0f, 3.0f / 8.0f, 1.0f / 4.0f, 1.0f / 16.0f};
    float sr = 0.0f, sg = 0.0f, sb = 0.0f, wsum = 0.0f;
#pragma unroll
    for (int dy = -2; dy <= 2; dy++) {
        const int qy = py + spacing * dy;
        if (qy < 0 || qy >= height) continue;
        // the ten records of a tap row are loaded before any of them is used (ten loads in flight per lane); a tap outside the
        // frame reads the centre column's record of that row instead and is dropped below
        R xr[5], gr[5];
        bool in[5];
#pragma unroll
        for (int dx = -2; dx <= 2; dx++) {
            const int qx = px + spacing * dx;
            in[dx + 2] = qx >= 0 && qx < width;
            const size_t q = (size_t)qy * (size_t)width + (size_t)(in[dx + 2] ? qx : px);
            xr[dx + 2] = x[q];
            gr[dx + 2] = guide[q];
        }
#pragma unroll
        for (int dx = -2; dx <= 2; dx++) {
            const R xq = xr[dx + 2], gq = gr[dx + 2];
            if (!in[dx + 2] || xq.w == 0.0f) continue;
            float wn = ptm::fmax2(0.0f, gp.x * gq.x + gp.y * gq.y + gp.z * gq.z);
            for (int e = 0; e < normal_power_log2; e++) wn = wn * wn;
            const float rd = (gp.w - gq.w) * inv_zp;
            const float wz = 1.0f / (1.0f + (rd * rd) * kz);
            float w = ((h[dy + 2] * h[dx + 2]) * wn) * wz;
            if (COLOR) {
                const float dl = lp - lum(xq.x, xq.y, xq.z);
                w = w * (1.0f / (1.0f + (dl * dl) * kc));
            }
            sr = sr + xq.x * w; sg = sg + xq.y * w; sb = sb + xq.z * w;
            wsum = wsum + w;
        }
    }
    const float inv = 1.0f / wsum;
    return Rec{sr * inv, sg * inv, sb * inv, 1.0f};
}

// out = x_last * a' for filterable pixels, x_last otherwise
PT_HD void dn_store(const Rec& x, const float* albedo, float albedo_floor, float* out) {
    if (x.w != 0.0f) {
        out[0] = x.x * ptm::fmax2(albedo[0], albedo_floor);
        out[1] = x.y * ptm::fmax2(albedo[1], albedo_floor);
        out[2] = x.z * ptm::fmax2(albedo[2], albedo_floor);
    } else {
        out[0] = x.x; out[1] = x.y; out[2] = x.z;
    }
}

// Device side (pt_denoise.hip).  guide / xa / xb: width * height records each, device memory owned by the caller (the scene
// handle); color .. out: device pointers.  Enqueues 1 + iterations kernels on `stream`, no host sync.  Returns a hipError_t.
int run_device(const Resolved& r, const float* color, const float* albedo, const float* normal, const float* depth, float* out,
               void* guide, void* xa, void* xb, void* hip_stream);
// Host twin: the same three functions over the frame, pass by pass (so `out` may alias `color`).
void run_host(const Resolved& r, const float* color, const float* albedo, const float* normal, const float* depth, float* out);

}  // namespace ptdn
