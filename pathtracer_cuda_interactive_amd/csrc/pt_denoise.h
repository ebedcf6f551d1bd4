// pt_denoise.h — the per-pixel rules of pt_denoise (include/pt_api.h) and pt_denoise_variance,
// written once for the device kernels of pt_denoise.hip and for the host twins pt_denoise_host and pt_denoise_variance_host:
// an edge-avoiding à-trous filter on albedo-divided colour, guided by first-hit normal and depth, and in the variance mode
// by a per-pixel luminance variance that travels through the iterations.  The two calls share one tap walk (filter<Mode>),
// one pair of guide weights (guide_weights), one parameter check (resolve_common) and one host driver (run_host, here, so a
// plain host compile of this header runs what the host twins run: tests/native/post_rules_check.cpp).
//
// Every operation is an IEEE fp32 + - * / in the order written (no contraction: the build forbids it), so the device, the
// host twin and a numpy restatement give the same bits.  Weights are rational (1 / (1 + x^2 k)) instead of exp for that reason.
//
// Layout: two 16-B records per pixel.
//   guide  (n.x, n.y, n.z, z)      constant over the iterations
//   colour (x.r, x.g, x.b, f)      ping-ponged between the iterations.  pt_denoise: f = 1 filterable (max albedo channel > 0),
//                                  0 not.  pt_denoise_variance: f = v >= 0 filterable, the variance of the pixel's luminance;
//                                  v = -1 not filterable
// One pass packs them (dn_prep / vdn_prep), one pass per iteration gathers 25 taps of both (filter; the 3 x 3 variance
// prefilter of the variance mode reads colour records only); the last iteration multiplies the albedo back and writes the
// caller's frame (dn_store / vdn_store).
#pragma once

#include <stdint.h>

#include <vector>

#include "../../include/pt_api.h"
#include "pt_math.h"

namespace ptdn {

struct Rec { float x, y, z, w; };            // 16 B; float4 on the device, the same bytes on the host
static_assert(sizeof(Rec) == 16, "Rec must be 16 bytes");

// What a tap's weight is made of besides the kernel h and the guide weights, and what the colour record's fourth word means.
enum class Mode : int32_t {
    Plain,                                   // pt_denoise, sigma_c == 0
    Color,                                   // pt_denoise, sigma_c != 0: 1 / (1 + dl^2 kc_k)
    Variance,                                // pt_denoise_variance: den / (den + dl^2), den = sigma_l^2 g + var_floor
};

// pt_denoise_params or pt_vdenoise_params with the defaults resolved and the per-iteration constants worked out (host side, fp32)
struct Resolved {
    int32_t width, height, iterations, normal_power_log2;
    float scale, albedo_floor;
    float kz;                                // 1 / sigma_z^2
    Mode mode;
    float kl[8];                             // per iteration.  Color: 1 / (sigma_c 2^-k)^2; Variance: sigma_l * sigma_l; Plain: 0
    float min_history;                       // Variance: (float)min_history: exact, at most 65536
    float var_floor;                         // Variance
};

inline bool pos_finite(float v) { return v > 0.0f && v <= 3.402823466e+38f; }

// The fields the two parameter structs share, checked in the order of the structs; sigma_2 is the field between sigma_z and
// scale (sigma_c / sigma_l).  nullptr, or the name of the first field that is out of range.
template <class P>
inline const char* resolve_common(const P* d, float sigma_2, const char* sigma_2_name, Resolved* r) {
    if (d->width <= 0 || d->height <= 0) return "width / height";
    if ((int64_t)d->width * (int64_t)d->height > (1ll << 30)) return "width * height (more than 2^30 pixels)";
    if (d->iterations < 0 || d->iterations > 8) return "iterations";
    if (d->normal_power_log2 < 0 || d->normal_power_log2 > 10) return "normal_power_log2";
    if (d->sigma_z != 0.0f && !pos_finite(d->sigma_z)) return "sigma_z";
    if (sigma_2 != 0.0f && !pos_finite(sigma_2)) return sigma_2_name;
    if (d->scale != 0.0f && !pos_finite(d->scale)) return "scale";
    if (d->albedo_floor != 0.0f && !pos_finite(d->albedo_floor)) return "albedo_floor";
    r->width = d->width; r->height = d->height;
    r->iterations = d->iterations ? d->iterations : 5;
    r->normal_power_log2 = d->normal_power_log2;
    r->scale = d->scale != 0.0f ? d->scale : 1.0f;
    r->albedo_floor = d->albedo_floor != 0.0f ? d->albedo_floor : 0.01f;
    const float sz = d->sigma_z != 0.0f ? d->sigma_z : 0.05f;
    r->kz = 1.0f / (sz * sz);
    r->min_history = r->var_floor = 0.0f;
    return nullptr;
}

// nullptr, or the name of the first field that is out of range
inline const char* resolve(const pt_denoise_params* d, Resolved* r) {
    if (const char* bad = resolve_common(d, d->sigma_c, "sigma_c", r)) return bad;
    r->mode = d->sigma_c != 0.0f ? Mode::Color : Mode::Plain;
    for (int k = 0; k < 8; k++) {
        const float sc = d->sigma_c * (1.0f / (float)(1 << k));     // exact: a power of two
        r->kl[k] = r->mode == Mode::Color ? 1.0f / (sc * sc) : 0.0f;
    }
    return nullptr;
}

inline const char* vresolve(const pt_vdenoise_params* d, Resolved* r) {
    if (const char* bad = resolve_common(d, d->sigma_l, "sigma_l", r)) return bad;
    if (d->min_history < 0 || d->min_history > 65536) return "min_history";
    if (d->var_floor != 0.0f && !pos_finite(d->var_floor)) return "var_floor";
    r->mode = Mode::Variance;
    const float sl = d->sigma_l != 0.0f ? d->sigma_l : 4.0f;
    for (int k = 0; k < 8; k++) r->kl[k] = sl * sl;
    r->min_history = (float)(d->min_history ? d->min_history : 4);
    r->var_floor = d->var_floor != 0.0f ? d->var_floor : 1e-10f;
    return nullptr;
}

// The caller's frames of either call.  moments, hist_len, out_variance: pt_denoise_variance only (out_variance may be null).
struct Frames {
    const float *color, *albedo, *normal, *depth, *moments, *hist_len;
    float *out, *out_variance;
};

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

// wn and wz: the two guide weights of a tap q seen from p
PT_HD void guide_weights(float npx, float npy, float npz, float zp, float inv_zp, float nqx, float nqy, float nqz, float zq,
                         int normal_power_log2, float kz, float& wn, float& wz) {
    wn = ptm::fmax2(0.0f, npx * nqx + npy * nqy + npz * nqz);
    for (int e = 0; e < normal_power_log2; e++) wn = wn * wn;
    const float rd = (zp - zq) * inv_zp;
    wz = 1.0f / (1.0f + (rd * rd) * kz);
}

// the not-filterable mark in a colour record's fourth word
template <Mode M>
PT_HD bool unfilterable(float w) {
    if constexpr (M == Mode::Variance) return w < 0.0f;
    else return w == 0.0f;
}

// x_{k+1} (Variance: and v_{k+1}) of pixel (px, py) from the records of iteration k; spacing = 1 << k.  Taps in the order
// dy = -2..2 (outer), dx = -2..2 (inner): the sums are not associative.  Every tap is clipped to the frame before its address
// is formed.  kl: Resolved::kl[k].  Variance: the luminance tolerance of a tap is the 3 x 3 average g of v_k around p
// (spacing 1, colour records only).
template <Mode M, class R>
PT_HD Rec filter(const R* __restrict__ guide, const R* __restrict__ x, int px, int py, int width, int height, int spacing,
                 int normal_power_log2, float kz, float kl, float var_floor) {
    constexpr bool V = M == Mode::Variance;
    const size_t p = (size_t)py * (size_t)width + (size_t)px;
    const R xp = x[p];
    if (unfilterable<M>(xp.w)) return Rec{xp.x, xp.y, xp.z, V ? -1.0f : 0.0f};
    const R gp = guide[p];
    const float inv_zp = 1.0f / ptm::fmax2(gp.w, 1e-20f);
    const float lp = M != Mode::Plain ? lum(xp.x, xp.y, xp.z) : 0.0f;
    float den = 0.0f;
    if constexpr (V) {
        const float c3[3] = {1.0f / 4.0f, 1.0f / 2.0f, 1.0f / 4.0f};
        float gsum = 0.0f, cwsum = 0.0f;
#pragma unroll
        for (int dy = -1; dy <= 1; dy++) {
            const int qy = py + dy;
            if (qy < 0 || qy >= height) continue;
            float vr[3];                                             // -1 also for a tap outside the frame
#pragma unroll
            for (int dx = -1; dx <= 1; dx++) {
                const int qx = px + dx;
                const bool in = qx >= 0 && qx < width;
                const float v = x[(size_t)qy * (size_t)width + (size_t)(in ? qx : px)].w;
                vr[dx + 1] = in ? v : -1.0f;
            }
#pragma unroll
            for (int dx = -1; dx <= 1; dx++) {
                if (vr[dx + 1] < 0.0f) continue;
                const float cw = c3[dy + 1] * c3[dx + 1];
                gsum = gsum + vr[dx + 1] * cw;
                cwsum = cwsum + cw;
            }
        }
        const float g = gsum * (1.0f / cwsum);
        den = kl * g + var_floor;
    }
    const float h[5] = {1.0f / 16.0f, 1.0f / 4.0f, 3.0f / 8.0f, 1.0f / 4.0f, 1.0f / 16.0f};
    float sr = 0.0f, sg = 0.0f, sb = 0.0f, vsum = 0.0f, wsum = 0.0f;
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
            if (!in[dx + 2] || unfilterable<M>(xq.w)) continue;
            float wn, wz;
            guide_weights(gp.x, gp.y, gp.z, gp.w, inv_zp, gq.x, gq.y, gq.z, gq.w, normal_power_log2, kz, wn, wz);
            float w = ((h[dy + 2] * h[dx + 2]) * wn) * wz;
            if constexpr (M != Mode::Plain) {
                const float dl = lp - lum(xq.x, xq.y, xq.z);
                if constexpr (V) w = w * (den / (den + dl * dl));
                else w = w * (1.0f / (1.0f + (dl * dl) * kl));
            }
            sr = sr + xq.x * w; sg = sg + xq.y * w; sb = sb + xq.z * w;
            if constexpr (V) vsum = vsum + xq.w * (w * w);
            wsum = wsum + w;
        }
    }
    const float inv = 1.0f / wsum;
    return Rec{sr * inv, sg * inv, sb * inv, V ? vsum * (inv * inv) : 1.0f};
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

// ---- pt_denoise_variance: the first and the last pass -----------------------------------------------------------------------

// The guide record, x_0 and v_0 of pixel (px, py) from the caller's frames.  Only a pixel whose history is shorter than
// min_history gathers: 7 x 7 taps at spacing 1 of the neighbours' albedo (filterable?), normal, depth and moments, each
// clipped to the frame before its address is formed.
PT_HD void vdn_prep(const Resolved& r, const float* __restrict__ color, const float* __restrict__ albedo,
                    const float* __restrict__ normal, const float* __restrict__ depth, const float* __restrict__ moments,
                    const float* __restrict__ hist_len, int px, int py, Rec& guide, Rec& x0) {
    const size_t p = (size_t)py * (size_t)r.width + (size_t)px;
    dn_prep(color + 3 * p, albedo + 3 * p, normal + 3 * p, depth[p], r.scale, r.albedo_floor, guide, x0);
    if (x0.w == 0.0f) { x0.w = -1.0f; return; }
    const float L = hist_len[p];
    const float m1 = moments[2 * p], m2 = moments[2 * p + 1];
    const float tv = ptm::fmax2(0.0f, m2 - m1 * m1);
    float v = tv;
    if (!(L >= r.min_history)) {
        const float inv_zp = 1.0f / ptm::fmax2(guide.w, 1e-20f);
        float s1 = 0.0f, s2 = 0.0f, ws = 0.0f;
        for (int dy = -3; dy <= 3; dy++) {
            const int qy = py + dy;
            if (qy < 0 || qy >= r.height) continue;
#pragma unroll
            for (int dx = -3; dx <= 3; dx++) {
                const int qx = px + dx;
                if (qx < 0 || qx >= r.width) continue;
                const size_t q = (size_t)qy * (size_t)r.width + (size_t)qx;
                if (!filterable(albedo + 3 * q)) continue;
                float wn, wz;
                guide_weights(guide.x, guide.y, guide.z, guide.w, inv_zp, normal[3 * q], normal[3 * q + 1], normal[3 * q + 2],
                              depth[q], r.normal_power_log2, r.kz, wn, wz);
                const float w = wn * wz;
                s1 = s1 + moments[2 * q] * w; s2 = s2 + moments[2 * q + 1] * w;
                ws = ws + w;
            }
        }
        if (ws > 0.0f) {
            const float inv = 1.0f / ws;
            const float M1 = s1 * inv, M2 = s2 * inv;
            v = ptm::fmax2(0.0f, M2 - M1 * M1) * (4.0f / ptm::fmax2(L, 1.0f));
        }
    }
    x0.w = v;
}

// out = x_last * a' for filterable pixels, x_last otherwise; the variance of a pixel that is not filterable is 0
PT_HD void vdn_store(const Rec& x, const float* albedo, float albedo_floor, float* out, float* out_variance) {
    dn_store(Rec{x.x, x.y, x.z, x.w < 0.0f ? 0.0f : 1.0f}, albedo, albedo_floor, out);
    if (out_variance) *out_variance = x.w < 0.0f ? 0.0f : x.w;
}

// Device side (pt_denoise.hip), both calls.  guide / xa / xb: width * height records each, device memory owned by the caller
// (the scene handle); f: device pointers.  Enqueues 1 + iterations kernels on `stream`, no host sync.  Returns a hipError_t.
int run_device(const Resolved& r, const Frames& f, void* guide, void* xa, void* xb, void* hip_stream);

// Iteration k of the host twin over the frame
template <Mode M>
inline void filter_pass(const Resolved& r, int k, const Rec* guide, const Rec* src, Rec* dst) {
    for (int py = 0; py < r.height; py++)
        for (int px = 0; px < r.width; px++)
            dst[(size_t)py * r.width + px] =
                filter<M>(guide, src, px, py, r.width, r.height, 1 << k, r.normal_power_log2, r.kz, r.kl[k], r.var_floor);
}

// Host twin of both calls: the same functions over the frame, pass by pass (so f.out may alias f.color).
inline void run_host(const Resolved& r, const Frames& f) {
    const bool variance = r.mode == Mode::Variance;
    const size_t npix = (size_t)r.width * (size_t)r.height;
    std::vector<Rec> guide(npix), xa(npix), xb(npix);
    for (int py = 0; py < r.height; py++)
        for (int px = 0; px < r.width; px++) {
            const size_t p = (size_t)py * r.width + px;
            if (variance) vdn_prep(r, f.color, f.albedo, f.normal, f.depth, f.moments, f.hist_len, px, py, guide[p], xa[p]);
            else dn_prep(f.color + 3 * p, f.albedo + 3 * p, f.normal + 3 * p, f.depth[p], r.scale, r.albedo_floor, guide[p], xa[p]);
        }
    Rec* xs[2] = {xa.data(), xb.data()};
    for (int k = 0; k < r.iterations; k++) {
        const Rec* src = xs[k & 1];
        Rec* dst = xs[(k + 1) & 1];
        if (variance) filter_pass<Mode::Variance>(r, k, guide.data(), src, dst);
        else if (r.mode == Mode::Color) filter_pass<Mode::Color>(r, k, guide.data(), src, dst);
        else filter_pass<Mode::Plain>(r, k, guide.data(), src, dst);
    }
    const Rec* last = xs[r.iterations & 1];
    for (size_t p = 0; p < npix; p++) {
        if (variance) vdn_store(last[p], f.albedo + 3 * p, r.albedo_floor, f.out + 3 * p, f.out_variance ? f.out_variance + p : nullptr);
        else dn_store(last[p], f.albedo + 3 * p, r.albedo_floor, f.out + 3 * p);
    }
}

}  // namespace ptdn
