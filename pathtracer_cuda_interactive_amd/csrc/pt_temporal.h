// pt_temporal.h — the per-pixel rules of pt_render_guides' motion part and of pt_temporal_accumulate (include/pt_api.h,
// DESIGN.md §19), written once for the device (aov_kernel<., true> in pt_kernels.h, pt_temporal.hip) and for the host twin
// pt_temporal_accumulate_host.  pt_temporal_accumulate_moments is the same function, accumulate_pixel, with
// MOMENTS = true: it carries two luminance moments on the same taps, and pt_temporal_accumulate_adaptive is that
// with ADAPTIVE = true: pt_temporal_gradient's per-tile lambda shortens the history.  The host twins' frame loop, run_host, is
// here too, so a plain host compile of this header runs what pt_temporal_accumulate*_host run (tests/native/post_rules_check.cpp).
//
// Every operation is an IEEE fp32 + - * / sqrt in the order written (no contraction: the build forbids it), so the device, the
// host twin and a numpy restatement give the same bits.
#pragma once

#include <stdint.h>

#include "../../include/pt_api.h"
#include "pt_denoise.h"      // lum, filterable: the moments of pt_temporal_accumulate_moments live in pt_denoise's demodulated space
#include "pt_math.h"

namespace ptt {

PT_HD bool finite32(float v) { return __builtin_fabsf(v) <= 3.402823466e+38f; }   // false for inf and NaN

// The previous camera of pt_motion_params, by value in the kernel's arguments.
struct PrevCam {
    float origin[3], top_left[3], horizontal[3], vertical[3];
};

// Projection of the previous position Q of a pixel's surface point into the previous camera: continuous pixel coordinates
// (the centre of pixel (i, j) is (i + 0.5, j + 0.5)) and the distance from the previous camera.  False — and zeros — where
// Q is not in front of that camera or a result is not finite.
PT_HD bool project_previous(ptm::V3 Q, const PrevCam& c, int width, int height, float& mx, float& my, float& prev_depth) {
    const ptm::V3 o = ptm::mk(c.origin[0], c.origin[1], c.origin[2]);
    const ptm::V3 tl = ptm::mk(c.top_left[0], c.top_left[1], c.top_left[2]);
    const ptm::V3 hz = ptm::mk(c.horizontal[0], c.horizontal[1], c.horizontal[2]);
    const ptm::V3 vt = ptm::mk(c.vertical[0], c.vertical[1], c.vertical[2]);
    const ptm::V3 e = Q - o;
    const ptm::V3 a = tl - o;
    const ptm::V3 hv = ptm::cross(hz, vt);
    const float D = ptm::dot(a, hv);
    const float n0 = ptm::dot(e, hv);
    const float s = n0 / D;
    const float n1 = ptm::dot(a, ptm::cross(e, vt));
    const float n2 = ptm::dot(a, ptm::cross(hz, e));
    const float x = (n1 / n0) * (float)width;
    const float y = (-(n2 / n0)) * (float)height;
    const float z = ptm::sqrt_exact(ptm::dot(e, e));
    const bool ok = s > 0.0f && finite32(x) && finite32(y) && finite32(z);
    mx = ok ? x : 0.0f;
    my = ok ? y : 0.0f;
    prev_depth = ok ? z : 0.0f;
    return ok;
}

// pt_temporal_params with the defaults resolved
struct Resolved {
    int32_t width, height;
    float max_history;               // (float)max_history: exact, at most 65536
    float sigma_z, normal_min, scale;
};

// nullptr, or the name of the first field that is out of range
inline const char* resolve(const pt_temporal_params* t, Resolved* r) {
    auto pos_finite = [](float v) { return v > 0.0f && v <= 3.402823466e+38f; };
    if (t->width <= 0 || t->height <= 0) return "width / height";
    if ((int64_t)t->width * (int64_t)t->height > (1ll << 30)) return "width * height (more than 2^30 pixels)";
    if (t->max_history < 0 || t->max_history > 65536) return "max_history";
    if (t->sigma_z != 0.0f && !pos_finite(t->sigma_z)) return "sigma_z";
    if (!(t->normal_min >= -1.0f && t->normal_min <= 1.0f)) return "normal_min";
    if (t->scale != 0.0f && !pos_finite(t->scale)) return "scale";
    r->width = t->width; r->height = t->height;
    r->max_history = (float)(t->max_history ? t->max_history : 32);
    r->sigma_z = t->sigma_z != 0.0f ? t->sigma_z : 0.1f;
    r->normal_min = t->normal_min;
    r->scale = t->scale != 0.0f ? t->scale : 1.0f;
    return nullptr;
}

// pt_temporal_gradient's map as pt_temporal_accumulate_adaptive reads it: [th, tw] tiles of stride x stride pixels
struct Lambda {
    const float* map;
    int32_t stride, tw, th;
};

// One pixel of pt_temporal_accumulate (MOMENTS = false) and of pt_temporal_accumulate_moments (MOMENTS = true: the same
// colour and length from the same instantiation of every line, and the first two moments of the demodulated luminance carried
// on the same taps with the same weights).  io.hist_color == nullptr: no history.  The four tap addresses are formed only
// after the clip to the frame.  io.out_color may be io.color: a pixel reads only its own colour.  MOMENTS = false never reads
// io.albedo, io.hist_moments or io.out_moments (they are null there) nor albedo_floor.  ADAPTIVE = true (with MOMENTS):
// pt_temporal_accumulate_adaptive — a pixel that continues a history reads the lambda of the tile its motion vector lands in and,
// where that is positive, blends with a larger weight; lam is read in no other case.
template <bool MOMENTS, bool ADAPTIVE = false>
PT_HD void accumulate_pixel(const Resolved& r, float albedo_floor, int px, int py, const pt_temporal_io& io, const Lambda& lam = Lambda{}) {
    const size_t p = (size_t)py * (size_t)r.width + (size_t)px;
    const float cr = io.color[3 * p] * r.scale, cg = io.color[3 * p + 1] * r.scale, cb = io.color[3 * p + 2] * r.scale;
    float m1 = 0.0f, m2 = 0.0f;
    if constexpr (MOMENTS) {
        const float* al = io.albedo + 3 * p;
        const float l = ptdn::filterable(al) ? ptdn::lum(cr / ptm::fmax2(al[0], albedo_floor), cg / ptm::fmax2(al[1], albedo_floor),
                                                         cb / ptm::fmax2(al[2], albedo_floor))
                                             : ptdn::lum(cr, cg, cb);
        m1 = l; m2 = l * l;
    }
    float o_r = cr, o_g = cg, o_b = cb, o_len = 1.0f, o_m1 = m1, o_m2 = m2;            // the fallback
    const float zp = io.prev_depth[p];
    if (io.hist_color && zp != 0.0f) {
        const float x = io.motion[2 * p] - 0.5f, y = io.motion[2 * p + 1] - 0.5f;
        if (x >= -1.0f && x < (float)r.width && y >= -1.0f && y < (float)r.height) {
            const float x0 = __builtin_floorf(x), y0 = __builtin_floorf(y);
            const float fx = x - x0, fy = y - y0;
            const int ix = (int)x0, iy = (int)y0;
            const float nx = io.normal[3 * p], ny = io.normal[3 * p + 1], nz = io.normal[3 * p + 2];
            const float tol = r.sigma_z * zp;
            float sr = 0.0f, sg = 0.0f, sb = 0.0f, lsum = 0.0f, ms1 = 0.0f, ms2 = 0.0f, wsum = 0.0f;
#pragma unroll
            for (int dy = 0; dy < 2; dy++) {
#pragma unroll
                for (int dx = 0; dx < 2; dx++) {
                    const int qx = ix + dx, qy = iy + dy;
                    if (qx < 0 || qx >= r.width || qy < 0 || qy >= r.height) continue;
                    const float b = (dx ? fx : 1.0f - fx) * (dy ? fy : 1.0f - fy);
                    const size_t q = (size_t)qy * (size_t)r.width + (size_t)qx;
                    const float hl = io.hist_len[q], hz = io.hist_depth[q];
                    if (!(hl > 0.0f) || hz == 0.0f) continue;
                    if (!(__builtin_fabsf(hz - zp) <= tol)) continue;
                    if (!(nx * io.hist_normal[3 * q] + ny * io.hist_normal[3 * q + 1] + nz * io.hist_normal[3 * q + 2] >= r.normal_min)) continue;
                    sr = sr + io.hist_color[3 * q] * b; sg = sg + io.hist_color[3 * q + 1] * b; sb = sb + io.hist_color[3 * q + 2] * b;
                    lsum = lsum + hl * b;
                    if constexpr (MOMENTS) { ms1 = ms1 + io.hist_moments[2 * q] * b; ms2 = ms2 + io.hist_moments[2 * q + 1] * b; }
                    wsum = wsum + b;
                }
            }
            if (wsum > 0.0f) {
                const float inv = 1.0f / wsum;
                const float hr = sr * inv, hg = sg * inv, hb = sb * inv;
                const float n = ptm::fmin2(lsum * inv + 1.0f, r.max_history);
                float a = 1.0f / n;
                if constexpr (ADAPTIVE) {
                    int jx = (int)__builtin_floorf(io.motion[2 * p]), jy = (int)__builtin_floorf(io.motion[2 * p + 1]);
                    jx = jx < 0 ? 0 : (jx > r.width - 1 ? r.width - 1 : jx);
                    jy = jy < 0 ? 0 : (jy > r.height - 1 ? r.height - 1 : jy);
                    const int tx = jx / lam.stride, ty_raw = jy / lam.stride;
                    const int ty = ty_raw > lam.th - 1 ? lam.th - 1 : ty_raw;
                    const float lv = lam.map[(size_t)ty * (size_t)lam.tw + (size_t)tx];
                    const float L = lv > 1.0f ? 1.0f : lv;                              // a NaN stays one and fails the next test
                    if (L > 0.0f) {
                        a = a + L * (1.0f - a);
                        o_len = 1.0f / a;
                    } else {
                        o_len = n;
                    }
                } else {
                    o_len = n;
                }
                o_r = hr + (cr - hr) * a; o_g = hg + (cg - hg) * a; o_b = hb + (cb - hb) * a;
                if constexpr (MOMENTS) {
                    const float h1 = ms1 * inv, h2 = ms2 * inv;
                    o_m1 = h1 + (m1 - h1) * a; o_m2 = h2 + (m2 - h2) * a;
                }
            }
        }
    }
    io.out_color[3 * p] = o_r; io.out_color[3 * p + 1] = o_g; io.out_color[3 * p + 2] = o_b;
    io.out_len[p] = o_len;
    if constexpr (MOMENTS) { io.out_moments[2 * p] = o_m1; io.out_moments[2 * p + 1] = o_m2; }
}

// Device side (pt_temporal.hip): one kernel on `stream`, no host sync.  lam: nullptr, or (with moments) the map of
// pt_temporal_accumulate_adaptive.  Returns a hipError_t.
int run_device(const Resolved& r, bool moments, float albedo_floor, const pt_temporal_io& io, const Lambda* lam, void* hip_stream);

// Host twin: the same function over the frame.
inline void run_host(const Resolved& r, bool moments, float albedo_floor, const pt_temporal_io& io, const Lambda* lam = nullptr) {
    for (int py = 0; py < r.height; py++)
        for (int px = 0; px < r.width; px++) {
            if (lam) accumulate_pixel<true, true>(r, albedo_floor, px, py, io, *lam);
            else if (moments) accumulate_pixel<true>(r, albedo_floor, px, py, io);
            else accumulate_pixel<false>(r, albedo_floor, px, py, io);
        }
}

}  // namespace ptt
