// Runs the host twins of the four image-space stages (pt_denoise, pt_denoise_variance, pt_temporal_accumulate,
// pt_temporal_accumulate_moments) the way pt_*_host run them - ptdn::resolve / vresolve + ptdn::run_host and ptt::resolve +
// ptt::run_host of csrc/pt_denoise.h and csrc/pt_temporal.h, not a re-typed loop - on the smallest frames where the clipping of
// a tap can go wrong, with every buffer an exactly-sized heap allocation, so that a tap address formed outside the frame is a
// report of AddressSanitizer.  (On the device such a read returns garbage silently, and the tap is then often dropped anyway.)
//   frames (W x H): 1 x 1, 1 x 2, 2 x 1, 5 x 3, 65 x 5 (the last straddles a 64 x 4 tile in both directions);
//   the filters: 8 iterations (spacing 128 far exceeds every frame), without and with the colour term and in the variance
//     mode with min_history above every history length (every filterable pixel takes the 7 x 7 gather), out == color and
//     out != color, with and without the variance output;
//   the temporal rules: every pixel sees every pair of the motion values -1, -0.5, W - 0.5, W (H for y), +-inf, NaN and two
//     inside the frame, with and without history, out_color == color and out_color != color; the plain call has null albedo
//     and moments pointers, and its colour and length must equal the moments call's byte for byte.
// Stand-alone; built with -fsanitize=address,undefined by tests/test_post_rules_host.py.  Exit code 0 = all held.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <limits>
#include <memory>
#include <random>

#include "pt_denoise.h"
#include "pt_temporal.h"

namespace {

int g_errors = 0;

void fail(const char* what, int w, int h) {
    if (g_errors++ < 10) std::fprintf(stderr, "FAIL: %s (%d x %d)\n", what, w, h);
}

// an exactly-sized heap allocation of n floats
struct Buf {
    std::unique_ptr<float[]> p;
    size_t n;
    explicit Buf(size_t count) : p(new float[count]), n(count) { fill(0.0f); }
    Buf(const Buf& o) : p(new float[o.n]), n(o.n) { std::memcpy(p.get(), o.p.get(), n * sizeof(float)); }
    void fill(float v) { for (size_t i = 0; i < n; i++) p[i] = v; }
    float* get() { return p.get(); }
    bool same_bytes(const Buf& o) const { return n == o.n && std::memcmp(p.get(), o.p.get(), n * sizeof(float)) == 0; }
};

struct Frame {
    int w, h;
    size_t npix;
    Buf color, albedo, normal, depth, moments, hist_len;
    Frame(int w_, int h_, std::mt19937& rng)
        : w(w_), h(h_), npix((size_t)w_ * h_), color(3 * npix), albedo(3 * npix), normal(3 * npix), depth(npix), moments(2 * npix),
          hist_len(npix) {
        std::uniform_real_distribution<float> u(0.0f, 1.0f);
        for (size_t p = 0; p < npix; p++) {
            const bool lit = rng() % 5 != 0;                         // a fifth of the pixels are not filterable
            for (int c = 0; c < 3; c++) {
                color.p[3 * p + c] = 4.0f * u(rng);
                albedo.p[3 * p + c] = lit ? (rng() % 4 ? u(rng) : 0.001f) : 0.0f;
            }
            normal.p[3 * p] = 0.0f; normal.p[3 * p + 1] = 0.1f * u(rng); normal.p[3 * p + 2] = 1.0f;
            depth.p[p] = 1.0f + 0.01f * u(rng);
            const float m1 = u(rng);
            moments.p[2 * p] = m1; moments.p[2 * p + 1] = m1 * m1 + 0.1f * u(rng);
            hist_len.p[p] = (float)(rng() % 4);                     // 0 .. 3: below min_history everywhere
        }
    }
};

void check_filters(int w, int h, std::mt19937& rng) {
    Frame f(w, h, rng);
    // pt_denoise without and with the colour term
    for (float sigma_c : {0.0f, 0.5f}) {
        const pt_denoise_params d = {w, h, 8, 2, 0.0f, sigma_c, 0.0f, 0.0f};
        ptdn::Resolved r;
        if (ptdn::resolve(&d, &r)) { fail("pt_denoise_params rejected", w, h); return; }
        Buf out(3 * f.npix), in_place(f.color);
        ptdn::run_host(r, ptdn::Frames{f.color.get(), f.albedo.get(), f.normal.get(), f.depth.get(), nullptr, nullptr, out.get(), nullptr});
        ptdn::run_host(r, ptdn::Frames{in_place.get(), f.albedo.get(), f.normal.get(), f.depth.get(), nullptr, nullptr, in_place.get(), nullptr});
        if (!out.same_bytes(in_place)) fail("pt_denoise: out == color differs from out != color", w, h);
    }
    // pt_denoise_variance: every filterable pixel gathers its 7 x 7 window
    const pt_vdenoise_params d = {w, h, 8, 2, 0.0f, 0.0f, 0.0f, 0.0f, 65536, 0.0f};
    ptdn::Resolved r;
    if (ptdn::vresolve(&d, &r)) { fail("pt_vdenoise_params rejected", w, h); return; }
    Buf out(3 * f.npix), var(f.npix), in_place(f.color), no_var(3 * f.npix);
    ptdn::run_host(r, ptdn::Frames{f.color.get(), f.albedo.get(), f.normal.get(), f.depth.get(), f.moments.get(), f.hist_len.get(),
                                   out.get(), var.get()});
    ptdn::run_host(r, ptdn::Frames{in_place.get(), f.albedo.get(), f.normal.get(), f.depth.get(), f.moments.get(), f.hist_len.get(),
                                   in_place.get(), nullptr});
    ptdn::run_host(r, ptdn::Frames{f.color.get(), f.albedo.get(), f.normal.get(), f.depth.get(), f.moments.get(), f.hist_len.get(),
                                   no_var.get(), nullptr});
    if (!out.same_bytes(in_place)) fail("pt_denoise_variance: out == color differs from out != color", w, h);
    if (!out.same_bytes(no_var)) fail("pt_denoise_variance: the frame depends on the variance output", w, h);
}

void check_temporal(int w, int h, std::mt19937& rng) {
    Frame f(w, h, rng);
    const float inf = std::numeric_limits<float>::infinity(), nan = std::numeric_limits<float>::quiet_NaN();
    // motion holds x + 0.5: these are the values of the issue in x itself and in motion
    const float xs[] = {-1.0f, -0.5f, (float)w - 0.5f, (float)w, inf, -inf, nan, 0.5f, 0.5f * (float)w,
                        -0.5f, 0.0f, (float)w, (float)w + 0.5f};
    const float ys[] = {-1.0f, -0.5f, (float)h - 0.5f, (float)h, inf, -inf, nan, 0.5f, 0.5f * (float)h,
                        -0.5f, 0.0f, (float)h, (float)h + 0.5f};
    const int nx = sizeof xs / sizeof xs[0], ny = sizeof ys / sizeof ys[0];
    const pt_temporal_params t = {w, h, 8, 0.0f, 0.9f, 0.0f};
    ptt::Resolved r;
    if (ptt::resolve(&t, &r)) { fail("pt_temporal_params rejected", w, h); return; }
    // the history: mostly usable (the taps are kept, so their records are read), a few records empty
    Buf hist_color(3 * f.npix), hist_normal(f.normal), hist_depth(f.depth), hist_len(f.npix), hist_moments(f.moments), prev_depth(f.depth);
    for (size_t p = 0; p < f.npix; p++) {
        for (int c = 0; c < 3; c++) hist_color.p[3 * p + c] = f.color.p[3 * p + c] * 0.5f;
        hist_len.p[p] = (float)(rng() % 12);
        if (rng() % 7 == 0) hist_depth.p[p] = 0.0f;
        if (rng() % 7 == 0) prev_depth.p[p] = 0.0f;
    }
    Buf motion(2 * f.npix);
    for (int shift = 0; shift < nx * ny; shift++) {              // every pixel sees every pair
        for (size_t p = 0; p < f.npix; p++) {
            const size_t k = (p + (size_t)shift) % (size_t)(nx * ny);
            motion.p[2 * p] = xs[k % nx];
            motion.p[2 * p + 1] = ys[k / nx];
        }
        for (int with_history = 0; with_history < 2; with_history++) {
            const float* hc = with_history ? hist_color.get() : nullptr;
            const float* hn = with_history ? hist_normal.get() : nullptr;
            const float* hz = with_history ? hist_depth.get() : nullptr;
            const float* hl = with_history ? hist_len.get() : nullptr;
            const float* hm = with_history ? hist_moments.get() : nullptr;
            Buf oc(3 * f.npix), ol(f.npix), oc_m(3 * f.npix), ol_m(f.npix), om(2 * f.npix);
            const pt_temporal_io plain = {f.color.get(), nullptr, f.normal.get(), motion.get(), prev_depth.get(), hc, hn, hz, hl, nullptr,
                                          oc.get(), ol.get(), nullptr};
            const pt_temporal_io mom = {f.color.get(), f.albedo.get(), f.normal.get(), motion.get(), prev_depth.get(), hc, hn, hz, hl, hm,
                                        oc_m.get(), ol_m.get(), om.get()};
            ptt::run_host(r, false, 0.01f, plain);
            ptt::run_host(r, true, 0.01f, mom);
            if (!oc.same_bytes(oc_m) || !ol.same_bytes(ol_m)) fail("the plain rule's colour or length differs from the moments rule's", w, h);
            // out_color == color
            Buf c1(f.color), c2(f.color), ol1(f.npix), ol2(f.npix), om2(2 * f.npix);
            const pt_temporal_io plain_ip = {c1.get(), nullptr, f.normal.get(), motion.get(), prev_depth.get(), hc, hn, hz, hl, nullptr,
                                             c1.get(), ol1.get(), nullptr};
            const pt_temporal_io mom_ip = {c2.get(), f.albedo.get(), f.normal.get(), motion.get(), prev_depth.get(), hc, hn, hz, hl, hm,
                                           c2.get(), ol2.get(), om2.get()};
            ptt::run_host(r, false, 0.01f, plain_ip);
            ptt::run_host(r, true, 0.01f, mom_ip);
            if (!c1.same_bytes(oc) || !ol1.same_bytes(ol)) fail("pt_temporal_accumulate: out_color == color differs", w, h);
            if (!c2.same_bytes(oc) || !ol2.same_bytes(ol) || !om2.same_bytes(om)) fail("pt_temporal_accumulate_moments: out_color == color differs", w, h);
        }
    }
}

}  // namespace

int main() {
    std::mt19937 rng(20240607u);
    const int frames[][2] = {{1, 1}, {1, 2}, {2, 1}, {5, 3}, {65, 5}};
    for (const auto& wh : frames) {
        check_filters(wh[0], wh[1], rng);
        check_temporal(wh[0], wh[1], rng);
    }
    if (g_errors) { std::fprintf(stderr, "%d checks failed\n", g_errors); return 1; }
    std::puts("post rules: all held");
    return 0;
}
