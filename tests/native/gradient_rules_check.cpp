// Runs the host twins of pt_temporal_gradient and pt_temporal_accumulate_adaptive the way pt_*_host run them - ptg::resolve +
// ptg::run_host of csrc/pt_gradient.h and ptt::resolve + ptt::run_host with a ptt::Lambda of csrc/pt_temporal.h, not a re-typed
// loop - on the smallest frames where a tile, a tap or a map index can go wrong, with every buffer an exactly-sized heap
// allocation, so that an address formed outside a frame, the re-traced rows or the map is a report of AddressSanitizer.
//   frames (W x H): 1 x 1, 1 x 2, 2 x 1, 5 x 3, 65 x 5, 67 x 5; strides 1, 2, 3, 5, 16 where the frame has a sampled row;
//   the gradient: 8 iterations (spacing 128 far exceeds every grid); equal inputs must give +0 at every tile;
//   the accumulation: every pixel sees every pair of the motion values -0.5, 0, W - 0.5, W, W + 0.5 (H for y), +-inf, NaN and
//     two inside the frame, under a map of 0, NaN, negative entries and entries above 1; with an all-zero map the three outputs
//     must equal pt_temporal_accumulate_moments' byte for byte; with no history the map is a null pointer.
// Stand-alone; built with -fsanitize=address,undefined by tests/test_gradient_rules_host.py.  Exit code 0 = all held.
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <limits>
#include <memory>
#include <random>

#include "pt_gradient.h"
#include "pt_temporal.h"

namespace {

int g_errors = 0;

void fail(const char* what, int w, int h, int s) {
    if (g_errors++ < 10) std::fprintf(stderr, "FAIL: %s (%d x %d, stride %d)\n", what, w, h, s);
}

// an exactly-sized heap allocation of n floats
struct Buf {
    std::unique_ptr<float[]> p;
    size_t n;
    explicit Buf(size_t count) : p(new float[count]), n(count) { for (size_t i = 0; i < n; i++) p[i] = 0.0f; }
    float* get() { return p.get(); }
    bool same_bytes(const Buf& o) const { return n == o.n && std::memcmp(p.get(), o.p.get(), n * sizeof(float)) == 0; }
};

void check_gradient(int w, int h, int s, std::mt19937& rng) {
    const pt_gradient_params g = {w, h, s, 8, 0.0f, 0.0f};
    ptg::Resolved r;
    if (ptg::resolve(&g, &r)) { fail("pt_gradient_params rejected", w, h, s); return; }
    std::uniform_real_distribution<float> u(0.0f, 2.0f);
    Buf prev(3 * (size_t)w * h), same(3 * (size_t)w * r.th), changed(3 * (size_t)w * r.th), lam(( size_t)r.tw * r.th);
    for (size_t i = 0; i < prev.n; i++) prev.p[i] = u(rng);
    for (int ty = 0; ty < r.th; ty++)
        for (int i = 0; i < 3 * w; i++) {
            same.p[(size_t)ty * 3 * w + i] = prev.p[(size_t)(r.r0 + s * ty) * 3 * w + i];
            changed.p[(size_t)ty * 3 * w + i] = same.p[(size_t)ty * 3 * w + i] * (rng() % 3 ? 1.0f : 0.25f);
        }
    ptg::run_host(r, prev.get(), same.get(), lam.get());
    for (size_t t = 0; t < lam.n; t++) {
        uint32_t bits;
        std::memcpy(&bits, &lam.p[t], 4);
        if (bits != 0) { fail("equal inputs: lambda is not +0", w, h, s); break; }
    }
    ptg::run_host(r, prev.get(), changed.get(), lam.get());
    for (size_t t = 0; t < lam.n; t++)
        if (!(lam.p[t] >= 0.0f && lam.p[t] <= 1.0f)) { fail("lambda outside [0, 1]", w, h, s); break; }
}

void check_adaptive(int w, int h, int s, std::mt19937& rng) {
    const pt_temporal_params t = {w, h, 8, 0.0f, 0.9f, 0.0f};
    ptt::Resolved r;
    if (ptt::resolve(&t, &r)) { fail("pt_temporal_params rejected", w, h, s); return; }
    int32_t r0, tw, th;
    if (!ptg::tile_grid(w, h, s, &r0, &tw, &th)) { fail("no tile grid", w, h, s); return; }
    const size_t npix = (size_t)w * h;
    const float inf = std::numeric_limits<float>::infinity(), nan = std::numeric_limits<float>::quiet_NaN();
    const float xs[] = {-0.5f, -0.25f, 0.0f, (float)w - 0.5f, (float)w, (float)w + 0.25f, (float)w + 0.5f, inf, -inf, nan, 0.5f, 0.5f * (float)w};
    const float ys[] = {-0.5f, -0.25f, 0.0f, (float)h - 0.5f, (float)h, (float)h + 0.25f, (float)h + 0.5f, inf, -inf, nan, 0.5f, 0.5f * (float)h};
    const int nx = sizeof xs / sizeof xs[0], ny = sizeof ys / sizeof ys[0];
    std::uniform_real_distribution<float> u(0.0f, 1.0f);
    Buf color(3 * npix), albedo(3 * npix), normal(3 * npix), depth(npix), hist_color(3 * npix), hist_len(npix), hist_moments(2 * npix);
    for (size_t p = 0; p < npix; p++) {
        for (int c = 0; c < 3; c++) {
            color.p[3 * p + c] = 4.0f * u(rng);
            hist_color.p[3 * p + c] = 2.0f * u(rng);
            albedo.p[3 * p + c] = rng() % 5 ? u(rng) : 0.0f;
        }
        normal.p[3 * p + 2] = 1.0f;
        depth.p[p] = 1.0f + 0.01f * u(rng);
        hist_len.p[p] = (float)(rng() % 12);
        hist_moments.p[2 * p] = u(rng); hist_moments.p[2 * p + 1] = 1.0f + u(rng);
    }
    Buf zero((size_t)tw * th), mixed((size_t)tw * th);
    const float entries[] = {0.0f, nan, -0.5f, 3.0f, 0.5f, 1.0f, -0.0f};
    for (size_t i = 0; i < mixed.n; i++) mixed.p[i] = entries[rng() % 7];
    Buf motion(2 * npix);
    for (int shift = 0; shift < nx * ny; shift++) {              // every pixel sees every pair
        for (size_t p = 0; p < npix; p++) {
            const size_t k = (p + (size_t)shift) % (size_t)(nx * ny);
            motion.p[2 * p] = xs[k % nx];
            motion.p[2 * p + 1] = ys[k / nx];
        }
        Buf oc(3 * npix), ol(npix), om(2 * npix), oc0(3 * npix), ol0(npix), om0(2 * npix), oc1(3 * npix), ol1(npix), om1(2 * npix);
        pt_temporal_io io = {color.get(), albedo.get(), normal.get(), motion.get(), depth.get(), hist_color.get(), normal.get(),
                             depth.get(), hist_len.get(), hist_moments.get(), oc.get(), ol.get(), om.get()};
        ptt::run_host(r, true, 0.01f, io);
        io.out_color = oc0.get(); io.out_len = ol0.get(); io.out_moments = om0.get();
        const ptt::Lambda lam0 = {zero.get(), s, tw, th};
        ptt::run_host(r, true, 0.01f, io, &lam0);
        if (!oc0.same_bytes(oc) || !ol0.same_bytes(ol) || !om0.same_bytes(om)) fail("a map of zeros differs from the moments rule", w, h, s);
        io.out_color = oc1.get(); io.out_len = ol1.get(); io.out_moments = om1.get();
        const ptt::Lambda lam1 = {mixed.get(), s, tw, th};
        ptt::run_host(r, true, 0.01f, io, &lam1);
        for (size_t p = 0; p < npix; p++)
            if (!(ol1.p[p] >= 1.0f && ol1.p[p] <= 8.0f)) { fail("out_len outside [1, max_history]", w, h, s); break; }
        // no history: the map is never read
        io.hist_color = io.hist_normal = io.hist_depth = io.hist_len = io.hist_moments = nullptr;
        const ptt::Lambda none = {nullptr, s, tw, th};
        ptt::run_host(r, true, 0.01f, io, &none);
    }
}

}  // namespace

int main() {
    std::mt19937 rng(20240921u);
    const int frames[][2] = {{1, 1}, {1, 2}, {2, 1}, {5, 3}, {65, 5}, {67, 5}};
    for (const auto& wh : frames)
        for (int s : {1, 2, 3, 5, 16}) {
            if (wh[1] <= s / 2) continue;
            check_gradient(wh[0], wh[1], s, rng);
            check_adaptive(wh[0], wh[1], s, rng);
        }
    if (g_errors) { std::fprintf(stderr, "%d checks failed\n", g_errors); return 1; }
    std::puts("gradient rules: all held");
    return 0;
}
