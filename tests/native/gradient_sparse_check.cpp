// Runs the host twins of pt_gradient_pixels and pt_temporal_gradient_sparse the way pt_*_host run them - ptg::resolve,
// ptg::pixels_host and ptg::run_host_sparse of csrc/pt_gradient.h, not a re-typed loop - on the smallest frames where a tile, a
// tap, a clamp or a list entry can go wrong, with every buffer an exactly-sized heap allocation, so that an address formed
// outside the frame, the list, the re-traced pixels or the map is a report of AddressSanitizer.
//   frames (W x H): 1 x 1, 1 x 2, 2 x 1, 5 x 3, 65 x 5, 67 x 5; strides 1, 2, 3, 5, 16 where the frame has a sampled row;
//   the pixel choice: seeds 0, 1, 0xffffffff and a few more; every pixel must lie in its tile and in the frame;
//   the reduce: 8 iterations (spacing 128 far exceeds every grid); prev_color equal to the re-traced pixels at the list must
//     give +0 at every tile; lists with entries -1, W * H, INT32_MIN and INT32_MAX must form no address, and a list of such
//     entries alone must give +0 at every tile.
// Stand-alone; built with -fsanitize=address,undefined by tests/test_gradient_sparse_host.py.  Exit code 0 = all held.
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <limits>
#include <memory>
#include <random>

#include "pt_gradient.h"

namespace {

int g_errors = 0;

void fail(const char* what, int w, int h, int s) {
    if (g_errors++ < 10) std::fprintf(stderr, "FAIL: %s (%d x %d, stride %d)\n", what, w, h, s);
}

// an exactly-sized heap allocation of n elements
template <class T>
struct Buf {
    std::unique_ptr<T[]> p;
    size_t n;
    explicit Buf(size_t count) : p(new T[count]), n(count) { for (size_t i = 0; i < n; i++) p[i] = T(0); }
    T* get() { return p.get(); }
};

bool all_plus_zero(Buf<float>& lam) {
    for (size_t t = 0; t < lam.n; t++) {
        uint32_t bits;
        std::memcpy(&bits, &lam.p[t], 4);
        if (bits != 0) return false;
    }
    return true;
}

void check(int w, int h, int s, std::mt19937& rng) {
    const pt_gradient_params g = {w, h, s, 8, 0.0f, 0.0f};
    ptg::Resolved r;
    if (ptg::resolve(&g, &r)) { fail("pt_gradient_params rejected", w, h, s); return; }
    const size_t ntiles = (size_t)r.tw * r.th;
    std::uniform_real_distribution<float> u(0.0f, 2.0f);
    Buf<float> prev(3 * (size_t)w * h), same(3 * ntiles), changed(3 * ntiles), lam(ntiles);
    Buf<int32_t> px(ntiles), bad(ntiles), mixed(ntiles);
    for (size_t i = 0; i < prev.n; i++) prev.p[i] = u(rng);
    const int32_t outside[] = {-1, w * h, std::numeric_limits<int32_t>::min(), std::numeric_limits<int32_t>::max()};
    for (uint32_t seed : {0u, 1u, 0xffffffffu, 12345u, (uint32_t)rng()}) {
        ptg::pixels_host(r, seed, px.get());
        for (int ty = 0; ty < r.th; ty++)
            for (int tx = 0; tx < r.tw; tx++) {
                const int32_t e = px.p[(size_t)ty * r.tw + tx];
                const int x = e % w, y = e / w;
                if (e < 0 || e >= w * h || x / s != tx || y / s != ty) fail("a pixel outside its tile or the frame", w, h, s);
            }
        for (size_t t = 0; t < ntiles; t++) {
            for (int c = 0; c < 3; c++) {
                same.p[3 * t + c] = prev.p[3 * (size_t)px.p[t] + c];
                changed.p[3 * t + c] = same.p[3 * t + c] * (rng() % 3 ? 1.0f : 0.25f);
            }
            bad.p[t] = outside[rng() % 4];
            mixed.p[t] = rng() % 2 ? px.p[t] : outside[rng() % 4];
        }
        ptg::run_host_sparse(r, prev.get(), px.get(), same.get(), lam.get());
        if (!all_plus_zero(lam)) fail("equal inputs: lambda is not +0", w, h, s);
        ptg::run_host_sparse(r, prev.get(), px.get(), changed.get(), lam.get());
        for (size_t t = 0; t < lam.n; t++)
            if (!(lam.p[t] >= 0.0f && lam.p[t] <= 1.0f)) { fail("lambda outside [0, 1]", w, h, s); break; }
        ptg::run_host_sparse(r, prev.get(), bad.get(), changed.get(), lam.get());
        if (!all_plus_zero(lam)) fail("a list of entries outside the frame: lambda is not +0", w, h, s);
        ptg::run_host_sparse(r, prev.get(), mixed.get(), same.get(), lam.get());
        if (!all_plus_zero(lam)) fail("entries outside the frame among equal inputs: lambda is not +0", w, h, s);
        ptg::run_host_sparse(r, prev.get(), mixed.get(), changed.get(), lam.get());
        for (size_t t = 0; t < lam.n; t++)
            if (!(lam.p[t] >= 0.0f && lam.p[t] <= 1.0f)) { fail("lambda outside [0, 1] with a mixed list", w, h, s); break; }
    }
}

}  // namespace

int main() {
    std::mt19937 rng(20241019u);
    const int frames[][2] = {{1, 1}, {1, 2}, {2, 1}, {5, 3}, {65, 5}, {67, 5}};
    for (const auto& wh : frames)
        for (int s : {1, 2, 3, 5, 16}) {
            if (wh[1] <= s / 2) continue;
            check(wh[0], wh[1], s, rng);
        }
    if (g_errors) { std::fprintf(stderr, "%d checks failed\n", g_errors); return 1; }
    std::puts("sparse gradient rules: all held");
    return 0;
}
