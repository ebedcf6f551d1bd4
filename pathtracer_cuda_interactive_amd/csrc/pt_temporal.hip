// pt_temporal.hip — the kernel of pt_temporal_accumulate, pt_temporal_accumulate_moments and pt_temporal_accumulate_adaptive
// (the rule and the host twins' loop: pt_temporal.h).
//
// One thread per pixel, the 64 x 4 pixel tiles of pt_tile.h: a wave covers 64 consecutive pixels of a row, so its own records
// are consecutive bytes and, where neighbouring pixels move alike, so are the two tap rows it gathers.  No LDS, no scratch:
// at most four taps, each used once.
#include <hip/hip_runtime.h>

#include "pt_temporal.h"
#include "pt_tile.h"

namespace ptt {

namespace {

// the pointers travel by value in the kernel's arguments; LAM is the Lambda of the adaptive kernel and nothing in the other two,
// whose arguments and body stay what they were
template <bool MOMENTS, bool ADAPTIVE = false, class... LAM>
__global__ __launch_bounds__(pttile::kTileThreads) void accumulate_kernel(Resolved r, float albedo_floor, pt_temporal_io io, LAM... lam) {
    int px, py;
    if (!pttile::pixel(r.width, r.height, px, py)) return;
    accumulate_pixel<MOMENTS, ADAPTIVE>(r, albedo_floor, px, py, io, lam...);
}

}  // namespace

int run_device(const Resolved& r, bool moments, float albedo_floor, const pt_temporal_io& io, const Lambda* lam, void* hip_stream) {
    const dim3 grid = pttile::grid(r.width, r.height), block(pttile::kTileThreads);
    hipStream_t stream = reinterpret_cast<hipStream_t>(hip_stream);
    if (lam)
        hipLaunchKernelGGL((accumulate_kernel<true, true, Lambda>), grid, block, 0, stream, r, albedo_floor, io, *lam);
    else
        hipLaunchKernelGGL(moments ? accumulate_kernel<true> : accumulate_kernel<false>, grid, block, 0, stream, r, albedo_floor, io);
    return (int)hipGetLastError();
}

}  // namespace ptt
