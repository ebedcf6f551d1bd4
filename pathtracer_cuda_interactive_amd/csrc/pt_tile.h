// pt_tile.h — the launch shape of the image-space kernels (pt_denoise.hip, pt_temporal.hip): one thread per pixel, 64 x 4
// pixel tiles, so a wave covers 64 consecutive pixels of a row.
#pragma once

#include <hip/hip_runtime.h>

namespace pttile {

constexpr int kTileW = 64, kTileH = 4, kTileThreads = kTileW * kTileH;

inline dim3 grid(int width, int height) {
    return dim3((unsigned)((width + kTileW - 1) / kTileW), (unsigned)((height + kTileH - 1) / kTileH));
}

#ifdef __HIPCC__
// The pixel of this thread; false outside the frame.
__device__ __forceinline__ bool pixel(int width, int height, int& px, int& py) {
    px = blockIdx.x * kTileW + (threadIdx.x & (kTileW - 1));
    py = blockIdx.y * kTileH + (threadIdx.x / kTileW);
    return px < width && py < height;
}
#endif

}  // namespace pttile
