// pt_tree_cost.hip — the surface-area cost of a DNode array (pt_tree_cost.h), summed in a fixed order.
//
// A refit keeps a tree's topology, so its quality decays with the geometry; the sum of its boxes' areas — what a ray without
// pruning pays, up to a constant — says by how much.  Two launches: every workgroup reduces its own stretch of
// the array to one partial (nodes in index order per thread, lanes in lane order per wave, waves in wave order), then ONE
// workgroup adds the partials in index order.  No floating-point atomics, nothing handed between workgroups inside a launch
// (the per-XCD L2s are not coherent: DESIGN.md §18) — the result is the same bits on every run and on every grid.
#include <hip/hip_runtime.h>

#include <string>

#include "pt_internal.h"
#include "pt_layout.h"
#include "pt_tree_cost.h"

#pragma STDC FP_CONTRACT OFF

namespace {

using ptl::DNode;

#define HIPC(expr)                                                                                  \
    do {                                                                                            \
        hipError_t e_ = (expr);                                                                     \
        if (e_ != hipSuccess)                                                                       \
            return pt_fail(e_ == hipErrorNoDevice ? PT_ERR_NO_DEVICE : PT_ERR_DEVICE,                \
                           std::string(#expr) + ": " + hipGetErrorString(e_));                      \
    } while (0)

constexpr int kThreads = 256;
constexpr int kWaves = kThreads / 64;
constexpr int kItems = 4;                          // consecutive nodes per thread
constexpr int kBlockNodes = kThreads * kItems;     // nodes per partial

__device__ __forceinline__ double box_area(float lx, float ly, float lz, float hx, float hy, float hz) {
    const double ex = (double)hx - (double)lx, ey = (double)hy - (double)ly, ez = (double)hz - (double)lz;
    return 2.0 * ((ex * ey + ey * ez) + ez * ex);
}

// one 64-B record as four 16-B loads: lmin.xyz lmax.x | lmax.yz rmin.xy | rmin.z rmax.xyz | left right pad pad
__device__ __forceinline__ double node_cost(const DNode* __restrict__ nd) {
    const float4* q = reinterpret_cast<const float4*>(nd);
    const float4 a = q[0], b = q[1], c = q[2], d = q[3];
    double s = 0.0;
    if (__builtin_bit_cast(int32_t, d.x) >= 0) s = s + box_area(a.x, a.y, a.z, a.w, b.x, b.y);
    if (__builtin_bit_cast(int32_t, d.y) >= 0) s = s + box_area(b.z, b.w, c.x, c.y, c.z, c.w);
    return s;
}

__global__ __launch_bounds__(kThreads) void cost_partial_kernel(const DNode* __restrict__ nodes, int num_nodes, double* __restrict__ partials) {
    __shared__ double lane_sum[kThreads];
    __shared__ double wave_sum[kWaves];
    const int first = ((int)blockIdx.x * kThreads + (int)threadIdx.x) * kItems;
    double s = 0.0;
    for (int i = 0; i < kItems; i++)
        if (first + i < num_nodes) s = s + node_cost(nodes + first + i);
    lane_sum[threadIdx.x] = s;
    __syncthreads();
    if ((threadIdx.x & 63) == 0) {
        double w = 0.0;
        for (int l = 0; l < 64; l++) w = w + lane_sum[threadIdx.x + l];
        wave_sum[threadIdx.x >> 6] = w;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        double t = 0.0;
        for (int w = 0; w < kWaves; w++) t = t + wave_sum[w];
        partials[blockIdx.x] = t;
    }
}

__global__ __launch_bounds__(kThreads) void cost_total_kernel(const double* __restrict__ partials, int n, double* __restrict__ out) {
    __shared__ double stage[kThreads];
    double t = 0.0;                                 // thread 0's alone
    for (int base = 0; base < n; base += kThreads) {
        const int k = base + (int)threadIdx.x;
        stage[threadIdx.x] = k < n ? partials[k] : 0.0;
        __syncthreads();
        if (threadIdx.x == 0) {
            const int m = n - base < kThreads ? n - base : kThreads;
            for (int i = 0; i < m; i++) t = t + stage[i];
        }
        __syncthreads();
    }
    if (threadIdx.x == 0) *out = t;
}

}  // namespace

namespace ptc {

size_t partials_needed(int num_nodes) { return num_nodes > 0 ? ((size_t)num_nodes + kBlockNodes - 1) / kBlockNodes : 1; }

int tree_cost(const void* dnodes_dev, int num_nodes, double* partials_dev, double* out_dev) {
    if (!dnodes_dev || num_nodes <= 0 || !partials_dev || !out_dev) return pt_fail(PT_ERR_INVALID_ARG, "tree_cost: bad argument");
    const int blocks = (int)partials_needed(num_nodes);
    hipLaunchKernelGGL(cost_partial_kernel, dim3((unsigned)blocks), dim3(kThreads), 0, nullptr, static_cast<const DNode*>(dnodes_dev), num_nodes,
                       partials_dev);
    HIPC(hipGetLastError());
    hipLaunchKernelGGL(cost_total_kernel, dim3(1), dim3(kThreads), 0, nullptr, partials_dev, blocks, out_dev);
    HIPC(hipGetLastError());
    return PT_OK;
}

}  // namespace ptc
