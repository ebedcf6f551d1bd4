// pt_scene_transform.hip — the device half of pt_scene_transform: one kernel that makes the staged primitive records from the
// rest records the handle keeps and an 84-B entry per group (pt_transform.h).  Memory-bound: 196 B per shape move (96 in, 96
// out, 4 of group id); the arithmetic is 27 multiply-adds per triangle.
#include <hip/hip_runtime.h>

#include <string>

#include "pt_internal.h"
#include "pt_layout.h"
#include "pt_scene_transform.h"
#include "pt_transform.h"

namespace {

using ptl::DNormals;
using ptl::DPrim;

constexpr int kThreads = 256;

__device__ __forceinline__ float4 ld4(const void* p, int i) { return reinterpret_cast<const float4*>(p)[i]; }
__device__ __forceinline__ void st4(void* p, int i, float4 v) { reinterpret_cast<float4*>(p)[i] = v; }

// One thread per shape: six 16-B loads, six 16-B stores.  The entry comes through the cache; consecutive shapes almost always
// share a group, so a wave whose active lanes agree reads it once with a wave-uniform address.  Both paths fill the same 21
// values and run the same arithmetic on them.
__global__ __launch_bounds__(kThreads) void transform_kernel(const DPrim* __restrict__ rest_p, const DNormals* __restrict__ rest_n,
                                                             const int32_t* __restrict__ group, const float* __restrict__ table, int N,
                                                             DPrim* __restrict__ out_p, DNormals* __restrict__ out_n) {
    const int i = blockIdx.x * kThreads + threadIdx.x;
    if (i >= N) return;
    float4 a = ld4(rest_p + i, 0), b = ld4(rest_p + i, 1), c = ld4(rest_p + i, 2);          // v0..3 | v4..7 | v8 info light pad
    float4 na = ld4(rest_n + i, 0), nb = ld4(rest_n + i, 1), nc = ld4(rest_n + i, 2);       // n0..3 | n4..7 | n8 pad pad pad
    const int g = group[i];
    if (g >= 0) {
        float e[ptx::kEntryFloats];
        const int g0 = __builtin_amdgcn_readfirstlane(g);
        if (__ballot(g != g0) == 0ull) {
            const float* src = table + (size_t)g0 * ptx::kEntryFloats;
            for (int k = 0; k < ptx::kEntryFloats; k++) e[k] = src[k];
        } else {
            const float* src = table + (size_t)g * ptx::kEntryFloats;
            for (int k = 0; k < ptx::kEntryFloats; k++) e[k] = src[k];
        }
        const float* m = e;
        const float* cf = e + 12;
        if (__builtin_bit_cast(uint32_t, c.y) & 0x80000000u) {                               // sphere: centre and radius
            const ptm::V3 q = ptx::point(m, ptm::mk(a.x, a.y, a.z));
            a = make_float4(q.x, q.y, q.z, ptx::radius(m, a.w));
        } else {
            const ptm::V3 p0 = ptx::point(m, ptm::mk(a.x, a.y, a.z));
            const ptm::V3 p1 = ptx::point(m, ptm::mk(a.w, b.x, b.y));
            const ptm::V3 p2 = ptx::point(m, ptm::mk(b.z, b.w, c.x));
            a = make_float4(p0.x, p0.y, p0.z, p1.x);
            b = make_float4(p1.y, p1.z, p2.x, p2.y);
            c.x = p2.z;
            const ptm::V3 n0 = ptx::normal(cf, ptm::mk(na.x, na.y, na.z));
            const ptm::V3 n1 = ptx::normal(cf, ptm::mk(na.w, nb.x, nb.y));
            const ptm::V3 n2 = ptx::normal(cf, ptm::mk(nb.z, nb.w, nc.x));
            na = make_float4(n0.x, n0.y, n0.z, n1.x);
            nb = make_float4(n1.y, n1.z, n2.x, n2.y);
            nc.x = n2.z;
        }
    }
    st4(out_p + i, 0, a); st4(out_p + i, 1, b); st4(out_p + i, 2, c);
    st4(out_n + i, 0, na); st4(out_n + i, 1, nb); st4(out_n + i, 2, nc);
}

}  // namespace

int ptx::transform_records(const void* rest_prims_dev, const void* rest_normals_dev, const int32_t* group_dev, const float* table_dev,
                           int N, void* out_prims_dev, void* out_normals_dev) {
    if (!rest_prims_dev || !rest_normals_dev || !group_dev || !table_dev || !out_prims_dev || !out_normals_dev || N <= 0)
        return pt_fail(PT_ERR_INVALID_ARG, "transform_records: bad argument");
    const int G = (N + kThreads - 1) / kThreads;
    hipLaunchKernelGGL(transform_kernel, dim3(G), dim3(kThreads), 0, nullptr, reinterpret_cast<const DPrim*>(rest_prims_dev),
                       reinterpret_cast<const DNormals*>(rest_normals_dev), group_dev, table_dev, N, reinterpret_cast<DPrim*>(out_prims_dev),
                       reinterpret_cast<DNormals*>(out_normals_dev));
    const hipError_t err = hipGetLastError();
    if (err != hipSuccess) return pt_fail(PT_ERR_DEVICE, std::string("transform_kernel: ") + hipGetErrorString(err));
    return PT_OK;
}
