// pt_scene_refit.hip — the device half of pt_scene_update: both trees of a handle keep their topology and get exact new boxes.
// (The reference has no counterpart: it rebuilds its BVH on the host for every load, bvh.cu:16-54.)
//
// A DNode carries the boxes of its two CHILDREN, so "the box of node k" lives in k's parent, in the child slot k hangs from
// (24 bytes at offset 0 or 24 of the parent's record).  Refit = leaf boxes into their parents' slots, then level by level,
// deepest first: a node at depth d reads its own two child boxes — written by depth d + 1 or by the leaf pass — and writes
// their union into its parent's slot.  Every child of a depth-d node sits at depth d + 1, so the nodes of one level are
// independent.  Levels are separated by kernel boundaries or, inside the single-workgroup launch, by __syncthreads(); nothing
// is handed between workgroups inside a launch and nothing spins.  DESIGN.md §18.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <exception>
#include <string>

#include "pt_internal.h"
#include "pt_layout.h"
#include "pt_scene_refit.h"

namespace {

using ptl::DNode;
using ptl::DPrim;

#define HIPF(expr)                                                                                  \
    do {                                                                                            \
        hipError_t e_ = (expr);                                                                     \
        if (e_ != hipSuccess)                                                                       \
            return pt_fail(e_ == hipErrorNoDevice ? PT_ERR_NO_DEVICE : PT_ERR_DEVICE,                \
                           std::string(#expr) + ": " + hipGetErrorString(e_));                      \
    } while (0)

constexpr int kThreads = 256;
constexpr int kMaxLevels = 256;       // caller's trees: <= 64 levels (scene.h:251); the library's own: <= 2 log2 n + 18
static_assert(kThreads == kMaxLevels, "the plan kernels keep one LDS counter per level and thread");
constexpr int kNarrow = 1024;        // a level of at most this many nodes is "narrow": four nodes per thread of one workgroup
constexpr int kWholeTreeNodes = 4096; // trees up to this size whose levels are all narrow are refitted by one launch

// ---- plan -------------------------------------------------------------------------------------------------------------------

struct PlanCtl {
    unsigned int err;
    unsigned int count[kMaxLevels];   // nodes per depth; reused as the fill cursor of every level
};

__global__ void plan_links_kernel(const DNode* __restrict__ nodes, int num_nodes, int N, int32_t* __restrict__ parent_slot,
                                  int32_t* __restrict__ leaf_slot, PlanCtl* __restrict__ ctl) {
    const int k = blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= num_nodes) return;
    const int32_t child[2] = {nodes[k].left, nodes[k].right};
    for (int side = 0; side < 2; side++) {
        const int32_t c = child[side];
        if (c >= 0) {
            if (c >= num_nodes || c == 0) { atomicOr(&ctl->err, 1u); continue; }
            parent_slot[c] = 2 * k + side;
        } else {
            const int32_t prim = ~c;
            if (prim < 0 || prim >= N) { atomicOr(&ctl->err, 1u); continue; }
            leaf_slot[prim] = 2 * k + side;
        }
    }
}
// depth of every node by a walk to the root (node 0), as relay_level_kernel does it for a node pool
__global__ void plan_depth_kernel(int num_nodes, const int32_t* __restrict__ parent_slot, int32_t* __restrict__ depth,
                                  PlanCtl* __restrict__ ctl) {
    // counted per workgroup in LDS first: a million device-scope atomics on a few dozen words took most of the plan build
    __shared__ unsigned int hist[kMaxLevels];
    hist[threadIdx.x] = 0;                                // kThreads == kMaxLevels
    __syncthreads();
    const int k = blockIdx.x * blockDim.x + threadIdx.x;
    if (k < num_nodes) {
        int e = 0;
        bool ok = true;
        for (int v = k; v != 0 && ok; e++) {
            const int32_t ps = parent_slot[v];
            if (ps < 0 || e >= kMaxLevels - 1) { ok = false; break; }
            v = ps >> 1;
        }
        if (ok) {
            depth[k] = e;
            atomicAdd(&hist[e], 1u);
        } else {
            atomicOr(&ctl->err, 2u);
            depth[k] = -1;
        }
    }
    __syncthreads();
    if (hist[threadIdx.x]) atomicAdd(&ctl->count[threadIdx.x], hist[threadIdx.x]);
}
__global__ void plan_order_kernel(int num_nodes, const int32_t* __restrict__ depth, const int32_t* __restrict__ level_begin,
                                  int32_t* __restrict__ order, PlanCtl* __restrict__ ctl) {
    // a workgroup reserves its nodes' places level by level: ranks inside the workgroup from LDS, one atomic per level it holds
    __shared__ unsigned int hist[kMaxLevels];             // count of the level, then the workgroup's first place in it
    hist[threadIdx.x] = 0;                                // kThreads == kMaxLevels
    __syncthreads();
    const int k = blockIdx.x * blockDim.x + threadIdx.x;
    const int32_t d = k < num_nodes ? depth[k] : -1;
    const unsigned int rank = d >= 0 ? atomicAdd(&hist[d], 1u) : 0u;
    __syncthreads();
    if (hist[threadIdx.x]) hist[threadIdx.x] = atomicAdd(&ctl->count[threadIdx.x], hist[threadIdx.x]);
    __syncthreads();
    if (d >= 0) order[level_begin[d] + (int32_t)(hist[d] + rank)] = k;       // the order inside a level does not matter
}

__global__ void plan_leaves_kernel(const int32_t* __restrict__ leaf_slot, int N, int num_nodes, PlanCtl* __restrict__ ctl) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < N && (leaf_slot[i] < 0 || leaf_slot[i] >= 2 * num_nodes)) atomicOr(&ctl->err, 4u);
}

// ---- boxes ------------------------------------------------------------------------------------------------------------------

struct Box {
    float lo[3], hi[3];
};
__device__ __forceinline__ float hmin(float a, float b) { return a < b ? a : b; }   // vecmath.h: tmin / tmax
__device__ __forceinline__ float hmax(float a, float b) { return a > b ? a : b; }

// scene_build.cpp: one AABB per primitive
__device__ __forceinline__ Box prim_box(const DPrim& p) {
    Box b;
    if (p.info < 0) {                                     // sphere: bit 31 of info
        for (int c = 0; c < 3; c++) { b.lo[c] = p.v[c] - p.v[3]; b.hi[c] = p.v[c] + p.v[3]; }
    } else {
        for (int c = 0; c < 3; c++) {
            b.lo[c] = hmin(hmin(p.v[c], p.v[3 + c]), p.v[6 + c]);
            b.hi[c] = hmax(hmax(p.v[c], p.v[3 + c]), p.v[6 + c]);
        }
    }
    return b;
}
__device__ __forceinline__ bool box_finite(const Box& b) {
    bool ok = true;
    for (int c = 0; c < 3; c++) ok = ok && __builtin_isfinite(b.lo[c]) && __builtin_isfinite(b.hi[c]);
    return ok;
}
// every coordinate the box was made from: `a < b ? a : b` drops a NaN in its first argument, so a finite box does not prove it
__device__ __forceinline__ bool prim_finite(const DPrim& p) {
    const int n = p.info < 0 ? 4 : 9;                     // sphere: centre and radius
    bool ok = true;
    for (int c = 0; c < 9; c++) ok = ok && (c >= n || __builtin_isfinite(p.v[c]));
    return ok;
}
// a box into child slot `slot` = node * 2 + side: 24 bytes at offset 0 or 24 of a 64-byte aligned record
__device__ __forceinline__ void store_slot(DNode* __restrict__ nodes, int32_t slot, const Box& b) {
    float2* at = reinterpret_cast<float2*>(reinterpret_cast<float*>(nodes + (slot >> 1)) + 6 * (slot & 1));
    at[0] = make_float2(b.lo[0], b.lo[1]);
    at[1] = make_float2(b.lo[2], b.hi[0]);
    at[2] = make_float2(b.hi[1], b.hi[2]);
}
// node k's own box = the union of its two child boxes, into its parent's slot
__device__ __forceinline__ void lift_node(DNode* __restrict__ nodes, int32_t k, const int32_t* __restrict__ parent_slot) {
    const int32_t slot = parent_slot[k];
    if (slot < 0) return;                                 // the root's box is never tested
    const float4* rec = reinterpret_cast<const float4*>(nodes + k);
    const float4 a = rec[0], b = rec[1], c = rec[2];      // lmin.xyz lmax.x | lmax.yz rmin.xy | rmin.z rmax.xyz
    Box u;
    u.lo[0] = hmin(a.x, b.z); u.lo[1] = hmin(a.y, b.w); u.lo[2] = hmin(a.z, c.x);
    u.hi[0] = hmax(a.w, c.y); u.hi[1] = hmax(b.x, c.z); u.hi[2] = hmax(b.y, c.w);
    store_slot(nodes, slot, u);
}

__global__ void leaf_boxes_kernel(const DPrim* __restrict__ prims, int N, float* __restrict__ boxes, unsigned int* __restrict__ status) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= N) return;
    const DPrim p = prims[i];
    const Box b = prim_box(p);
    float* o = boxes + 6 * (size_t)i;
    for (int c = 0; c < 3; c++) { o[c] = b.lo[c]; o[3 + c] = b.hi[c]; }
    if (!prim_finite(p) || !box_finite(b)) atomicOr(status, 1u);
}
__global__ void scatter_leaves_kernel(const float* __restrict__ boxes, int N, const int32_t* __restrict__ leaf_slot, DNode* __restrict__ nodes) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= N) return;
    const float* s = boxes + 6 * (size_t)i;
    Box b;
    for (int c = 0; c < 3; c++) { b.lo[c] = s[c]; b.hi[c] = s[3 + c]; }
    store_slot(nodes, leaf_slot[i], b);
}
// the other way round (pt_scene_rebuild): every node hands the boxes of its leaf children to boxes[prim]
__global__ void gather_leaves_kernel(const DNode* __restrict__ nodes, int num_nodes, int N, float* __restrict__ boxes) {
    const int k = blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= num_nodes) return;
    const float4* rec = reinterpret_cast<const float4*>(nodes + k);
    const float4 a = rec[0], b = rec[1], c = rec[2];      // lmin.xyz lmax.x | lmax.yz rmin.xy | rmin.z rmax.xyz
    const int32_t left = nodes[k].left, right = nodes[k].right;
    if (left < 0 && ~left < N) {
        float* o = boxes + 6 * (size_t)~left;
        o[0] = a.x; o[1] = a.y; o[2] = a.z; o[3] = a.w; o[4] = b.x; o[5] = b.y;
    }
    if (right < 0 && ~right < N) {
        float* o = boxes + 6 * (size_t)~right;
        o[0] = b.z; o[1] = b.w; o[2] = c.x; o[3] = c.y; o[4] = c.z; o[5] = c.w;
    }
}
// one wide level: order[begin .. begin + count)
__global__ void lift_level_kernel(DNode* __restrict__ nodes, const int32_t* __restrict__ order, int begin, int count,
                                  const int32_t* __restrict__ parent_slot) {
    const int j = blockIdx.x * blockDim.x + threadIdx.x;
    if (j < count) lift_node(nodes, order[begin + j], parent_slot);
}
// ONE workgroup: levels top_level .. 1, a barrier between them (the stores of a level and the loads of the next are this
// workgroup's own, on one CU).  N > 0: the leaf pass first, from the staged records, nothing written unless every record and
// every box is finite.  nodes_oct: the 8 octant tables at the end (pt_scene_life.hip: upload_tree — octant bit k set <=> the two planes of axis k
// trade places).
__global__ __launch_bounds__(kThreads) void refit_top_kernel(DNode* __restrict__ nodes, DNode* __restrict__ nodes_oct, int num_nodes,
                                                             const int32_t* __restrict__ parent_slot, const int32_t* __restrict__ leaf_slot,
                                                             const int32_t* __restrict__ order, const int32_t* __restrict__ level_begin,
                                                             int top_level, const DPrim* __restrict__ prims, int N,
                                                             unsigned int* __restrict__ status) {
    if (blockIdx.x != 0) return;
    const int tid = threadIdx.x;
    if (N > 0) {
        int bad = 0;
        for (int i = tid; i < N; i += kThreads) {
            const DPrim p = prims[i];
            bad |= prim_finite(p) && box_finite(prim_box(p)) ? 0 : 1;
        }
        if (__syncthreads_or(bad)) {
            if (tid == 0) atomicOr(status, 1u);
            return;
        }
        for (int i = tid; i < N; i += kThreads) store_slot(nodes, leaf_slot[i], prim_box(prims[i]));
        __syncthreads();
    }
    for (int d = top_level; d >= 1; d--) {
        const int begin = level_begin[d], end = level_begin[d + 1];
        for (int j = begin + tid; j < end; j += kThreads) lift_node(nodes, order[j], parent_slot);
        __syncthreads();
    }
    if (nodes_oct) {
        for (int j = tid; j < 8 * num_nodes; j += kThreads) {
            const int o = j / num_nodes, k = j - o * num_nodes;
            DNode n = nodes[k];
            for (int ax = 0; ax < 3; ax++)
                if (o & (1 << ax)) {
                    float t = n.lmin[ax]; n.lmin[ax] = n.lmax[ax]; n.lmax[ax] = t;
                    t = n.rmin[ax]; n.rmin[ax] = n.rmax[ax]; n.rmax[ax] = t;
                }
            nodes_oct[j] = n;
        }
    }
}
int grid_for(int n) { return (n + kThreads - 1) / kThreads; }

}  // namespace

void ptf::plan_release(Plan* p) {
    if (p->arena) (void)hipFree(p->arena);
    *p = Plan();
}

int ptf::plan_build(const void* dnodes_dev, int num_nodes, int N, Plan* out) {
    if (!dnodes_dev || !out || N < 2 || num_nodes != N - 1) return pt_fail(PT_ERR_INVALID_ARG, "refit plan: bad argument");
    plan_release(out);
    const DNode* nodes = reinterpret_cast<const DNode*>(dnodes_dev);
    const size_t nn = (size_t)num_nodes;
    auto round256 = [](size_t b) { return (b + 255) & ~(size_t)255; };
    const size_t o_parent = 0, o_leaf = o_parent + round256(nn * 4), o_order = o_leaf + round256((size_t)N * 4),
                 o_begin = o_order + round256(nn * 4), total = o_begin + round256((kMaxLevels + 1) * 4);
    unsigned char* arena = nullptr;
    HIPF(hipMalloc(reinterpret_cast<void**>(&arena), total));
    out->arena = arena;
    out->parent_slot = reinterpret_cast<int32_t*>(arena + o_parent);
    out->leaf_slot = reinterpret_cast<int32_t*>(arena + o_leaf);
    out->order = reinterpret_cast<int32_t*>(arena + o_order);
    out->level_begin = reinterpret_cast<int32_t*>(arena + o_begin);
    // working memory of the build only: every node's depth, and the counters
    unsigned char* tmp = nullptr;
    const size_t o_ctl = round256(nn * 4);
    if (hipMalloc(reinterpret_cast<void**>(&tmp), o_ctl + sizeof(PlanCtl)) != hipSuccess) {
        plan_release(out);
        return pt_fail(PT_ERR_DEVICE, "refit plan: out of device memory");
    }
    struct Free { void* p; ~Free() { (void)hipFree(p); } } tmp_guard{tmp};
    int32_t* depth = reinterpret_cast<int32_t*>(tmp);
    PlanCtl* ctl = reinterpret_cast<PlanCtl*>(tmp + o_ctl);
    auto bail = [&](int rc) { plan_release(out); return rc; };
    PlanCtl h;
    // 0xff: "no parent" / "no leaf" — a slot that stays so is an inconsistent array and fails the build below
    if (hipMemsetAsync(arena, 0xff, o_order, nullptr) != hipSuccess || hipMemsetAsync(ctl, 0, sizeof(PlanCtl), nullptr) != hipSuccess)
        return bail(pt_fail(PT_ERR_DEVICE, "refit plan: memset failed"));
    const int G = grid_for(num_nodes);
    hipLaunchKernelGGL(plan_links_kernel, dim3(G), dim3(kThreads), 0, nullptr, nodes, num_nodes, N, out->parent_slot, out->leaf_slot, ctl);
    hipLaunchKernelGGL(plan_depth_kernel, dim3(G), dim3(kThreads), 0, nullptr, num_nodes, out->parent_slot, depth, ctl);
    if (hipGetLastError() != hipSuccess || hipMemcpy(&h, ctl, sizeof h, hipMemcpyDeviceToHost) != hipSuccess)
        return bail(pt_fail(PT_ERR_DEVICE, "refit plan: kernels failed"));
    if (h.err) return bail(pt_fail(PT_ERR_UNSUPPORTED, "refit plan: the node array is not a tree of at most 256 levels rooted at node 0"));
    int levels = 0;
    size_t seen = 0;
    std::vector<int32_t>& lb = out->level_begin_host;
    lb.assign(kMaxLevels + 1, 0);
    for (int d = 0; d < kMaxLevels; d++) {
        lb[d] = (int32_t)seen;
        seen += h.count[d];
        if (h.count[d]) levels = d + 1;
    }
    lb[kMaxLevels] = (int32_t)seen;
    if (seen != nn || h.count[0] != 1) return bail(pt_fail(PT_ERR_UNSUPPORTED, "refit plan: inconsistent node array"));
    if (hipMemcpy(out->level_begin, lb.data(), lb.size() * sizeof(int32_t), hipMemcpyHostToDevice) != hipSuccess ||
        hipMemsetAsync(ctl, 0, sizeof(PlanCtl), nullptr) != hipSuccess)
        return bail(pt_fail(PT_ERR_DEVICE, "refit plan: upload failed"));
    hipLaunchKernelGGL(plan_order_kernel, dim3(G), dim3(kThreads), 0, nullptr, num_nodes, depth, out->level_begin, out->order, ctl);
    // every primitive must have found its leaf (leaf_slot is what the scatter indexes the node array with): count of leaf
    // slots = 2 * inner nodes - (inner nodes - 1) = N holds for any binary tree that passed the checks above with in-range,
    // distinct children; a primitive named twice would leave another one without a slot.  Checked where the table lives: one
    // word comes back, not 4 bytes per primitive.
    hipLaunchKernelGGL(plan_leaves_kernel, dim3(grid_for(N)), dim3(kThreads), 0, nullptr, out->leaf_slot, N, num_nodes, ctl);
    unsigned int leaf_err = 1;
    if (hipGetLastError() != hipSuccess || hipMemcpy(&leaf_err, &ctl->err, sizeof leaf_err, hipMemcpyDeviceToHost) != hipSuccess)
        return bail(pt_fail(PT_ERR_DEVICE, "refit plan: kernels failed"));
    if (leaf_err) return bail(pt_fail(PT_ERR_UNSUPPORTED, "refit plan: a primitive has no leaf"));
    out->levels = levels;
    int top = 0;
    while (top + 1 < levels && lb[top + 2] - lb[top + 1] <= kNarrow) top++;
    out->narrow_top = top;
    out->whole_tree = top == levels - 1 && num_nodes <= kWholeTreeNodes;
    out->built = true;
    return PT_OK;
}

int ptf::leaf_boxes(const void* prims_dev, int N, float* boxes_dev, unsigned int* status_dev) {
    hipLaunchKernelGGL(leaf_boxes_kernel, dim3(grid_for(N)), dim3(kThreads), 0, nullptr, reinterpret_cast<const DPrim*>(prims_dev), N,
                       boxes_dev, status_dev);
    HIPF(hipGetLastError());
    return PT_OK;
}

int ptf::tree_leaf_boxes(const void* dnodes_dev, int num_nodes, int N, float* boxes_dev) {
    if (!dnodes_dev || !boxes_dev || N < 2 || num_nodes != N - 1) return pt_fail(PT_ERR_INVALID_ARG, "leaf boxes of a tree: bad argument");
    hipLaunchKernelGGL(gather_leaves_kernel, dim3(grid_for(num_nodes)), dim3(kThreads), 0, nullptr, reinterpret_cast<const DNode*>(dnodes_dev),
                       num_nodes, N, boxes_dev);
    HIPF(hipGetLastError());
    return PT_OK;
}

int ptf::refit_tree(const Plan& plan, void* dnodes_dev, void* dnodes_oct_dev, int num_nodes, const void* prims_dev,
                    const float* boxes_dev, int N, unsigned int* status_dev) {
    if (!plan.built || !dnodes_dev || num_nodes != N - 1) return pt_fail(PT_ERR_INVALID_ARG, "refit: bad argument");
    // octant tables exist only for trees small enough for LDS, far below kWholeTreeNodes: the single-workgroup launch makes them
    if (dnodes_oct_dev && !plan.whole_tree) return pt_fail(PT_ERR_INVALID_ARG, "refit: octant tables on a tree of wide levels");
    DNode* nodes = reinterpret_cast<DNode*>(dnodes_dev);
    DNode* oct = reinterpret_cast<DNode*>(dnodes_oct_dev);
    const DPrim* prims = reinterpret_cast<const DPrim*>(prims_dev);
    if (plan.whole_tree) {
        hipLaunchKernelGGL(refit_top_kernel, dim3(1), dim3(kThreads), 0, nullptr, nodes, oct, num_nodes, plan.parent_slot, plan.leaf_slot,
                           plan.order, plan.level_begin, plan.levels - 1, prims, N, status_dev);
        HIPF(hipGetLastError());
        return PT_OK;
    }
    if (!boxes_dev) return pt_fail(PT_ERR_INVALID_ARG, "refit: leaf boxes missing");
    hipLaunchKernelGGL(scatter_leaves_kernel, dim3(grid_for(N)), dim3(kThreads), 0, nullptr, boxes_dev, N, plan.leaf_slot, nodes);
    for (int d = plan.levels - 1; d > plan.narrow_top; d--) {
        const int begin = plan.level_begin_host[d], count = plan.level_begin_host[d + 1] - begin;
        hipLaunchKernelGGL(lift_level_kernel, dim3(grid_for(count)), dim3(kThreads), 0, nullptr, nodes, plan.order, begin, count, plan.parent_slot);
    }
    if (plan.narrow_top >= 1)
        hipLaunchKernelGGL(refit_top_kernel, dim3(1), dim3(kThreads), 0, nullptr, nodes, static_cast<DNode*>(nullptr), num_nodes,
                           plan.parent_slot, plan.leaf_slot, plan.order, plan.level_begin, plan.narrow_top, static_cast<const DPrim*>(nullptr), 0,
                           status_dev);
    HIPF(hipGetLastError());
    return PT_OK;
}
