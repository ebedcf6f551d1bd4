// pt_kernels.h — the gfx950 kernels of the path tracer (included only by pt_api.hip).
//
//   trace_kernel_v2<RES,PRUNE,STATS,THRESH,INNER,MINW,SPEC>   persistent wavefront path tracer with decoupled
//        traversal / shading scheduling (default).  Replaces render + setup_rand (main.cu:30-62) and all they call.
//   trace_kernel<LDS_SCENE,PRUNE,STATS>   the simpler segment-synchronous schedule (option "kernel" = 1).
//   resolve_kernel     ordered per-pixel sum of the per-sample radiances (main.cu:47,50 / 72-86).
//   intersect_kernel, math_kernel, exact_math_kernel   test hooks behind pt_debug_*.
#pragma once

#include <hip/hip_runtime.h>

#include <type_traits>

#include "pt_layout.h"
#include "pt_leaf_sweep.h"
#include "pt_math.h"
#include "pt_path_bank.h"
#include "pt_path_index.h"
#include "pt_sweep_layout.h"
#include "pt_sweep_families.h"
#include "pt_sweep_skip.h"
#include "pt_sweep_pairs.h"
#include "pt_temporal.h"
#include "pt_trace.h"

namespace ptk {

using namespace ptl;


#ifndef PT_BLOCK
#define PT_BLOCK 256
#endif
constexpr int kBlock = PT_BLOCK;     // 4 waves (PT_BLOCK: block-size experiments)
constexpr uint32_t kMaxChunk = 256;  // most work items a wave reserves per atomic (RenderDev::chunk)

__device__ __forceinline__ uint32_t lane_rank(unsigned long long mask) {
    return __builtin_amdgcn_mbcnt_hi((uint32_t)(mask >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)mask, 0u));
}

__device__ __forceinline__ unsigned long long wave_sum(unsigned long long v) {
    for (int off = 32; off > 0; off >>= 1) v += __shfl_down(v, off, 64);
    return v;
}


// ---- work distribution ---------------------------------------------------------------------------------------
// The frame is cut into rp.num_regions bands of rows.  A wave first serves the band that belongs to the XCD it runs
// on (HW_REG_XCC_ID), so the rays an XCD's L2 sees start in 1/8 of the image; when that band is exhausted it steals
// from the next ones.  Each band has its own work counter (128 B apart); a wave reserves rp.chunk items per atomic
// (256 for full frames; down to 64 for small launches so that every resident wave gets work).
// Placement only affects speed: every work item is rendered exactly once whatever XCD picks it up.
constexpr int kCounterStride = 32;   // uint32 slots between region counters (one 128-B line each)

struct WorkFeed {
    uint32_t cur, end;       // reserved chunk [cur, end) of region-local item ids
    uint32_t region;
    uint32_t tried;          // regions found exhausted so far
    bool exhausted;
};

__device__ __forceinline__ void feed_init(WorkFeed& f, const RenderDev& rp) {
    f.cur = 0; f.end = 0; f.tried = 0; f.exhausted = false;
    const uint32_t xcc = (uint32_t)__builtin_amdgcn_s_getreg(6164) & 15u;     // hwreg(HW_REG_XCC_ID, 0, 4)
    f.region = xcc % (uint32_t)rp.num_regions;
}

// Wave-uniform.  Makes sure a non-empty chunk is reserved unless every region is exhausted.
// (Issuing the next reservation ahead of time, to take the atomic's round trip off the critical path, was measured and
// rejected: the pending result costs more than it hides — cbox +5.5 %, profiles/r02_tune_round36_*.log.)
__device__ __forceinline__ void feed_reserve(WorkFeed& f, const RenderDev& rp, uint32_t* work_counters, int lane) {
    while (f.cur >= f.end && !f.exhausted) {
        const uint32_t total = region_rows(rp, f.region) * (uint32_t)rp.width * (uint32_t)rp.spp_pass;
        const uint32_t chunk = rp.chunk;
        uint32_t base = 0;
        if (lane == 0) base = atomicAdd(&work_counters[f.region * kCounterStride], chunk);
        base = __builtin_amdgcn_readfirstlane(base);
        if (base < total) {
            f.cur = base;
            f.end = min(base + chunk, total);
        } else if (++f.tried >= (uint32_t)rp.num_regions) {
            f.exhausted = true;
        } else {
            f.region = (f.region + 1) % (uint32_t)rp.num_regions;
        }
    }
}

struct PathStart {
    ptd::Ray ray;
    ptm::Pcg rng;
    uint32_t sample_index;   // slot in the sample-major scratch buffer
};

// main.cu:32-44 for region-local work item `item` of `region`: (sample, pixel) -> PCG stream, jitter, primary ray.
template <bool LIST = false>
__device__ __forceinline__ PathStart start_path(const RenderDev& rp, uint32_t region, uint32_t item) {
    const PathIndex px = path_index<LIST>(rp, region, item);
    PathStart ps;
    ps.rng = ptm::pcg_init(px.stream, rp.seed);
    const float ru = ptm::pcg_float(ps.rng);
    const float u = ((float)px.col + ru) / (float)px.img_width;
    const float rv = ptm::pcg_float(ps.rng);
    const float v = ((float)px.j + rv) / (float)rp.height;
    ps.ray = ptd::primary_ray(rp, u, v);
    ps.sample_index = px.sample_index;
    return ps;
}

// The launch constants read again from the kernel-argument segment, where the runtime put them.  The bank's generation step
// uses this copy: it runs once per 64 paths, and what only it needs of RenderDev (three camera vectors, height, seed, ...)
// then no longer occupies scalar registers across the whole trace loop, where they overflowed into lanes of a VGPR and were
// read back inside the traversal burst.  The empty asm keeps the loads from being hoisted out of the loop again.
// Both forms of the copy load the same bytes.  WORDS exists for the register allocator alone: which form ends without
// a stack slot differs between the STATS builds (word by word) and the others (block copy); see the ScratchSize of the
// instantiations in the assembly metadata before changing it.
struct TraceKernelArgs {             // the parameter list of the trace kernels, for offsetof
    SceneDev scn; RenderDev rp; LdsPlan lp; float4* samples; uint32_t* work_counter; unsigned long long* counters;
};
template <bool WORDS>
__device__ __forceinline__ RenderDev reload_render_args() {
    typedef const __attribute__((address_space(4))) unsigned char* KernargPtr;
    KernargPtr p = (KernargPtr)__builtin_amdgcn_kernarg_segment_ptr();
    asm volatile("" : "+s"(p));
    if (WORDS) {
        struct Words { uint32_t w[sizeof(RenderDev) / 4]; };
        typedef const __attribute__((address_space(4))) uint32_t* WordPtr;
        WordPtr q = (WordPtr)(p + offsetof(TraceKernelArgs, rp));
        Words v;
#pragma unroll
        for (uint32_t i = 0; i < sizeof(RenderDev) / 4; i++) v.w[i] = q[i];
        return __builtin_bit_cast(RenderDev, v);
    }
    RenderDev r;
    __builtin_memcpy(&r, (const void*)(p + offsetof(TraceKernelArgs, rp)), sizeof(RenderDev));
    return r;
}

// Path bank (pt_path_bank.h): trace_kernel_v2 instantiations on LDS-resident scenes of triangles with diffuse materials
// generate path starts 64 at a time at full wave width and hand them out in the scheduler phase.  -DPT_PATH_BANK=0 builds
// every kernel with the per-phase start_path (A/B library).
#ifndef PT_PATH_BANK
#define PT_PATH_BANK 1
#endif
// Only the default schedule of LDS-resident scenes (THRESH 40, burst 162: pt_api.hip, pick_kernel_v2) takes the bank: every
// such instantiation keeps ScratchSize 0 at its register cap with the five bank registers, while some of the other burst
// shapes, compiled in for tuning runs, would start to spill; those keep the per-phase start_path.
constexpr bool path_bank_on(int res, int spec, bool nee, bool list, int thresh, int inner) {
    return PT_PATH_BANK && (res == 1 || res == 2) && spec == 2 && !nee && !list && thresh == 40 && inner == 162;
}

// Which bank kernels also carry the item's index (BankIndex: three more registers per lane) and hand it out in place of
// computing path_index again in the lane that takes a path.  The sweep kernel always does (pt_trace_sweep_body.h).  Of the
// tree kernels those that keep ScratchSize 0 and their occupancy with it: at 5 blocks per CU the register-stack kernels and the
// LDS-stack kernels that do not count; every instantiation at 6 blocks per CU sits at its cap of 80 registers and would spill
// (profiles/r13_phase_overhead.log §2).
constexpr bool bank_index_on(bool reg, bool stats, int minw) { return minw <= 5 && (reg || !stats); }

__device__ __forceinline__ void stage_to_lds(void* dst, const void* src, uint32_t bytes) {
    float4* d = reinterpret_cast<float4*>(dst);
    const float4* s = reinterpret_cast<const float4*>(src);
    for (uint32_t i = threadIdx.x; i < bytes / 16; i += blockDim.x) d[i] = s[i];
}

// Node placement in LDS: kLdsNodeStride bytes between consecutive nodes of a table.  64 = densely packed (4 bank
// positions for ds_read_b128), 80 = 16 bank positions.  Set by -DPT_LDS_NODE_STRIDE for experiments.
#ifndef PT_LDS_NODE_STRIDE
#define PT_LDS_NODE_STRIDE 64
#endif
constexpr uint32_t kLdsNodeStride = PT_LDS_NODE_STRIDE;
__device__ __forceinline__ void stage_nodes_to_lds(void* dst, const DNode* src, uint32_t n) {
    const float4* s = reinterpret_cast<const float4*>(src);
    for (uint32_t i = threadIdx.x; i < n * 4; i += blockDim.x)
        *reinterpret_cast<float4*>(reinterpret_cast<unsigned char*>(dst) + (i >> 2) * kLdsNodeStride + (i & 3) * 16) = s[i];
}

// The scene as this kernel instantiation sees it: staged into LDS by the whole workgroup (small scenes) or read in
// place from global memory.  Must be called by every thread of the block (it contains a __syncthreads()).
// RES = residency of the scene: 0 global memory, 1 staged in LDS, 2 staged in LDS with 8 ray-octant node tables,
// 3 global memory with the top of the tree cached in LDS.
template <int RES>
__device__ __forceinline__ ptd::SceneView make_scene_view(const SceneDev& scn, const LdsPlan& lp, unsigned char* smem) {
    ptd::SceneView sv;
    sv.top_nodes = nullptr;
    sv.top_count = 0;
    if (RES == 1 || RES == 2) {
        const uint32_t oct_pitch = oct_table_pitch((uint32_t)scn.num_nodes, kLdsNodeStride);
        if (RES == 2) {
            for (uint32_t o = 0; o < 8; o++)
                stage_nodes_to_lds(smem + lp.nodes_off + o * oct_pitch, scn.nodes_oct + (size_t)o * scn.num_nodes, (uint32_t)scn.num_nodes);
        } else {
            stage_nodes_to_lds(smem + lp.nodes_off, scn.nodes, (uint32_t)scn.num_nodes);
        }
        stage_to_lds(smem + lp.prims_off, scn.prims, (uint32_t)scn.num_prims * sizeof(DPrim));
        stage_to_lds(smem + lp.normals_off, scn.normals, (uint32_t)scn.num_prims * sizeof(DNormals));
        stage_to_lds(smem + lp.mats_off, scn.materials, (uint32_t)scn.num_materials * sizeof(DMaterial));
        stage_to_lds(smem + lp.emis_off, scn.emission, (uint32_t)scn.num_emission * sizeof(DEmission));
        __syncthreads();
        sv.nodes = reinterpret_cast<const DNode*>(smem + lp.nodes_off);
        sv.prims = reinterpret_cast<const DPrim*>(smem + lp.prims_off);
        sv.normals = reinterpret_cast<const DNormals*>(smem + lp.normals_off);
        sv.materials = reinterpret_cast<const DMaterial*>(smem + lp.mats_off);
        sv.emission = reinterpret_cast<const DEmission*>(smem + lp.emis_off);
        sv.node_stride = kLdsNodeStride;
        sv.oct_stride = RES == 2 ? oct_pitch : 0u;
    } else {
        if (RES == 3) {              // top of the tree (nodes [0, top_count), breadth-first) staged next to the stacks
            stage_to_lds(smem + lp.nodes_off, scn.nodes, lp.top_count * (uint32_t)sizeof(DNode));
            __syncthreads();
            sv.top_nodes = reinterpret_cast<const DNode*>(smem + lp.nodes_off);
            sv.top_count = lp.top_count;
        }
        sv.nodes = scn.nodes; sv.prims = scn.prims; sv.normals = scn.normals;
        sv.materials = scn.materials; sv.emission = scn.emission;
        sv.node_stride = sizeof(DNode);
        sv.oct_stride = 0;
    }
    sv.lights = scn.lights;
    sv.num_emission = scn.num_emission;
    sv.root_ref = scn.root_ref;
    sv.fixed_order = scn.fixed_order;
    sv.ref_nodes = scn.ref_nodes; sv.ref_path = scn.ref_path; sv.ref_anc = scn.ref_anc; sv.ref_levels = scn.ref_levels;
    sv.bg = ptm::mk(scn.bg[0], scn.bg[1], scn.bg[2]);
    return sv;
}

// pt_counters: per-wave sums, one atomic per wave and counter.  Same-address atomics serialise in L2 (~5 ns each:
// 12 k of them at the end of a 6144-wave launch were ~60 us of every frame), so the sums are spread over kCounterSlots
// slots of one 128-B line each, picked by workgroup id; the host adds the slots up (pt_get_counters).
// Slot layout (uint64): [0] paths [1] segments [2] node visits [3] leaf tests [4..11] schedule diagnostics
// [12] segments traced on the caller's tree in reference order (exact traversal on the internal tree: zero direction component).
// After the slots: launch timeline [kTimelineBase + 0..7] and two 128-bin histograms (STATS builds only).
constexpr int kCounterSlots = 64;
constexpr int kSlotStride = 16;
constexpr int kTimelineBase = kCounterSlots * kSlotStride;
constexpr int kNumCounters = kTimelineBase + 8 + 2 * 128;

__device__ __forceinline__ unsigned long long* counter_slot(unsigned long long* counters) {
    return counters + (blockIdx.x % kCounterSlots) * kSlotStride;
}

template <bool STATS>
__device__ __forceinline__ void flush_counters(unsigned long long* counters, int lane, uint32_t n_paths, uint32_t n_segs,
                                               const ptd::TravStats& st) {
    const unsigned long long a = wave_sum(n_paths), b = wave_sum(n_segs);
    const unsigned long long c = STATS ? wave_sum(st.nodes) : 0ull, d = STATS ? wave_sum(st.leaves) : 0ull;
    if (lane == 0) {
        unsigned long long* slot = counter_slot(counters);
        atomicAdd(&slot[0], a);
        atomicAdd(&slot[1], b);
        if (STATS) { atomicAdd(&slot[2], c); atomicAdd(&slot[3], d); }
    }
}

template <bool LDS_SCENE, bool PRUNE, bool STATS, bool LIST = false>
__global__ __launch_bounds__(kBlock) void trace_kernel(SceneDev scn, RenderDev rp, LdsPlan lp,
                                                       float4* __restrict__ samples,
                                                       uint32_t* __restrict__ work_counter,
                                                       unsigned long long* __restrict__ counters) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    const ptd::SceneView sv = make_scene_view<(LDS_SCENE ? 1 : 0)>(scn, lp, smem);

    const int lane = threadIdx.x & 63;
    const int wave = threadIdx.x >> 6;
    int32_t* stk = reinterpret_cast<int32_t*>(smem + lp.stack_off) + (size_t)wave * scn.stack_cap * 64 + lane;

    WorkFeed feed;
    feed_init(feed, rp);
    bool alive = false;
    ptd::Ray ray;
    ptm::V3 L = ptm::mk(0, 0, 0), T = ptm::mk(1, 1, 1);
    ptm::Pcg rng;
    rng.state = 0; rng.inc = 1;
    int depth = 0;
    uint32_t my_w = 0;
    uint32_t n_paths = 0, n_segs = 0;
    ptd::TravStats st;
    st.nodes = 0; st.leaves = 0;
    ray.org = ptm::mk(0, 0, 0); ray.dir = ptm::mk(0, 0, 1); ray.tnear = 0; ray.tfar = 0;

    for (;;) {
        // ---- refill dead lanes with new paths
        const unsigned long long need = __ballot(!alive);
        if (need) {
            feed_reserve(feed, rp, work_counter, lane);
            const uint32_t avail = feed.end - feed.cur;
            if (avail) {
                const uint32_t rank = lane_rank(need);
                const uint32_t n = (uint32_t)__popcll(need);
                if (!alive && rank < avail) {
                    const PathStart ps = start_path<LIST>(rp, feed.region, feed.cur + rank);
                    ray = ps.ray;
                    rng = ps.rng;
                    my_w = ps.sample_index;
                    L = ptm::mk(0, 0, 0);
                    T = ptm::mk(1, 1, 1);
                    depth = 0;
                    alive = true;
                    n_paths++;
                }
                feed.cur += min(n, avail);
            }
        }
        if (!__any(alive)) {
            if (feed.exhausted) break;
            continue;
        }
        // ---- one path segment per live lane (radiance.cuh:24-75)
        if (alive) {
            n_segs++;
            const ptd::Hit h = ptd::intersect<PRUNE, STATS>(sv, ray, stk, st);
            bool cont = false;
            if (h.prim < 0) {
                L = L + T * sv.bg;                          // radiance.cuh:27-30
            } else {
                const ptd::Surface sf = ptd::make_surface<false>(sv, ray, h);
                cont = ptd::shade_and_bounce<false>(sv, sf, ray, rng, L, T, depth, rp.rr_depth);
                depth++;
                if (depth >= rp.max_depth) cont = false;
            }
            if (!cont) {
                samples[my_w] = make_float4(L.x, L.y, L.z, 0.0f);
                alive = false;
            }
        }
    }
    // ---- work counters (pt_counters)
    flush_counters<STATS>(counters, lane, n_paths, n_segs, st);
}

// trace_kernel_v2 — same work, different schedule: traversal is decoupled from shading.
// Every lane runs a small state machine {traversing | waiting for the scheduler phase}.  The wave keeps
// executing traversal steps (a burst of inner-node visits and leaf tests per iteration, shaped by INNER: see the
// burst code below) for the lanes that still traverse; lanes whose traversal finished wait until at least THRESH lanes can make progress in the
// scheduler phase, which then (1) shades the finished segments, (2) refills dead lanes with new paths and
// (3) starts the next traversal — so the traversal loop runs with mostly full waves instead of draining to
// the slowest ray of every segment.  Per-lane arithmetic is untouched: results stay bit-identical.
// SPEC = specialisation on scene content: 0 generic, 1 no spheres, 2 no spheres and only diffuse materials.
// RES = where the scene lives (make_scene_view): 0 global memory, 1 LDS, 2 LDS with octant node tables, 3 global memory
// with the top of the tree cached in LDS.  MINW = minimum waves per SIMD the register allocation must allow.
// NEE = built with next-event estimation (PT_RENDER_NEE): a lane alternates between closest-hit traversals and the
// any-hit traversal of its light sample's shadow ray; the same step functions serve both.
// LIST = adaptive rounds after the first (start_path).
// REG = the traversal stack is a register (ptd::RegStack) instead of an LDS column: the host launches these instantiations
// where reg_stack_on holds, with an LdsPlan that has no stack columns.  Same nodes, same leaves, same order.
// The body is csrc/pt_trace_v2_body.h, included into the two kernels below it: trace_kernel_v2 (REG = false) and
// trace_kernel_v2_reg (REG = true; the schedule and scene content it is compiled for are fixed).  One text, two kernels with
// their own parameters: a shared device function taking the launch arguments by reference changed the register allocation of
// kernels this flag does not concern (scene1's +3.5 %: profiles/r10_reg_stack.log §3).
template <int RES, bool PRUNE, bool STATS, int THRESH, int INNER, int MINW, int SPEC, bool NEE = false, bool LIST = false>
__global__ __launch_bounds__(kBlock, (kBlock > 256 ? 1 : MINW)) void trace_kernel_v2(SceneDev scn, RenderDev rp, LdsPlan lp,
                                                          float4* __restrict__ samples,
                                                          uint32_t* __restrict__ work_counter,
                                                          unsigned long long* __restrict__ counters) {
    constexpr bool REG = false;
#include "pt_trace_v2_body.h"
}

// The register-stack kernels: the default schedule of LDS-resident scenes (THRESH 40, burst 162) on triangles with diffuse
// materials (SPEC 2), no next-event estimation, no pixel list.
template <int RES, bool PRUNE, bool STATS, int MINW>
__global__ __launch_bounds__(kBlock, (kBlock > 256 ? 1 : MINW)) void trace_kernel_v2_reg(SceneDev scn, RenderDev rp, LdsPlan lp,
                                                              float4* __restrict__ samples,
                                                              uint32_t* __restrict__ work_counter,
                                                              unsigned long long* __restrict__ counters) {
    constexpr int THRESH = 40, INNER = 162, SPEC = 2;
    constexpr bool NEE = false, LIST = false, REG = true;
#include "pt_trace_v2_body.h"
}

// The leaf-sweep kernel (pt_leaf_sweep.h, body: pt_trace_sweep_body.h): trace_kernel_v2_reg<2, false, false, MINW>'s launches on
// scenes of at most 64 primitives in at most kSweepMaxBoxes groups of equal leaf boxes (leaf_sweep_on) find their leaves by
// testing every group's box when a segment starts instead of walking the tree.  Same leaves tested, same closest hit, same
// frame.  A third text rather than a flag of the body above: what that body compiles to for every other instantiation stays
// as it is.  The sweep's tables (pt_sweep_layout.h) come behind the arguments every trace kernel takes (SweepKernelArgs, for
// offsetof) as a pointer, the group count, the pitch of the box tables and the pairs per class of the sweep loop
// (pt_sweep_pairs.h), and are staged into the node region of the tree kernel's LdsPlan.
// PT_SWEEP_LEAF_STEPS: leaf tests per iteration between two scheduler checks; PT_SWEEP_THRESH: lanes that must be able to make
// progress for a scheduler phase to run (-D: A/B libraries).  A phase carries the whole sweep whatever its width, so it pays to
// wait for a fuller one than the tree kernel's 40: cbox 640x480x64 at 1.669 / 1.649 / 1.693 ms per frame with 40 / 48 / 56, and
// 1.706 / 1.669 / 1.698 / 1.679 with 3 / 4 / 5 / 6 leaf steps at 40 (profiles/r12_sweep_layout.log §7).  Measured again with the
// skip word (pt_sweep_skip.h: about three tests per segment): 1.425 at 4 / 48 against 1.462 at 3 / 48, 1.500 at 3 / 40 and
// 1.435 at 4 / 40 (profiles/r18_self_skip.log §5).
#ifndef PT_SWEEP_LEAF_STEPS
#define PT_SWEEP_LEAF_STEPS 4
#endif
#ifndef PT_SWEEP_THRESH
#define PT_SWEEP_THRESH 48
#endif
struct SweepLayoutDev {
    const unsigned char* tab;       // box tables in class order (build_sweep_pair_tables), then slot records (build_sweep_layout), global memory
    uint32_t groups;                // 1 .. kSweepMaxBoxes
    uint32_t box_pitch;             // sweep_classes_pitch of the two below
    SweepPairClasses classes;       // pairs per class of the sweep loop (pt_sweep_pairs.h), scalars
    SweepFamilyClasses fam;         // records per PAIR2 class in front of them (pt_sweep_families.h), read from the kernel arguments inside the phase
    const unsigned char* skip;      // the skip table in the order of `tab` (pt_sweep_skip.h), or one of zeros: kSweepSkipTableBytes of global memory
};
struct SweepKernelArgs {
    SceneDev scn; RenderDev rp; LdsPlan lp; float4* samples; uint32_t* work_counter; unsigned long long* counters; SweepLayoutDev sweep;
};
static_assert(offsetof(SweepKernelArgs, rp) == offsetof(TraceKernelArgs, rp), "reload_render_args reads rp at TraceKernelArgs' offset");
static_assert(offsetof(SweepLayoutDev, fam) + 16 <= sizeof(SweepLayoutDev), "step (3) reads the three PAIR2 count words as one load of four: the fourth must lie inside the argument");

// make_scene_view<2> for the sweep kernel: the node region of the plan takes the box tables as they are and the slot records
// with their edges made here (sweep_stage_record); prims, normals, materials and emission are staged where every kernel has
// them, shading reads them by primitive id.  sv.nodes names the region but nothing walks it.  Called by every thread of the block.
__device__ __forceinline__ ptd::SceneView make_sweep_view(const SceneDev& scn, const LdsPlan& lp, const SweepLayoutDev& sweep,
                                                          unsigned char* smem) {
    const uint32_t slots_off = sweep_slots_off(sweep.groups);
    stage_to_lds(smem + lp.nodes_off, sweep.tab, slots_off);
    const DPrim* gslots = reinterpret_cast<const DPrim*>(sweep.tab + slots_off);
    DPrim* lslots = reinterpret_cast<DPrim*>(smem + lp.nodes_off + slots_off);
    for (uint32_t i = threadIdx.x; i < (uint32_t)scn.num_prims; i += blockDim.x) {
        const float4 a = ptd::ld4(gslots + i, 0), b = ptd::ld4(gslots + i, 1), c = ptd::ld4(gslots + i, 2);
        DPrim g;
        g.v[0] = a.x; g.v[1] = a.y; g.v[2] = a.z; g.v[3] = a.w; g.v[4] = b.x; g.v[5] = b.y; g.v[6] = b.z; g.v[7] = b.w; g.v[8] = c.x;
        g.info = __builtin_bit_cast(int32_t, c.y); g.light = __builtin_bit_cast(int32_t, c.z); g.pad = __builtin_bit_cast(int32_t, c.w);
        const DPrim r = sweep_stage_record(g);
        float4* d = reinterpret_cast<float4*>(lslots + i);
        d[0] = make_float4(r.v[0], r.v[1], r.v[2], r.v[3]);
        d[1] = make_float4(r.v[4], r.v[5], r.v[6], r.v[7]);
        d[2] = make_float4(r.v[8], c.y, c.z, c.w);
    }
    // the skip entries behind the slot records, still inside the node region (pt_sweep_skip.h: sweep_skip_fits)
    stage_to_lds(smem + lp.nodes_off + sweep_skip_off(sweep.groups, (uint32_t)scn.num_prims), sweep.skip, sweep_skip_bytes((uint32_t)scn.num_prims));
    stage_to_lds(smem + lp.prims_off, scn.prims, (uint32_t)scn.num_prims * sizeof(DPrim));
    stage_to_lds(smem + lp.normals_off, scn.normals, (uint32_t)scn.num_prims * sizeof(DNormals));
    stage_to_lds(smem + lp.mats_off, scn.materials, (uint32_t)scn.num_materials * sizeof(DMaterial));
    stage_to_lds(smem + lp.emis_off, scn.emission, (uint32_t)scn.num_emission * sizeof(DEmission));
    __syncthreads();
    ptd::SceneView sv;
    sv.top_nodes = nullptr;
    sv.top_count = 0;
    sv.nodes = reinterpret_cast<const DNode*>(smem + lp.nodes_off);
    sv.prims = reinterpret_cast<const DPrim*>(smem + lp.prims_off);
    sv.normals = reinterpret_cast<const DNormals*>(smem + lp.normals_off);
    sv.materials = reinterpret_cast<const DMaterial*>(smem + lp.mats_off);
    sv.emission = reinterpret_cast<const DEmission*>(smem + lp.emis_off);
    sv.node_stride = kLdsNodeStride;
    sv.oct_stride = sweep.box_pitch;
    sv.lights = scn.lights;
    sv.num_emission = scn.num_emission;
    sv.root_ref = scn.root_ref;
    sv.fixed_order = scn.fixed_order;
    sv.ref_nodes = scn.ref_nodes; sv.ref_path = scn.ref_path; sv.ref_anc = scn.ref_anc; sv.ref_levels = scn.ref_levels;
    sv.bg = ptm::mk(scn.bg[0], scn.bg[1], scn.bg[2]);
    return sv;
}

// The sweep's record stream (step (3) of pt_trace_sweep_body.h).  An octant's table is ONE run of records in class order, so at
// every point "the next 32 bytes at bx" are the first four 8-byte pairs of whichever record comes next, of whatever class:
// PAIR2's whole record, a sharing pair's first four pairs of five, a general pair's first four of six, the single's three and
// one more.  Those four pairs are the WINDOW: eight registers, one instance of them live across all class loops.  A body
//   - forms all its differences out of the window (and out of its tail, below) into other registers,
//   - then reads the 32 bytes behind its own record into the window,
//   - then does its multiplies, minima and maxima, compares and the hit word,
// so the next record's LDS round trip runs under this record's arithmetic, across a loop's exit as well as inside it, and the
// wait in front of a turn's first v_sub_f32 is for reads the body before it issued.  The TAIL of a record is what the window
// does not hold (a sharing pair's 5th pair, a general pair's 5th and 6th): the body reads it itself at entry, in front of the
// window's differences, and takes its differences last.  An empty class is skipped and the window stays what it is: the bytes
// at bx.  The body that runs last reads 32 bytes it does not use: sweep_stream_end (pt_sweep_families.h) bounds them.
// The scheduling barriers pin that order (left to itself the compiler computes in place and reads at the top of a turn);
// they add no instruction.  No float operation differs from the loops without a window: v_sub_f32 then v_mul_f32 on the same
// operands, minima and maxima in the same axis order.
typedef float SweepF2 __attribute__((ext_vector_type(2)));
typedef const __attribute__((address_space(3))) SweepF2* SweepLdsF2;
struct SweepWindow { SweepF2 p0, p1, p2, p3; };
// reads the window `pairs` 8-byte pairs behind bx and returns that pointer; the empty statement keeps the add behind the reads
// (in front of them it takes a copy of the pointer)
__device__ __forceinline__ SweepLdsF2 sweep_window_read(SweepWindow& w, SweepLdsF2 bx, int pairs) {
    __builtin_amdgcn_sched_barrier(0);
    w.p0 = bx[pairs]; w.p1 = bx[pairs + 1]; w.p2 = bx[pairs + 2]; w.p3 = bx[pairs + 3];
    __builtin_amdgcn_sched_barrier(0);
    asm volatile("" : "+v"(bx));
    return bx + pairs;
}
template <int A> __device__ __forceinline__ float sweep_axis(const ptm::V3& v) { return A == 0 ? v.x : A == 1 ? v.y : v.z; }

// The two compares of a pair of boxes and the hit word's two adds with carry (pt_trace_sweep_body.h has the account of the s_nop).
__device__ __forceinline__ void sweep_shift_in_two(uint32_t& h, float tfa, float tna, float tfb, float tnb) {
    unsigned long long mb;
    asm("v_cmp_ge_f32_e32 vcc, %2, %3\n\t"
        "v_cmp_ge_f32_e64 %1, %4, %5\n\t"
        "s_nop 0\n\t"
        "v_addc_co_u32_e32 %0, vcc, %0, %0, vcc\n\t"
        "v_addc_co_u32_e64 %0, vcc, %0, %0, %1"
        : "+v"(h), "=&s"(mb) : "v"(tfa), "v"(tna), "v"(tfb), "v"(tnb) : "vcc");
}

// The sweep loop over `count` pairs that share axis AX (pt_sweep_pairs.h: SHARE_a, or SHARE_FLAT_a with FLAT), the window `w`
// holding the first four pairs of the record at `bx`; shifts two hit bits per pair into h and returns the pointer behind the
// class, the window read there.  The box test is visit_node<false, true>'s — tn = max(max(x, y), z) over the near products,
// tf = min(min(x, y), z) over the far ones, hit where tf >= max(0, tn) — with the shared axis's products, the same v_sub_f32
// and v_mul_f32 on the same operands, formed once for both boxes (FLAT: one product is near and far).
template <int AX, bool FLAT>
__device__ __forceinline__ SweepLdsF2 sweep_shared_pairs(SweepLdsF2 bx, SweepWindow& w, uint32_t count, const ptm::V3& o, const ptm::V3& inv, uint32_t& h) {
    constexpr int B = AX == 0 ? 1 : 0, C = AX == 2 ? 1 : 2;
    const float oa = sweep_axis<AX>(o), ia = sweep_axis<AX>(inv), ob = sweep_axis<B>(o), ib = sweep_axis<B>(inv), oc = sweep_axis<C>(o), ic = sweep_axis<C>(inv);
#pragma clang loop vectorize(disable) interleave(disable) unroll(disable)
    for (uint32_t k = count; k != 0; k--) {
        const SweepF2 bf = bx[4];                                   // the tail: B's far planes
        __builtin_amdgcn_sched_barrier(0);
        const float d_sn = w.p0.x - oa, d_sf = FLAT ? 0.0f : w.p0.y - oa;
        const float d_anb = w.p1.x - ob, d_anc = w.p1.y - oc, d_afb = w.p2.x - ob, d_afc = w.p2.y - oc;
        const float d_bnb = w.p3.x - ob, d_bnc = w.p3.y - oc;
        const float d_bfb = bf.x - ob, d_bfc = bf.y - oc;
        bx = sweep_window_read(w, bx, 5);
        float na[3], fa[3], nb[3], fb[3];
        na[AX] = d_sn * ia;
        fa[AX] = FLAT ? na[AX] : d_sf * ia;
        nb[AX] = na[AX]; fb[AX] = fa[AX];
        na[B] = d_anb * ib; na[C] = d_anc * ic; fa[B] = d_afb * ib; fa[C] = d_afc * ic;
        nb[B] = d_bnb * ib; nb[C] = d_bnc * ic; fb[B] = d_bfb * ib; fb[C] = d_bfc * ic;
        const float tfa = ptm::fmin2(ptm::fmin2(fa[0], fa[1]), fa[2]), tna = ptm::fmax2(0.0f, ptm::fmax2(ptm::fmax2(na[0], na[1]), na[2]));
        const float tfb = ptm::fmin2(ptm::fmin2(fb[0], fb[1]), fb[2]), tnb = ptm::fmax2(0.0f, ptm::fmax2(ptm::fmax2(nb[0], nb[1]), nb[2]));
        sweep_shift_in_two(h, tfa, tna, tfb, tnb);
    }
    return bx;
}

// The sweep loop over `count` PAIR2 records (pt_sweep_families.h): two boxes with the same interval on both axes other than U,
// FB / FC: the lower / upper of those is flat.  Each shared axis's products once for both boxes, a flat one's once in all; the
// same v_sub_f32 and v_mul_f32 on the same operands as the general pair, minima and maxima in its axis order.  The record is
// the window, no tail.
template <int U, bool FB, bool FC>
__device__ __forceinline__ SweepLdsF2 sweep_pair2(SweepLdsF2 bx, SweepWindow& w, uint32_t count, const ptm::V3& o, const ptm::V3& inv, uint32_t& h) {
    constexpr int B = U == 0 ? 1 : 0, C = U == 2 ? 1 : 2;
    const float ou = sweep_axis<U>(o), iu = sweep_axis<U>(inv), ob = sweep_axis<B>(o), ib = sweep_axis<B>(inv), oc = sweep_axis<C>(o), ic = sweep_axis<C>(inv);
#pragma clang loop vectorize(disable) interleave(disable) unroll(disable)
    for (uint32_t k = count; k != 0; k--) {
        const float d_nb = w.p0.x - ob, d_fb = FB ? 0.0f : w.p0.y - ob;
        const float d_nc = w.p1.x - oc, d_fc = FC ? 0.0f : w.p1.y - oc;
        const float d_anu = w.p2.x - ou, d_afu = w.p2.y - ou, d_bnu = w.p3.x - ou, d_bfu = w.p3.y - ou;
        bx = sweep_window_read(w, bx, 4);
        float na[3], fa[3], nb[3], fb[3];
        na[B] = d_nb * ib;
        fa[B] = FB ? na[B] : d_fb * ib;
        na[C] = d_nc * ic;
        fa[C] = FC ? na[C] : d_fc * ic;
        nb[B] = na[B]; fb[B] = fa[B]; nb[C] = na[C]; fb[C] = fa[C];
        na[U] = d_anu * iu; fa[U] = d_afu * iu;
        nb[U] = d_bnu * iu; fb[U] = d_bfu * iu;
        const float tfa = ptm::fmin2(ptm::fmin2(fa[0], fa[1]), fa[2]), tna = ptm::fmax2(0.0f, ptm::fmax2(ptm::fmax2(na[0], na[1]), na[2]));
        const float tfb = ptm::fmin2(ptm::fmin2(fb[0], fb[1]), fb[2]), tnb = ptm::fmax2(0.0f, ptm::fmax2(ptm::fmax2(nb[0], nb[1]), nb[2]));
        sweep_shift_in_two(h, tfa, tna, tfb, tnb);
    }
    return bx;
}

template <int MINW>
__global__ __launch_bounds__(kBlock, (kBlock > 256 ? 1 : MINW)) void trace_kernel_v2_sweep(SceneDev scn, RenderDev rp, LdsPlan lp,
                                                                float4* __restrict__ samples,
                                                                uint32_t* __restrict__ work_counter,
                                                                unsigned long long* __restrict__ counters,
                                                                SweepLayoutDev sweep) {
    constexpr int N_LEAF = PT_SWEEP_LEAF_STEPS;
#include "pt_trace_sweep_body.h"
}

// mode 0: fb = (prev + sum) * scale   (prev = accum if !first)        [final pass of pt_render]
// mode 1: accum = prev + sum          (prev = accum if !first else 0) [intermediate pass]
// mode 2: accum = first ? sum : accum + sum, sum started from zero    [render_progressive, main.cu:72-86]
__global__ __launch_bounds__(256) void resolve_kernel(const float4* __restrict__ samples, float* __restrict__ accum,
                                                      float* __restrict__ fb, uint32_t npix, int spp_pass,
                                                      int mode, int first, float scale) {
    const uint32_t pix = blockIdx.x * blockDim.x + threadIdx.x;
    if (pix >= npix) return;
    ptm::V3 sum = ptm::mk(0, 0, 0);
    if (mode != 2 && !first) sum = ptm::mk(accum[3 * (size_t)pix], accum[3 * (size_t)pix + 1], accum[3 * (size_t)pix + 2]);
    for (int s = 0; s < spp_pass; s++) {
        const float4 v = samples[(size_t)s * npix + pix];
        sum = sum + ptm::mk(v.x, v.y, v.z);                 // main.cu:47 color += radiance(...)
    }
    if (mode == 0) {
        sum = sum * scale;                                  // main.cu:50 color / float(spp) == color * (1/spp)
        fb[3 * (size_t)pix] = sum.x; fb[3 * (size_t)pix + 1] = sum.y; fb[3 * (size_t)pix + 2] = sum.z;
    } else if (mode == 1) {
        accum[3 * (size_t)pix] = sum.x; accum[3 * (size_t)pix + 1] = sum.y; accum[3 * (size_t)pix + 2] = sum.z;
    } else {
        if (!first) {
            sum = ptm::mk(accum[3 * (size_t)pix], accum[3 * (size_t)pix + 1], accum[3 * (size_t)pix + 2]) + sum;
        }
        accum[3 * (size_t)pix] = sum.x; accum[3 * (size_t)pix + 1] = sum.y; accum[3 * (size_t)pix + 2] = sum.z;
    }
}

// pt_render_adaptive: one thread per entry of the round's pixel list (round 0: no list, entry = packed pixel id).  Continues the
// pixel's fp32 sum (the order of resolve_kernel: ((0 + s0) + s1) + ...) and its fp64 moments S1 = sum Y, S2 = sum Y^2 over the
// pass's samples [spp_pass][n], sample by sample.  On the last pass of a round (check) it applies the stopping rule at
// n_total samples (pt_api.h): a pixel that stops gets fb = sum * (1/n), spp_map and err_map; the others are appended to
// list_out, one atomic per wave.  The list order may differ from run to run; no output depends on it.
struct AdaptiveArgs {
    const uint32_t* list_in;        // nullptr = round 0 (entry t is pixel t)
    uint32_t n;                     // entries of this round
    int spp_pass;                   // samples of this pass
    int first;                      // first pass of the first round: sums start from zero
    int check;                      // last pass of a round: apply the rule at n_total
    int n_total;                    // samples of every listed pixel after this round
    int max_spp;
    double z;                       // Phi^-1(1 - p/2)
    double max_error, min_luminance;
    float* sum;                     // [npix][3]
    double* mom;                    // [npix][2]
    uint32_t* list_out;
    uint32_t* count_out;
    float* fb;                      // [npix][3]
    int32_t* spp_map;               // [npix] or nullptr
    float* err_map;                 // [npix] or nullptr
};

__global__ __launch_bounds__(256) void adaptive_resolve_kernel(const float4* __restrict__ samples, AdaptiveArgs a) {
    const uint32_t t = blockIdx.x * blockDim.x + threadIdx.x;
    const bool in = t < a.n;
    bool more = false;
    uint32_t pix = 0;
    if (in) {
        pix = a.list_in ? a.list_in[t] : t;
        ptm::V3 sum = ptm::mk(0, 0, 0);
        double s1 = 0.0, s2 = 0.0;
        if (!a.first) {
            sum = ptm::mk(a.sum[3 * (size_t)pix], a.sum[3 * (size_t)pix + 1], a.sum[3 * (size_t)pix + 2]);
            s1 = a.mom[2 * (size_t)pix]; s2 = a.mom[2 * (size_t)pix + 1];
        }
        for (int s = 0; s < a.spp_pass; s++) {
            const float4 v = samples[(size_t)s * a.n + t];
            sum = sum + ptm::mk(v.x, v.y, v.z);
            const double y = 0.2126 * (double)v.x + 0.7152 * (double)v.y + 0.0722 * (double)v.z;   // no contraction (-ffp-contract=off)
            s1 = s1 + y;
            s2 = s2 + y * y;
        }
        bool stop = false;
        double err = 0.0;
        if (a.check) {
            const double n = (double)a.n_total;
            double var = __builtin_inf();
            if (a.n_total > 1) {
                const double v = (s2 - s1 * s1 / n) / (n - 1.0);
                var = v < 0.0 ? 0.0 : v;                    // NaN stays NaN
            }
            const double half = a.z * sqrt(var / n);
            const double mean = s1 / n;
            const double den = mean < a.min_luminance ? a.min_luminance : mean;
            err = half == 0.0 ? 0.0 : half / den;
            stop = err <= a.max_error || a.n_total >= a.max_spp;
        }
        if (stop) {
            sum = sum * (1.0f / (float)a.n_total);          // resolve_kernel / the oracle: sum * (1/spp), correctly rounded
            a.fb[3 * (size_t)pix] = sum.x; a.fb[3 * (size_t)pix + 1] = sum.y; a.fb[3 * (size_t)pix + 2] = sum.z;
            if (a.spp_map) a.spp_map[pix] = a.n_total;
            if (a.err_map) a.err_map[pix] = (float)err;
        } else {
            a.sum[3 * (size_t)pix] = sum.x; a.sum[3 * (size_t)pix + 1] = sum.y; a.sum[3 * (size_t)pix + 2] = sum.z;
            a.mom[2 * (size_t)pix] = s1; a.mom[2 * (size_t)pix + 1] = s2;
            more = a.check != 0;
        }
    }
    const unsigned long long mask = __ballot(more);
    if (mask == 0ull) return;
    const int lane = threadIdx.x & 63;
    uint32_t base = 0;
    if (lane == 0) base = atomicAdd(a.count_out, (uint32_t)__popcll(mask));
    base = __shfl(base, 0, 64);
    if (more) a.list_out[base + lane_rank(mask)] = pix;
}

template <bool PRUNE>
__global__ __launch_bounds__(kBlock) void intersect_kernel(SceneDev scn, const float* __restrict__ rays, int n,
                                                           float* __restrict__ out_tuv, int32_t* __restrict__ out_prim,
                                                           int32_t* __restrict__ reruns) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    ptd::SceneView sv;
    sv.nodes = scn.nodes; sv.prims = scn.prims; sv.normals = scn.normals;
    sv.materials = scn.materials; sv.emission = scn.emission; sv.lights = scn.lights;
    sv.top_nodes = nullptr; sv.top_count = 0;
    sv.node_stride = sizeof(DNode);
    sv.num_emission = scn.num_emission; sv.root_ref = scn.root_ref; sv.fixed_order = scn.fixed_order;
    sv.ref_nodes = scn.ref_nodes; sv.ref_path = scn.ref_path; sv.ref_anc = scn.ref_anc; sv.ref_levels = scn.ref_levels;
    sv.bg = ptm::mk(0, 0, 0);
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int cap = scn.fallback && scn.redo_cap > scn.stack_cap ? scn.redo_cap : scn.stack_cap;   // one column serves both trees
    int32_t* stk = reinterpret_cast<int32_t*>(smem) + (size_t)wave * cap * 64 + lane;
    const int k = blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= n) return;
    ptd::Ray r;
    r.org = ptm::mk(rays[8 * k], rays[8 * k + 1], rays[8 * k + 2]);
    r.dir = ptm::mk(rays[8 * k + 3], rays[8 * k + 4], rays[8 * k + 5]);
    r.tnear = rays[8 * k + 6];
    r.tfar = rays[8 * k + 7];
    ptd::TravStats st;
    ptd::Hit h;
    if (scn.fallback) {                                   // internal tree; the caller's for rays with a zero direction component
        ptd::SceneView sv_ref = sv;
        sv_ref.nodes = scn.ref_nodes; sv_ref.root_ref = scn.ref_root_ref; sv_ref.fixed_order = 0;
        bool rerun;
        h = ptd::intersect_any_tree<PRUNE>(sv, sv_ref, r, stk, rerun);
        if (rerun) atomicAdd(reruns, 1);
    } else {
        h = ptd::intersect<PRUNE, false>(sv, r, stk, st);
    }
    out_prim[k] = h.prim;
    out_tuv[3 * k] = h.prim < 0 ? 0.0f : h.t;
    out_tuv[3 * k + 1] = h.prim < 0 ? 0.0f : h.u;
    out_tuv[3 * k + 2] = h.prim < 0 ? 0.0f : h.v;
}

// pt_render_aov: guide buffers of the first hit, one lane per selected pixel.  The ray goes through the pixel CENTRE and is
// traced like a camera segment of a render (primary_ray, tnear 0, tfar +inf) with intersect_kernel's traversal: the internal
// tree with ties settled in the caller's visit order where there is one, else the caller's; stack columns in LDS.
// rp carries the camera, width / height and the row selection only.  Any output may be null.
//   prim    shape id, -1 on a miss                 depth   t, 0 on a miss
//   normal  make_surface's shading normal turned towards the camera as shade_and_bounce turns it; 0 on a miss
//   albedo  the material's reflectance, (1,1,1) for a mirror; 0 on a miss and where a render adds emission at this hit
//
// MOTION (pt_render_guides): from the same hit, where the surface point was in the previous frame — (prim, u, v) names the same
// point of a triangle in the previous primitive records, a sphere carries its point along by its centre and radius — projected
// into the previous camera (pt_temporal.h: project_previous).  mo.prev_prims = the current records or the ones that were live
// before the last geometry update.  motion = (0, 0) and prev_depth = 0 on a miss and wherever the rule calls the pixel invalid.
struct MotionDev {
    ptt::PrevCam cam;
    const DPrim* prev_prims;
    float* motion;                  // [rows, W, 2] or null
    float* prev_depth;              // [rows, W] or null
};

// What pixel k's guide buffers get from the closest hit `h` of its pixel-centre ray `r` (the rule above), written once for
// aov_kernel and for the lane-refilling query kernel (pt_query.h): make_surface, the emission / albedo / normal rule, and with
// MOTION the surface point followed into the previous records and projected into the previous camera.
template <bool MOTION>
__device__ __forceinline__ void write_guides(const ptd::SceneView& sv, const RenderDev& rp, const ptd::Ray& r, const ptd::Hit& h,
                                             const uint32_t k, float* __restrict__ albedo, float* __restrict__ normal,
                                             float* __restrict__ depth, int32_t* __restrict__ prim, const MotionDev& mo) {
    ptm::V3 n = ptm::mk(0.0f, 0.0f, 0.0f), a = n;
    float t = 0.0f;
    if (h.prim >= 0) {
        const ptd::Surface sf = ptd::make_surface<false>(sv, r, h);
        t = h.t;
        n = sf.n;
        const float wi_n = ptm::dot(-r.dir, n);
        bool emits = false;                              // shade_and_bounce's emission test (radiance.cuh:35-43)
        if (sf.light >= 0 && sf.light < sv.num_emission) {
            const float4 e = ptd::ld4(sv.emission + sf.light, 0);
            emits = __builtin_bit_cast(int32_t, e.w) != 0 && wi_n > 0.0f;
        }
        if (wi_n < 0.0f) n = -n;
        if (!emits) {
            const float4 m0 = ptd::ld4(sv.materials + sf.material, 0);
            a = __builtin_bit_cast(int32_t, m0.x) == 1 ? ptm::mk(1.0f, 1.0f, 1.0f) : ptm::mk(m0.y, m0.z, m0.w);
        }
    }
    if (prim) prim[k] = h.prim < 0 ? -1 : h.prim;
    if (depth) depth[k] = t;
    if (normal) { normal[3 * (size_t)k] = n.x; normal[3 * (size_t)k + 1] = n.y; normal[3 * (size_t)k + 2] = n.z; }
    if (albedo) { albedo[3 * (size_t)k] = a.x; albedo[3 * (size_t)k + 1] = a.y; albedo[3 * (size_t)k + 2] = a.z; }
    if (MOTION) {
        float mx = 0.0f, my = 0.0f, pz = 0.0f;
        if (h.prim >= 0) {
            const float4 c0 = ptd::ld4(sv.prims + h.prim, 0), c2 = ptd::ld4(sv.prims + h.prim, 2);
            const float4 q0 = ptd::ld4(mo.prev_prims + h.prim, 0), q1 = ptd::ld4(mo.prev_prims + h.prim, 1),
                         q2 = ptd::ld4(mo.prev_prims + h.prim, 2);
            const bool sphere = __builtin_bit_cast(int32_t, c2.y) < 0, sphere_prev = __builtin_bit_cast(int32_t, q2.y) < 0;
            if (sphere == sphere_prev) {
                ptm::V3 Q;
                if (sphere) {
                    const ptm::V3 P = r.org + r.dir * h.t;
                    Q = ptm::mk(q0.x, q0.y, q0.z) + (P - ptm::mk(c0.x, c0.y, c0.z)) * (q0.w / c0.w);
                } else {
                    const float w = (1.0f - h.u) - h.v;
                    Q = (ptm::mk(q0.x, q0.y, q0.z) * w + ptm::mk(q0.w, q1.x, q1.y) * h.u) + ptm::mk(q1.z, q1.w, q2.x) * h.v;
                }
                (void)ptt::project_previous(Q, mo.cam, rp.width, rp.height, mx, my, pz);
            }
        }
        if (mo.motion) { mo.motion[2 * (size_t)k] = mx; mo.motion[2 * (size_t)k + 1] = my; }
        if (mo.prev_depth) mo.prev_depth[k] = pz;
    }
}

template <bool PRUNE, bool MOTION = false>
__global__ __launch_bounds__(kBlock) void aov_kernel(SceneDev scn, RenderDev rp, float* __restrict__ albedo,
                                                     float* __restrict__ normal, float* __restrict__ depth,
                                                     int32_t* __restrict__ prim, MotionDev mo = MotionDev{}) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    ptd::SceneView sv;
    sv.nodes = scn.nodes; sv.prims = scn.prims; sv.normals = scn.normals;
    sv.materials = scn.materials; sv.emission = scn.emission; sv.lights = scn.lights;
    sv.top_nodes = nullptr; sv.top_count = 0;
    sv.node_stride = sizeof(DNode);
    sv.num_emission = scn.num_emission; sv.root_ref = scn.root_ref; sv.fixed_order = scn.fixed_order;
    sv.ref_nodes = scn.ref_nodes; sv.ref_path = scn.ref_path; sv.ref_anc = scn.ref_anc; sv.ref_levels = scn.ref_levels;
    sv.bg = ptm::mk(0, 0, 0);
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int cap = scn.fallback && scn.redo_cap > scn.stack_cap ? scn.redo_cap : scn.stack_cap;   // one column serves both trees
    int32_t* stk = reinterpret_cast<int32_t*>(smem) + (size_t)wave * cap * 64 + lane;
    const uint32_t k = blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= rp.npix) return;
    const uint32_t row = fastdiv(k, rp.div_width);
    const int i = (int)(k - row * (uint32_t)rp.width);
    const int j = rp.row_begin + (int)row * rp.row_step;
    const float u = ((float)i + 0.5f) / (float)rp.width;
    const float v = ((float)j + 0.5f) / (float)rp.height;
    const ptd::Ray r = ptd::primary_ray(rp, u, v);
    ptd::TravStats st;
    ptd::Hit h;
    if (scn.fallback) {
        ptd::SceneView sv_ref = sv;
        sv_ref.nodes = scn.ref_nodes; sv_ref.root_ref = scn.ref_root_ref; sv_ref.fixed_order = 0;
        bool rerun;
        h = ptd::intersect_any_tree<PRUNE>(sv, sv_ref, r, stk, rerun);
    } else {
        h = ptd::intersect<PRUNE, false>(sv, r, stk, st);
    }
    write_guides<MOTION>(sv, rp, r, h, k, albedo, normal, depth, prim, mo);
}

// Inner-node visits of a fixed set of probe rays through the tree `scn` points at (pt_scene_life.hip: validate_and_build chooses
// between the caller's tree and the internal one by this count).  Ray k starts on primitive hash(k) mod N — its centroid,
// or the point of a sphere facing the direction — and leaves into a uniform direction: the shape of a segment after a bounce.
// Both trees in one launch: blockIdx.y picks the tree and its counter (two launches of 128 blocks each ran one after the other
// on half a chip).
__global__ __launch_bounds__(kBlock) void probe_kernel(SceneDev scn0, SceneDev scn1, unsigned long long* __restrict__ visits2) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    const SceneDev& scn = blockIdx.y ? scn1 : scn0;
    unsigned long long* visits = visits2 + blockIdx.y;
    ptd::SceneView sv;
    sv.nodes = scn.nodes; sv.prims = scn.prims; sv.normals = scn.normals;
    sv.materials = scn.materials; sv.emission = scn.emission; sv.lights = scn.lights;
    sv.top_nodes = nullptr; sv.top_count = 0;
    sv.node_stride = sizeof(DNode);
    sv.num_emission = scn.num_emission; sv.root_ref = scn.root_ref; sv.fixed_order = scn.fixed_order;
    sv.ref_nodes = scn.ref_nodes; sv.ref_path = scn.ref_path; sv.ref_anc = scn.ref_anc; sv.ref_levels = scn.ref_levels;
    sv.bg = ptm::mk(0, 0, 0);
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    int32_t* stk = reinterpret_cast<int32_t*>(smem) + (size_t)wave * scn.stack_cap * 64 + lane;
    const uint32_t k = blockIdx.x * blockDim.x + threadIdx.x;
    ptm::Pcg rng = ptm::pcg_init(k, 0x9e3779b9u);
    const uint32_t prim = (uint32_t)(((unsigned long long)ptm::pcg_next(rng) * (unsigned long long)scn.num_prims) >> 32);
    const float z = 1.0f - 2.0f * ptm::pcg_float(rng);
    const float phi = 6.2831853f * ptm::pcg_float(rng);
    const float rr = __builtin_sqrtf(__builtin_fmaxf(0.0f, 1.0f - z * z));
    ptd::Ray r;
    float sn, cs;
    ptm::sincos_det(phi, sn, cs);                        // own sin / cos: the same probe rays, hence the same choice of tree, on every ROCm build
    r.dir = ptm::mk(rr * cs, rr * sn, z);
    const DPrim* pr = scn.prims + prim;
    const float4 a = ptd::ld4(pr, 0), b = ptd::ld4(pr, 1), c = ptd::ld4(pr, 2);
    if (__builtin_bit_cast(int32_t, c.y) < 0) {          // sphere: center + radius * dir
        r.org = ptm::mk(a.x + a.w * r.dir.x, a.y + a.w * r.dir.y, a.z + a.w * r.dir.z);
    } else {
        r.org = ptm::mk((a.x + a.w + b.z) * (1.0f / 3.0f), (a.y + b.x + b.w) * (1.0f / 3.0f), (a.z + b.y + c.x) * (1.0f / 3.0f));
    }
    r.tnear = 1e-4f;
    r.tfar = FLT_MAX;
    ptd::TravStats st;
    st.nodes = 0; st.leaves = 0;
    (void)ptd::intersect<false, true>(sv, r, stk, st);
    const unsigned long long sum = wave_sum((unsigned long long)st.nodes);
    if (lane == 0) atomicAdd(visits, sum);
}

__global__ void math_kernel(int op, const float* __restrict__ x, const float* __restrict__ y,
                            float* __restrict__ o0, float* __restrict__ o1, int n) {
    const int k = blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= n) return;
    if (op == 0) {
        float s, c;
        ptm::sincos_det(x[k], s, c);
        o0[k] = s; o1[k] = c;
    } else if (op == 1) {
        o0[k] = ptm::pow_det(x[k], y[k]);
    } else {
        // PCG: stream = bits of x[k], seed = bits of y[k]; out0 = 1st float draw, out1 = 2nd
        ptm::Pcg r = ptm::pcg_init((uint64_t)__builtin_bit_cast(uint32_t, x[k]), (uint64_t)__builtin_bit_cast(uint32_t, y[k]));
        o0[k] = ptm::pcg_float(r);
        o1[k] = ptm::pcg_float(r);
    }
}

// pt_debug_exact_math: a fast sequence of pt_math.h against the IEEE expression it stands for, on the fp32 bit patterns
// begin .. begin + count - 1 (grid-stride).  op 0: rcp_exact(x) vs 1.0f / x, 1: div_pi_exact(x) vs x / kPi,
// 2: sqrt_exact(x) vs sqrtf(x), 3: the bare v_rcp_f32 vs 1.0f / x (a control: it must differ somewhere).
// Counts the inputs whose result bits differ; *first = smallest such offset from begin.
__global__ void exact_math_kernel(int op, uint32_t begin, uint64_t count, unsigned long long* __restrict__ bad,
                                  uint32_t* __restrict__ first) {
    const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
    unsigned long long nbad = 0;
    uint32_t fb = 0xffffffffu;
    for (uint64_t k = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; k < count; k += stride) {
        const float x = __builtin_bit_cast(float, begin + (uint32_t)k);
        float got, want;
        if (op == 0) { got = ptm::rcp_exact(x); want = 1.0f / x; }
        else if (op == 1) { got = ptm::div_pi_exact(x); want = x / ptm::kPi; }
        else if (op == 2) { got = ptm::sqrt_exact(x); want = __builtin_sqrtf(x); }
        else { got = __builtin_amdgcn_rcpf(x); want = 1.0f / x; }
        if (__builtin_bit_cast(uint32_t, got) != __builtin_bit_cast(uint32_t, want)) {
            nbad++;
            fb = min(fb, (uint32_t)k);
        }
    }
    if (nbad) {
        atomicAdd(bad, nbad);
        atomicMin(first, fb);
    }
}


}  // namespace ptk
