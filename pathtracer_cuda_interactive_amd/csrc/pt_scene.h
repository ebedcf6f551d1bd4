// pt_scene.h — the scene handle, and what pt_scene_life.hip (its lifecycle: create, update, transform, rebuild, destroy) and
// pt_api.hip (everything a live handle is used for, and the kernels) share.  Not part of the C ABI.
// pt_kernels.h, pt_kernel_q.h and pt_query.h define non-template kernels, so exactly one unit may include them: pt_api.hip.
// What this header needs of their constants it restates (ptkc below); pt_api.hip, which sees both, asserts that they agree.
#pragma once
#include <hip/hip_runtime.h>

#include <algorithm>
#include <chrono>
#include <cstdint>
#include <string>
#include <utility>
#include <vector>

#include "../../include/pt_api.h"
#include "pt_internal.h"
#include "pt_layout.h"
#include "pt_leaf_sweep.h"
#include "pt_sweep_families.h"
#include "pt_sweep_skip.h"
#include "pt_sweep_pairs.h"
#include "pt_scene_refit.h"

#define HIP_TRY(expr)                                                                              \
    do {                                                                                           \
        hipError_t e_ = (expr);                                                                    \
        if (e_ != hipSuccess)                                                                      \
            return pt_fail(e_ == hipErrorNoDevice ? PT_ERR_NO_DEVICE : PT_ERR_DEVICE,              \
                           std::string(#expr) + ": " + hipGetErrorString(e_));                     \
    } while (0)

// An entry point makes the scene's device current under a DeviceGuard named `guard` (below), or returns the status of the attempt.
#define ENTER_DEVICE(S) DeviceGuard guard; if (int grc_ = guard.enter((S)->device)) return grc_

namespace ptkc {   // pt_kernels.h / pt_query.h restated (see above)
constexpr int kBlock = 256, kCounterStride = 32, kQueryRing = 64, kLdsNodeStride = 64;
}

using namespace ptl;   // the device layouts, as both units read them

template <class T>
struct DevBuf {
    T* p = nullptr;
    size_t n = 0;
    DevBuf() = default;
    DevBuf(const DevBuf&) = delete;
    DevBuf& operator=(const DevBuf&) = delete;
    // moves trade contents, so that std::swap of a DevBuf — or of a struct of them — moves pointer and count together
    DevBuf(DevBuf&& o) noexcept { swap(o); }
    DevBuf& operator=(DevBuf&& o) noexcept { swap(o); return *this; }
    ~DevBuf() { release(); }          // the owner makes the buffer's device current first (pt_scene_destroy)
    int ensure(size_t count) {
        if (count <= n && p) return PT_OK;
        if (p) { (void)hipFree(p); p = nullptr; n = 0; }
        HIP_TRY(hipMalloc(reinterpret_cast<void**>(&p), std::max<size_t>(count, 1) * sizeof(T)));
        n = count;
        return PT_OK;
    }
    void release() { if (p) (void)hipFree(p); p = nullptr; n = 0; }
    void swap(DevBuf& o) { std::swap(p, o.p); std::swap(n, o.n); }
};

// Makes the scene's device current for the duration of a call and restores the caller's device afterwards.
struct DeviceGuard {
    int prev = -1;
    bool switched = false;
    int enter(int device) {
        if (hipGetDevice(&prev) != hipSuccess) prev = -1;
        if (prev != device) {
            HIP_TRY(hipSetDevice(device));
            switched = true;
        }
        return PT_OK;
    }
    ~DeviceGuard() { if (switched && prev >= 0) (void)hipSetDevice(prev); }
};

// Wall time of a call's stages: lap() is the microseconds since the last lap (or the start), total() those since the start.
struct StageClock {
    using clk = std::chrono::steady_clock;
    const clk::time_point t0 = clk::now();
    clk::time_point t_lap = t0;
    static int64_t us(clk::time_point from, clk::time_point to) { return (int64_t)std::chrono::duration_cast<std::chrono::microseconds>(to - from).count(); }
    int64_t lap() { const clk::time_point from = t_lap; t_lap = clk::now(); return us(from, t_lap); }
    int64_t total() const { return us(t0, clk::now()); }
    void rewind() { t_lap = t0; }     // the lap under way counts from the start
};

constexpr uint32_t kLdsSceneLimit = 36 * 1024;   // scenes up to this size (64-B nodes) are staged whole into LDS
constexpr int kMaxFramesInFlight = 4;            // frame slots a handle may hold (option frames_in_flight)
#ifndef PT_FRAMES_IN_FLIGHT
#define PT_FRAMES_IN_FLIGHT 2
#endif
constexpr int kDefaultFramesInFlight = PT_FRAMES_IN_FLIGHT;
constexpr size_t kWorkBytes = 8 * ptkc::kCounterStride * sizeof(uint32_t);   // 8 band counters, one 128-B line each
constexpr size_t kWorkWords = kWorkBytes / sizeof(unsigned long long);

struct pt_scene {
    int device = 0;
    int num_cus = 0;
    size_t lds_per_block_max = 0;
    // scene arrays.  Two layouts of the hierarchy: tree[0] = the caller's tree (the reference's, bvh.cu:16-54), tree[1] = the
    // library's internal tree over the SAME leaf boxes, made at create time (validate_and_build: the full-sweep surface-area
    // tree of pt_tree_sweep.h / pt_sweep_build.hip, or the caller's own topology in internal form).  Exact traversal runs on
    // tree[1] and falls back to tree[0] for the rays whose result depends on the visit order (see launch_render).
    // A Tree is moved and swapped whole (std::swap: buffers and metadata together, whatever members it has).
    struct Tree {
        DevBuf<DNode> nodes;
        DevBuf<DNode> nodes_oct;     // [8][num_nodes] octant-specialised copies (small scenes only)
        bool have_oct = false;
        int32_t num_nodes = 0, root_ref = 0, stack_cap = 0;
        uint32_t top_avail = 0;      // nodes [0, top_avail) are the top of the tree in breadth-first order (0 = plain pre-order)
        int depth = 0;
    } tree[2];
    bool have_fast = false;
    DevBuf<unsigned long long> ref_path;   // per primitive: its root-to-leaf turns in the caller's tree (ties on t, pt_trace.h: ref_visits_first)
    DevBuf<int32_t> ref_anc;         // per primitive and level: the inner node of the caller's tree there
    int32_t ref_levels = 0;
    bool fast_is_callers_topology = false;   // tree[1] = the caller's own tree in internal form (the sweep tree did not win)
    DevBuf<DPrim> prims;
    DevBuf<DNormals> normals;
    DevBuf<DMaterial> materials;
    DevBuf<DEmission> emission;
    DevBuf<DLight> lights;
    SceneDev dev{};
    uint32_t scene_bytes = 0;
    // pt_scene_update: new primitive records and leaf boxes are made and checked in staging memory before the handle changes
    // (the record buffers then trade places with prims / normals); one refit plan per tree, made on the first geometry update
    DevBuf<DPrim> st_prims;
    DevBuf<DNormals> st_normals;
    // pt_render_guides: the primitive records that were live before the last successful geometry update.  Allocated on the
    // first geometry update; the three record buffers then rotate (staging -> current -> previous -> staging), so that an
    // update that fails in staging destroys neither set and none is ever copied.
    DevBuf<DPrim> prev_prims;
    bool have_prev = false;
    DevBuf<float> st_boxes;
    DevBuf<unsigned int> st_status;
    ptf::Plan refit_plan[2];
    int64_t updates = 0, update_us[4] = {0, 0, 0, 0};   // [0] total [1] records + uploads [2] refit + octant tables [3] plan build
    // pt_scene_transform: the group of every shape and the table of group entries (pt_transform.h); the REST records, a copy of
    // prims / normals made on the first transform after pt_scene_create or a geometry update, which every transform starts from
    DevBuf<int32_t> group_of;
    DevBuf<float> group_tab;
    int32_t num_groups = 0;
    bool have_groups = false;
    DevBuf<DPrim> rest_prims;
    DevBuf<DNormals> rest_normals;
    bool have_rest = false;
    int64_t transforms = 0, transform_us[4] = {0, 0, 0, 0};   // [0] total [1] records [2] refit [3] snapshot + plan build
    // pt_scene_rebuild: calls that succeeded, those among them a policy made (option rebuild_at_permille), whether the last one
    // adopted its tree and that tree's probe ratio; wall time: [0] total [1] leaf boxes + build [2] re-layout + probe
    // [3] plan + sweep tables.  no_fast_why: why pt_scene_create kept no internal tree (the refusal's message).
    int64_t rebuilds = 0, rebuilds_auto = 0, rebuild_adopted = 0, rebuild_cost_permille = 0, rebuild_us[4] = {0, 0, 0, 0};
    const char* no_fast_why = "";
    // tree-cost telemetry (pt_tree_cost.hip; options tree_cost, rebuild_at_permille): per tree the cost of the boxes as built
    // (taken before the first refit that follows) and after the last refit.  cost_dev / cost_host: [0..1] reference, [2..3]
    // current, device results and their pinned host copies; the copies are enqueued behind the refit and read once the call
    // has synchronised (cost_pending_*).
    int64_t opt_tree_cost = 0, opt_rebuild_at = 0;
    DevBuf<double> cost_partials, cost_dev;
    double* cost_host = nullptr;
    double cost_ref[2] = {0.0, 0.0}, cost_now[2] = {0.0, 0.0};
    bool cost_have_ref[2] = {false, false}, cost_pending_ref[2] = {false, false}, cost_pending_now[2] = {false, false};
    bool cost_on() const { return opt_tree_cost != 0 || opt_rebuild_at != 0; }
    // The telemetry starts afresh whenever it is switched on: what was measured before it went off belongs to boxes, perhaps to
    // a tree, that refits and rebuilds without it have since replaced.
    void cost_forget() {
        for (int t = 0; t < 2; t++) {
            cost_ref[t] = cost_now[t] = 0.0;
            cost_have_ref[t] = false;
        }
        cost_drop_pending();
    }
    // A refused refit leaves the handle as it was: what it had enqueued is not collected by a later call.
    void cost_drop_pending() {
        for (int t = 0; t < 2; t++) cost_pending_ref[t] = cost_pending_now[t] = false;
    }
    bool tri_only = false;           // the scene holds no sphere
    bool diffuse_only = false;       // every material is DIFFUSE
    // scratch
    DevBuf<float> accum;
    DevBuf<float> fb_tmp;
    // pt_render_adaptive: per packed pixel the running fp32 sum and fp64 moments, the two ping-pong lists of pixels still
    // sampled, the next list's length, and host-output staging for spp_map / err_map
    DevBuf<float> ad_sum;
    DevBuf<double> ad_mom;
    DevBuf<uint32_t> ad_list[2];
    DevBuf<uint32_t> ad_count;
    DevBuf<int32_t> ad_spp_tmp;
    DevBuf<float> ad_err_tmp;
    int64_t info_adaptive_rounds = 0;
    // pt_denoise: the guide record and the two ping-pong colour records per pixel (pt_denoise.h), and staging of a frame that
    // comes in host memory (run_staged: the planes of the call; the result goes back through the colour plane)
    DevBuf<float4> dn_guide, dn_x[2];
    DevBuf<float> dn_host;
    DevBuf<float> tp_host;           // pt_temporal_accumulate(_moments): staging of a call that comes in host memory
    // pt_denoise_variance: records of its own (a call may be in flight on another stream than pt_denoise's) and staging of a
    // call that comes in host memory
    DevBuf<float4> vd_guide, vd_x[2];
    DevBuf<float> vd_host;
    // pt_temporal_gradient: the two ping-pong tile records (pt_gradient.h, two float4 per tile), allocated on first use and
    // grown when a larger frame arrives, and staging of a call that comes in host memory
    DevBuf<float4> gr_x[2];
    DevBuf<float> gr_host;
    // pt_render_pixels: staging of a list that comes in host memory (the colours go back through fb_tmp)
    DevBuf<int32_t> px_list;
    // pt_trace_rays / pt_render_guides_async (pt_query.h): every launch of the query kernel takes the next work counter of a ring
    // (a 128-B line each), cleared on the launch's stream; the entry's event is recorded behind the launch, and a launch that
    // finds the event of its entry still pending makes its stream wait for it — two launches in flight never share a counter.
    // Staging of a pt_trace_rays call that comes in host memory: grown on demand, freed with the handle.
    DevBuf<uint32_t> q_counters;
    hipEvent_t q_event[ptkc::kQueryRing] = {};
    uint64_t q_seq = 0;                                   // query launches so far
    DevBuf<float> q_rays, q_tuv;
    DevBuf<int32_t> q_prim;
    int64_t opt_query_blocks = 0;                         // 0 = automatic grid, else exactly this many blocks
    int64_t opt_query_refill = 0;                         // 0 = automatic, else idle lanes from which a wave refills (1 .. 64)
    int64_t opt_query_guides = 0;                         // pt_render_guides_async: 0 = automatic, 1 = the refilling kernel, 2 = aov_kernel
    int64_t info_query_guides = 0;                        // the last pt_render_guides_async ran on the refilling kernel (1) or on aov_kernel (0)
    int64_t info_query_grid = 0;                          // blocks of the last query launch
    const void* q_cfg_fn = nullptr;                       // occupancy of the last query kernel variant used (as cfg_fn below)
    uint32_t q_cfg_lds = 0;
    int q_cfg_occ = 0;
    void drop_query() {
        q_counters.release(); q_rays.release(); q_tuv.release(); q_prim.release();
        for (auto& e : q_event) { if (e) (void)hipEventDestroy(e); e = nullptr; }
    }
    // What a frame's trace kernel writes lives in a frame slot; render call k uses slot k % frames_in_flight.  With more than one
    // slot a single-pass frame runs on the slot's own stream: the trace kernel at once (it reads the immutable scene and writes
    // the slot only), the resolve — the one step that touches the caller's buffer — once the caller's stream has reached the
    // point of the call (in_ev), and the caller's stream continues behind the resolve (free_ev).  The next frame's trace kernel
    // then fills the CUs while this one's last paths drain (the tail of a persistent launch is a partly empty chip), and
    // everything the caller can observe stays in the order of the caller's stream.  Both waits across streams sit beside the
    // chain trace k -> resolve k -> trace k + slots, which is in order on ONE stream (an event wait across streams costs tens of
    // microseconds on this runtime; with the resolve on the caller's stream, two of them per frame sat on that chain and
    // two slots rendered slower than one).  A slot is reused once the resolve that read its samples has finished (free_ev).
    struct FrameSlot {
        DevBuf<float4> samples;
        // control block: [0, kWorkBytes) the band work counters, then the statistics (kNumCounters uint64, pt_kernels.h)
        DevBuf<unsigned long long> ctl;
        DevBuf<int32_t> redo_stack;  // global-memory traversal stacks of the reference-order reruns (one column per lane of the grid)
        hipStream_t stream = nullptr;
        hipEvent_t free_ev = nullptr, in_ev = nullptr;
        hipStream_t free_stream = nullptr;   // the stream free_ev was last recorded on
        bool used = false;
    } slot[kMaxFramesInFlight];
    int cur_slot = 0;                // the slot of the last render call
    int64_t opt_frames_in_flight = kDefaultFramesInFlight;
    FrameSlot& cur() { return slot[cur_slot]; }
    const FrameSlot& cur() const { return slot[cur_slot]; }
    uint32_t* work_counter() const { return reinterpret_cast<uint32_t*>(cur().ctl.p); }
    unsigned long long* counters() const { return cur().ctl.p ? cur().ctl.p + kWorkWords : nullptr; }
    void drop_slots() {
        for (auto& f : slot) {
            f.samples.release(); f.ctl.release(); f.redo_stack.release();
            if (f.stream) (void)hipStreamDestroy(f.stream);
            if (f.free_ev) (void)hipEventDestroy(f.free_ev);
            if (f.in_ev) (void)hipEventDestroy(f.in_ev);
            f.stream = nullptr; f.free_ev = nullptr; f.in_ev = nullptr; f.used = false;
        }
    }
    hipStream_t last_stream = nullptr;
    bool have_timing = false;
    // options
    int64_t opt_blocks_per_cu = 0;
    int64_t opt_scratch_bytes = 0;
    int64_t opt_force_global = 0;
    int64_t opt_stats = 0;
    int64_t opt_specialize = 1;      // compile-time specialisation on scene content (no spheres -> sphere code removed)
    int64_t opt_octants = 1;         // use the 8 ray-octant node tables when the scene is small enough
    int64_t opt_top_cache = 1;       // scenes in global memory: keep the top of the tree in LDS
    int64_t opt_fast_tree = 1;       // exact traversal on the library's internal tree where one was kept (0 = on the caller's tree)
    int64_t opt_chunk = 0;           // work items a wave reserves per atomic (0 = automatic)
    int64_t opt_lds_budget_kb = 0;   // scenes in global memory: LDS per block for traversal stacks + top-of-tree cache (0 = 26 KB: 6 blocks per CU)
    int64_t opt_item_order = 1;      // work item order inside a band: 1 = row-major (all samples of a row, then the next row), 0 = sample-major
    int64_t opt_xcd_regions = 0;     // 0 = 8 row bands (one per XCD); 1 = a single work queue
    int64_t opt_kernel = 2;          // 2 = decoupled traversal/shading (default), 1 = segment-synchronous wavefront kernel,
                                     // 3 = paths regrouped across the waves of a workgroup (pt_kernel_q.h; LDS-resident scenes, else as 2)
    int64_t opt_q_target = 0, opt_q_swap = 0, opt_q_low = 0;   // schedule knobs of kernel 3; 0 = automatic
    int64_t opt_v2_thresh = 0, opt_v2_inner = 0, opt_v2_minw = 0;   // 0 = auto (see v2_schedule)
    int64_t opt_reg_stack = 1;      // 1 = register traversal stack where it applies (choose_trace), 0 = always the LDS stack
    int64_t opt_leaf_sweep = 1;     // 1 = leaves found by the box sweep where it applies (choose_trace), 0 = always the tree
    int64_t opt_sweep_pairs = 1;    // 1 = the sweep's groups paired by shared axis intervals (pt_sweep_pairs.h), 0 = table order, every pair general
    int64_t opt_sweep_families = 1; // under sweep_pairs 1: 1 = PAIR2 records in front of the pairs (pt_sweep_families.h), 0 = the pairs alone
    // the groups of equal leaf boxes of tree[1] (pt_leaf_sweep.h), made at scene creation where the tree was built on the host
    // and the scene has at most 64 primitives.  sweep_groups = 0: none (also after a geometry update: boxes that were equal need
    // not be any more); it may exceed what a launch admits, sweep.count then stays 0.
    SweepTable sweep{};
    int sweep_groups = 0;
    // what a sweep launch stages in place of the octant node tables (pt_sweep_layout.h: box tables, then slot records), made
    // and uploaded with sweep.count, dropped with it
    DevBuf<unsigned char> sweep_tab;
    // the same of the groups in class order, which option "sweep_pairs" 1 launches (sweep_tab is option 0's), one per value of
    // option "sweep_families": [0] the pair classes alone (pt_sweep_pairs.h), [1] PAIR2 records in front (pt_sweep_families.h)
    DevBuf<unsigned char> sweep_tab_pairs[2];
    SweepClasses sweep_classes[2] = {};
    // the classes a sweep launch runs under the options as they stand, and their table; all zero / null: no tables
    SweepClasses sweep_classes_now() const {
        if (!sweep.count) return SweepClasses{};
        return opt_sweep_pairs && sweep_tab_pairs[opt_sweep_families].p ? sweep_classes[opt_sweep_families] : sweep_classes_of_pairs(sweep_pairs_none(sweep.count));
    }
    const unsigned char* sweep_tab_now() const { return opt_sweep_pairs && sweep_tab_pairs[opt_sweep_families].p ? sweep_tab_pairs[opt_sweep_families].p : sweep_tab.p; }
    // the skip tables (pt_sweep_skip.h), made, uploaded and dropped with the tables above: kSweepSkipTableBytes each, [0] all
    // zero (option "sweep_self_skip" 0), [1] in sweep_tab's group order, [2] and [3] in sweep_tab_pairs[0]'s and [1]'s
    DevBuf<unsigned char> sweep_skip;
    SweepSkipInfo sweep_skip_info[3] = {};
    int64_t opt_sweep_self_skip = 1; // 1 = a bounce skips the leaf tests of the plane it starts on, 0 = every group the sweep hits is tested
    int sweep_skip_index() const { return !opt_sweep_self_skip ? 0 : opt_sweep_pairs && sweep_tab_pairs[opt_sweep_families].p ? 2 + (int)opt_sweep_families : 1; }
    const unsigned char* sweep_skip_now() const { return sweep_skip.p ? sweep_skip.p + (size_t)sweep_skip_index() * kSweepSkipTableBytes : nullptr; }
    SweepSkipInfo sweep_skip_info_now() const { return sweep.count && sweep_skip.p && sweep_skip_index() ? sweep_skip_info[sweep_skip_index() - 1] : SweepSkipInfo{0, 0}; }
    // info of last launch
    // wall time of pt_scene_create's stages, microseconds: [0] total [1] primitive records [2] caller's tree checked and re-laid
    // [3] internal tree built [4] ... re-laid [5] uploads + probe [6] tie tables; built_on_device: the sweep ran on the GPU
    int64_t create_us[7] = {0, 0, 0, 0, 0, 0, 0}, sweep_on_device = 0;
    int64_t info_grid = 0, info_lds_bytes = 0, info_lds_scene = 0, info_passes = 0, info_occupancy = 0, info_blocks_per_cu = 0, info_debug_reruns = 0, fast_cost_permille = 0, info_kernel = 0, info_trace_variant = 0, info_path_bank = 0, info_reg_stack = 0, info_leaf_sweep = 0;
    struct PassEvents { hipEvent_t t0, t1, r0, r1; };            // trace begin, trace end (on the trace kernel's stream); resolve begin, end (caller's)
    // HIP events of the last `opt_timing_frames` render calls (a ring; default 1): a caller that enqueues frame after frame
    // without a host sync in between — bench.py's timed loop — reads every frame's kernel time afterwards (pt_get_frame_times)
    struct FrameRec { std::vector<PassEvents> ev; size_t passes = 0; };
    std::vector<FrameRec> frames;
    uint64_t frame_seq = 0;                                      // render calls so far; the last one sits in frames[(frame_seq - 1) % size]
    int64_t opt_timing_frames = 1;
    const FrameRec* last_frame() const { return frame_seq && !frames.empty() ? &frames[(frame_seq - 1) % frames.size()] : nullptr; }
    void drop_events() {
        for (auto& f : frames)
            for (auto& pe : f.ev) { (void)hipEventDestroy(pe.t0); (void)hipEventDestroy(pe.t1); (void)hipEventDestroy(pe.r0); (void)hipEventDestroy(pe.r1); }
        frames.clear();
        frame_seq = 0;
    }
    // launch configuration of the last kernel variant used (occupancy query and attribute call are not free per frame)
    const void* cfg_fn = nullptr;
    uint32_t cfg_lds = 0;
    int cfg_occ = 0;
    // What is not a DevBuf: events and streams, the refit plans, the pinned cost copies; the owner has made the handle's device current
    // and quiet (pt_scene_destroy).  The scene arrays go first, in pt_scene_destroy's old order (kept: a create that follows was slower behind another; why is not known).
    ~pt_scene() {
        drop_query();
        for (auto& T : tree) { T.nodes.release(); T.nodes_oct.release(); }
        drop_slots(); drop_events();
        prims.release(); normals.release(); materials.release(); emission.release(); lights.release();
        for (auto& pl : refit_plan) ptf::plan_release(&pl);
        if (cost_host) (void)hipHostFree(cost_host);
    }
};

// Points a kernel argument block (select_tree: the handle's own) at one of the two trees; fallback: exact traversal on the internal tree — ties settled in the
// caller's visit order, rays with a zero direction component traced on tree[0].
// (T: the tree itself — S->tree[which], or pt_scene_rebuild's candidate for tree[1])
inline void tree_view(const pt_scene* S, SceneDev& dv, const pt_scene::Tree& T, int which, bool fallback) {
    dv.nodes = T.nodes.p;
    dv.nodes_oct = T.have_oct ? T.nodes_oct.p : nullptr;
    dv.num_nodes = T.num_nodes;
    dv.root_ref = T.root_ref;
    dv.stack_cap = T.stack_cap;
    dv.fallback = fallback ? 1 : 0;
    dv.ref_nodes = S->tree[0].nodes.p;
    dv.ref_root_ref = S->tree[0].root_ref;
    dv.redo_cap = S->tree[0].stack_cap;
    dv.redo_stack = S->cur().redo_stack.p;
    dv.fixed_order = which == 1 ? 1 : 0;
    dv.ref_path = S->ref_path.p;
    dv.ref_anc = S->ref_anc.p;
    dv.ref_levels = S->ref_levels;
}
inline void tree_view(const pt_scene* S, SceneDev& dv, int which, bool fallback) { tree_view(S, dv, S->tree[which], which, fallback); }
inline void select_tree(pt_scene* S, int which, bool fallback = false) { tree_view(S, S->dev, which, fallback); }

// Tree t's cost after the last refit over its cost as built (or as last rebuilt), x 1000 (pt_scene_life.hip: tree-cost telemetry).
inline int64_t cost_permille(const pt_scene* S, int t) {
    if (!S->cost_have_ref[t] || !(S->cost_ref[t] > 0.0) || !(S->cost_now[t] > 0.0)) return 1000;
    return (int64_t)(1000.0 * S->cost_now[t] / S->cost_ref[t] + 0.5);
}

// Inner visits of the probe rays (pt_kernels.h: probe_kernel) through the trees d0 and d1 point at, into v[0] and v[1].
// (Defined in pt_api.hip, beside the kernel.)
int probe_trees(const SceneDev& d0, const SceneDev& d1, unsigned long long v[2]);
// Every one of n floats in device memory finite?  (Defined in pt_api.hip with its kernel, which stays in that unit's code object.)
bool boxes_finite_device(const float* v_dev, size_t n);
