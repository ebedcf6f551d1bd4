// pt_api.hip — kernels and C ABI of libpt_hip.so (gfx950 only).  See include/pt_api.h.
//
// Host half of the library: scene validation and re-layout, scratch management, kernel selection and launch,
// the extern "C" entry points.  The kernels live in pt_kernels.h, the device functions in pt_trace.h / pt_math.h.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <initializer_list>
#include <iterator>
#include <limits>
#include <mutex>
#include <queue>
#include <string>
#include <type_traits>
#include <utility>
#include <vector>

#include "../../include/pt_api.h"
#include "pt_internal.h"
#include "pt_tree_sweep.h"
#include "pt_sweep_build.h"
#include "pt_scene_prep.h"
#include "pt_scene_refit.h"
#include "pt_tree_cost.h"
#include "pt_scene_transform.h"
#include "pt_transform.h"
#include "pt_denoise.h"
#include "pt_gradient.h"
#include "pt_temporal.h"
#include "pt_kernels.h"
#include "pt_kernel_q.h"
#include "pt_query.h"

using namespace ptl;
using namespace ptk;

// ------------------------------------------------------------------------------------------
// host side
// ------------------------------------------------------------------------------------------
namespace {

thread_local std::string g_err;

int fail(int code, const std::string& msg) {
    g_err = msg;
    return code;
}

}  // namespace

int pt_fail(int code, const std::string& msg) { return fail(code, msg); }

namespace {

#define HIP_TRY(expr)                                                                              \
    do {                                                                                           \
        hipError_t e_ = (expr);                                                                    \
        if (e_ != hipSuccess)                                                                      \
            return fail(e_ == hipErrorNoDevice ? PT_ERR_NO_DEVICE : PT_ERR_DEVICE,                 \
                        std::string(#expr) + ": " + hipGetErrorString(e_));                        \
    } while (0)

template <class T>
struct DevBuf {
    T* p = nullptr;
    size_t n = 0;
    DevBuf() = default;
    DevBuf(const DevBuf&) = delete;
    DevBuf& operator=(const DevBuf&) = delete;
    ~DevBuf() { release(); }          // the owner makes the buffer's device current first (pt_scene_destroy)
    int ensure(size_t count) {
        if (count <= n && p) return PT_OK;
        if (p) { (void)hipFree(p); p = nullptr; n = 0; }
        HIP_TRY(hipMalloc(reinterpret_cast<void**>(&p), std::max<size_t>(count, 1) * sizeof(T)));
        n = count;
        return PT_OK;
    }
    void release() { if (p) (void)hipFree(p); p = nullptr; n = 0; }
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

constexpr uint32_t kLdsSceneLimit = 36 * 1024;   // scenes up to this size (64-B nodes) are staged whole into LDS
constexpr uint32_t kOctNodeLimit = 24 * 1024;    // 8 octant copies of the node table must fit in this many bytes of LDS
constexpr int kMaxStack = 64;                    // the reference's own cap (scene.h:251)
constexpr int kMinInternalTree = 16;              // primitives below which no internal tree is built (a handful of nodes either way: scene1, 4 shapes, is 6 % slower with one)
constexpr int kDeviceSweepMin = 4096;             // primitives from which the internal tree is built on the device (below: a few ms on the host either way)
constexpr int kProbeRays = 32768;                // validate_and_build: rays that choose between the caller's tree and the internal one
constexpr uint64_t kDefaultScratchBytes = 8ull << 30;   // per-sample scratch cap (3 % of the 288 GB of HBM): every sample pass
                                                        // pays the launch floor once (buddha stand-in 135.6 ms in 5 passes, 130.6 in 1)
#ifndef PT_TOP_NODES
#define PT_TOP_NODES 512
#endif
constexpr uint32_t kTopNodes = PT_TOP_NODES;              // scenes read from global memory: this many nodes are numbered breadth-first
                                                 // from the root, so that [0, k) is the top of the tree for every k (LDS cache)
#ifndef PT_TOP_LDS_KB
#define PT_TOP_LDS_KB 26
#endif
constexpr uint32_t kTopLdsBudget = PT_TOP_LDS_KB * 1024;    // LDS per block that keeps 6 blocks per CU resident (160 KB / 6)
constexpr uint32_t kMaxLdsBudget = 160 * 1024;               // the breadth-first numbered prefix is sized for the largest budget an option may ask for
constexpr int kMaxFramesInFlight = 4;            // frame slots a handle may hold (option frames_in_flight)
#ifndef PT_FRAMES_IN_FLIGHT
#define PT_FRAMES_IN_FLIGHT 2
#endif
constexpr int kDefaultFramesInFlight = PT_FRAMES_IN_FLIGHT;
constexpr size_t kWorkBytes = 8 * kCounterStride * sizeof(uint32_t);   // 8 band counters, one 128-B line each
constexpr size_t kWorkWords = kWorkBytes / sizeof(unsigned long long);

uint32_t align16(uint32_t v) { return (v + 15u) & ~15u; }

// every float finite?  (leaf boxes that stayed on the device)
__global__ void finite_kernel(const float* __restrict__ v, size_t n, unsigned int* __restrict__ bad) {
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n && !__builtin_isfinite(v[i])) atomicAdd(bad, 1u);
}
bool boxes_finite_device(const float* v_dev, size_t n) {
    unsigned int* bad = nullptr;
    if (hipMalloc(reinterpret_cast<void**>(&bad), sizeof(unsigned int)) != hipSuccess) return false;
    unsigned int h = 1;
    if (hipMemset(bad, 0, sizeof(unsigned int)) == hipSuccess) {
        hipLaunchKernelGGL(finite_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, nullptr, v_dev, n, bad);
        if (hipMemcpy(&h, bad, sizeof h, hipMemcpyDeviceToHost) != hipSuccess) h = 1;
    }
    (void)hipFree(bad);
    return h == 0;
}

// PT_SWEEP_BUILD=host in the environment keeps the internal tree's build on the host (A/B timing, debugging)
bool host_sweep_forced() {
    const char* v = std::getenv("PT_SWEEP_BUILD");
    return v && std::string(v) == "host";
}

}  // namespace

struct pt_scene {
    int device = 0;
    int num_cus = 0;
    size_t lds_per_block_max = 0;
    // scene arrays.  Two layouts of the hierarchy: tree[0] = the caller's tree (the reference's, bvh.cu:16-54), tree[1] = the
    // library's internal tree over the SAME leaf boxes, made at create time (validate_and_build: the full-sweep surface-area
    // tree of pt_tree_sweep.h / pt_sweep_build.hip, or the caller's own topology in internal form).  Exact traversal runs on
    // tree[1] and falls back to tree[0] for the rays whose result depends on the visit order (see launch_render).
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
    hipEvent_t q_event[ptq::kQueryRing] = {};
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
    // the groups of equal leaf boxes of tree[1] (pt_leaf_sweep.h), made at scene creation where the tree was built on the host
    // and the scene has at most 64 primitives.  sweep_groups = 0: none (also after a geometry update: boxes that were equal need
    // not be any more); it may exceed what a launch admits, sweep.count then stays 0.
    SweepTable sweep{};
    int sweep_groups = 0;
    // what a sweep launch stages in place of the octant node tables (pt_sweep_layout.h: box tables, then slot records), made
    // and uploaded with sweep.count, dropped with it
    DevBuf<unsigned char> sweep_tab;
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
};

namespace {

// Points a kernel argument block (select_tree: the handle's own) at one of the two trees; fallback: exact traversal on the internal tree — ties settled in the
// caller's visit order, rays with a zero direction component traced on tree[0].
// (T: the tree itself — S->tree[which], or pt_scene_rebuild's candidate for tree[1])
void tree_view(const pt_scene* S, SceneDev& dv, const pt_scene::Tree& T, int which, bool fallback) {
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
void tree_view(const pt_scene* S, SceneDev& dv, int which, bool fallback) { tree_view(S, dv, S->tree[which], which, fallback); }
void select_tree(pt_scene* S, int which, bool fallback = false) { tree_view(S, S->dev, which, fallback); }

struct TreeHost {
    std::vector<DNode> nodes;
    int32_t root_ref = 0;
    int depth = 1;
    int stack_need = 1;            // stack entries a traversal can hold at once (without the sentinel)
    std::vector<int32_t> inner_of_pool;   // caller's node pool index -> index in `nodes` (-1: a leaf)
    uint32_t top_avail = 0;
};

// pt_bvh_node pool (one node per leaf and per inner node, bvh.cuh:7-15) -> inner-only DNodes carrying both child boxes.
// Validates the topology.  leaf_boxes (optional, [N][6]): receives every primitive's leaf box.  *nested: every node's box
// below the root contains its children's boxes.
int convert_tree(const pt_bvh_node* in, int num_nodes, int root, int N, TreeHost& out, float* leaf_boxes, bool* nested, bool internal = false) {
    std::vector<int32_t> inner_id(num_nodes, -1);
    std::vector<DNode>& nodes = out.nodes;
    nodes.clear();
    nodes.reserve(N > 1 ? N - 1 : 1);
    int depth = 1;
    std::vector<char> prim_seen(N, 0);
    auto leaf_ok = [&](const pt_bvh_node& nd) { return nd.prim >= 0 && nd.prim < N; };
    auto contains = [](const pt_bvh_node& outer, const pt_bvh_node& inner) {
        for (int k = 0; k < 3; k++)
            if (!(inner.bmin[k] >= outer.bmin[k] && inner.bmax[k] <= outer.bmax[k])) return false;
        return true;
    };
    const pt_bvh_node& rootn = in[root];
    if (rootn.prim != -1) {
        if (!leaf_ok(rootn)) return fail(PT_ERR_BAD_SCENE, "leaf primitive id out of range");
        out.root_ref = ~rootn.prim;
        prim_seen[rootn.prim] = 1;
        if (leaf_boxes) { std::memcpy(leaf_boxes + 6 * (size_t)rootn.prim, rootn.bmin, 12); std::memcpy(leaf_boxes + 6 * (size_t)rootn.prim + 3, rootn.bmax, 12); }
    } else {
        // The internal tree is traversed left child first (pt_trace.h: visit_node).  While the left subtree is being worked
        // on, the right child waits on the stack: entries needed = max(1 + need(left), need(right)), so the child that needs
        // less goes LEFT and the need of a node is the larger of its children's, plus one only when they are equal — the
        // Strahler number of the tree, at most log2(leaves) + 1 whatever its depth.
        std::vector<int32_t> need;
        if (internal) {                                               // (the library's own tree: no validation needed here)
            need.assign(num_nodes, 0);
            std::vector<int32_t> pre, open;
            open.push_back(root);
            while (!open.empty()) {
                const int32_t k = open.back();
                open.pop_back();
                pre.push_back(k);
                for (int32_t ch : {in[k].left, in[k].right})
                    if (in[ch].prim == -1) open.push_back(ch);
            }
            for (size_t k = pre.size(); k-- > 0;) {                  // parents come before their children in `pre`
                const pt_bvh_node& nd = in[pre[k]];
                const int32_t a = need[nd.left], b = need[nd.right];
                need[pre[k]] = a == b ? a + 1 : std::max(a, b);
            }
            out.stack_need = need[root];
        }
        auto swapped = [&](const pt_bvh_node& nd) { return internal && need[nd.left] > need[nd.right]; };
        // DFS pre-order: a parent and the subtree of the child it lists first are contiguous in memory
        struct Item { int32_t ref_node; int depth; };
        std::vector<Item> todo;
        todo.push_back({root, 1});
        size_t visited = 0;
        std::vector<int32_t> order;
        while (!todo.empty()) {
            Item it = todo.back();
            todo.pop_back();
            const pt_bvh_node& nd = in[it.ref_node];
            if (++visited > (size_t)num_nodes) return fail(PT_ERR_BAD_SCENE, "BVH is not a tree (cycle)");
            if (inner_id[it.ref_node] != -1) return fail(PT_ERR_BAD_SCENE, "BVH node referenced twice");
            if (nd.left < 0 || nd.left >= num_nodes || nd.right < 0 || nd.right >= num_nodes)
                return fail(PT_ERR_BAD_SCENE, "BVH child index out of range");
            inner_id[it.ref_node] = (int32_t)order.size();
            order.push_back(it.ref_node);
            if (it.depth + 1 > depth) depth = it.depth + 1;
            const pt_bvh_node& ln = in[nd.left];
            const pt_bvh_node& rn = in[nd.right];
            if (it.ref_node != root && nested && !(contains(nd, ln) && contains(nd, rn))) *nested = false;
            const bool sw = swapped(nd);
            const int32_t first = sw ? nd.right : nd.left, second = sw ? nd.left : nd.right;
            if (in[second].prim == -1) todo.push_back({second, it.depth + 1});
            if (in[first].prim == -1) todo.push_back({first, it.depth + 1});
        }
        // Scenes too big for LDS: renumber so that the first kTopNodes ids are the top of the tree in breadth-first order
        // (every ray starts there; the kernel keeps a prefix of them in LDS), the rest stays in pre-order.
        if ((size_t)N * (sizeof(DPrim) + sizeof(DNormals)) + order.size() * sizeof(DNode) > kLdsSceneLimit && order.size() > 1) {
            // only as many as fit next to the traversal stacks (make_plan)
            const uint32_t stack_bytes = (uint32_t)(kBlock / 64) * (uint32_t)((internal ? out.stack_need : std::max(depth - 1, 1)) + 1) * 64u * 4u;
            const size_t want = std::min<size_t>(kTopNodes, kMaxLdsBudget > stack_bytes ? (kMaxLdsBudget - stack_bytes) / sizeof(DNode) : 0);
            // which ones: without pruning a node is visited iff the ray hits its box, so the nodes most rays visit are the ones
            // with the largest boxes — take them in order of surface area (a child's box is never larger than its parent's,
            // so every prefix of this list is closed under "parent of"; the kernel stages a prefix)
            std::vector<int32_t> top;
            std::vector<char> in_top(num_nodes, 0);
            auto area = [&](int32_t k) {
                const pt_bvh_node& b = in[k];
                const double x = (double)b.bmax[0] - b.bmin[0], y = (double)b.bmax[1] - b.bmin[1], z = (double)b.bmax[2] - b.bmin[2];
                return 2.0 * (x * y + y * z + z * x);
            };
            typedef std::pair<double, int32_t> Cand;                  // (area, -position in pre-order): ties go to the earlier node
            std::priority_queue<Cand> open;
            if (want) open.push(Cand(std::numeric_limits<double>::infinity(), 0));
            while (!open.empty() && top.size() < want) {
                const int32_t k = order[(size_t)-open.top().second];
                open.pop();
                top.push_back(k);
                const pt_bvh_node& nd = in[k];
                for (int32_t ch : {nd.left, nd.right})
                    if (in[ch].prim == -1) open.push(Cand(area(ch), -inner_id[ch]));
            }
            for (int32_t r : top) in_top[r] = 1;
            std::vector<int32_t> renum(top);
            for (int32_t r : order)
                if (!in_top[r]) renum.push_back(r);
            order.swap(renum);
            for (size_t k = 0; k < order.size(); k++) inner_id[order[k]] = (int32_t)k;
            out.top_avail = (uint32_t)top.size();
        }
        nodes.resize(order.size());
        for (size_t k = 0; k < order.size(); k++) {
            const pt_bvh_node& nd = in[order[k]];
            const bool sw = swapped(nd);
            const int32_t li = sw ? nd.right : nd.left, ri = sw ? nd.left : nd.right;
            const pt_bvh_node& ln = in[li];
            const pt_bvh_node& rn = in[ri];
            DNode& o = nodes[k];
            std::memcpy(o.lmin, ln.bmin, 12); std::memcpy(o.lmax, ln.bmax, 12);
            std::memcpy(o.rmin, rn.bmin, 12); std::memcpy(o.rmax, rn.bmax, 12);
            for (const pt_bvh_node* ch : {&ln, &rn})
                if (ch->prim != -1) {
                    if (!leaf_ok(*ch)) return fail(PT_ERR_BAD_SCENE, "leaf primitive id out of range");
                    if (prim_seen[ch->prim]) return fail(PT_ERR_BAD_SCENE, "primitive referenced by two leaves");
                    prim_seen[ch->prim] = 1;
                    if (leaf_boxes) { std::memcpy(leaf_boxes + 6 * (size_t)ch->prim, ch->bmin, 12); std::memcpy(leaf_boxes + 6 * (size_t)ch->prim + 3, ch->bmax, 12); }
                }
            o.left = ln.prim != -1 ? ~ln.prim : inner_id[li];
            o.right = rn.prim != -1 ? ~rn.prim : inner_id[ri];
            o.pad0 = o.pad1 = 0;
        }
        out.root_ref = 0;
    }
    for (int i = 0; i < N; i++)
        if (!prim_seen[i]) return fail(PT_ERR_BAD_SCENE, "primitive not covered by any leaf");
    if (!internal && depth - 1 > kMaxStack - 1)
        return fail(PT_ERR_BAD_SCENE, "BVH deeper than the traversal stack (reference cap 64, scene.h:251)");
    out.depth = depth;
    out.inner_of_pool.swap(inner_id);
    if (!internal) out.stack_need = std::max(depth - 1, 1);           // nearer child first: a pending sibling per level
    if (nodes.empty()) nodes.resize(1);   // single-primitive scene: no inner nodes; keep a dummy so pointers are valid
    return PT_OK;
}

// ---- checks and conversions pt_scene_create and pt_scene_update share -------------------------------------------------------
int check_materials(const pt_scene_desc* d) {
    for (int m = 0; m < d->num_materials; m++)
        if (d->materials[m].type < PT_MAT_DIFFUSE || d->materials[m].type > PT_MAT_PHONG)
            return fail(PT_ERR_BAD_SCENE, "unknown material type (scene.h:410 asserts)");
    return PT_OK;
}
int check_meshes(const pt_scene_desc* d, int num_materials) {
    for (int m = 0; m < d->num_meshes; m++) {
        const pt_mesh& me = d->meshes[m];
        if (me.num_vertices <= 0 || me.num_faces <= 0 || !me.positions || !me.indices)
            return fail(PT_ERR_BAD_SCENE, "empty mesh");
        if (!me.normals) return fail(PT_ERR_BAD_SCENE, "mesh without vertex normals (required, SURVEY H5a)");
        if (me.material_id < 0 || me.material_id >= num_materials) return fail(PT_ERR_BAD_SCENE, "mesh material id out of range");
    }
    return PT_OK;
}
bool all_diffuse(const pt_scene_desc* d) {
    for (int m = 0; m < d->num_materials; m++)
        if (d->materials[m].type != PT_MAT_DIFFUSE) return false;
    return true;
}
// materials and lights as the kernels read them; N = number of shapes (an area light names its emitting shape)
int pack_shading(const pt_scene_desc* d, int N, std::vector<DMaterial>& mats, std::vector<DEmission>& emis, std::vector<DLight>& dlights) {
    mats.resize(d->num_materials);
    for (int m = 0; m < d->num_materials; m++) {
        const pt_material& src = d->materials[m];
        mats[m] = DMaterial{src.type, src.reflectance[0], src.reflectance[1], src.reflectance[2], src.eta, src.exponent, 0.0f, 0.0f};
    }
    emis.resize(std::max(d->num_lights, 1));
    std::memset(emis.data(), 0, sizeof(DEmission) * emis.size());
    for (int l = 0; l < d->num_lights; l++) {
        const pt_light& src = d->lights[l];
        emis[l] = DEmission{src.radiance[0], src.radiance[1], src.radiance[2], src.type == PT_LIGHT_DIFFUSE_AREA ? 1 : 0};
    }
    dlights.resize(std::max(d->num_lights, 1));
    std::memset(dlights.data(), 0, sizeof(DLight) * dlights.size());
    for (int l = 0; l < d->num_lights; l++) {
        const pt_light& src = d->lights[l];
        dlights[l] = DLight{src.radiance[0], src.radiance[1], src.radiance[2], src.type == PT_LIGHT_DIFFUSE_AREA ? 1 : 0,
                            src.position[0], src.position[1], src.position[2], src.shape_id};
        if (src.type == PT_LIGHT_DIFFUSE_AREA && (src.shape_id < 0 || src.shape_id >= N))
            return fail(PT_ERR_BAD_SCENE, "area light refers to a shape that does not exist");
    }
    return PT_OK;
}

// ---- the internal-tree stage: what pt_scene_create and pt_scene_rebuild both run ---------------------------------------------
// A tree the host made, into T's buffers with its metadata.
int upload_tree(pt_scene::Tree& T, const TreeHost& H) {
    const std::vector<DNode>& nodes = H.nodes;
    // 8 ray-octant copies of the node table for LDS-resident scenes: octant bit k set <=> 1/d[k] < 0, in which case
    // Hit() swaps the two slab distances of axis k (bbox.cuh:40-55); here the two planes are swapped instead.
    T.have_oct = false;
    if (nodes.size() * 8 * sizeof(DNode) <= kOctNodeLimit) {
        std::vector<DNode> nodes_oct(nodes.size() * 8);
        for (int o = 0; o < 8; o++)
            for (size_t k = 0; k < nodes.size(); k++) {
                DNode n = nodes[k];
                for (int ax = 0; ax < 3; ax++)
                    if (o & (1 << ax)) { std::swap(n.lmin[ax], n.lmax[ax]); std::swap(n.rmin[ax], n.rmax[ax]); }
                nodes_oct[(size_t)o * nodes.size() + k] = n;
            }
        int r;
        if ((r = T.nodes_oct.ensure(nodes_oct.size()))) return r;
        HIP_TRY(hipMemcpy(T.nodes_oct.p, nodes_oct.data(), nodes_oct.size() * sizeof(DNode), hipMemcpyHostToDevice));
        T.have_oct = true;
    }
    int r;
    if ((r = T.nodes.ensure(nodes.size()))) return r;
    HIP_TRY(hipMemcpy(T.nodes.p, nodes.data(), nodes.size() * sizeof(DNode), hipMemcpyHostToDevice));
    T.num_nodes = (int32_t)nodes.size();
    T.root_ref = H.root_ref;
    T.stack_cap = H.stack_need + 1;                         // + the kDone sentinel at the bottom
    T.top_avail = H.top_avail;
    T.depth = H.depth;
    return PT_OK;
}

// The sweep tree of N leaf boxes in device memory, built (pt_sweep_build.hip) and re-laid (pt_scene_prep.hip) there, into T.
// built(): called between the two (stage timing).  false: the builder handed the input back (depth guard) or something
// failed; T.nodes is released and the host builder is next.
template <class Built>
bool internal_tree_device(const float* boxes_dev, int N, pt_scene::Tree& T, Built built) {
    DevBuf<pt_bvh_node> fpool_dev;
    DevBuf<int32_t> fiop_dev;
    int32_t fdepth = 0;
    double dev_ms = 0;
    const size_t pool_nodes = 2 * (size_t)N - 1;
    const bool ok = !fpool_dev.ensure(pool_nodes) && !fiop_dev.ensure(pool_nodes) && !T.nodes.ensure((size_t)N - 1) &&
                    boxes_finite_device(boxes_dev, (size_t)N * 6) &&
                    pts::sweep_build_on_device(boxes_dev, N, fpool_dev.p, &fdepth, &dev_ms) == PT_OK;
    built();
    ptp::RelayResult r1;
    if (ok && ptp::relay_tree_device(fpool_dev.p, (int)pool_nodes, 0, N, true, T.nodes.p, fiop_dev.p, nullptr, kBlock, kTopNodes,
                                     kMaxLdsBudget, &r1) == PT_OK && r1.nested) {
        T.have_oct = false; T.num_nodes = N - 1; T.root_ref = 0; T.stack_cap = r1.stack_need + 1; T.top_avail = r1.top_avail; T.depth = r1.depth;
        return true;
    }
    (void)hipGetLastError();
    T.nodes.release();
    return false;
}

// The same tree by the host builder (pt_tree_sweep.h), in internal form.  built(): called once the builder has run.
template <class Built>
bool internal_tree_host(const std::vector<float>& leaf_boxes, int N, TreeHost& fast, Built built) {
    for (size_t k = 0; k < leaf_boxes.size(); k++)
        if (!std::isfinite(leaf_boxes[k])) return false;
    std::vector<pt_bvh_node> fnodes;
    int32_t froot = 0, fdepth = 0;
    bool ok = true;
    try {
        pts::build_sweep_tree(leaf_boxes.data(), N, fnodes, &froot, &fdepth);
    } catch (const std::exception&) {        // out of host memory: the caller's tree serves alone
        ok = false;
    }
    built();
    bool fnested = true;
    return ok && convert_tree(fnodes.data(), (int)fnodes.size(), froot, N, fast, nullptr, &fnested, true) == PT_OK && fnested;
}

// Inner visits of the probe rays (pt_kernels.h: probe_kernel) through the trees d0 and d1 point at, into v[0] and v[1].
int probe_trees(const SceneDev& d0, const SceneDev& d1, unsigned long long v[2]) {
    DevBuf<unsigned long long> visits;
    int rc;
    if ((rc = visits.ensure(2))) return rc;
    HIP_TRY(hipMemset(visits.p, 0, 2 * sizeof(unsigned long long)));
    const uint32_t lds = (uint32_t)(kBlock / 64) * (uint32_t)std::max(d0.stack_cap, d1.stack_cap) * 64u * 4u;
    hipLaunchKernelGGL(probe_kernel, dim3(kProbeRays / kBlock, 2), dim3(kBlock), lds, nullptr, d0, d1, visits.p);
    HIP_TRY(hipGetLastError());
    v[0] = v[1] = 0;
    HIP_TRY(hipMemcpy(v, visits.p, 2 * sizeof(unsigned long long), hipMemcpyDeviceToHost));
    return PT_OK;
}
int64_t probe_permille(const unsigned long long v[2]) { return v[0] ? (int64_t)((1000ull * v[1] + v[0] / 2) / v[0]) : 1000; }
bool probe_wins(const unsigned long long v[2]) { return v[1] * 100ull < v[0] * 90ull; }   // at least 10 % fewer boxes

// The leaf sweep's groups of equal leaf boxes (pt_leaf_sweep.h) and its tables (pt_sweep_layout.h) from an internal tree as the
// host built it; prims: the N <= kSweepMaxPrims records on the host.  groups = 0: none; sweep.count stays 0 where a launch
// would not admit them.
int make_sweep_tables(const TreeHost& fast, const DPrim* prims, int N, SweepTable& sweep, int& sweep_groups, DevBuf<unsigned char>& sweep_tab) {
    sweep = SweepTable{};
    sweep_groups = 0;
    SweepGroup groups[kSweepMaxPrims];
    const int n = build_sweep_groups(fast.nodes.data(), (int)fast.nodes.size(), N, kLdsNodeStride, groups);
    if (n > 0) {
        sweep_groups = n;
        std::vector<unsigned char> tab(n <= kSweepMaxBoxes ? sweep_layout_bytes((uint32_t)n, (uint32_t)N) : 0);
        if (n <= kSweepMaxBoxes && build_sweep_layout(groups, n, fast.nodes.data(), (int)fast.nodes.size(), kLdsNodeStride, prims, N, tab.data())) {
            int rc;
            if ((rc = sweep_tab.ensure(tab.size()))) return rc;
            HIP_TRY(hipMemcpy(sweep_tab.p, tab.data(), tab.size(), hipMemcpyHostToDevice));
            sweep.count = (uint32_t)n;
            std::copy(groups, groups + n, sweep.g);
        }
    }
    return PT_OK;
}

int validate_and_build(const pt_scene_desc* d, pt_scene* S) {
    if (!d) return fail(PT_ERR_INVALID_ARG, "null scene description");
    if (d->num_shapes <= 0 || !d->shapes) return fail(PT_ERR_BAD_SCENE, "scene has no shapes");
    if (d->num_nodes != 2 * d->num_shapes - 1 || !d->nodes)
        return fail(PT_ERR_BAD_SCENE, "BVH must have 2*num_shapes-1 nodes (bvh.cu:16-54)");
    if (d->root < 0 || d->root >= d->num_nodes) return fail(PT_ERR_BAD_SCENE, "BVH root out of range");
    if (d->num_materials <= 0 || !d->materials) return fail(PT_ERR_BAD_SCENE, "scene has no materials");
    if (d->num_meshes < 0 || (d->num_meshes > 0 && !d->meshes)) return fail(PT_ERR_BAD_SCENE, "bad mesh array");
    if (d->num_lights < 0 || (d->num_lights > 0 && !d->lights)) return fail(PT_ERR_BAD_SCENE, "bad light array");
    int crc;
    if ((crc = check_materials(d)) || (crc = check_meshes(d, d->num_materials))) return crc;

    // ---- primitives
    using clk = std::chrono::steady_clock;
    auto us_since = [](clk::time_point t0) { return (int64_t)std::chrono::duration_cast<std::chrono::microseconds>(clk::now() - t0).count(); };
    const clk::time_point t_all = clk::now();
    clk::time_point t_stage = t_all;
    const int N = d->num_shapes;
    const bool on_device = N >= kDeviceSweepMin && !host_sweep_forced();     // big scenes are prepared on the device (see below)
    std::vector<DPrim> prims(on_device ? 0 : N);
    std::vector<DNormals> normals(on_device ? 0 : N);
    S->tri_only = true;
    if (on_device) {
        int prc, has_sphere = 0;
        if ((prc = S->prims.ensure((size_t)N)) || (prc = S->normals.ensure((size_t)N))) return prc;
        if ((prc = ptp::prims_device(d, S->prims.p, S->normals.p, &has_sphere))) return prc;
        S->tri_only = !has_sphere;
    } else {
    std::memset(prims.data(), 0, sizeof(DPrim) * N);
    std::memset(normals.data(), 0, sizeof(DNormals) * N);
    for (int i = 0; i < N; i++) {
        const pt_shape& s = d->shapes[i];
        DPrim& p = prims[i];
        if (s.type == PT_SHAPE_SPHERE) {
            if (s.material_id < 0 || s.material_id >= d->num_materials) return fail(PT_ERR_BAD_SCENE, "sphere material id out of range");
            p.v[0] = s.center[0]; p.v[1] = s.center[1]; p.v[2] = s.center[2]; p.v[3] = s.radius;
            p.info = (int32_t)(0x80000000u | (uint32_t)s.material_id);
            p.light = s.area_light_id;
            S->tri_only = false;
        } else if (s.type == PT_SHAPE_TRIANGLE) {
            if (s.mesh_index < 0 || s.mesh_index >= d->num_meshes) return fail(PT_ERR_BAD_SCENE, "triangle mesh index out of range");
            const pt_mesh& me = d->meshes[s.mesh_index];
            if (s.face_index < 0 || s.face_index >= me.num_faces) return fail(PT_ERR_BAD_SCENE, "triangle face index out of range");
            const int32_t* idx = me.indices + 3 * (size_t)s.face_index;
            for (int k = 0; k < 3; k++) {
                if (idx[k] < 0 || idx[k] >= me.num_vertices) return fail(PT_ERR_BAD_SCENE, "vertex index out of range");
                for (int c = 0; c < 3; c++) {
                    p.v[3 * k + c] = me.positions[3 * (size_t)idx[k] + c];
                    normals[i].n[3 * k + c] = me.normals[3 * (size_t)idx[k] + c];
                }
            }
            p.info = me.material_id;
            p.light = me.area_light_id;
        } else {
            return fail(PT_ERR_BAD_SCENE, "unknown shape type");
        }
    }
    }

    S->diffuse_only = all_diffuse(d);

    S->create_us[1] = us_since(t_stage); t_stage = clk::now();
    // ---- BVH: the caller's tree (validated), and the internal tree over the same leaf boxes
    // From kDeviceSweepMin primitives up all of it happens on the device (pt_scene_prep.hip, pt_sweep_build.hip): the caller's
    // pool goes up once, is checked and re-laid there, its leaf boxes feed the sweep builder, the builder's pool is re-laid in
    // turn — nothing of either tree comes back to the host.  The host code below serves small scenes, PT_SWEEP_BUILD=host, and
    // whatever the device path hands back (input that runs into the sweep builder's depth guard).
    TreeHost ref;
    TreeHost fast;
    bool have_fast = false;
    bool trees_on_device = false;              // tree[0] (and tree[1] when have_fast) already sit in S->tree[]
    int ref_depth = 0;
    size_t ref_inner = 0;
    DevBuf<pt_bvh_node> pool_dev;              // the caller's pool and the map pool index -> DNode index (tie tables)
    DevBuf<int32_t> iop_dev;
    S->sweep_on_device = 0;
    if (on_device) {
        DevBuf<float> boxes_dev;
        ptp::RelayResult r0;
        int prc;
        if ((prc = pool_dev.ensure((size_t)d->num_nodes)) || (prc = iop_dev.ensure((size_t)d->num_nodes)) || (prc = boxes_dev.ensure((size_t)N * 6)) ||
            (prc = S->tree[0].nodes.ensure((size_t)N - 1)))
            return prc;
        HIP_TRY(hipMemcpy(pool_dev.p, d->nodes, (size_t)d->num_nodes * sizeof(pt_bvh_node), hipMemcpyHostToDevice));
        prc = ptp::relay_tree_device(pool_dev.p, d->num_nodes, d->root, N, false, S->tree[0].nodes.p, iop_dev.p, boxes_dev.p, kBlock, kTopNodes,
                                     kMaxLdsBudget, &r0);
        if (prc) return prc;                   // PT_ERR_BAD_SCENE with the host path's messages
        {
            pt_scene::Tree& T0 = S->tree[0];
            T0.have_oct = false; T0.num_nodes = N - 1; T0.root_ref = 0; T0.stack_cap = r0.stack_need + 1; T0.top_avail = r0.top_avail; T0.depth = r0.depth;
        }
        ref_depth = r0.depth;
        ref_inner = (size_t)N - 1;
        trees_on_device = true;
        S->create_us[2] = us_since(t_stage); t_stage = clk::now();
        if (r0.nested) {
            // (why a tree of the library's own may stand in for a nested caller's tree: see the host path below)
            if (internal_tree_device(boxes_dev.p, N, S->tree[1], [&] { S->create_us[3] = us_since(t_stage); t_stage = clk::now(); })) {
                have_fast = true;
                S->sweep_on_device = 1;
            } else {
                // the device builder handed the input back (depth guard) or failed: the host builder, from the leaf boxes
                std::vector<float> leaf_boxes((size_t)N * 6);
                have_fast = hipMemcpy(leaf_boxes.data(), boxes_dev.p, leaf_boxes.size() * sizeof(float), hipMemcpyDeviceToHost) == hipSuccess &&
                            internal_tree_host(leaf_boxes, N, fast, [] {});
            }
            if (!have_fast) S->no_fast_why = "the internal tree could not be built";
        } else {
            S->no_fast_why = "the caller's boxes do not nest";
        }
    } else {
        std::vector<float> leaf_boxes((size_t)N * 6);
        bool nested = true;
        int trc = convert_tree(d->nodes, d->num_nodes, d->root, N, ref, leaf_boxes.data(), &nested);
        if (trc) return trc;
        ref_depth = ref.depth;
        ref_inner = ref.nodes.size();
        S->create_us[2] = us_since(t_stage); t_stage = clk::now();
        if (N >= kMinInternalTree && nested) {
            // A leaf is tested by the reference iff the ray hits every box on its way down (scene.h:278-297, no pruning).  The slab
            // test is monotone in the box (rounding is), so where every box contains its children's that is: iff it hits the LEAF's
            // own box — whatever the tree above it.  `nested` says the caller's tree is of that kind; then any tree over the same
            // leaf boxes tests the same leaves, and only the ORDER of the tests (ties on t, scene.h:270) still depends on the tree.
            // The tree: all cuts along x, y and z at every node (pt_tree_sweep.h), as deep as it likes — traversed left child
            // first, its stack need is its Strahler number, not its depth (convert_tree).
            have_fast = internal_tree_host(leaf_boxes, N, fast, [&] { S->create_us[3] = us_since(t_stage); t_stage = clk::now(); });
            if (!have_fast) S->no_fast_why = "the internal tree could not be built";
        } else {
            S->no_fast_why = N < kMinInternalTree ? "fewer than 16 shapes" : "the caller's boxes do not nest";
        }
    }
    S->create_us[4] = us_since(t_stage); t_stage = clk::now();
    // trees the device path made are in S->tree[] already; what the host made is uploaded below
    const TreeHost* hosts[2] = {trees_on_device ? nullptr : &ref, (have_fast && !S->sweep_on_device) ? &fast : nullptr};
    std::vector<DMaterial> mats;
    std::vector<DEmission> emis;
    std::vector<DLight> dlights;
    int rc;
    if ((rc = pack_shading(d, N, mats, emis, dlights))) return rc;
    for (int t = 0; t < 2; t++)
        if (hosts[t] && (rc = upload_tree(S->tree[t], *hosts[t]))) return rc;
    S->have_fast = have_fast;
    if (!on_device && ((rc = S->prims.ensure(prims.size())) || (rc = S->normals.ensure(normals.size())))) return rc;
    if ((rc = S->materials.ensure(mats.size()))) return rc;
    if ((rc = S->emission.ensure(emis.size()))) return rc;
    if ((rc = S->lights.ensure(dlights.size()))) return rc;
    HIP_TRY(hipMemcpy(S->lights.p, dlights.data(), dlights.size() * sizeof(DLight), hipMemcpyHostToDevice));
    if (!on_device) {
        HIP_TRY(hipMemcpy(S->prims.p, prims.data(), prims.size() * sizeof(DPrim), hipMemcpyHostToDevice));
        HIP_TRY(hipMemcpy(S->normals.p, normals.data(), normals.size() * sizeof(DNormals), hipMemcpyHostToDevice));
    }
    HIP_TRY(hipMemcpy(S->materials.p, mats.data(), mats.size() * sizeof(DMaterial), hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(S->emission.p, emis.data(), emis.size() * sizeof(DEmission), hipMemcpyHostToDevice));

    SceneDev& dv = S->dev;
    dv.prims = S->prims.p; dv.normals = S->normals.p;
    dv.materials = S->materials.p; dv.emission = S->emission.p; dv.lights = S->lights.p;
    dv.num_prims = N;
    dv.num_materials = d->num_materials;
    dv.num_emission = d->num_lights;
    dv.bg[0] = d->background[0]; dv.bg[1] = d->background[1]; dv.bg[2] = d->background[2];
    // Keep the internal tree only where it is the better one FOR THIS KIND OF RAY: without pruning a node is visited iff the
    // ray hits its box, and what the boxes of a tree add up to depends on the scene (a soup of large overlapping triangles is
    // better off with the caller's median splits than with cuts of the Morton order; a far-away ground sphere skews any
    // surface-area estimate).  So measure: the same probe rays — from random points on the primitives into uniform
    // directions, which is where and how the segments after the first bounce start — through both trees, inner visits counted.
    S->fast_cost_permille = 0;
    if (have_fast) {
        select_tree(S, 0);
        const SceneDev d0 = S->dev;
        select_tree(S, 1);
        const SceneDev d1 = S->dev;
        unsigned long long v[2] = {0, 0};
        if ((rc = probe_trees(d0, d1, v))) return rc;
        S->fast_cost_permille = probe_permille(v);
        if (!probe_wins(v)) {                               // not at least 10 % fewer boxes: the sweep tree is not worth having
            S->have_fast = false;
            S->no_fast_why = "the sweep tree lost the probe on an LDS-resident scene";
            S->tree[1].nodes.release();
            S->tree[1].nodes_oct.release();
            S->tree[1].have_oct = false;
            // ... but the way the internal tree is TRAVERSED still is, for scenes in global memory: left child first with the
            // children ordered for a short stack, leaves set aside, ties settled in place.  So the caller's own topology becomes the
            // internal tree (a caller who hands in a tree as good as the sweep tree: 5.43 -> 4.9 ms on bunny,
            // profiles/r02_device_bvh_build.log).
            const bool global_scene = (size_t)N * (sizeof(DPrim) + sizeof(DNormals)) + ref_inner * sizeof(DNode) > kLdsSceneLimit;
            if (global_scene) {
                TreeHost own;
                bool own_nested = true;
                if (convert_tree(d->nodes, d->num_nodes, d->root, N, own, nullptr, &own_nested, true) == PT_OK && own_nested) {
                    if ((rc = upload_tree(S->tree[1], own))) return rc;
                    S->have_fast = true;
                    S->fast_is_callers_topology = true;
                }
            }
        }
    }
    S->create_us[5] = us_since(t_stage); t_stage = clk::now();
    if (S->have_fast) {
        // what settles ties on t in the caller's visit order: every primitive's path from the caller's root (turn bits) and
        // the inner nodes along it.  (Depth <= 64 levels of leaves and inner nodes: at most 63 turns.)
        const int levels = std::max(ref_depth - 1, 1);
        const size_t anc_words = (size_t)N * (size_t)levels;
        if (S->ref_path.ensure((size_t)N) || S->ref_anc.ensure(anc_words)) {
            // no room for the tables (num_shapes x depth words): the scene simply keeps to the caller's tree
            (void)hipGetLastError();
            S->have_fast = false;
            S->no_fast_why = "there was no room for the tie tables";
            S->fast_is_callers_topology = false;
            S->ref_path.release(); S->ref_anc.release();
            S->tree[1].nodes.release(); S->tree[1].nodes_oct.release(); S->tree[1].have_oct = false;
        } else {
            bool made = false;
            if (trees_on_device) {
                // on the device: every leaf of the caller's pool (uploaded above) walks to the root (pt_scene_prep.hip) — a
                // depth-first walk over a million leaves writing a 100 MB table is 150 ms of host time, and the table would
                // have to be uploaded
                DevBuf<int32_t> parent_dev;
                if (!parent_dev.ensure((size_t)d->num_nodes) && hipMemset(S->ref_anc.p, 0, anc_words * sizeof(int32_t)) == hipSuccess)
                    made = ptp::tie_tables_device(pool_dev.p, d->num_nodes, d->root, iop_dev.p, N, levels, parent_dev.p, S->ref_path.p, S->ref_anc.p) == PT_OK;
                if (!made) return fail(PT_ERR_DEVICE, "tie tables on the device failed");
            }
            if (!made) {
                std::vector<unsigned long long> path(N, 0ull);
                std::vector<int32_t> anc(anc_words, 0);
                struct Walk { int32_t node; int32_t level; unsigned long long turns; };
                std::vector<Walk> todo;
                std::vector<int32_t> trail(levels, 0);
                todo.push_back({d->root, 0, 0ull});
                while (!todo.empty()) {
                    const Walk w = todo.back();
                    todo.pop_back();
                    const pt_bvh_node& nd = d->nodes[w.node];
                    if (nd.prim != -1) {
                        path[nd.prim] = w.turns;
                        std::memcpy(&anc[(size_t)nd.prim * levels], trail.data(), (size_t)w.level * sizeof(int32_t));
                        continue;
                    }
                    trail[w.level] = ref.inner_of_pool[w.node];
                    // depth-first, left subtree first: `trail` below w.level is still this node's path when its right child is taken up
                    todo.push_back({nd.right, w.level + 1, w.turns | (1ull << w.level)});
                    todo.push_back({nd.left, w.level + 1, w.turns});
                }
                HIP_TRY(hipMemcpy(S->ref_path.p, path.data(), path.size() * sizeof(unsigned long long), hipMemcpyHostToDevice));
                HIP_TRY(hipMemcpy(S->ref_anc.p, anc.data(), anc.size() * sizeof(int32_t), hipMemcpyHostToDevice));
            }
            S->ref_levels = levels;
        }
    }
    // the leaf sweep's groups of equal leaf boxes (pt_leaf_sweep.h), from the internal tree as the host built it
    S->sweep = SweepTable{};
    S->sweep_groups = 0;
    if (S->have_fast && hosts[1] && !S->fast_is_callers_topology && N <= kSweepMaxPrims &&
        (rc = make_sweep_tables(fast, prims.data(), N, S->sweep, S->sweep_groups, S->sweep_tab)))
        return rc;
    // everything the scene holds is complete from here on: trace kernels run on streams of the handle's own (FrameSlot) that do
    // not synchronise with the stream the preparation kernels ran on
    HIP_TRY(hipDeviceSynchronize());
    S->create_us[6] = us_since(t_stage);
    S->create_us[0] = us_since(t_all);
    select_tree(S, 0);
    S->scene_bytes = (uint32_t)std::min<size_t>(
        ref_inner * sizeof(DNode) + (size_t)N * (sizeof(DPrim) + sizeof(DNormals)) + mats.size() * sizeof(DMaterial) +
            emis.size() * sizeof(DEmission) + 64, 0xffffffffu);
    return PT_OK;
}

// The tree a render traverses: the internal tree on the default kernel where scene creation kept one (see launch_render), the
// caller's tree otherwise.  Pruned traversal (opt-in, tolerance semantics: DESIGN.md §6) takes the internal tree as well — left
// child first like the exact one, so that its short stacks hold; bunny 7.55 -> 3.89 ms, no pixel moved.
int which_tree(const pt_scene* S) {
    return (S->have_fast && S->opt_fast_tree && S->opt_kernel >= 2) ? 1 : 0;
}

// Residency the next launch will use (see make_plan).
int scene_residency(const pt_scene* S, int which = 0) {
    const pt_scene::Tree& T = S->tree[which];
    if (S->opt_force_global || S->scene_bytes > kLdsSceneLimit)
        return (T.top_avail > 0 && S->opt_top_cache && S->opt_kernel >= 2 && !S->opt_force_global) ? 3 : 0;
    if (S->opt_kernel >= 2 && S->opt_octants && T.have_oct) return 2;
    return 1;
}

// (thresh, inner, min-waves-per-SIMD) variants compiled in; inner < 0 selects the "vote" burst of -inner steps, 1..9 a
// burst of `inner` inner steps + 1 leaf step, >= 100 the encoded burst REPS*100 + N_INNER*10 + N_LEAF (pt_kernels.h).
// Measured on MI355X (tests/tools/gpu_tune.py, tests/tools/gpu_ab.py, profiles/r01_tune_round*.log): LDS-resident scenes are
// fastest with T40 / 6 inner + 2 leaf steps / W6 (cbox 3.77 ms against 3.99 with 3+1, 4.10 with 4+1, 3.92 with two rounds of
// 3+1; sphere and mixed scenes 1-6 % ahead of the vote burst they used before; r01_tune_round21/22), scenes in global memory with
// T32 / I4 / W6 (bunny 10.7 ms; every other burst shape within 1 %).  I8 and unbounded descent are slower, T56 starves the
// scheduler phase, W6 (<= 80 VGPRs -> 6 waves/SIMD) beats the unconstrained 82-VGPR build by 3-5 %, W8 (64 VGPRs, spills)
// is 5-8 % slower.  Re-checked on the internal tree (fewer inner visits per leaf test): 6 + 2 still wins on LDS-resident scenes
// (cbox: 5+2 +2.4 %, 4+2 +4.6 %, 3+2 +5.4 %, two rounds of 2+1 +13 %; thresholds 24 / 32 / 48 / 56: +1.7 / 0.0 / +1.2 / +7.5 %; profiles/r02_tune_round44_lds_bursts_rejected.log,
// r02_tune_round46_thresh_rejected.log).
struct V2Schedule {
    int thresh, inner, minw;
};
constexpr V2Schedule kV2Schedules[] = {
    {40, -6, 6}, {32, 4, 6}, {40, 4, 6}, {40, 3, 6}, {40, 162, 6}, {32, 1004, 6}, {32, 1231, 6},
    {32, 1231, 5}, {40, 162, 5},        // 96 VGPRs, 5 waves per SIMD: for the instantiations that spill under the 80-VGPR cap
};

// A schedule of trace_kernel_v2 with its zeros, 0 = automatic, resolved for a residency; set_aside: on the internal tree.
// LDS-resident: 6 inner + 2 leaf steps; global memory: 4 + 1 on the caller's tree; on the internal tree two rounds of
// 3 + 1 with leaves set aside (v2_inner 1000 + burst).  Setting leaves aside: bunny -2.2 %, dragon stand-in -3.4 %
// against the plain 4 + 1 (LDS-resident scenes lose 9 % with it: profiles/r02_tune_round43_postponed_leaves.log); two
// rounds of 3 + 1 instead of one of 4 + 1: teapot -8.5 %, bunny -1.2 %, buddha stand-in -1.5 %, dragon stand-in -1.8 %
// (r02_tune_round48_global_thresh.log, r02_tune_round49_global_burst.log; thresholds 24 / 40 / 48 lose, so do three rounds of
// 3 + 1 and two of 2 + 1, and every set-aside shape on LDS-resident scenes: r02_tune_round50_more_bursts_rejected.log; 7 / 8 waves per
// SIMD by register cap, with the blocks to match: +11..16 % / +28..41 % from the spills, r02_tune_round51_more_waves_rejected.log).
constexpr V2Schedule v2_schedule(V2Schedule s, bool lds, bool set_aside) {
    if (s.thresh == 0) s.thresh = lds ? 40 : 32;
    if (s.inner == 0) s.inner = lds ? 162 : (set_aside ? 1231 : 4);
    if (s.minw == 0) s.minw = 6;
    return s;
}

// Everything about a trace launch that is settled before a kernel is looked up.  launch_render and the info keys that
// describe the next launch read the same one (choose_trace).
struct TraceChoice {
    int which;                   // the tree traversed (which_tree)
    int res;                     // 0 scene in global memory, 1 scene staged in LDS, 2 staged in LDS with the 8 octant node tables,
                                 // 3 scene in global memory with the top of the tree cached in LDS
    int family;                  // 1 trace_kernel, 2 trace_kernel_v2 (_reg, _sweep), 3 trace_kernel_q
    bool prune, stats, nee, list, postpone;
    int spec;                    // 0 generic scene content, 1 triangles only, 2 triangles with diffuse materials only
    V2Schedule sched;            // family 2
    bool reg_stack;              // the kernel keeps its traversal stack in a register (pt_reg_stack.h), the block has no stack columns
    bool sweep;                  // trace_kernel_v2_sweep stands in for the register-stack entry
    int block_threads;
    int feed_waves;              // waves per block that draw from the work feed
    int redo_lanes;              // lanes per block that rerun segments in reference order (one global-memory stack column each)
    bool lds_scene() const { return res == 1 || res == 2; }
};

int choose_trace(const pt_scene* S, int traversal, bool nee, bool listed, TraceChoice* out) {
    TraceChoice c{};
    // Exact traversal runs on the internal tree where scene creation kept one.  What depends on the visit order is handled the
    // reference's way: two valid hits with equal t (the first one VISITED wins, scene.h:270) are ordered by one box test in
    // the caller's tree (pt_trace.h: ref_visits_first); rays with a zero direction component (1/d infinite: the monotonicity
    // argument of validate_and_build does not cover 0 * inf) are traced on the caller's tree in reference order.
    c.which = which_tree(S);
    c.res = scene_residency(S, c.which);
    const bool exact = traversal == PT_TRAVERSAL_EXACT;
    if (nee && (S->opt_kernel < 2 || !exact))
        return fail(PT_ERR_UNSUPPORTED, "PT_RENDER_NEE runs on the default kernel with exact traversal only");
    // kernel 3 (paths regrouped across the waves of a workgroup) serves exact traversal without next-event estimation or a pixel
    // list; those run on kernel 2
    c.family = S->opt_kernel == 1 ? 1 : (S->opt_kernel == 3 && !nee && exact && !listed) ? 3 : 2;
    c.prune = !exact; c.stats = S->opt_stats != 0; c.nee = nee; c.list = listed;
    // scenes in global memory set leaves aside on the internal tree (order-free leaf tests need its tie handling)
    c.postpone = c.family == 3 && !c.lds_scene() && c.which == 1;
    c.spec = !(S->tri_only && S->opt_specialize) ? 0 : (S->diffuse_only ? 2 : 1);
    if (nee && c.spec == 1) c.spec = 0;     // with NEE: generic scene content or triangles-with-diffuse-materials only
    // The LIST and NEE kernels are compiled for the automatic schedule of every residency only — the v2_* knobs change no bit,
    // so these launches ignore them — and NEE sets no leaves aside.
    if (c.family == 2)
        c.sched = v2_schedule((nee || listed) ? V2Schedule{0, 0, 6} : V2Schedule{(int)S->opt_v2_thresh, (int)S->opt_v2_inner, (int)S->opt_v2_minw},
                              c.lds_scene(), c.which == 1 && !nee);
    // The traversal stack in a register: option "reg_stack" allows it, the launch runs trace_kernel_v2 without next-event
    // estimation or a pixel list on a scene of triangles with diffuse materials (the instantiations compiled with it:
    // find_trace), and reg_stack_on holds for its residency, schedule and tree.  The schedule must be the automatic one:
    // options "v2_thresh" / "v2_inner" name an instantiation of trace_kernel_v2, and a caller who sets them gets that one
    // (the tuning tools and the test of every compiled instantiation select kernels that way).  Decided before the LDS plan
    // is made: such a block has no stack columns.
    const pt_scene::Tree& T = S->tree[c.which];
    c.reg_stack = S->opt_reg_stack && c.family == 2 && !nee && !listed && c.spec == 2 && !S->opt_v2_thresh && !S->opt_v2_inner &&
                  (c.sched.minw == 5 || c.sched.minw == 6) &&
                  reg_stack_on(c.res, c.sched.thresh, c.sched.inner, c.which == 1, T.stack_cap - 1, T.num_nodes, S->dev.num_prims);
    // Leaves found by the box sweep (pt_leaf_sweep.h): option "leaf_sweep" allows it, the launch is one of
    // trace_kernel_v2_reg<2, false, false, MINW> (register stack, octant tables, exact, not counting), and the handle holds a group
    // table that fits: made at scene creation, dropped by a geometry update.  The kernel stands in for that table entry: same
    // LDS plan, and it reports that entry's "trace_variant", "reg_stack" and "path_bank"; info "leaf_sweep" alone tells them apart.
    // The sweep's own tables (pt_sweep_layout.h) go where that plan has the octant node tables: a launch whose tables do not fit
    // there takes the tree (a binary tree over 3 primitives or more always leaves the room).
    c.sweep = S->opt_leaf_sweep && leaf_sweep_on(c.reg_stack, exact, c.stats, c.res, S->dev.num_prims, (int)S->sweep.count) &&
              S->sweep_tab.p && sweep_layout_fits(S->sweep.count, (uint32_t)S->dev.num_prims, (uint32_t)T.num_nodes, kLdsNodeStride);
    c.block_threads = c.family == 3 ? kQBlock : kBlock;
    c.feed_waves = c.family == 3 ? kQS : kBlock / 64;
    c.redo_lanes = c.family == 3 ? kQS * 64 : kBlock;            // kernel 3: its S-waves rerun
    *out = c;
    return PT_OK;
}

// LDS plan of trace_kernel and trace_kernel_v2 (the latter keeps 16-bit stacks for LDS scenes, none with a register stack).
LdsPlan make_plan(const pt_scene* S, const TraceChoice& c) {
    LdsPlan lp{};
    const pt_scene::Tree& T = S->tree[c.which];
    uint32_t off = 0;
    if (c.res == 3) {
        // as many top nodes as fit next to the stacks within the block's LDS budget (default: without costing a resident block)
        const uint32_t stack_bytes = (uint32_t)(kBlock / 64) * (uint32_t)T.stack_cap * 64u * 4u;
        const uint32_t budget = S->opt_lds_budget_kb > 0 ? (uint32_t)S->opt_lds_budget_kb * 1024u : kTopLdsBudget;
        const uint32_t room = budget > stack_bytes ? budget - stack_bytes : 0u;
        lp.top_count = std::min<uint32_t>(T.top_avail, room / (uint32_t)sizeof(DNode));
        lp.nodes_off = 0;
        off = lp.top_count * (uint32_t)sizeof(DNode);
    } else if (c.res != 0) {
        lp.nodes_off = off;
        off = align16(off + (c.res == 2 ? 8u * oct_table_pitch((uint32_t)T.num_nodes, kLdsNodeStride)
                                        : (uint32_t)T.num_nodes * kLdsNodeStride));
        lp.prims_off = off; off = align16(off + (uint32_t)S->dev.num_prims * sizeof(DPrim));
        lp.normals_off = off; off = align16(off + (uint32_t)S->dev.num_prims * sizeof(DNormals));
        lp.mats_off = off; off = align16(off + (uint32_t)S->dev.num_materials * sizeof(DMaterial));
        lp.emis_off = off; off = align16(off + (uint32_t)std::max(S->dev.num_emission, 1) * sizeof(DEmission));
    }
    lp.stack_off = off;
    const bool stack16 = c.lds_scene() && c.family >= 2;
    if (!c.reg_stack) off += (uint32_t)(kBlock / 64) * (uint32_t)T.stack_cap * 64u * (stack16 ? 2u : 4u);
    lp.total = align16(off);
    return lp;
}

// LDS plan of trace_kernel_q, from make_plan's: the staged scene as for v2, 16-bit traversal stacks for the kQT traversal waves
// only, then the control words and the two rings (contiguous: the kernel clears them in one sweep).  Also settles the schedule knobs.
QParams make_plan_q(const pt_scene* S, const TraceChoice& c, LdsPlan& lp) {
    QParams q{};
    const pt_scene::Tree& T = S->tree[c.which];
    const uint32_t stack_bytes = (uint32_t)kQT * (uint32_t)T.stack_cap * 64u * (c.lds_scene() ? 2u : 4u);
    // scenes in global memory carry 32-bit stacks as deep as the tree's Strahler number: they run with rings of half the size, and
    // the top of the tree takes what two workgroups per CU leave (160 KB / 2, minus stacks and rings)
    uint32_t ring = kQRing;
    if (!c.lds_scene()) ring = std::max<uint32_t>(64u, kQRing / 2);
    q.ring_log2 = 0;
    while ((1u << q.ring_log2) < ring) q.ring_log2++;
    const uint32_t ring_bytes = kQCtlBytes + 2u * ring * kQEntryBytes;
    if (c.res == 3) {
        const uint32_t budget = S->opt_lds_budget_kb > 0 ? (uint32_t)S->opt_lds_budget_kb * 1024u : 80u * 1024u;
        const uint32_t used = stack_bytes + ring_bytes + 64u;
        lp.top_count = std::min<uint32_t>(T.top_avail, budget > used ? (budget - used) / (uint32_t)sizeof(DNode) : 0u);
        lp.nodes_off = 0;
        lp.stack_off = lp.top_count * (uint32_t)sizeof(DNode);
    }
    uint32_t off = align16(lp.stack_off + stack_bytes);
    q.ctl_off = off; off += kQCtlBytes;
    q.shade_off = off; off += ring * kQEntryBytes;
    q.ready_off = off; off += ring * kQEntryBytes;
    lp.total = align16(off);
    // Paths in flight per workgroup.  The bound that keeps the rings from filling up for good (pt_kernel_q.h): with every
    // T-lane holding a finished path, a ring that cannot take a wave's worth more (> ring - 64 entries each) — that many
    // paths must not exist:  target <= T-lanes + 2 x ring - 128.
    const int32_t t_lanes = kQT * 64, cap = t_lanes + 2 * (int32_t)ring - 128;
    int32_t target = S->opt_q_target > 0 ? (int32_t)S->opt_q_target : t_lanes + (int32_t)ring;
    q.target = std::max(64, std::min(target, cap));
    q.swap = S->opt_q_swap > 0 ? (int32_t)std::min<int64_t>(S->opt_q_swap, 64) : 16;
    q.low = S->opt_q_low > 0 ? (int32_t)S->opt_q_low : 8;
    return q;
}

// The LDS plan of a launch and, for kernel 3, its schedule parameters.
int plan_trace(const pt_scene* S, const TraceChoice& c, LdsPlan* lp, QParams* qp) {
    *lp = make_plan(S, c);
    if (lp->total > S->lds_per_block_max) return fail(PT_ERR_DEVICE, "LDS plan exceeds the per-block limit");
    if (c.family != 3) return PT_OK;
    *qp = make_plan_q(S, c, *lp);
    if (lp->total > S->lds_per_block_max) return fail(PT_ERR_DEVICE, "LDS plan exceeds the per-block limit");
    return PT_OK;
}

// Info "trace_variant": the template arguments of a trace kernel in one int64 (packing: include/pt_api.h).  find_trace hands
// it back next to the kernel, both made from the same template arguments (v1k / v2k / v2rk / qk), so that the value reported
// for a launch cannot disagree with the kernel launched.
constexpr int64_t trace_variant(int family, int res, bool prune, bool stats, int spec, bool nee, bool list, bool postpone,
                                int thresh, int inner, int minw, bool reg = false) {
    return (int64_t)family | (int64_t)res << 4 | (int64_t)prune << 6 | (int64_t)stats << 7 | (int64_t)spec << 8 |
           (int64_t)nee << 10 | (int64_t)list << 11 | (int64_t)postpone << 12 | (int64_t)reg << 13 | (int64_t)thresh << 16 |
           (int64_t)(uint16_t)(int16_t)inner << 24 | (int64_t)minw << 40;
}
// The three argument lists of the trace kernels; TraceChoice says which one an entry's kernel takes (launch_trace).
using TraceFn = void (*)(SceneDev, RenderDev, LdsPlan, float4*, uint32_t*, unsigned long long*);
using TraceFnQ = void (*)(SceneDev, RenderDev, LdsPlan, QParams, float4*, uint32_t*, unsigned long long*);
using SweepFn = void (*)(SceneDev, RenderDev, LdsPlan, float4*, uint32_t*, unsigned long long*, SweepLayoutDev);
struct TraceEntry {
    const void* fn = nullptr;
    int64_t variant = 0;
    int bank = 0;        // info "path_bank": the kernel hands out path starts from a register bank (pt_kernels.h: path_bank_on)
    int reg = 0;         // info "reg_stack": the kernel keeps its traversal stack in a register (pt_reg_stack.h)
};
template <bool LDS_SCENE, bool PRUNE, bool STATS, bool LIST>
TraceEntry v1k() {
    return {reinterpret_cast<const void*>(&trace_kernel<LDS_SCENE, PRUNE, STATS, LIST>),
            trace_variant(1, LDS_SCENE, PRUNE, STATS, 0, false, LIST, false, 0, 0, 0)};
}
template <int RES, bool PRUNE, bool STATS, int THRESH, int INNER, int MINW, int SPEC, bool NEE, bool LIST>
TraceEntry v2k() {
    static_assert(INNER >= -32768 && INNER <= 32767 && THRESH >= 0 && THRESH < 256 && MINW >= 0 && MINW < 16, "trace_variant fields");
    return {reinterpret_cast<const void*>(&trace_kernel_v2<RES, PRUNE, STATS, THRESH, INNER, MINW, SPEC, NEE, LIST>),
            trace_variant(2, RES, PRUNE, STATS, SPEC, NEE, LIST, false, THRESH, INNER, MINW), path_bank_on(RES, SPEC, NEE, LIST, THRESH, INNER)};
}
template <int RES, bool PRUNE, bool STATS, int MINW>
TraceEntry v2rk() {          // trace_kernel_v2_reg: the template arguments of its trace_v2, and the register-stack bit
    return {reinterpret_cast<const void*>(&trace_kernel_v2_reg<RES, PRUNE, STATS, MINW>),
            trace_variant(2, RES, PRUNE, STATS, 2, false, false, false, 40, 162, MINW, true), path_bank_on(RES, 2, false, false, 40, 162), 1};
}
template <int RES, bool STATS, int SPEC, bool POSTPONE>
TraceEntry qk() {
    return {reinterpret_cast<const void*>(&trace_kernel_q<RES, STATS, SPEC, POSTPONE>),
            trace_variant(3, RES, false, STATS, SPEC, false, false, POSTPONE, 0, 0, 0)};
}

// Which instantiations of the trace kernels are compiled: find_trace names a kernel only where its predicate holds, and
// tests/golden/trace_kernels.txt lists the result.
// trace_kernel_v2 — with NEE: exact traversal, generic scene content or triangles with diffuse materials, the automatic
// schedule of the residency without leaves set aside; with a pixel list: the automatic schedules of the residency; otherwise
// every schedule of kV2Schedules.
constexpr bool v2_compiled(int res, bool prune, V2Schedule s, int spec, bool nee, bool list) {
    const bool lds = res == 1 || res == 2;
    const bool automatic = s.minw == 6 && s.thresh == (lds ? 40 : 32) && (lds ? s.inner == 162 : s.inner == 4 || (s.inner == 1231 && !nee));
    if (nee) return !prune && spec != 1 && automatic;
    return !list || automatic;
}
// trace_kernel_q: LDS-resident scenes set no leaves aside.
constexpr bool q_compiled(int res, bool postpone) { return !(postpone && (res == 1 || res == 2)); }

// f(std::integral_constant<., V>) for the V among Vs that equals v: a runtime value becomes a template argument.  No such V: no kernel.
template <auto... Vs, class T, class F>
TraceEntry among(T v, F f) {
    TraceEntry r{};
    (void)((v == (T)Vs ? (r = f(std::integral_constant<decltype(Vs), Vs>{}), true) : false) || ...);
    return r;
}
#define PT_CONST(x) decltype(x)::value

// The kernel of a choice, or no kernel where none is compiled for it (options "v2_thresh" / "v2_inner" / "v2_minw").
// with_sweep = false: the table entry the sweep kernel stands in for.
TraceEntry find_trace(const TraceChoice& c, bool with_sweep = true) {
    if (c.family == 1)
        return among<false, true>(c.lds_scene(), [&](auto L) { return among<false, true>(c.prune, [&](auto P) {
               return among<false, true>(c.stats, [&](auto S) { return among<false, true>(c.list, [&](auto LI) {
                   return v1k<PT_CONST(L), PT_CONST(P), PT_CONST(S), PT_CONST(LI)>(); }); }); }); });
    if (c.family == 3)
        return among<0, 1, 2, 3>(c.res, [&](auto R) { return among<false, true>(c.stats, [&](auto S) {
               return among<0, 1, 2>(c.spec, [&](auto SP) { return among<false, true>(c.postpone, [&](auto PO) {
                   if constexpr (q_compiled(PT_CONST(R), PT_CONST(PO))) return qk<PT_CONST(R), PT_CONST(S), PT_CONST(SP), PT_CONST(PO)>();
                   else return TraceEntry{}; }); }); }); });
    // trace_kernel_v2_reg (choose_trace: spec 2, thresh 40, burst 162): the default schedule of LDS-resident scenes of triangles
    // with diffuse materials, both register caps.  Each keeps ScratchSize 0 within its cap (profiles/r10_reg_stack.log has the table).
    if (c.reg_stack)
        return among<1, 2>(c.res, [&](auto R) { return among<5, 6>(c.sched.minw, [&](auto W) {
               return among<false, true>(c.prune, [&](auto P) { return among<false, true>(c.stats, [&](auto S) {
                   TraceEntry e = v2rk<PT_CONST(R), PT_CONST(P), PT_CONST(S), PT_CONST(W)>();
                   if (c.sweep && with_sweep) e.fn = reinterpret_cast<const void*>(&trace_kernel_v2_sweep<PT_CONST(W)>);   // keeps the entry's variant
                   return e; }); }); }); });
    if (c.sched.inner >= 1000 && c.which != 1) return {};      // order-free leaf tests need the internal tree's tie handling
    static_assert(std::size(kV2Schedules) == 9, "the index list below enumerates kV2Schedules");
    int si = -1;
    for (int k = 0; k < (int)std::size(kV2Schedules); k++)
        if (kV2Schedules[k].thresh == c.sched.thresh && kV2Schedules[k].inner == c.sched.inner && kV2Schedules[k].minw == c.sched.minw) si = k;
    return among<0, 1, 2, 3, 4, 5, 6, 7, 8>(si, [&](auto SI) { return among<0, 1, 2, 3>(c.res, [&](auto R) {
           return among<false, true>(c.nee, [&](auto N) { return among<false, true>(c.list, [&](auto LI) {
           static constexpr V2Schedule s = kV2Schedules[PT_CONST(SI)];
           // (most NEE and LIST schedules end here: the lambdas below are not instantiated for them, which the build time notices)
           if constexpr (!v2_compiled(PT_CONST(R), false, s, 0, PT_CONST(N), PT_CONST(LI))) return TraceEntry{};
           else return among<0, 1, 2>(c.spec, [&](auto SP) { return among<false, true>(c.prune, [&](auto P) {
           return among<false, true>(c.stats, [&](auto S) {
               if constexpr (v2_compiled(PT_CONST(R), PT_CONST(P), s, PT_CONST(SP), PT_CONST(N), PT_CONST(LI)))
                   return v2k<PT_CONST(R), PT_CONST(P), PT_CONST(S), s.thresh, s.inner, s.minw, PT_CONST(SP), PT_CONST(N), PT_CONST(LI)>();
               else return TraceEntry{}; }); }); }); }); }); }); });
}
#undef PT_CONST

// The one typed launch of a trace kernel: the entry's kernel takes the argument list of the choice's family.
void launch_trace(const pt_scene* S, const TraceChoice& c, const TraceEntry& e, int grid, hipStream_t stream, const RenderDev& rd,
                  const LdsPlan& lp, const QParams& qp, float4* samples) {
    void* const fn = const_cast<void*>(e.fn);
    if (c.family == 3)
        hipLaunchKernelGGL(reinterpret_cast<TraceFnQ>(fn), dim3(grid), dim3(c.block_threads), lp.total, stream, S->dev, rd, lp, qp,
                           samples, S->work_counter(), S->counters());
    else if (c.sweep)
        hipLaunchKernelGGL(reinterpret_cast<SweepFn>(fn), dim3(grid), dim3(c.block_threads), lp.total, stream, S->dev, rd, lp,
                           samples, S->work_counter(), S->counters(), SweepLayoutDev{S->sweep_tab.p, S->sweep.count, 0u});
    else
        hipLaunchKernelGGL(reinterpret_cast<TraceFn>(fn), dim3(grid), dim3(c.block_threads), lp.total, stream, S->dev, rd, lp,
                           samples, S->work_counter(), S->counters());
}

// Sums the kCounterSlots per-workgroup counter slots of the last frame (the caller has synchronised the stream).
int read_slot_sums(const pt_scene* S, unsigned long long* out) {
    std::vector<unsigned long long> raw(kTimelineBase);
    HIP_TRY(hipMemcpy(raw.data(), S->counters(), raw.size() * sizeof(unsigned long long), hipMemcpyDeviceToHost));
    std::fill(out, out + kSlotStride, 0ull);
    for (int s = 0; s < kCounterSlots; s++)
        for (int k = 0; k < kSlotStride; k++) out[k] += raw[(size_t)s * kSlotStride + k];
    return PT_OK;
}

// Blocks of a trace launch: every resident slot of the device, or fewer when there is not enough work to fill them.
int launch_grid(int num_cus, int blocks_per_cu, uint64_t work_items, int block_threads = kBlock) {
    const uint64_t blocks_needed = (work_items + (uint64_t)block_threads - 1) / (uint64_t)block_threads;
    return (int)std::max<uint64_t>(1, std::min<uint64_t>((uint64_t)num_cus * (uint64_t)blocks_per_cu, blocks_needed));
}

struct RowSel {
    int begin, step, count;
};

int select_rows(const pt_render_params* p, RowSel* out) {
    int rb = p->row_begin, re = p->row_end;
    if (rb == 0 && re == 0) re = p->height;
    int step = p->row_stride > 1 ? p->row_stride : 1;
    if (rb < 0 || re > p->height || rb > re) return fail(PT_ERR_INVALID_ARG, "row range outside the image");
    int n = 0;
    for (int j = rb; j < re; j += step) n++;
    *out = RowSel{rb, step, n};
    return PT_OK;
}

// One round of pt_render_adaptive.  Round 0 opens a frame like any render call (slot, counters, timing record) and traces every
// selected pixel; later rounds continue that frame — same slot, counters and timing record — and trace only the pixels of
// args.list_in (handed to launch_render as its pixel list).  The resolve of every pass is adaptive_resolve_kernel.  Adaptive
// frames run on the caller's stream.
struct AdaptiveRound {
    int round;
    AdaptiveArgs args;               // n, spp_pass, first and check are set per pass by launch_render
};

// A pixel list (RenderDev::list): the launch is a frame of n rows of width 1 whose row k is the pixel list[k], a packed id
// (selected row * image width + column; under "all rows" the pixel index).  Device memory, read by the trace kernel.  The
// later rounds of pt_render_adaptive and pt_render_pixels.
struct PixelList {
    const uint32_t* list;
    uint32_t n;
};

// The checks on a render call's arguments that come before its frame is opened, and its row selection.
int check_render_args(const pt_scene* S, const pt_render_params* p, const float* out_dev, const PixelList* pl, RowSel* rows) {
    if (!S || !p || (!out_dev && !(pl && pl->n == 0))) return fail(PT_ERR_INVALID_ARG, "null argument");
    if (p->width <= 0 || p->height <= 0 || p->spp <= 0) return fail(PT_ERR_INVALID_ARG, "width, height and spp must be positive");
    if (p->sample_offset < 0 || p->stream_stride < 0) return fail(PT_ERR_INVALID_ARG, "negative sample_offset / stream_stride");
    // PCG stream = pixel_index*stride + sample_offset + s: samples [sample_offset, sample_offset + spp) must stay below the
    // stride, or pixel p's sample `stride + k` would replay pixel p+1's sample k (identical random sequences in neighbouring
    // pixels).  With the default stride (0 -> spp) that allows sample_offset 0 only: progressive callers pass an explicit
    // stride = any upper bound on the total sample count.
    if ((int64_t)p->sample_offset + p->spp > (int64_t)(p->stream_stride > 0 ? p->stream_stride : p->spp))
        return fail(PT_ERR_INVALID_ARG, p->stream_stride > 0
                        ? "sample_offset + spp exceeds stream_stride: PCG streams of neighbouring pixels would overlap"
                        : "sample_offset > 0 needs an explicit stream_stride >= total sample count (default stride = spp)");
    return select_rows(p, rows);
}

// What opening a frame settles: the call's frame slot (see pt_scene::FrameSlot) and its record in the timing ring.
struct OpenFrame {
    int in_flight;
    bool timing;                 // false: no HIP events around the kernels (four records less per frame)
    bool prev_busy;              // the previous call's frame is still on the GPU
    pt_scene::FrameSlot* slot;
    pt_scene::FrameRec* rec;
    size_t pass_base;            // passes of earlier adaptive rounds of this frame
};
// cont: a later adaptive round, which continues the frame of round 0
int open_frame(pt_scene* S, hipStream_t stream, bool cont, OpenFrame* f) {
    f->in_flight = (int)std::min<int64_t>(kMaxFramesInFlight, std::max<int64_t>(1, S->opt_frames_in_flight));
    f->timing = S->opt_timing_frames > 0;
    // Is the previous call's frame still on the GPU?  If not there is nothing to overlap with, and this frame runs on the
    // caller's stream as with one slot: a caller that synchronises after every frame (a display loop) does not pay for two
    // event waits across streams per frame.
    f->prev_busy = false;
    if (!cont && f->in_flight > 1 && S->frame_seq > 0 && S->cur().used) {
        f->prev_busy = hipEventQuery(S->cur().free_ev) == hipErrorNotReady;
        (void)hipGetLastError();
    }
    if (!cont) S->cur_slot = (int)(S->frame_seq % (uint64_t)f->in_flight);
    f->slot = &S->cur();
    int rc = f->slot->ctl.ensure(kWorkWords + kNumCounters);
    if (rc) return rc;
    if (!f->slot->free_ev) HIP_TRY(hipEventCreateWithFlags(&f->slot->free_ev, hipEventDisableTiming));
    S->last_stream = stream;
    S->have_timing = false;
    if (!cont) {
        S->info_passes = 0;
        // this call's slot of the timing ring
        const size_t ring = (size_t)std::max<int64_t>(1, S->opt_timing_frames);
        if (S->frames.size() != ring) { S->drop_events(); S->frames.resize(ring); }
        S->frames[S->frame_seq % S->frames.size()].passes = 0;
        S->frame_seq++;
    }
    f->rec = &S->frames[(S->frame_seq - 1) % S->frames.size()];
    f->pass_base = f->rec->passes;
    return PT_OK;
}

// A frame with nothing to trace: its counters read zero.
int empty_frame(pt_scene* S, pt_scene::FrameSlot& slot, hipStream_t stream) {
    S->info_trace_variant = 0;
    S->info_path_bank = 0;
    S->info_reg_stack = 0;
    S->info_leaf_sweep = 0;
    if (slot.used && slot.free_stream != stream) HIP_TRY(hipStreamWaitEvent(stream, slot.free_ev, 0));
    HIP_TRY(hipMemsetAsync(slot.ctl.p, 0, (kWorkWords + kTimelineBase) * sizeof(unsigned long long), stream));
    HIP_TRY(hipEventRecord(slot.free_ev, stream));
    slot.used = true; slot.free_stream = stream;
    return PT_OK;
}

// Samples per pass — bounded by the scratch budget and by 2^30 work items per launch — and the passes that makes; the sample
// buffer of the slot (and, for several passes of a plain render, the accumulator) allocated to match.
int plan_passes(pt_scene* S, const pt_render_params* p, int mode, bool adaptive, pt_scene::FrameSlot& slot, uint64_t npix,
                uint64_t* spp_pass_out, int* n_pass_out) {
    if (npix > (1ull << 30)) return fail(PT_ERR_INVALID_ARG, "more than 2^30 pixels per call");
    uint64_t scratch = S->opt_scratch_bytes > 0 ? (uint64_t)S->opt_scratch_bytes : kDefaultScratchBytes;
    if (S->opt_scratch_bytes <= 0 && std::min<uint64_t>(scratch, npix * (uint64_t)p->spp * sizeof(float4)) > slot.samples.n * sizeof(float4)) {
        // the buffer must grow under the default budget: never to more than a quarter of what is free on the device right
        // now, so that several handles / ranks on one GPU, or a smaller GPU, split into more passes instead of failing
        size_t free_b = 0, total_b = 0;
        if (hipMemGetInfo(&free_b, &total_b) == hipSuccess)
            scratch = std::min<uint64_t>(scratch, std::max<uint64_t>((uint64_t)free_b / 4, slot.samples.n * sizeof(float4)));
    }
    uint64_t spp_pass = std::max<uint64_t>(1, std::min<uint64_t>(scratch / (npix * sizeof(float4)), (1ull << 30) / npix));
    spp_pass = std::min<uint64_t>(spp_pass, (uint64_t)p->spp);
    if (mode == 2 && spp_pass < (uint64_t)p->spp)
        return fail(PT_ERR_UNSUPPORTED, "pt_render_accumulate: spp of one call must fit the scratch budget (single pass)");
    // allocation failure (another handle took the memory meanwhile): halve the samples per pass and retry
    int rc;
    while ((rc = slot.samples.ensure(npix * spp_pass))) {
        if (spp_pass == 1 || mode == 2) return rc;
        (void)hipGetLastError();
        spp_pass = (spp_pass + 1) / 2;
    }
    const int n_pass = (int)(((uint64_t)p->spp + spp_pass - 1) / spp_pass);
    if (mode == 2 && n_pass > 1)
        return fail(PT_ERR_UNSUPPORTED, "pt_render_accumulate: spp of one call must fit the scratch budget (single pass)");
    if (n_pass > 1 && !adaptive && (rc = S->accum.ensure(npix * 3))) return rc;
    *spp_pass_out = spp_pass;
    *n_pass_out = n_pass;
    return PT_OK;
}

// Resident blocks per CU of a kernel with its LDS plan: the launch configuration of the last kernel used is kept (occupancy
// query and attribute call are not free per frame).
int launch_occupancy(pt_scene* S, const void* fn, int block_threads, uint32_t lds, int* occ) {
    if (S->cfg_fn != fn || S->cfg_lds != lds) {
        if (lds > 64 * 1024)
            HIP_TRY(hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
        int q = 0;
        HIP_TRY(hipOccupancyMaxActiveBlocksPerMultiprocessor(&q, fn, block_threads, lds));
        S->cfg_fn = fn; S->cfg_lds = lds; S->cfg_occ = std::max(q, 1);
    }
    *occ = S->cfg_occ;
    return PT_OK;
}

// Blocks per CU a launch takes of the `occ` the occupancy query allows.
int launch_blocks_per_cu(const pt_scene* S, bool lds_scene, int occ, bool own_stream, int in_flight) {
    // scenes read from global memory: 6 blocks per CU (what 80 VGPRs allow) with a 26 KB stack + top-of-tree budget each.
    // With the internal tree's short stacks (its Strahler number, not its depth) the sixth block no longer costs cached nodes
    // worth having: bunny +0.6 %, buddha stand-in -1.1 %, dragon stand-in -7.6 % against 5 blocks of 31 KB
    // (profiles/r02_tune_round41_lds_budget.log, r02_tune_round42_blocks.log).  LDS-resident scenes take every block they can get.
    int bpc = S->opt_blocks_per_cu > 0 ? (int)S->opt_blocks_per_cu : (!lds_scene ? std::min(occ, 6) : occ);
    // Single-pass frames of a handle with more than one slot run on the slot's stream while an earlier frame is on the GPU
    // (pt_scene::FrameSlot).  Such a frame does not take every resident slot of the chip: the waves of a launch run dry
    // together, and while its blocks sit on their last few paths a successor that may only ENTER as they leave starts late.
    // With three slots a frame takes half of each CU — two frames are resident side by side, half a frame apart, the third
    // enters where the first leaves — with two slots all but one block per CU (cbox 2.55 ms per frame with full grids,
    // 2.50 with 5 + 1 of 6, 2.49 with 3 + 3 and three slots; bunny 4.64 / 4.53 / 4.39; profiles/r03_frames_in_flight.log).
    if (own_stream && S->opt_blocks_per_cu <= 0) bpc = std::max(1, in_flight >= 3 ? bpc / 2 : bpc - 1);
    return bpc;
}

// The slot's own stream and the event that marks the point of the call on the caller's stream, made on first use.
int slot_stream(pt_scene::FrameSlot& slot) {
    if (!slot.stream) {
        // A stream of the lowest priority: the runtime maps streams onto a few hardware queues PER PRIORITY (4 by default),
        // and two streams on one hardware queue run in order.  Among the application's own normal-priority streams the two
        // slot streams ended up sharing a queue with each other or with the caller's as often as not (one more stream in
        // the process: 2.70 ms per cbox frame with two slots against 2.69 with one; on queues of their own 2.53 —
        // profiles/r03_frames_in_flight.log).  Low rather than high: a frame waits for the caller's other GPU work (the
        // RCCL gather of the rank's rows, N > 1), not the other way round.  PT_SLOT_STREAM_PRIORITY=normal|high: A/B runs.
        const char* pr = std::getenv("PT_SLOT_STREAM_PRIORITY");
        const std::string want = pr ? pr : "low";
        int least = 0, greatest = 0;
        if (want != "normal" && hipDeviceGetStreamPriorityRange(&least, &greatest) == hipSuccess && least != greatest)
            HIP_TRY(hipStreamCreateWithPriority(&slot.stream, hipStreamNonBlocking, want == "high" ? greatest : least));
        else
            HIP_TRY(hipStreamCreateWithFlags(&slot.stream, hipStreamNonBlocking));
    }
    if (!slot.in_ev) HIP_TRY(hipEventCreateWithFlags(&slot.in_ev, hipEventDisableTiming));
    return PT_OK;
}

// The render arguments of a pass of sn samples from sample s0 on; feed_waves: the waves of the launch that draw from the work
// feed.  A pixel list is a frame of n rows of width 1 (RenderDev::list).
RenderDev pass_render_dev(const pt_scene* S, const pt_render_params* p, const RowSel& rows, const PixelList* pl, int s0, int sn,
                          uint64_t feed_waves) {
    const int vrows = pl ? (int)pl->n : rows.count, vwidth = pl ? 1 : p->width;
    const uint64_t npix = (uint64_t)vrows * (uint64_t)vwidth;
    RenderDev rd{};
    std::memcpy(rd.cam_origin, p->cam_origin, 12);
    std::memcpy(rd.cam_top_left, p->cam_top_left, 12);
    std::memcpy(rd.cam_horizontal, p->cam_horizontal, 12);
    std::memcpy(rd.cam_vertical, p->cam_vertical, 12);
    rd.width = vwidth; rd.height = p->height;
    rd.row_begin = rows.begin; rd.row_step = rows.step; rd.num_rows = vrows;
    rd.list = pl ? pl->list : nullptr;
    rd.img_width = p->width;
    rd.div_img_width = make_fastdiv((uint32_t)p->width);
    rd.spp_pass = sn;
    rd.sample_base = p->sample_offset + s0;
    rd.stream_stride = p->stream_stride > 0 ? p->stream_stride : p->spp;
    rd.seed = p->seed;
    rd.max_depth = p->max_depth > 0 ? p->max_depth : 50;
    rd.rr_depth = p->rr_depth >= 0 ? p->rr_depth : 5;
    rd.npix = (uint32_t)npix;
    rd.total_work = (uint32_t)(npix * (uint64_t)sn);
    rd.num_regions = S->opt_xcd_regions > 0 ? (int)std::min<int64_t>(S->opt_xcd_regions, 8) : 8;
    rd.rows_per_region = (vrows + rd.num_regions - 1) / rd.num_regions;
    rd.div_width = make_fastdiv((uint32_t)vwidth);
    rd.div_spp = make_fastdiv((uint32_t)sn);
    rd.row_major = S->opt_item_order == 1 ? 1 : 0;
    rd.div_npix_full = make_fastdiv((uint32_t)rd.rows_per_region * (uint32_t)vwidth);
    {   // the band that holds the remainder rows (all bands after it are empty)
        const int full = vrows / rd.rows_per_region, rest = vrows - full * rd.rows_per_region;
        rd.short_region = rest ? full : -1;
        rd.div_npix_last = make_fastdiv((uint32_t)std::max(rest, 1) * (uint32_t)vwidth);
    }
    // chunk: work items a wave reserves per atomic.  Big launches (a wave traces >= 2048 items): 128 — the waves of a
    // launch run dry within two paths' time of each other instead of four (cbox -1.9 %, bunny -0.9 % against 256; 64
    // buys nothing more and saturates the counters on cheap scenes: profiles/r02_tune_round36_*.log); mid-size
    // launches 256; small launches (interactive 1-2 spp frames) down to 64 so that the items are spread over all
    // resident waves instead of the first total/256 of them
    const uint64_t per_wave = rd.total_work / feed_waves;
    rd.chunk = per_wave >= 2048 ? 128u
             : per_wave >= 4 * kMaxChunk ? kMaxChunk : (uint32_t)std::max<uint64_t>(64, std::min<uint64_t>(kMaxChunk, (per_wave / 64) * 64));
    if (S->opt_chunk > 0) rd.chunk = (uint32_t)std::min<int64_t>(kMaxChunk, std::max<int64_t>(64, (S->opt_chunk / 64) * 64));
    return rd;
}

// The four events of pass ev_pass of a frame's timing record, created where the record does not hold them yet.
int pass_events(pt_scene::FrameRec& rec, size_t ev_pass) {
    if (rec.ev.size() > ev_pass) return PT_OK;
    pt_scene::PassEvents fresh{};
    hipEvent_t* const ev[4] = {&fresh.t0, &fresh.t1, &fresh.r0, &fresh.r1};
    for (int k = 0; k < 4; k++) {
        const hipError_t ee = hipEventCreate(ev[k]);
        if (ee == hipSuccess) continue;
        while (k-- > 0) (void)hipEventDestroy(*ev[k]);
        return fail(PT_ERR_DEVICE, std::string("hipEventCreate: ") + hipGetErrorString(ee));
    }
    rec.ev.push_back(fresh);
    return PT_OK;
}

// What resolve_kernel does with a pass: rmode 2 adds the pass's partial sum (progressive: every pass adds its own; first only
// if sample_offset == 0 and pass 0), 0 writes the mean after the last pass, 1 accumulates a pass before the last.
struct ResolveMode {
    int rmode, rfirst;
    float scale;
};
ResolveMode resolve_mode(int mode, const pt_render_params* p, bool first, bool last) {
    if (mode == 2) return {2, (first && p->sample_offset == 0) ? 1 : 0, 1.0f};
    if (last) return {0, first ? 1 : 0, 1.0f / (float)p->spp};
    return {1, first ? 1 : 0, 1.0f};
}

// mode: 0 = pt_render (fb = mean), 2 = pt_render_accumulate (accum (+)= sum); ad: a round of pt_render_adaptive (mode 0);
// pl: the pixels to trace in place of the selected rows (out_dev is then [n, 3]; n == 0: an empty frame, out_dev may be null)
int launch_render(pt_scene* S, const pt_render_params* p, float* out_dev, int mode, hipStream_t stream,
                  const AdaptiveRound* ad = nullptr, const PixelList* pl = nullptr) {
    RowSel rows;
    int rc = check_render_args(S, p, out_dev, pl, &rows);
    if (rc) return rc;
    DeviceGuard guard;
    { int grc = guard.enter(S->device); if (grc) return grc; }
    const bool cont = ad && ad->round > 0;
    OpenFrame f;
    if ((rc = open_frame(S, stream, cont, &f))) return rc;
    pt_scene::FrameSlot& slot = *f.slot;
    if (rows.count == 0 || (pl && pl->n == 0)) return empty_frame(S, slot, stream);

    const bool listed = pl != nullptr;
    const uint64_t npix = listed ? (uint64_t)pl->n : (uint64_t)rows.count * (uint64_t)p->width;
    uint64_t spp_pass;
    int n_pass;
    if ((rc = plan_passes(S, p, mode, ad != nullptr, slot, npix, &spp_pass, &n_pass))) return rc;

    const int traversal = p->traversal == PT_TRAVERSAL_DEFAULT ? PT_TRAVERSAL_EXACT : p->traversal;
    if (traversal != PT_TRAVERSAL_EXACT && traversal != PT_TRAVERSAL_PRUNED) return fail(PT_ERR_INVALID_ARG, "unknown traversal mode");
    if (p->flags & ~PT_RENDER_NEE) return fail(PT_ERR_INVALID_ARG, "unknown bits in pt_render_params.flags");
    TraceChoice c;
    LdsPlan lp;
    QParams qp{};
    if ((rc = choose_trace(S, traversal, (p->flags & PT_RENDER_NEE) != 0, listed, &c)) || (rc = plan_trace(S, c, &lp, &qp))) return rc;
    const TraceEntry e = find_trace(c);
    if (!e.fn) return fail(PT_ERR_INVALID_ARG, "no kernel variant compiled for these v2_thresh / v2_inner options");
    int occ;
    if ((rc = launch_occupancy(S, e.fn, c.block_threads, lp.total, &occ))) return rc;
    // (a pixel list stays on the caller's stream: its trace kernel reads the caller's memory)
    const bool own_stream = !ad && !listed && f.in_flight > 1 && n_pass == 1 && f.prev_busy;
    const int bpc = launch_blocks_per_cu(S, c.lds_scene(), occ, own_stream, f.in_flight);
    S->info_kernel = c.family;
    S->info_trace_variant = e.variant;
    S->info_path_bank = e.bank;
    S->info_reg_stack = e.reg;
    S->info_leaf_sweep = c.sweep ? 1 : 0;
    S->info_occupancy = occ;
    S->info_blocks_per_cu = bpc;
    S->info_lds_bytes = lp.total;
    S->info_lds_scene = c.lds_scene();

    // one global-memory stack column per lane of a grid that reruns segments in reference order (rare: latency does not matter).
    // Sized from the grid, not from an assumed blocks-per-CU: `blocks_per_cu` is a caller's option and the kernel indexes the
    // buffer by blockIdx (pt_kernels.h: redo_stk).
    const auto redo_words = [&](int grid) { return (size_t)grid * (size_t)c.redo_lanes * (size_t)S->tree[0].stack_cap; };
    // the LARGEST grid this call launches: pass 0 traces the most samples
    if (c.which == 1 && (rc = slot.redo_stack.ensure(redo_words(launch_grid(S->num_cus, bpc, npix * spp_pass, c.block_threads))))) return rc;
    select_tree(S, c.which, c.which == 1);
    hipStream_t tstream = stream;
    if (own_stream) {
        if ((rc = slot_stream(slot))) return rc;
        tstream = slot.stream;
        HIP_TRY(hipEventRecord(slot.in_ev, stream));
    }
    if (slot.used && slot.free_stream != tstream) HIP_TRY(hipStreamWaitEvent(tstream, slot.free_ev, 0));   // the resolve that last read this slot's samples
    // one memset per frame: work counters + the 64 counter slots (+ timeline / histograms when a STATS kernel will run)
    // (a later adaptive round clears the work counters only: the frame's statistics run on over all its rounds)
    HIP_TRY(hipMemsetAsync(slot.ctl.p, 0, (kWorkWords + (cont ? 0 : S->opt_stats ? kNumCounters : kTimelineBase)) * sizeof(unsigned long long), tstream));
    for (int pass = 0; pass < n_pass; pass++) {
        const int s0 = pass * (int)spp_pass;
        const int sn = std::min<int>((int)spp_pass, p->spp - s0);
        const int grid = launch_grid(S->num_cus, bpc, npix * (uint64_t)sn, c.block_threads);
        if (c.which == 1 && redo_words(grid) > slot.redo_stack.n)
            return fail(PT_ERR_DEVICE, "internal error: rerun stacks smaller than the grid");
        S->info_grid = grid;
        const RenderDev rd = pass_render_dev(S, p, rows, pl, s0, sn, (uint64_t)grid * (uint64_t)c.feed_waves);

        const size_t ev_pass = f.pass_base + (size_t)pass;
        if (f.timing && (rc = pass_events(*f.rec, ev_pass))) return rc;
        const pt_scene::PassEvents pe = f.timing ? f.rec->ev[ev_pass] : pt_scene::PassEvents{};
        if (pass > 0) HIP_TRY(hipMemsetAsync(slot.ctl.p, 0, kWorkBytes, tstream));
        if (f.timing) HIP_TRY(hipEventRecord(pe.t0, tstream));
        launch_trace(S, c, e, grid, tstream, rd, lp, qp, slot.samples.p);
        HIP_TRY(hipGetLastError());
        if (f.timing) HIP_TRY(hipEventRecord(pe.t1, tstream));
        if (own_stream) HIP_TRY(hipStreamWaitEvent(tstream, slot.in_ev, 0));   // the resolve writes the caller's buffer
        if (f.timing) HIP_TRY(hipEventRecord(pe.r0, tstream));

        const bool first = pass == 0, last = pass == n_pass - 1;
        const unsigned rblocks = (unsigned)((npix + 255) / 256);
        if (ad) {
            AdaptiveArgs aa = ad->args;
            aa.n = (uint32_t)npix;
            aa.spp_pass = sn;
            aa.first = ad->round == 0 && first;
            aa.check = last;
            hipLaunchKernelGGL(adaptive_resolve_kernel, dim3(rblocks), dim3(256), 0, tstream, slot.samples.p, aa);
        } else {
            const ResolveMode r = resolve_mode(mode, p, first, last);
            hipLaunchKernelGGL(resolve_kernel, dim3(rblocks), dim3(256), 0, tstream, slot.samples.p, mode == 2 ? out_dev : S->accum.p,
                               out_dev, (uint32_t)npix, sn, r.rmode, r.rfirst, r.scale);
        }
        HIP_TRY(hipGetLastError());
        if (f.timing) HIP_TRY(hipEventRecord(pe.r1, tstream));
        HIP_TRY(hipEventRecord(slot.free_ev, tstream));
        slot.used = true; slot.free_stream = tstream;
        if (own_stream) HIP_TRY(hipStreamWaitEvent(stream, slot.free_ev, 0));
        S->info_passes++;
        if (f.timing) f.rec->passes = ev_pass + 1;
    }
    S->have_timing = f.timing;
    return PT_OK;
}

// The frame's counters, summed over the counter slots, once its stream has drained; zeros where the handle has no control block
// yet.  Enters the handle's device under the caller's guard.
int synced_slot_sums(pt_scene* S, DeviceGuard& guard, unsigned long long* c) {
    { int grc = guard.enter(S->device); if (grc) return grc; }
    HIP_TRY(hipStreamSynchronize(S->last_stream));
    std::fill(c, c + kSlotStride, 0ull);
    return S->cur().ctl.p ? read_slot_sums(S, c) : PT_OK;
}

// trace_kernel_q bounds every wait on its rings; a wait that ran into its bound leaves a mark in counter slot 15 and an
// invalid frame behind.  c: the frame's slot sums.
int schedule_error(const pt_scene* S, const unsigned long long* c) {
    if (S->info_kernel != 3 || !c[15]) return PT_OK;
    return fail(PT_ERR_DEVICE, "trace_kernel_q: schedule error, frame invalid (bits " + std::to_string(c[15]) + ": 1 bounded wait ran out, 2 ring entry corrupted, 4 impossible path state)");
}
// (The stream has been synchronised.)
int check_schedule_error(const pt_scene* S) {
    if (S->info_kernel != 3 || !S->cur().ctl.p) return PT_OK;
    unsigned long long c[kSlotStride];
    int rc = read_slot_sums(S, c);
    return rc ? rc : schedule_error(S, c);
}

// HIP-event times of one recorded render call, summed over its sample passes (the events must have completed).
int frame_times(const pt_scene::FrameRec& f, double* kernel_ms, double* resolve_ms) {
    double t = 0, r = 0;
    for (size_t k = 0; k < f.passes; k++) {
        float ms = 0;
        HIP_TRY(hipEventElapsedTime(&ms, f.ev[k].t0, f.ev[k].t1));
        t += ms;
        HIP_TRY(hipEventElapsedTime(&ms, f.ev[k].r0, f.ev[k].r1));
        r += ms;
    }
    *kernel_ms = t;
    *resolve_ms = r;
    return PT_OK;
}


// The staging buffers of a geometry change: new records and vertex normals, the buffer the live records retire into, the status word.
int ensure_staging(pt_scene* S) {
    const size_t N = (size_t)S->dev.num_prims;
    int rc;
    if ((rc = S->st_prims.ensure(N)) || (rc = S->prev_prims.ensure(N)) || (rc = S->st_normals.ensure(N)) || (rc = S->st_status.ensure(1)))
        return rc;
    return PT_OK;
}

// ---- tree-cost telemetry (pt_tree_cost.hip) ---------------------------------------------------------------------------------
int ensure_cost(pt_scene* S) {
    int rc;
    const size_t need = std::max(ptc::partials_needed(S->tree[0].num_nodes), ptc::partials_needed(S->tree[1].num_nodes));
    if ((rc = S->cost_partials.ensure(need)) || (rc = S->cost_dev.ensure(4))) return rc;
    if (!S->cost_host) HIP_TRY(hipHostMalloc(reinterpret_cast<void**>(&S->cost_host), 4 * sizeof(double), hipHostMallocDefault));
    return PT_OK;
}
// T's cost into cost_dev[slot] and from there to cost_host[slot], all on the default stream; read once that has synchronised
int enqueue_cost(pt_scene* S, const pt_scene::Tree& T, int slot) {
    int rc;
    if ((rc = ptc::tree_cost(T.nodes.p, T.num_nodes, S->cost_partials.p, S->cost_dev.p + slot))) return rc;
    HIP_TRY(hipMemcpyAsync(S->cost_host + slot, S->cost_dev.p + slot, sizeof(double), hipMemcpyDeviceToHost, nullptr));
    return PT_OK;
}
// after the synchronise that closes the call: what adopt_staged enqueued
void collect_costs(pt_scene* S) {
    for (int t = 0; t < 2; t++) {
        if (S->cost_pending_ref[t]) { S->cost_ref[t] = S->cost_host[t]; S->cost_have_ref[t] = true; }
        if (S->cost_pending_now[t]) S->cost_now[t] = S->cost_host[2 + t];
        S->cost_pending_ref[t] = S->cost_pending_now[t] = false;
    }
}
int64_t cost_permille(const pt_scene* S, int t) {
    if (!S->cost_have_ref[t] || !(S->cost_ref[t] > 0.0) || !(S->cost_now[t] > 0.0)) return 1000;
    return (int64_t)(1000.0 * S->cost_now[t] / S->cost_ref[t] + 0.5);
}

// What pt_scene_update and pt_scene_transform do once new records stand in st_prims / st_normals: the refit plans where none
// exist yet, leaf boxes and the status read-back, both trees refitted, and only then the handle changes — the three record
// buffers rotate (staging -> current -> previous) and the box sweep is dropped.  `who` heads the messages.  *us_plan: wall
// microseconds of the plan build (left alone where none was due); *us_refit: of everything after it.
int adopt_staged(pt_scene* S, const char* who, bool tri_only, int64_t* us_plan, int64_t* us_refit) {
    using clk = std::chrono::steady_clock;
    auto us_since = [](clk::time_point t0) { return (int64_t)std::chrono::duration_cast<std::chrono::microseconds>(clk::now() - t0).count(); };
    const int N = S->dev.num_prims;
    int rc;
    clk::time_point t_stage = clk::now();
    const int n_trees = N > 1 ? (S->have_fast ? 2 : 1) : 0;   // one shape: a dummy node, the root is never box-tested
    bool whole = true, planned = false;
    for (int t = 0; t < n_trees; t++) {
        ptf::Plan& pl = S->refit_plan[t];
        if (!pl.built) {
            if ((rc = ptf::plan_build(S->tree[t].nodes.p, S->tree[t].num_nodes, N, &pl))) return rc;
            planned = true;
        }
        whole = whole && pl.whole_tree;
        // octant tables are made by the single-workgroup launch alone; they exist only for trees far smaller than its reach
        if (S->tree[t].have_oct && !pl.whole_tree) return fail(PT_ERR_UNSUPPORTED, std::string(who) + ": octant tables on a tree of wide levels");
    }
    if (planned) { *us_plan = std::max<int64_t>(us_since(t_stage), 1); t_stage = clk::now(); }
    const bool costs = S->cost_on() && n_trees > 0;
    for (int t = 0; t < 2; t++) S->cost_pending_ref[t] = S->cost_pending_now[t] = false;
    if (costs) {
        // the reference cost of a tree that has none yet: from the boxes as they stand, before this refit writes them
        if ((rc = ensure_cost(S))) return rc;
        for (int t = 0; t < n_trees; t++)
            if (!S->cost_have_ref[t]) {
                if ((rc = enqueue_cost(S, S->tree[t], t))) return rc;
                S->cost_pending_ref[t] = true;
            }
    }
    HIP_TRY(hipMemsetAsync(S->st_status.p, 0, sizeof(unsigned int), nullptr));
    unsigned int bad = 0;
    if (!whole || n_trees == 0) {
        // the leaf boxes, checked before any node array is written (a tree done by one launch checks for itself)
        if ((rc = S->st_boxes.ensure((size_t)N * 6)) || (rc = ptf::leaf_boxes(S->st_prims.p, N, S->st_boxes.p, S->st_status.p))) return rc;
        HIP_TRY(hipMemcpy(&bad, S->st_status.p, sizeof bad, hipMemcpyDeviceToHost));
    }
    for (int t = 0; t < n_trees && !bad; t++) {
        pt_scene::Tree& T = S->tree[t];
        if ((rc = ptf::refit_tree(S->refit_plan[t], T.nodes.p, T.have_oct ? T.nodes_oct.p : nullptr, T.num_nodes, S->st_prims.p,
                                  whole ? nullptr : S->st_boxes.p, N, S->st_status.p)))
            return rc;
    }
    if (whole && n_trees) HIP_TRY(hipMemcpy(&bad, S->st_status.p, sizeof bad, hipMemcpyDeviceToHost));
    if (bad) return fail(PT_ERR_UNSUPPORTED, std::string(who) + ": a new coordinate, radius or leaf box is not finite");
    // behind the refit on its stream; the caller reads it after the synchronise that closes the call (collect_costs).  The
    // trees are written: a launch that fails here costs the measurement, not the update.
    for (int t = 0; costs && t < n_trees; t++) S->cost_pending_now[t] = enqueue_cost(S, S->tree[t], 2 + t) == PT_OK;
    std::swap(S->prev_prims.p, S->st_prims.p); std::swap(S->prev_prims.n, S->st_prims.n);   // the new records, for a moment
    std::swap(S->prims.p, S->prev_prims.p); std::swap(S->prims.n, S->prev_prims.n);         // current -> previous, new -> current
    S->have_prev = true;
    std::swap(S->normals.p, S->st_normals.p); std::swap(S->normals.n, S->st_normals.n);
    S->dev.prims = S->prims.p; S->dev.normals = S->normals.p;
    S->tri_only = tri_only;
    S->sweep_groups = 0; S->sweep.count = 0;     // leaf boxes that were equal need not be any more: back to the tree
    S->sweep_tab.release();                      // (no frame is in flight: the update synchronised before it wrote)
    *us_refit = us_since(t_stage);
    return PT_OK;
}

// pt_scene_rebuild (include/pt_api.h) between the two synchronises: the caller has made the device current and quiet, and
// synchronises again before a frame may start.  Everything is made in buffers of its own — leaf boxes out of tree[0], the
// candidate by pt_scene_create's internal-tree stage, its refit plan, its sweep tables — and only then does the handle change,
// by steps that cannot fail.  tree[0], the tie tables and every record set are read, never written.
int rebuild_scene(pt_scene* S) {
    using clk = std::chrono::steady_clock;
    auto us_since = [](clk::time_point t0) { return (int64_t)std::chrono::duration_cast<std::chrono::microseconds>(clk::now() - t0).count(); };
    if (!S->have_fast)
        return fail(PT_ERR_UNSUPPORTED, std::string("pt_scene_rebuild: the handle holds no tie tables, pt_scene_create kept no internal tree: ") +
                                            (S->no_fast_why[0] ? S->no_fast_why : "none was built"));
    const int N = S->dev.num_prims;
    const pt_scene::Tree& T0 = S->tree[0];
    const clk::time_point t_all = clk::now();
    clk::time_point t_stage = t_all;
    int64_t us[4] = {0, 0, 0, 0};
    int rc;
    // ---- leaf boxes: what the caller's tree holds (the caller's own before a geometry update, the exact ones after)
    DevBuf<float> boxes_dev;
    if ((rc = boxes_dev.ensure((size_t)N * 6)) || (rc = ptf::tree_leaf_boxes(T0.nodes.p, T0.num_nodes, N, boxes_dev.p))) return rc;
    // ---- build: create's branches
    pt_scene::Tree cand;
    TreeHost fast;
    auto built = [&] { us[1] = us_since(t_stage); t_stage = clk::now(); };
    bool on_device = N >= kDeviceSweepMin && !host_sweep_forced() && internal_tree_device(boxes_dev.p, N, cand, built);
    if (!on_device) {
        std::vector<float> leaf_boxes((size_t)N * 6);
        HIP_TRY(hipMemcpy(leaf_boxes.data(), boxes_dev.p, leaf_boxes.size() * sizeof(float), hipMemcpyDeviceToHost));
        t_stage = t_all;                              // stage 1 runs from the start of the call, whichever builder ends it
        if (!internal_tree_host(leaf_boxes, N, fast, built))
            return fail(PT_ERR_UNSUPPORTED, "pt_scene_rebuild: no internal tree could be built of the leaf boxes (not finite, or they no longer nest)");
        if ((rc = upload_tree(cand, fast))) return rc;
    }
    boxes_dev.release();
    // ---- probe: create's rays and create's rule, the caller's tree as it stands against the candidate.  (As at create: no tie
    // tables in view, the probe counts box tests.)
    SceneDev d0 = S->dev, d1 = S->dev;
    tree_view(S, d0, 0, false);
    tree_view(S, d1, cand, 1, false);
    for (SceneDev* dv : {&d0, &d1}) { dv->ref_path = nullptr; dv->ref_anc = nullptr; dv->ref_levels = 0; dv->redo_stack = nullptr; }
    unsigned long long v[2] = {0, 0};
    if ((rc = probe_trees(d0, d1, v))) return rc;
    const bool adopt = probe_wins(v);
    us[2] = us_since(t_stage); t_stage = clk::now();
    // ---- what goes with an adopted tree: its refit plan where the handle has refitted before (the next update does not pay for
    // it), the box sweep of a small scene under create's admission rules, its cost where telemetry is on
    ptf::Plan plan;
    SweepTable sweep{};
    int sweep_groups = 0;
    DevBuf<unsigned char> sweep_tab;
    double cost = 0.0;
    if (adopt) {
        if (S->refit_plan[1].built && (rc = ptf::plan_build(cand.nodes.p, cand.num_nodes, N, &plan))) return rc;
        struct PlanGuard { ptf::Plan* p; ~PlanGuard() { if (p) ptf::plan_release(p); } } plan_guard{&plan};
        if (!on_device && N <= kSweepMaxPrims) {
            std::vector<DPrim> prims((size_t)N);
            HIP_TRY(hipMemcpy(prims.data(), S->prims.p, prims.size() * sizeof(DPrim), hipMemcpyDeviceToHost));
            if ((rc = make_sweep_tables(fast, prims.data(), N, sweep, sweep_groups, sweep_tab))) return rc;
        }
        if (S->cost_on()) {
            if ((rc = ensure_cost(S)) || (rc = enqueue_cost(S, cand, 3))) return rc;
            HIP_TRY(hipStreamSynchronize(nullptr));
            cost = S->cost_host[3];
        }
        // ---- adoption
        pt_scene::Tree& T1 = S->tree[1];
        std::swap(T1.nodes.p, cand.nodes.p); std::swap(T1.nodes.n, cand.nodes.n);
        std::swap(T1.nodes_oct.p, cand.nodes_oct.p); std::swap(T1.nodes_oct.n, cand.nodes_oct.n);
        T1.have_oct = cand.have_oct; T1.num_nodes = cand.num_nodes; T1.root_ref = cand.root_ref; T1.stack_cap = cand.stack_cap;
        T1.top_avail = cand.top_avail; T1.depth = cand.depth;
        S->have_fast = true;
        S->fast_is_callers_topology = false;
        S->fast_cost_permille = probe_permille(v);
        S->sweep_on_device = on_device ? 1 : 0;
        std::swap(S->refit_plan[1], plan);            // the old plan goes with the old tree, once the call is timed
        plan_guard.p = &plan;
        S->sweep = sweep;
        S->sweep_groups = sweep_groups;
        std::swap(S->sweep_tab.p, sweep_tab.p); std::swap(S->sweep_tab.n, sweep_tab.n);
        S->cfg_fn = nullptr;                          // stack and LDS needs follow the tree: the next launch asks again
        S->q_cfg_fn = nullptr;
        if (S->cost_on()) { S->cost_ref[1] = S->cost_now[1] = cost; S->cost_have_ref[1] = true; }
    } else if (S->cost_have_ref[1] && S->cost_now[1] > 0.0) {
        S->cost_ref[1] = S->cost_now[1];              // no better tree to be had of these boxes: a policy waits for the next drift
    }
    us[3] = us_since(t_stage);
    us[0] = us_since(t_all);
    select_tree(S, 0);
    S->rebuilds++;
    S->rebuild_adopted = adopt ? 1 : 0;
    S->rebuild_cost_permille = probe_permille(v);
    std::copy(us, us + 4, S->rebuild_us);
    return PT_OK;
}

// The policy of option rebuild_at_permille, inside a geometry update or transform that has refitted: the internal tree's cost
// is awaited and compared, and the rebuild runs before the call's closing synchronise.  A rebuild that fails leaves the refitted
// tree in place and does not fail the call.
void rebuild_by_policy(pt_scene* S) {
    if (S->opt_rebuild_at <= 0 || !S->have_fast || !S->cost_pending_now[1]) return;
    if (hipStreamSynchronize(nullptr) != hipSuccess) return;
    collect_costs(S);
    if (cost_permille(S, 1) < S->opt_rebuild_at) return;
    if (rebuild_scene(S) == PT_OK) S->rebuilds_auto++;
}

// pt_scene_update (include/pt_api.h).  Order of events: everything that can be refused is made and checked first — argument
// counts and the desc on the host, primitive records and leaf boxes in staging memory on the device — and only then does the
// handle change: node arrays written, record buffers traded, shading tables overwritten.
int update_scene(pt_scene* S, const pt_scene_desc* d, int flags) {
    using clk = std::chrono::steady_clock;
    auto us_since = [](clk::time_point t0) { return (int64_t)std::chrono::duration_cast<std::chrono::microseconds>(clk::now() - t0).count(); };
    const bool geometry = (flags & PT_UPDATE_GEOMETRY) != 0, shading = (flags & PT_UPDATE_SHADING) != 0;
    const int N = S->dev.num_prims;
    if (geometry && d->num_shapes != N) return fail(PT_ERR_INVALID_ARG, "pt_scene_update: num_shapes differs from pt_scene_create's");
    if (shading && d->num_materials != S->dev.num_materials) return fail(PT_ERR_INVALID_ARG, "pt_scene_update: num_materials differs from pt_scene_create's");
    if (shading && d->num_lights != S->dev.num_emission) return fail(PT_ERR_INVALID_ARG, "pt_scene_update: num_lights differs from pt_scene_create's");
    int rc;
    std::vector<DMaterial> mats;
    std::vector<DEmission> emis;
    std::vector<DLight> dlights;
    if (shading) {
        if (!d->materials) return fail(PT_ERR_BAD_SCENE, "scene has no materials");
        if (d->num_lights > 0 && !d->lights) return fail(PT_ERR_BAD_SCENE, "bad light array");
        if ((rc = check_materials(d)) || (rc = pack_shading(d, N, mats, emis, dlights))) return rc;
    }
    if (geometry) {
        if (!d->shapes) return fail(PT_ERR_BAD_SCENE, "scene has no shapes");
        if (d->num_meshes < 0 || (d->num_meshes > 0 && !d->meshes)) return fail(PT_ERR_BAD_SCENE, "bad mesh array");
        if ((rc = check_meshes(d, S->dev.num_materials))) return rc;
    }
    DeviceGuard guard;
    { int grc = guard.enter(S->device); if (grc) return grc; }
    // frames of this handle that are still in flight, on the caller's streams and on the slots' own, read the scene
    HIP_TRY(hipDeviceSynchronize());
    const clk::time_point t_all = clk::now();
    int64_t us_records = 0, us_refit = 0, us_plan = 0;
    if (geometry) {
        const clk::time_point t_stage = clk::now();
        pt_scene_desc dg = *d;                                // material ids are checked against the handle's table
        dg.num_materials = S->dev.num_materials;
        int has_sphere = 0;
        if ((rc = ensure_staging(S))) return rc;
        if ((rc = ptp::prims_device(&dg, S->st_prims.p, S->st_normals.p, &has_sphere))) return rc;
        us_records = us_since(t_stage);
        if ((rc = adopt_staged(S, "pt_scene_update", !has_sphere, &us_plan, &us_refit))) return rc;
        S->have_rest = false;                        // the next pt_scene_transform starts from these records
        rebuild_by_policy(S);
    }
    if (shading) {
        const clk::time_point t_stage = clk::now();
        HIP_TRY(hipMemcpy(S->materials.p, mats.data(), mats.size() * sizeof(DMaterial), hipMemcpyHostToDevice));
        HIP_TRY(hipMemcpy(S->emission.p, emis.data(), emis.size() * sizeof(DEmission), hipMemcpyHostToDevice));
        HIP_TRY(hipMemcpy(S->lights.p, dlights.data(), dlights.size() * sizeof(DLight), hipMemcpyHostToDevice));
        S->dev.bg[0] = d->background[0]; S->dev.bg[1] = d->background[1]; S->dev.bg[2] = d->background[2];
        S->diffuse_only = all_diffuse(d);
        us_records += us_since(t_stage);
    }
    // the handle's own streams do not synchronise with the default stream the kernels above ran on
    HIP_TRY(hipDeviceSynchronize());
    collect_costs(S);
    select_tree(S, 0);
    S->updates++;
    S->update_us[0] = us_since(t_all); S->update_us[1] = us_records; S->update_us[2] = us_refit; S->update_us[3] = us_plan;
    return PT_OK;
}

// pt_scene_transform (include/pt_api.h).  pt_scene_update's order of events with another producer of the staged records: the
// matrices are checked and their entries made on the host, the rest records are snapshot where none are held, one kernel writes
// the staged records from them (pt_scene_transform.hip), and adopt_staged does the rest.
int transform_scene(pt_scene* S, const pt_transform* transforms, int32_t num_groups) {
    using clk = std::chrono::steady_clock;
    auto us_since = [](clk::time_point t0) { return (int64_t)std::chrono::duration_cast<std::chrono::microseconds>(clk::now() - t0).count(); };
    if (!S->have_groups) return fail(PT_ERR_INVALID_ARG, "pt_scene_transform: the scene has no group assignment (pt_scene_set_groups)");
    if (num_groups != S->num_groups) return fail(PT_ERR_INVALID_ARG, "pt_scene_transform: num_groups differs from pt_scene_set_groups'");
    if (num_groups > 0 && !transforms) return fail(PT_ERR_INVALID_ARG, "pt_scene_transform: null transforms");
    std::vector<ptx::Entry> tab((size_t)std::max(num_groups, 1));
    for (int32_t g = 0; g < num_groups; g++)
        if (const int bad = ptx::prepare(&transforms[g], &tab[(size_t)g]))
            return fail(ptx::refusal_status(bad), "pt_scene_transform: transforms[" + std::to_string(g) + "]: " + ptx::refusal(bad));
    const int N = S->dev.num_prims;
    DeviceGuard guard;
    { int grc = guard.enter(S->device); if (grc) return grc; }
    // frames of this handle that are still in flight, on the caller's streams and on the slots' own, read the scene
    HIP_TRY(hipDeviceSynchronize());
    const clk::time_point t_all = clk::now();
    int64_t us_records = 0, us_refit = 0, us_once = 0;
    int rc;
    if ((rc = ensure_staging(S)) || (rc = S->group_tab.ensure(tab.size() * ptx::kEntryFloats))) return rc;
    const bool snapshot = !S->have_rest;
    if (snapshot) {
        const clk::time_point t_stage = clk::now();
        if ((rc = S->rest_prims.ensure((size_t)N)) || (rc = S->rest_normals.ensure((size_t)N))) return rc;
        HIP_TRY(hipMemcpyAsync(S->rest_prims.p, S->prims.p, (size_t)N * sizeof(DPrim), hipMemcpyDeviceToDevice, nullptr));
        HIP_TRY(hipMemcpyAsync(S->rest_normals.p, S->normals.p, (size_t)N * sizeof(DNormals), hipMemcpyDeviceToDevice, nullptr));
        HIP_TRY(hipStreamSynchronize(nullptr));           // paid once: timed on its own
        us_once = std::max<int64_t>(us_since(t_stage), 1);
    }
    const clk::time_point t_stage = clk::now();
    HIP_TRY(hipMemcpy(S->group_tab.p, tab.data(), tab.size() * sizeof(ptx::Entry), hipMemcpyHostToDevice));
    if ((rc = ptx::transform_records(S->rest_prims.p, S->rest_normals.p, S->group_of.p, S->group_tab.p, N, S->st_prims.p, S->st_normals.p)))
        return rc;
    us_records = us_since(t_stage);
    int64_t us_plan = 0;
    if ((rc = adopt_staged(S, "pt_scene_transform", S->tri_only, &us_plan, &us_refit))) return rc;
    rebuild_by_policy(S);
    // the handle's own streams do not synchronise with the default stream the kernels above ran on
    HIP_TRY(hipDeviceSynchronize());
    collect_costs(S);
    S->have_rest = true;                                // (a refused call leaves the flag as it was: the next one copies again)
    select_tree(S, 0);
    S->transforms++;
    S->transform_us[0] = us_since(t_all); S->transform_us[1] = us_records; S->transform_us[2] = us_refit; S->transform_us[3] = us_once + us_plan;
    return PT_OK;
}

// What a guide pass (pt_render_aov, pt_render_guides, pt_render_guides_async) takes from pt_render_params: the camera, the frame
// and the row selection as the kernels read them, the traversal mode, the number of selected pixels.
int guide_render_dev(const pt_render_params* p, RenderDev* rd_out, int* traversal_out, uint64_t* npix_out) {
    if (p->width <= 0 || p->height <= 0) return fail(PT_ERR_INVALID_ARG, "width and height must be positive");
    const int traversal = p->traversal == PT_TRAVERSAL_DEFAULT ? PT_TRAVERSAL_EXACT : p->traversal;
    if (traversal != PT_TRAVERSAL_EXACT && traversal != PT_TRAVERSAL_PRUNED) return fail(PT_ERR_INVALID_ARG, "unknown traversal mode");
    RowSel rows;
    int rc = select_rows(p, &rows);
    if (rc) return rc;
    const uint64_t npix = (uint64_t)rows.count * (uint64_t)p->width;
    if (npix > (1ull << 30)) return fail(PT_ERR_INVALID_ARG, "more than 2^30 pixels per call");
    RenderDev rd{};
    std::memcpy(rd.cam_origin, p->cam_origin, sizeof rd.cam_origin);
    std::memcpy(rd.cam_top_left, p->cam_top_left, sizeof rd.cam_top_left);
    std::memcpy(rd.cam_horizontal, p->cam_horizontal, sizeof rd.cam_horizontal);
    std::memcpy(rd.cam_vertical, p->cam_vertical, sizeof rd.cam_vertical);
    rd.width = p->width; rd.height = p->height;
    rd.row_begin = rows.begin; rd.row_step = rows.step; rd.num_rows = rows.count;
    rd.npix = (uint32_t)npix;
    rd.div_width = make_fastdiv((uint32_t)p->width);
    *rd_out = rd;
    *traversal_out = traversal;
    *npix_out = npix;
    return PT_OK;
}

// ... and from pt_motion_params: the previous camera and the record set that holds the previous geometry.
void guide_motion_dev(const pt_scene* S, const pt_motion_params* m, MotionDev* mo) {
    std::memcpy(mo->cam.origin, m->prev_cam_origin, sizeof mo->cam.origin);
    std::memcpy(mo->cam.top_left, m->prev_cam_top_left, sizeof mo->cam.top_left);
    std::memcpy(mo->cam.horizontal, m->prev_cam_horizontal, sizeof mo->cam.horizontal);
    std::memcpy(mo->cam.vertical, m->prev_cam_vertical, sizeof mo->cam.vertical);
    // a handle that was never updated has previous = current
    mo->prev_prims = m->geometry == PT_MOTION_GEOMETRY_PREVIOUS && S->have_prev ? S->prev_prims.p : S->prims.p;
}

// pt_render_aov (m == nullptr) and pt_render_guides: one aov_kernel launch on the default stream, blocking.
int guide_pass(pt_scene* S, const pt_render_params* p, const pt_motion_params* m, const pt_guide_buffers& out, int on_device) {
    float *albedo = out.albedo, *normal = out.normal, *depth = out.depth;
    int32_t* prim = out.prim;
    float *motion = m ? out.motion : nullptr, *prev_depth = m ? out.prev_depth : nullptr;
    RenderDev rd{};
    int traversal = 0;
    uint64_t npix = 0;
    int rc = guide_render_dev(p, &rd, &traversal, &npix);
    if (rc) return rc;
    if (npix == 0 || (!albedo && !normal && !depth && !prim && !motion && !prev_depth)) return PT_OK;
    DeviceGuard guard;
    { int grc = guard.enter(S->device); if (grc) return grc; }
    // host outputs are staged in buffers of this call
    DevBuf<float> d_albedo, d_normal, d_depth, d_motion, d_prev_depth;
    DevBuf<int32_t> d_prim;
    float *o_albedo = albedo, *o_normal = normal, *o_depth = depth;
    int32_t* o_prim = prim;
    if (!on_device) {
        if ((albedo && (rc = d_albedo.ensure(npix * 3))) || (normal && (rc = d_normal.ensure(npix * 3))) ||
            (depth && (rc = d_depth.ensure(npix))) || (prim && (rc = d_prim.ensure(npix))) ||
            (motion && (rc = d_motion.ensure(npix * 2))) || (prev_depth && (rc = d_prev_depth.ensure(npix))))
            return rc;
        o_albedo = albedo ? d_albedo.p : nullptr; o_normal = normal ? d_normal.p : nullptr;
        o_depth = depth ? d_depth.p : nullptr; o_prim = prim ? d_prim.p : nullptr;
    }
    MotionDev mo{};
    if (m) {
        guide_motion_dev(S, m, &mo);
        mo.motion = on_device ? motion : (motion ? d_motion.p : nullptr);
        mo.prev_depth = on_device ? prev_depth : (prev_depth ? d_prev_depth.p : nullptr);
    }
    // the tree a render traverses (pt_debug_intersect's choice): the internal one with ties settled in the caller's visit order
    // and reference-order reruns where scene creation kept one and "fast_tree" is on, else the caller's
    const bool fast = S->have_fast && S->opt_fast_tree;
    select_tree(S, fast ? 1 : 0, fast);
    const int cap = fast && S->dev.redo_cap > S->dev.stack_cap ? S->dev.redo_cap : S->dev.stack_cap;
    const uint32_t lds = (uint32_t)(kBlock / 64) * (uint32_t)cap * 64u * 4u;
    const dim3 grid((unsigned)((npix + kBlock - 1) / kBlock));
    if (m && traversal == PT_TRAVERSAL_PRUNED)
        hipLaunchKernelGGL((aov_kernel<true, true>), grid, dim3(kBlock), lds, nullptr, S->dev, rd, o_albedo, o_normal, o_depth, o_prim, mo);
    else if (m)
        hipLaunchKernelGGL((aov_kernel<false, true>), grid, dim3(kBlock), lds, nullptr, S->dev, rd, o_albedo, o_normal, o_depth, o_prim, mo);
    else if (traversal == PT_TRAVERSAL_PRUNED)
        hipLaunchKernelGGL(aov_kernel<true>, grid, dim3(kBlock), lds, nullptr, S->dev, rd, o_albedo, o_normal, o_depth, o_prim);
    else
        hipLaunchKernelGGL(aov_kernel<false>, grid, dim3(kBlock), lds, nullptr, S->dev, rd, o_albedo, o_normal, o_depth, o_prim);
    HIP_TRY(hipGetLastError());
    if (on_device) {
        HIP_TRY(hipStreamSynchronize(nullptr));
        return PT_OK;
    }
    if (albedo) HIP_TRY(hipMemcpy(albedo, d_albedo.p, npix * 3 * sizeof(float), hipMemcpyDeviceToHost));
    if (normal) HIP_TRY(hipMemcpy(normal, d_normal.p, npix * 3 * sizeof(float), hipMemcpyDeviceToHost));
    if (depth) HIP_TRY(hipMemcpy(depth, d_depth.p, npix * sizeof(float), hipMemcpyDeviceToHost));
    if (prim) HIP_TRY(hipMemcpy(prim, d_prim.p, npix * sizeof(int32_t), hipMemcpyDeviceToHost));
    if (motion) HIP_TRY(hipMemcpy(motion, d_motion.p, npix * 2 * sizeof(float), hipMemcpyDeviceToHost));
    if (prev_depth) HIP_TRY(hipMemcpy(prev_depth, d_prev_depth.p, npix * sizeof(float), hipMemcpyDeviceToHost));
    return PT_OK;
}

// One launch of the lane-refilling query kernel (pt_query.h) on `stream`, without a host sync: the handle's tree choice in an
// argument block of its own (the handle's is not touched), the grid, the next work counter of the ring.
// src: ptq::kSrcClosest / kSrcAny / kSrcGuides; q.n > 0.
int query_launch(pt_scene* S, int src, bool prune, bool motion, ptq::QueryDev q, const RenderDev& rd, const MotionDev& mo, hipStream_t stream) {
    using namespace ptq;
    typedef void (*QueryFn)(SceneDev, QueryDev, RenderDev, MotionDev);
    const QueryFn fn = src == kSrcAny       ? query_kernel<kSrcAny, false>
                       : src == kSrcClosest ? (prune ? query_kernel<kSrcClosest, true> : query_kernel<kSrcClosest, false>)
                       : motion             ? (prune ? query_kernel<kSrcGuides, true, true> : query_kernel<kSrcGuides, false, true>)
                                            : (prune ? query_kernel<kSrcGuides, true, false> : query_kernel<kSrcGuides, false, false>);
    // the tree a render traverses (guide_pass has the rule)
    const bool fast = S->have_fast && S->opt_fast_tree;
    SceneDev dv = S->dev;
    tree_view(S, dv, fast ? 1 : 0, fast);
    const int cap = fast && dv.redo_cap > dv.stack_cap ? dv.redo_cap : dv.stack_cap;
    const uint32_t lds = (uint32_t)(kBlock / 64) * (uint32_t)cap * 64u * 4u;
    if (S->q_cfg_fn != (const void*)fn || S->q_cfg_lds != lds) {
        if (lds > 64 * 1024)
            HIP_TRY(hipFuncSetAttribute((const void*)fn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
        int occ = 0;
        HIP_TRY(hipOccupancyMaxActiveBlocksPerMultiprocessor(&occ, (const void*)fn, kBlock, lds));
        S->q_cfg_fn = (const void*)fn; S->q_cfg_lds = lds; S->q_cfg_occ = std::max(occ, 1);
    }
    // resident blocks x CUs, and no more blocks than give every lane a ray; "query_blocks" overrides both
    // (four blocks per CU where more are resident: 1,048,576 random rays on bunny 0.789 ms on 1,024 blocks against 0.875 on 2,048
    // and 1.134 on 512, profiles/query_time.log)
    const int bpc = S->opt_blocks_per_cu > 0 ? (int)S->opt_blocks_per_cu : std::min(S->q_cfg_occ, 4);
    const uint64_t by_work = ((uint64_t)q.n + (uint64_t)kBlock - 1) / (uint64_t)kBlock;
    const int grid = S->opt_query_blocks > 0 ? (int)S->opt_query_blocks
                                             : (int)std::max<uint64_t>(1, std::min<uint64_t>((uint64_t)S->num_cus * (uint64_t)bpc, by_work));
    int rc;
    if ((rc = S->q_counters.ensure((size_t)kQueryRing * kQueryCounterStride))) return rc;
    const size_t entry = (size_t)(S->q_seq % (uint64_t)kQueryRing);
    hipEvent_t& ev = S->q_event[entry];
    if (!ev) {
        HIP_TRY(hipEventCreateWithFlags(&ev, hipEventDisableTiming));
    } else if (hipEventQuery(ev) != hipSuccess) {        // the launch that used this counter last may still run
        (void)hipGetLastError();
        HIP_TRY(hipStreamWaitEvent(stream, ev, 0));
    }
    q.counter = S->q_counters.p + entry * kQueryCounterStride;
    q.refill = S->opt_query_refill > 0 ? (uint32_t)S->opt_query_refill : (uint32_t)kQueryRefill;
    // the waves' first ranges are their own (pt_query.h): the counter starts behind them, and a launch they cover never reads it
    const uint64_t first_ranges = (uint64_t)grid * (uint64_t)(kBlock / 64) * (uint64_t)kQueryChunk;
    if (first_ranges < (uint64_t)q.n)
        HIP_TRY(hipMemsetD32Async(reinterpret_cast<hipDeviceptr_t>(q.counter), (int)first_ranges, 1, stream));
    hipLaunchKernelGGL(fn, dim3((unsigned)grid), dim3(kBlock), lds, stream, dv, q, rd, mo);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipEventRecord(ev, stream));
    S->q_seq++;
    S->info_query_grid = grid;
    return PT_OK;
}

// pt_trace_rays behind its null-scene check.
int trace_rays_call(pt_scene* S, const float* rays, int32_t n, int mode, int traversal_in, float* out_tuv, int32_t* out_prim, int on_device,
                    void* hip_stream) {
    const char* fn = "pt_trace_rays: ";
    if (mode != PT_QUERY_CLOSEST && mode != PT_QUERY_ANY) return fail(PT_ERR_INVALID_ARG, std::string(fn) + "unknown mode");
    const int traversal = traversal_in == PT_TRAVERSAL_DEFAULT ? PT_TRAVERSAL_EXACT : traversal_in;
    if (traversal != PT_TRAVERSAL_EXACT && traversal != PT_TRAVERSAL_PRUNED) return fail(PT_ERR_INVALID_ARG, std::string(fn) + "unknown traversal");
    if (n < 0 || n > (1 << 30)) return fail(PT_ERR_INVALID_ARG, std::string(fn) + "n must be 0 .. 2^30");
    if (n == 0) return PT_OK;
    if (!rays) return fail(PT_ERR_INVALID_ARG, std::string(fn) + "null rays");
    if (!out_prim) return fail(PT_ERR_INVALID_ARG, std::string(fn) + "null out_prim");
    const bool closest = mode == PT_QUERY_CLOSEST;
    if (closest && !out_tuv) return fail(PT_ERR_INVALID_ARG, std::string(fn) + "null out_tuv");
    DeviceGuard guard;
    { int grc = guard.enter(S->device); if (grc) return grc; }
    ptq::QueryDev q{};
    q.n = (uint32_t)n;
    const bool prune = closest && traversal == PT_TRAVERSAL_PRUNED;      // a lane that stops at its first hit has nothing to prune by
    const int src = closest ? ptq::kSrcClosest : ptq::kSrcAny;
    if (on_device) {
        q.rays = rays; q.out_tuv = closest ? out_tuv : nullptr; q.out_prim = out_prim;
        return query_launch(S, src, prune, false, q, RenderDev{}, MotionDev{}, (hipStream_t)hip_stream);
    }
    int rc;
    if ((rc = S->q_rays.ensure((size_t)n * 8)) || (closest && (rc = S->q_tuv.ensure((size_t)n * 3))) || (rc = S->q_prim.ensure((size_t)n))) return rc;
    HIP_TRY(hipMemcpy(S->q_rays.p, rays, (size_t)n * 8 * sizeof(float), hipMemcpyHostToDevice));
    q.rays = S->q_rays.p; q.out_tuv = closest ? S->q_tuv.p : nullptr; q.out_prim = S->q_prim.p;
    if ((rc = query_launch(S, src, prune, false, q, RenderDev{}, MotionDev{}, nullptr))) return rc;
    if (closest) HIP_TRY(hipMemcpy(out_tuv, S->q_tuv.p, (size_t)n * 3 * sizeof(float), hipMemcpyDeviceToHost));
    HIP_TRY(hipMemcpy(out_prim, S->q_prim.p, (size_t)n * sizeof(int32_t), hipMemcpyDeviceToHost));
    return PT_OK;
}

// pt_render_guides_async behind its null checks: guide_pass's arguments and rules, the query kernel on the caller's stream.
int guides_async_call(pt_scene* S, const pt_render_params* p, const pt_motion_params* m, const pt_guide_buffers& out, void* hip_stream) {
    RenderDev rd{};
    int traversal = 0;
    uint64_t npix = 0;
    int rc = guide_render_dev(p, &rd, &traversal, &npix);
    if (rc) return rc;
    float *motion = m ? out.motion : nullptr, *prev_depth = m ? out.prev_depth : nullptr;
    if (npix == 0 || (!out.albedo && !out.normal && !out.depth && !out.prim && !motion && !prev_depth)) return PT_OK;
    DeviceGuard guard;
    { int grc = guard.enter(S->device); if (grc) return grc; }
    MotionDev mo{};
    if (m) {
        guide_motion_dev(S, m, &mo);
        mo.motion = motion;
        mo.prev_depth = prev_depth;
    }
    // Camera rays are coherent: the 64 pixels of a one-shot wave walk almost the same nodes and finish together, and the
    // refilling kernel measured slower on them at every scene and size tried.  So the automatic choice is
    // aov_kernel, on the caller's stream and on an argument block of this call; "query_guides" = 1 or an explicit "query_blocks"
    // takes the refilling kernel.
    const bool refill = S->opt_query_guides == 1 || (S->opt_query_guides == 0 && S->opt_query_blocks > 0);
    S->info_query_guides = refill ? 1 : 0;
    if (!refill) {
        const bool fast = S->have_fast && S->opt_fast_tree;
        SceneDev dv = S->dev;
        tree_view(S, dv, fast ? 1 : 0, fast);
        const int cap = fast && dv.redo_cap > dv.stack_cap ? dv.redo_cap : dv.stack_cap;
        const uint32_t lds = (uint32_t)(kBlock / 64) * (uint32_t)cap * 64u * 4u;
        const dim3 grid((unsigned)((npix + kBlock - 1) / kBlock));
        hipStream_t stream = (hipStream_t)hip_stream;
        if (m && traversal == PT_TRAVERSAL_PRUNED)
            hipLaunchKernelGGL((aov_kernel<true, true>), grid, dim3(kBlock), lds, stream, dv, rd, out.albedo, out.normal, out.depth, out.prim, mo);
        else if (m)
            hipLaunchKernelGGL((aov_kernel<false, true>), grid, dim3(kBlock), lds, stream, dv, rd, out.albedo, out.normal, out.depth, out.prim, mo);
        else if (traversal == PT_TRAVERSAL_PRUNED)
            hipLaunchKernelGGL((aov_kernel<true, false>), grid, dim3(kBlock), lds, stream, dv, rd, out.albedo, out.normal, out.depth, out.prim, mo);
        else
            hipLaunchKernelGGL((aov_kernel<false, false>), grid, dim3(kBlock), lds, stream, dv, rd, out.albedo, out.normal, out.depth, out.prim, mo);
        HIP_TRY(hipGetLastError());
        return PT_OK;
    }
    ptq::QueryDev q{};
    q.n = (uint32_t)npix;
    q.albedo = out.albedo; q.normal = out.normal; q.depth = out.depth; q.prim = out.prim;
    return query_launch(S, ptq::kSrcGuides, traversal == PT_TRAVERSAL_PRUNED, m != nullptr, q, rd, mo, (hipStream_t)hip_stream);
}

// Arguments of pt_temporal_accumulate, pt_temporal_accumulate_moments and their host twins: nulls, the forbidden aliases, the
// parameter ranges.  fn: the entry point's name for the message; moments: albedo and the moments planes are expected.
int temporal_args(const char* fn, bool moments, const pt_temporal_params* t, float albedo_floor, const pt_temporal_io* io,
                  ptt::Resolved* r, float* floor_out) {
    const std::string pre = std::string(fn) + ": ";
    if (!t) return fail(PT_ERR_INVALID_ARG, pre + "null pt_temporal_params");
    if (!io) return fail(PT_ERR_INVALID_ARG, pre + "null pt_temporal_io");
    if (!io->color || (moments && !io->albedo) || !io->normal || !io->motion || !io->prev_depth || !io->out_color || !io->out_len ||
        (moments && !io->out_moments))
        return fail(PT_ERR_INVALID_ARG, pre + (moments ? "null color, albedo, normal, motion, prev_depth, out_color, out_len or out_moments"
                                                       : "null color, normal, motion, prev_depth, out_color or out_len"));
    const int n_hist = (io->hist_color != nullptr) + (io->hist_normal != nullptr) + (io->hist_depth != nullptr) +
                       (io->hist_len != nullptr) + (moments && io->hist_moments != nullptr);
    if (n_hist != 0 && n_hist != (moments ? 5 : 4))
        return fail(PT_ERR_INVALID_ARG, pre + "hist_color, hist_normal, hist_depth, hist_len" + (moments ? ", hist_moments" : "") +
                                            " must be given together or all be null");
    if (n_hist && io->out_color == io->hist_color) return fail(PT_ERR_INVALID_ARG, pre + "out_color must not be hist_color (neighbours are gathered)");
    if (n_hist && io->out_len == io->hist_len) return fail(PT_ERR_INVALID_ARG, pre + "out_len must not be hist_len (neighbours are gathered)");
    if (moments && n_hist && io->out_moments == io->hist_moments)
        return fail(PT_ERR_INVALID_ARG, pre + "out_moments must not be hist_moments (neighbours are gathered)");
    if (const char* bad = ptt::resolve(t, r)) return fail(PT_ERR_INVALID_ARG, std::string("pt_temporal_params.") + bad + " out of range");
    if (albedo_floor != 0.0f && !(albedo_floor > 0.0f && albedo_floor <= 3.402823466e+38f))
        return fail(PT_ERR_INVALID_ARG, pre + "albedo_floor out of range");
    *floor_out = albedo_floor != 0.0f ? albedo_floor : 0.01f;
    return PT_OK;
}

// pt_temporal_accumulate's eleven pointers as the pt_temporal_io of the shared rule; the moments' three stay null
pt_temporal_io temporal_io(const float* color, const float* normal, const float* motion, const float* prev_depth,
                           const float* hist_color, const float* hist_normal, const float* hist_depth, const float* hist_len,
                           float* out_color, float* out_len) {
    return {color, nullptr, normal, motion, prev_depth, hist_color, hist_normal, hist_depth, hist_len, nullptr, out_color, out_len, nullptr};
}

// Arguments of pt_denoise_variance and its host twin.
int vdenoise_args(const pt_vdenoise_params* d, const ptdn::Frames& f, ptdn::Resolved* r) {
    if (!d) return fail(PT_ERR_INVALID_ARG, "pt_denoise_variance: null pt_vdenoise_params");
    if (!f.color || !f.albedo || !f.normal || !f.depth || !f.out) return fail(PT_ERR_INVALID_ARG, "pt_denoise_variance: null color, albedo, normal, depth or out");
    if (!f.moments) return fail(PT_ERR_INVALID_ARG, "pt_denoise_variance: null moments");
    if (!f.hist_len) return fail(PT_ERR_INVALID_ARG, "pt_denoise_variance: null hist_len");
    if (const char* bad = ptdn::vresolve(d, r)) return fail(PT_ERR_INVALID_ARG, std::string("pt_vdenoise_params.") + bad + " out of range");
    return PT_OK;
}

// Arguments of pt_denoise and its host twin.
int denoise_args(const pt_denoise_params* d, const ptdn::Frames& f, ptdn::Resolved* r) {
    if (!d || !f.color || !f.albedo || !f.normal || !f.depth || !f.out) return fail(PT_ERR_INVALID_ARG, "null argument");
    if (const char* bad = ptdn::resolve(d, r)) return fail(PT_ERR_INVALID_ARG, std::string("pt_denoise_params.") + bad + " out of range");
    return PT_OK;
}

// One plane of an image-space call: the slots of the call's pointer struct that hold it and its floats per pixel.  `in`: the
// kernels read it; `out`: they write it; both (pt_denoise's colour): the result goes over the input.  A plane may be absent:
// the caller's pointers in its slots are null (a history, the variance output) and stay null.
struct Plane {
    const float** in;
    float** out;
    int floats;
};

// The tail of the four image-space entry points, after their arguments are checked and the scene's device is current: run
// the kernels (`run(stream)`, a hipError_t) on the caller's pointers, or for a call that comes in host memory stage it through
// `staging`: one buffer of the sum of the planes, the inputs copied in plane by plane, the slots pointed at the device planes
// for `run` on the default stream, the outputs copied back.  A plane that a call does not have is 0 floats wide.
template <size_t N, class Run>
int run_staged(const char* fn, int on_device, void* hip_stream, DevBuf<float>& staging, size_t npix, const Plane (&planes)[N], Run run) {
    auto launch = [&](void* stream) {
        const hipError_t e = (hipError_t)run(stream);
        return e != hipSuccess ? fail(PT_ERR_DEVICE, std::string(fn) + ": " + hipGetErrorString(e)) : PT_OK;
    };
    if (on_device) return launch(hip_stream);
    size_t floats = 0;
    for (const Plane& pl : planes) floats += (size_t)pl.floats;
    int rc = staging.ensure(npix * floats);
    if (rc) return rc;
    float* host_out[N];
    float* dev = staging.p;
    for (size_t i = 0; i < N; i++) {
        const Plane& pl = planes[i];
        host_out[i] = pl.out ? *pl.out : nullptr;
        if (pl.in && *pl.in) {
            HIP_TRY(hipMemcpy(dev, *pl.in, npix * (size_t)pl.floats * sizeof(float), hipMemcpyHostToDevice));
            *pl.in = dev;
        }
        if (host_out[i]) *pl.out = dev;
        dev += npix * (size_t)pl.floats;
    }
    if ((rc = launch(nullptr))) return rc;
    for (size_t i = 0; i < N; i++)
        if (host_out[i]) HIP_TRY(hipMemcpy(host_out[i], *planes[i].out, npix * (size_t)planes[i].floats * sizeof(float), hipMemcpyDeviceToHost));
    return PT_OK;
}

// The lambda map of pt_temporal_accumulate_adaptive and its host twin, after temporal_args: the pointer, the stride, the tile grid.
int adaptive_args(const char* fn, const ptt::Resolved& r, const float* lambda, int32_t stride, ptt::Lambda* lam) {
    const std::string pre = std::string(fn) + ": ";
    if (!lambda) return fail(PT_ERR_INVALID_ARG, pre + "null lambda");
    if (stride < 0 || stride > 16) return fail(PT_ERR_INVALID_ARG, pre + "stride out of range");
    int32_t r0;
    *lam = ptt::Lambda{lambda, stride ? stride : 3, 0, 0};
    if (!ptg::tile_grid(r.width, r.height, lam->stride, &r0, &lam->tw, &lam->th))
        return fail(PT_ERR_INVALID_ARG, pre + "height: no sampled row (height <= stride / 2)");
    return PT_OK;
}

// pt_temporal_accumulate (moments = false), pt_temporal_accumulate_moments and, with a lambda map, pt_temporal_accumulate_adaptive
int temporal_call(const char* fn, bool moments, pt_scene* S, const pt_temporal_params* t, float albedo_floor, const pt_temporal_io* io_in,
                  int on_device, void* hip_stream, bool adaptive = false, const float* lambda = nullptr, int32_t stride = 0) {
    if (!S) return fail(PT_ERR_INVALID_ARG, std::string(fn) + ": null scene");
    ptt::Resolved r;
    float floor_v;
    int rc = temporal_args(fn, moments, t, albedo_floor, io_in, &r, &floor_v);
    if (rc) return rc;
    ptt::Lambda lam{};
    if (adaptive && (rc = adaptive_args(fn, r, lambda, stride, &lam))) return rc;
    DeviceGuard guard;
    { int grc = guard.enter(S->device); if (grc) return grc; }
    pt_temporal_io io = *io_in;
    const Plane planes[] = {{&io.color, nullptr, 3}, {&io.albedo, nullptr, moments ? 3 : 0}, {&io.normal, nullptr, 3},
                            {&io.motion, nullptr, 2}, {&io.prev_depth, nullptr, 1},
                            {&io.hist_color, nullptr, 3}, {&io.hist_normal, nullptr, 3}, {&io.hist_depth, nullptr, 1},
                            {&io.hist_len, nullptr, 1}, {&io.hist_moments, nullptr, moments ? 2 : 0},
                            {nullptr, &io.out_color, 3}, {nullptr, &io.out_len, 1}, {nullptr, &io.out_moments, moments ? 2 : 0}};
    // a staged adaptive call: the map rides behind the planes of the staging buffer (at most one float per pixel: a plane more)
    const Plane planes_lam[] = {planes[0], planes[1], planes[2], planes[3], planes[4], planes[5], planes[6], planes[7], planes[8],
                                planes[9], planes[10], planes[11], planes[12], {nullptr, nullptr, 1}};
    const size_t npix = (size_t)r.width * (size_t)r.height;
    if (adaptive && !on_device) {
        // no history: the map is never read, and need not be readable
        const bool read = io.hist_color != nullptr;
        size_t floats = 0;
        for (const Plane& pl : planes) floats += (size_t)pl.floats;
        return run_staged(fn, 0, hip_stream, S->tp_host, npix, planes_lam, [&](void* stream) {
            float* d_lam = S->tp_host.p + npix * floats;
            if (read) {
                const hipError_t e = hipMemcpy(d_lam, lam.map, (size_t)lam.tw * (size_t)lam.th * sizeof(float), hipMemcpyHostToDevice);
                if (e != hipSuccess) return (int)e;
            }
            lam.map = d_lam;
            return ptt::run_device(r, true, floor_v, io, &lam, stream);
        });
    }
    return run_staged(fn, on_device, hip_stream, S->tp_host, npix, planes,
                      [&](void* stream) { return ptt::run_device(r, moments, floor_v, io, adaptive ? &lam : nullptr, stream); });
}

// pt_temporal_gradient behind its argument checks: the record buffers, then the kernels; a call that comes in host memory is
// staged through one buffer of the handle (the two frames in, the map out) on the default stream.
int gradient_call(pt_scene* S, const ptg::Resolved& r, const float* prev_color, const float* resampled, float* lambda_out, int on_device,
                  void* hip_stream) {
    const char* fn = "pt_temporal_gradient";
    DeviceGuard guard;
    { int grc = guard.enter(S->device); if (grc) return grc; }
    const size_t ntiles = (size_t)r.tw * (size_t)r.th;
    int rc;
    if ((rc = S->gr_x[0].ensure(2 * ntiles)) || (rc = S->gr_x[1].ensure(2 * ntiles))) return rc;
    auto launch = [&](const float* a, const float* b, float* out, void* stream) {
        const hipError_t e = (hipError_t)ptg::run_device(r, a, b, out, S->gr_x[0].p, S->gr_x[1].p, stream);
        return e != hipSuccess ? fail(PT_ERR_DEVICE, std::string(fn) + ": " + hipGetErrorString(e)) : PT_OK;
    };
    if (on_device) return launch(prev_color, resampled, lambda_out, hip_stream);
    const size_t n_prev = (size_t)r.width * (size_t)r.height * 3, n_res = (size_t)r.width * (size_t)r.th * 3;
    if ((rc = S->gr_host.ensure(n_prev + n_res + ntiles))) return rc;
    float *d_prev = S->gr_host.p, *d_res = d_prev + n_prev, *d_lam = d_res + n_res;
    HIP_TRY(hipMemcpy(d_prev, prev_color, n_prev * sizeof(float), hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(d_res, resampled, n_res * sizeof(float), hipMemcpyHostToDevice));
    if ((rc = launch(d_prev, d_res, d_lam, nullptr))) return rc;
    HIP_TRY(hipMemcpy(lambda_out, d_lam, ntiles * sizeof(float), hipMemcpyDeviceToHost));
    return PT_OK;
}

// Arguments of pt_temporal_gradient and its host twin.
int gradient_args(const char* fn, const pt_gradient_params* g, const float* prev_color, const float* resampled, const float* lambda_out,
                  ptg::Resolved* r) {
    const std::string pre = std::string(fn) + ": ";
    if (!g) return fail(PT_ERR_INVALID_ARG, pre + "null pt_gradient_params");
    if (!prev_color) return fail(PT_ERR_INVALID_ARG, pre + "null prev_color");
    if (!resampled) return fail(PT_ERR_INVALID_ARG, pre + "null resampled");
    if (!lambda_out) return fail(PT_ERR_INVALID_ARG, pre + "null lambda_out");
    if (const char* bad = ptg::resolve(g, r)) return fail(PT_ERR_INVALID_ARG, std::string("pt_gradient_params.") + bad + " out of range");
    return PT_OK;
}

// Arguments of the sparse variant's four entry points: the struct, then the pointers in the order of the parameter list.
int sparse_args(const char* fn, const pt_gradient_params* g, std::initializer_list<std::pair<const char*, const void*>> ptrs, ptg::Resolved* r) {
    const std::string pre = std::string(fn) + ": ";
    if (!g) return fail(PT_ERR_INVALID_ARG, pre + "null pt_gradient_params");
    for (const auto& q : ptrs)
        if (!q.second) return fail(PT_ERR_INVALID_ARG, pre + "null " + q.first);
    if (const char* bad = ptg::resolve(g, r)) return fail(PT_ERR_INVALID_ARG, std::string("pt_gradient_params.") + bad + " out of range");
    return PT_OK;
}

// pt_gradient_pixels behind its argument checks: one kernel; a list that goes to host memory is made in the handle's staging
// buffer on the default stream and copied out.
int gradient_pixels_call(pt_scene* S, const ptg::Resolved& r, uint32_t seed, int32_t* pixels_out, int on_device, void* hip_stream) {
    const char* fn = "pt_gradient_pixels";
    DeviceGuard guard;
    { int grc = guard.enter(S->device); if (grc) return grc; }
    const size_t ntiles = (size_t)r.tw * (size_t)r.th;
    int rc;
    int32_t* d_out = pixels_out;
    if (!on_device) {
        if ((rc = S->px_list.ensure(ntiles))) return rc;
        d_out = S->px_list.p;
    }
    const hipError_t e = (hipError_t)ptg::pixels_device(r, seed, d_out, on_device ? hip_stream : nullptr);
    if (e != hipSuccess) return fail(PT_ERR_DEVICE, std::string(fn) + ": " + hipGetErrorString(e));
    if (!on_device) HIP_TRY(hipMemcpy(pixels_out, d_out, ntiles * sizeof(int32_t), hipMemcpyDeviceToHost));
    return PT_OK;
}

// pt_temporal_gradient_sparse behind its argument checks, as gradient_call: the staging buffer of a call in host memory holds
// the frame, the re-traced pixels, the list (4 bytes per entry, like a float) and the map.
int gradient_sparse_call(pt_scene* S, const ptg::Resolved& r, const float* prev_color, const int32_t* pixels, const float* resampled,
                         float* lambda_out, int on_device, void* hip_stream) {
    const char* fn = "pt_temporal_gradient_sparse";
    DeviceGuard guard;
    { int grc = guard.enter(S->device); if (grc) return grc; }
    const size_t ntiles = (size_t)r.tw * (size_t)r.th;
    int rc;
    if ((rc = S->gr_x[0].ensure(2 * ntiles)) || (rc = S->gr_x[1].ensure(2 * ntiles))) return rc;
    auto launch = [&](const float* a, const int32_t* px, const float* b, float* out, void* stream) {
        const hipError_t e = (hipError_t)ptg::run_device_sparse(r, a, px, b, out, S->gr_x[0].p, S->gr_x[1].p, stream);
        return e != hipSuccess ? fail(PT_ERR_DEVICE, std::string(fn) + ": " + hipGetErrorString(e)) : PT_OK;
    };
    if (on_device) return launch(prev_color, pixels, resampled, lambda_out, hip_stream);
    static_assert(sizeof(int32_t) == sizeof(float), "the list rides in the float staging buffer");
    const size_t n_prev = (size_t)r.width * (size_t)r.height * 3, n_res = ntiles * 3;
    if ((rc = S->gr_host.ensure(n_prev + n_res + 2 * ntiles))) return rc;
    float *d_prev = S->gr_host.p, *d_res = d_prev + n_prev, *d_lam = d_res + n_res;
    int32_t* d_px = reinterpret_cast<int32_t*>(d_lam + ntiles);
    HIP_TRY(hipMemcpy(d_prev, prev_color, n_prev * sizeof(float), hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(d_res, resampled, n_res * sizeof(float), hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(d_px, pixels, ntiles * sizeof(int32_t), hipMemcpyHostToDevice));
    if ((rc = launch(d_prev, d_px, d_res, d_lam, nullptr))) return rc;
    HIP_TRY(hipMemcpy(lambda_out, d_lam, ntiles * sizeof(float), hipMemcpyDeviceToHost));
    return PT_OK;
}

// pt_denoise and pt_denoise_variance behind their argument checks: the record buffers, then the kernels.  The frame is
// written over the colour plane of a staged call.
int denoise_call(const char* fn, pt_scene* S, const ptdn::Resolved& r, ptdn::Frames f, DevBuf<float4>& guide, DevBuf<float4> (&x)[2],
                 DevBuf<float>& staging, int on_device, void* hip_stream) {
    DeviceGuard guard;
    { int grc = guard.enter(S->device); if (grc) return grc; }
    const size_t npix = (size_t)r.width * (size_t)r.height;
    int rc;
    if ((rc = guide.ensure(npix)) || (rc = x[0].ensure(npix)) || (rc = x[1].ensure(npix))) return rc;
    const bool variance = r.mode == ptdn::Mode::Variance;
    const Plane planes[] = {{&f.color, &f.out, 3}, {&f.albedo, nullptr, 3}, {&f.normal, nullptr, 3}, {&f.depth, nullptr, 1},
                            {&f.moments, nullptr, variance ? 2 : 0}, {&f.hist_len, nullptr, variance ? 1 : 0},
                            {nullptr, &f.out_variance, variance ? 1 : 0}};
    return run_staged(fn, on_device, hip_stream, staging, npix, planes,
                      [&](void* stream) { return ptdn::run_device(r, f, guide.p, x[0].p, x[1].p, stream); });
}

// the host twins of pt_denoise and pt_denoise_variance behind their argument checks
int denoise_host_call(const char* fn, const ptdn::Resolved& r, const ptdn::Frames& f) {
    try {
        ptdn::run_host(r, f);
    } catch (const std::exception& e) {
        return fail(PT_ERR_DEVICE, std::string(fn) + ": " + e.what());
    }
    return PT_OK;
}

}  // namespace

// ------------------------------------------------------------------------------------------
// C ABI
// ------------------------------------------------------------------------------------------
extern "C" {

int pt_api_version(void) { return PT_API_VERSION; }
const char* pt_last_error(void) { return g_err.c_str(); }

int pt_scene_create(const pt_scene_desc* desc, pt_scene** out) {
    if (!out) return fail(PT_ERR_INVALID_ARG, "null output pointer");
    *out = nullptr;
    int ndev = 0;
    hipError_t e = hipGetDeviceCount(&ndev);
    if (e != hipSuccess || ndev <= 0) return fail(PT_ERR_NO_DEVICE, "no HIP device available: the path tracer has no CPU fallback");
    pt_scene* S = new pt_scene();
    auto bail = [&](int rc) { pt_scene_destroy(S); return rc; };
    if (hipGetDevice(&S->device) != hipSuccess) return bail(fail(PT_ERR_DEVICE, "hipGetDevice failed"));
    hipDeviceProp_t prop;
    if (hipGetDeviceProperties(&prop, S->device) != hipSuccess) return bail(fail(PT_ERR_DEVICE, "hipGetDeviceProperties failed"));
    S->num_cus = prop.multiProcessorCount;
    S->lds_per_block_max = prop.sharedMemPerBlock;
    int rc = validate_and_build(desc, S);
    if (rc) return bail(rc);
    *out = S;
    return PT_OK;
}

int pt_scene_destroy(pt_scene* S) {
    if (!S) return PT_OK;
    DeviceGuard guard;
    (void)guard.enter(S->device);
    if (S->last_stream || S->have_timing || S->q_seq) (void)hipDeviceSynchronize();
    S->drop_query();
    for (auto& T : S->tree) { T.nodes.release(); T.nodes_oct.release(); } S->drop_slots(); S->prims.release(); S->normals.release(); S->materials.release(); S->emission.release();
    S->lights.release(); S->sweep_tab.release(); S->accum.release(); S->fb_tmp.release();
    S->ad_sum.release(); S->ad_mom.release(); S->ad_list[0].release(); S->ad_list[1].release(); S->ad_count.release();
    S->ad_spp_tmp.release(); S->ad_err_tmp.release();
    S->dn_guide.release(); S->dn_x[0].release(); S->dn_x[1].release(); S->dn_host.release(); S->tp_host.release();
    S->vd_guide.release(); S->vd_x[0].release(); S->vd_x[1].release(); S->vd_host.release();
    S->gr_x[0].release(); S->gr_x[1].release(); S->gr_host.release(); S->px_list.release();
    S->st_prims.release(); S->prev_prims.release(); S->st_normals.release(); S->st_boxes.release(); S->st_status.release();
    S->group_of.release(); S->group_tab.release(); S->rest_prims.release(); S->rest_normals.release();
    for (auto& pl : S->refit_plan) ptf::plan_release(&pl);
    S->cost_partials.release(); S->cost_dev.release();
    if (S->cost_host) (void)hipHostFree(S->cost_host);
    S->cost_host = nullptr;
    S->drop_events();
    delete S;
    return PT_OK;
}

int pt_scene_update(pt_scene* S, const pt_scene_desc* desc, int flags) {
    if (!S) return fail(PT_ERR_INVALID_ARG, "pt_scene_update: null scene");
    if (!desc) return fail(PT_ERR_INVALID_ARG, "pt_scene_update: null scene description");
    if (flags == 0 || (flags & ~(PT_UPDATE_GEOMETRY | PT_UPDATE_SHADING)))
        return fail(PT_ERR_INVALID_ARG, "pt_scene_update: flags must be PT_UPDATE_GEOMETRY, PT_UPDATE_SHADING or both");
    return update_scene(S, desc, flags);
}

int pt_scene_rebuild(pt_scene* S, int flags) {
    if (!S) return fail(PT_ERR_INVALID_ARG, "pt_scene_rebuild: null scene");
    if (flags != 0) return fail(PT_ERR_INVALID_ARG, "pt_scene_rebuild: flags must be 0 (reserved)");
    DeviceGuard guard;
    { int grc = guard.enter(S->device); if (grc) return grc; }
    // frames of this handle that are still in flight, on the caller's streams and on the slots' own, read the scene
    HIP_TRY(hipDeviceSynchronize());
    const int rc = rebuild_scene(S);
    // the handle's own streams do not synchronise with the default stream the kernels above ran on
    const hipError_t e = hipDeviceSynchronize();
    if (rc) return rc;
    HIP_TRY(e);
    return PT_OK;
}

int pt_scene_set_groups(pt_scene* S, const int32_t* group_of_shape, int32_t num_groups) {
    if (!S) return fail(PT_ERR_INVALID_ARG, "pt_scene_set_groups: null scene");
    if (!group_of_shape) return fail(PT_ERR_INVALID_ARG, "pt_scene_set_groups: null group_of_shape");
    if (num_groups < 0 || num_groups > (1 << 20)) return fail(PT_ERR_INVALID_ARG, "pt_scene_set_groups: num_groups must be in [0, 2^20]");
    const int N = S->dev.num_prims;
    for (int k = 0; k < N; k++)
        if (group_of_shape[k] < -1 || group_of_shape[k] >= num_groups)
            return fail(PT_ERR_INVALID_ARG, "pt_scene_set_groups: group_of_shape[" + std::to_string(k) + "] is not in [-1, num_groups)");
    DeviceGuard guard;
    { int grc = guard.enter(S->device); if (grc) return grc; }
    int rc = S->group_of.ensure((size_t)N);
    if (rc) return rc;
    S->have_groups = false;                              // a copy that fails leaves no assignment, not half of one
    HIP_TRY(hipMemcpy(S->group_of.p, group_of_shape, (size_t)N * sizeof(int32_t), hipMemcpyHostToDevice));
    S->num_groups = num_groups;
    S->have_groups = true;
    return PT_OK;
}

int pt_scene_transform(pt_scene* S, const pt_transform* transforms, int32_t num_groups) {
    if (!S) return fail(PT_ERR_INVALID_ARG, "pt_scene_transform: null scene");
    return transform_scene(S, transforms, num_groups);
}

int pt_transform_geometry_host(const pt_transform* t, int32_t n, const float* positions, const float* normals, float* positions_out,
                               float* normals_out) {
    if (!t || n < 0 || !positions || !positions_out || (normals == nullptr) != (normals_out == nullptr))
        return fail(PT_ERR_INVALID_ARG, "pt_transform_geometry_host: null transform or array, or normals without normals_out");
    ptx::Entry e;
    if (const int bad = ptx::prepare(t, &e)) return fail(ptx::refusal_status(bad), "pt_transform_geometry_host: transform: " + ptx::refusal(bad));
    for (int32_t k = 0; k < n; k++) {
        const ptm::V3 p = ptx::point(e.m, ptm::mk(positions[3 * (size_t)k], positions[3 * (size_t)k + 1], positions[3 * (size_t)k + 2]));
        positions_out[3 * (size_t)k] = p.x; positions_out[3 * (size_t)k + 1] = p.y; positions_out[3 * (size_t)k + 2] = p.z;
        if (normals) {
            const ptm::V3 q = ptx::normal(e.c, ptm::mk(normals[3 * (size_t)k], normals[3 * (size_t)k + 1], normals[3 * (size_t)k + 2]));
            normals_out[3 * (size_t)k] = q.x; normals_out[3 * (size_t)k + 1] = q.y; normals_out[3 * (size_t)k + 2] = q.z;
        }
    }
    return PT_OK;
}

int pt_transform_sphere_host(const pt_transform* t, const float* center, float radius, float* center_out, float* radius_out) {
    if (!t || !center || !center_out || !radius_out) return fail(PT_ERR_INVALID_ARG, "pt_transform_sphere_host: null argument");
    ptx::Entry e;
    if (const int bad = ptx::prepare(t, &e)) return fail(ptx::refusal_status(bad), "pt_transform_sphere_host: transform: " + ptx::refusal(bad));
    const ptm::V3 p = ptx::point(e.m, ptm::mk(center[0], center[1], center[2]));
    center_out[0] = p.x; center_out[1] = p.y; center_out[2] = p.z;
    *radius_out = ptx::radius(e.m, radius);
    return PT_OK;
}

int pt_render_async(pt_scene* S, const pt_render_params* p, float* fb_dev, void* hip_stream) {
    return launch_render(S, p, fb_dev, 0, reinterpret_cast<hipStream_t>(hip_stream));
}

int pt_render_accumulate(pt_scene* S, const pt_render_params* p, float* accum_dev, void* hip_stream) {
    return launch_render(S, p, accum_dev, 2, reinterpret_cast<hipStream_t>(hip_stream));
}

int pt_render(pt_scene* S, const pt_render_params* p, float* fb, int fb_on_device) {
    if (!S || !p || !fb) return fail(PT_ERR_INVALID_ARG, "null argument");
    if (fb_on_device) {
        int rc = launch_render(S, p, fb, 0, nullptr);
        if (rc) return rc;
        HIP_TRY(hipStreamSynchronize(nullptr));
        return check_schedule_error(S);
    }
    RowSel rows;
    int rc = select_rows(p, &rows);
    if (rc) return rc;
    if (p->width <= 0) return fail(PT_ERR_INVALID_ARG, "width must be positive");
    const size_t n = (size_t)rows.count * (size_t)p->width * 3;
    DeviceGuard guard;
    { int grc = guard.enter(S->device); if (grc) return grc; }
    if ((rc = S->fb_tmp.ensure(n))) return rc;
    rc = launch_render(S, p, S->fb_tmp.p, 0, nullptr);
    if (rc) return rc;
    HIP_TRY(hipMemcpy(fb, S->fb_tmp.p, n * sizeof(float), hipMemcpyDeviceToHost));
    return check_schedule_error(S);
}

int pt_render_pixels(pt_scene* S, const pt_render_params* p, const int32_t* pixels, int32_t n, float* out, int on_device,
                     void* hip_stream) {
    const std::string pre = "pt_render_pixels: ";
    if (!S) return fail(PT_ERR_INVALID_ARG, pre + "null scene");
    if (!p) return fail(PT_ERR_INVALID_ARG, pre + "null p");
    if (n < 0) return fail(PT_ERR_INVALID_ARG, pre + "n is negative");
    if (n > (1 << 30)) return fail(PT_ERR_INVALID_ARG, pre + "n above 2^30");
    if (n > 0 && !pixels) return fail(PT_ERR_INVALID_ARG, pre + "null pixels");
    if (n > 0 && !out) return fail(PT_ERR_INVALID_ARG, pre + "null out");
    if (p->row_begin != 0 || (p->row_end != 0 && p->row_end != p->height) || (p->row_stride != 0 && p->row_stride != 1))
        return fail(PT_ERR_INVALID_ARG, pre + "row_begin / row_end / row_stride must select every row: the list names the pixels");
    if (on_device || n == 0) {
        const PixelList pl{reinterpret_cast<const uint32_t*>(pixels), (uint32_t)n};
        return launch_render(S, p, out, 0, reinterpret_cast<hipStream_t>(hip_stream), nullptr, &pl);
    }
    if (p->width <= 0 || p->height <= 0 || p->spp <= 0) return fail(PT_ERR_INVALID_ARG, "width, height and spp must be positive");
    const int64_t frame = (int64_t)p->width * (int64_t)p->height;
    for (int32_t k = 0; k < n; k++)
        if (pixels[k] < 0 || (int64_t)pixels[k] >= frame)
            return fail(PT_ERR_INVALID_ARG, pre + "pixels[" + std::to_string(k) + "] = " + std::to_string(pixels[k]) + " is outside the frame");
    DeviceGuard guard;
    { int grc = guard.enter(S->device); if (grc) return grc; }
    int rc;
    if ((rc = S->px_list.ensure((size_t)n)) || (rc = S->fb_tmp.ensure((size_t)n * 3))) return rc;
    HIP_TRY(hipMemcpy(S->px_list.p, pixels, (size_t)n * sizeof(int32_t), hipMemcpyHostToDevice));
    const PixelList pl{reinterpret_cast<const uint32_t*>(S->px_list.p), (uint32_t)n};
    if ((rc = launch_render(S, p, S->fb_tmp.p, 0, nullptr, nullptr, &pl))) return rc;
    HIP_TRY(hipMemcpy(out, S->fb_tmp.p, (size_t)n * 3 * sizeof(float), hipMemcpyDeviceToHost));
    return PT_OK;
}

int pt_render_adaptive(pt_scene* S, const pt_render_params* p, const pt_adaptive_params* a, float* fb, int32_t* spp_map,
                       float* err_map, int on_device) {
    if (!S || !p || !a || !fb) return fail(PT_ERR_INVALID_ARG, "null argument");
    if (p->width <= 0 || p->height <= 0 || p->spp <= 0) return fail(PT_ERR_INVALID_ARG, "width, height and spp must be positive");
    if (a->batch_spp < 0 || a->max_spp < 0) return fail(PT_ERR_INVALID_ARG, "negative batch_spp / max_spp");
    const int64_t max_spp = a->max_spp > 0 ? a->max_spp : 32 * (int64_t)p->spp;
    const int batch = a->batch_spp > 0 ? a->batch_spp : p->spp;
    if (max_spp < p->spp) return fail(PT_ERR_INVALID_ARG, "max_spp below spp (the first round)");
    if (max_spp > (1 << 20)) return fail(PT_ERR_INVALID_ARG, "max_spp above 2^20");
    if (!(a->max_error > 0.0f) || !std::isfinite(a->max_error)) return fail(PT_ERR_INVALID_ARG, "max_error must be positive and finite");
    if (a->p_value != 0.0f && !(a->p_value > 0.0f && a->p_value < 1.0f)) return fail(PT_ERR_INVALID_ARG, "p_value must lie in (0, 1)");
    if (!(a->min_luminance >= 0.0f) || !std::isfinite(a->min_luminance))
        return fail(PT_ERR_INVALID_ARG, "min_luminance must be finite and >= 0");
    if (p->sample_offset != 0) return fail(PT_ERR_INVALID_ARG, "pt_render_adaptive: sample_offset must be 0");
    if (p->stream_stride != 0 && p->stream_stride < max_spp)
        return fail(PT_ERR_INVALID_ARG, "stream_stride below max_spp: PCG streams of neighbouring pixels would overlap");
    RowSel rows;
    int rc = select_rows(p, &rows);
    if (rc) return rc;
    const uint64_t npix = (uint64_t)rows.count * (uint64_t)p->width;
    if (npix > (1ull << 30)) return fail(PT_ERR_INVALID_ARG, "more than 2^30 pixels per call");
    // z = Phi^-1(1 - p/2): the root of erfc(z / sqrt 2) = p, by bisection (erfc falls monotonically)
    const double pv = a->p_value != 0.0f ? (double)a->p_value : 0.05;
    double zlo = 0.0, zhi = 64.0;
    for (int k = 0; k < 200; k++) {
        const double mid = 0.5 * (zlo + zhi);
        (std::erfc(mid / std::sqrt(2.0)) > pv ? zlo : zhi) = mid;
    }
    DeviceGuard guard;
    { int grc = guard.enter(S->device); if (grc) return grc; }
    S->info_adaptive_rounds = 0;
    pt_render_params pr = *p;
    pr.stream_stride = p->stream_stride > 0 ? p->stream_stride : (int32_t)max_spp;
    if (npix == 0) {                 // no rows selected: an empty frame (its counters read zero)
        if ((rc = launch_render(S, &pr, fb, 0, nullptr))) return rc;
        HIP_TRY(hipStreamSynchronize(nullptr));
        return PT_OK;
    }
    if ((rc = S->ad_sum.ensure(npix * 3)) || (rc = S->ad_mom.ensure(npix * 2)) || (rc = S->ad_list[0].ensure(npix)) ||
        (rc = S->ad_list[1].ensure(npix)) || (rc = S->ad_count.ensure(1)))
        return rc;
    float* fb_d = fb;
    int32_t* spp_d = spp_map;
    float* err_d = err_map;
    if (!on_device) {
        if ((rc = S->fb_tmp.ensure(npix * 3))) return rc;
        fb_d = S->fb_tmp.p;
        if (spp_map && (rc = S->ad_spp_tmp.ensure(npix))) return rc;
        if (err_map && (rc = S->ad_err_tmp.ensure(npix))) return rc;
        spp_d = spp_map ? S->ad_spp_tmp.p : nullptr;
        err_d = err_map ? S->ad_err_tmp.p : nullptr;
    }
    AdaptiveRound ar{};
    ar.args.z = 0.5 * (zlo + zhi);
    ar.args.max_error = a->max_error;
    ar.args.min_luminance = a->min_luminance;
    ar.args.max_spp = (int)max_spp;
    ar.args.sum = S->ad_sum.p;
    ar.args.mom = S->ad_mom.p;
    ar.args.count_out = S->ad_count.p;
    ar.args.fb = fb_d;
    ar.args.spp_map = spp_d;
    ar.args.err_map = err_d;
    // checkpoints n = spp, spp + batch, spp + 2 batch, ... cut at max_spp: they depend on these three numbers only (a round too
    // big for the scratch budget runs in several sample passes before its one check)
    int n = 0;
    uint32_t n_list = (uint32_t)npix;
    for (int round = 0;; round++) {
        const int spp_r = round == 0 ? p->spp : (int)std::min<int64_t>(batch, max_spp - n);
        pr.spp = spp_r;
        pr.sample_offset = n;
        ar.round = round;
        ar.args.list_in = round == 0 ? nullptr : S->ad_list[(round - 1) & 1].p;
        ar.args.list_out = S->ad_list[round & 1].p;
        ar.args.n_total = n + spp_r;
        HIP_TRY(hipMemsetAsync(S->ad_count.p, 0, sizeof(uint32_t), nullptr));
        const PixelList pl{ar.args.list_in, n_list};
        if ((rc = launch_render(S, &pr, fb_d, 0, nullptr, &ar, round == 0 ? nullptr : &pl))) return rc;
        n += spp_r;
        S->info_adaptive_rounds = round + 1;
        HIP_TRY(hipMemcpy(&n_list, S->ad_count.p, sizeof(uint32_t), hipMemcpyDeviceToHost));   // the one read-back per round
        if (n_list == 0) break;
        if (n >= max_spp || n_list > npix) return fail(PT_ERR_DEVICE, "internal error: adaptive list after the last checkpoint");
    }
    if ((rc = check_schedule_error(S))) return rc;
    if (!on_device) {
        HIP_TRY(hipMemcpy(fb, fb_d, npix * 3 * sizeof(float), hipMemcpyDeviceToHost));
        if (spp_map) HIP_TRY(hipMemcpy(spp_map, spp_d, npix * sizeof(int32_t), hipMemcpyDeviceToHost));
        if (err_map) HIP_TRY(hipMemcpy(err_map, err_d, npix * sizeof(float), hipMemcpyDeviceToHost));
    } else {
        HIP_TRY(hipStreamSynchronize(nullptr));
    }
    return PT_OK;
}

int pt_render_aov(pt_scene* S, const pt_render_params* p, float* albedo, float* normal, float* depth, int32_t* prim, int on_device) {
    if (!S || !p) return fail(PT_ERR_INVALID_ARG, "null argument");
    const pt_guide_buffers out{albedo, normal, depth, prim, nullptr, nullptr};
    return guide_pass(S, p, nullptr, out, on_device);
}

int pt_render_guides(pt_scene* S, const pt_render_params* p, const pt_motion_params* m, const pt_guide_buffers* out, int on_device) {
    if (!S) return fail(PT_ERR_INVALID_ARG, "pt_render_guides: null scene");
    if (!p) return fail(PT_ERR_INVALID_ARG, "pt_render_guides: null p");
    if (!m) return fail(PT_ERR_INVALID_ARG, "pt_render_guides: null m");
    if (!out) return fail(PT_ERR_INVALID_ARG, "pt_render_guides: null out");
    if (m->geometry != PT_MOTION_GEOMETRY_CURRENT && m->geometry != PT_MOTION_GEOMETRY_PREVIOUS)
        return fail(PT_ERR_INVALID_ARG, "pt_motion_params.geometry must be PT_MOTION_GEOMETRY_CURRENT or PT_MOTION_GEOMETRY_PREVIOUS");
    return guide_pass(S, p, m, *out, on_device);
}

int pt_render_guides_async(pt_scene* S, const pt_render_params* p, const pt_motion_params* m, const pt_guide_buffers* out, void* hip_stream) {
    if (!S) return fail(PT_ERR_INVALID_ARG, "pt_render_guides_async: null scene");
    if (!p) return fail(PT_ERR_INVALID_ARG, "pt_render_guides_async: null p");
    if (!out) return fail(PT_ERR_INVALID_ARG, "pt_render_guides_async: null out");
    if (m && m->geometry != PT_MOTION_GEOMETRY_CURRENT && m->geometry != PT_MOTION_GEOMETRY_PREVIOUS)
        return fail(PT_ERR_INVALID_ARG, "pt_motion_params.geometry must be PT_MOTION_GEOMETRY_CURRENT or PT_MOTION_GEOMETRY_PREVIOUS");
    return guides_async_call(S, p, m, *out, hip_stream);
}

int pt_trace_rays(pt_scene* S, const float* rays, int32_t n, int mode, int traversal, float* out_tuv, int32_t* out_prim, int on_device,
                  void* hip_stream) {
    if (!S) return fail(PT_ERR_INVALID_ARG, "pt_trace_rays: null scene");
    return trace_rays_call(S, rays, n, mode, traversal, out_tuv, out_prim, on_device, hip_stream);
}

int pt_temporal_accumulate(pt_scene* S, const pt_temporal_params* t, const float* color, const float* normal, const float* motion,
                           const float* prev_depth, const float* hist_color, const float* hist_normal, const float* hist_depth,
                           const float* hist_len, float* out_color, float* out_len, int on_device, void* hip_stream) {
    const pt_temporal_io io = temporal_io(color, normal, motion, prev_depth, hist_color, hist_normal, hist_depth, hist_len, out_color, out_len);
    return temporal_call("pt_temporal_accumulate", false, S, t, 0.0f, &io, on_device, hip_stream);
}

int pt_temporal_accumulate_host(const pt_temporal_params* t, const float* color, const float* normal, const float* motion,
                                const float* prev_depth, const float* hist_color, const float* hist_normal, const float* hist_depth,
                                const float* hist_len, float* out_color, float* out_len) {
    const pt_temporal_io io = temporal_io(color, normal, motion, prev_depth, hist_color, hist_normal, hist_depth, hist_len, out_color, out_len);
    ptt::Resolved r;
    float floor_v;
    int rc = temporal_args("pt_temporal_accumulate", false, t, 0.0f, &io, &r, &floor_v);
    if (rc) return rc;
    ptt::run_host(r, false, floor_v, io);
    return PT_OK;
}

int pt_temporal_accumulate_moments(pt_scene* S, const pt_temporal_params* t, float albedo_floor, const pt_temporal_io* io, int on_device,
                                   void* hip_stream) {
    return temporal_call("pt_temporal_accumulate_moments", true, S, t, albedo_floor, io, on_device, hip_stream);
}

int pt_temporal_accumulate_moments_host(const pt_temporal_params* t, float albedo_floor, const pt_temporal_io* io) {
    ptt::Resolved r;
    float floor_v;
    int rc = temporal_args("pt_temporal_accumulate_moments", true, t, albedo_floor, io, &r, &floor_v);
    if (rc) return rc;
    ptt::run_host(r, true, floor_v, *io);
    return PT_OK;
}

int pt_temporal_gradient(pt_scene* S, const pt_gradient_params* g, const float* prev_color, const float* resampled, float* lambda_out,
                         int on_device, void* hip_stream) {
    if (!S) return fail(PT_ERR_INVALID_ARG, "pt_temporal_gradient: null scene");
    ptg::Resolved r;
    int rc = gradient_args("pt_temporal_gradient", g, prev_color, resampled, lambda_out, &r);
    if (rc) return rc;
    return gradient_call(S, r, prev_color, resampled, lambda_out, on_device, hip_stream);
}

int pt_temporal_gradient_host(const pt_gradient_params* g, const float* prev_color, const float* resampled, float* lambda_out) {
    ptg::Resolved r;
    int rc = gradient_args("pt_temporal_gradient_host", g, prev_color, resampled, lambda_out, &r);
    if (rc) return rc;
    try {
        ptg::run_host(r, prev_color, resampled, lambda_out);
    } catch (const std::exception& e) {
        return fail(PT_ERR_DEVICE, std::string("pt_temporal_gradient_host: ") + e.what());
    }
    return PT_OK;
}

int pt_gradient_pixels(pt_scene* S, const pt_gradient_params* g, uint32_t seed, int32_t* pixels_out, int on_device, void* hip_stream) {
    if (!S) return fail(PT_ERR_INVALID_ARG, "pt_gradient_pixels: null scene");
    ptg::Resolved r;
    int rc = sparse_args("pt_gradient_pixels", g, {{"pixels_out", pixels_out}}, &r);
    if (rc) return rc;
    return gradient_pixels_call(S, r, seed, pixels_out, on_device, hip_stream);
}

int pt_gradient_pixels_host(const pt_gradient_params* g, uint32_t seed, int32_t* pixels_out) {
    ptg::Resolved r;
    int rc = sparse_args("pt_gradient_pixels_host", g, {{"pixels_out", pixels_out}}, &r);
    if (rc) return rc;
    ptg::pixels_host(r, seed, pixels_out);
    return PT_OK;
}

int pt_temporal_gradient_sparse(pt_scene* S, const pt_gradient_params* g, const float* prev_color, const int32_t* pixels,
                                const float* resampled, float* lambda_out, int on_device, void* hip_stream) {
    if (!S) return fail(PT_ERR_INVALID_ARG, "pt_temporal_gradient_sparse: null scene");
    ptg::Resolved r;
    int rc = sparse_args("pt_temporal_gradient_sparse", g,
                         {{"prev_color", prev_color}, {"pixels", pixels}, {"resampled", resampled}, {"lambda_out", lambda_out}}, &r);
    if (rc) return rc;
    return gradient_sparse_call(S, r, prev_color, pixels, resampled, lambda_out, on_device, hip_stream);
}

int pt_temporal_gradient_sparse_host(const pt_gradient_params* g, const float* prev_color, const int32_t* pixels, const float* resampled,
                                     float* lambda_out) {
    ptg::Resolved r;
    int rc = sparse_args("pt_temporal_gradient_sparse_host", g,
                         {{"prev_color", prev_color}, {"pixels", pixels}, {"resampled", resampled}, {"lambda_out", lambda_out}}, &r);
    if (rc) return rc;
    try {
        ptg::run_host_sparse(r, prev_color, pixels, resampled, lambda_out);
    } catch (const std::exception& e) {
        return fail(PT_ERR_DEVICE, std::string("pt_temporal_gradient_sparse_host: ") + e.what());
    }
    return PT_OK;
}

int pt_temporal_accumulate_adaptive(pt_scene* S, const pt_temporal_params* t, float albedo_floor, const pt_temporal_io* io,
                                    const float* lambda, int32_t stride, int on_device, void* hip_stream) {
    return temporal_call("pt_temporal_accumulate_adaptive", true, S, t, albedo_floor, io, on_device, hip_stream, true, lambda, stride);
}

int pt_temporal_accumulate_adaptive_host(const pt_temporal_params* t, float albedo_floor, const pt_temporal_io* io, const float* lambda,
                                         int32_t stride) {
    const char* fn = "pt_temporal_accumulate_adaptive";
    ptt::Resolved r;
    float floor_v;
    int rc = temporal_args(fn, true, t, albedo_floor, io, &r, &floor_v);
    if (rc) return rc;
    ptt::Lambda lam{};
    if ((rc = adaptive_args(fn, r, lambda, stride, &lam))) return rc;
    ptt::run_host(r, true, floor_v, *io, &lam);
    return PT_OK;
}

int pt_denoise_variance(pt_scene* S, const pt_vdenoise_params* d, const float* color, const float* albedo, const float* normal,
                        const float* depth, const float* moments, const float* hist_len, float* out, float* out_variance,
                        int on_device, void* hip_stream) {
    if (!S) return fail(PT_ERR_INVALID_ARG, "pt_denoise_variance: null scene");
    const ptdn::Frames f{color, albedo, normal, depth, moments, hist_len, out, out_variance};
    ptdn::Resolved r;
    int rc = vdenoise_args(d, f, &r);
    if (rc) return rc;
    return denoise_call("pt_denoise_variance", S, r, f, S->vd_guide, S->vd_x, S->vd_host, on_device, hip_stream);
}

int pt_denoise_variance_host(const pt_vdenoise_params* d, const float* color, const float* albedo, const float* normal,
                             const float* depth, const float* moments, const float* hist_len, float* out, float* out_variance) {
    const ptdn::Frames f{color, albedo, normal, depth, moments, hist_len, out, out_variance};
    ptdn::Resolved r;
    int rc = vdenoise_args(d, f, &r);
    if (rc) return rc;
    return denoise_host_call("pt_denoise_variance_host", r, f);
}

int pt_denoise(pt_scene* S, const pt_denoise_params* d, const float* color, const float* albedo, const float* normal,
               const float* depth, float* out, int on_device, void* hip_stream) {
    if (!S) return fail(PT_ERR_INVALID_ARG, "null argument");
    const ptdn::Frames f{color, albedo, normal, depth, nullptr, nullptr, out, nullptr};
    ptdn::Resolved r;
    int rc = denoise_args(d, f, &r);
    if (rc) return rc;
    return denoise_call("pt_denoise", S, r, f, S->dn_guide, S->dn_x, S->dn_host, on_device, hip_stream);
}

int pt_denoise_host(const pt_denoise_params* d, const float* color, const float* albedo, const float* normal, const float* depth,
                    float* out) {
    const ptdn::Frames f{color, albedo, normal, depth, nullptr, nullptr, out, nullptr};
    ptdn::Resolved r;
    int rc = denoise_args(d, f, &r);
    if (rc) return rc;
    return denoise_host_call("pt_denoise_host", r, f);
}

int pt_get_counters(pt_scene* S, pt_counters* out) {
    if (!S || !out) return fail(PT_ERR_INVALID_ARG, "null argument");
    std::memset(out, 0, sizeof *out);
    DeviceGuard guard;
    unsigned long long c[kSlotStride];
    int rc = synced_slot_sums(S, guard, c);
    if (rc || !S->cur().ctl.p) return rc;
    out->paths = c[0]; out->segments = c[1]; out->node_visits = c[2]; out->leaf_tests = c[3];
    if ((rc = schedule_error(S, c))) return rc;
    if (S->have_timing && S->last_frame()) {
        int rc2 = frame_times(*S->last_frame(), &out->kernel_ms, &out->resolve_ms);
        if (rc2) return rc2;
    }
    return PT_OK;
}

int pt_get_frame_times(pt_scene* S, int max_frames, double* kernel_ms, double* resolve_ms, int* n_out) {
    if (!S || !kernel_ms || !resolve_ms || !n_out || max_frames < 0) return fail(PT_ERR_INVALID_ARG, "bad argument");
    *n_out = 0;
    DeviceGuard guard;
    { int grc = guard.enter(S->device); if (grc) return grc; }
    HIP_TRY(hipStreamSynchronize(S->last_stream));
    const uint64_t have = std::min<uint64_t>(S->frame_seq, S->frames.size());
    const int n = (int)std::min<uint64_t>(have, (uint64_t)max_frames);
    for (int k = 0; k < n; k++) {                        // oldest first
        const pt_scene::FrameRec& f = S->frames[(S->frame_seq - (uint64_t)n + (uint64_t)k) % S->frames.size()];
        int rc = frame_times(f, &kernel_ms[k], &resolve_ms[k]);
        if (rc) return rc;
    }
    *n_out = n;
    return PT_OK;
}

int pt_scene_set_option(pt_scene* S, const char* key, int64_t value) {
    if (!S || !key) return fail(PT_ERR_INVALID_ARG, "null argument");
    const std::string k(key);
    if (k == "blocks_per_cu") {
        if (value < 0 || value > 32) return fail(PT_ERR_INVALID_ARG, "blocks_per_cu must be 0 (automatic) .. 32");
        S->opt_blocks_per_cu = value;
    }
    else if (k == "scratch_bytes") S->opt_scratch_bytes = value;
    else if (k == "force_global") S->opt_force_global = value;
    else if (k == "stats") S->opt_stats = value;
    else if (k == "xcd_regions") S->opt_xcd_regions = value;
    else if (k == "octants") S->opt_octants = value;
    else if (k == "top_cache") S->opt_top_cache = value;
    else if (k == "fast_tree") S->opt_fast_tree = value;
    else if (k == "lds_budget_kb") S->opt_lds_budget_kb = value;
    else if (k == "chunk") S->opt_chunk = value;
    else if (k == "item_order") S->opt_item_order = value;
    else if (k == "specialize") S->opt_specialize = value;
    else if (k == "timing_frames") {
        if (value < 0 || value > 4096) return fail(PT_ERR_INVALID_ARG, "timing_frames must be 0 .. 4096");
        S->opt_timing_frames = value;
    }
    else if (k == "kernel") { if (value < 1 || value > 3) return fail(PT_ERR_INVALID_ARG, "kernel must be 1, 2 or 3"); S->opt_kernel = value; }
    else if (k == "frames_in_flight") {
        if (value < 1 || value > kMaxFramesInFlight) return fail(PT_ERR_INVALID_ARG, "frames_in_flight must be 1 .. " + std::to_string(kMaxFramesInFlight));
        S->opt_frames_in_flight = value;
    }
    else if (k == "q_target") S->opt_q_target = value;
    else if (k == "q_swap") S->opt_q_swap = value;
    else if (k == "q_low") S->opt_q_low = value;
    else if (k == "v2_thresh") S->opt_v2_thresh = value;
    else if (k == "v2_inner") S->opt_v2_inner = value;
    else if (k == "v2_minw") S->opt_v2_minw = value;
    else if (k == "reg_stack") { if (value != 0 && value != 1) return fail(PT_ERR_INVALID_ARG, "reg_stack must be 0 or 1"); S->opt_reg_stack = value; }
    else if (k == "leaf_sweep") { if (value != 0 && value != 1) return fail(PT_ERR_INVALID_ARG, "leaf_sweep must be 0 or 1"); S->opt_leaf_sweep = value; }
    else if (k == "query_refill") { if (value < 0 || value > 64) return fail(PT_ERR_INVALID_ARG, "query_refill must be 0 (automatic) .. 64"); S->opt_query_refill = value; }
    else if (k == "query_guides") { if (value < 0 || value > 2) return fail(PT_ERR_INVALID_ARG, "query_guides must be 0 (automatic), 1 or 2"); S->opt_query_guides = value; }
    else if (k == "query_blocks") { if (value < 0 || value > 4096) return fail(PT_ERR_INVALID_ARG, "query_blocks must be 0 (automatic) .. 4096"); S->opt_query_blocks = value; }
    else if (k == "tree_cost") { if (value != 0 && value != 1) return fail(PT_ERR_INVALID_ARG, "tree_cost must be 0 or 1"); S->opt_tree_cost = value; }
    else if (k == "rebuild_at_permille") {
        if (value != 0 && value < 1001) return fail(PT_ERR_INVALID_ARG, "rebuild_at_permille must be 0 (never) or at least 1001");
        S->opt_rebuild_at = value;
    }
    else return fail(PT_ERR_INVALID_ARG, "unknown option " + k);
    return PT_OK;
}

int pt_scene_get_info(pt_scene* S, const char* key, int64_t* value) {
    if (!S || !key || !value) return fail(PT_ERR_INVALID_ARG, "null argument");
    const std::string k(key);
    // what the next plain render decides (exact unless the key says pruned; without NEE or a pixel list, so it cannot fail)
    TraceChoice next;
    (void)choose_trace(S, k == "vgprs_pruned" ? PT_TRAVERSAL_PRUNED : PT_TRAVERSAL_EXACT, false, false, &next);
    DeviceGuard guard;
    unsigned long long c[kSlotStride];
    if (k == "grid") *value = S->info_grid;
    else if (k == "lds_bytes") *value = S->info_lds_bytes;
    else if (k == "lds_scene") *value = S->info_lds_scene;
    else if (k == "residency") *value = next.res;
    else if (k == "passes") *value = S->info_passes;
    else if (k == "adaptive_rounds") *value = S->info_adaptive_rounds;
    else if (k == "occupancy") *value = S->info_occupancy;                // what the occupancy query allows
    else if (k == "blocks_per_cu") *value = S->info_blocks_per_cu;        // what the last launch used
    else if (k == "redo_segments") {                                     // STATS: segments rerun in reference order by the last render
        int rc = synced_slot_sums(S, guard, c);
        if (rc) return rc;
        *value = (int64_t)c[12];
    }
    else if (k == "num_cus") *value = S->num_cus;
    else if (k == "bvh_depth") *value = S->tree[0].depth;
    else if (k == "stack_entries") *value = S->tree[next.which].stack_cap;   // per lane, sentinel included
    else if (k == "fast_tree") *value = S->have_fast ? 1 : 0;             // an internal tree exists (the caller's tree is nested)
    else if (k == "debug_reruns") *value = S->info_debug_reruns;          // rays the last pt_debug_intersect reran in reference order
    else if (k == "fast_tree_cost_permille") *value = S->fast_cost_permille;   // summed inner-box area, internal tree / caller's tree x 1000 (0: none built)
    else if (k == "fast_tree_is_callers") *value = (S->have_fast && S->fast_is_callers_topology) ? 1 : 0;
    else if (k == "fast_tree_on") *value = next.which;       // ... and the next exact render traverses it
    else if (k == "fast_tree_depth") *value = S->have_fast ? S->tree[1].depth : 0;
    else if (k == "scene_bytes") *value = S->scene_bytes;
    else if (k == "num_inner_nodes") *value = S->tree[0].num_nodes;
    else if (k == "top_nodes") *value = make_plan(S, next).top_count;     // make_plan's count even on kernel 3, whose make_plan_q caches another
    else if (k == "device") *value = S->device;
    else if (k == "sweep_on_device") *value = S->sweep_on_device;         // the internal tree was built on the GPU (pt_sweep_build.hip)
    else if (k.rfind("create_us", 0) == 0 && k.size() == 10 && k[9] >= '0' && k[9] <= '6') *value = S->create_us[k[9] - '0'];
    else if (k == "prev_geometry") *value = S->have_prev ? 1 : 0;         // records from before the last geometry update are kept (pt_render_guides)
    else if (k == "updates") *value = S->updates;                         // successful pt_scene_update calls so far
    else if (k.rfind("update_us", 0) == 0 && k.size() == 10 && k[9] >= '0' && k[9] <= '3') *value = S->update_us[k[9] - '0'];
    else if (k == "groups") *value = S->have_groups ? S->num_groups : 0;  // groups of the assignment pt_scene_set_groups made (0: none)
    else if (k == "rest_geometry") *value = S->have_rest ? 1 : 0;         // a snapshot of the rest records is held (pt_scene_transform)
    else if (k == "transforms") *value = S->transforms;                   // successful pt_scene_transform calls so far
    else if (k.rfind("transform_us", 0) == 0 && k.size() == 13 && k[12] >= '0' && k[12] <= '3') *value = S->transform_us[k[12] - '0'];
    else if (k == "rebuilds") *value = S->rebuilds;                       // successful pt_scene_rebuild calls so far, a policy's included
    else if (k == "rebuilds_auto") *value = S->rebuilds_auto;             // ... those that option rebuild_at_permille made
    else if (k == "rebuild_adopted") *value = S->rebuild_adopted;         // the last one adopted its tree (1) or kept the one it had (0)
    else if (k == "rebuild_cost_permille") *value = S->rebuild_cost_permille;   // the last candidate's probe ratio (as fast_tree_cost_permille)
    else if (k.rfind("rebuild_us", 0) == 0 && k.size() == 11 && k[10] >= '0' && k[10] <= '3') *value = S->rebuild_us[k[10] - '0'];
    else if (k == "tree_cost0_bits" || k == "tree_cost1_bits") {
        // option tree_cost: the fp64 bit pattern of tree 0's / 1's cost after the last refit (0: no such tree, nothing measured)
        const int t = k[9] - '0';
        const double c = (S->cost_on() && (t == 0 || S->have_fast)) ? S->cost_now[t] : 0.0;
        *value = c > 0.0 ? __builtin_bit_cast(int64_t, c) : 0;
    }
    else if (k == "tree_cost0_permille" || k == "tree_cost1_permille") {
        // ... and that cost over the cost of the boxes as built (or as last rebuilt), x 1000; 1000 before any refit
        const int t = k[9] - '0';
        *value = (S->cost_on() && (t == 0 || S->have_fast)) ? cost_permille(S, t) : 1000;
    }
    else if (k == "refit_shape0" || k == "refit_shape1") {
        // how a geometry update refits tree 0 (the caller's) / 1 (the internal one): 0 no plan (no such tree, a one-shape scene, or
        // no geometry update yet), 1 one launch, 2 scatter + a launch per wide level + the narrow top, 3 scatter + the narrow top alone
        const ptf::Plan& pl = S->refit_plan[k[11] - '0'];
        *value = !pl.built ? 0 : pl.whole_tree ? 1 : pl.narrow_top < pl.levels - 1 ? 2 : 3;
    }
    else if (k == "kernel") *value = S->info_kernel;                      // the kernel the last render ran on (1, 2 or 3)
    else if (k == "trace_variant") *value = S->info_trace_variant;        // ... and its template arguments (include/pt_api.h)
    else if (k == "path_bank") *value = S->info_path_bank;                // ... which handed out path starts from a register bank (1) or not
    else if (k == "leaf_sweep") *value = S->info_leaf_sweep;              // ... finding its leaves by the box sweep (1: trace_kernel_v2_sweep) or on the tree (0)
    else if (k == "sweep_boxes") *value = S->sweep_groups;                // groups of equal leaf boxes the handle holds for the sweep (0: none)
    else if (k == "reg_stack") *value = S->info_reg_stack;                // ... with the traversal stack in a register (1) or in LDS / global memory (0)
    else if (k == "block_threads") *value = S->info_kernel == 3 ? kQBlock : kBlock;
    else if (k == "frames_in_flight") *value = S->opt_frames_in_flight;
    else if (k == "query_chunk") *value = ptq::kQueryChunk;               // ray indices a wave of the query kernel reserves per atomic
    else if (k == "query_guides") *value = S->info_query_guides;          // the last pt_render_guides_async ran on the refilling kernel (1) or on aov_kernel (0)
    else if (k == "query_grid") *value = S->info_query_grid;              // blocks of the last query launch (pt_trace_rays, pt_render_guides_async)
    else if (k.rfind("qdiag", 0) == 0 && k.size() >= 6 && k.size() <= 7 && k.find_first_not_of("0123456789", 5) == std::string::npos &&
             std::stoi(k.substr(5)) < 11) {
        // schedule diagnostics of the last STATS render of trace_kernel_q: counter slots [4..14], see pt_kernel_q.h
        int rc = synced_slot_sums(S, guard, c);
        if (rc) return rc;
        *value = (int64_t)c[4 + std::stoi(k.substr(5))];
    }
    else if (k.rfind("diag", 0) == 0 && k.size() >= 5 && k.size() <= 7 && k.find_first_not_of("0123456789", 4) == std::string::npos &&
             std::stoi(k.substr(4)) < 8 + kNumCounters - kTimelineBase) {
        // schedule diagnostics / launch timeline of the last STATS render (trace_kernel_v2): see pt_kernels.h
        unsigned long long v = 0;
        const int idx = std::stoi(k.substr(4));
        if (idx < 8) {                                    // schedule diagnostics: summed over the counter slots
            int rc = synced_slot_sums(S, guard, c);
            if (rc) return rc;
            v = c[4 + idx];
        } else {                                          // launch timeline / histograms
            { int grc = guard.enter(S->device); if (grc) return grc; }
            HIP_TRY(hipStreamSynchronize(S->last_stream));
            if (S->cur().ctl.p) HIP_TRY(hipMemcpy(&v, S->counters() + kTimelineBase + (idx - 8), sizeof v, hipMemcpyDeviceToHost));
        }
        *value = (int64_t)v;
    }
    else if (k == "vgprs" || k == "vgprs_pruned") {
        // of the next render without NEE or a pixel list; a launch that would take the sweep kernel reports the entry it stands in for
        hipFuncAttributes fa;
        const void* f = find_trace(next, false).fn;
        if (!f) return fail(PT_ERR_INVALID_ARG, "no such kernel variant");
        HIP_TRY(hipFuncGetAttributes(&fa, f));
        *value = fa.numRegs;
    } else return fail(PT_ERR_INVALID_ARG, "unknown info key " + k);
    return PT_OK;
}

int pt_debug_math(int op, const float* x, const float* y, float* out0, float* out1, int n) {
    if (!x || !y || !out0 || !out1 || n < 0 || op < 0 || op > 2) return fail(PT_ERR_INVALID_ARG, "bad argument");
    if (n == 0) return PT_OK;
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) return fail(PT_ERR_NO_DEVICE, "no HIP device available");
    DevBuf<float> dx, dy, d0, d1;
    int rc;
    if ((rc = dx.ensure(n)) || (rc = dy.ensure(n)) || (rc = d0.ensure(n)) || (rc = d1.ensure(n))) return rc;
    hipError_t e = hipMemcpy(dx.p, x, n * sizeof(float), hipMemcpyHostToDevice);
    if (e == hipSuccess) e = hipMemcpy(dy.p, y, n * sizeof(float), hipMemcpyHostToDevice);
    if (e == hipSuccess) e = hipMemset(d1.p, 0, n * sizeof(float));
    if (e == hipSuccess) {
        hipLaunchKernelGGL(math_kernel, dim3((n + 255) / 256), dim3(256), 0, nullptr, op, dx.p, dy.p, d0.p, d1.p, n);
        e = hipGetLastError();
    }
    if (e == hipSuccess) e = hipMemcpy(out0, d0.p, n * sizeof(float), hipMemcpyDeviceToHost);
    if (e == hipSuccess) e = hipMemcpy(out1, d1.p, n * sizeof(float), hipMemcpyDeviceToHost);
    if (e != hipSuccess) return fail(PT_ERR_DEVICE, std::string("pt_debug_math: ") + hipGetErrorString(e));
    return PT_OK;
}

int pt_debug_exact_math(int op, uint32_t begin, uint64_t count, uint64_t* mismatches, int64_t* first_mismatch) {
    if (!mismatches || !first_mismatch || op < 0 || op > 3 || count > (1ull << 32) - begin)
        return fail(PT_ERR_INVALID_ARG, "bad argument");
    *mismatches = 0;
    *first_mismatch = -1;
    if (count == 0) return PT_OK;
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) return fail(PT_ERR_NO_DEVICE, "no HIP device available");
    DevBuf<unsigned long long> dbad;
    DevBuf<uint32_t> dfirst;
    int rc;
    if ((rc = dbad.ensure(1)) || (rc = dfirst.ensure(1))) return rc;
    unsigned long long nbad = 0;
    uint32_t first = 0xffffffffu;
    hipError_t e = hipMemcpy(dbad.p, &nbad, sizeof(nbad), hipMemcpyHostToDevice);
    if (e == hipSuccess) e = hipMemcpy(dfirst.p, &first, sizeof(first), hipMemcpyHostToDevice);
    if (e == hipSuccess) {
        const uint64_t blocks = std::min<uint64_t>((count + 255) / 256, 4096);
        hipLaunchKernelGGL(exact_math_kernel, dim3((unsigned)blocks), dim3(256), 0, nullptr, op, begin, count, dbad.p, dfirst.p);
        e = hipGetLastError();
    }
    if (e == hipSuccess) e = hipMemcpy(&nbad, dbad.p, sizeof(nbad), hipMemcpyDeviceToHost);
    if (e == hipSuccess) e = hipMemcpy(&first, dfirst.p, sizeof(first), hipMemcpyDeviceToHost);
    if (e != hipSuccess) return fail(PT_ERR_DEVICE, std::string("pt_debug_exact_math: ") + hipGetErrorString(e));
    *mismatches = nbad;
    if (nbad) *first_mismatch = (int64_t)begin + first;
    return PT_OK;
}

int pt_debug_math_host(int op, const float* x, const float* y, float* out0, float* out1, int n) {
    if (!x || !y || !out0 || !out1 || n < 0 || op < 0 || op > 2) return fail(PT_ERR_INVALID_ARG, "bad argument");
    for (int k = 0; k < n; k++) {
        if (op == 0) {
            ptm::sincos_det(x[k], out0[k], out1[k]);
        } else if (op == 1) {
            out0[k] = ptm::pow_det(x[k], y[k]);
            out1[k] = 0.0f;
        } else {
            ptm::Pcg r = ptm::pcg_init((uint64_t)__builtin_bit_cast(uint32_t, x[k]), (uint64_t)__builtin_bit_cast(uint32_t, y[k]));
            out0[k] = ptm::pcg_float(r);
            out1[k] = ptm::pcg_float(r);
        }
    }
    return PT_OK;
}

int pt_bvh_build_sweep(const pt_scene_desc* d, pt_bvh_node* out_nodes, int32_t* out_root, int32_t* out_depth, double* out_build_ms) {
    if (!d || !out_nodes || !out_root) return fail(PT_ERR_INVALID_ARG, "bad argument");
    const int N = d->num_shapes;
    if (N <= 0 || !d->nodes || d->num_nodes != 2 * N - 1) return fail(PT_ERR_BAD_SCENE, "needs the leaf boxes of a 2*num_shapes-1 node pool");
    std::vector<float> boxes((size_t)N * 6);
    std::vector<char> seen(N, 0);
    for (int k = 0; k < d->num_nodes; k++) {
        const pt_bvh_node& nd = d->nodes[k];
        if (nd.prim == -1) continue;
        if (nd.prim < 0 || nd.prim >= N || seen[nd.prim]) return fail(PT_ERR_BAD_SCENE, "leaves must cover every shape exactly once");
        seen[nd.prim] = 1;
        std::memcpy(&boxes[(size_t)nd.prim * 6], nd.bmin, 12);
        std::memcpy(&boxes[(size_t)nd.prim * 6 + 3], nd.bmax, 12);
    }
    for (int i = 0; i < N; i++)
        if (!seen[i]) return fail(PT_ERR_BAD_SCENE, "leaves must cover every shape exactly once");
    for (float v : boxes)
        if (!std::isfinite(v)) return fail(PT_ERR_BAD_SCENE, "leaf box is not finite");
    const auto t0 = std::chrono::steady_clock::now();
    std::vector<pt_bvh_node> nodes;
    int32_t root = 0, depth = 0;
    try {
        pts::build_sweep_tree(boxes.data(), N, nodes, &root, &depth);
    } catch (const std::exception& e) {
        return fail(PT_ERR_DEVICE, std::string("pt_bvh_build_sweep: ") + e.what());
    }
    std::memcpy(out_nodes, nodes.data(), nodes.size() * sizeof(pt_bvh_node));
    *out_root = root;
    if (out_depth) *out_depth = depth;
    if (out_build_ms) *out_build_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
    return PT_OK;
}

int pt_bvh_build_sweep_device(const pt_scene_desc* d, pt_bvh_node* out_nodes, int32_t* out_root, int32_t* out_depth, double* out_build_ms) {
    if (!d || !out_nodes || !out_root) return fail(PT_ERR_INVALID_ARG, "bad argument");
    const int N = d->num_shapes;
    if (N <= 0 || !d->nodes || d->num_nodes != 2 * N - 1) return fail(PT_ERR_BAD_SCENE, "needs the leaf boxes of a 2*num_shapes-1 node pool");
    std::vector<float> boxes((size_t)N * 6);
    std::vector<char> seen(N, 0);
    for (int k = 0; k < d->num_nodes; k++) {
        const pt_bvh_node& nd = d->nodes[k];
        if (nd.prim == -1) continue;
        if (nd.prim < 0 || nd.prim >= N || seen[nd.prim]) return fail(PT_ERR_BAD_SCENE, "leaves must cover every shape exactly once");
        seen[nd.prim] = 1;
        std::memcpy(&boxes[(size_t)nd.prim * 6], nd.bmin, 12);
        std::memcpy(&boxes[(size_t)nd.prim * 6 + 3], nd.bmax, 12);
    }
    for (int i = 0; i < N; i++)
        if (!seen[i]) return fail(PT_ERR_BAD_SCENE, "leaves must cover every shape exactly once");
    for (float v : boxes)
        if (!std::isfinite(v)) return fail(PT_ERR_BAD_SCENE, "leaf box is not finite");
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) return fail(PT_ERR_NO_DEVICE, "no HIP device available");
    std::vector<pt_bvh_node> nodes;
    int32_t root = 0, depth = 0;
    int rc = pts::sweep_build_device(boxes.data(), N, nodes, &root, &depth, out_build_ms);
    if (rc) return rc;
    std::memcpy(out_nodes, nodes.data(), nodes.size() * sizeof(pt_bvh_node));
    *out_root = root;
    if (out_depth) *out_depth = depth;
    return PT_OK;
}

int pt_debug_intersect(pt_scene* S, const float* rays, int n, int traversal, float* out_tuv, int32_t* out_prim) {
    if (!S || !rays || !out_tuv || !out_prim || n < 0) return fail(PT_ERR_INVALID_ARG, "bad argument");
    if (n == 0) return PT_OK;
    DeviceGuard guard;
    { int grc = guard.enter(S->device); if (grc) return grc; }
    DevBuf<float> dr, dt;
    DevBuf<int32_t> dp, dn;
    int rc;
    if ((rc = dr.ensure((size_t)n * 8)) || (rc = dt.ensure((size_t)n * 3)) || (rc = dp.ensure(n)) || (rc = dn.ensure(1))) return rc;
    // the tree renders traverse — exact and pruned alike (which_tree): the internal tree with ties settled in the caller's visit
    // order and reference-order reruns when there is one (whatever the scene's size: this kernel reads nodes from global
    // memory), so that the closest hits — ties included — can be checked ray by ray; else the caller's
    const bool fast = S->have_fast && S->opt_fast_tree;
    select_tree(S, fast ? 1 : 0, fast);
    const int cap = fast && S->dev.redo_cap > S->dev.stack_cap ? S->dev.redo_cap : S->dev.stack_cap;
    const uint32_t lds = (uint32_t)(kBlock / 64) * (uint32_t)cap * 64u * 4u;
    hipError_t e = hipMemcpy(dr.p, rays, (size_t)n * 8 * sizeof(float), hipMemcpyHostToDevice);
    if (e == hipSuccess) e = hipMemset(dn.p, 0, sizeof(int32_t));
    if (e == hipSuccess) {
        if (traversal == PT_TRAVERSAL_PRUNED)
            hipLaunchKernelGGL(intersect_kernel<true>, dim3((n + kBlock - 1) / kBlock), dim3(kBlock), lds, nullptr, S->dev, dr.p, n, dt.p, dp.p, dn.p);
        else
            hipLaunchKernelGGL(intersect_kernel<false>, dim3((n + kBlock - 1) / kBlock), dim3(kBlock), lds, nullptr, S->dev, dr.p, n, dt.p, dp.p, dn.p);
        e = hipGetLastError();
    }
    int32_t reruns = 0;
    if (e == hipSuccess) e = hipMemcpy(&reruns, dn.p, sizeof(int32_t), hipMemcpyDeviceToHost);
    if (e == hipSuccess) S->info_debug_reruns = reruns;
    if (e == hipSuccess) e = hipMemcpy(out_tuv, dt.p, (size_t)n * 3 * sizeof(float), hipMemcpyDeviceToHost);
    if (e == hipSuccess) e = hipMemcpy(out_prim, dp.p, (size_t)n * sizeof(int32_t), hipMemcpyDeviceToHost);
    if (e != hipSuccess) return fail(PT_ERR_DEVICE, std::string("pt_debug_intersect: ") + hipGetErrorString(e));
    return PT_OK;
}

}  // extern "C"
