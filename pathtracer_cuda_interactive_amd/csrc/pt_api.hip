// pt_api.hip — kernels and C ABI of libpt_hip.so (gfx950 only).  See include/pt_api.h.
//
// Host half of a live handle: scratch management, kernel selection and launch, guides and queries, the image-space stages,
// options and info, the debug entry points.  The handle and its lifecycle: pt_scene.h, pt_scene_life.hip.  The kernels live
// in pt_kernels.h, the device functions in pt_trace.h / pt_math.h.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <initializer_list>
#include <iterator>
#include <limits>
#include <mutex>
#include <type_traits>

#include "pt_scene.h"
#include "pt_transform.h"
#include "pt_denoise.h"
#include "pt_gradient.h"
#include "pt_temporal.h"
#include "pt_kernels.h"
#include "pt_kernel_q.h"
#include "pt_query.h"

using namespace ptk;

static thread_local std::string g_err;
int pt_fail(int code, const std::string& msg) { g_err = msg; return code; }
static int fail(int code, const std::string& msg) { return pt_fail(code, msg); }

static_assert(ptkc::kBlock == ptk::kBlock && ptkc::kLdsNodeStride == ptk::kLdsNodeStride && ptkc::kCounterStride == ptk::kCounterStride &&
                  ptkc::kQueryRing == ptq::kQueryRing, "pt_scene.h restates these constants of pt_kernels.h / pt_query.h (a -DPT_BLOCK or -DPT_LDS_NODE_STRIDE build changes them there too)");

// every float finite?  (leaf boxes that stayed on the device)
namespace {
__global__ void finite_kernel(const float* __restrict__ v, size_t n, unsigned int* __restrict__ bad) {
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n && !__builtin_isfinite(v[i])) atomicAdd(bad, 1u);
}
}  // namespace
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

constexpr int kProbeRays = 32768;                // pt_scene_create, pt_scene_rebuild: rays that choose between the caller's tree and the internal one

// Inner visits of the probe rays (pt_kernels.h: probe_kernel) through the trees d0 and d1 point at, into v[0] and v[1] (pt_scene.h).
int probe_trees(const SceneDev& d0, const SceneDev& d1, unsigned long long v[2]) {
    DevBuf<unsigned long long> visits;
    if (int rc = visits.ensure(2)) return rc;
    HIP_TRY(hipMemset(visits.p, 0, 2 * sizeof(unsigned long long)));
    const uint32_t lds = (uint32_t)(kBlock / 64) * (uint32_t)std::max(d0.stack_cap, d1.stack_cap) * 64u * 4u;
    hipLaunchKernelGGL(probe_kernel, dim3(kProbeRays / kBlock, 2), dim3(kBlock), lds, nullptr, d0, d1, visits.p);
    HIP_TRY(hipGetLastError());
    v[0] = v[1] = 0;
    HIP_TRY(hipMemcpy(v, visits.p, 2 * sizeof(unsigned long long), hipMemcpyDeviceToHost));
    return PT_OK;
}

namespace {

constexpr uint64_t kDefaultScratchBytes = 8ull << 30;   // per-sample scratch cap (3 % of the 288 GB of HBM): every sample pass
                                                        // pays the launch floor once (buddha stand-in 135.6 ms in 5 passes, 130.6 in 1)
#ifndef PT_TOP_LDS_KB
#define PT_TOP_LDS_KB 26
#endif
constexpr uint32_t kTopLdsBudget = PT_TOP_LDS_KB * 1024;    // LDS per block that keeps 6 blocks per CU resident (160 KB / 6)

uint32_t align16(uint32_t v) { return (v + 15u) & ~15u; }

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
              S->sweep_tab.p && sweep_layout_fits(S->sweep.count, (uint32_t)S->dev.num_prims, (uint32_t)T.num_nodes, kLdsNodeStride) &&
              S->sweep_skip.p && sweep_skip_fits(S->sweep.count, (uint32_t)S->dev.num_prims, (uint32_t)T.num_nodes, kLdsNodeStride);
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
    else if (c.sweep) {
        // options "sweep_pairs", "sweep_families": the tables in class order, or in the groups' own order with every pair general;
        // option "sweep_self_skip": the skip table in that order, or the one of zeros
        const SweepClasses cls = S->sweep_classes_now();
        hipLaunchKernelGGL(reinterpret_cast<SweepFn>(fn), dim3(grid), dim3(c.block_threads), lp.total, stream, S->dev, rd, lp,
                           samples, S->work_counter(), S->counters(),
                           SweepLayoutDev{S->sweep_tab_now(), S->sweep.count, sweep_classes_pitch(cls), cls.pairs, cls.fam, S->sweep_skip_now()});
    } else
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
    ENTER_DEVICE(S);
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
    if (int grc = guard.enter(S->device)) return grc;
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
    ENTER_DEVICE(S);
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
    ENTER_DEVICE(S);
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
    ENTER_DEVICE(S);
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
    ENTER_DEVICE(S);
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
    ENTER_DEVICE(S);
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
    ENTER_DEVICE(S);
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
    ENTER_DEVICE(S);
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
    ENTER_DEVICE(S);
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

// Info keys "<prefix>0" .. "<prefix><count - 1>": *value = a[digit]; false: k is no such key.
bool indexed_key(const std::string& k, const std::string& prefix, int count, const int64_t* a, int64_t* value) {
    const bool hit = k.size() == prefix.size() + 1 && k.compare(0, prefix.size(), prefix) == 0 && k.back() >= '0' && k.back() < '0' + count;
    if (hit) *value = a[k.back() - '0'];
    return hit;
}

}  // namespace

// ------------------------------------------------------------------------------------------
// C ABI
// ------------------------------------------------------------------------------------------
extern "C" {

int pt_api_version(void) { return PT_API_VERSION; }
const char* pt_last_error(void) { return g_err.c_str(); }

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
    ENTER_DEVICE(S);
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
    ENTER_DEVICE(S);
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
    ENTER_DEVICE(S);
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
    ENTER_DEVICE(S);
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
    else if (k == "sweep_pairs") { if (value != 0 && value != 1) return fail(PT_ERR_INVALID_ARG, "sweep_pairs must be 0 or 1"); S->opt_sweep_pairs = value; }
    else if (k == "sweep_families") { if (value != 0 && value != 1) return fail(PT_ERR_INVALID_ARG, "sweep_families must be 0 or 1"); S->opt_sweep_families = value; }
    else if (k == "sweep_self_skip") { if (value != 0 && value != 1) return fail(PT_ERR_INVALID_ARG, "sweep_self_skip must be 0 or 1"); S->opt_sweep_self_skip = value; }
    else if (k == "query_refill") { if (value < 0 || value > 64) return fail(PT_ERR_INVALID_ARG, "query_refill must be 0 (automatic) .. 64"); S->opt_query_refill = value; }
    else if (k == "query_guides") { if (value < 0 || value > 2) return fail(PT_ERR_INVALID_ARG, "query_guides must be 0 (automatic), 1 or 2"); S->opt_query_guides = value; }
    else if (k == "query_blocks") { if (value < 0 || value > 4096) return fail(PT_ERR_INVALID_ARG, "query_blocks must be 0 (automatic) .. 4096"); S->opt_query_blocks = value; }
    else if (k == "tree_cost" || k == "rebuild_at_permille") {
        if (k == "tree_cost" && value != 0 && value != 1) return fail(PT_ERR_INVALID_ARG, "tree_cost must be 0 or 1");
        if (k == "rebuild_at_permille" && value != 0 && value < 1001) return fail(PT_ERR_INVALID_ARG, "rebuild_at_permille must be 0 (never) or at least 1001");
        const bool was_on = S->cost_on();
        (k == "tree_cost" ? S->opt_tree_cost : S->opt_rebuild_at) = value;
        if (!was_on && S->cost_on()) S->cost_forget();    // switched on: references are taken anew (include/pt_api.h)
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
    else if (indexed_key(k, "create_us", 7, S->create_us, value) || indexed_key(k, "update_us", 4, S->update_us, value) ||
             indexed_key(k, "transform_us", 4, S->transform_us, value) || indexed_key(k, "rebuild_us", 4, S->rebuild_us, value)) {}   // stage times (pt_scene.h)
    else if (k == "prev_geometry") *value = S->have_prev ? 1 : 0;         // records from before the last geometry update are kept (pt_render_guides)
    else if (k == "updates") *value = S->updates;                         // successful pt_scene_update calls so far
    else if (k == "groups") *value = S->have_groups ? S->num_groups : 0;  // groups of the assignment pt_scene_set_groups made (0: none)
    else if (k == "rest_geometry") *value = S->have_rest ? 1 : 0;         // a snapshot of the rest records is held (pt_scene_transform)
    else if (k == "transforms") *value = S->transforms;                   // successful pt_scene_transform calls so far
    else if (k == "rebuilds") *value = S->rebuilds;                       // successful pt_scene_rebuild calls so far, a policy's included
    else if (k == "rebuilds_auto") *value = S->rebuilds_auto;             // ... those that option rebuild_at_permille made
    else if (k == "rebuild_adopted") *value = S->rebuild_adopted;         // the last one adopted its tree (1) or kept the one it had (0)
    else if (k == "rebuild_cost_permille") *value = S->rebuild_cost_permille;   // the last candidate's probe ratio (as fast_tree_cost_permille)
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
    else if (k.rfind("sweep_share_pairs", 0) == 0 || k.rfind("sweep_flat_pairs", 0) == 0 || k == "sweep_general_pairs") {
        // the classes a sweep launch of this handle runs under the options "sweep_pairs" and "sweep_families" as they stand; 0: no tables.
        // A PAIR2 is a pair that shares (pt_sweep_families.h: sweep_classes_sharing)
        const SweepClasses c = S->sweep_classes_now();
        const bool flat = k[6] == 'f';
        const std::string axis = k.substr(flat ? 16 : 17);
        if (k == "sweep_general_pairs") *value = c.pairs.general;
        else if (axis.empty()) *value = sweep_classes_sharing(c, flat, -1);
        else if (axis == "_x" || axis == "_y" || axis == "_z") *value = sweep_classes_sharing(c, flat, axis[1] - 'x');
        else return fail(PT_ERR_INVALID_ARG, "unknown info key " + k);
    }
    else if (k == "sweep_pair2_records") *value = sweep_pair2_records(S->sweep_classes_now().fam);      // PAIR2 records of that launch
    else if (k == "sweep_valu_model") *value = sweep_valu_model(S->sweep_classes_now());                // the count model's VALU of its sweep loops
    else if (k == "sweep_skip_groups") *value = S->sweep_skip_info_now().groups;     // groups a bounce can skip under the options as they stand (pt_sweep_skip.h)
    else if (k == "sweep_skip_planes") *value = S->sweep_skip_info_now().planes;     // ... and the distinct planes they lie on
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
            if (int grc = guard.enter(S->device)) return grc;
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

int pt_debug_intersect(pt_scene* S, const float* rays, int n, int traversal, float* out_tuv, int32_t* out_prim) {
    if (!S || !rays || !out_tuv || !out_prim || n < 0) return fail(PT_ERR_INVALID_ARG, "bad argument");
    if (n == 0) return PT_OK;
    ENTER_DEVICE(S);
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
