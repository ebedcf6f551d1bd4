// pt_query.h — the lane-refilling query kernel behind pt_trace_rays and pt_render_guides_async (include/pt_api.h).
//
// The one-shot query kernels (intersect_kernel, aov_kernel: pt_kernels.h) give every lane one ray and run it to completion, so a
// wave lives as long as its slowest ray.  Here a launch is a fixed set of waves that work through the rays of the call: a lane
// that holds no ray takes the next one, so a ray that walks hundreds of nodes holds up one lane and not the other 63.
//
// Per lane and iteration of the wave's loop:
//   1. a lane that holds no ray takes one (below) and starts it: trav_begin, and on a handle that traverses its internal tree the
//      test of intersect_any_tree — a ray whose 1/d is not finite starts on the caller's tree instead;
//   2. one unit of work, the step functions of pt_trace.h as intersect() strings them together: inner_steps while the lane holds
//      an inner node, then one leaf_step if it holds a leaf;
//   3. a lane whose traversal is finished (kDone) stores its result and holds no ray again.
// A lane on the internal tree settles ties on t inside leaf_step (ref_visits_first); a lane on the caller's tree runs
// intersect<false, false>'s steps, whatever the traversal mode — intersect_any_tree's two halves, taken per lane.
//
// Work hand-out.  The rays of a launch are the indices [0, n).  A wave owns a range [cur, end) of them.  Its first range is
// its own: wave w of the grid starts with [w * kQueryChunk, (w + 1) * kQueryChunk), and the launch's counter starts at
// waves * kQueryChunk (set on the launch's stream).  When a lane needs a ray and the range is empty, lane 0 reserves the next
// kQueryChunk indices with one atomicAdd on the counter and the wave reads the old value (readfirstlane); a launch whose first
// ranges cover [0, n) never touches the counter.  The lanes that need a ray take cur + their rank among those lanes (__ballot
// and mbcnt).  The counter is only ever added to and never read in any other way: no lane waits for another wave, and every
// loop ends when a reservation starts at or past n.
// One hot counter word sustains ~88 returning adds per microsecond, and a wave that waits for its add holds 64 lanes.  With a
// reservation per wave to START (measured: 2,400 waves on cbox at 640x480, two adds each) the adds alone took 55 us of a kernel
// whose one-shot twin takes 19; hence the static first ranges.  What is left is one add per kQueryChunk = 64 rays beyond the
// first ranges plus one per wave that finds the end: a 1280x960 frame on 4,096 waves is 19,000 adds, a fifth of a millisecond
// if nothing else took time (on a scene as small as cbox nothing else does).
//
// Every launch needs a counter of its own; the handle keeps a ring of kQueryRing of them (pt_scene.h).
#pragma once

#include "pt_kernels.h"

namespace ptq {

using namespace ptl;
using ptk::kBlock;

constexpr int kQueryChunk = 64;        // ray indices per range (a multiple of 64): info "query_chunk"
constexpr int kQueryRing = 64;         // work counters a handle rotates through, one per launch in flight
constexpr int kQueryRefill = 16;       // idle lanes from which a wave stores results and hands out rays (option "query_refill")
constexpr int kQueryCounterStride = 32;    // uint32 words between two counters of the ring: a 128-B line each

// what a launch traces and where the results go
enum : int { kSrcClosest = 0, kSrcAny = 1, kSrcGuides = 2 };

struct QueryDev {
    uint32_t* counter;              // the launch's work counter, waves * kQueryChunk at its start
    uint32_t n;                     // rays of the launch
    uint32_t refill;                // idle lanes of a wave from which it stores results and hands out rays, 1 .. 64
    const float* rays;              // [n, 8] (the explicit list)
    float* out_tuv;                 // [n, 3] closest
    int32_t* out_prim;              // [n]    closest: primitive or -1; any: 1 / 0
    float* albedo;                  // guides: pt_render_aov's four, any of them null
    float* normal;
    float* depth;
    int32_t* prim;
};

// SRC: kSrcClosest / kSrcAny on the explicit list, kSrcGuides on the pixel-centre camera rays of rp's row selection.
template <int SRC, bool PRUNE, bool MOTION = false>
__global__ __launch_bounds__(kBlock) void query_kernel(SceneDev scn, QueryDev q, RenderDev rp, ptk::MotionDev mo) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    constexpr bool ANY = SRC == kSrcAny;
    ptd::SceneView sv;
    sv.nodes = scn.nodes; sv.prims = scn.prims; sv.normals = scn.normals;
    sv.materials = scn.materials; sv.emission = scn.emission; sv.lights = scn.lights;
    sv.top_nodes = nullptr; sv.top_count = 0;
    sv.node_stride = sizeof(DNode); sv.oct_stride = 0;
    sv.num_emission = scn.num_emission; sv.root_ref = scn.root_ref; sv.fixed_order = scn.fixed_order;
    sv.ref_nodes = scn.ref_nodes; sv.ref_path = scn.ref_path; sv.ref_anc = scn.ref_anc; sv.ref_levels = scn.ref_levels;
    sv.bg = ptm::mk(0, 0, 0);
    ptd::SceneView sv_ref = sv;                                      // the caller's tree, where the handle traverses its internal one
    sv_ref.nodes = scn.ref_nodes; sv_ref.root_ref = scn.ref_root_ref; sv_ref.fixed_order = 0;
    const bool fallback = scn.fallback != 0;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int cap = scn.fallback && scn.redo_cap > scn.stack_cap ? scn.redo_cap : scn.stack_cap;   // one column serves both trees
    int32_t* stk = reinterpret_cast<int32_t*>(smem) + (size_t)wave * cap * 64 + lane;
    const ptd::LdsStack<int32_t> s{stk};
    ptd::stack_init(stk);                                 // entry 0 stays the done value: pushes start at entry 1

    ptd::Ray ray{};
    ptd::Trav t{};
    uint32_t idx = 0;
    bool have = false;                                    // this lane holds ray idx
    bool on_ref = false;                                  // ... and traces it on the caller's tree in the reference's order
    // the wave's range of ray indices (uniform): first its own
    const uint32_t waves = gridDim.x * (uint32_t)(kBlock / 64);
    const uint32_t first = (blockIdx.x * (uint32_t)(kBlock / 64) + (uint32_t)wave) * (uint32_t)kQueryChunk;
    uint32_t cur = first < q.n ? first : q.n;
    uint32_t end = first + (uint32_t)kQueryChunk < q.n ? first + (uint32_t)kQueryChunk : q.n;
    const bool all_static = (uint64_t)waves * (uint64_t)kQueryChunk >= (uint64_t)q.n;   // the first ranges cover the launch
    bool drained = false;                                 // no index is left for this wave (uniform)

    for (;;) {
        const bool done = have && t.cur == kDone;
        const unsigned long long idle = __ballot(!have || done);
        // results are stored and rays handed out for q.refill lanes at a time (the tail of a wave: for all that are left), so
        // that the code around a traversal — the ray's set-up, the guide rule — runs on that many lanes, not on one
        if ((uint32_t)__popcll(idle) >= q.refill) {
            if (done) {
                const ptd::Hit h = t.best;
                if (SRC == kSrcGuides) {
                    ptk::write_guides<MOTION>(sv, rp, ray, h, idx, q.albedo, q.normal, q.depth, q.prim, mo);
                } else if (ANY) {
                    q.out_prim[idx] = h.prim >= 0 ? 1 : 0;
                } else {
                    q.out_prim[idx] = h.prim;
                    q.out_tuv[3 * (size_t)idx] = h.prim < 0 ? 0.0f : h.t;
                    q.out_tuv[3 * (size_t)idx + 1] = h.prim < 0 ? 0.0f : h.u;
                    q.out_tuv[3 * (size_t)idx + 2] = h.prim < 0 ? 0.0f : h.v;
                }
                have = false;
            }
            if (!drained) {
                if (cur == end) {
                    uint32_t base = q.n;
                    if (!all_static) {
                        if (lane == 0) base = atomicAdd(q.counter, (uint32_t)kQueryChunk);
                        base = (uint32_t)__builtin_amdgcn_readfirstlane((int)base);
                    }
                    if (base >= q.n) {
                        drained = true;
                    } else {
                        cur = base;
                        end = base + (uint32_t)kQueryChunk < q.n ? base + (uint32_t)kQueryChunk : q.n;
                    }
                }
                if (!drained) {
                    // (a lane the range has no index left for asks again on the wave's next hand-out)
                    const uint32_t avail = end - cur, rank = ptk::lane_rank(idle), wanted = (uint32_t)__popcll(idle);
                    if (!have && rank < avail) {
                        have = true;
                        idx = cur + rank;
                        if (SRC == kSrcGuides) {
                            const uint32_t row = fastdiv(idx, rp.div_width);
                            const int i = (int)(idx - row * (uint32_t)rp.width);
                            const int j = rp.row_begin + (int)row * rp.row_step;
                            const float u = ((float)i + 0.5f) / (float)rp.width;
                            const float v = ((float)j + 0.5f) / (float)rp.height;
                            ray = ptd::primary_ray(rp, u, v);
                        } else {
                            const float* rr = q.rays + 8 * (size_t)idx;         // (4-byte aligned is all the caller owes)
                            ray.org = ptm::mk(rr[0], rr[1], rr[2]);
                            ray.dir = ptm::mk(rr[3], rr[4], rr[5]);
                            ray.tnear = rr[6];
                            ray.tfar = rr[7];
                        }
                        ptd::trav_begin(sv, ray, t, s);
                        on_ref = fallback && !(__builtin_isfinite(t.inv.x) && __builtin_isfinite(t.inv.y) && __builtin_isfinite(t.inv.z));
                        if (on_ref) ptd::trav_begin(sv_ref, ray, t, s);
                    }
                    cur += wanted < avail ? wanted : avail;
                }
            }
            if (drained && idle == ~0ull) break;
        }

        if (have && t.cur != kDone) {
            // this lane's tree: the node table, the visit order, and whether it prunes
            ptd::SceneView svl = sv;
            svl.nodes = on_ref ? sv_ref.nodes : sv.nodes;
            svl.fixed_order = on_ref ? 0 : sv.fixed_order;
            while (t.cur >= 0) {
                if (PRUNE && !ANY && !on_ref) ptd::inner_step<true, false>(svl, ray.org, t, s);
                else ptd::inner_step<false, false>(svl, ray.org, t, s);
            }
            if (t.cur != kDone) ptd::leaf_step<false, ANY>(svl, ray, t, s, ANY, !ANY && fallback && !on_ref);
        }
    }
}

}  // namespace ptq
