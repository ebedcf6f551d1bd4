// pt_scene_life.hip — the lifecycle of a scene handle (libpt_hip.so, gfx950 only).  See include/pt_api.h.
//
// pt_scene_create in stages (validate_and_build), the three ways to change a live scene — pt_scene_update, pt_scene_transform
// (with pt_scene_set_groups), pt_scene_rebuild —, pt_scene_destroy, and the two stand-alone tree builders.  Host code; every kernel is pt_api.hip's (pt_scene.h says why).
#include <cmath>
#include <cstdlib>
#include <cstring>
#include <exception>
#include <limits>
#include <queue>

#include "pt_scene.h"
#include "pt_tree_sweep.h"
#include "pt_sweep_build.h"
#include "pt_scene_prep.h"
#include "pt_tree_cost.h"
#include "pt_scene_transform.h"
#include "pt_transform.h"
#include "pt_sweep_layout.h"
#include "pt_sweep_families.h"
#include "pt_sweep_skip.h"
#include "pt_sweep_pairs.h"

namespace {
using namespace ptkc;

constexpr uint32_t kOctNodeLimit = 24 * 1024;    // 8 octant copies of the node table must fit in this many bytes of LDS
constexpr int kMaxStack = 64;                    // the reference's own cap (scene.h:251)
constexpr int kMinInternalTree = 16;              // primitives below which no internal tree is built (a handful of nodes either way: scene1, 4 shapes, is 6 % slower with one)
constexpr int kDeviceSweepMin = 4096;             // primitives from which the internal tree is built on the device (below: a few ms on the host either way)
#ifndef PT_TOP_NODES
#define PT_TOP_NODES 512
#endif
constexpr uint32_t kTopNodes = PT_TOP_NODES;     // scenes read from global memory: this many nodes are numbered breadth-first from the root, so that [0, k) is the top of the tree for every k (LDS cache)
constexpr uint32_t kMaxLdsBudget = 160 * 1024;               // the breadth-first numbered prefix is sized for the largest budget an option may ask for

// Scenes of kDeviceSweepMin primitives and more are prepared on the device — records, both trees, tie tables — unless
// PT_SWEEP_BUILD=host in the environment keeps the work on the host (A/B timing, debugging)
bool prepared_on_device(int N) {
    const char* v = std::getenv("PT_SWEEP_BUILD");
    return N >= kDeviceSweepMin && !(v && std::string(v) == "host");
}

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
        if (!leaf_ok(rootn)) return pt_fail(PT_ERR_BAD_SCENE, "leaf primitive id out of range");
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
            if (++visited > (size_t)num_nodes) return pt_fail(PT_ERR_BAD_SCENE, "BVH is not a tree (cycle)");
            if (inner_id[it.ref_node] != -1) return pt_fail(PT_ERR_BAD_SCENE, "BVH node referenced twice");
            if (nd.left < 0 || nd.left >= num_nodes || nd.right < 0 || nd.right >= num_nodes)
                return pt_fail(PT_ERR_BAD_SCENE, "BVH child index out of range");
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
                    if (!leaf_ok(*ch)) return pt_fail(PT_ERR_BAD_SCENE, "leaf primitive id out of range");
                    if (prim_seen[ch->prim]) return pt_fail(PT_ERR_BAD_SCENE, "primitive referenced by two leaves");
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
        if (!prim_seen[i]) return pt_fail(PT_ERR_BAD_SCENE, "primitive not covered by any leaf");
    if (!internal && depth - 1 > kMaxStack - 1)
        return pt_fail(PT_ERR_BAD_SCENE, "BVH deeper than the traversal stack (reference cap 64, scene.h:251)");
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
            return pt_fail(PT_ERR_BAD_SCENE, "unknown material type (scene.h:410 asserts)");
    return PT_OK;
}
int check_meshes(const pt_scene_desc* d, int num_materials) {
    for (int m = 0; m < d->num_meshes; m++) {
        const pt_mesh& me = d->meshes[m];
        if (me.num_vertices <= 0 || me.num_faces <= 0 || !me.positions || !me.indices)
            return pt_fail(PT_ERR_BAD_SCENE, "empty mesh");
        if (!me.normals) return pt_fail(PT_ERR_BAD_SCENE, "mesh without vertex normals (required, SURVEY H5a)");
        if (me.material_id < 0 || me.material_id >= num_materials) return pt_fail(PT_ERR_BAD_SCENE, "mesh material id out of range");
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
    emis.assign(std::max(d->num_lights, 1), DEmission{});          // (no padding in either record)
    dlights.assign(std::max(d->num_lights, 1), DLight{});
    for (int l = 0; l < d->num_lights; l++) {
        const pt_light& src = d->lights[l];
        emis[l] = DEmission{src.radiance[0], src.radiance[1], src.radiance[2], src.type == PT_LIGHT_DIFFUSE_AREA ? 1 : 0};
        dlights[l] = DLight{src.radiance[0], src.radiance[1], src.radiance[2], src.type == PT_LIGHT_DIFFUSE_AREA ? 1 : 0,
                            src.position[0], src.position[1], src.position[2], src.shape_id};
        if (src.type == PT_LIGHT_DIFFUSE_AREA && (src.shape_id < 0 || src.shape_id >= N))
            return pt_fail(PT_ERR_BAD_SCENE, "area light refers to a shape that does not exist");
    }
    return PT_OK;
}
// One DPrim (+ DNormals) per shape, gathered from the meshes on the host: the twin of ptp::prims_device, ids checked with the
// same messages.  *tri_only: the scene holds no sphere.
int pack_prims_host(const pt_scene_desc* d, std::vector<DPrim>& prims, std::vector<DNormals>& normals, bool* tri_only) {
    const int N = d->num_shapes;
    prims.resize(N);
    normals.resize(N);
    std::memset(prims.data(), 0, sizeof(DPrim) * N);
    std::memset(normals.data(), 0, sizeof(DNormals) * N);
    *tri_only = true;
    for (int i = 0; i < N; i++) {
        const pt_shape& s = d->shapes[i];
        DPrim& p = prims[i];
        if (s.type == PT_SHAPE_SPHERE) {
            if (s.material_id < 0 || s.material_id >= d->num_materials) return pt_fail(PT_ERR_BAD_SCENE, "sphere material id out of range");
            p.v[0] = s.center[0]; p.v[1] = s.center[1]; p.v[2] = s.center[2]; p.v[3] = s.radius;
            p.info = (int32_t)(0x80000000u | (uint32_t)s.material_id);
            p.light = s.area_light_id;
            *tri_only = false;
        } else if (s.type == PT_SHAPE_TRIANGLE) {
            if (s.mesh_index < 0 || s.mesh_index >= d->num_meshes) return pt_fail(PT_ERR_BAD_SCENE, "triangle mesh index out of range");
            const pt_mesh& me = d->meshes[s.mesh_index];
            if (s.face_index < 0 || s.face_index >= me.num_faces) return pt_fail(PT_ERR_BAD_SCENE, "triangle face index out of range");
            const int32_t* idx = me.indices + 3 * (size_t)s.face_index;
            for (int k = 0; k < 3; k++) {
                if (idx[k] < 0 || idx[k] >= me.num_vertices) return pt_fail(PT_ERR_BAD_SCENE, "vertex index out of range");
                for (int c = 0; c < 3; c++) {
                    p.v[3 * k + c] = me.positions[3 * (size_t)idx[k] + c];
                    normals[i].n[3 * k + c] = me.normals[3 * (size_t)idx[k] + c];
                }
            }
            p.info = me.material_id;
            p.light = me.area_light_id;
        } else {
            return pt_fail(PT_ERR_BAD_SCENE, "unknown shape type");
        }
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
        if (int r = T.nodes_oct.ensure(nodes_oct.size())) return r;
        HIP_TRY(hipMemcpy(T.nodes_oct.p, nodes_oct.data(), nodes_oct.size() * sizeof(DNode), hipMemcpyHostToDevice));
        T.have_oct = true;
    }
    if (int r = T.nodes.ensure(nodes.size())) return r;
    HIP_TRY(hipMemcpy(T.nodes.p, nodes.data(), nodes.size() * sizeof(DNode), hipMemcpyHostToDevice));
    T.num_nodes = (int32_t)nodes.size(); T.root_ref = H.root_ref; T.top_avail = H.top_avail; T.depth = H.depth;
    T.stack_cap = H.stack_need + 1;                         // + the kDone sentinel at the bottom
    return PT_OK;
}
// The metadata of a tree that ptp::relay_tree_device has written into T.nodes.
void relaid_tree(pt_scene::Tree& T, int N, const ptp::RelayResult& r) {
    T.have_oct = false; T.num_nodes = N - 1; T.root_ref = 0; T.stack_cap = r.stack_need + 1; T.top_avail = r.top_avail; T.depth = r.depth;
}

// A candidate for tree[1]: where the device built it, `tree` holds it; where the host did, `host` holds it and upload_tree
// brings it into `tree` when the caller is ready to.  copy_error: the leaf boxes did not come down to the host builder.
struct InternalTree {
    pt_scene::Tree tree;
    TreeHost host;
    bool ok = false, on_device = false;
    hipError_t copy_error = hipSuccess;
};

// The sweep tree of N leaf boxes, which come in device memory, in host memory or both (null: not there), and the one decision
// between its two builders.  Boxes on the device go to the device builder (pt_sweep_build.hip, re-laid by pt_scene_prep.hip)
// where scenes of N shapes are prepared there; what it hands back (its depth guard, a failure) and everything else goes to the
// host builder (pt_tree_sweep.h, re-laid by convert_tree), the boxes copied down where they have to be.  built(again) runs when
// a builder has finished, before the re-layout — again: the host builder has taken over from the device's — and owns the stage times.
template <class Built>
InternalTree internal_tree(const float* boxes_dev, const float* boxes_host, int N, Built built) {
    InternalTree c;
    const bool try_device = boxes_dev && prepared_on_device(N);
    if (try_device) {
        DevBuf<pt_bvh_node> fpool_dev; DevBuf<int32_t> fiop_dev;
        int32_t fdepth = 0; double dev_ms = 0;
        const size_t pool_nodes = 2 * (size_t)N - 1;
        const bool ok = !fpool_dev.ensure(pool_nodes) && !fiop_dev.ensure(pool_nodes) && !c.tree.nodes.ensure((size_t)N - 1) &&
                        boxes_finite_device(boxes_dev, (size_t)N * 6) &&
                        pts::sweep_build_on_device(boxes_dev, N, fpool_dev.p, &fdepth, &dev_ms) == PT_OK;
        built(false);
        ptp::RelayResult r1;
        c.ok = c.on_device = ok && ptp::relay_tree_device(fpool_dev.p, (int)pool_nodes, 0, N, true, c.tree.nodes.p, fiop_dev.p, nullptr, kBlock,
                                                          kTopNodes, kMaxLdsBudget, &r1) == PT_OK && r1.nested;
        if (c.ok) { relaid_tree(c.tree, N, r1); return c; }
        (void)hipGetLastError();
        c.tree.nodes.release();
    }
    std::vector<float> copy(boxes_host ? 0 : (size_t)N * 6);
    if (!boxes_host) {
        c.copy_error = hipMemcpy(copy.data(), boxes_dev, copy.size() * sizeof(float), hipMemcpyDeviceToHost);
        if (c.copy_error != hipSuccess) return c;
        boxes_host = copy.data();
    }
    for (size_t k = 0; k < (size_t)N * 6; k++)
        if (!std::isfinite(boxes_host[k])) return c;
    std::vector<pt_bvh_node> fnodes;
    int32_t froot = 0, fdepth = 0;
    bool ok = true, fnested = true;
    try {
        pts::build_sweep_tree(boxes_host, N, fnodes, &froot, &fdepth);
    } catch (const std::exception&) {        // out of host memory: the caller's tree serves alone
        ok = false;
    }
    built(try_device);
    c.ok = ok && convert_tree(fnodes.data(), (int)fnodes.size(), froot, N, c.host, nullptr, &fnested, true) == PT_OK && fnested;
    return c;
}

// pt_scene_create keeps no internal tree after all: tree[1] and the tie tables go, `why` is what pt_scene_rebuild will say.
void drop_internal_tree(pt_scene* S, const char* why) {
    S->have_fast = S->fast_is_callers_topology = false;
    S->no_fast_why = why;
    S->tree[1].nodes.release(); S->tree[1].nodes_oct.release(); S->tree[1].have_oct = false;
    S->ref_path.release(); S->ref_anc.release();
}

int64_t probe_permille(const unsigned long long v[2]) { return v[0] ? (int64_t)((1000ull * v[1] + v[0] / 2) / v[0]) : 1000; }
bool probe_wins(const unsigned long long v[2]) { return v[1] * 100ull < v[0] * 90ull; }   // at least 10 % fewer boxes

// The leaf sweep's groups of equal leaf boxes (pt_leaf_sweep.h) and its tables (pt_sweep_layout.h) from an internal tree as the
// host built it; prims: the N <= kSweepMaxPrims records on the host.  groups = 0: none; sweep.count stays 0 where a launch
// would not admit them.  The tables are made twice: in the groups' own order with every pair general (sweep_tab), and in the
// class order (sweep_tab_pairs, classes), once per value of option "sweep_families" (pt_sweep_families.h; [0]: the pair classes
// of pt_sweep_pairs.h alone); options "sweep_pairs" and "sweep_families" choose among them at a launch.  Each of the three has
// its skip table (pt_sweep_skip.h) in its own group order, in sweep_skip behind a table of zeros (option "sweep_self_skip").
int make_sweep_tables(const TreeHost& fast, const DPrim* prims, int N, SweepTable& sweep, int& sweep_groups, DevBuf<unsigned char>& sweep_tab,
                      DevBuf<unsigned char> (&sweep_tab_pairs)[2], SweepClasses (&classes)[2], DevBuf<unsigned char>& sweep_skip,
                      SweepSkipInfo (&skip_info)[3]) {
    sweep = SweepTable{};
    sweep_groups = 0;
    for (SweepClasses& c : classes) c = SweepClasses{};
    for (SweepSkipInfo& i : skip_info) i = SweepSkipInfo{0, 0};
    SweepGroup groups[kSweepMaxPrims];
    const int n = build_sweep_groups(fast.nodes.data(), (int)fast.nodes.size(), N, kLdsNodeStride, groups);
    if (n > 0) {
        sweep_groups = n;
        std::vector<unsigned char> tab(n <= kSweepMaxBoxes ? sweep_layout_bytes((uint32_t)n, (uint32_t)N) : 0);
        SweepGroup paired[kSweepMaxBoxes];
        int perm[kSweepMaxBoxes];
        SweepClasses cls[2] = {};
        std::vector<unsigned char> tab_pairs[2];
        std::vector<unsigned char> skip(4 * (size_t)kSweepSkipTableBytes, 0);      // [0] stays zero
        SweepSkipInfo si[3] = {};
        const DNode* nodes = fast.nodes.data();
        const int num_nodes = (int)fast.nodes.size();
        bool ok = n <= kSweepMaxBoxes && build_sweep_layout(groups, n, nodes, num_nodes, kLdsNodeStride, prims, N, tab.data()) &&
                  build_sweep_skip(groups, n, nodes, num_nodes, kLdsNodeStride, prims, N, skip.data() + kSweepSkipTableBytes, &si[0]);
        for (int m = 0; ok && m < 2; m++) {
            tab_pairs[m].resize(tab.size());
            ok = build_sweep_families(groups, n, nodes, num_nodes, kLdsNodeStride, m, paired, perm, &cls[m]) &&
                 build_sweep_layout(paired, n, nodes, num_nodes, kLdsNodeStride, prims, N, tab_pairs[m].data()) &&
                 build_sweep_family_tables(paired, n, cls[m], nodes, num_nodes, kLdsNodeStride, tab_pairs[m].data()) &&
                 build_sweep_skip(paired, n, nodes, num_nodes, kLdsNodeStride, prims, N, skip.data() + (2 + m) * (size_t)kSweepSkipTableBytes, &si[1 + m]);
        }
        // every table a launch can choose must hold the kernel's record stream, its read past the last record included
        // (pt_sweep_families.h: sweep_stream_fits).  A table is at most its pitch long and a scene has a primitive, so the end
        // is at most 32 bytes into the first slot record: a table that fails this is a bug in the layout, not a scene to decline
        if (ok && !(sweep_stream_fits(sweep_classes_of_pairs(sweep_pairs_none((uint32_t)n)), (uint32_t)n, (uint32_t)N) &&
                    sweep_stream_fits(cls[0], (uint32_t)n, (uint32_t)N) && sweep_stream_fits(cls[1], (uint32_t)n, (uint32_t)N)))
            return pt_fail(PT_ERR_UNSUPPORTED, "sweep tables: the record stream would read past the staged sweep region");
        if (ok) {
            if (int rc = sweep_tab.ensure(tab.size())) return rc;
            HIP_TRY(hipMemcpy(sweep_tab.p, tab.data(), tab.size(), hipMemcpyHostToDevice));
            for (int m = 0; m < 2; m++) {
                if (int rc = sweep_tab_pairs[m].ensure(tab_pairs[m].size())) return rc;
                HIP_TRY(hipMemcpy(sweep_tab_pairs[m].p, tab_pairs[m].data(), tab_pairs[m].size(), hipMemcpyHostToDevice));
                classes[m] = cls[m];
            }
            if (int rc = sweep_skip.ensure(skip.size())) return rc;
            HIP_TRY(hipMemcpy(sweep_skip.p, skip.data(), skip.size(), hipMemcpyHostToDevice));
            std::copy(si, si + 3, skip_info);
            sweep.count = (uint32_t)n;
            std::copy(groups, groups + n, sweep.g);
        }
    }
    return PT_OK;
}

// ---- pt_scene_create: the stages of validate_and_build, in its order ----------------------------------------------------------
// 1: the description as a whole
int check_desc(const pt_scene_desc* d) {
    if (!d) return pt_fail(PT_ERR_INVALID_ARG, "null scene description");
    if (d->num_shapes <= 0 || !d->shapes) return pt_fail(PT_ERR_BAD_SCENE, "scene has no shapes");
    if (d->num_nodes != 2 * d->num_shapes - 1 || !d->nodes)
        return pt_fail(PT_ERR_BAD_SCENE, "BVH must have 2*num_shapes-1 nodes (bvh.cu:16-54)");
    if (d->root < 0 || d->root >= d->num_nodes) return pt_fail(PT_ERR_BAD_SCENE, "BVH root out of range");
    if (d->num_materials <= 0 || !d->materials) return pt_fail(PT_ERR_BAD_SCENE, "scene has no materials");
    if (d->num_meshes < 0 || (d->num_meshes > 0 && !d->meshes)) return pt_fail(PT_ERR_BAD_SCENE, "bad mesh array");
    if (d->num_lights < 0 || (d->num_lights > 0 && !d->lights)) return pt_fail(PT_ERR_BAD_SCENE, "bad light array");
    if (int rc = check_materials(d)) return rc;
    return check_meshes(d, d->num_materials);
}

// What create's stages hand on.  on_device (prepared_on_device): records and trees are made in device memory and the host vectors stay empty, or the other way round.
struct CreateState {
    bool on_device = false, nested = true;                                      // nested: every box of the caller's tree contains its children's
    std::vector<DPrim> prims; std::vector<DNormals> normals;                    // 2: the records on the host
    TreeHost ref; std::vector<float> boxes_host; DevBuf<float> boxes_dev;       // 3: the caller's tree as the host converted it; the leaf boxes [N][6]
    DevBuf<pt_bvh_node> pool_dev; DevBuf<int32_t> iop_dev;                      //    the caller's pool and the map pool index -> DNode index (tie tables)
    int ref_depth = 0; size_t ref_inner = 0;
    InternalTree cand;                                                          // 4: the candidate for tree[1]
};

// 3: the caller's tree, validated and re-laid — on the host (convert_tree; stage 5 uploads it) or on the device, where the pool
// goes up once and is checked and re-laid into S->tree[0] there (pt_scene_prep.hip: PT_ERR_BAD_SCENE with the host path's messages)
int callers_tree(const pt_scene_desc* d, pt_scene* S, CreateState& c) {
    const int N = d->num_shapes;
    int rc;
    if (!c.on_device) {
        c.boxes_host.resize((size_t)N * 6);
        if ((rc = convert_tree(d->nodes, d->num_nodes, d->root, N, c.ref, c.boxes_host.data(), &c.nested))) return rc;
        c.ref_depth = c.ref.depth; c.ref_inner = c.ref.nodes.size();
        return PT_OK;
    }
    ptp::RelayResult r0;
    if ((rc = c.pool_dev.ensure((size_t)d->num_nodes)) || (rc = c.iop_dev.ensure((size_t)d->num_nodes)) || (rc = c.boxes_dev.ensure((size_t)N * 6)) ||
        (rc = S->tree[0].nodes.ensure((size_t)N - 1)))
        return rc;
    HIP_TRY(hipMemcpy(c.pool_dev.p, d->nodes, (size_t)d->num_nodes * sizeof(pt_bvh_node), hipMemcpyHostToDevice));
    if ((rc = ptp::relay_tree_device(c.pool_dev.p, d->num_nodes, d->root, N, false, S->tree[0].nodes.p, c.iop_dev.p, c.boxes_dev.p, kBlock,
                                     kTopNodes, kMaxLdsBudget, &r0)))
        return rc;
    relaid_tree(S->tree[0], N, r0);
    c.nested = r0.nested != 0; c.ref_depth = r0.depth; c.ref_inner = (size_t)N - 1;
    return PT_OK;
}

// 5: shading tables, what the host made of records and trees, and the kernel argument block
int upload_scene(const pt_scene_desc* d, pt_scene* S, CreateState& c) {
    const int N = d->num_shapes;
    std::vector<DMaterial> mats; std::vector<DEmission> emis; std::vector<DLight> dlights;
    int rc;
    if ((rc = pack_shading(d, N, mats, emis, dlights))) return rc;
    if (!c.on_device && (rc = upload_tree(S->tree[0], c.ref))) return rc;
    if (c.cand.ok) {
        if (!c.cand.on_device && (rc = upload_tree(c.cand.tree, c.cand.host))) return rc;
        std::swap(S->tree[1], c.cand.tree);
    }
    S->have_fast = c.cand.ok;
    if (!c.on_device && ((rc = S->prims.ensure(c.prims.size())) || (rc = S->normals.ensure(c.normals.size())))) return rc;
    if ((rc = S->materials.ensure(mats.size())) || (rc = S->emission.ensure(emis.size())) || (rc = S->lights.ensure(dlights.size()))) return rc;
    HIP_TRY(hipMemcpy(S->lights.p, dlights.data(), dlights.size() * sizeof(DLight), hipMemcpyHostToDevice));
    if (!c.on_device) {
        HIP_TRY(hipMemcpy(S->prims.p, c.prims.data(), c.prims.size() * sizeof(DPrim), hipMemcpyHostToDevice));
        HIP_TRY(hipMemcpy(S->normals.p, c.normals.data(), c.normals.size() * sizeof(DNormals), hipMemcpyHostToDevice));
    }
    HIP_TRY(hipMemcpy(S->materials.p, mats.data(), mats.size() * sizeof(DMaterial), hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(S->emission.p, emis.data(), emis.size() * sizeof(DEmission), hipMemcpyHostToDevice));
    SceneDev& dv = S->dev;
    dv.prims = S->prims.p; dv.normals = S->normals.p;
    dv.materials = S->materials.p; dv.emission = S->emission.p; dv.lights = S->lights.p;
    dv.num_prims = N; dv.num_materials = d->num_materials; dv.num_emission = d->num_lights;
    dv.bg[0] = d->background[0]; dv.bg[1] = d->background[1]; dv.bg[2] = d->background[2];
    return PT_OK;
}

// 6: keep the internal tree only where it is the better one FOR THIS KIND OF RAY: without pruning a node is visited iff the ray hits
// its box, and what the boxes of a tree add up to depends on the scene (a soup of large overlapping triangles is better off with the
// caller's median splits than with cuts of the Morton order; a far-away ground sphere skews any surface-area estimate).  So measure:
// the same probe rays — from random points on the primitives into uniform directions, where and how the segments after the first bounce start — through both trees, inner visits counted.
int probe_and_decide(const pt_scene_desc* d, pt_scene* S, size_t ref_inner) {
    S->fast_cost_permille = 0;
    if (!S->have_fast) return PT_OK;
    const int N = d->num_shapes;
    int rc;
    select_tree(S, 0);
    const SceneDev d0 = S->dev;
    select_tree(S, 1);
    const SceneDev d1 = S->dev;
    unsigned long long v[2] = {0, 0};
    if ((rc = probe_trees(d0, d1, v))) return rc;
    S->fast_cost_permille = probe_permille(v);
    if (probe_wins(v)) return PT_OK;
    // not at least 10 % fewer boxes: the sweep tree is not worth having
    drop_internal_tree(S, "the sweep tree lost the probe on an LDS-resident scene");
    // ... but the way the internal tree is TRAVERSED still is, for scenes in global memory: left child first with the children ordered
    // for a short stack, leaves set aside, ties settled in place.  So the caller's own topology becomes the internal tree (a caller
    // who hands in a tree as good as the sweep tree: 5.43 -> 4.9 ms on bunny, profiles/r02_device_bvh_build.log).
    const bool global_scene = (size_t)N * (sizeof(DPrim) + sizeof(DNormals)) + ref_inner * sizeof(DNode) > kLdsSceneLimit;
    if (global_scene) {
        TreeHost own;
        bool own_nested = true;
        if (convert_tree(d->nodes, d->num_nodes, d->root, N, own, nullptr, &own_nested, true) == PT_OK && own_nested) {
            if ((rc = upload_tree(S->tree[1], own))) return rc;
            S->have_fast = S->fast_is_callers_topology = true;
        }
    }
    return PT_OK;
}

// 7: what settles ties on t in the caller's visit order: every primitive's path from the caller's root (turn bits) and the
// inner nodes along it.  (Depth <= 64 levels of leaves and inner nodes: at most 63 turns.)  The host's walk, beside
// ptp::tie_tables_device; inner_of_pool: convert_tree's map of the caller's pool.
int tie_tables_host(const pt_scene_desc* d, const std::vector<int32_t>& inner_of_pool, int levels, unsigned long long* path_dev, int32_t* anc_dev) {
    const int N = d->num_shapes;
    std::vector<unsigned long long> path(N, 0ull);
    std::vector<int32_t> anc((size_t)N * (size_t)levels, 0);
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
        trail[w.level] = inner_of_pool[w.node];
        // depth-first, left subtree first: `trail` below w.level is still this node's path when its right child is taken up
        todo.push_back({nd.right, w.level + 1, w.turns | (1ull << w.level)});
        todo.push_back({nd.left, w.level + 1, w.turns});
    }
    HIP_TRY(hipMemcpy(path_dev, path.data(), path.size() * sizeof(unsigned long long), hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(anc_dev, anc.data(), anc.size() * sizeof(int32_t), hipMemcpyHostToDevice));
    return PT_OK;
}
int tie_tables(const pt_scene_desc* d, pt_scene* S, const CreateState& c) {
    if (!S->have_fast) return PT_OK;
    const int N = d->num_shapes;
    const int levels = std::max(c.ref_depth - 1, 1);
    const size_t anc_words = (size_t)N * (size_t)levels;
    if (S->ref_path.ensure((size_t)N) || S->ref_anc.ensure(anc_words)) {
        // no room for the tables (num_shapes x depth words): the scene simply keeps to the caller's tree
        (void)hipGetLastError();
        drop_internal_tree(S, "there was no room for the tie tables");
        return PT_OK;
    }
    if (c.on_device) {
        // on the device: every leaf of the caller's pool (uploaded in stage 3) walks to the root (pt_scene_prep.hip) — a depth-first
        // walk over a million leaves writing a 100 MB table is 150 ms of host time, and the table would have to be uploaded
        DevBuf<int32_t> parent_dev;
        const bool made = !parent_dev.ensure((size_t)d->num_nodes) && hipMemset(S->ref_anc.p, 0, anc_words * sizeof(int32_t)) == hipSuccess &&
                          ptp::tie_tables_device(c.pool_dev.p, d->num_nodes, d->root, c.iop_dev.p, N, levels, parent_dev.p, S->ref_path.p, S->ref_anc.p) == PT_OK;
        if (!made) return pt_fail(PT_ERR_DEVICE, "tie tables on the device failed");
    } else if (int rc = tie_tables_host(d, c.ref.inner_of_pool, levels, S->ref_path.p, S->ref_anc.p)) return rc;
    S->ref_levels = levels;
    return PT_OK;
}

// pt_scene_create's order of events.  The host halves serve small scenes, PT_SWEEP_BUILD=host, and what the device builder hands back.
int validate_and_build(const pt_scene_desc* d, pt_scene* S) {
    int rc;
    if ((rc = check_desc(d))) return rc;                                            // 1
    StageClock clock;
    const int N = d->num_shapes;
    CreateState c;
    c.on_device = prepared_on_device(N);
    if (c.on_device) {                                                              // 2: primitive records, on the device or for stage 5 to upload
        int has_sphere = 0;
        if ((rc = S->prims.ensure((size_t)N)) || (rc = S->normals.ensure((size_t)N)) || (rc = ptp::prims_device(d, S->prims.p, S->normals.p, &has_sphere))) return rc;
        S->tri_only = !has_sphere;
    } else if ((rc = pack_prims_host(d, c.prims, c.normals, &S->tri_only))) return rc;
    S->diffuse_only = all_diffuse(d);
    S->create_us[1] = clock.lap();
    if ((rc = callers_tree(d, S, c))) return rc;                                    // 3
    S->create_us[2] = clock.lap();
    // 4: the internal tree over the same leaf boxes.  A leaf is tested by the reference iff the ray hits every box on its way
    // down (scene.h:278-297, no pruning).  The slab test is monotone in the box (rounding is), so where every box contains its
    // children's that is: iff it hits the LEAF's own box — whatever the tree above it.  `nested` says the caller's tree is of
    // that kind; then any tree over the same leaf boxes tests the same leaves, and only the ORDER of the tests (ties on t,
    // scene.h:270) still depends on the tree.  The tree: all cuts along x, y and z at every node (pt_tree_sweep.h), as deep as
    // it likes — traversed left child first, its stack need is its Strahler number, not its depth (convert_tree).
    if (N < kMinInternalTree) {
        S->no_fast_why = "fewer than 16 shapes";
    } else if (!c.nested) {
        S->no_fast_why = "the caller's boxes do not nest";
    } else {
        c.cand = internal_tree(c.boxes_dev.p, c.on_device ? nullptr : c.boxes_host.data(), N,
                               [&](bool again) { if (!again) S->create_us[3] = clock.lap(); });
        if (!c.cand.ok) S->no_fast_why = "the internal tree could not be built";
    }
    S->sweep_on_device = c.cand.on_device ? 1 : 0;
    c.boxes_dev.release();
    std::vector<float>().swap(c.boxes_host);
    S->create_us[4] = clock.lap();
    if ((rc = upload_scene(d, S, c))) return rc;                                    // 5
    if ((rc = probe_and_decide(d, S, c.ref_inner))) return rc;                      // 6
    S->create_us[5] = clock.lap();
    if ((rc = tie_tables(d, S, c))) return rc;                                      // 7
    // 8: the leaf sweep's groups of equal leaf boxes (pt_leaf_sweep.h), from the internal tree as the host built it
    S->sweep = SweepTable{}; S->sweep_groups = 0;
    if (S->have_fast && !c.cand.on_device && !S->fast_is_callers_topology && N <= kSweepMaxPrims &&
        (rc = make_sweep_tables(c.cand.host, c.prims.data(), N, S->sweep, S->sweep_groups, S->sweep_tab, S->sweep_tab_pairs, S->sweep_classes, S->sweep_skip, S->sweep_skip_info)))
        return rc;
    // complete from here on: trace kernels run on the handle's own streams (FrameSlot), which do not synchronise with this one
    HIP_TRY(hipDeviceSynchronize());
    S->create_us[6] = clock.lap(); S->create_us[0] = clock.total();
    select_tree(S, 0);
    S->scene_bytes = (uint32_t)std::min<size_t>(
        c.ref_inner * sizeof(DNode) + (size_t)N * (sizeof(DPrim) + sizeof(DNormals)) + (size_t)d->num_materials * sizeof(DMaterial) +
            (size_t)std::max(d->num_lights, 1) * sizeof(DEmission) + 64, 0xffffffffu);
    return PT_OK;
}

// The staging buffers of a geometry change: new records and vertex normals, the buffer the live records retire into, the status word.
int ensure_staging(pt_scene* S) {
    const size_t N = (size_t)S->dev.num_prims;
    int rc;
    if ((rc = S->st_prims.ensure(N)) || (rc = S->prev_prims.ensure(N)) || (rc = S->st_normals.ensure(N))) return rc;
    return S->st_status.ensure(1);
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

// What pt_scene_update and pt_scene_transform do once new records stand in st_prims / st_normals: the refit plans where none
// exist yet, leaf boxes and the status read-back, both trees refitted, and only then the handle changes — the three record
// buffers rotate (staging -> current -> previous) and the box sweep is dropped.  `who` heads the messages.  *us_plan: wall
// microseconds of the plan build (left alone where none was due); *us_refit: of everything after it.
int adopt_staged(pt_scene* S, const char* who, bool tri_only, int64_t* us_plan, int64_t* us_refit) {
    const int N = S->dev.num_prims;
    int rc;
    StageClock clock;
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
        if (S->tree[t].have_oct && !pl.whole_tree) return pt_fail(PT_ERR_UNSUPPORTED, std::string(who) + ": octant tables on a tree of wide levels");
    }
    if (planned) *us_plan = std::max<int64_t>(clock.lap(), 1);
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
    if (bad) return pt_fail(PT_ERR_UNSUPPORTED, std::string(who) + ": a new coordinate, radius or leaf box is not finite");
    // behind the refit on its stream; the caller reads it after the synchronise that closes the call (collect_costs).  The
    // trees are written: a launch that fails here costs the measurement, not the update.
    for (int t = 0; costs && t < n_trees; t++) S->cost_pending_now[t] = enqueue_cost(S, S->tree[t], 2 + t) == PT_OK;
    S->prev_prims.swap(S->st_prims);             // the new records, for a moment
    S->prims.swap(S->prev_prims);                // current -> previous, new -> current
    S->have_prev = true;
    S->normals.swap(S->st_normals);
    S->dev.prims = S->prims.p; S->dev.normals = S->normals.p;
    S->tri_only = tri_only;
    S->sweep_groups = 0; S->sweep.count = 0;     // leaf boxes that were equal need not be any more: back to the tree
    S->sweep_tab.release();                      // (no frame is in flight: the update synchronised before it wrote)
    for (int m = 0; m < 2; m++) { S->sweep_tab_pairs[m].release(); S->sweep_classes[m] = SweepClasses{}; }
    S->sweep_skip.release();
    for (SweepSkipInfo& i : S->sweep_skip_info) i = SweepSkipInfo{0, 0};
    *us_refit = clock.lap();
    return PT_OK;
}

// pt_scene_rebuild (include/pt_api.h) between the two synchronises: the caller has made the device current and quiet, and
// synchronises again before a frame may start.  Everything is made in buffers of its own — leaf boxes out of tree[0], the
// candidate by pt_scene_create's internal-tree stage, its refit plan, its sweep tables — and only then does the handle change,
// by steps that cannot fail.  tree[0], the tie tables and every record set are read, never written.
int rebuild_scene(pt_scene* S) {
    if (!S->have_fast)
        return pt_fail(PT_ERR_UNSUPPORTED, std::string("pt_scene_rebuild: the handle holds no tie tables, pt_scene_create kept no internal tree: ") +
                                               (S->no_fast_why[0] ? S->no_fast_why : "none was built"));
    const int N = S->dev.num_prims;
    const pt_scene::Tree& T0 = S->tree[0];
    StageClock clock;
    int64_t us[4] = {0, 0, 0, 0};
    int rc;
    // ---- leaf boxes: what the caller's tree holds (the caller's own before a geometry update, the exact ones after)
    DevBuf<float> boxes_dev;
    if ((rc = boxes_dev.ensure((size_t)N * 6)) || (rc = ptf::tree_leaf_boxes(T0.nodes.p, T0.num_nodes, N, boxes_dev.p))) return rc;
    // ---- build: create's stage.  Stage 1 runs from the start of the call, whichever builder ends it.
    InternalTree cand = internal_tree(boxes_dev.p, nullptr, N, [&](bool again) { if (again) clock.rewind(); us[1] = clock.lap(); });
    if (cand.copy_error != hipSuccess)               // with the text of the HIP_TRY this copy used to stand in
        return pt_fail(cand.copy_error == hipErrorNoDevice ? PT_ERR_NO_DEVICE : PT_ERR_DEVICE, std::string("hipMemcpy(leaf_boxes.data(), boxes_dev.p, leaf_boxes.size() * sizeof(float), hipMemcpyDeviceToHost): ") + hipGetErrorString(cand.copy_error));
    if (!cand.ok)
        return pt_fail(PT_ERR_UNSUPPORTED, "pt_scene_rebuild: no internal tree could be built of the leaf boxes (not finite, or they no longer nest)");
    if (!cand.on_device && (rc = upload_tree(cand.tree, cand.host))) return rc;
    boxes_dev.release();
    // ---- probe: create's rays and create's rule, the caller's tree as it stands against the candidate.  (As at create: no tie
    // tables in view, the probe counts box tests.)
    SceneDev d0 = S->dev, d1 = S->dev;
    tree_view(S, d0, 0, false);
    tree_view(S, d1, cand.tree, 1, false);
    for (SceneDev* dv : {&d0, &d1}) { dv->ref_path = nullptr; dv->ref_anc = nullptr; dv->ref_levels = 0; dv->redo_stack = nullptr; }
    unsigned long long v[2] = {0, 0};
    if ((rc = probe_trees(d0, d1, v))) return rc;
    const bool adopt = probe_wins(v);
    us[2] = clock.lap();
    // ---- what goes with an adopted tree: its refit plan where the handle has refitted before (the next update does not pay for
    // it), the box sweep of a small scene under create's admission rules, its cost where telemetry is on
    ptf::Plan plan;
    SweepTable sweep{}; int sweep_groups = 0; DevBuf<unsigned char> sweep_tab, sweep_tab_pairs[2], sweep_skip; SweepClasses sweep_classes[2] = {}; SweepSkipInfo sweep_skip_info[3] = {};
    double cost = 0.0;
    if (adopt) {
        if (S->refit_plan[1].built && (rc = ptf::plan_build(cand.tree.nodes.p, cand.tree.num_nodes, N, &plan))) return rc;
        struct PlanGuard { ptf::Plan* p; ~PlanGuard() { if (p) ptf::plan_release(p); } } plan_guard{&plan};
        if (!cand.on_device && N <= kSweepMaxPrims) {
            std::vector<DPrim> prims((size_t)N);
            HIP_TRY(hipMemcpy(prims.data(), S->prims.p, prims.size() * sizeof(DPrim), hipMemcpyDeviceToHost));
            if ((rc = make_sweep_tables(cand.host, prims.data(), N, sweep, sweep_groups, sweep_tab, sweep_tab_pairs, sweep_classes, sweep_skip, sweep_skip_info))) return rc;
        }
        if (S->cost_on()) {
            if ((rc = ensure_cost(S)) || (rc = enqueue_cost(S, cand.tree, 3))) return rc;
            HIP_TRY(hipStreamSynchronize(nullptr));
            cost = S->cost_host[3];
        }
        // ---- adoption: swaps, nothing that can fail
        std::swap(S->tree[1], cand.tree);
        S->have_fast = true; S->fast_is_callers_topology = false;
        S->fast_cost_permille = probe_permille(v);
        S->sweep_on_device = cand.on_device ? 1 : 0;
        std::swap(S->refit_plan[1], plan);            // the old plan goes with the old tree, once the call is timed
        plan_guard.p = &plan;
        S->sweep = sweep; S->sweep_groups = sweep_groups;
        S->sweep_tab.swap(sweep_tab);
        for (int m = 0; m < 2; m++) { S->sweep_tab_pairs[m].swap(sweep_tab_pairs[m]); S->sweep_classes[m] = sweep_classes[m]; }
        S->sweep_skip.swap(sweep_skip);
        std::copy(sweep_skip_info, sweep_skip_info + 3, S->sweep_skip_info);
        S->cfg_fn = S->q_cfg_fn = nullptr;            // stack and LDS needs follow the tree: the next launch asks again
        if (S->cost_on()) { S->cost_ref[1] = S->cost_now[1] = cost; S->cost_have_ref[1] = true; }
    } else if (S->cost_on() && S->cost_have_ref[1] && S->cost_now[1] > 0.0) {
        S->cost_ref[1] = S->cost_now[1];              // no better tree to be had of these boxes: a policy waits for the next drift
    }
    us[3] = clock.lap();
    us[0] = clock.total();
    select_tree(S, 0);
    S->rebuilds++; S->rebuild_adopted = adopt ? 1 : 0; S->rebuild_cost_permille = probe_permille(v);
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
    const bool geometry = (flags & PT_UPDATE_GEOMETRY) != 0, shading = (flags & PT_UPDATE_SHADING) != 0;
    const int N = S->dev.num_prims;
    if (geometry && d->num_shapes != N) return pt_fail(PT_ERR_INVALID_ARG, "pt_scene_update: num_shapes differs from pt_scene_create's");
    if (shading && d->num_materials != S->dev.num_materials) return pt_fail(PT_ERR_INVALID_ARG, "pt_scene_update: num_materials differs from pt_scene_create's");
    if (shading && d->num_lights != S->dev.num_emission) return pt_fail(PT_ERR_INVALID_ARG, "pt_scene_update: num_lights differs from pt_scene_create's");
    int rc;
    std::vector<DMaterial> mats; std::vector<DEmission> emis; std::vector<DLight> dlights;
    if (shading) {
        if (!d->materials) return pt_fail(PT_ERR_BAD_SCENE, "scene has no materials");
        if (d->num_lights > 0 && !d->lights) return pt_fail(PT_ERR_BAD_SCENE, "bad light array");
        if ((rc = check_materials(d)) || (rc = pack_shading(d, N, mats, emis, dlights))) return rc;
    }
    if (geometry) {
        if (!d->shapes) return pt_fail(PT_ERR_BAD_SCENE, "scene has no shapes");
        if (d->num_meshes < 0 || (d->num_meshes > 0 && !d->meshes)) return pt_fail(PT_ERR_BAD_SCENE, "bad mesh array");
        if ((rc = check_meshes(d, S->dev.num_materials))) return rc;
    }
    ENTER_DEVICE(S);
    // frames of this handle that are still in flight, on the caller's streams and on the slots' own, read the scene
    HIP_TRY(hipDeviceSynchronize());
    StageClock clock;
    int64_t us_records = 0, us_refit = 0, us_plan = 0;
    if (geometry) {
        pt_scene_desc dg = *d;                                // material ids are checked against the handle's table
        dg.num_materials = S->dev.num_materials;
        int has_sphere = 0;
        if ((rc = ensure_staging(S))) return rc;
        if ((rc = ptp::prims_device(&dg, S->st_prims.p, S->st_normals.p, &has_sphere))) return rc;
        us_records = clock.lap();
        if ((rc = adopt_staged(S, "pt_scene_update", !has_sphere, &us_plan, &us_refit))) { S->cost_drop_pending(); return rc; }
        S->have_rest = false;                        // the next pt_scene_transform starts from these records
        rebuild_by_policy(S);
    }
    if (shading) {
        (void)clock.lap();
        HIP_TRY(hipMemcpy(S->materials.p, mats.data(), mats.size() * sizeof(DMaterial), hipMemcpyHostToDevice));
        HIP_TRY(hipMemcpy(S->emission.p, emis.data(), emis.size() * sizeof(DEmission), hipMemcpyHostToDevice));
        HIP_TRY(hipMemcpy(S->lights.p, dlights.data(), dlights.size() * sizeof(DLight), hipMemcpyHostToDevice));
        S->dev.bg[0] = d->background[0]; S->dev.bg[1] = d->background[1]; S->dev.bg[2] = d->background[2];
        S->diffuse_only = all_diffuse(d);
        us_records += clock.lap();
    }
    // the handle's own streams do not synchronise with the default stream the kernels above ran on
    HIP_TRY(hipDeviceSynchronize());
    collect_costs(S);
    select_tree(S, 0);
    S->updates++;
    S->update_us[0] = clock.total(); S->update_us[1] = us_records; S->update_us[2] = us_refit; S->update_us[3] = us_plan;
    return PT_OK;
}

// pt_scene_transform (include/pt_api.h).  pt_scene_update's order of events with another producer of the staged records: the
// matrices are checked and their entries made on the host, the rest records are snapshot where none are held, one kernel writes
// the staged records from them (pt_scene_transform.hip), and adopt_staged does the rest.
int transform_scene(pt_scene* S, const pt_transform* transforms, int32_t num_groups) {
    if (!S->have_groups) return pt_fail(PT_ERR_INVALID_ARG, "pt_scene_transform: the scene has no group assignment (pt_scene_set_groups)");
    if (num_groups != S->num_groups) return pt_fail(PT_ERR_INVALID_ARG, "pt_scene_transform: num_groups differs from pt_scene_set_groups'");
    if (num_groups > 0 && !transforms) return pt_fail(PT_ERR_INVALID_ARG, "pt_scene_transform: null transforms");
    std::vector<ptx::Entry> tab((size_t)std::max(num_groups, 1));
    for (int32_t g = 0; g < num_groups; g++)
        if (const int bad = ptx::prepare(&transforms[g], &tab[(size_t)g]))
            return pt_fail(ptx::refusal_status(bad), "pt_scene_transform: transforms[" + std::to_string(g) + "]: " + ptx::refusal(bad));
    const int N = S->dev.num_prims;
    ENTER_DEVICE(S);
    // frames of this handle that are still in flight, on the caller's streams and on the slots' own, read the scene
    HIP_TRY(hipDeviceSynchronize());
    StageClock clock;
    int64_t us_records = 0, us_refit = 0, us_once = 0;
    int rc;
    if ((rc = ensure_staging(S)) || (rc = S->group_tab.ensure(tab.size() * ptx::kEntryFloats))) return rc;
    const bool snapshot = !S->have_rest;
    if (snapshot) {
        (void)clock.lap();
        if ((rc = S->rest_prims.ensure((size_t)N)) || (rc = S->rest_normals.ensure((size_t)N))) return rc;
        HIP_TRY(hipMemcpyAsync(S->rest_prims.p, S->prims.p, (size_t)N * sizeof(DPrim), hipMemcpyDeviceToDevice, nullptr));
        HIP_TRY(hipMemcpyAsync(S->rest_normals.p, S->normals.p, (size_t)N * sizeof(DNormals), hipMemcpyDeviceToDevice, nullptr));
        HIP_TRY(hipStreamSynchronize(nullptr));           // paid once: timed on its own
        us_once = std::max<int64_t>(clock.lap(), 1);
    }
    (void)clock.lap();
    HIP_TRY(hipMemcpy(S->group_tab.p, tab.data(), tab.size() * sizeof(ptx::Entry), hipMemcpyHostToDevice));
    if ((rc = ptx::transform_records(S->rest_prims.p, S->rest_normals.p, S->group_of.p, S->group_tab.p, N, S->st_prims.p, S->st_normals.p)))
        return rc;
    us_records = clock.lap();
    int64_t us_plan = 0;
    if ((rc = adopt_staged(S, "pt_scene_transform", S->tri_only, &us_plan, &us_refit))) { S->cost_drop_pending(); return rc; }
    rebuild_by_policy(S);
    // the handle's own streams do not synchronise with the default stream the kernels above ran on
    HIP_TRY(hipDeviceSynchronize());
    collect_costs(S);
    S->have_rest = true;                                // (a refused call leaves the flag as it was: the next one copies again)
    select_tree(S, 0);
    S->transforms++;
    S->transform_us[0] = clock.total(); S->transform_us[1] = us_records; S->transform_us[2] = us_refit; S->transform_us[3] = us_once + us_plan;
    return PT_OK;
}

// pt_bvh_build_sweep(_device): the arguments checked, and the leaf boxes [N][6] of d's pool — every shape in exactly one leaf, every box finite.
int pool_leaf_boxes(const pt_scene_desc* d, const pt_bvh_node* out_nodes, const int32_t* out_root, std::vector<float>& boxes) {
    if (!d || !out_nodes || !out_root) return pt_fail(PT_ERR_INVALID_ARG, "bad argument");
    const int N = d->num_shapes;
    if (N <= 0 || !d->nodes || d->num_nodes != 2 * N - 1) return pt_fail(PT_ERR_BAD_SCENE, "needs the leaf boxes of a 2*num_shapes-1 node pool");
    boxes.resize((size_t)N * 6);
    std::vector<char> seen(N, 0);
    for (int k = 0; k < d->num_nodes; k++) {
        const pt_bvh_node& nd = d->nodes[k];
        if (nd.prim == -1) continue;
        if (nd.prim < 0 || nd.prim >= N || seen[nd.prim]) return pt_fail(PT_ERR_BAD_SCENE, "leaves must cover every shape exactly once");
        seen[nd.prim] = 1;
        std::memcpy(&boxes[(size_t)nd.prim * 6], nd.bmin, 12);
        std::memcpy(&boxes[(size_t)nd.prim * 6 + 3], nd.bmax, 12);
    }
    for (int i = 0; i < N; i++)
        if (!seen[i]) return pt_fail(PT_ERR_BAD_SCENE, "leaves must cover every shape exactly once");
    for (float v : boxes)
        if (!std::isfinite(v)) return pt_fail(PT_ERR_BAD_SCENE, "leaf box is not finite");
    return PT_OK;
}

}  // namespace

extern "C" {   // ---- C ABI: the lifecycle entry points

int pt_scene_create(const pt_scene_desc* desc, pt_scene** out) {
    if (!out) return pt_fail(PT_ERR_INVALID_ARG, "null output pointer");
    *out = nullptr;
    int ndev = 0;
    hipError_t e = hipGetDeviceCount(&ndev);
    if (e != hipSuccess || ndev <= 0) return pt_fail(PT_ERR_NO_DEVICE, "no HIP device available: the path tracer has no CPU fallback");
    pt_scene* S = new pt_scene();
    auto bail = [&](int rc) { pt_scene_destroy(S); return rc; };
    if (hipGetDevice(&S->device) != hipSuccess) return bail(pt_fail(PT_ERR_DEVICE, "hipGetDevice failed"));
    hipDeviceProp_t prop;
    if (hipGetDeviceProperties(&prop, S->device) != hipSuccess) return bail(pt_fail(PT_ERR_DEVICE, "hipGetDeviceProperties failed"));
    S->num_cus = prop.multiProcessorCount;
    S->lds_per_block_max = prop.sharedMemPerBlock;
    if (int rc = validate_and_build(desc, S)) return bail(rc);
    *out = S;
    return PT_OK;
}

int pt_scene_destroy(pt_scene* S) {
    if (!S) return PT_OK;
    DeviceGuard guard;
    (void)guard.enter(S->device);
    if (S->last_stream || S->have_timing || S->q_seq) (void)hipDeviceSynchronize();
    delete S;                        // ~pt_scene: events, streams, plans and pinned memory, then every buffer
    return PT_OK;
}

int pt_scene_update(pt_scene* S, const pt_scene_desc* desc, int flags) {
    if (!S) return pt_fail(PT_ERR_INVALID_ARG, "pt_scene_update: null scene");
    if (!desc) return pt_fail(PT_ERR_INVALID_ARG, "pt_scene_update: null scene description");
    if (flags == 0 || (flags & ~(PT_UPDATE_GEOMETRY | PT_UPDATE_SHADING)))
        return pt_fail(PT_ERR_INVALID_ARG, "pt_scene_update: flags must be PT_UPDATE_GEOMETRY, PT_UPDATE_SHADING or both");
    return update_scene(S, desc, flags);
}

int pt_scene_rebuild(pt_scene* S, int flags) {
    if (!S) return pt_fail(PT_ERR_INVALID_ARG, "pt_scene_rebuild: null scene");
    if (flags != 0) return pt_fail(PT_ERR_INVALID_ARG, "pt_scene_rebuild: flags must be 0 (reserved)");
    ENTER_DEVICE(S);
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
    if (!S) return pt_fail(PT_ERR_INVALID_ARG, "pt_scene_set_groups: null scene");
    if (!group_of_shape) return pt_fail(PT_ERR_INVALID_ARG, "pt_scene_set_groups: null group_of_shape");
    if (num_groups < 0 || num_groups > (1 << 20)) return pt_fail(PT_ERR_INVALID_ARG, "pt_scene_set_groups: num_groups must be in [0, 2^20]");
    const int N = S->dev.num_prims;
    for (int k = 0; k < N; k++)
        if (group_of_shape[k] < -1 || group_of_shape[k] >= num_groups)
            return pt_fail(PT_ERR_INVALID_ARG, "pt_scene_set_groups: group_of_shape[" + std::to_string(k) + "] is not in [-1, num_groups)");
    ENTER_DEVICE(S);
    if (int rc = S->group_of.ensure((size_t)N)) return rc;
    S->have_groups = false;                              // a copy that fails leaves no assignment, not half of one
    HIP_TRY(hipMemcpy(S->group_of.p, group_of_shape, (size_t)N * sizeof(int32_t), hipMemcpyHostToDevice));
    S->num_groups = num_groups;
    S->have_groups = true;
    return PT_OK;
}

int pt_scene_transform(pt_scene* S, const pt_transform* transforms, int32_t num_groups) {
    if (!S) return pt_fail(PT_ERR_INVALID_ARG, "pt_scene_transform: null scene");
    return transform_scene(S, transforms, num_groups);
}

int pt_bvh_build_sweep(const pt_scene_desc* d, pt_bvh_node* out_nodes, int32_t* out_root, int32_t* out_depth, double* out_build_ms) {
    std::vector<float> boxes;
    if (int rc = pool_leaf_boxes(d, out_nodes, out_root, boxes)) return rc;
    const auto t0 = std::chrono::steady_clock::now();
    std::vector<pt_bvh_node> nodes;
    int32_t root = 0, depth = 0;
    try {
        pts::build_sweep_tree(boxes.data(), d->num_shapes, nodes, &root, &depth);
    } catch (const std::exception& e) {
        return pt_fail(PT_ERR_DEVICE, std::string("pt_bvh_build_sweep: ") + e.what());
    }
    std::memcpy(out_nodes, nodes.data(), nodes.size() * sizeof(pt_bvh_node));
    *out_root = root; if (out_depth) *out_depth = depth;
    if (out_build_ms) *out_build_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
    return PT_OK;
}

int pt_bvh_build_sweep_device(const pt_scene_desc* d, pt_bvh_node* out_nodes, int32_t* out_root, int32_t* out_depth, double* out_build_ms) {
    std::vector<float> boxes;
    if (int rc = pool_leaf_boxes(d, out_nodes, out_root, boxes)) return rc;
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) return pt_fail(PT_ERR_NO_DEVICE, "no HIP device available");
    std::vector<pt_bvh_node> nodes;
    int32_t root = 0, depth = 0;
    int rc = pts::sweep_build_device(boxes.data(), d->num_shapes, nodes, &root, &depth, out_build_ms);
    if (rc) return rc;
    std::memcpy(out_nodes, nodes.data(), nodes.size() * sizeof(pt_bvh_node));
    *out_root = root; if (out_depth) *out_depth = depth;
    return PT_OK;
}

}  // extern "C"
