// The box sweep's skip table (csrc/pt_sweep_skip.h): a bounce that starts on an axis-aligned plane does not test that plane's
// triangles.  Three things are checked on the CPU, with the library's own arithmetic (csrc/pt_math.h, host half):
//   1. the lemma: Möller–Trumbore as pt_trace.h's leaf_test_slot runs it (p0 and the staged edges of sweep_stage_record, the same
//      products and sums in the same order) keeps no hit of a triangle whose three vertices have coordinate c on an axis when the
//      origin has it too, for tnear 0 and 1e-4: random, huge, denormal and equal vertices, +0.0 against -0.0, planes at 0, 548.8
//      and 1e30, directions random, nearly in the plane, with zero components and with a denormal divisor.  One ulp off the
//      plane the test CAN keep a hit, and does in some of the cases: the skip needs equality;
//   2. the table: for every order a launch can sweep in (the groups' own, the pair classes, the families) every primitive's
//      entry equals a brute-force grouping by (axis, float-equal c) of the boxes, the tables made before it keep every byte,
//      and the fixed scenes give the masks written next to them (split wall, parallel walls, rotated blocks, 1 / 31 / 32 groups);
//   3. the kernel's rule: over 2048 segments per scene that start on the scene's own triangles at p0 w + p1 u + p2 v, the groups
//      the plain sweep hits minus the skip word lose only leaf tests that the plain loop rejects, and the closest hit is
//      bit-equal.
// `sweep_skip_check FILE` runs 2 and 3 on the N x 9 floats of FILE (the triangles of a scene, by primitive) and prints
// "groups G skip_groups S planes P skipped_tests T of U".
// Stand-alone; built with -fsanitize=address,undefined by tests/test_sweep_skip_host.py.  Exit code 0 = all held.
#include <cfloat>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <random>
#include <vector>

#include "pt_math.h"
#include "pt_sweep_families.h"
#include "pt_sweep_skip.h"

namespace {

using ptl::DNode;
using ptl::DPrim;
using ptl::SweepClasses;
using ptl::SweepGroup;
using ptl::SweepSkipEntry;
using ptm::V3;

uint64_t errors = 0;
void fail(const char* what, int n = -1) {
    if (errors++ < 10) std::fprintf(stderr, "FAIL: %s (n = %d)\n", what, n);
}

// ---- 1. the leaf test ----------------------------------------------------------------------------------------------------
struct Kept { bool kept; float t, u, v; };
// leaf_test_slot of pt_trace.h up to its compare, on a record as the block stages it
Kept leaf_test(const DPrim& staged, V3 o, V3 d, float tnear) {
    const V3 p0 = ptm::mk(staged.v[0], staged.v[1], staged.v[2]), e1 = ptm::mk(staged.v[3], staged.v[4], staged.v[5]), e2 = ptm::mk(staged.v[6], staged.v[7], staged.v[8]);
    const V3 s1 = ptm::cross(d, e2);
    const float divisor = ptm::dot(s1, e1);
    if (divisor != 0.0f) {
        const float inv_divisor = ptm::rcp_exact(divisor);
        const V3 s = o - p0;
        const float u = ptm::dot(s, s1) * inv_divisor;
        const V3 s2 = ptm::cross(s, e1);
        const float v = ptm::dot(d, s2) * inv_divisor;
        const float tt = ptm::dot(e2, s2) * inv_divisor;
        if (tt > tnear && u >= 0.0f && v >= 0.0f && u + v <= 1.0f) return {true, tt, u, v};
    }
    return {false, 0.0f, 0.0f, 0.0f};
}
DPrim triangle(const float* p) {
    DPrim r{};
    std::memcpy(r.v, p, 36);
    r.info = 0; r.light = -1; r.pad = 0;
    return r;
}

float pick(std::mt19937& rng, int kind) {
    std::uniform_real_distribution<float> u(-1.0f, 1.0f);
    switch (kind) {
        case 0: return 600.0f * u(rng);
        case 1: return u(rng) * 3.0e38f;                                  // huge: differences and products overflow
        case 2: return u(rng) * 1.0e-39f;                                 // denormal
        case 3: return u(rng) * 1.0e19f;
        default: return (rng() & 1u) ? 0.0f : -0.0f;
    }
}

void check_lemma() {
    std::mt19937 rng(20240917u);
    const float planes[] = {0.0f, -0.0f, 548.8f, 1.0e30f, -165.0f, 1.0e-40f};
    uint64_t tested = 0, with_divisor = 0, off_plane_kept = 0, off_plane = 0;
    for (int axis = 0; axis < 3; axis++)
        for (float c : planes)
            for (int vk = 0; vk < 5; vk++)             // how the vertices are drawn
                for (int dk = 0; dk < 5; dk++)         // how the direction is drawn
                    for (int rep = 0; rep < 400; rep++) {
                        float p[9];
                        for (int k = 0; k < 9; k++) p[k] = pick(rng, vk);
                        if (rep % 7 == 3) std::memcpy(p + 3, p, 12);                         // two equal vertices
                        if (rep % 11 == 5) { std::memcpy(p + 3, p, 12); std::memcpy(p + 6, p, 12); }
                        for (int v = 0; v < 3; v++) p[3 * v + axis] = c == 0.0f ? ((rng() & 1u) ? 0.0f : -0.0f) : c;
                        float o[3] = {pick(rng, rep % 3 == 0 ? 0 : vk), pick(rng, rep % 3 == 0 ? 0 : vk), pick(rng, rep % 3 == 0 ? 0 : vk)};
                        if (rep % 2) {               // an origin inside the triangle, as a bounce has it
                            std::uniform_real_distribution<float> u01(0.0f, 1.0f);
                            float u = u01(rng), v = u01(rng);
                            if (u + v > 1.0f) { u = 1.0f - u; v = 1.0f - v; }
                            const float w = (1.0f - u) - v;
                            for (int a = 0; a < 3; a++) o[a] = p[a] * w + p[3 + a] * u + p[6 + a] * v;
                        }
                        o[axis] = c == 0.0f ? ((rng() & 1u) ? 0.0f : -0.0f) : c;
                        float d[3];
                        std::uniform_real_distribution<float> u(-1.0f, 1.0f);
                        for (int a = 0; a < 3; a++) d[a] = u(rng);
                        if (dk == 1) d[axis] *= 1.0e-6f;                                     // nearly in the plane
                        if (dk == 2) d[(axis + 1 + (int)(rng() % 2u)) % 3] = (rng() & 1u) ? 0.0f : -0.0f;
                        if (dk == 3) d[axis] = (rng() & 1u) ? 0.0f : -0.0f;                  // in the plane: divisor +-0
                        if (dk == 4) for (int a = 0; a < 3; a++) d[a] *= 1.0e-36f;           // small products: a denormal divisor among them
                        const DPrim st = ptl::sweep_stage_record(triangle(p));
                        const V3 ov = ptm::mk(o[0], o[1], o[2]), dv = ptm::mk(d[0], d[1], d[2]);
                        for (float tnear : {0.0f, 1.0e-4f}) {
                            tested++;
                            if (leaf_test(st, ov, dv, tnear).kept) fail("a triangle in the origin's plane was kept", axis);
                        }
                        const float div = ptm::dot(ptm::cross(dv, ptm::mk(st.v[6], st.v[7], st.v[8])), ptm::mk(st.v[3], st.v[4], st.v[5]));
                        with_divisor += div != 0.0f;
                        // the reverse: one ulp off the plane, an origin over the triangle and a direction towards it
                        if (vk == 0 && dk == 0 && (rep % 2) && c == 548.8f) {
                            float o2[3] = {o[0], o[1], o[2]};
                            o2[axis] = std::nextafterf(c, 1.0e30f);
                            const V3 d2 = ptm::mk(axis == 0 ? -0.05f : d[0], axis == 1 ? -0.05f : d[1], axis == 2 ? -0.05f : d[2]);
                            off_plane++;
                            off_plane_kept += leaf_test(st, ptm::mk(o2[0], o2[1], o2[2]), d2, 1.0e-4f).kept;
                        }
                    }
    std::printf("lemma: %llu tests, %llu with a divisor, none kept; one ulp off the plane %llu of %llu kept\n", (unsigned long long)tested,
                (unsigned long long)with_divisor, (unsigned long long)off_plane_kept, (unsigned long long)off_plane);
    if (with_divisor * 4 < tested / 2) fail("too few cases reach the compare");
    if (off_plane_kept == 0) fail("one ulp off the plane never kept a hit: the reverse case shows nothing");
}

// ---- 2. the table --------------------------------------------------------------------------------------------------------
struct Scene {
    std::vector<DPrim> prims;
    std::vector<DNode> nodes;
};
void tri_box(const DPrim& p, float* box) {
    for (int a = 0; a < 3; a++) {
        box[a] = std::fmin(std::fmin(p.v[a], p.v[3 + a]), p.v[6 + a]);
        box[3 + a] = std::fmax(std::fmax(p.v[a], p.v[3 + a]), p.v[6 + a]);
    }
}
// A random binary tree over the primitives in inner-only form (tests/native/sweep_pairs_check.cpp has the same one), every
// leaf with its triangle's own box.
Scene make_scene(const std::vector<float>& tris, std::mt19937& rng) {
    Scene s;
    const int n = (int)(tris.size() / 9);
    for (int k = 0; k < n; k++) s.prims.push_back(triangle(&tris[9 * (size_t)k]));
    s.nodes.resize((size_t)n - 1);
    std::memset(s.nodes.data(), 0, s.nodes.size() * sizeof(DNode));
    std::vector<int32_t> order(n);
    for (int k = 0; k < n; k++) order[k] = k;
    for (int k = n - 1; k > 0; k--) std::swap(order[k], order[rng() % (uint32_t)(k + 1)]);
    int next = 0;
    struct Job { int lo, hi, node; };
    std::vector<Job> todo{{0, n, next++}};
    while (!todo.empty()) {
        const Job j = todo.back();
        todo.pop_back();
        const int mid = j.lo + 1 + (int)(rng() % (uint32_t)(j.hi - j.lo - 1));
        for (int side = 0; side < 2; side++) {
            const int lo = side ? mid : j.lo, hi = side ? j.hi : mid;
            int32_t ref;
            if (hi - lo == 1) {
                ref = ~order[lo];
                tri_box(s.prims[order[lo]], side ? s.nodes[j.node].rmin : s.nodes[j.node].lmin);
            } else {
                ref = next++;
                todo.push_back({lo, hi, ref});
            }
            (side ? s.nodes[j.node].right : s.nodes[j.node].left) = ref;
        }
    }
    return s;
}

// One order a launch can sweep in, with everything made for it.
struct Built {
    int count = 0;
    SweepGroup g[ptl::kSweepMaxBoxes];
    std::vector<unsigned char> tab, skip;
    uint32_t pitch = 0;
    ptl::SweepSkipInfo info{0, 0};
};
// order: 0 the groups' own (every pair general), 1 the pair classes, 2 the families
bool build(const Scene& s, int order, Built* b) {
    const int n = (int)s.prims.size(), num_nodes = (int)s.nodes.size();
    SweepGroup groups[ptl::kSweepMaxPrims];
    const int count = ptl::build_sweep_groups(s.nodes.data(), num_nodes, n, 64u, groups);
    if (count < 1 || count > ptl::kSweepMaxBoxes) return false;
    b->count = count;
    b->tab.assign(ptl::sweep_layout_bytes((uint32_t)count, (uint32_t)n), 0);
    SweepClasses cls = ptl::sweep_classes_of_pairs(ptl::sweep_pairs_none((uint32_t)count));
    if (order == 0) {
        std::copy(groups, groups + count, b->g);
        if (!ptl::build_sweep_layout(b->g, count, s.nodes.data(), num_nodes, 64u, s.prims.data(), n, b->tab.data())) return false;
    } else {
        int perm[ptl::kSweepMaxBoxes];
        if (!ptl::build_sweep_families(groups, count, s.nodes.data(), num_nodes, 64u, order - 1, b->g, perm, &cls) ||
            !ptl::build_sweep_layout(b->g, count, s.nodes.data(), num_nodes, 64u, s.prims.data(), n, b->tab.data()) ||
            !ptl::build_sweep_family_tables(b->g, count, cls, s.nodes.data(), num_nodes, 64u, b->tab.data()))
            return false;
    }
    b->pitch = ptl::sweep_classes_pitch(cls);
    const std::vector<unsigned char> before = b->tab;
    // the skip table behind a guard of its own size: the builder writes kSweepSkipTableBytes and no more
    b->skip.assign(ptl::kSweepSkipTableBytes, 0xa5);
    if (!ptl::build_sweep_skip(b->g, count, s.nodes.data(), num_nodes, 64u, s.prims.data(), n, b->skip.data(), &b->info)) return false;
    if (before != b->tab) fail("the skip table's builder changed a byte of the tables", order);
    if (!ptl::sweep_skip_fits((uint32_t)count, (uint32_t)n, (uint32_t)num_nodes, 64u)) fail("the entries do not fit the node region", n);
    return true;
}
const float* group_box(const Scene& s, const SweepGroup& g) {
    return ptl::sweep_group_box(g, s.nodes.data(), (int)s.nodes.size(), 64u);
}
SweepSkipEntry entry(const Built& b, int prim) {
    SweepSkipEntry e;
    std::memcpy(&e, b.skip.data() + (size_t)prim * sizeof(e), sizeof(e));
    return e;
}
int group_of(const Built& b, int prim) {
    for (int k = 0; k < b.count; k++)
        if ((ptl::sweep_group_mask(b.g[k]) >> prim) & 1ull) return k;
    return -1;
}
// brute force: the lowest axis on which the group's box is flat, and every group whose box is flat there at a float-equal c
void check_table(const Scene& s, const Built& b, int order) {
    const int n = (int)s.prims.size();
    uint32_t skip_groups = 0;
    for (int k = 0; k < b.count; k++) {
        const float* box = group_box(s, b.g[k]);
        int axis = -1;
        for (int a = 2; a >= 0; a--)
            if (box[a] == box[3 + a]) axis = a;
        uint32_t mask = 0;
        for (int j = 0; j < b.count && axis >= 0; j++) {
            const float* bj = group_box(s, b.g[j]);
            if (bj[axis] == box[axis] && bj[3 + axis] == box[axis]) mask |= 1u << (31 - j);
        }
        skip_groups += mask != 0;
        if (axis >= 0 && !((mask >> (31 - k)) & 1u)) fail("brute force lost the group itself", k);
        for (int prim = 0; prim < n; prim++) {
            if (group_of(b, prim) != k) continue;
            const SweepSkipEntry e = entry(b, prim);
            if (e.mask != mask) fail("mask differs from the brute-force grouping", order * 1000 + prim);
            if (mask && ((int)e.axis != axis || !(e.c == box[axis]))) fail("axis or plane differs", order * 1000 + prim);
            if (!mask && (e.axis != 0u || std::memcmp(&e.c, "\0\0\0\0", 4) != 0)) fail("an entry without a mask is not zero", prim);
            if (e.mask & ~(0xffffffffu << (32 - b.count))) fail("a bit below the last group", prim);
        }
    }
    if (b.info.groups != skip_groups) fail("info: groups", order);
    for (size_t k = (size_t)n * sizeof(SweepSkipEntry); k < b.skip.size(); k++)
        if (b.skip[k] != 0) { fail("bytes behind the last entry are not zero", order); break; }
}

// ---- 3. the kernel's rule ------------------------------------------------------------------------------------------------
struct Best { float t, u, v; int32_t prim; };
struct RuleCounts { uint64_t tests = 0, skipped = 0, on_plane = 0, bounces = 0; };

// the groups whose box the segment hits, by the slab test of the plain loop on the group's own box (near / far by the octant)
uint32_t hit_word(const Scene& s, const Built& b, const float* o, const float* inv) {
    uint32_t h = 0;
    for (int k = 0; k < b.count; k++) {
        const float* box = group_box(s, b.g[k]);
        float nr[3], fr[3];
        for (int a = 0; a < 3; a++) {
            const bool neg = std::signbit(inv[a]);
            nr[a] = (box[neg ? 3 + a : a] - o[a]) * inv[a];
            fr[a] = (box[neg ? a : 3 + a] - o[a]) * inv[a];
        }
        const float tn = ptm::fmax2(0.0f, ptm::fmax2(ptm::fmax2(nr[0], nr[1]), nr[2])), tf = ptm::fmin2(ptm::fmin2(fr[0], fr[1]), fr[2]);
        h = h + h + (tf >= tn ? 1u : 0u);
    }
    return ptl::sweep_hits_align(h, (uint32_t)b.count);
}
// the burst: groups in table order, a group's primitives along the chain of its slot records
Best burst(const Scene& s, const Built& b, uint32_t hits, V3 o, V3 d, float tnear, uint32_t only_rejected_of, uint64_t* tests) {
    const DPrim* slots = reinterpret_cast<const DPrim*>(b.tab.data() + ptl::sweep_slots_off((uint32_t)b.count));
    Best best{FLT_MAX, 0.0f, 0.0f, -1};
    (void)s;
    while (hits) {
        const uint32_t k = ptl::sweep_first_group(hits);
        hits = ptl::sweep_clear_group(hits, k);
        for (uint32_t slot = k;;) {
            DPrim rec;
            std::memcpy(&rec, &slots[slot], sizeof(rec));
            const uint32_t link = (uint32_t)rec.pad;
            const Kept r = leaf_test(ptl::sweep_stage_record(rec), o, d, tnear);
            (*tests)++;
            if (((only_rejected_of >> (31 - k)) & 1u) && r.kept) fail("a skipped leaf test would have passed the plain loop's compare", (int)k);
            // ties on t: the lower primitive, whatever the order of the tests (the kernel asks the caller's tree)
            const int32_t prim = (int32_t)ptl::sweep_link_prim(link);
            if (r.kept && (r.t < best.t || (r.t == best.t && best.prim >= 0 && prim < best.prim))) best = Best{r.t, r.u, r.v, prim};
            slot = ptl::sweep_link_next(link);
            if (slot == 0) break;
        }
    }
    return best;
}
void check_rule(const Scene& s, const Built& b, std::mt19937& rng, RuleCounts* rc) {
    const int n = (int)s.prims.size();
    std::uniform_real_distribution<float> u01(0.0f, 1.0f), sym(-1.0f, 1.0f);
    for (int r = 0; r < 2048; r++) {
        const int prim = (int)(rng() % (uint32_t)n);
        const DPrim& p = s.prims[prim];
        float u = u01(rng), v = u01(rng);
        if (u + v > 1.0f) { u = 1.0f - u; v = 1.0f - v; }
        const float w = (1.0f - u) - v;
        float o[3], d[3], inv[3];
        for (int a = 0; a < 3; a++) o[a] = p.v[a] * w + p.v[3 + a] * u + p.v[6 + a] * v;
        for (int a = 0; a < 3; a++) d[a] = sym(rng);
        if (r % 9 == 4) d[rng() % 3u] *= 1.0e-5f;
        for (int a = 0; a < 3; a++) inv[a] = ptm::rcp_exact(d[a]);
        if (!(std::isfinite(inv[0]) && std::isfinite(inv[1]) && std::isfinite(inv[2]))) continue;      // the kernel reruns these on the tree
        const SweepSkipEntry e = entry(b, prim);
        const uint32_t skip = ptl::sweep_skip_word(e, o);
        const uint32_t hits = hit_word(s, b, o, inv);
        rc->bounces++;
        rc->on_plane += skip != 0;
        const V3 ov = ptm::mk(o[0], o[1], o[2]), dv = ptm::mk(d[0], d[1], d[2]);
        for (float tnear : {1.0e-4f, 0.0f}) {
            uint64_t t_plain = 0, t_skip = 0;
            const Best plain = burst(s, b, hits, ov, dv, tnear, skip, &t_plain);
            const Best skipped = burst(s, b, hits & ~skip, ov, dv, tnear, 0u, &t_skip);
            if (std::memcmp(&plain, &skipped, sizeof(Best)) != 0) fail("the closest hit differs", prim);
            if (tnear != 0.0f) { rc->tests += t_plain; rc->skipped += t_plain - t_skip; }
        }
        if (skip && !(hits & skip & (0x80000000u >> group_of(b, prim)))) fail("the sweep does not hit the group the bounce left", prim);
    }
}

// ---- scenes --------------------------------------------------------------------------------------------------------------
void quad(std::vector<float>& t, int axis, float c, float lo0, float hi0, float lo1, float hi1) {
    const int b = axis == 0 ? 1 : 0, cc = axis == 2 ? 1 : 2;
    float P[4][3];
    const float x[4] = {lo0, hi0, hi0, lo0}, y[4] = {lo1, lo1, hi1, hi1};
    for (int k = 0; k < 4; k++) { P[k][axis] = c; P[k][b] = x[k]; P[k][cc] = y[k]; }
    const int idx[6] = {0, 1, 2, 0, 2, 3};
    for (int k : idx) t.insert(t.end(), P[k], P[k] + 3);
}
void rotated_block(std::vector<float>& t, float cx, float cy, float cz, float angle) {
    // four upright faces of a block turned about y: boxes flat on no axis; its top, flat on y
    const float cs = std::cos(angle), sn = std::sin(angle), h = 0.4f;
    float c[4][2];
    for (int k = 0; k < 4; k++) {
        const float x = (k == 0 || k == 3) ? -h : h, z = k < 2 ? -h : h;
        c[k][0] = cx + cs * x - sn * z; c[k][1] = cz + sn * x + cs * z;
    }
    for (int k = 0; k < 4; k++) {
        const int j = (k + 1) % 4;
        const float P[4][3] = {{c[k][0], cy - h, c[k][1]}, {c[j][0], cy - h, c[j][1]}, {c[j][0], cy + h, c[j][1]}, {c[k][0], cy + h, c[k][1]}};
        const int idx[6] = {0, 1, 2, 0, 2, 3};
        for (int i : idx) t.insert(t.end(), P[i], P[i] + 3);
    }
}

struct Result { int groups; ptl::SweepSkipInfo info; RuleCounts rc; };
Result check_scene(const std::vector<float>& tris, uint32_t seed, int trees) {
    std::mt19937 rng(seed);
    Result res{0, {0, 0}, {}};
    for (int t = 0; t < trees; t++) {
        const Scene s = make_scene(tris, rng);
        for (int order = 0; order < 3; order++) {
            Built b;
            if (!build(s, order, &b)) { fail("tables refused", order); continue; }
            check_table(s, b, order);
            RuleCounts rc;
            check_rule(s, b, rng, &rc);
            if (t == 0 && order == 2) { res.groups = b.count; res.info = b.info; res.rc = rc; }
        }
    }
    return res;
}
// the mask of primitive `prim` in the groups' own order, first tree
uint32_t mask_of(const std::vector<float>& tris, int prim, int* group = nullptr) {
    std::mt19937 rng(5u);
    const Scene s = make_scene(tris, rng);
    Built b;
    if (!build(s, 0, &b)) { fail("tables refused"); return 0; }
    if (group) *group = group_of(b, prim);
    return entry(b, prim).mask;
}

void check_fixed() {
    {   // a wall split into two coplanar groups, and a third quad elsewhere: the two name each other
        std::vector<float> t;
        quad(t, 0, 548.8f, 0.0f, 200.0f, 0.0f, 500.0f);
        quad(t, 0, 548.8f, 200.0f, 559.2f, 0.0f, 500.0f);
        quad(t, 1, 0.0f, 0.0f, 500.0f, 0.0f, 500.0f);
        int g0 = -1, g2 = -1, g4 = -1;
        const uint32_t m0 = mask_of(t, 0, &g0), m2 = mask_of(t, 2, &g2), m4 = mask_of(t, 4, &g4);
        if (m0 != m2 || m0 != ((0x80000000u >> g0) | (0x80000000u >> g2)) || g0 == g2) fail("split wall");
        if (m4 != (0x80000000u >> g4)) fail("split wall: the floor");
        const Result r = check_scene(t, 11u, 4);
        if (r.groups != 3 || r.info.groups != 3 || r.info.planes != 2 || r.rc.skipped == 0) fail("split wall: counts");
    }
    {   // two parallel walls at different c, and the same wall at -0.0 against +0.0 (one plane)
        std::vector<float> t;
        quad(t, 2, 1.0f, -1.0f, 1.0f, -1.0f, 1.0f);
        quad(t, 2, 2.0f, -1.0f, 1.0f, -1.0f, 1.0f);
        quad(t, 1, 0.0f, -1.0f, 0.0f, -1.0f, 1.0f);
        quad(t, 1, -0.0f, 0.0f, 1.0f, -1.0f, 1.0f);
        int g0 = -1, g2 = -1, g4 = -1, g6 = -1;
        const uint32_t m0 = mask_of(t, 0, &g0), m2 = mask_of(t, 2, &g2), m4 = mask_of(t, 4, &g4), m6 = mask_of(t, 6, &g6);
        if (m0 != (0x80000000u >> g0) || m2 != (0x80000000u >> g2)) fail("parallel walls share a mask");
        if (m4 != m6 || m4 != ((0x80000000u >> g4) | (0x80000000u >> g6))) fail("-0.0 and +0.0 are one plane");
        const Result r = check_scene(t, 12u, 4);
        if (r.groups != 4 || r.info.groups != 4 || r.info.planes != 3) fail("parallel walls: counts");
    }
    {   // rotated blocks on a floor: the upright faces have mask 0, the tops and the floor their own planes
        std::vector<float> t;
        quad(t, 1, 0.0f, -3.0f, 3.0f, -3.0f, 3.0f);
        rotated_block(t, -1.0f, 0.4f, 0.2f, 0.3f);
        rotated_block(t, 1.1f, 0.4f, -0.3f, -0.5f);
        for (int prim = 2; prim < 18; prim++)
            if (mask_of(t, prim) != 0u) fail("an upright face of a rotated block has a mask", prim);
        if (mask_of(t, 0) == 0u) fail("the floor has no mask");
        const Result r = check_scene(t, 13u, 4);
        if (r.groups != 9 || r.info.groups != 1 || r.info.planes != 1) fail("rotated blocks: counts");
    }
    for (int groups : {1, 31, 32}) {   // parallel quads along z: group k alone in its plane; bits 31 and 0
        std::vector<float> t;
        for (int k = 0; k < groups; k++) quad(t, 2, -0.5f * (float)(k + 1), -1.0f - 0.1f * (float)k, 1.0f + 0.1f * (float)k, -1.0f, 1.0f);
        for (int k = 0; k < groups; k++) {
            int g = -1;
            const uint32_t m = mask_of(t, 2 * k, &g);
            if (g < 0 || m != (0x80000000u >> g) || mask_of(t, 2 * k + 1) != m) fail("one group per plane", k);
        }
        const Result r = check_scene(t, 14u + (uint32_t)groups, 2);
        if (r.groups != groups || (int)r.info.groups != groups || (int)r.info.planes != groups) fail("groups along z: counts", groups);
    }
}

}  // namespace

int main(int argc, char** argv) {
    if (argc > 1) {
        std::FILE* f = std::fopen(argv[1], "rb");
        if (!f) { std::fprintf(stderr, "cannot open %s\n", argv[1]); return 2; }
        std::vector<float> tris;
        float buf[9];
        while (std::fread(buf, sizeof(float), 9, f) == 9) tris.insert(tris.end(), buf, buf + 9);
        std::fclose(f);
        if (tris.size() < 18 || tris.size() / 9 > (size_t)ptl::kSweepMaxPrims) { std::fprintf(stderr, "2 .. 64 triangles\n"); return 2; }
        const Result r = check_scene(tris, 99u, 4);
        std::printf("groups %d skip_groups %u planes %u skipped_tests %llu of %llu on_plane %llu of %llu\n", r.groups, r.info.groups, r.info.planes,
                    (unsigned long long)r.rc.skipped, (unsigned long long)r.rc.tests, (unsigned long long)r.rc.on_plane, (unsigned long long)r.rc.bounces);
    } else {
        check_lemma();
        check_fixed();
    }
    if (errors) { std::fprintf(stderr, "sweep_skip_check: %llu errors\n", (unsigned long long)errors); return 1; }
    std::puts("sweep_skip_check: ok");
    return 0;
}
