// The sweep's groups paired by shared axis intervals and the box tables in class order (csrc/pt_sweep_pairs.h).  For every set
// of leaf boxes, under several random trees (the order of the groups follows the tree):
//   - build_sweep_pairs gives a permutation of the groups, the class counts add up, and it gives the same one when asked again;
//   - every SHARE pair has the same interval on its axis BIT FOR BIT, every SHARE_FLAT pair the same plane with min == max,
//     -0.0 and +0.0 are never taken for equal, and no two groups left to the general pairs and the tail share an interval;
//   - the tables are exactly as large as the layout says (ASan sees a byte too many), never larger than build_sweep_layout's,
//     their pitch is an odd number of 8-byte units and the 8 tables start at 8 different bank positions; with every pair general
//     they are build_sweep_layout's tables byte for byte;
//   - slot k of the layout made of the permuted groups is the first primitive of permuted group k, and its chain is the group;
//   - the kernel's loops in plain C++ (pt_kernels.h: sweep_shared_pairs, pt_trace_sweep_body.h step (3): the same subtractions,
//     products, maxima and minima in the same order) over the class-ordered tables give, for some thousand rays in all 8 octants
//     (origins inside, outside and exactly on planes of the boxes), the hit word of today's loop over build_sweep_layout's
//     tables with the permutation applied.
// Sets: fixed ones (1 group, 2 groups, 32 groups of 16 coplanar pairs, 31 groups that share nothing, signed zeros, a box flat on
// two axes, every class on every axis at once) and random ones with planted intervals.  `sweep_pairs_check FILE [MIN_SHARING]`
// checks the N x 6 floats of FILE (the leaf boxes of a scene) the same way, fails below MIN_SHARING sharing pairs under any tree,
// and prints the classes of the first tree: "groups G flat x y z share x y z general g single s".
// Stand-alone; built with -fsanitize=address,undefined by tests/test_sweep_pairs_host.py.  Exit code 0 = all held.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <random>
#include <vector>

#include "pt_sweep_pairs.h"

namespace {

using ptl::DNode;
using ptl::DPrim;
using ptl::SweepGroup;
using ptl::SweepPairClasses;

uint64_t errors = 0;
void fail(const char* what, int n = -1) {
    if (errors++ < 10) std::fprintf(stderr, "FAIL: %s (n = %d)\n", what, n);
}

struct Box { float v[6]; };
bool same_bits(float a, float b) { return std::memcmp(&a, &b, 4) == 0; }

// A random binary tree over primitives 0 .. n-1 in inner-only form (tests/native/leaf_sweep_check.cpp has the same one).
std::vector<DNode> random_tree(int n, const std::vector<Box>& box, std::mt19937& rng) {
    std::vector<DNode> nodes((size_t)n - 1);
    std::memset(nodes.data(), 0, nodes.size() * sizeof(DNode));
    std::vector<int32_t> prims(n);
    for (int k = 0; k < n; k++) prims[k] = k;
    for (int k = n - 1; k > 0; k--) std::swap(prims[k], prims[rng() % (uint32_t)(k + 1)]);
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
                ref = ~prims[lo];
                std::memcpy(side ? nodes[j.node].rmin : nodes[j.node].lmin, box[prims[lo]].v, sizeof(Box));
            } else {
                ref = next++;
                todo.push_back({lo, hi, ref});
            }
            (side ? nodes[j.node].right : nodes[j.node].left) = ref;
        }
    }
    return nodes;
}

std::vector<DPrim> make_prims(int n) {
    std::vector<DPrim> p(n);
    for (int k = 0; k < n; k++) {
        for (int c = 0; c < 9; c++) p[k].v[c] = (float)(100 * k + c) * 0.37f - 50.0f;
        p[k].info = 1000 + k;
        p[k].light = -1;
        p[k].pad = 0x5a5a5a5a;
    }
    return p;
}

struct Ray { float o[3], inv[3]; uint32_t oct; };

// hits = 2 * hits + hit, the kernel's add-with-carry
void shift_in(uint32_t& h, float tf, float tn0) { h = h + h + (tf >= tn0 ? 1u : 0u); }

// Today's loop over build_sweep_layout's tables: box_sides of pt_trace_sweep_body.h, group by group.
uint32_t sweep_plain(const unsigned char* tab, uint32_t pitch, int count, const Ray& r) {
    const float* p = reinterpret_cast<const float*>(tab + r.oct * pitch);
    uint32_t h = 0;
    for (int k = 0; k < count; k++, p += 6) {
        const float tn = std::fmax(std::fmax((p[0] - r.o[0]) * r.inv[0], (p[1] - r.o[1]) * r.inv[1]), (p[2] - r.o[2]) * r.inv[2]);
        const float tf = std::fmin(std::fmin((p[3] - r.o[0]) * r.inv[0], (p[4] - r.o[1]) * r.inv[1]), (p[5] - r.o[2]) * r.inv[2]);
        shift_in(h, tf, std::fmax(0.0f, tn));
    }
    return ptl::sweep_hits_align(h, (uint32_t)count);
}

// The class loops over build_sweep_pair_tables' tables: sweep_shared_pairs<AX, FLAT> of pt_kernels.h, then the general pairs and the tail.
uint32_t sweep_classes(const unsigned char* tab, uint32_t pitch, const SweepPairClasses& cls, int count, const Ray& r) {
    const float* p = reinterpret_cast<const float*>(tab + r.oct * pitch);
    uint32_t h = 0;
    for (int c = 0; c < 6; c++) {
        const int ax = c % 3, B = ax == 0 ? 1 : 0, C = ax == 2 ? 1 : 2;
        const bool flat = c < 3;
        for (int k = flat ? cls.flat[ax] : cls.share[ax]; k != 0; k--, p += ptl::kSweepSharedPairFloats) {
            float na[3], fa[3], nb[3], fb[3];
            na[ax] = (p[0] - r.o[ax]) * r.inv[ax];
            fa[ax] = flat ? na[ax] : (p[1] - r.o[ax]) * r.inv[ax];
            nb[ax] = na[ax]; fb[ax] = fa[ax];
            na[B] = (p[2] - r.o[B]) * r.inv[B]; na[C] = (p[3] - r.o[C]) * r.inv[C]; fa[B] = (p[4] - r.o[B]) * r.inv[B]; fa[C] = (p[5] - r.o[C]) * r.inv[C];
            nb[B] = (p[6] - r.o[B]) * r.inv[B]; nb[C] = (p[7] - r.o[C]) * r.inv[C]; fb[B] = (p[8] - r.o[B]) * r.inv[B]; fb[C] = (p[9] - r.o[C]) * r.inv[C];
            shift_in(h, std::fmin(std::fmin(fa[0], fa[1]), fa[2]), std::fmax(0.0f, std::fmax(std::fmax(na[0], na[1]), na[2])));
            shift_in(h, std::fmin(std::fmin(fb[0], fb[1]), fb[2]), std::fmax(0.0f, std::fmax(std::fmax(nb[0], nb[1]), nb[2])));
        }
    }
    for (int k = 2 * cls.general + cls.single; k != 0; k--, p += 6) {
        const float tn = std::fmax(std::fmax((p[0] - r.o[0]) * r.inv[0], (p[1] - r.o[1]) * r.inv[1]), (p[2] - r.o[2]) * r.inv[2]);
        const float tf = std::fmin(std::fmin((p[3] - r.o[0]) * r.inv[0], (p[4] - r.o[1]) * r.inv[1]), (p[5] - r.o[2]) * r.inv[2]);
        shift_in(h, tf, std::fmax(0.0f, tn));
    }
    return ptl::sweep_hits_align(h, (uint32_t)count);
}

// Rays in every octant: origins inside the scene's bounds, outside of them, and with coordinates taken from the boxes' own
// planes (plane - o == 0); directions with no zero component (such a ray does not reach the sweep: its 1/d is not finite).
std::vector<Ray> make_rays(const std::vector<Box>& box, int per_octant, uint32_t seed) {
    std::mt19937 rng(seed);
    float lo = 3.0e38f, hi = -3.0e38f;
    for (const Box& b : box)
        for (int c = 0; c < 6; c++) { lo = std::fmin(lo, b.v[c]); hi = std::fmax(hi, b.v[c]); }
    const float mid = 0.5f * (lo + hi), half = 0.5f * (hi - lo) + 0.25f;
    std::uniform_real_distribution<float> u(-1.0f, 1.0f), pos(0.01f, 1.0f);
    std::vector<Ray> rays;
    for (uint32_t oct = 0; oct < 8; oct++)
        for (int k = 0; k < per_octant; k++) {
            Ray r;
            r.oct = oct;
            const float reach = k % 4 == 3 ? 2.5f : 1.0f;
            for (int a = 0; a < 3; a++) {
                r.o[a] = mid + reach * half * u(rng);
                if (k % 4 == 1 || (k % 4 == 2 && a == (k / 4) % 3)) r.o[a] = box[rng() % box.size()].v[a + 3 * (rng() & 1u)];
                const float d = ((oct >> a) & 1u) ? -pos(rng) : pos(rng);
                r.inv[a] = 1.0f / d;
            }
            rays.push_back(r);
        }
    return rays;
}

struct Result { int count = 0; SweepPairClasses cls{}; };

Result check_set(const std::vector<DNode>& nodes, int n, const std::vector<Box>& box, const std::vector<Ray>& rays) {
    Result res;
    SweepGroup g[ptl::kSweepMaxPrims];
    const uint32_t stride = 64u;
    const int num_nodes = (int)nodes.size();
    const int count = ptl::build_sweep_groups(nodes.data(), num_nodes, n, stride, g);
    res.count = count;
    if (count < 1) { fail("no groups", n); return res; }
    SweepGroup out[ptl::kSweepMaxBoxes], out2[ptl::kSweepMaxBoxes];
    int perm[ptl::kSweepMaxBoxes], perm2[ptl::kSweepMaxBoxes];
    SweepPairClasses cls{}, cls2{};
    if (count > ptl::kSweepMaxBoxes) {
        if (ptl::build_sweep_pairs(g, count, nodes.data(), num_nodes, stride, out, perm, &cls)) fail("more groups than hit bits paired", n);
        return res;
    }
    if (!ptl::build_sweep_pairs(g, count, nodes.data(), num_nodes, stride, out, perm, &cls)) { fail("pairing refused", n); return res; }
    res.cls = cls;
    // a permutation, the same one every time
    uint32_t seen = 0;
    for (int k = 0; k < count; k++) {
        if (perm[k] < 0 || perm[k] >= count || ((seen >> perm[k]) & 1u)) { fail("not a permutation", n); return res; }
        seen |= 1u << perm[k];
        if (std::memcmp(&out[k], &g[perm[k]], sizeof(SweepGroup)) != 0) fail("out[k] is not groups[perm[k]]", n);
    }
    if (!ptl::build_sweep_pairs(g, count, nodes.data(), num_nodes, stride, out2, perm2, &cls2) || std::memcmp(perm, perm2, sizeof(int) * (size_t)count) != 0 ||
        std::memcmp(&cls, &cls2, sizeof cls) != 0)
        fail("pairing is not deterministic", n);
    if (ptl::sweep_pairs_groups(cls) != (uint32_t)count || cls.single != (count & 1)) fail("class counts do not add up", n);
    // the classes are what they say
    auto gbox = [&](int k) { return box[ptl::sweep_lowest(ptl::sweep_group_mask(out[k]))].v; };
    int k = 0;
    for (int c = 0; c < 6; c++) {
        const int ax = c % 3;
        for (int p = 0; p < (c < 3 ? cls.flat[ax] : cls.share[ax]); p++, k += 2) {
            const float *a = gbox(k), *b = gbox(k + 1);
            if (!same_bits(a[ax], b[ax]) || !same_bits(a[3 + ax], b[3 + ax])) fail("a sharing pair whose intervals differ in their bits", n);
            const bool is_flat = same_bits(a[ax], a[3 + ax]);
            if ((c < 3) != is_flat) fail("SHARE_FLAT on an interval that is not flat, or SHARE on one that is", n);
            if (c >= 3)                      // greedy by saving: a SHARE pair has no flat plane in common on another axis
                for (int x = 0; x < 3; x++)
                    if (same_bits(a[x], b[x]) && same_bits(a[3 + x], b[3 + x]) && same_bits(a[x], a[3 + x])) fail("a SHARE pair that could be SHARE_FLAT", n);
        }
    }
    for (int i = k; i < count; i++)
        for (int j = i + 1; j < count; j++)
            for (int x = 0; x < 3; x++)
                if (same_bits(gbox(i)[x], gbox(j)[x]) && same_bits(gbox(i)[3 + x], gbox(j)[3 + x])) fail("two leftover groups share an interval", n);
    // layouts: today's, and the permuted one with its tables in class order
    const std::vector<DPrim> prims = make_prims(n);
    const uint32_t bytes = ptl::sweep_layout_bytes((uint32_t)count, (uint32_t)n), slots_off = ptl::sweep_slots_off((uint32_t)count);
    std::vector<unsigned char> plain(bytes), paired(bytes), again(bytes);
    if (!ptl::build_sweep_layout(g, count, nodes.data(), num_nodes, stride, prims.data(), n, plain.data()) ||
        !ptl::build_sweep_layout(out, count, nodes.data(), num_nodes, stride, prims.data(), n, paired.data())) { fail("layout refused", n); return res; }
    std::vector<unsigned char> slots_before(paired.begin() + slots_off, paired.end());
    if (!ptl::build_sweep_pair_tables(out, count, cls, nodes.data(), num_nodes, stride, paired.data())) { fail("pair tables refused", n); return res; }
    if (std::memcmp(slots_before.data(), paired.data() + slots_off, slots_before.size()) != 0) fail("pair tables touched the slot records", n);
    const uint32_t pitch = ptl::sweep_pairs_pitch(cls), plain_pitch = ptl::sweep_box_pitch((uint32_t)count);
    if (pitch > plain_pitch || pitch % 8u || !((pitch / 8u) & 1u)) fail("pitch: larger than today's or not an odd number of 8-byte units", n);
    uint32_t positions = 0;
    for (uint32_t o = 0; o < 8; o++) positions |= 1u << ((o * pitch / 8u) % 32u);
    if (__builtin_popcount(positions) != 8) fail("two box tables start at the same bank position", n);
    again = plain;
    const SweepPairClasses none = ptl::sweep_pairs_none((uint32_t)count);
    if (ptl::sweep_pairs_pitch(none) != plain_pitch || !ptl::build_sweep_pair_tables(g, count, none, nodes.data(), num_nodes, stride, again.data()) || again != plain)
        fail("every pair general: not build_sweep_layout's tables", n);
    SweepPairClasses bad = cls;
    bad.general++;
    if (ptl::build_sweep_pair_tables(out, count, bad, nodes.data(), num_nodes, stride, again.data())) fail("classes that do not add up accepted", n);
    // slot k: the first primitive of permuted group k, its chain the group
    const DPrim* slots = reinterpret_cast<const DPrim*>(paired.data() + slots_off);
    for (int s = 0; s < count; s++) {
        uint64_t m = ptl::sweep_group_mask(out[s]), chain = 0;
        if ((int)ptl::sweep_link_prim((uint32_t)slots[s].pad) != ptl::sweep_lowest(m)) fail("slot k is not the first primitive of permuted group k", n);
        for (int slot = s, steps = 0; steps <= n; steps++) {
            const uint32_t link = (uint32_t)slots[slot].pad;
            chain |= 1ull << ptl::sweep_link_prim(link);
            slot = (int)ptl::sweep_link_next(link);
            if (slot == 0) break;
            if (slot < count || slot >= n) { fail("chain leaves the successors", n); break; }
        }
        if (chain != m) fail("chain is not the permuted group", n);
    }
    // hit words
    for (const Ray& r : rays) {
        const uint32_t hp = sweep_plain(plain.data(), plain_pitch, count, r), hc = sweep_classes(paired.data(), pitch, cls, count, r);
        uint32_t want = 0;
        for (int s = 0; s < count; s++)
            if (hp & (0x80000000u >> perm[s])) want |= 0x80000000u >> s;
        if (hc != want) { fail("hit word of the class loops is not today's with the permutation applied", n); break; }
        if (sweep_classes(plain.data(), plain_pitch, none, count, r) != hp) { fail("every pair general: not today's hit word", n); break; }
    }
    return res;
}

// A set under several trees; returns the classes of the first and the smallest number of sharing pairs seen.
Result check_boxes(const std::vector<Box>& box, uint32_t seed, int trees, int* min_sharing = nullptr) {
    const int n = (int)box.size();
    const std::vector<Ray> rays = make_rays(box, 384, seed);
    std::mt19937 rng(seed);
    Result first;
    for (int t = 0; t < trees; t++) {
        const Result r = check_set(random_tree(n, box, rng), n, box, rays);
        if (t == 0) first = r;
        const int sharing = (int)(ptl::sweep_pairs_flat(r.cls) + ptl::sweep_pairs_shared(r.cls));
        if (min_sharing && (t == 0 || sharing < *min_sharing)) *min_sharing = sharing;
    }
    return first;
}

Box mk(float x0, float y0, float z0, float x1, float y1, float z1) { return Box{{x0, y0, z0, x1, y1, z1}}; }
Box distinct(int k) { const float f = (float)k; return mk(-1.0f - 0.11f * f, -2.0f - 0.13f * f, -3.0f - 0.17f * f, 1.0f + 0.19f * f, 2.0f + 0.23f * f, 3.0f + 0.29f * f); }

void fixed_sets() {
    {   // 2 primitives with one box: ONE group, the tail alone
        const Result r = check_boxes({distinct(0), distinct(0)}, 1, 1);
        if (r.count != 1 || r.cls.single != 1 || ptl::sweep_pairs_groups(r.cls) != 1) fail("one group");
    }
    {   // 2 groups that share nothing: one general pair
        const Result r = check_boxes({distinct(0), distinct(1)}, 2, 2);
        if (r.count != 2 || r.cls.general != 1 || r.cls.single) fail("two groups");
    }
    {   // 32 groups: 16 planes z = const with two different boxes each -> 16 pairs of SHARE_FLAT_z, the hit word full
        std::vector<Box> box;
        for (int k = 0; k < 16; k++) {
            const float z = -0.5f * (float)(k + 1), s = 0.4f + 0.1f * (float)k;
            box.push_back(mk(-s, -s, z, s, s, z));
            box.push_back(mk(-0.9f * s, -0.2f * s, z, 0.3f * s, 0.9f * s, z));
        }
        const Result r = check_boxes(box, 3, 4);
        if (r.count != 32 || r.cls.flat[2] != 16 || r.cls.general || r.cls.single) fail("32 groups in 16 coplanar pairs");
    }
    {   // 31 groups that share nothing: 15 general pairs and the tail, the order and the tables of today
        std::vector<Box> box;
        for (int k = 0; k < 31; k++) box.push_back(distinct(k));
        const Result r = check_boxes(box, 4, 3);
        if (r.count != 31 || r.cls.general != 15 || r.cls.single != 1) fail("31 groups that share nothing");
    }
    {   // -0.0 and +0.0: two planes.  Flat boxes in z = -0 and z = +0 with nothing else in common: no pair
        const Result r = check_boxes({mk(-2, -1, -0.0f, -0.5f, 1, -0.0f), mk(0.5f, -1.5f, 0.0f, 2, 1.25f, 0.0f)}, 5, 2);
        if (ptl::sweep_pairs_flat(r.cls) || ptl::sweep_pairs_shared(r.cls) || r.cls.general != 1) fail("-0.0 and +0.0 paired as one plane");
    }
    {   // ... with the same y interval: SHARE_y, not SHARE_FLAT_z; and [-0, 1] is not [+0, 1]
        const Result r = check_boxes({mk(-2, -1, -0.0f, -0.5f, 1, -0.0f), mk(0.5f, -1, 0.0f, 2, 1, 0.0f), mk(3, -0.0f, 1, 4, 1, 2), mk(5, 0.0f, 3, 6, 1, 4)}, 6, 4);
        if (r.cls.flat[2] || r.cls.share[1] != 1 || r.cls.general != 1) fail("signed zeros: SHARE_y alone expected");
    }
    {   // a box flat on two axes (a segment along x) in the plane of a floor panel: SHARE_FLAT_y; two such segments: the lower axis wins
        const Result r = check_boxes({mk(-1.8f, -1, -1.9f, 1.6f, -1, 1.4f), mk(-0.6f, -1, -0.5f, 0.9f, -1, -0.5f), distinct(2)}, 7, 3);
        if (r.cls.flat[1] != 1 || r.cls.single != 1) fail("flat on two axes: SHARE_FLAT_y expected");
        const Result s = check_boxes({mk(-0.6f, -1, -0.5f, 0.9f, -1, -0.5f), mk(0.2f, -1, -0.5f, 1.9f, -1, -0.5f)}, 8, 2);
        if (s.cls.flat[1] != 1 || s.cls.flat[2]) fail("flat on two shared axes: the lower axis");
        const Result p = check_boxes({mk(1, 2, 3, 1, 2, 3), mk(1, 2, 3.5f, 1, 2, 3.5f), distinct(1), distinct(3)}, 9, 2);       // points
        if (p.cls.flat[0] != 1 || p.cls.general != 1) fail("boxes flat on three axes");
    }
    {   // every class on every axis at once, and leftovers
        std::vector<Box> box;
        for (int a = 0; a < 3; a++) {
            Box f0 = distinct(10 + a), f1 = distinct(13 + a), s0 = distinct(16 + a), s1 = distinct(19 + a);
            f0.v[a] = f0.v[3 + a] = f1.v[a] = f1.v[3 + a] = 0.25f * (float)(a + 1);
            s1.v[a] = s0.v[a]; s1.v[3 + a] = s0.v[3 + a];
            box.insert(box.end(), {f0, f1, s0, s1});
        }
        box.push_back(distinct(30)); box.push_back(distinct(31)); box.push_back(distinct(32));
        const Result r = check_boxes(box, 10, 6);
        for (int a = 0; a < 3; a++)
            if (r.cls.flat[a] != 1 || r.cls.share[a] != 1) fail("every class on every axis", a);
        if (r.cls.general != 1 || r.cls.single != 1) fail("every class: the leftovers");
    }
}

void random_sets() {
    std::mt19937 rng(77);
    for (int rep = 0; rep < 60; rep++) {
        const int n = 2 + (int)(rng() % 47u);
        // intervals drawn from a small pool per axis (some flat, +0 and -0 among the bounds), boxes drawn from those
        std::vector<Box> box(n);
        float pool[3][6][2];
        for (int a = 0; a < 3; a++)
            for (int k = 0; k < 6; k++) {
                const float lo = (float)((int)(rng() % 9u) - 4) * 0.5f * ((rng() & 1u) ? 1.0f : -1.0f);
                pool[a][k][0] = lo;
                pool[a][k][1] = (rng() % 3u) ? lo + 0.25f * (float)(1 + rng() % 5u) : lo;
            }
        for (int p = 0; p < n; p++)
            for (int a = 0; a < 3; a++) {
                if (rng() % 3u) {
                    const int k = (int)(rng() % 6u);
                    box[p].v[a] = pool[a][k][0]; box[p].v[3 + a] = pool[a][k][1];
                } else {
                    box[p].v[a] = -5.0f + 0.01f * (float)(rng() % 400u); box[p].v[3 + a] = 1.0f + 0.01f * (float)(rng() % 400u);
                }
            }
        check_boxes(box, 100u + (uint32_t)rep, 2);
    }
}

int scene_boxes(const char* path, int want_sharing) {
    std::FILE* f = std::fopen(path, "rb");
    if (!f) { std::fprintf(stderr, "cannot open %s\n", path); return 2; }
    std::vector<Box> box;
    Box b;
    while (std::fread(b.v, sizeof(float), 6, f) == 6) box.push_back(b);
    std::fclose(f);
    const int n = (int)box.size();
    if (n < 2 || n > ptl::kSweepMaxPrims) { std::fprintf(stderr, "%d boxes\n", n); return 2; }
    int min_sharing = 0;
    const Result r = check_boxes(box, 5, 8, &min_sharing);
    if (min_sharing < want_sharing) fail("fewer sharing pairs than asked for", min_sharing);
    std::printf("groups %d flat %d %d %d share %d %d %d general %d single %d\n", r.count, r.cls.flat[0], r.cls.flat[1], r.cls.flat[2],
                r.cls.share[0], r.cls.share[1], r.cls.share[2], r.cls.general, r.cls.single);
    return errors ? 1 : 0;
}

}  // namespace

int main(int argc, char** argv) {
    if (argc > 1) return scene_boxes(argv[1], argc > 2 ? std::atoi(argv[2]) : 0);
    fixed_sets();
    random_sets();
    if (errors) {
        std::fprintf(stderr, "%llu checks failed\n", (unsigned long long)errors);
        return 1;
    }
    std::puts("sweep_pairs_check: ok");
    return 0;
}
