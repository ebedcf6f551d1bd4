// The sweep's PAIR2 records (csrc/pt_sweep_families.h): two groups sharing two axis intervals, in front of the pair classes of
// csrc/pt_sweep_pairs.h.  For every set of leaf boxes, under several random trees (the order of the groups follows the tree) and
// under both values of option "sweep_families" (on, off):
//   - build_sweep_families gives a permutation of the groups, the class counts add up, and it gives the same one when asked again;
//     mode off is build_sweep_pairs' order and classes exactly;
//   - every record shares what its class says BIT FOR BIT — a PAIR2 both axes other than u, each flat or not as its class says —
//     so -0.0 and +0.0 are never taken for equal;
//   - the count model's sum is never above that of build_sweep_pairs' pairing, and a set small enough to try every placement
//     (up to 9 groups) has no placement with a smaller sum;
//   - the tables are exactly as large as the layout says (ASan sees a byte too many), never larger than build_sweep_layout's,
//     their pitch is an odd number of 8-byte units and the 8 tables start at 8 different bank positions; the slot records are
//     not touched; classes that do not add up are refused;
//   - the kernel's loops in plain C++ (pt_kernels.h: sweep_pair2, sweep_shared_pairs, pt_trace_sweep_body.h step (3): the same
//     subtractions, products, maxima and minima in the same order) over the class-ordered tables give, for some thousand rays in
//     all 8 octants (origins inside, outside and exactly on planes of the boxes), the hit word of the plain loop over
//     build_sweep_layout's tables with the permutation applied.
// Sets: fixed ones (1, 2, 3, 4, 5, 31 and 32 groups, every PAIR2 class, signed zeros, a box flat on two axes) and random ones with
// planted intervals.  `sweep_families_check FILE` checks the N x 6 floats of FILE (the leaf boxes of a scene) the same way and
// prints, of the first tree, "groups G model ON OFF pair2 <12> flat x y z share x y z general g single s" (the classes of mode on).
// Stand-alone; built with -fsanitize=address,undefined by tests/test_sweep_families_host.py.  Exit code 0 = all held.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <random>
#include <vector>

#include "pt_sweep_families.h"

namespace {

using ptl::DNode;
using ptl::DPrim;
using ptl::SweepClasses;
using ptl::SweepGroup;

uint64_t errors = 0;
void fail(const char* what, int n = -1) {
    if (errors++ < 10) std::fprintf(stderr, "FAIL: %s (n = %d)\n", what, n);
}

struct Box { float v[6]; };
bool same_bits(float a, float b) { return std::memcmp(&a, &b, 4) == 0; }

// A random binary tree over primitives 0 .. n-1 in inner-only form (tests/native/sweep_pairs_check.cpp has the same one).
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
void shift_in(uint32_t& h, const float* n, const float* f) {
    shift_in(h, std::fmin(std::fmin(f[0], f[1]), f[2]), std::fmax(0.0f, std::fmax(std::fmax(n[0], n[1]), n[2])));
}
float slab(float plane, const Ray& r, int a) { return (plane - r.o[a]) * r.inv[a]; }

// The plain loop over build_sweep_layout's tables: box_sides of pt_trace_sweep_body.h, group by group.
const float* sweep_general(const float* p, int groups, const Ray& r, uint32_t& h) {
    for (int k = 0; k < groups; k++, p += 6) {
        const float n[3] = {slab(p[0], r, 0), slab(p[1], r, 1), slab(p[2], r, 2)}, f[3] = {slab(p[3], r, 0), slab(p[4], r, 1), slab(p[5], r, 2)};
        shift_in(h, n, f);
    }
    return p;
}
uint32_t sweep_plain(const unsigned char* tab, uint32_t pitch, int count, const Ray& r) {
    uint32_t h = 0;
    sweep_general(reinterpret_cast<const float*>(tab + r.oct * pitch), count, r, h);
    return ptl::sweep_hits_align(h, (uint32_t)count);
}

// The class loops over build_sweep_family_tables' tables: sweep_pair2<U, FB, FC>, sweep_shared_pairs<AX, FLAT>
// of pt_kernels.h, then the general pairs and the tail.
uint32_t sweep_classes(const unsigned char* tab, uint32_t pitch, const SweepClasses& cls, int count, const Ray& r) {
    const float* p = reinterpret_cast<const float*>(tab + r.oct * pitch);
    uint32_t h = 0;
    for (int u = 0; u < 3; u++)
        for (int fl = 0; fl < 4; fl++) {
            const int B = u == 0 ? 1 : 0, C = u == 2 ? 1 : 2;
            const bool fb = fl & 1, fc = fl & 2;
            for (int k = cls.fam.pair2[u][fl]; k != 0; k--, p += ptl::kSweepPair2Floats) {
                float na[3], fa[3], nb[3], fbb[3];
                na[B] = slab(p[0], r, B); fa[B] = fb ? na[B] : slab(p[1], r, B);
                na[C] = slab(p[2], r, C); fa[C] = fc ? na[C] : slab(p[3], r, C);
                nb[B] = na[B]; fbb[B] = fa[B]; nb[C] = na[C]; fbb[C] = fa[C];
                na[u] = slab(p[4], r, u); fa[u] = slab(p[5], r, u); nb[u] = slab(p[6], r, u); fbb[u] = slab(p[7], r, u);
                shift_in(h, na, fa);
                shift_in(h, nb, fbb);
            }
        }
    for (int c = 0; c < 6; c++) {
        const int ax = c % 3, B = ax == 0 ? 1 : 0, C = ax == 2 ? 1 : 2;
        const bool flat = c < 3;
        for (int k = flat ? cls.pairs.flat[ax] : cls.pairs.share[ax]; k != 0; k--, p += ptl::kSweepSharedPairFloats) {
            float na[3], fa[3], nb[3], fb[3];
            na[ax] = slab(p[0], r, ax);
            fa[ax] = flat ? na[ax] : slab(p[1], r, ax);
            nb[ax] = na[ax]; fb[ax] = fa[ax];
            na[B] = slab(p[2], r, B); na[C] = slab(p[3], r, C); fa[B] = slab(p[4], r, B); fa[C] = slab(p[5], r, C);
            nb[B] = slab(p[6], r, B); nb[C] = slab(p[7], r, C); fb[B] = slab(p[8], r, B); fb[C] = slab(p[9], r, C);
            shift_in(h, na, fa);
            shift_in(h, nb, fb);
        }
    }
    sweep_general(p, 2 * cls.pairs.general + cls.pairs.single, r, h);
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

// The smallest model sum over EVERY placement of a small set, by the model's own rules and nothing of the search's.
int brute_best(const std::vector<const float*>& b, uint32_t used) {
    const int n = (int)b.size();
    int i = 0;
    while (i < n && ((used >> i) & 1u)) i++;
    if (i == n) return 0;
    auto shares = [&](int p, int q, int a) { return same_bits(b[p][a], b[q][a]) && same_bits(b[p][3 + a], b[q][3 + a]); };
    auto axis_cost = [&](int p, int a) { return same_bits(b[p][a], b[p][3 + a]) ? 2 : 4; };
    // group i is left over: counted 17.5 each, corrected by the caller for the single (x2 to stay in integers)
    int best = 35 + brute_best(b, used | 1u << i);
    for (int j = i + 1; j < n; j++) {
        if ((used >> j) & 1u) continue;
        int cost = 1 + 10, shared = 0;
        for (int a = 0; a < 3; a++) {
            if (shares(i, j, a) && shared < 2) { cost += axis_cost(i, a); shared++; }
            else cost += 8;
        }
        if (!shared) continue;
        best = std::min(best, 2 * cost + brute_best(b, used | 1u << i | 1u << j));
    }
    return best;
}

struct Result { int count = 0; SweepClasses cls[2] = {}; uint32_t model[2] = {0, 0}; };

void check_mode(const std::vector<DNode>& nodes, int n, const std::vector<Box>& box, const std::vector<Ray>& rays, const SweepGroup* g, int count,
                int mode, Result& res) {
    const uint32_t stride = 64u;
    const int num_nodes = (int)nodes.size();
    SweepGroup out[ptl::kSweepMaxBoxes], out2[ptl::kSweepMaxBoxes];
    int perm[ptl::kSweepMaxBoxes], perm2[ptl::kSweepMaxBoxes];
    SweepClasses cls{}, cls2{};
    if (!ptl::build_sweep_families(g, count, nodes.data(), num_nodes, stride, mode, out, perm, &cls)) { fail("families refused", n); return; }
    res.cls[mode] = cls;
    res.model[mode] = ptl::sweep_valu_model(cls);
    // a permutation, the same one every time
    uint32_t seen = 0;
    for (int k = 0; k < count; k++) {
        if (perm[k] < 0 || perm[k] >= count || ((seen >> perm[k]) & 1u)) { fail("not a permutation", n); return; }
        seen |= 1u << perm[k];
        if (std::memcmp(&out[k], &g[perm[k]], sizeof(SweepGroup)) != 0) fail("out[k] is not groups[perm[k]]", n);
    }
    if (!ptl::build_sweep_families(g, count, nodes.data(), num_nodes, stride, mode, out2, perm2, &cls2) ||
        std::memcmp(perm, perm2, sizeof(int) * (size_t)count) != 0 || std::memcmp(&cls, &cls2, sizeof cls) != 0)
        fail("placement is not deterministic", n);
    if (ptl::sweep_classes_groups(cls) != (uint32_t)count || cls.pairs.single != (count & 1)) fail("class counts do not add up", n);
    if (mode == ptl::kSweepFamiliesOff) {
        ptl::SweepPairClasses pc{};
        if (!ptl::build_sweep_pairs(g, count, nodes.data(), num_nodes, stride, out2, perm2, &pc) || std::memcmp(perm, perm2, sizeof(int) * (size_t)count) != 0 ||
            std::memcmp(&cls.pairs, &pc, sizeof pc) != 0 || ptl::sweep_pair2_records(cls.fam))
            fail("mode off is not build_sweep_pairs' pairing", n);
    }
    // the records are what their classes say
    auto gbox = [&](int k) { return box[ptl::sweep_lowest(ptl::sweep_group_mask(out[k]))].v; };
    auto shares = [&](int p, int q, int a, bool flat) {
        const float *x = gbox(p), *y = gbox(q);
        return same_bits(x[a], y[a]) && same_bits(x[3 + a], y[3 + a]) && same_bits(x[a], x[3 + a]) == flat;
    };
    int k = 0;
    for (int u = 0; u < 3; u++)
        for (int fl = 0; fl < 4; fl++)
            for (int p = 0; p < cls.fam.pair2[u][fl]; p++, k += 2)
                if (!shares(k, k + 1, u == 0 ? 1 : 0, fl & 1) || !shares(k, k + 1, u == 2 ? 1 : 2, fl & 2)) fail("a PAIR2 that does not share what its class says", n);
    for (int c = 0; c < 6; c++)
        for (int p = 0; p < (c < 3 ? cls.pairs.flat[c % 3] : cls.pairs.share[c % 3]); p++, k += 2)
            if (!shares(k, k + 1, c % 3, c < 3)) fail("a sharing pair that does not share what its class says", n);
    if (mode != ptl::kSweepFamiliesOff)
        for (int i = k; i < count; i++)
            for (int j = i + 1; j < count; j++)
                for (int x = 0; x < 3; x++)
                    if (same_bits(gbox(i)[x], gbox(j)[x]) && same_bits(gbox(i)[3 + x], gbox(j)[3 + x])) fail("two leftover groups share an interval", n);
    // layouts: the plain one, and the permuted one with its tables in class order
    const std::vector<DPrim> prims = make_prims(n);
    const uint32_t bytes = ptl::sweep_layout_bytes((uint32_t)count, (uint32_t)n), slots_off = ptl::sweep_slots_off((uint32_t)count);
    std::vector<unsigned char> plain(bytes), placed(bytes), again(bytes);
    if (!ptl::build_sweep_layout(g, count, nodes.data(), num_nodes, stride, prims.data(), n, plain.data()) ||
        !ptl::build_sweep_layout(out, count, nodes.data(), num_nodes, stride, prims.data(), n, placed.data())) { fail("layout refused", n); return; }
    std::vector<unsigned char> slots_before(placed.begin() + slots_off, placed.end());
    // the box region alone, in a buffer of exactly its size: ASan sees a byte written behind it
    std::vector<unsigned char> region(slots_off);
    if (!ptl::build_sweep_family_tables(out, count, cls, nodes.data(), num_nodes, stride, region.data())) { fail("family tables refused", n); return; }
    if (!ptl::build_sweep_family_tables(out, count, cls, nodes.data(), num_nodes, stride, placed.data())) { fail("family tables refused", n); return; }
    if (std::memcmp(region.data(), placed.data(), slots_off) != 0) fail("family tables differ between two calls", n);
    if (std::memcmp(slots_before.data(), placed.data() + slots_off, slots_before.size()) != 0) fail("family tables touched the slot records", n);
    const uint32_t pitch = ptl::sweep_classes_pitch(cls), plain_pitch = ptl::sweep_box_pitch((uint32_t)count);
    if (pitch > plain_pitch || pitch % 8u || !((pitch / 8u) & 1u)) fail("pitch: larger than the plain one or not an odd number of 8-byte units", n);
    uint32_t positions = 0;
    for (uint32_t o = 0; o < 8; o++) positions |= 1u << ((o * pitch / 8u) % 32u);
    if (__builtin_popcount(positions) != 8) fail("two box tables start at the same bank position", n);
    for (uint32_t b = 8u * pitch; b < slots_off; b++)
        if (placed[b]) { fail("bytes behind the 8 tables are not zero", n); break; }
    SweepClasses bad = cls;
    bad.pairs.general++;
    if (ptl::build_sweep_family_tables(out, count, bad, nodes.data(), num_nodes, stride, again.data())) fail("classes that do not add up accepted", n);
    // slot k: the first primitive of permuted group k
    const DPrim* slots = reinterpret_cast<const DPrim*>(placed.data() + slots_off);
    for (int s = 0; s < count; s++)
        if ((int)ptl::sweep_link_prim((uint32_t)slots[s].pad) != ptl::sweep_lowest(ptl::sweep_group_mask(out[s]))) fail("slot k is not the first primitive of permuted group k", n);
    // hit words
    for (const Ray& r : rays) {
        const uint32_t hp = sweep_plain(plain.data(), plain_pitch, count, r), hc = sweep_classes(placed.data(), pitch, cls, count, r);
        uint32_t want = 0;
        for (int s = 0; s < count; s++)
            if (hp & (0x80000000u >> perm[s])) want |= 0x80000000u >> s;
        if (hc != want) { fail("hit word of the class loops is not the plain loop's with the permutation applied", n); break; }
    }
}

Result check_set(const std::vector<DNode>& nodes, int n, const std::vector<Box>& box, const std::vector<Ray>& rays) {
    Result res;
    SweepGroup g[ptl::kSweepMaxPrims];
    const int num_nodes = (int)nodes.size();
    const int count = ptl::build_sweep_groups(nodes.data(), num_nodes, n, 64u, g);
    res.count = count;
    if (count < 1) { fail("no groups", n); return res; }
    if (count > ptl::kSweepMaxBoxes) {
        SweepGroup out[ptl::kSweepMaxBoxes];
        int perm[ptl::kSweepMaxBoxes];
        SweepClasses cls{};
        if (ptl::build_sweep_families(g, count, nodes.data(), num_nodes, 64u, ptl::kSweepFamiliesOn, out, perm, &cls)) fail("more groups than hit bits placed", n);
        return res;
    }
    for (int mode = 0; mode < 2; mode++) check_mode(nodes, n, box, rays, g, count, mode, res);
    if (res.model[ptl::kSweepFamiliesOn] > res.model[ptl::kSweepFamiliesOff]) fail("the model's sum is above that of build_sweep_pairs' pairing", n);
    if (count <= 9) {
        std::vector<const float*> b;
        for (int k = 0; k < count; k++) b.push_back(box[ptl::sweep_lowest(ptl::sweep_group_mask(g[k]))].v);
        // leftovers were counted 17.5 each (x 2: 35): an odd count's single has no pointer, 17
        if ((int)(2u * res.model[ptl::kSweepFamiliesOn]) != brute_best(b, 0u) - (count & 1)) fail("not the smallest sum over every placement", n);
    }
    return res;
}

Result check_boxes(const std::vector<Box>& box, uint32_t seed, int trees, Result* worst = nullptr) {
    const int n = (int)box.size();
    const std::vector<Ray> rays = make_rays(box, 256, seed);
    std::mt19937 rng(seed);
    Result first;
    for (int t = 0; t < trees; t++) {
        const Result r = check_set(random_tree(n, box, rng), n, box, rays);
        if (t == 0) first = r;
        if (worst)
            for (int m = 0; m < 2; m++)
                if (t == 0 || r.model[m] > worst->model[m]) worst->model[m] = r.model[m];
    }
    return first;
}

Box mk(float x0, float y0, float z0, float x1, float y1, float z1) { return Box{{x0, y0, z0, x1, y1, z1}}; }
Box distinct(int k) { const float f = (float)k; return mk(-1.0f - 0.11f * f, -2.0f - 0.13f * f, -3.0f - 0.17f * f, 1.0f + 0.19f * f, 2.0f + 0.23f * f, 3.0f + 0.29f * f); }
// box k with the interval of axis a set to [lo, hi]
Box with(Box b, int a, float lo, float hi) { b.v[a] = lo; b.v[3 + a] = hi; return b; }

void fixed_sets() {
    const int A = ptl::kSweepFamiliesOn, O = ptl::kSweepFamiliesOff;
    {   // 2 primitives with one box: ONE group, the tail alone
        const Result r = check_boxes({distinct(0), distinct(0)}, 1, 1);
        if (r.count != 1 || r.cls[A].pairs.single != 1 || r.model[A] != 17) fail("one group");
    }
    {   // 2 groups: nothing shared / two axes shared
        const Result r = check_boxes({distinct(0), distinct(1)}, 2, 2);
        if (r.count != 2 || r.cls[A].pairs.general != 1 || r.model[A] != 35) fail("two groups");
        const Result s = check_boxes({distinct(0), with(distinct(0), 0, -7, 8)}, 3, 2);
        if (s.cls[A].fam.pair2[0][0] != 1 || s.model[A] != 27 || s.model[O] != 31) fail("two groups sharing y and z");
    }
    {   // 3, 4, 5 groups sharing x and y (flat): a PAIR2 and the single, two PAIR2, two and the single
        std::vector<Box> box;
        for (int k = 0; k < 5; k++) box.push_back(with(with(distinct(k), 0, -0.5f, 0.75f), 1, 0.25f, 0.25f));
        const Result r3 = check_boxes({box[0], box[1], box[2]}, 4, 3), r4 = check_boxes({box[0], box[1], box[2], box[3]}, 5, 3), r5 = check_boxes(box, 6, 3);
        if (r3.count != 3 || r3.cls[A].fam.pair2[2][2] != 1 || r3.cls[A].pairs.single != 1 || r3.model[A] != 25 + 17) fail("three groups");
        if (r4.count != 4 || r4.cls[A].fam.pair2[2][2] != 2 || r4.model[A] != 50 || r4.model[O] != 58) fail("four groups");
        if (r5.count != 5 || r5.cls[A].fam.pair2[2][2] != 2 || r5.cls[A].pairs.single != 1 || r5.model[A] != 67) fail("five groups");
    }
    {   // every PAIR2 class: u = x, y, z and each flatness of the two shared axes
        std::vector<Box> box;
        int k = 0;
        for (int u = 0; u < 3; u++)
            for (int fl = 0; fl < 4; fl++) {
                const int b = u == 0 ? 1 : 0, c = u == 2 ? 1 : 2;
                const float lo = 0.125f * (float)(4 * u + fl + 1);
                Box p = with(with(distinct(k), b, lo, (fl & 1) ? lo : lo + 0.5f), c, -lo, (fl & 2) ? -lo : -lo + 0.25f), q = p;
                q.v[u] -= 0.3f; q.v[3 + u] += 0.4f;
                box.push_back(p); box.push_back(q);
                k += 2;
            }
        const Result r = check_boxes(box, 8, 3);
        for (int u = 0; u < 3; u++)
            for (int fl = 0; fl < 4; fl++)
                if (r.cls[A].fam.pair2[u][fl] != 1) fail("every PAIR2 class", 4 * u + fl);
        if (r.count != 24 || r.model[A] != 3 * (27 + 25 + 25 + 23)) fail("every PAIR2 class: the sum");
    }
    {   // 32 groups: 16 planes z = const with two boxes of one x interval each -> 16 PAIR2_y (x, flat z), the hit word full
        std::vector<Box> box;
        for (int k = 0; k < 32; k++) box.push_back(with(with(distinct(k), 2, -0.5f * (float)(k / 2 + 1), -0.5f * (float)(k / 2 + 1)), 0, -1.0f - (float)(k / 2), 2.0f));
        const Result r = check_boxes(box, 10, 3);
        if (r.count != 32 || r.cls[A].fam.pair2[1][2] != 16 || r.model[A] != 16 * 25 || r.cls[O].pairs.flat[2] != 16) fail("32 groups in 16 PAIR2");
        // 32 groups that ALL share one interval: every pairing is as good as the greedy one, which stays
        std::vector<Box> all;
        for (int k = 0; k < 32; k++) all.push_back(with(distinct(k), 0, -1.0f, 2.0f));
        const Result s = check_boxes(all, 11, 2);
        if (s.count != 32 || s.cls[A].pairs.share[0] != 16 || s.model[A] != 16 * 31) fail("32 groups sharing one interval");
    }
    {   // 31 groups that share nothing: 15 general pairs and the tail, the plain order
        std::vector<Box> box;
        for (int k = 0; k < 31; k++) box.push_back(distinct(k));
        const Result r = check_boxes(box, 12, 3);
        if (r.count != 31 || r.cls[A].pairs.general != 15 || r.cls[A].pairs.single != 1 || r.model[A] != 15 * 35 + 17) fail("31 groups that share nothing");
        // 31 groups: 15 PAIR2_x (y, z) and the tail
        for (int k = 0; k < 31; k++) box[k] = with(with(box[k], 1, 0.5f * (float)(k / 2), 0.5f * (float)(k / 2) + 3.0f), 2, -0.25f * (float)(k / 2), 1.0f);
        const Result s = check_boxes(box, 13, 3);
        if (s.cls[A].fam.pair2[0][0] != 15 || s.cls[A].pairs.single != 1 || s.model[A] != 15 * 27 + 17) fail("31 groups: 15 PAIR2 and the tail");
    }
    {   // -0.0 and +0.0: two planes.  Same x interval, z = -0 against z = +0: SHARE_x and no PAIR2
        const Result r = check_boxes({mk(-2, -1, -0.0f, -0.5f, 1, -0.0f), mk(-2, -1.5f, 0.0f, -0.5f, 1.25f, 0.0f)}, 14, 2);
        if (ptl::sweep_pair2_records(r.cls[A].fam) || r.cls[A].pairs.share[0] != 1) fail("-0.0 and +0.0 shared as one plane in a PAIR2");
        const Result s = check_boxes({with(distinct(0), 1, -0.0f, 1.0f), with(distinct(1), 1, 0.0f, 1.0f)}, 16, 2);
        if (s.cls[A].pairs.general != 1) fail("[-0, 1] and [+0, 1] taken for one interval");
    }
    {   // boxes flat on two axes (segments along x on one line): PAIR2_x with both shared axes flat
        const Result r = check_boxes({mk(-0.6f, -1, -0.5f, 0.9f, -1, -0.5f), mk(0.2f, -1, -0.5f, 1.9f, -1, -0.5f), distinct(2)}, 17, 3);
        if (r.cls[A].fam.pair2[0][3] != 1 || r.cls[A].pairs.single != 1 || r.model[A] != 23 + 17 || r.cls[O].pairs.flat[1] != 1) fail("flat on two shared axes");
        // a segment in the plane of a floor panel: flat on two axes, one shared -> SHARE_FLAT_y as before
        const Result s = check_boxes({mk(-1.8f, -1, -1.9f, 1.6f, -1, 1.4f), mk(-0.6f, -1, -0.5f, 0.9f, -1, -0.5f), distinct(2)}, 18, 3);
        if (s.cls[A].pairs.flat[1] != 1 || ptl::sweep_pair2_records(s.cls[A].fam)) fail("flat on two axes, one shared");
    }
    {   // the pairing matters: a - b share y, b - c share y and z (flat), c - d share z.  Greedy takes the flat pair on z first; the best is PAIR2(b, c)
        Box a = distinct(0), b = distinct(1), c = distinct(2), d = distinct(3), e = distinct(4);
        a = with(a, 1, -1, 1); b = with(with(b, 1, -1, 1), 2, -2, -2); c = with(with(c, 1, -1, 1), 2, -2, -2); d = with(d, 2, -2, -2); e = with(e, 2, -2, -2);
        const Result r = check_boxes({a, b, c, d, e}, 19, 4);
        // best: PAIR2(b, c) 25 + SHARE_FLAT(d, e) 29 + a single 17 = 71
        if (r.model[A] != 71 || r.cls[A].fam.pair2[0][2] != 1 || r.cls[A].pairs.flat[2] != 1) fail("chain of five");
    }
}

void random_sets() {
    std::mt19937 rng(78);
    for (int rep = 0; rep < 60; rep++) {
        const int n = rep < 24 ? 2 + (int)(rng() % 8u) : 2 + (int)(rng() % 47u);
        // intervals drawn from a small pool per axis (some flat, +0 and -0 among the bounds), boxes drawn from those
        std::vector<Box> box(n);
        float pool[3][6][2];
        const int pool_size = rep % 3 == 0 ? 2 : 6;
        for (int a = 0; a < 3; a++)
            for (int k = 0; k < 6; k++) {
                const float lo = (float)((int)(rng() % 9u) - 4) * 0.5f * ((rng() & 1u) ? 1.0f : -1.0f);
                pool[a][k][0] = lo;
                pool[a][k][1] = (rng() % 3u) ? lo + 0.25f * (float)(1 + rng() % 5u) : lo;
            }
        for (int p = 0; p < n; p++)
            for (int a = 0; a < 3; a++) {
                if (rng() % 3u) {
                    const int k = (int)(rng() % (uint32_t)pool_size);
                    box[p].v[a] = pool[a][k][0]; box[p].v[3 + a] = pool[a][k][1];
                } else {
                    box[p].v[a] = -5.0f + 0.01f * (float)(rng() % 400u); box[p].v[3 + a] = 1.0f + 0.01f * (float)(rng() % 400u);
                }
            }
        check_boxes(box, 200u + (uint32_t)rep, 2);
    }
}

int scene_boxes(const char* path) {
    std::FILE* f = std::fopen(path, "rb");
    if (!f) { std::fprintf(stderr, "cannot open %s\n", path); return 2; }
    std::vector<Box> box;
    Box b;
    while (std::fread(b.v, sizeof(float), 6, f) == 6) box.push_back(b);
    std::fclose(f);
    const int n = (int)box.size();
    if (n < 2 || n > ptl::kSweepMaxPrims) { std::fprintf(stderr, "%d boxes\n", n); return 2; }
    Result worst;
    const Result r = check_boxes(box, 5, 8, &worst);
    const SweepClasses& c = r.cls[ptl::kSweepFamiliesOn];
    // the sums: the largest over the trees (the smallest sum does not depend on the order of the groups, so they agree)
    std::printf("groups %d model %u %u pair2", r.count, worst.model[ptl::kSweepFamiliesOn], worst.model[ptl::kSweepFamiliesOff]);
    for (int u = 0; u < 3; u++)
        for (int fl = 0; fl < 4; fl++) std::printf(" %d", c.fam.pair2[u][fl]);
    std::printf(" flat %d %d %d share %d %d %d general %d single %d\n", c.pairs.flat[0], c.pairs.flat[1], c.pairs.flat[2], c.pairs.share[0], c.pairs.share[1],
                c.pairs.share[2], c.pairs.general, c.pairs.single);
    return errors ? 1 : 0;
}

}  // namespace

int main(int argc, char** argv) {
    if (argc > 1) return scene_boxes(argv[1]);
    fixed_sets();
    random_sets();
    if (errors) {
        std::fprintf(stderr, "%llu checks failed\n", (unsigned long long)errors);
        return 1;
    }
    std::puts("sweep_families_check: ok");
    return 0;
}
