// The sweep kernel's record stream (csrc/pt_kernels.h: SweepWindow, csrc/pt_trace_sweep_body.h step (3)) as a CPU model over the
// tables csrc/pt_sweep_families.h and csrc/pt_sweep_pairs.h make: one window of four 8-byte pairs, read at the start of the
// lane's octant table and then by every body behind its own record, whatever comes next; a body takes its differences out of the
// window (and out of its tail, which it reads itself), THEN overwrites the window, then multiplies.  For every set of leaf boxes,
// under random trees, for the tables of option "sweep_families" on and off and for the plain table (every pair general):
//   - every body finds the window read at its own record, and window and tail hold exactly that record's bytes — the record is
//     made here from the permuted groups' boxes, not taken from the table;
//   - every read stays inside the region a block stages (sweep_layout_bytes; the model reads a buffer of exactly that size, so
//     ASan sees a byte too many), and the furthest byte read over the eight octants is sweep_stream_end's, which
//     sweep_stream_fits accepts;
//   - the hit word over 2048 rays (all 8 octants; origins inside, outside and exactly on planes of the boxes) is the plain
//     loop's over build_sweep_layout's tables with the permutation applied.
// Sets: 1 group (the single alone), 2 (one pair, no single), 3 (a pair and the single), 5, 31 and 32 groups; each of the 19 pair
// classes alone at trip count 1; every ordered pair of the 20 classes (the single among them) with one record each, so that each
// class's first record is fetched by each other class's last body; 60 random sets with planted intervals.
// `sweep_stream_check FILE [TREES]` checks the N x 6 floats of FILE (the leaf boxes of a scene) the same way under TREES random trees
// (8) and prints the classes of the first tree as tests/native/sweep_families_check.cpp does.
// Stand-alone; built with -fsanitize=address,undefined by tests/test_sweep_stream_host.py.  Exit code 0 = all held.
#include <algorithm>
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

void shift_in(uint32_t& h, float tf, float tn0) { h = h + h + (tf >= tn0 ? 1u : 0u); }
void shift_in(uint32_t& h, const float* n, const float* f) {
    shift_in(h, std::fmin(std::fmin(f[0], f[1]), f[2]), std::fmax(0.0f, std::fmax(std::fmax(n[0], n[1]), n[2])));
}
float slab(float plane, const Ray& r, int a) { return (plane - r.o[a]) * r.inv[a]; }

// The plain loop over build_sweep_layout's tables, group by group, no window.
uint32_t sweep_plain(const unsigned char* tab, uint32_t pitch, int count, const Ray& r) {
    uint32_t h = 0;
    const float* p = reinterpret_cast<const float*>(tab + r.oct * pitch);
    for (int k = 0; k < count; k++, p += 6) {
        const float n[3] = {slab(p[0], r, 0), slab(p[1], r, 1), slab(p[2], r, 2)}, f[3] = {slab(p[3], r, 0), slab(p[4], r, 1), slab(p[5], r, 2)};
        shift_in(h, n, f);
    }
    return ptl::sweep_hits_align(h, (uint32_t)count);
}

// ---- the stream -------------------------------------------------------------------------------------------------------------
// The staged region and what the stream has read of it.  Offsets are bytes from the start of the region, as the kernel's are
// from the start of the node region in LDS.
struct Stream {
    const std::vector<unsigned char>* region;
    uint32_t bx = 0;               // the record the next body works on
    float win[8];                  // the window
    uint32_t win_at = ~0u;         // where it was read
    uint32_t end = 0;              // one past the furthest byte read
    bool ok = true;

    void read(float* dst, uint32_t at, uint32_t bytes) {
        if ((size_t)at + bytes > region->size()) { ok = false; std::memset(dst, 0, bytes); return; }
        std::memcpy(dst, region->data() + at, bytes);          // a buffer of exactly the staged size: ASan is the second check
        end = std::max(end, at + bytes);
    }
    void read_window(uint32_t at) { read(win, at, ptl::kSweepWindowBytes); win_at = at; }
};

// What a body must have received: `want` (the record made from the boxes) against window and tail.
void check_record(Stream& s, const float* tail, const float* want, uint32_t floats, int n) {
    const uint32_t in_window = std::min(floats, 8u);
    if (s.win_at != s.bx) fail("a body whose window was not read at its record", n);
    if (std::memcmp(s.win, want, 4u * in_window) != 0) fail("the window does not hold the record's first pairs", n);
    if (floats > 8u && std::memcmp(tail, want + 8, 4u * (floats - 8u)) != 0) fail("the tail does not hold the record's last pairs", n);
}

// near / far planes of a box for an octant: bit a set <=> 1/d[a] < 0, the near plane is the box's max
void planes(const float* box, uint32_t oct, float* nf) {
    for (int a = 0; a < 3; a++) {
        const bool neg = (oct >> a) & 1u;
        nf[a] = box[neg ? 3 + a : a];
        nf[3 + a] = box[neg ? a : 3 + a];
    }
}

// The sweep of one ray through the stream: the bodies of pt_kernels.h (sweep_pair2, sweep_shared_pairs) and of step (3) (the
// general pair, the single) in the kernel's order — differences, the window's read, products.  boxes[k]: permuted group k.
uint32_t sweep_stream(Stream& s, uint32_t pitch, const SweepClasses& cls, int count, const std::vector<const float*>& boxes, const Ray& r, int n) {
    uint32_t h = 0;
    int g = 0;
    s.bx = r.oct * pitch;
    s.read_window(s.bx);                                   // in front of the reciprocals
    float A[6], B[6], want[12], d[12], tail[4];
    for (int u = 0; u < 3; u++)
        for (int fl = 0; fl < 4; fl++) {
            const int b = u == 0 ? 1 : 0, c = u == 2 ? 1 : 2;
            const bool fb = fl & 1, fc = fl & 2;
            for (int k = cls.fam.pair2[u][fl]; k != 0; k--, g += 2) {
                planes(boxes[g], r.oct, A); planes(boxes[g + 1], r.oct, B);
                const float rec[8] = {A[b], fb ? 0.0f : A[3 + b], A[c], fc ? 0.0f : A[3 + c], A[u], A[3 + u], B[u], B[3 + u]};
                check_record(s, nullptr, rec, 8, n);
                const int axis[8] = {b, b, c, c, u, u, u, u};
                for (int i = 0; i < 8; i++) d[i] = s.win[i] - r.o[axis[i]];
                s.read_window(s.bx + 32u);
                s.bx += 32u;
                float na[3], fa[3], nb[3], fbb[3];
                na[b] = d[0] * r.inv[b]; fa[b] = fb ? na[b] : d[1] * r.inv[b];
                na[c] = d[2] * r.inv[c]; fa[c] = fc ? na[c] : d[3] * r.inv[c];
                nb[b] = na[b]; fbb[b] = fa[b]; nb[c] = na[c]; fbb[c] = fa[c];
                na[u] = d[4] * r.inv[u]; fa[u] = d[5] * r.inv[u]; nb[u] = d[6] * r.inv[u]; fbb[u] = d[7] * r.inv[u];
                shift_in(h, na, fa);
                shift_in(h, nb, fbb);
            }
        }
    for (int c6 = 0; c6 < 6; c6++) {
        const int ax = c6 % 3, b = ax == 0 ? 1 : 0, c = ax == 2 ? 1 : 2;
        const bool flat = c6 < 3;
        for (int k = flat ? cls.pairs.flat[ax] : cls.pairs.share[ax]; k != 0; k--, g += 2) {
            planes(boxes[g], r.oct, A); planes(boxes[g + 1], r.oct, B);
            const float rec[10] = {A[ax], flat ? 0.0f : A[3 + ax], A[b], A[c], A[3 + b], A[3 + c], B[b], B[c], B[3 + b], B[3 + c]};
            s.read(tail, s.bx + 32u, 8u);                  // the tail, at entry
            check_record(s, tail, rec, 10, n);
            const int axis[10] = {ax, ax, b, c, b, c, b, c, b, c};
            for (int i = 0; i < 8; i++) d[i] = s.win[i] - r.o[axis[i]];
            for (int i = 8; i < 10; i++) d[i] = tail[i - 8] - r.o[axis[i]];
            s.read_window(s.bx + 40u);
            s.bx += 40u;
            float na[3], fa[3], nb[3], fb[3];
            na[ax] = d[0] * r.inv[ax]; fa[ax] = flat ? na[ax] : d[1] * r.inv[ax];
            nb[ax] = na[ax]; fb[ax] = fa[ax];
            na[b] = d[2] * r.inv[b]; na[c] = d[3] * r.inv[c]; fa[b] = d[4] * r.inv[b]; fa[c] = d[5] * r.inv[c];
            nb[b] = d[6] * r.inv[b]; nb[c] = d[7] * r.inv[c]; fb[b] = d[8] * r.inv[b]; fb[c] = d[9] * r.inv[c];
            shift_in(h, na, fa);
            shift_in(h, nb, fb);
        }
    }
    for (int k = cls.pairs.general; k != 0; k--, g += 2) {
        planes(boxes[g], r.oct, want); planes(boxes[g + 1], r.oct, want + 6);
        s.read(tail, s.bx + 32u, 16u);
        check_record(s, tail, want, 12, n);
        for (int i = 0; i < 8; i++) d[i] = s.win[i] - r.o[i % 3];
        for (int i = 8; i < 12; i++) d[i] = tail[i - 8] - r.o[i % 3];
        s.read_window(s.bx + 48u);
        s.bx += 48u;
        float p[12];
        for (int i = 0; i < 12; i++) p[i] = d[i] * r.inv[i % 3];
        shift_in(h, p, p + 3);
        shift_in(h, p + 6, p + 9);
    }
    if (cls.pairs.single) {                                // three pairs of the window, nothing read
        planes(boxes[g], r.oct, want);
        check_record(s, nullptr, want, 6, n);
        float p[6];
        for (int i = 0; i < 6; i++) p[i] = (s.win[i] - r.o[i % 3]) * r.inv[i % 3];
        shift_in(h, p, p + 3);
        g++;
    }
    if (g != count) fail("the classes do not add up to the groups", n);
    return ptl::sweep_hits_align(h, (uint32_t)count);
}

// Rays in every octant (tests/native/sweep_families_check.cpp has the same ones).
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

struct Result { int count = 0; SweepClasses cls[2] = {}; };

// One table (region: the whole staged layout) under its classes: the stream of every ray, the bound, the hit words.
void check_table(const std::vector<unsigned char>& region, const SweepClasses& cls, int count, int n, const std::vector<const float*>& boxes,
                 const int* perm, const std::vector<unsigned char>& plain, const std::vector<Ray>& rays) {
    const uint32_t pitch = ptl::sweep_classes_pitch(cls), plain_pitch = ptl::sweep_box_pitch((uint32_t)count);
    if (!ptl::sweep_stream_fits(cls, (uint32_t)count, (uint32_t)n)) fail("sweep_stream_fits refuses a table the layout holds", n);
    if (ptl::sweep_stream_end(cls) > region.size()) { fail("sweep_stream_end lies behind the staged region", n); return; }
    uint32_t end = 0, octants = 0;
    for (const Ray& r : rays) {
        Stream s;
        s.region = &region;
        const uint32_t hs = sweep_stream(s, pitch, cls, count, boxes, r, n), hp = sweep_plain(plain.data(), plain_pitch, count, r);
        if (!s.ok) { fail("the stream read outside the staged region", n); return; }
        end = std::max(end, s.end);
        octants |= 1u << r.oct;
        uint32_t want = 0;
        for (int k = 0; k < count; k++)
            if (hp & (0x80000000u >> perm[k])) want |= 0x80000000u >> k;
        if (hs != want) { fail("hit word of the stream is not the plain loop's with the permutation applied", n); return; }
    }
    if (octants != 0xffu) fail("rays do not cover the eight octants", n);
    if (end != ptl::sweep_stream_end(cls)) fail("the furthest byte read is not sweep_stream_end's", n);
}

Result check_set(const std::vector<DNode>& nodes, int n, const std::vector<Box>& box, const std::vector<Ray>& rays) {
    Result res;
    const uint32_t stride = 64u;
    SweepGroup g[ptl::kSweepMaxPrims];
    const int num_nodes = (int)nodes.size();
    const int count = ptl::build_sweep_groups(nodes.data(), num_nodes, n, stride, g);
    res.count = count;
    if (count < 1) { fail("no groups", n); return res; }
    if (count > ptl::kSweepMaxBoxes) return res;
    const std::vector<DPrim> prims = make_prims(n);
    const uint32_t bytes = ptl::sweep_layout_bytes((uint32_t)count, (uint32_t)n);
    std::vector<unsigned char> plain(bytes);
    if (!ptl::build_sweep_layout(g, count, nodes.data(), num_nodes, stride, prims.data(), n, plain.data())) { fail("layout refused", n); return res; }
    auto gbox = [&](const SweepGroup& grp) { return box[ptl::sweep_lowest(ptl::sweep_group_mask(grp))].v; };
    {   // the plain table: every pair general, the groups in their own order
        std::vector<const float*> boxes;
        int ident[ptl::kSweepMaxBoxes];
        for (int k = 0; k < count; k++) { boxes.push_back(gbox(g[k])); ident[k] = k; }
        check_table(plain, ptl::sweep_classes_of_pairs(ptl::sweep_pairs_none((uint32_t)count)), count, n, boxes, ident, plain, rays);
    }
    for (int mode = 0; mode < 2; mode++) {
        SweepGroup out[ptl::kSweepMaxBoxes];
        int perm[ptl::kSweepMaxBoxes];
        SweepClasses cls{};
        std::vector<unsigned char> placed(bytes);
        if (!ptl::build_sweep_families(g, count, nodes.data(), num_nodes, stride, mode, out, perm, &cls) ||
            !ptl::build_sweep_layout(out, count, nodes.data(), num_nodes, stride, prims.data(), n, placed.data()) ||
            !ptl::build_sweep_family_tables(out, count, cls, nodes.data(), num_nodes, stride, placed.data())) { fail("tables refused", n); return res; }
        res.cls[mode] = cls;
        std::vector<const float*> boxes;
        for (int k = 0; k < count; k++) boxes.push_back(gbox(out[k]));
        check_table(placed, cls, count, n, boxes, perm, plain, rays);
    }
    return res;
}

Result check_boxes(const std::vector<Box>& box, uint32_t seed, int trees) {
    const int n = (int)box.size();
    const std::vector<Ray> rays = make_rays(box, 256, seed);
    std::mt19937 rng(seed);
    Result first;
    for (int t = 0; t < trees; t++) {
        const Result r = check_set(random_tree(n, box, rng), n, box, rays);
        if (t == 0) first = r;
    }
    return first;
}

Box mk(float x0, float y0, float z0, float x1, float y1, float z1) { return Box{{x0, y0, z0, x1, y1, z1}}; }
Box distinct(int k) { const float f = (float)k; return mk(-1.0f - 0.11f * f, -2.0f - 0.13f * f, -3.0f - 0.17f * f, 1.0f + 0.19f * f, 2.0f + 0.23f * f, 3.0f + 0.29f * f); }
Box with(Box b, int a, float lo, float hi) { b.v[a] = lo; b.v[3 + a] = hi; return b; }

// The 20 classes in table order: 0 .. 11 PAIR2 (4 u + fb + 2 fc), 12 .. 14 SHARE_FLAT_x y z, 15 .. 17 SHARE_x y z, 18 general, 19 single.
constexpr int kClasses = 20, kGeneral = 18, kSingle = 19;
// One record of class c from boxes k, k + 1 (the single: k alone) with a bound of its own, so that two records share nothing.
void add_record(std::vector<Box>& box, int c, int k) {
    const float lo = 0.125f * (float)(k + 1);
    if (c < 12) {
        const int u = c / 4, fl = c % 4, b = u == 0 ? 1 : 0, cc = u == 2 ? 1 : 2;
        Box p = with(with(distinct(k), b, lo, (fl & 1) ? lo : lo + 0.5f), cc, -lo, (fl & 2) ? -lo : -lo + 0.25f), q = p;
        q.v[u] -= 0.3f; q.v[3 + u] += 0.4f;
        box.push_back(p); box.push_back(q);
    } else if (c < kGeneral) {
        const int ax = c % 3;
        const float hi = c < 15 ? lo : lo + 0.5f;
        box.push_back(with(distinct(k), ax, lo, hi)); box.push_back(with(distinct(k + 1), ax, lo, hi));
    } else {
        box.push_back(distinct(k));
        if (c == kGeneral) box.push_back(distinct(k + 1));
    }
}
uint32_t class_count(const SweepClasses& cls, int c) {
    return c < 12 ? cls.fam.pair2[c / 4][c % 4] : c < 15 ? cls.pairs.flat[c - 12] : c < kGeneral ? cls.pairs.share[c - 15] : c == kGeneral ? cls.pairs.general : cls.pairs.single;
}
// the classes of `r` (families on) are one record each of the listed classes and nothing else
bool classes_are(const Result& r, std::initializer_list<int> want) {
    for (int c = 0; c < kClasses; c++) {
        uint32_t n = 0;
        for (int w : want) n += w == c;
        if (class_count(r.cls[ptl::kSweepFamiliesOn], c) != n) return false;
    }
    return true;
}

void fixed_sets() {
    const int A = ptl::kSweepFamiliesOn;
    {   // 1 group (2 primitives with one box): the single alone, the stream's first read is its only one
        const Result r = check_boxes({distinct(0), distinct(0)}, 1, 1);
        if (r.count != 1 || !classes_are(r, {kSingle})) fail("one group");
    }
    {   // 2 groups: one pair, no single: the body that starts the stream ends it and reads past the table
        const Result r = check_boxes({distinct(0), distinct(1)}, 2, 2);
        if (r.count != 2 || !classes_are(r, {kGeneral})) fail("two groups");
    }
    {   // 3 groups: a pair and the single
        const Result r = check_boxes({distinct(0), distinct(1), distinct(2)}, 3, 2);
        if (r.count != 3 || !classes_are(r, {kGeneral, kSingle})) fail("three groups");
    }
    {   // 5 groups sharing x and y (flat): two PAIR2 and the single
        std::vector<Box> box;
        for (int k = 0; k < 5; k++) box.push_back(with(with(distinct(k), 0, -0.5f, 0.75f), 1, 0.25f, 0.25f));
        const Result r = check_boxes(box, 6, 3);
        if (r.count != 5 || r.cls[A].fam.pair2[2][2] != 2 || r.cls[A].pairs.single != 1) fail("five groups");
    }
    {   // 31 groups that share nothing (15 general pairs and the single); 31 as 15 PAIR2_x and the single
        std::vector<Box> box;
        for (int k = 0; k < 31; k++) box.push_back(distinct(k));
        const Result r = check_boxes(box, 12, 2);
        if (r.count != 31 || r.cls[A].pairs.general != 15 || r.cls[A].pairs.single != 1) fail("31 groups that share nothing");
        for (int k = 0; k < 31; k++) box[k] = with(with(box[k], 1, 0.5f * (float)(k / 2), 0.5f * (float)(k / 2) + 3.0f), 2, -0.25f * (float)(k / 2), 1.0f);
        const Result s = check_boxes(box, 13, 2);
        if (s.cls[A].fam.pair2[0][0] != 15 || s.cls[A].pairs.single != 1) fail("31 groups: 15 PAIR2 and the single");
    }
    {   // 32 groups: 16 PAIR2_y (x, flat z); 32 that share nothing: 16 general pairs, the longest table, the furthest read
        std::vector<Box> box;
        for (int k = 0; k < 32; k++) box.push_back(with(with(distinct(k), 2, -0.5f * (float)(k / 2 + 1), -0.5f * (float)(k / 2 + 1)), 0, -1.0f - (float)(k / 2), 2.0f));
        const Result r = check_boxes(box, 10, 2);
        if (r.count != 32 || r.cls[A].fam.pair2[1][2] != 16) fail("32 groups in 16 PAIR2");
        for (int k = 0; k < 32; k++) box[k] = distinct(k);
        const Result s = check_boxes(box, 11, 2);
        if (s.count != 32 || s.cls[A].pairs.general != 16) fail("32 groups that share nothing");
    }
    // each pair class alone at trip count 1 (the single alone: one group, above)
    for (int c = 0; c < kSingle; c++) {
        std::vector<Box> box;
        add_record(box, c, 0);
        const Result r = check_boxes(box, 20u + (uint32_t)c, 2);
        if (r.count != 2 || !classes_are(r, {c})) fail("a class alone at trip count 1", c);
    }
    // every ordered pair of classes, one record each: a's body fetches b's record.  With b the single this is "every class empty
    // but the single's neighbour".
    for (int a = 0; a < kSingle; a++)
        for (int b = a + 1; b < kClasses; b++) {
            std::vector<Box> box;
            add_record(box, a, 0);
            add_record(box, b, 2);
            const Result r = check_boxes(box, 100u + (uint32_t)(kClasses * a + b), 2);
            if (!classes_are(r, {a, b})) fail("a transition between two classes", kClasses * a + b);
        }
}

void random_sets() {
    std::mt19937 rng(79);
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
        check_boxes(box, 300u + (uint32_t)rep, 2);
    }
}

int scene_boxes(const char* path, int trees) {
    std::FILE* f = std::fopen(path, "rb");
    if (!f) { std::fprintf(stderr, "cannot open %s\n", path); return 2; }
    std::vector<Box> box;
    Box b;
    while (std::fread(b.v, sizeof(float), 6, f) == 6) box.push_back(b);
    std::fclose(f);
    const int n = (int)box.size();
    if (n < 2 || n > ptl::kSweepMaxPrims) { std::fprintf(stderr, "%d boxes\n", n); return 2; }
    const Result r = check_boxes(box, 5, trees);
    const SweepClasses& c = r.cls[ptl::kSweepFamiliesOn];
    std::printf("groups %d model %u stream_end %u staged %u pair2", r.count, ptl::sweep_valu_model(c), ptl::sweep_stream_end(c),
                ptl::sweep_layout_bytes((uint32_t)r.count, (uint32_t)n));
    for (int u = 0; u < 3; u++)
        for (int fl = 0; fl < 4; fl++) std::printf(" %d", c.fam.pair2[u][fl]);
    std::printf(" flat %d %d %d share %d %d %d general %d single %d\n", c.pairs.flat[0], c.pairs.flat[1], c.pairs.flat[2], c.pairs.share[0], c.pairs.share[1],
                c.pairs.share[2], c.pairs.general, c.pairs.single);
    return errors ? 1 : 0;
}

}  // namespace

int main(int argc, char** argv) {
    if (argc > 1) return scene_boxes(argv[1], argc > 2 ? std::max(1, std::atoi(argv[2])) : 8);
    fixed_sets();
    random_sets();
    if (errors) {
        std::fprintf(stderr, "%llu checks failed\n", (unsigned long long)errors);
        return 1;
    }
    std::puts("sweep_stream_check: ok");
    return 0;
}
