// The tables a sweep launch stages (csrc/pt_sweep_layout.h): box tables per octant and chained slot records.  Checks:
//   - random trees over 2 .. 64 primitives whose leaf boxes are drawn from a small pool (planted equal boxes, groups of every
//     size): every primitive sits in exactly one chain, the chain from slot k visits exactly the primitives of group k's mask
//     (in ascending order), slot 0 is never a successor, and a record carries its primitive's own DPrim words;
//   - the box table of octant o holds, for every group, the near and far selection of that group's box, bit for bit, and the
//     8 tables start at 8 different 8-byte positions of LDS's 64 banks;
//   - a hit word, accumulated the way the kernel does (hits = 2 * hits + hit, then aligned), turned into tested primitives by
//     taking the first set group and walking its chain, gives the OR of the hit groups' masks, groups in table order: for at
//     most 16 groups every hit word, for 17 .. 32 groups a fixed set of random words plus all-zero, all-one and each single bit;
//   - fixed shapes: four equal boxes (a chain of four), 32 groups of one, 64 primitives in 32 pairs, one group of two, two
//     primitives in two groups; more than 32 groups are refused;
//   - the fit predicate: every binary tree over 2 .. 64 primitives leaves the room, for every group count, and the predicate
//     turns exactly at the node region's size;
//   - the staged record: p0 kept, e1 = p1 - p0, e2 = p2 - p0, the other three words untouched.
// Stand-alone; built with -fsanitize=address,undefined by tests/test_sweep_layout_host.py.  Exit code 0 = all held.
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <random>
#include <vector>

#include "pt_sweep_layout.h"

namespace {

using ptl::DNode;
using ptl::DPrim;
using ptl::SweepGroup;

uint64_t errors = 0;
void fail(const char* what, int n = -1) {
    if (errors++ < 10) std::fprintf(stderr, "FAIL: %s (n = %d)\n", what, n);
}

struct Box { float v[6]; };

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
        p[k].light = k % 3 == 0 ? k : -1;
        p[k].pad = 0x5a5a5a5a;                      // the layout overwrites it
    }
    return p;
}

// The primitives a lane tests for the hit word it holds after the sweep, in the order it tests them (the kernel's burst).
std::vector<int> walk(uint32_t hits, const DPrim* slots, int n, bool& ok) {
    std::vector<int> order;
    uint32_t pend = 0;
    int steps = 0;
    while ((hits | pend) != 0u) {
        uint32_t slot = pend;
        if (pend == 0u) {
            slot = ptl::sweep_first_group(hits);
            hits = ptl::sweep_clear_group(hits, slot);
        }
        if (slot >= (uint32_t)n || ++steps > n) { ok = false; return order; }
        const uint32_t link = (uint32_t)slots[slot].pad;
        order.push_back((int)ptl::sweep_link_prim(link));
        pend = ptl::sweep_link_next(link);
    }
    return order;
}

void check_hit_word(uint32_t word, int count, const SweepGroup* g, const DPrim* slots, int n) {
    // the kernel's accumulation: group 0 first, one bit shifted in per group
    uint32_t h = 0;
    uint64_t want = 0;
    std::vector<int> want_order;
    for (int k = 0; k < count; k++) {
        const uint32_t hit = (word >> k) & 1u;
        h = 2u * h + hit;
        if (hit) {
            uint64_t m = ptl::sweep_group_mask(g[k]);
            want |= m;
            while (m) { want_order.push_back(ptl::sweep_lowest(m)); m = ptl::sweep_clear_lowest(m); }
        }
    }
    bool ok = true;
    const std::vector<int> got = walk(ptl::sweep_hits_align(h, (uint32_t)count), slots, n, ok);
    if (!ok) { fail("walk leaves the table or does not end", n); return; }
    uint64_t tested = 0;
    for (int p : got) {
        if (p < 0 || p >= n || ((tested >> p) & 1ull)) { fail("a primitive tested twice or out of range", n); return; }
        tested |= 1ull << p;
    }
    if (tested != want) fail("hit word: tested primitives are not the OR of the hit groups' masks", n);
    if (got != want_order) fail("hit word: not in group order", n);
}

// Builds groups and layout over `nodes` and checks everything; want_groups < 0: any.  Returns the group count.
int check_layout(const std::vector<DNode>& nodes, int n, const std::vector<Box>& box, int want_groups) {
    SweepGroup g[ptl::kSweepMaxPrims];
    const uint32_t stride = 64u;
    const int count = ptl::build_sweep_groups(nodes.data(), (int)nodes.size(), n, stride, g);
    if (count < 1) { fail("no groups", n); return count; }
    if (want_groups >= 0 && count != want_groups) fail("group count", n);
    const std::vector<DPrim> prims = make_prims(n);
    if (count > ptl::kSweepMaxBoxes) {
        std::vector<unsigned char> none(64);
        if (ptl::build_sweep_layout(g, count, nodes.data(), (int)nodes.size(), stride, prims.data(), n, none.data()))
            fail("more groups than hit bits accepted", n);
        return count;
    }
    const uint32_t bytes = ptl::sweep_layout_bytes((uint32_t)count, (uint32_t)n);
    std::vector<unsigned char> tab(bytes);            // exactly as large as the layout says: ASan sees a byte too many
    if (!ptl::build_sweep_layout(g, count, nodes.data(), (int)nodes.size(), stride, prims.data(), n, tab.data())) {
        fail("layout refused", n);
        return count;
    }
    if (!ptl::sweep_layout_fits((uint32_t)count, (uint32_t)n, (uint32_t)nodes.size(), stride)) fail("a binary tree's node region is too small", n);
    // box tables
    const uint32_t pitch = ptl::sweep_box_pitch((uint32_t)count);
    if (pitch < (uint32_t)count * 24u || pitch % 8u || !((pitch / 8u) & 1u)) fail("pitch is not an odd number of 8-byte units", n);
    uint32_t positions = 0;
    for (uint32_t o = 0; o < 8; o++) positions |= 1u << ((o * pitch / 8u) % 32u);
    if (__builtin_popcount(positions) != 8) fail("two box tables start at the same bank position", n);
    for (int k = 0; k < count; k++) {
        const uint64_t m = ptl::sweep_group_mask(g[k]);
        const float* b = box[ptl::sweep_lowest(m)].v;
        for (uint32_t o = 0; o < 8; o++) {
            float want[6];
            for (int a = 0; a < 3; a++) {
                const bool neg = (o >> a) & 1u;
                want[a] = neg ? b[3 + a] : b[a];
                want[3 + a] = neg ? b[a] : b[3 + a];
            }
            if (std::memcmp(tab.data() + o * pitch + (uint32_t)k * 24u, want, 24) != 0) fail("box table: not the near / far selection of the group's box", n);
        }
    }
    // slot records and chains
    if (ptl::sweep_slots_off((uint32_t)count) != 8u * pitch || ptl::sweep_slots_off((uint32_t)count) % 16u) fail("slot records are not 16-byte aligned behind the tables", n);
    std::vector<DPrim> slots(n);
    std::memcpy(slots.data(), tab.data() + ptl::sweep_slots_off((uint32_t)count), (size_t)n * sizeof(DPrim));
    uint64_t seen = 0;
    std::vector<int> slot_used(n, 0);
    for (int k = 0; k < count; k++) {
        uint64_t chain = 0;
        int slot = k, last = -1, steps = 0;
        for (;;) {
            if (slot < 0 || slot >= n || slot_used[slot]++) { fail("a slot in two chains or out of range", n); break; }
            const uint32_t link = (uint32_t)slots[slot].pad;
            const int prim = (int)ptl::sweep_link_prim(link);
            if (prim >= n || prim <= last) { fail("chain: primitive out of range or not ascending", n); break; }
            last = prim;
            if ((seen | chain) >> prim & 1ull) fail("a primitive in two chains", n);
            chain |= 1ull << prim;
            DPrim want = prims[prim];
            want.pad = (int32_t)link;
            if (std::memcmp(&slots[slot], &want, sizeof(DPrim)) != 0) fail("record: not the primitive's words", n);
            const int next = (int)ptl::sweep_link_next(link);
            if (next == 0) break;
            if (next < count) fail("a group's first slot as a successor", n);
            slot = next;
            if (++steps > n) { fail("chain does not end", n); break; }
        }
        if (chain != ptl::sweep_group_mask(g[k])) fail("chain is not the group's mask", n);
        seen |= chain;
    }
    if (seen != (n == 64 ? ~0ull : (1ull << n) - 1ull)) fail("a primitive in no chain", n);
    for (int s = 0; s < n; s++)
        if (slot_used[s] != 1) fail("a slot in no chain", n);
    // hit words
    std::mt19937 rng(1000u + (uint32_t)n * 64u + (uint32_t)count);
    if (count <= 16) {
        for (uint32_t w = 0; w < (1u << count); w++) check_hit_word(w, count, g, slots.data(), n);
    } else {
        const uint32_t all = count == 32 ? ~0u : (1u << count) - 1u;
        check_hit_word(0u, count, g, slots.data(), n);
        check_hit_word(all, count, g, slots.data(), n);
        for (int k = 0; k < count; k++) check_hit_word(1u << k, count, g, slots.data(), n);
        for (int r = 0; r < 64; r++) check_hit_word((uint32_t)rng() & all, count, g, slots.data(), n);
    }
    return count;
}

void random_layouts() {
    std::mt19937 rng(12);
    bool saw[4] = {false, false, false, false};      // a group of 4 or more, 32 groups, an odd count, a count above 16
    for (int n = 2; n <= 64; n++) {
        for (int rep = 0; rep < 6; rep++) {
            const int pool = 1 + (int)(rng() % (uint32_t)std::min(n, 32));
            std::vector<Box> boxes(pool), box(n);
            for (int k = 0; k < pool; k++)
                for (int c = 0; c < 6; c++) boxes[k].v[c] = (c < 3 ? -1.0f : 1.0f) * ((float)k + 0.125f * (float)(c + 1));
            for (int p = 0; p < n; p++) box[p] = boxes[rng() % (uint32_t)pool];
            const int count = check_layout(random_tree(n, box, rng), n, box, -1);
            if (count >= 1 && count <= 32) {
                saw[1] = saw[1] || count == 32;
                saw[2] = saw[2] || (count & 1);
                saw[3] = saw[3] || count > 16;
                saw[0] = saw[0] || n >= 4 * count;
            }
        }
    }
    if (!saw[0] || !saw[2] || !saw[3]) fail("random layouts: a shape never drawn");
}

void fixed_shapes() {
    std::mt19937 rng(5);
    auto distinct = [](int k) { Box b; for (int c = 0; c < 6; c++) b.v[c] = (c < 3 ? -1.0f : 1.0f) * (float)(k + 1) + 0.25f * (float)c; return b; };
    {   // four triangles with one common box: one group, a chain of four
        std::vector<Box> box(4, distinct(0));
        check_layout(random_tree(4, box, rng), 4, box, 1);
    }
    {   // one group of two, two primitives in two groups
        std::vector<Box> same(2, distinct(3)), two{distinct(1), distinct(2)};
        check_layout(random_tree(2, same, rng), 2, same, 1);
        check_layout(random_tree(2, two, rng), 2, two, 2);
    }
    for (int n : {31, 32}) {   // n groups of one: odd and even counts at the top of the range
        std::vector<Box> box(n);
        for (int p = 0; p < n; p++) box[p] = distinct(p);
        check_layout(random_tree(n, box, rng), n, box, n);
    }
    {   // 64 primitives in 32 pairs, the pairs scattered over the tree
        std::vector<Box> box(64);
        for (int p = 0; p < 64; p++) box[p] = distinct(p % 32);
        check_layout(random_tree(64, box, rng), 64, box, 32);
    }
    {   // 33 groups: a group table, but no layout
        std::vector<Box> box(40);
        for (int p = 0; p < 40; p++) box[p] = distinct(p % 33);
        check_layout(random_tree(40, box, rng), 40, box, 33);
    }
    {   // +0 and -0 are different boxes, and the table holds the bits
        std::vector<Box> z(2);
        std::memset(z.data(), 0, 2 * sizeof(Box));
        z[1].v[0] = -0.0f;
        check_layout(random_tree(2, z, rng), 2, z, 2);
    }
}

void fit_predicate() {
    using ptl::sweep_layout_fits;
    using ptl::sweep_layout_bytes;
    for (uint32_t n = 2; n <= 64; n++)
        for (uint32_t g = 1; g <= std::min<uint32_t>(n, 32u); g++) {
            if (!sweep_layout_fits(g, n, n - 1, 64u)) fail("a binary tree's node region is too small", (int)n);
            if (n >= 3 && sweep_layout_bytes(g, n) > 240u * n + 128u) fail("layout above 240 N + 128 bytes", (int)n);
            if (sweep_layout_bytes(g, n) != 8u * ptl::sweep_box_pitch(g) + 48u * n) fail("layout size", (int)n);
        }
    // the bound itself: a node region of R bytes admits a layout of exactly R bytes and not one of R + 48.
    // 6 nodes of 64 B: 8 * (384 + 16) = 3200 B.  16 groups: 8 * 392 = 3136 B of boxes; one more record fills it to 3184, two overflow.
    static_assert(8u * (6u * 64u + 16u) == 3200u, "node region of 6 nodes");
    if (ptl::sweep_slots_off(16u) != 3136u) fail("16 groups: 3136 bytes of box tables");
    if (!sweep_layout_fits(16u, 1u, 6u, 64u)) fail("3184 bytes into 3200");
    if (sweep_layout_fits(16u, 2u, 6u, 64u)) fail("3232 bytes into 3200");
    // 7 groups: 8 * 168 = 1344 B of boxes; 2 nodes: 8 * (128 + 16) = 1152 B; 3 nodes: 8 * 208 = 1664 B = 1344 + 320: 6 records fit, 7 do not
    if (sweep_layout_fits(7u, 1u, 2u, 64u)) fail("1392 bytes into 1152");
    if (!sweep_layout_fits(7u, 6u, 3u, 64u)) fail("1632 bytes into 1664");
    if (sweep_layout_fits(7u, 7u, 3u, 64u)) fail("1680 bytes into 1664");
}

void staged_record() {
    const std::vector<DPrim> prims = make_prims(5);
    for (const DPrim& g : prims) {
        const DPrim r = ptl::sweep_stage_record(g);
        for (int a = 0; a < 3; a++) {
            const float e1 = g.v[3 + a] - g.v[a], e2 = g.v[6 + a] - g.v[a];
            if (std::memcmp(&r.v[a], &g.v[a], 4) || std::memcmp(&r.v[3 + a], &e1, 4) || std::memcmp(&r.v[6 + a], &e2, 4)) fail("staged record: p0, e1, e2");
        }
        if (r.info != g.info || r.light != g.light || r.pad != g.pad) fail("staged record: info, light, link");
    }
}

void hit_word_helpers() {
    for (uint32_t groups = 1; groups <= 32; groups++)
        for (uint32_t k = 0; k < groups; k++) {
            uint32_t h = 0;
            for (uint32_t j = 0; j < groups; j++) h = 2u * h + (j == k ? 1u : 0u);
            const uint32_t a = ptl::sweep_hits_align(h, groups);
            if (a != 0x80000000u >> k || ptl::sweep_first_group(a) != k || ptl::sweep_clear_group(a, k) != 0u) fail("hit word of one group", (int)groups);
            if (ptl::sweep_clear_group(~0u, k) != ~(0x80000000u >> k)) fail("clear leaves the other groups", (int)groups);
        }
}

}  // namespace

int main() {
    random_layouts();
    fixed_shapes();
    fit_predicate();
    staged_record();
    hit_word_helpers();
    if (errors) {
        std::fprintf(stderr, "%llu checks failed\n", (unsigned long long)errors);
        return 1;
    }
    std::puts("sweep_layout_check: ok");
    return 0;
}
