// The group table and the candidate mask of the leaf sweep (csrc/pt_leaf_sweep.h).  Checks:
//   - random trees over 1, 2, 31, 32, 33, 63 and 64 primitives whose leaf boxes are drawn from a small pool (so that groups
//     of every size occur): every primitive is in exactly one group, the members of a group have the same box bit for bit and
//     no two groups do, every offset lies inside the node table and names the box of a member, on the left or right half of
//     its parent's record;
//   - all primitives in one group (every box equal) and no two boxes equal (as many groups as primitives, 64 included);
//   - +0 and -0 are different boxes; a table of 65 primitives, a leaf named twice, a leaf missing, a reference out of range
//     and a scene without a node are refused;
//   - take-lowest-and-clear over every single bit, over the full mask (0, 1, .., 63 in order, then empty) and over random masks;
//   - leaf_sweep_on at its bounds.
// Stand-alone; built with -fsanitize=address,undefined by tests/test_leaf_sweep_host.py.  Exit code 0 = all held.
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <random>
#include <vector>

#include "pt_leaf_sweep.h"

namespace {

using ptl::DNode;
using ptl::SweepGroup;

uint64_t errors = 0;
void fail(const char* what, int n = -1) {
    if (errors++ < 10) std::fprintf(stderr, "FAIL: %s (n = %d)\n", what, n);
}

struct Box { float v[6]; };

// A random binary tree over primitives 0 .. n-1 in inner-only form: node k holds its two children's boxes and references.
// Inner boxes are left zero: the builder reads leaf halves only.
std::vector<DNode> random_tree(int n, const std::vector<Box>& box, std::mt19937& rng) {
    std::vector<DNode> nodes;
    if (n < 2) return nodes;
    nodes.resize((size_t)n - 1);
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

void check_table(const std::vector<DNode>& nodes, int n, const std::vector<Box>& box, uint32_t stride, int want_groups) {
    SweepGroup g[ptl::kSweepMaxPrims];
    const int count = ptl::build_sweep_groups(nodes.data(), (int)nodes.size(), n, stride, g);
    if (count < 1 || count > n) { fail("group count out of range", n); return; }
    if (want_groups >= 0 && count != want_groups) fail("group count", n);
    uint64_t seen = 0;
    for (int k = 0; k < count; k++) {
        const uint64_t m = ptl::sweep_group_mask(g[k]);
        if (m == 0) fail("empty group", n);
        if (seen & m) fail("a primitive in two groups", n);
        seen |= m;
        // the offset: inside the table, a left or right half, of a record whose child on that side is a member
        const uint32_t node = g[k].box_off / stride, rest = g[k].box_off % stride;
        if (node >= nodes.size() || (rest != 0 && rest != ptl::kSweepBoxBytes) || g[k].box_off + ptl::kSweepBoxBytes > nodes.size() * stride) {
            fail("offset outside the table", n);
            continue;
        }
        const int32_t ref = rest ? nodes[node].right : nodes[node].left;
        if (ref >= 0 || !((m >> ~ref) & 1ull)) fail("offset does not name a member's box", n);
        const float* b = rest ? nodes[node].rmin : nodes[node].lmin;
        for (int p = 0; p < n; p++)
            if (((m >> p) & 1ull) != (uint64_t)(std::memcmp(b, box[p].v, sizeof(Box)) == 0)) fail("membership is not box equality", n);
    }
    if (seen != (n == 64 ? ~0ull : (1ull << n) - 1ull)) fail("a primitive in no group", n);
}

void tables() {
    std::mt19937 rng(7);
    const int sizes[] = {2, 31, 32, 33, 63, 64};
    for (int n : sizes) {
        for (int rep = 0; rep < 40; rep++) {
            // pool of distinct boxes; a primitive draws one: groups of mixed sizes
            const int pool = 1 + (int)(rng() % (uint32_t)n);
            std::vector<Box> boxes(pool), box(n);
            for (int k = 0; k < pool; k++)
                for (int c = 0; c < 6; c++) boxes[k].v[c] = (float)k + 0.125f * (float)c;
            for (int p = 0; p < n; p++) box[p] = boxes[rng() % (uint32_t)pool];
            check_table(random_tree(n, box, rng), n, box, rep & 1 ? 80u : 64u, -1);
        }
        std::vector<Box> same(n), distinct(n);
        for (int p = 0; p < n; p++)
            for (int c = 0; c < 6; c++) { same[p].v[c] = 0.5f * (float)c; distinct[p].v[c] = (float)p - (float)c; }
        check_table(random_tree(n, same, rng), n, same, 64u, 1);
        check_table(random_tree(n, distinct, rng), n, distinct, 64u, n);
    }
    // +0 and -0: equal as numbers, different boxes (the test is on bits, like the kernel's operands)
    std::vector<Box> z(2);
    std::memset(z.data(), 0, 2 * sizeof(Box));
    z[1].v[0] = -0.0f;
    check_table(random_tree(2, z, rng), 2, z, 64u, 2);
}

void refusals() {
    std::mt19937 rng(11);
    SweepGroup g[ptl::kSweepMaxPrims];
    std::vector<Box> box(65);
    for (int p = 0; p < 65; p++)
        for (int c = 0; c < 6; c++) box[p].v[c] = (float)(p + c);
    // one primitive: no node, no box to test
    if (ptl::build_sweep_groups(nullptr, 0, 1, 64u, g) != -1) fail("a scene without a node");
    std::vector<DNode> t65 = random_tree(65, box, rng);
    if (ptl::build_sweep_groups(t65.data(), (int)t65.size(), 65, 64u, g) != -1) fail("65 primitives");
    std::vector<DNode> t = random_tree(8, box, rng);
    if (ptl::build_sweep_groups(t.data(), (int)t.size(), 8, 64u, g) != 8) fail("8 distinct boxes");
    if (ptl::build_sweep_groups(t.data(), (int)t.size(), 7, 64u, g) != -1) fail("a reference out of range");
    if (ptl::build_sweep_groups(t.data(), (int)t.size(), 9, 64u, g) != -1) fail("a primitive without a leaf");
    for (auto& nd : t)
        if (nd.left < 0 && nd.right < 0) { nd.right = nd.left; break; }
    if (ptl::build_sweep_groups(t.data(), (int)t.size(), 8, 64u, g) != -1) fail("a primitive named twice");
}

void masks() {
    for (int b = 0; b < 64; b++) {
        const uint64_t m = 1ull << b;
        if (ptl::sweep_lowest(m) != b) fail("lowest of a single bit", b);
        if (ptl::sweep_clear_lowest(m) != 0) fail("clear of a single bit", b);
        // ... and with every higher bit set as well
        const uint64_t up = ~0ull << b;
        if (ptl::sweep_lowest(up) != b) fail("lowest below set bits", b);
        if (ptl::sweep_clear_lowest(up) != (b == 63 ? 0ull : ~0ull << (b + 1))) fail("clear below set bits", b);
    }
    uint64_t m = ~0ull;
    for (int b = 0; b < 64; b++) {
        if (m == 0 || ptl::sweep_lowest(m) != b) fail("full mask: order", b);
        m = ptl::sweep_clear_lowest(m);
    }
    if (m != 0) fail("full mask: not empty after 64 takes");
    std::mt19937_64 rng(3);
    for (int k = 0; k < 20000; k++) {
        uint64_t r = rng() & rng();
        const uint64_t start = r;
        uint64_t taken = 0;
        int last = -1, steps = 0;
        while (r) {
            const int b = ptl::sweep_lowest(r);
            if (b <= last || !((start >> b) & 1ull)) fail("random mask: take");
            last = b;
            taken |= 1ull << b;
            r = ptl::sweep_clear_lowest(r);
            if (++steps > 64) { fail("random mask: does not end"); break; }
        }
        if (taken != start) fail("random mask: bits lost");
    }
}

void predicate() {
    using ptl::leaf_sweep_on;
    static_assert(ptl::kSweepMaxBoxes <= ptl::kSweepMaxPrims, "a group holds at least one primitive");
    static_assert(leaf_sweep_on(true, true, false, 2, 64, ptl::kSweepMaxBoxes), "largest launch admitted");
    static_assert(leaf_sweep_on(true, true, false, 2, 2, 1), "smallest");
    static_assert(!leaf_sweep_on(true, true, false, 2, 65, 32), "65 primitives");
    static_assert(!leaf_sweep_on(true, true, false, 2, 64, ptl::kSweepMaxBoxes + 1), "one group too many");
    static_assert(!leaf_sweep_on(true, true, false, 2, 64, 0), "no table");
    static_assert(!leaf_sweep_on(false, true, false, 2, 38, 25), "LDS stack");
    static_assert(!leaf_sweep_on(true, false, false, 2, 38, 25), "pruned traversal");
    static_assert(!leaf_sweep_on(true, true, true, 2, 38, 25), "counting frames");
    static_assert(!leaf_sweep_on(true, true, false, 1, 38, 25), "one node table");
    volatile int prims = 64, groups = ptl::kSweepMaxBoxes;
    if (!leaf_sweep_on(true, true, false, 2, prims, groups)) fail("predicate at its bounds");
    if (leaf_sweep_on(true, true, false, 2, prims + 1, groups) || leaf_sweep_on(true, true, false, 2, prims, groups + 1)) fail("predicate past its bounds");
    static_assert(sizeof(ptl::SweepTable) == 16 + 16 * ptl::kSweepMaxBoxes, "SweepTable layout");
}

// `leaf_sweep_check FILE`: FILE holds N x 6 floats, the leaf boxes of a scene (min.xyz max.xyz).  Builds the table over a random
// tree of them, checks it like the others and prints the group sizes: "groups G sizes s1 s2 ...".
int scene_groups(const char* path) {
    std::FILE* f = std::fopen(path, "rb");
    if (!f) { std::fprintf(stderr, "cannot open %s\n", path); return 2; }
    std::vector<Box> box;
    Box b;
    while (std::fread(b.v, sizeof(float), 6, f) == 6) box.push_back(b);
    std::fclose(f);
    const int n = (int)box.size();
    if (n < 2 || n > ptl::kSweepMaxPrims) { std::fprintf(stderr, "%d boxes\n", n); return 2; }
    std::mt19937 rng(5);
    const std::vector<DNode> nodes = random_tree(n, box, rng);
    check_table(nodes, n, box, 64u, -1);
    SweepGroup g[ptl::kSweepMaxPrims];
    const int count = ptl::build_sweep_groups(nodes.data(), (int)nodes.size(), n, 64u, g);
    std::printf("groups %d sizes", count);
    for (int k = 0; k < count; k++) std::printf(" %d", __builtin_popcountll(ptl::sweep_group_mask(g[k])));
    std::printf("\n");
    return errors ? 1 : 0;
}

}  // namespace

int main(int argc, char** argv) {
    if (argc > 1) return scene_groups(argv[1]);
    tables();
    refusals();
    masks();
    predicate();
    if (errors) {
        std::fprintf(stderr, "%llu checks failed\n", (unsigned long long)errors);
        return 1;
    }
    std::puts("leaf_sweep_check: ok");
    return 0;
}
