// The register traversal stack of trace_kernel_v2 (csrc/pt_reg_stack.h) against a plain array stack, and the predicate that
// decides which launches take it.  Checks:
//   - random push / pop sequences of depth <= 4 over references in [-127, 126] give what the array stack gives, the word
//     after every operation is the one its contents spell out, and a pop at depth 0 yields the done value;
//   - the empty word yields the done value on every pop, however many, and stays the empty word;
//   - four pushes followed by four pops return the entries in reverse and leave the empty word;
//   - reg_stack_on holds at 127 primitives / 126 nodes / 4 entries and fails at 128 primitives, at 127 nodes, at 5 entries,
//     and off the residency, schedule and tree it is compiled for.
// Stand-alone; built with -fsanitize=address,undefined by tests/test_reg_stack_host.py.  Exit code 0 = all held.
#include <cstdint>
#include <cstdio>
#include <random>
#include <vector>

#include "pt_reg_stack.h"

namespace {

uint64_t errors = 0;
void fail(const char* what) {
    if (errors++ < 10) std::fprintf(stderr, "FAIL: %s\n", what);
}

// the word an array stack spells out: top in the low byte, 0x80 above the entries
uint32_t word_of(const std::vector<int32_t>& v) {
    uint32_t w = 0;
    for (int k = 0; k < ptl::kRegStackEntries; k++) {
        const size_t n = v.size();
        const uint32_t byte = (size_t)k < n ? (uint32_t)v[n - 1 - (size_t)k] & 0xffu : 0x80u;
        w |= byte << (8 * k);
    }
    return w;
}

void random_sequences(uint32_t seed) {
    std::mt19937 rng(seed);
    std::uniform_int_distribution<int32_t> ref(-127, 126);
    std::vector<int32_t> model;
    uint32_t w = ptl::kRegStackEmpty;
    for (int step = 0; step < 20000; step++) {
        const bool push = model.size() < (size_t)ptl::kRegStackEntries && (rng() & 1u);
        if (push) {
            const int32_t r = ref(rng);
            model.push_back(r);
            w = ptl::reg_stack_push(w, r);
        } else {
            const int32_t got = ptl::reg_stack_top(w);
            w = ptl::reg_stack_drop(w);
            if (model.empty()) {
                if (got != ptl::kRegStackDone) fail("pop at depth 0 is not the done value");
            } else {
                if (got != model.back()) fail("pop differs from the array stack");
                model.pop_back();
            }
        }
        if (w != word_of(model)) fail("word differs from its contents");
    }
}

void empty_pops() {
    uint32_t w = ptl::kRegStackEmpty;
    if (ptl::kRegStackEmpty != 0x80808080u || ptl::kRegStackDone != -128) fail("constants");
    for (int k = 0; k < 100; k++) {
        if (ptl::reg_stack_top(w) != ptl::kRegStackDone) fail("empty word: top is not the done value");
        w = ptl::reg_stack_drop(w);
        if (w != ptl::kRegStackEmpty) fail("empty word changed by a pop");
    }
}

void four_in_four_out() {
    const int32_t sets[][4] = {{-127, 126, 0, -1}, {125, -127, -127, 125}, {0, 0, 0, 0}, {-1, -2, -3, -4}, {126, 126, 126, 126}};
    for (const auto& e : sets) {
        uint32_t w = ptl::kRegStackEmpty;
        for (int k = 0; k < 4; k++) w = ptl::reg_stack_push(w, e[k]);
        for (int k = 3; k >= 0; k--) {
            if (ptl::reg_stack_top(w) != e[k]) fail("four pushes: entries do not come back in reverse");
            w = ptl::reg_stack_drop(w);
        }
        if (w != ptl::kRegStackEmpty) fail("four pushes, four pops: not the empty word");
        if (ptl::reg_stack_top(w) != ptl::kRegStackDone) fail("four pushes, four pops: next pop is not the done value");
    }
}

void predicate() {
    using ptl::reg_stack_on;
    static_assert(reg_stack_on(1, 40, 162, true, 4, 126, 127), "largest scene admitted");
    static_assert(reg_stack_on(2, 40, 162, true, 4, 126, 127), "largest scene admitted, octant tables");
    static_assert(reg_stack_on(2, 40, 162, true, 1, 1, 2), "small scene");
    static_assert(!reg_stack_on(2, 40, 162, true, 4, 126, 128), "128 primitives: ~127 is the done value");
    static_assert(!reg_stack_on(2, 40, 162, true, 4, 127, 127), "127 nodes");
    static_assert(!reg_stack_on(2, 40, 162, true, 5, 126, 127), "5 entries");
    static_assert(!reg_stack_on(0, 40, 162, true, 4, 126, 127) && !reg_stack_on(3, 40, 162, true, 4, 126, 127), "global memory");
    static_assert(!reg_stack_on(2, 32, 162, true, 4, 126, 127) && !reg_stack_on(2, 40, 4, true, 4, 126, 127), "other schedules");
    static_assert(!reg_stack_on(2, 40, 162, false, 4, 126, 127), "the caller's tree: nearer child first");
    // and at run time, as the host evaluates it
    volatile int prims = 127, nodes = 126, need = 4;
    if (!reg_stack_on(2, 40, 162, true, need, nodes, prims)) fail("predicate: 127 / 126 / 4");
    if (reg_stack_on(2, 40, 162, true, need, nodes, prims + 1)) fail("predicate: 128 primitives");
    if (reg_stack_on(2, 40, 162, true, need, nodes + 1, prims)) fail("predicate: 127 nodes");
    if (reg_stack_on(2, 40, 162, true, need + 1, nodes, prims)) fail("predicate: need 5");
    // every reference such a scene holds survives the byte: nodes 0 .. 125, leaves ~0 .. ~126
    for (int32_t r = ~126; r <= 125; r++) {
        const uint32_t w = ptl::reg_stack_push(ptl::kRegStackEmpty, r);
        if (ptl::reg_stack_top(w) != r || r == ptl::kRegStackDone) fail("reference does not survive the byte");
    }
}

}  // namespace

int main() {
    for (uint32_t seed = 1; seed <= 8; seed++) random_sequences(seed);
    empty_pops();
    four_in_four_out();
    predicate();
    if (errors) {
        std::fprintf(stderr, "%llu checks failed\n", (unsigned long long)errors);
        return 1;
    }
    std::puts("reg_stack_check: ok");
    return 0;
}
