// pt_leaf_sweep.h — the leaf sweep of trace_kernel_v2_sweep (pt_kernels.h): which leaves a ray tests, found without a tree.
//
// On the internal tree exact traversal tests a leaf if and only if the ray hits the leaf's own box (pt_scene_life.hip,
// validate_and_build: the slab test is monotone in the box and every box contains its children's).  The tree is one way to
// find that set; for a scene of a few dozen primitives it is cheaper to test every DISTINCT leaf box once when the segment
// starts, at the width of the scheduler phase.  Leaves whose boxes are equal bit for bit (the two triangles of an axis-aligned
// quad) pass or fail together and share one test: a group.
//
// A group names its box by the byte offset inside a node table: a leaf's box is the left or the right half of its parent's
// record, and every octant table holds it at that offset as (near planes, far planes).  The groups made here are what
// pt_sweep_layout.h lays out for the kernel: one box table per octant, one chained record per primitive.
//
// The header needs no HIP header, so the CPU test tests/native/leaf_sweep_check.cpp runs the same code.
#pragma once
#include <stdint.h>
#include <string.h>

#include "pt_layout.h"

#if defined(__HIPCC__)
#define PT_SWEEP_HD __host__ __device__ inline
#else
#define PT_SWEEP_HD inline
#endif

namespace ptl {

constexpr int kSweepMaxPrims = 64;     // one bit per primitive
// Groups a sweep launch may hold.  By instruction counts (23 VALU per group at ~47 active lanes against cbox's 9.4 inner visits
// of 41 VALU at ~29) the sweep breaks even near 30 groups; measured at 32 groups it is still 25 % ahead of the tree, which
// walks more nodes the more leaves there are (profiles/r11_leaf_sweep.log §7).  More than 32 cannot occur at present: a launch
// sweeps only with octant tables, which exist up to 48 inner nodes.
constexpr int kSweepMaxBoxes = 32;
constexpr uint32_t kSweepBoxBytes = 24;                // near.xyz far.xyz

struct alignas(16) SweepGroup {
    uint32_t box_off;              // byte offset of the box inside one node table (node index * stride + 0 or 24)
    uint32_t mask_lo, mask_hi;     // the primitives whose leaf has this box
    uint32_t pad;
};
static_assert(sizeof(SweepGroup) == 16, "SweepGroup is one 16-byte scalar load");

// The groups of a scene as the handle keeps them (the kernel receives the layout made of them: pt_sweep_layout.h).
struct SweepTable {
    uint32_t count;
    uint32_t pad[3];
    SweepGroup g[kSweepMaxBoxes];
};

PT_SWEEP_HD uint64_t sweep_group_mask(const SweepGroup& g) { return (uint64_t)g.mask_hi << 32 | g.mask_lo; }

// A mask of primitives: take the lowest, clear it.  (m != 0.)
PT_SWEEP_HD int32_t sweep_lowest(uint64_t m) { return (int32_t)__builtin_ctzll(m); }
PT_SWEEP_HD uint64_t sweep_clear_lowest(uint64_t m) { return m & (m - 1ull); }

// Groups the leaves of `nodes` (plain layout, inner nodes only: a child reference < 0 is the leaf of primitive ~ref) by the
// bit pattern of their boxes, in the order the leaves appear in the table.  `out` has room for kSweepMaxPrims groups: a scene
// of 64 primitives may have as many, which is more than a launch admits (leaf_sweep_on).
// Returns the number of groups, or -1 where no table can be made: no node (a scene of one primitive has no box to test),
// more than kSweepMaxPrims primitives, a reference out of range, a primitive that is the leaf of two nodes or of none.
inline int build_sweep_groups(const DNode* nodes, int num_nodes, int num_prims, uint32_t node_stride, SweepGroup* out) {
    if (num_nodes < 1 || num_prims < 1 || num_prims > kSweepMaxPrims) return -1;
    uint64_t seen = 0;
    int count = 0;
    const DNode* first[kSweepMaxPrims];      // the record and side (0 left, 1 right) that hold group k's box
    int first_side[kSweepMaxPrims];
    for (int k = 0; k < num_nodes; k++) {
        for (int side = 0; side < 2; side++) {
            const int32_t ref = side ? nodes[k].right : nodes[k].left;
            if (ref >= 0) continue;
            const int32_t prim = ~ref;
            if (prim < 0 || prim >= num_prims) return -1;
            const uint64_t bit = 1ull << prim;
            if (seen & bit) return -1;
            seen |= bit;
            const float* box = side ? nodes[k].rmin : nodes[k].lmin;       // min[3] then max[3], contiguous
            int g = 0;
            while (g < count && memcmp(box, first_side[g] ? first[g]->rmin : first[g]->lmin, kSweepBoxBytes) != 0) g++;
            if (g == count) {
                first[g] = &nodes[k];
                first_side[g] = side;
                out[g].box_off = (uint32_t)k * node_stride + (uint32_t)side * kSweepBoxBytes;
                out[g].mask_lo = 0; out[g].mask_hi = 0; out[g].pad = 0;
                count++;
            }
            out[g].mask_lo |= (uint32_t)bit;
            out[g].mask_hi |= (uint32_t)(bit >> 32);
        }
    }
    const uint64_t all = num_prims == 64 ? ~0ull : (1ull << num_prims) - 1ull;
    return seen == all ? count : -1;
}

// Which launches sweep: those that keep their traversal stack in a register (reg_stack_on: the default schedule on the
// internal tree of a small LDS-resident scene), tracing exactly, not counting, with the 8 octant tables staged (residency 2:
// the sweep reads near and far planes as stored), on a scene whose primitives fit the mask and whose groups fit the table.
constexpr bool leaf_sweep_on(bool reg_stack, bool exact, bool stats, int res, int num_prims, int groups) {
    return reg_stack && exact && !stats && res == 2 && num_prims <= kSweepMaxPrims && groups >= 1 && groups <= kSweepMaxBoxes;
}

}  // namespace ptl
